"""CPU checks of the transducer decode (asr_rnnt_*): the fp64 host twin
asr_rnnt_greedy_host against tests/rnnt_reference.py, every refusal, the
from_torch layout, truncation at max_out and chunked decodes with the state
carried.  No GPU is needed or used."""
import numpy as np
import pytest
import torch

import rnnt_cases as rc
from conftest import asr
from rnnt_reference import Reference

REL = 1e-9   # the project's oracle bound: both sides are fp64 and differ in summation order only


def close(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= REL * (1.0 + np.abs(b))))


@pytest.mark.parametrize("case", rc.SMALL_CASES, ids=lambda c: c.name)
def test_twin_matches_reference(case):
    w, enc, ref = rc.reference(case)
    rc.check_conditions(case, ref)
    dec = rc.make_decoder(asr, case, w)
    res, state, cnt, gap = dec.decode_host(enc, rc.lengths_of(case), gaps=True)
    assert cnt.tolist() == ref["count"]
    for b, (tok, ts, lp, total) in enumerate(res):
        assert tok == ref["tokens"][b] and ts == ref["timesteps"][b]
        assert close(lp, ref["logps"][b]), (b, lp, ref["logps"][b])
        assert close(total, ref["total"][b])
        assert (np.isinf(gap[b]) and np.isinf(ref["gap"][b])) or close(gap[b], ref["gap"][b])
    assert close(state, ref["state"])
    dec.close()


def test_from_torch_layout_round_trip():
    torch.manual_seed(5)
    V, E, D, Hp, J, L = 11, 6, 16, 32, 16, 2
    emb, lstm = torch.nn.Embedding(V, D), torch.nn.LSTM(D, Hp, num_layers=L)
    enc_proj, pred_proj, out_proj = torch.nn.Linear(E, J), torch.nn.Linear(Hp, J), torch.nn.Linear(J, V)
    with torch.no_grad():
        out_proj.weight.mul_(6.0)
        out_proj.bias[V - 1] = 0.5
    dec = asr.TransducerDecoder.from_torch(emb, lstm, enc_proj, pred_proj, out_proj, blank=V - 1, activation="tanh",
                                           max_symbols=2)
    info = dec.info()
    assert (info["V"], info["blank"], info["E"], info["D"], info["Hp"], info["L"], info["J"], info["act"],
            info["max_symbols"]) == (V, V - 1, E, D, Hp, L, J, asr.RNNT_ACT_TANH, 2)
    assert not info["uploaded"]
    # [in][out]: the transposes of torch's [out][in]
    assert np.array_equal(dec.weights["emb"], emb.weight.detach().numpy())
    for l in range(L):
        assert np.array_equal(dec.weights["w_ih", l], getattr(lstm, f"weight_ih_l{l}").detach().numpy().T)
        assert np.array_equal(dec.weights["w_hh", l], getattr(lstm, f"weight_hh_l{l}").detach().numpy().T)
        assert np.array_equal(dec.weights["b_ih", l], getattr(lstm, f"bias_ih_l{l}").detach().numpy())
    assert np.array_equal(dec.weights["w_out"], out_proj.weight.detach().numpy().T)
    assert np.array_equal(dec.weights["w_pred"], pred_proj.weight.detach().numpy().T)
    assert np.array_equal(dec.weights["w_enc"], enc_proj.weight.detach().numpy().T)
    # and the modules themselves, run by torch, walk as the twin does
    T, B = 6, 2
    enc = torch.rand(T, B, E) * 2 - 1
    res, _state, cnt = dec.decode_host(enc.numpy())
    with torch.no_grad():
        for b in range(B):
            hc = (torch.zeros(L, 1, Hp), torch.zeros(L, 1, Hp))
            out, hc = lstm(emb(torch.tensor([[V - 1]])), hc)
            toks, tss = [], []
            for t in range(T):
                for _ in range(2):
                    z = torch.tanh(enc_proj(enc[t, b]) + pred_proj(out[0, 0]))
                    k = int(torch.argmax(out_proj(z)))
                    if k == V - 1:
                        break
                    toks.append(k), tss.append(t)
                    out, hc = lstm(emb(torch.tensor([[k]])), hc)
            assert (res[b][0], res[b][1]) == (toks, tss)
    assert int(cnt.sum()) > 0
    with pytest.raises(ValueError):
        asr.TransducerDecoder.from_torch(emb, torch.nn.LSTM(D, Hp, bidirectional=True), enc_proj, pred_proj, out_proj, 0)
    dec.close()


def test_truncation_at_max_out():
    case = rc.SMALL_CASES[6]   # s2-b0-m3
    w, enc, ref = rc.reference(case)
    dec = rc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case)
    full, state, cnt = dec.decode_host(enc, ln)
    assert max(ref["count"]) > 2
    for max_out in (0, 2):
        res, st, c = dec.decode_host(enc, ln, max_out=max_out)
        assert c.tolist() == ref["count"] and any(x > max_out for x in c)   # the count goes on
        for b in range(len(res)):
            n = min(max_out, ref["count"][b])
            assert res[b][0] == ref["tokens"][b][:n] and res[b][1] == ref["timesteps"][b][:n]
            assert np.array_equal(res[b][2], full[b][2][:n])
            assert res[b][3] == full[b][3]
        assert np.array_equal(st, state)    # the walk and the state went on
    # the reference truncates the same way
    tr = Reference(w, case.blank, case.act, case.max_symbols).decode(enc, case.lengths, max_out=2)
    assert tr["count"] == ref["count"] and tr["tokens"] == [t[:2] for t in ref["tokens"]]
    dec.close()


@pytest.mark.parametrize("case", [rc.SMALL_CASES[7], rc.SMALL_CASES[10]], ids=lambda c: c.name)
def test_chunked_decode_equals_whole(case):
    w, enc, ref = rc.reference(case)
    dec = rc.make_decoder(asr, case, w)
    ln = rc.lengths_of(case)
    T = enc.shape[0]
    whole, wstate, wcnt = dec.decode_host(enc, ln)
    cuts = [0, T // 3, T // 3 + 2, T]
    state, parts = None, [([], [], []) for _ in range(enc.shape[1])]
    for t0, t1 in zip(cuts, cuts[1:]):
        res, state, _c = dec.decode_host(enc[t0:t1], np.clip(ln - t0, 0, t1 - t0), state=state)
        for b, (tok, ts, lp, _total) in enumerate(res):
            parts[b][0].extend(tok), parts[b][1].extend(t + t0 for t in ts), parts[b][2].extend(lp.tolist())
    for b in range(enc.shape[1]):
        assert parts[b][0] == whole[b][0] == ref["tokens"][b]
        assert parts[b][1] == whole[b][1]
        assert parts[b][2] == whole[b][2].tolist()      # bit for bit: the twin's state is fp64
    assert np.array_equal(state, wstate)
    dec.close()


def test_refusals():
    case = rc.SMALL_CASES[4]
    w = rc.make_model(case)[0]
    T, B, E, D, Hp, J, V, L = case.shape

    def status(**kw):
        d = dict(V=V, blank=0, E=E, D=D, Hp=Hp, L=L, J=J, act="relu", max_symbols=2)
        d.update(kw)
        ww = dict(w)
        # the arrays must fit the descriptor for the Python side; the C side is what refuses
        ww["emb"] = np.zeros((d["V"], d["D"]), np.float32)
        ww["w_ih"] = [np.zeros((d["Hp"] if l else d["D"], 4 * d["Hp"]), np.float32) for l in range(d["L"])]
        ww["w_hh"] = [np.zeros((d["Hp"], 4 * d["Hp"]), np.float32) for l in range(d["L"])]
        ww["b_ih"] = ww["b_hh"] = [np.zeros(4 * d["Hp"], np.float32) for l in range(d["L"])]
        ww["w_enc"], ww["b_enc"] = np.zeros((d["E"], d["J"]), np.float32), np.zeros(d["J"], np.float32)
        ww["w_pred"], ww["b_pred"] = np.zeros((d["Hp"], d["J"]), np.float32), np.zeros(d["J"], np.float32)
        ww["w_out"], ww["b_out"] = np.zeros((d["J"], d["V"]), np.float32), np.zeros(d["V"], np.float32)
        try:
            asr.TransducerDecoder(asr.rnnt_desc(**d), ww).close()
        except asr.AsrError as e:
            return e.status
        return asr.ASR_OK

    assert status() == asr.ASR_OK
    assert status(V=1) == asr.ASR_ERR_ARG
    assert status(blank=-1) == asr.ASR_ERR_ARG and status(blank=V) == asr.ASR_ERR_ARG
    assert status(max_symbols=0) == asr.ASR_ERR_ARG      # no unbounded mode
    assert status(act=2) == asr.ASR_ERR_ARG
    assert status(L=3) == asr.ASR_ERR_UNSUPPORTED
    assert status(D=24) == asr.ASR_ERR_UNSUPPORTED and status(Hp=40) == asr.ASR_ERR_UNSUPPORTED
    assert status(J=8) == asr.ASR_ERR_UNSUPPORTED
    # the limit written in the header: 64 * (2 L (Hp + 4) + (J + 4)) + 4096 <= 160 KiB
    assert status(D=16, Hp=640, J=640, L=1) == asr.ASR_OK       # the required upper range
    assert status(D=16, Hp=320, J=320, L=2) == asr.ASR_OK
    assert status(D=16, Hp=816, J=816, L=1) == asr.ASR_OK
    assert status(D=16, Hp=832, J=832, L=1) == asr.ASR_ERR_UNSUPPORTED
    assert status(D=16, Hp=640, J=640, L=2) == asr.ASR_ERR_UNSUPPORTED
    lib = asr.lib()
    assert lib.asr_rnnt_create(None, None, None) == asr.ASR_ERR_ARG
    assert lib.asr_rnnt_upload(None) == asr.ASR_ERR_ARG
    assert lib.asr_rnnt_destroy(None) == asr.ASR_ERR_ARG
    assert lib.asr_rnnt_get_info(None, None) == asr.ASR_ERR_ARG
    assert lib.asr_rnnt_workspace_bytes(None, 1, 1) == 0

    dec = rc.make_decoder(asr, case, w)
    assert dec.workspace_bytes(0, 1) == 0 and dec.workspace_bytes(1, 0) == 0
    assert dec.workspace_bytes(3, 17) == 4 * (3 * 17 * J + 2 * 16 * (L * Hp + J))
    enc = np.zeros((2, 2, E), np.float32)
    i32, f64 = np.zeros(8, np.int32), np.zeros(8, np.float64)
    p = asr._ptr
    good = [dec.h, p(enc), None, 2, 2, 4, None, None, p(i32), p(i32), p(f64), p(i32), p(f64)]

    def both(i, value, want):
        a = list(good)
        a[i] = value
        assert lib.asr_rnnt_greedy_host(*a, None) == want, (i, value)
        assert lib.asr_rnnt_greedy(*a, p(f64), None) == want, (i, value)    # refused before any HIP call

    for i in (0, 1, 8, 9, 10, 11, 12):
        both(i, None, asr.ASR_ERR_ARG)
    both(3, 0, asr.ASR_ERR_ARG)
    both(4, 0, asr.ASR_ERR_ARG)
    both(5, -1, asr.ASR_ERR_ARG)
    both(3, 1 << 30, asr.ASR_ERR_UNSUPPORTED)       # T * (max_symbols + 1) and T * B
    assert lib.asr_rnnt_greedy(*good, None, None) == asr.ASR_ERR_ARG          # no workspace
    assert lib.asr_rnnt_greedy(*good, p(f64), None) == asr.ASR_ERR_STATE      # not uploaded
    assert lib.asr_rnnt_greedy_host(*good, None) == asr.ASR_OK
    with pytest.raises(ValueError):
        dec.decode_host(np.zeros((2, 2, E + 1), np.float32))
    dec.close()
