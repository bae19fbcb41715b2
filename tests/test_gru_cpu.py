"""CPU checks of the GRU entry points (asr_gru_workspace_bytes, asr_gru_fwd,
asr_gru_recur_fwd): exported, sized and argument-checked before any HIP call
(no GPU here; the fake device pointers are never dereferenced on the host)."""
import re
import subprocess

import pytest

from conftest import asr

NAMES = ["asr_gru_workspace_bytes", "asr_gru_fwd", "asr_gru_recur_fwd"]
FAKE = 0x10000   # a non-NULL, 16-byte aligned "device pointer"


def test_symbols_in_mirror_and_library():
    for n in NAMES:
        assert n in asr.EXPORTS, n
        assert hasattr(asr.lib(), n), n
    out = subprocess.run(["nm", "-D", "--defined-only", str(asr.LIB_PATH)], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (asr_[a-z0-9_]+)$", out, flags=re.M))
    assert set(NAMES) <= exported


@pytest.mark.parametrize("T,B,H", [(1, 1, 16), (7, 5, 16), (12, 50, 128), (5, 3, 144), (3, 16, 1024),
                                   (200, 1024, 2048)])
def test_workspace_bytes(T, B, H):
    n = asr.lib().asr_gru_workspace_bytes(T, B, H)
    assert n >= T * B * 3 * H * 4
    assert n % 16 == 0


def test_workspace_bytes_invalid_shape():
    L = asr.lib()
    assert L.asr_gru_workspace_bytes(4, 4, 0) == 0
    assert L.asr_gru_workspace_bytes(4, 4, 20) == 0
    assert L.asr_gru_workspace_bytes(4, 4, 2064) == 0
    assert L.asr_gru_workspace_bytes(0, 4, 16) == 0


def fwd(T, B, inp, H, ldh=None, null=None):
    """asr_gru_fwd with fake pointers; null: index of a pointer argument passed as NULL."""
    p = [FAKE] * 10   # x, h0, W_ih, W_hh, b_ih, b_hh, hiddens, hT, lengths, work
    if null is not None:
        p[null] = None
    return asr.lib().asr_gru_fwd(*p[:7], H if ldh is None else ldh, *p[7:], T, B, inp, H, 0, None)


def recur(T, B, H, ldh=None, null=None):
    p = [FAKE] * 8    # P, h0, W_hh, b_ih, b_hh, hiddens, hT, lengths
    if null is not None:
        p[null] = None
    return asr.lib().asr_gru_recur_fwd(*p[:6], H if ldh is None else ldh, *p[6:], T, B, H, 0, None)


@pytest.mark.parametrize("null", [0, 2, 3, 4, 5, 6, 9], ids=["x", "W_ih", "W_hh", "b_ih", "b_hh", "hiddens", "work"])
def test_err_arg_null_pointer_fwd(null):
    assert fwd(4, 4, 8, 16, null=null) == asr.ASR_ERR_ARG


@pytest.mark.parametrize("null", [0, 2, 3, 4, 5], ids=["P", "W_hh", "b_ih", "b_hh", "hiddens"])
def test_err_arg_null_pointer_recur(null):
    assert recur(4, 4, 16, null=null) == asr.ASR_ERR_ARG
    assert recur(4, 4, 256, null=null) == asr.ASR_ERR_ARG


def test_err_arg_sizes():
    assert fwd(0, 4, 8, 16) == asr.ASR_ERR_ARG
    assert fwd(4, 0, 8, 16) == asr.ASR_ERR_ARG
    assert fwd(4, 4, 0, 16) == asr.ASR_ERR_ARG
    assert fwd(4, 4, 8, 0) == asr.ASR_ERR_ARG
    assert fwd(4, 4, 8, 16, ldh=15) == asr.ASR_ERR_ARG
    assert recur(0, 4, 16) == asr.ASR_ERR_ARG
    assert recur(4, 0, 16) == asr.ASR_ERR_ARG
    assert recur(4, 4, 16, ldh=15) == asr.ASR_ERR_ARG
    assert recur(4, 4, 256, ldh=255) == asr.ASR_ERR_ARG


@pytest.mark.parametrize("H", [20, 2064])
def test_err_unsupported(H):
    assert fwd(4, 4, 8, H) == asr.ASR_ERR_UNSUPPORTED
    assert recur(4, 4, H) == asr.ASR_ERR_UNSUPPORTED


def test_err_unsupported_frame_beyond_one_buffer_resource():
    # B * 3H * 4 bytes of one frame's input projection past one buffer resource
    B, H = 1 << 18, 2048
    assert B * 3 * H * 4 > 0x7ff00000
    assert recur(1, B, H) == asr.ASR_ERR_UNSUPPORTED
    assert fwd(1, B, 8, H) == asr.ASR_ERR_UNSUPPORTED
    # and in the resident form: the smallest B at H = 128 whose frame is past it
    B = 0x7ff00000 // (3 * 128 * 4) + 1
    assert recur(1, B, 128) == asr.ASR_ERR_UNSUPPORTED


def test_err_unsupported_step_form_alignment():
    # the step form reads h rows with 16-byte loads; the resident form does not
    assert recur(4, 4, 256, ldh=258) == asr.ASR_ERR_UNSUPPORTED
    assert fwd(4, 4, 8, 256, ldh=258) == asr.ASR_ERR_UNSUPPORTED
    p = [FAKE] * 8
    p[5] = FAKE + 4   # hiddens not 16-byte aligned
    assert asr.lib().asr_gru_recur_fwd(*p[:6], 256, *p[6:], 4, 4, 256, 0, None) == asr.ASR_ERR_UNSUPPORTED
    p = [FAKE] * 8
    p[1] = FAKE + 8   # h0 not 16-byte aligned
    assert asr.lib().asr_gru_recur_fwd(*p[:6], 256, *p[6:], 4, 4, 256, 0, None) == asr.ASR_ERR_UNSUPPORTED


def state_overlap(H, h0, hT, B=4):
    """asr_gru_recur_fwd and asr_gru_fwd on an otherwise valid call with the given d_h0 / d_hT."""
    p, L = FAKE, asr.lib()
    return (L.asr_gru_recur_fwd(p, h0, p, p, p, p, H, hT, p, 4, B, H, 0, None),
            L.asr_gru_fwd(p, h0, p, p, p, p, p, H, hT, p, p, 4, B, 8, H, 0, None))


def test_err_arg_hT_over_h0():
    """d_hT over d_h0 ([B*H] floats each): the step form (H > 128) reads whole h0 rows while it
    stores hT, so even d_hT == d_h0 is refused there; a partial overlap is refused for every H."""
    B = 4
    assert state_overlap(256, FAKE, FAKE) == (asr.ASR_ERR_ARG,) * 2             # equal pointers, step form
    for H in (16, 256):
        n = B * H * 4
        for h0, hT in ((FAKE, FAKE + 16), (FAKE + 16, FAKE), (FAKE, FAKE + n - 16), (FAKE + n - 16, FAKE)):
            assert state_overlap(H, h0, hT, B) == (asr.ASR_ERR_ARG,) * 2, (H, h0, hT)
    # the H limits answer first: an unsupported shape stays ASR_ERR_UNSUPPORTED.  (d_hT == d_h0 at
    # H <= 128 is legal and cannot be shown with fake pointers, since the call would launch:
    # test_gated_rnn_edges_gpu.py's in-place tests run it at H = 48.)
    assert state_overlap(2064, FAKE, FAKE) == (asr.ASR_ERR_UNSUPPORTED,) * 2
    assert state_overlap(24, FAKE, FAKE) == (asr.ASR_ERR_UNSUPPORTED,) * 2
