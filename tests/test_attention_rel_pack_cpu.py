"""Host-only parts of asr.RelPositionMultiheadAttention: pack_torch's layout,
the table cache's range arithmetic and rel_needed_rows against the reference's
needed_rows.  No device."""
import numpy as np
import pytest
import torch

import attention_rel_reference as atr
from conftest import asr


def test_pack_torch_layout():
    E, H = 24, 3
    m = atr.RelPositionAttention(E, H)
    with torch.no_grad():
        m.pos_bias_u.uniform_(-1, 1)
        m.pos_bias_v.uniform_(-1, 1)
    w_in, b_in, w_pos, bu, bv, w_out, b_out = asr.RelPositionMultiheadAttention.pack_torch(m)
    assert [a.shape for a in (w_in, b_in, w_pos, bu, bv, w_out, b_out)] == [(E, 3 * E), (3 * E,), (E, E), (E,), (E,),
                                                                           (E, E), (E,)]
    x = torch.rand(5, E)
    with torch.no_grad():
        want = torch.cat([m.linear_q(x), m.linear_k(x), m.linear_v(x)], dim=1).numpy()
        assert np.allclose(x.numpy() @ w_in + b_in, want, atol=1e-6)
        assert np.allclose(x.numpy() @ w_pos, m.linear_pos(x).numpy(), atol=1e-6)
    assert np.array_equal(bu.reshape(H, -1), m.pos_bias_u.detach().numpy())
    m.linear_pos = torch.nn.Linear(E, E)                        # a bias on linear_pos is refused
    with pytest.raises(ValueError, match="linear_pos"):
        asr.RelPositionMultiheadAttention.pack_torch(m)


@pytest.mark.parametrize("cached, need, want", [
    (None, (9, -9), (9, -9)),                 # first call
    (None, (5, 2), (5, 0)),                   # always holds distance 0
    ((9, -9), (4, -4), (9, -9)),              # covered: kept (the same object)
    ((9, -9), (12, -3), (12, -9)),            # one side grows: the union
    ((47, -15), (47, -15), (47, -15)),
])
def test_table_range(cached, need, want):
    got = asr.RelPositionMultiheadAttention.table_range(cached, *need)
    assert got == want and (got is cached or got != cached)


@pytest.mark.parametrize("args", [(70, 70), (16, 48, 16, 2, 0, 32, 0), (43, 83, 1, 10, 3, 77, 67), (5, 9, 4, -1, 1, 0, 3)])
def test_rel_needed_rows_is_the_references(args):
    assert asr.rel_needed_rows(*args) == atr.needed_rows(*args)
