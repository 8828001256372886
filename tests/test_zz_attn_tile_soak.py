"""Repeated-run bitwise soak of the MFMA tile attention kernels (attn_tile.hip) at the sizes the C2 step launches them, beside the
HBM hammer stream of test_zz_race_soak.py: the kernels refill their LDS tiles (K / V / Q / dO panels, the dead-pair bytes, the row
statistics) once per streamed tile between two barriers, and the key-major and query-major workgroups of the backward share one
launch.  Every output of every repeated launch must equal the first launch bit for bit."""
import pytest
import torch

from test_attn_tile import _bwd_dense, attn_fwd, make_case, path, upstream
from test_zz_race_soak import soak

pytestmark = pytest.mark.gpu

C2 = {"self": (50, 50, 64, 8, 512, True), "cross": (50, 101, 64, 8, 512, False), "C3 cross": (70, 60, 64, 8, 512, False)}


@pytest.mark.parametrize("kind", sorted(C2))
def test_soak_attn_tile_forward(kind):
    op = make_case(*C2[kind])
    T, S, B, H, d = op.T, op.S, op.B, op.H, op.d
    from gtos_amd._lib import call, dt, stream
    o = torch.zeros(T, B, d, dtype=torch.bfloat16, device=op.qbuf.device)
    lse = torch.zeros(T, B, H, dtype=torch.float32, device=o.device)
    w = torch.zeros(T, S, B, H, dtype=torch.float32, device=o.device)

    def launch():
        call("gtos_rel_attn_fwd", dt(op.qbuf), 0, T, S, B, H, d, op.q().data_ptr(), op.qbuf.shape[2], op.k().data_ptr(), op.kbuf.shape[2],
             op.v().data_ptr(), op.vbuf.shape[2], None, None, op.key_pad.data_ptr() if op.key_pad is not None else None,
             op.attn_mask.data_ptr() if op.attn_mask is not None else None, float(op.scale), 0.2, 1357, o.data_ptr(), d, lse.data_ptr(),
             w.data_ptr(), stream())

    def no_inf():                                              # soak() wants finite outputs: the fully masked rows' lse is -inf by contract
        lse.nan_to_num_(neginf=-1e30)
    with path(True):
        launch()
        torch.cuda.synchronize()
        assert bool(torch.isinf(lse).any())
        soak("attn tile fwd " + kind, lambda: (launch(), no_inf()), [o, lse, w])


@pytest.mark.parametrize("kind", sorted(C2))
def test_soak_attn_tile_backward(kind):
    op = make_case(*C2[kind])
    d_o, d_w = upstream(op, True)
    with path(True):
        o, lse, w = attn_fwd(op, 0.2, 1357, True)
        dq, dk, dv = torch.zeros_like(op.q()), torch.zeros_like(op.k()), torch.zeros_like(op.v())
        soak("attn tile bwd " + kind, lambda: _bwd_dense(op, o, lse, w, d_o, d_w, dq, dk, dv, 0.2, 1357, scratch=False), [dq, dk, dv])
