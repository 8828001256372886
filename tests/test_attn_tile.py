"""The MFMA tile path of the relation-free attention (gtos_amd/csrc/attn_tile.hip) against fp64 and against the streaming kernels
(rel_attn.hip) it replaces for mode 0 in bf16.  GTOS_ATTN_TILE=0 sends a call back to the streaming kernels; the switch is read per
call, so one process runs both.

The yardstick of the fp64 comparison is the streaming path itself: for every tensor (o, w, dq, dk, dv) the tile path's largest
error against an fp64 restatement of MultiheadAttention on the same bf16-rounded inputs may be at most 1.5 x the streaming path's.
The entry points are called directly (the way ops.RelAttnFn calls them) so that operands can be slices of guarded buffers and a
forward of one path can be paired with the backward of the other."""
import contextlib
import os

import pytest
import torch

from tests_support import Guarded

pytestmark = pytest.mark.gpu

BF = torch.bfloat16


def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


@contextlib.contextmanager
def path(tile):
    old = os.environ.get("GTOS_ATTN_TILE")
    os.environ["GTOS_ATTN_TILE"] = "1" if tile else "0"
    try:
        yield
    finally:
        if old is None:
            del os.environ["GTOS_ATTN_TILE"]
        else:
            os.environ["GTOS_ATTN_TILE"] = old


def u8(t):
    return None if t is None else t.to(torch.uint8).contiguous()


class Operands(object):
    """q, k, v as channel slices of row buffers: q = qbuf[..., q_off:q_off+d] etc."""

    def __init__(self, qbuf, q_off, kbuf, k_off, vbuf, v_off, d, H, key_pad=None, attn_mask=None, scale=None):
        self.qbuf, self.kbuf, self.vbuf, self.offs, self.d, self.H = qbuf, kbuf, vbuf, (q_off, k_off, v_off), d, H
        self.T, self.B, self.S = qbuf.shape[0], qbuf.shape[1], kbuf.shape[0]
        self.key_pad, self.attn_mask = u8(key_pad), u8(attn_mask)
        self.scale = (d // H) ** -0.5 if scale is None else scale

    def q(self):
        return self.qbuf[..., self.offs[0]:self.offs[0] + self.d]

    def k(self):
        return self.kbuf[..., self.offs[1]:self.offs[1] + self.d]

    def v(self):
        return self.vbuf[..., self.offs[2]:self.offs[2] + self.d]


def _p(t, off=0):
    return None if t is None else t.data_ptr() + off * t.element_size()


def attn_fwd(op, p_drop=0.0, seed=0, need_w=False, mode=0, rel=None):
    from gtos_amd._lib import call, dt, stream
    T, S, B, H, d = op.T, op.S, op.B, op.H, op.d
    o = torch.empty(T, B, d, dtype=op.qbuf.dtype, device=op.qbuf.device)
    lse = torch.empty(T, B, H, dtype=torch.float32, device=o.device)
    w = torch.empty(T, S, B, H, dtype=torch.float32, device=o.device) if need_w else None
    call("gtos_rel_attn_fwd", dt(op.qbuf), mode, T, S, B, H, d, _p(op.qbuf, op.offs[0]), op.qbuf.shape[2], _p(op.kbuf, op.offs[1]), op.kbuf.shape[2],
         _p(op.vbuf, op.offs[2]), op.vbuf.shape[2], _p(rel), None, _p(op.key_pad), _p(op.attn_mask), float(op.scale), float(p_drop), seed,
         _p(o), d, _p(lse), _p(w), stream())
    return o, lse, w


def ref64(op, d_o, d_w):
    """fp64 MultiheadAttention on the stored operands: scores, the two masked_fill, softmax over keys (a fully masked row gives zero
    weights), weights @ v; gradients by autograd of <o, d_o> + <w, d_w>."""
    T, S, B, H, d = op.T, op.S, op.B, op.H, op.d
    q, k, v = (t.double().detach().clone().requires_grad_() for t in (op.q(), op.k(), op.v()))
    s = torch.einsum("ibhe,jbhe->ijbh", q.view(T, B, H, -1), k.view(S, B, H, -1)) * op.scale
    dead = torch.zeros(T, S, B, 1, dtype=torch.bool, device=s.device)
    if op.key_pad is not None:
        dead = dead | op.key_pad.bool()[None, :, :, None]
    if op.attn_mask is not None:
        dead = dead | op.attn_mask.bool()[:, :, None, None]
    s = s.masked_fill(dead, float("-inf"))
    mx = s.detach().amax(1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)
    w = e / e.sum(1, keepdim=True).clamp_min(1e-300)
    o = torch.einsum("ijbh,jbhe->ibhe", w, v.view(S, B, H, -1)).reshape(T, B, d)
    loss = (o * d_o.double()).sum()
    if d_w is not None:
        loss = loss + (w * d_w.double()).sum()
    loss.backward()
    return dict(o=o.detach(), w=w.detach(), dq=q.grad, dk=k.grad, dv=v.grad)


def run_path(op, tile, d_o, d_w, p_drop=0.0, seed=0, need_w=True):
    with path(tile):
        o, lse, w = attn_fwd(op, p_drop, seed, need_w or d_w is not None)
        dq, dk, dv = torch.empty_like(op.q()), torch.empty_like(op.k()), torch.empty_like(op.v())
        _bwd_dense(op, o, lse, w, d_o, d_w, dq, dk, dv, p_drop, seed, scratch=not tile)
    torch.cuda.synchronize()
    return dict(o=o, lse=lse, w=w, dq=dq, dk=dk, dv=dv)


def _bwd_dense(op, o, lse, w, d_o, d_w, dq, dk, dv, p_drop, seed, scratch=True):
    """attn_bwd with dense [rows,B,d] gradient outputs although the inputs are slices."""
    from gtos_amd._lib import call, dt, stream
    T, S, B, H, d = op.T, op.S, op.B, op.H, op.d
    pd = torch.empty(T, S, B, H, dtype=torch.float32, device=o.device) if scratch else None
    gs = torch.empty_like(pd) if scratch else None
    call("gtos_rel_attn_bwd", dt(op.qbuf), 0, T, S, B, H, d, _p(op.qbuf, op.offs[0]), op.qbuf.shape[2], _p(op.kbuf, op.offs[1]), op.kbuf.shape[2],
         _p(op.vbuf, op.offs[2]), op.vbuf.shape[2], None, None, None, _p(op.key_pad), _p(op.attn_mask), float(op.scale), float(p_drop), seed,
         _p(o), d, _p(lse), _p(w), _p(d_o), d, _p(d_w), _p(dq), d, _p(dk), d, _p(dv), d, None, 0, _p(pd), _p(gs), stream())


def make_case(T, S, B, H, d, causal, seed=0):
    """Self-attention layout when causal (q, k, v slices of one [T,B,3d] buffer), cross-attention otherwise (q its own buffer, k and v
    slices of a [S,B,2d] buffer).  Ragged key padding; graph 1 fully padded (cross) / query row 7 fully masked (both)."""
    g = torch.Generator().manual_seed(1000 * T + S + seed)
    if causal:
        assert T == S
        qkv = torch.randn(T, B, 3 * d, generator=g).to(dev(), BF)
        mask = torch.triu(torch.ones(T, S), 1).bool()
        mask[7, :] = True
        return Operands(qkv, 0, qkv, d, qkv, 2 * d, d, H, None, mask.to(dev()))
    q = torch.randn(T, B, d, generator=g).to(dev(), BF)
    kv = torch.randn(S, B, 2 * d, generator=g).to(dev(), BF)
    lens = torch.randint(S // 2, S + 1, (B,), generator=g)
    lens[1 % B] = 0 if B > 1 else S                                   # one fully padded graph
    pad = torch.arange(S)[:, None] >= lens[None, :]
    mask = torch.zeros(T, S, dtype=torch.bool)
    mask[7, :] = True                                                 # one fully masked query row
    return Operands(q, 0, kv, 0, kv, d, d, H, pad.to(dev()), mask.to(dev()))


def upstream(op, with_dw, seed=0):
    g = torch.Generator().manual_seed(77 + seed)
    d_o = torch.randn(op.T, op.B, op.d, generator=g).to(dev(), BF)
    d_w = torch.randn(op.T, op.S, op.B, op.H, generator=g).to(dev()) if with_dw else None
    return d_o, d_w


def max_err(got, want):
    return float((got.double() - want).abs().max())


SHAPES = [(50, 50, 64, 8, 512, True), (50, 101, 64, 8, 512, False), (70, 60, 8, 8, 512, False), (100, 301, 4, 8, 512, False),
          (33, 77, 3, 4, 128, False), (40, 70, 16, 2, 256, False)]
# The last shape is not one of the decoder's: it covers hd = 128 (32-key LDS tiles).  The fp32 weights w differ from fp64 by a few
# 1e-8 on both paths (one or two roundings of a score), so the ratio of the two maxima is a noisy statistic on a small tensor:
# the shape has 16 graphs (90 k weights) so that it is no smaller than the smallest of the decoder shapes above (30 k).


@pytest.mark.parametrize("with_dw", [False, True])
@pytest.mark.parametrize("T,S,B,H,d,causal", SHAPES)
def test_tile_against_fp64_no_worse_than_1p5x_streaming(T, S, B, H, d, causal, with_dw):
    """MEASURED lines: the two paths' largest errors against fp64 per tensor.  with_dw: the weights are returned and carry a gradient."""
    op = make_case(T, S, B, H, d, causal)
    d_o, d_w = upstream(op, with_dw)
    ref = ref64(op, d_o, d_w)
    tile, strm = run_path(op, True, d_o, d_w), run_path(op, False, d_o, d_w)
    bad = []
    for name in ("o", "w", "dq", "dk", "dv"):
        assert bool(torch.isfinite(tile[name].float()).all()), name
        et, es = max_err(tile[name], ref[name]), max_err(strm[name], ref[name])
        print("MEASURED attn_tile T%d S%d B%d H%d d%d dw%d %s: tile %.3e, streaming %.3e, ratio %.2f, |ref| max %.3g" % (
            T, S, B, H, d, with_dw, name, et, es, et / max(es, 1e-30), float(ref[name].abs().max())))
        if et > 1.5 * es:
            bad.append((name, et, es))
    # a fully masked row: o = 0, lse = -inf, like the streaming kernels
    assert float(tile["o"][7].float().abs().max()) == 0.0 and bool(torch.isinf(tile["lse"][7]).all())
    assert torch.equal(torch.isinf(tile["lse"]), torch.isinf(strm["lse"]))
    fin = ~torch.isinf(strm["lse"])
    torch.testing.assert_close(tile["lse"][fin], strm["lse"][fin], rtol=1e-5, atol=1e-5)
    assert not bad, "tile error above 1.5 x the streaming path's (tensor, tile, streaming): %s" % bad


def test_dropout_same_mask_same_values_and_bit_identical_reruns():
    op = make_case(50, 101, 64, 8, 512, False)
    with path(True):
        o1, _, w1 = attn_fwd(op, 0.2, 4242, True)
        o2, _, w2 = attn_fwd(op, 0.2, 4242, True)
        _, _, w0 = attn_fwd(op, 0.0, 0, True)
    with path(False):
        os_, _, ws = attn_fwd(op, 0.2, 4242, True)
    torch.cuda.synchronize()
    assert torch.equal(o1, o2) and torch.equal(w1, w2)
    assert torch.equal(w1 == 0, ws == 0)                                # every element, no exclusions
    kept = w1 > 0
    live = w0 > 0
    assert abs(float(kept[live].float().mean()) - 0.8) < 0.01
    torch.testing.assert_close(w1[kept], ws[kept], rtol=1e-4, atol=0.0)
    torch.testing.assert_close(w1[kept], (w0 / 0.8)[kept], rtol=1e-4, atol=1e-6)
    v = op.v().float().reshape(op.S, op.B, op.H, -1)
    # o must be the dropped weights applied to v.  o is a bf16 tensor here (the fp32 test this follows has rtol 1e-3): the relative bound
    # is the unit roundoff of the output format.  bf16 has 8 significand bits (7 stored + the implicit one), so an ulp in [1, 2) is 2^-7
    # and round-to-nearest is off by up to half of it, 2^-8 of a value just above 1 (measured: 3.89e-3 at |o| in [1, 2)).  The same bar
    # holds for the streaming kernels' o
    torch.testing.assert_close(o1.float().view(op.T, op.B, op.H, -1), torch.einsum("ijbh,jbhe->ibhe", w1, v), rtol=2.0 ** -8, atol=1e-3)
    torch.testing.assert_close(os_.float().view(op.T, op.B, op.H, -1), torch.einsum("ijbh,jbhe->ibhe", ws, v), rtol=2.0 ** -8, atol=1e-3)


@pytest.mark.parametrize("T,S,B,H,d,causal", [SHAPES[0], SHAPES[1], SHAPES[4]])
@pytest.mark.parametrize("fwd_tile", [True, False])
def test_mixed_paths_forward_on_one_backward_on_the_other(T, S, B, H, d, causal, fwd_tile):
    """Dropout on: the saved o / lse / w of one path feed the other path's backward; the regenerated mask must be the forward's."""
    op = make_case(T, S, B, H, d, causal, seed=3)
    d_o, d_w = upstream(op, True, seed=3)
    p, seed = 0.2, 991

    def grads(fwd_on_tile, bwd_on_tile):
        with path(fwd_on_tile):
            o, lse, w = attn_fwd(op, p, seed, True)
        dq, dk, dv = torch.empty_like(op.q()), torch.empty_like(op.k()), torch.empty_like(op.v())
        with path(bwd_on_tile):
            _bwd_dense(op, o, lse, w, d_o, d_w, dq, dk, dv, p, seed, scratch=True)
        torch.cuda.synchronize()
        return w, (dq, dk, dv)

    w, base = grads(False, False)                                        # the yardstick: streaming forward and backward
    keep = (w > 0).double() / (1 - p)                                    # the mask both paths draw (checked by the dropout test)
    ref = _ref64_dropout(op, d_o, d_w, keep)
    w2, mixed = grads(fwd_tile, not fwd_tile)
    assert torch.equal(w2 > 0, w > 0)
    for name, got, b0, r in zip(("dq", "dk", "dv"), mixed, base, ref):
        em, eb = max_err(got, r), max_err(b0, r)
        print("MEASURED attn_tile mixed fwd_tile=%d T%d S%d %s: mixed %.3e, streaming %.3e, ratio %.2f" % (fwd_tile, T, S, name, em, eb, em / max(eb, 1e-30)))
        assert em <= 1.5 * eb, (name, em, eb)


def _ref64_dropout(op, d_o, d_w, keep):
    T, S, B, H, d = op.T, op.S, op.B, op.H, op.d
    q, k, v = (t.double().detach().clone().requires_grad_() for t in (op.q(), op.k(), op.v()))
    s = torch.einsum("ibhe,jbhe->ijbh", q.view(T, B, H, -1), k.view(S, B, H, -1)) * op.scale
    dead = torch.zeros(T, S, B, 1, dtype=torch.bool, device=s.device)
    if op.key_pad is not None:
        dead = dead | op.key_pad.bool()[None, :, :, None]
    if op.attn_mask is not None:
        dead = dead | op.attn_mask.bool()[:, :, None, None]
    s = s.masked_fill(dead, float("-inf"))
    mx = s.detach().amax(1, keepdim=True)
    mx = torch.where(torch.isinf(mx), torch.zeros_like(mx), mx)
    e = torch.exp(s - mx)
    w = keep * e / e.sum(1, keepdim=True).clamp_min(1e-300)
    o = torch.einsum("ijbh,jbhe->ibhe", w, v.view(S, B, H, -1)).reshape(T, B, d)
    ((o * d_o.double()).sum() + (w * d_w.double()).sum()).backward()
    return q.grad, k.grad, v.grad


@pytest.mark.parametrize("layout", ["qkv", "q+kv"])
def test_strided_operands_and_guard_bands(layout):
    """q, k, v (and dq, dk, dv) as channel slices of wider row buffers with extra channels, NaN-banded allocations around every output
    (tests_support.Guarded): the kernels write the slices only, and the values match the dense call bit for bit."""
    T, S, B, H, d = (50, 50, 4, 8, 512) if layout == "qkv" else (50, 101, 4, 8, 512)
    g = torch.Generator().manual_seed(5)
    extra = 64                                                            # channels that belong to nobody
    if layout == "qkv":
        C = 3 * d + extra
        qbuf = torch.randn(T, B, C, generator=g).to(dev(), BF)
        kbuf = vbuf = qbuf
        offs = (extra, extra + d, extra + 2 * d)
        mask = torch.triu(torch.ones(T, S), 1).bool().to(dev())
        pad = None
    else:
        qbuf = torch.randn(T, B, d + extra, generator=g).to(dev(), BF)
        kbuf = vbuf = torch.randn(S, B, 2 * d + extra, generator=g).to(dev(), BF)
        offs = (extra, 0, d + extra)
        mask = None
        pad = (torch.arange(S)[:, None] >= torch.tensor([S, S - 30, 5, S - 1])[None, :]).to(dev())
    op = Operands(qbuf, offs[0], kbuf, offs[1], vbuf, offs[2], d, H, pad, mask)
    dense = Operands(op.q().contiguous(), 0, op.k().contiguous(), 0, op.v().contiguous(), 0, d, H, pad, mask)
    d_o, _ = upstream(op, False)
    with path(True):
        from gtos_amd._lib import call, dt, stream
        o_ref, lse_ref, _ = attn_fwd(dense)
        dq_r, dk_r, dv_r = torch.empty_like(dense.qbuf), torch.empty_like(dense.kbuf), torch.empty_like(dense.vbuf)
        _bwd_dense(dense, o_ref, lse_ref, None, d_o, None, dq_r, dk_r, dv_r, 0.0, 0, scratch=False)
        # guarded outputs of the forward
        og = Guarded(T * B, d, BF, dev(), lead=8, trail=8)
        lg = Guarded(T * B, H, torch.float32, dev(), lead=8, trail=8)
        call("gtos_rel_attn_fwd", dt(qbuf), 0, T, S, B, H, d, _p(qbuf, offs[0]), qbuf.shape[2], _p(kbuf, offs[1]), kbuf.shape[2],
             _p(vbuf, offs[2]), vbuf.shape[2], None, None, _p(op.key_pad), _p(op.attn_mask), float(op.scale), 0.0, 0,
             og.view.data_ptr(), d, lg.view.data_ptr(), None, stream())
        og.check("o"); lg.check("lse")
        assert torch.equal(og.view.reshape(T, B, d), o_ref) and torch.equal(lg.view.reshape(T, B, H), lse_ref)
        # gradient buffers with the inputs' geometry: the q / k / v channel slices are outputs, every other channel is band
        Cq, Ckv = qbuf.shape[2], kbuf.shape[2]
        gq = Guarded(T * B, Cq, BF, dev(), lead=8, trail=8)
        gq.regions = []
        if layout == "qkv":
            views = [gq.carve(gq.base + off, T * B, d, Cq) for off in offs]
            gkv = gq
        else:
            views = [gq.carve(gq.base + offs[0], T * B, d, Cq)]
            gkv = Guarded(S * B, Ckv, BF, dev(), lead=8, trail=8)
            gkv.regions = []
            views += [gkv.carve(gkv.base + off, S * B, d, Ckv) for off in offs[1:]]
        call("gtos_rel_attn_bwd", dt(qbuf), 0, T, S, B, H, d, _p(qbuf, offs[0]), Cq, _p(kbuf, offs[1]), Ckv, _p(vbuf, offs[2]), Ckv,
             None, None, None, _p(op.key_pad), _p(op.attn_mask), float(op.scale), 0.0, 0, _p(o_ref), d, _p(lse_ref), None, _p(d_o), d, None,
             views[0].data_ptr(), Cq, views[1].data_ptr(), Ckv, views[2].data_ptr(), Ckv, None, 0, None, None, stream())
        gq.check("dq buffer"); gkv.check("dk / dv buffer")
        for name, got, want in zip(("dq", "dk", "dv"), views, (dq_r, dk_r, dv_r)):
            assert torch.equal(got, want.reshape(got.shape)), name


def test_fallback_shapes_same_bits_with_the_switch_on_and_off():
    """fp32, the T = 1 decode step, the hd = 512 alignment layer and a mode-1 (dense relation operand rarb) call never reach the tile
    kernels.  The mode-2 (factored operand) call has its own test below."""
    g = torch.Generator().manual_seed(11)
    d, H, B = 512, 8, 8

    def both(fn):
        with path(True):
            a = fn()
        with path(False):
            b = fn()
        torch.cuda.synchronize()
        for x, y in zip(a, b):
            assert (x is None and y is None) or torch.equal(x, y)

    def fwd_bwd(op, need_w=False, d_w=None, **kw):
        def fn():
            o, lse, w = attn_fwd(op, 0.2, 31, need_w, **kw)
            if kw:
                return o, lse, w
            dq, dk, dv = torch.zeros_like(op.q()), torch.zeros_like(op.k()), torch.zeros_like(op.v())
            d_o = torch.ones_like(o)
            _bwd_dense(op, o, lse, w, d_o, d_w, dq, dk, dv, 0.2, 31, scratch=True)
            return o, lse, w, dq, dk, dv
        return fn

    q32, kv32 = torch.randn(50, B, d, generator=g).to(dev()), torch.randn(101, B, 2 * d, generator=g).to(dev())
    both(fwd_bwd(Operands(q32, 0, kv32, 0, kv32, d, d, H)))                                                   # fp32
    q1, kv = torch.randn(1, B, d, generator=g).to(dev(), BF), torch.randn(101, B, 2 * d, generator=g).to(dev(), BF)
    both(fwd_bwd(Operands(q1, 0, kv, 0, kv, d, d, H)))                                                        # T = 1
    q50 = torch.randn(50, B, d, generator=g).to(dev(), BF)
    dw = torch.randn(50, 101, B, 1, generator=g).to(dev())
    both(fwd_bwd(Operands(q50, 0, kv, 0, kv, d, d, 1), need_w=True, d_w=dw))                                  # alignment layer: H = 1, hd = 512
    n = 24
    qkv = torch.randn(n, B, 3 * d, generator=g).to(dev(), BF)
    rarb = (0.3 * torch.randn(n, n, B, 2 * d, generator=g)).to(dev(), BF)
    both(fwd_bwd(Operands(qkv, 0, qkv, d, qkv, 2 * d, d, H), mode=1, rel=rarb))                               # mode 1: dense relation operand


def test_autograd_function_skips_the_scratch_buffers_and_matches_the_raw_call():
    """ops.attention_core (what the decoder calls) on the tile path: same bits as the raw entry points, and the backward allocates no
    [T,S,B,H] hand-over buffers."""
    from gtos_amd import ops
    op = make_case(50, 101, 64, 8, 512, False)
    d_o, _ = upstream(op, False)
    ref = run_path(op, True, d_o, None, need_w=False)
    q, kv = op.qbuf.clone().requires_grad_(), op.kbuf.clone().requires_grad_()
    with path(True):
        o, _ = ops.attention_core(q, kv, (0, 0, 512), 512, 8, op.scale, key_pad=op.key_pad, attn_mask=op.attn_mask)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        o.backward(d_o)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - before
    assert torch.equal(o, ref["o"]) and torch.equal(q.grad, ref["dq"])
    assert torch.equal(kv.grad[..., :512], ref["dk"]) and torch.equal(kv.grad[..., 512:], ref["dv"])
    grads, scratch = (50 * 64 * 512 + 101 * 64 * 1024) * 2, 50 * 101 * 64 * 8 * 4
    assert peak < grads + scratch // 2, "the backward allocated %d bytes: the gradients are %d, one [T,S,B,H] fp32 buffer %d" % (peak, grads, scratch)


def test_fallback_mode2_factored_relation_forward_and_backward_same_bits():
    """Mode 2 (bank projection [R,2d] + idx_q / idx_k) through a bf16 GraphTransformer layer, forward and backward -- gtos_rel_attn_fwd,
    gtos_rel_attn_bwd with d_rel / ld_drel and the pd / gs hand-over, gtos_rel_attn_bwd_bank reading gs -- with the switch on and off:
    output, input gradient and bank gradient bit for bit.  No relation type is frequent enough to take the fp32-atomic (heavy) route,
    so every compared tensor is deterministic."""
    from gtos_amd.graph_transformer import GraphTransformer, set_compute_dtype
    from gtos_amd.ops import FactoredRelation
    n, B, d, H, R = 24, 8, 512, 8, 3000
    g = torch.Generator().manual_seed(21)
    bank, x = 0.5 * torch.randn(R, d, generator=g), torch.randn(n, B, d, generator=g)
    idx = torch.randint(0, R, (n, n, B), generator=g)
    pad = torch.zeros(n, B, dtype=torch.bool)
    pad[n - 3:, B - 1] = True
    wout = torch.randn(n, B, d, generator=g).to(dev())
    torch.manual_seed(4)
    m = GraphTransformer(1, d, 2 * d, H, 0.0).to(dev())
    set_compute_dtype(m, BF)

    def run(tile):
        with path(tile):
            m.zero_grad()
            bank_d, x_d = bank.to(dev()).requires_grad_(), x.to(dev()).requires_grad_()
            out = m(x_d, FactoredRelation(bank_d, idx.to(dev())), self_padding_mask=pad.to(dev()))
            (out.float() * wout).sum().backward()
            from gtos_amd import ops
            ops.join_side()
            torch.cuda.synchronize()
        return out.detach().clone(), x_d.grad.clone(), bank_d.grad.clone()

    on, on2, off = run(True), run(True), run(False)
    for name, a, a2, b in zip(("out", "dx", "dbank"), on, on2, off):
        assert float(a.float().abs().max()) > 0, name
        assert torch.equal(a, a2), name + ": not deterministic run to run, the comparison below would not mean anything"
        assert torch.equal(a, b), name


def test_python_predicate_never_says_tile_where_the_library_refuses():
    """ops._attn_tile_backward decides whether the pd / gs hand-over buffers are allocated; gtosi_attn_tile_covers decides which kernels
    run.  Sweep shapes, head counts, leading dimensions and channel offsets: wherever the Python side says 'tile' the backward must
    accept null pd / gs (it returns -15, raised as an error, when it would need them)."""
    from gtos_amd import ops
    g = torch.Generator().manual_seed(3)
    said_tile = 0
    for T in (1, 8, 16, 17, 50):
        for d, H in ((512, 8), (512, 1), (256, 2), (256, 8), (128, 4), (128, 16), (64, 2), (384, 6), (1024, 8)):
            for extra, q_off in ((0, 0), (8, 8), (16, 8), (24, 16)):
                S, B = 19, 2
                qbuf = torch.randn(T, B, d + extra, generator=g).to(dev(), BF)
                kbuf = torch.randn(S, B, 2 * d + extra, generator=g).to(dev(), BF)
                op = Operands(qbuf, q_off, kbuf, q_off, kbuf, d + q_off, d, H)
                with path(False):
                    o, lse, _ = attn_fwd(op)
                d_o = torch.ones_like(o)
                dqb, dkb = torch.zeros_like(qbuf), torch.zeros_like(kbuf)
                with path(True):
                    py = ops._attn_tile_backward(0, T, d, H, (qbuf.shape[2], kbuf.shape[2], d) + op.offs, (qbuf, kbuf, o, d_o, dqb, dkb))
                    if not py:
                        continue
                    said_tile += 1
                    from gtos_amd._lib import call, dt, stream
                    call("gtos_rel_attn_bwd", dt(qbuf), 0, T, S, B, H, d, _p(qbuf, op.offs[0]), qbuf.shape[2], _p(kbuf, op.offs[1]), kbuf.shape[2],
                         _p(kbuf, op.offs[2]), kbuf.shape[2], None, None, None, None, None, float(op.scale), 0.0, 0, _p(o), d, _p(lse), None, _p(d_o), d, None,
                         _p(dqb, op.offs[0]), dqb.shape[2], _p(dkb, op.offs[1]), dkb.shape[2], _p(dkb, op.offs[2]), dkb.shape[2], None, 0, None, None, stream())
    torch.cuda.synchronize()
    assert said_tile >= 20, said_tile
