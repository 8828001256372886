"""Label smoothing of the generate/copy loss (TokenGenerator(..., label_smoothing=eps), ops.copy_nll(..., label_smoothing=eps),
csrc/copy_ls.hip, csrc/copy_ls_kernels.h).

The loss of row r = (t, b) is the reference's label_smoothed_nll_loss on TokenGenerator's ll row:
    C = max(V, 1 + max(cp_seq)),  p_k = g softmax(x)_k [k < V] + c sum_{s: cp_seq[s,b] == k} a_s,  ll_k = log(p_k + 1e-12)
    loss_r = 0 at padded targets, else (1 - eps) (-ll_y) + (eps / C) (-sum_{k<C} ll_k).
CPU: the row header compiled with g++ against a float64 numpy statement of that loss and its gradient, the argument checks, and the
dry-run launch plans (eps > 0 takes the new entry points; eps = 0.0 given explicitly takes exactly today's).  GPU: the kernels against
float64 torch autograd inside NaN guard bands, eps = 0 bitwise at the op and to rounding at the model, the whole model against the
oracle with the loss formed from its differentiable ll row, and a captured graph replayed on a batch with another C."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver


DRIVER = r"""
#include "copy_ls_kernels.h"
using namespace gtos_ls;
extern "C" long long ws_words(int B, int S, int V) { return (long long)Layout(B, S, V).total; }
extern "C" void build(const int64_t* cp, int B, int S, int V, int* ws) { build_serial(cp, B, S, V, ws); }
extern "C" void row(const float* x, int V, float d0, float d1, const float* a, int S, int B, int b, int64_t y, int64_t pad, float eps,
                    const int* ws, float u, float* loss, float* sums, float* dx, float* dd, float* da) {
    row_serial(x, V, d0, d1, a, S, B, b, y, pad, eps, ws, u, loss, sums, dx, dd, da);
}
"""

EPS_SET = (0.0, 0.1, 0.5, 1.0)
PAD = 0


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = compile_host_driver(tmp_path_factory, "ls_host", DRIVER)
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    so.ws_words.argtypes, so.ws_words.restype = [I, I, I], ctypes.c_longlong
    so.build.argtypes, so.build.restype = [P, I, I, I, P], None
    so.row.argtypes = [P, I, F, F, P, I, I, I, L, L, F, P, F, P, P, P, P, P]
    so.row.restype = None
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ the loss, stated in float64
def reference_rows(x, div, a, cp, y, eps, pad=PAD):
    """x [R,V], div [R,2], a [R,S], cp [S,B] (row r belongs to graph r % B), y [R] -> loss [R], dx [R,V], ddiv [R,2], da [R,S]:
    the dense row of section 1 and its gradient (w_k = dloss/dp_k), in float64."""
    x, div, a = (np.asarray(v, np.float64) for v in (x, div, a))
    R, V = x.shape
    S, B = cp.shape
    C = max(V, 1 + int(cp.max())) if S else V
    s = np.exp(x - x.max(1, keepdims=True))
    s /= s.sum(1, keepdims=True)
    e = np.exp(div - div.max(1, keepdims=True))
    gc = e / e.sum(1, keepdims=True)
    g, c = gc[:, :1], gc[:, 1:]
    p = np.zeros((R, C))
    p[:, :V] = g * s
    ids = cp[:, np.arange(R) % B].T                                          # [R, S]
    rows = np.repeat(np.arange(R), S)
    np.add.at(p, (rows, ids.reshape(-1)), (c * a).reshape(-1))
    ll = np.log(p + 1e-12)
    live = y != pad
    yc = np.where((y >= 0) & (y < C), y, 0)
    ll_y = np.where((y >= 0) & (y < C), ll[np.arange(R), yc], math.log(1e-12))
    loss = np.where(live, (1 - eps) * -ll_y - eps / C * ll.sum(1), 0.0)
    hot = np.zeros((R, C))
    ok = live & (y >= 0) & (y < C)
    hot[np.arange(R)[ok], yc[ok]] = 1.0
    w = -((1 - eps) * hot + eps / C) / (p + 1e-12) * live[:, None]
    sw = (w[:, :V] * s).sum(1, keepdims=True)
    dx = g * s * (w[:, :V] - sw)
    wk = np.take_along_axis(w, ids, 1)                                       # [R, S] = w at each position's copy id
    dc = (a * wk).sum(1, keepdims=True)
    m = g * sw + c * dc
    ddiv = np.concatenate([g * (sw - m), c * (dc - m)], 1)
    da = c * wk
    return loss, dx, ddiv, da


def half_ulp_bf16(v):
    """half an ulp of a bf16 number of magnitude |v| (2^-9 to 2^-8 of it)"""
    v = np.abs(np.asarray(v, np.float64))
    return np.where(v > 0, np.exp2(np.floor(np.log2(np.maximum(v, 1e-300))) - 8), 0.0)


def within(name, got, ref, rel_max=1e-5, rel=1e-4, bf16_out=False):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bound = rel_max * np.abs(ref).max() + rel * np.abs(ref)
    if bf16_out:
        bound = bound + half_ulp_bf16(np.maximum(np.abs(ref), np.abs(got)))
    err = np.abs(got - ref)
    bad = ~(err <= bound)
    assert not bad.any(), "%s: %d element(s) outside the bar, worst err %.3e at ref %.3e (max |ref| %.3e)" % (
        name, int(bad.sum()), float(err[bad].max()), float(ref[bad][np.argmax(err[bad])]), float(np.abs(ref).max()))


def loss_within(got, ref, rel=1e-5, floor=1e-6):
    """1e-5 relative, and an absolute floor: a confident row's p(target) is an fp32 number near 1 (resolution 6e-8), so its loss
    -log(p) ~ 1e-4 is resolved to ~1e-7 absolute, as in the reference's fp32 row."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    bad = ~(np.abs(got - ref) <= rel * np.abs(ref) + floor * (ref != 0))
    assert not bad.any(), "loss: %d row(s) outside %.1e relative, e.g. %r vs %r" % (
        int(bad.sum()), rel, got[bad][:3].tolist(), ref[bad][:3].tolist())


def make_case(rng, T, B, V, S, wide, peaked, dup=True):
    """Random rows: copy ids on the vocabulary (below V, duplicated) and, when ``wide``, above it (so C > V); targets that are <pad>,
    vocabulary ids, copy ids below and above V and ids of other graphs.  With ``peaked``, a third of the rows put all but one g*s_k
    below 1e-12.  (Such a row's gradient is tiny unless its target is the peak, and the peak column's dx = g s (w - Sw) cancels in
    fp32 the way the plain loss's s - 1 does: the bars hold it to the largest gradient of the batch, as they hold every row.)"""
    R = T * B
    x = rng.standard_normal((R, V)).astype(np.float32) * 2
    if peaked:
        pk = np.nonzero(rng.random(R) < 1 / 3)[0]
        x[pk] = (rng.standard_normal((len(pk), V)) * 0.5).astype(np.float32)
        x[pk, rng.integers(0, V, len(pk))] += 40.0
    div = rng.standard_normal((R, 2)).astype(np.float32) * 2
    a = rng.random((R, S)).astype(np.float32)
    a[rng.random((R, S)) < 0.2] = 0.0
    a /= np.maximum(a.sum(1, keepdims=True), 1e-6)
    cp = np.empty((S, B), np.int64)
    nxt = V
    for b in range(B):
        for s in range(S):
            r = rng.random()
            if wide and r < 0.4:
                cp[s, b] = nxt + rng.integers(0, 3)          # a few ids >= V, repeated
            elif r < 0.7 or not dup:
                cp[s, b] = rng.integers(1, V)
            else:
                cp[s, b] = cp[rng.integers(0, s), b] if s else PAD
        nxt += 3
    y = rng.integers(1, V, R).astype(np.int64)
    for r in range(R):
        k = rng.random()
        if k < 0.1:
            y[r] = PAD
        elif k < 0.45 and S:
            y[r] = cp[rng.integers(0, S), r % B]              # a copy id of the row's own graph (below or above V)
        elif k < 0.5 and wide:
            y[r] = V + rng.integers(0, nxt - V)               # possibly another graph's id
    return x, div, a, cp, y


# ------------------------------------------------------------------------------------------------ CPU
def test_header_rows_match_float64_statement(host_lib):
    rng = np.random.default_rng(20261016)
    n_rows = 0
    seen = dict(pad=0, vocab=0, copy_lo=0, copy_hi=0, c_eq_v=0, c_gt_v=0, dup=0, peaked=0)
    for rep in range(6):
        for eps in EPS_SET:
            for V in (64, 37):
                for wide in (False, True):
                    for peaked in (False, True):
                        T, B, S = 8, 4, int(rng.integers(1, 12))
                        x, div, a, cp, y = make_case(rng, T, B, V, S, wide, peaked)
                        R = T * B
                        ws = np.zeros(host_lib.ws_words(B, S, V), np.int32)
                        cpc = np.ascontiguousarray(cp)
                        host_lib.build(_p(cpc), B, S, V, _p(ws))
                        C = max(V, 1 + int(cp.max()))
                        assert ws[0] == C
                        seen["c_eq_v" if C == V else "c_gt_v"] += 1
                        seen["dup"] += any(len(set(cp[:, b])) < S for b in range(B))
                        seen["peaked"] += peaked
                        loss = np.zeros(R, np.float32)
                        dx = np.zeros((R, V), np.float32)
                        dd = np.zeros((R, 2), np.float32)
                        da = np.zeros((R, S), np.float32)
                        sums = np.zeros(2, np.float32)
                        for r in range(R):
                            xr, ar = np.ascontiguousarray(x[r]), np.ascontiguousarray(a[r])
                            lo, dxr, ddr, dar = (np.zeros(1, np.float32), np.zeros(V, np.float32), np.zeros(2, np.float32),
                                                 np.zeros(S, np.float32))
                            host_lib.row(_p(xr), V, float(div[r, 0]), float(div[r, 1]), _p(ar), S, B, r % B, int(y[r]), PAD,
                                         float(np.float32(eps)), _p(ws), 1.0, _p(lo), _p(sums), _p(dxr), _p(ddr), _p(dar))
                            loss[r], dx[r], dd[r], da[r] = lo[0], dxr, ddr, dar
                            yb = int(y[r])
                            own = set(cp[:, r % B].tolist())
                            seen["pad" if yb == PAD else "copy_lo" if yb in own and yb < V else "copy_hi" if yb >= V
                                 else "vocab"] += 1
                        ref = reference_rows(x, div, a, cp, y, float(np.float32(eps)))
                        loss_within(loss, ref[0])
                        within("dx eps=%g V=%d" % (eps, V), dx, ref[1])
                        within("d_div eps=%g V=%d" % (eps, V), dd, ref[2])
                        within("d_align eps=%g V=%d" % (eps, V), da, ref[3])
                        n_rows += R
    assert n_rows >= 5000, n_rows
    assert all(v > 0 for v in seen.values()), seen


BAD_EPS = [True, False, -0.1, 1.5, float("nan"), float("inf"), "0.1", None, 1 + 1e-9]
GOOD_EPS = [0, 0.0, 0.1, 1, 1.0, np.float32(0.25)]


def test_constructor_and_setter_argument_checks():
    from gtos_amd.config import build_generator, default_vocabs
    from gtos_amd.decoder import DecodeLayer, TokenGenerator, set_label_smoothing
    from gtos_amd.generator import Generator
    vocabs = default_vocabs()
    for bad in BAD_EPS:
        with pytest.raises(ValueError):
            TokenGenerator(vocabs, 16, 8, 0.0, label_smoothing=bad)
        with pytest.raises(ValueError):
            DecodeLayer(vocabs, 1, 16, 32, 2, 8, 8, 0.0, label_smoothing=bad)
    tg = TokenGenerator(vocabs, 16, 8, 0.0)
    assert tg.label_smoothing == 0.0
    sd = set(tg.state_dict())
    for good in GOOD_EPS:
        t = TokenGenerator(vocabs, 16, 8, 0.0, label_smoothing=good)
        assert type(t.label_smoothing) is float and t.label_smoothing == float(good)
        assert set(t.state_dict()) == sd
    dl = DecodeLayer(vocabs, 1, 16, 32, 2, 8, 8, 0.0, 0.3)          # positional, after every reference argument
    assert dl.token_generator.label_smoothing == pytest.approx(0.3)
    for bad in BAD_EPS:
        with pytest.raises(ValueError):
            set_label_smoothing(dl, bad)
    assert dl.token_generator.label_smoothing == pytest.approx(0.3)  # a refused value changes nothing
    assert set_label_smoothing(dl, 0.1) is dl and dl.token_generator.label_smoothing == pytest.approx(0.1)
    assert not any("label_smoothing" in k for k in dl.state_dict())
    with pytest.raises(ValueError):
        build_generator(Generator, "C1", torch.device("cpu"), label_smoothing=2.0)
    m = build_generator(Generator, "C1", torch.device("cpu"), label_smoothing=0.1)
    m0 = build_generator(Generator, "C1", torch.device("cpu"))
    assert m.decoder.token_generator.label_smoothing == pytest.approx(0.1)
    assert m0.decoder.token_generator.label_smoothing == 0.0
    assert list(m.state_dict()) == list(m0.state_dict())
    assert set_label_smoothing(m0, 1) is m0 and m0.decoder.token_generator.label_smoothing == 1.0


def _dry_step(eps, **kw):
    """recorded launches of the third training step of a C1 bf16 Trainer (model built with label_smoothing=eps unless kw is empty)"""
    from dryrun import DryRun
    from gtos_amd import synth
    from gtos_amd.config import build_generator
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.relindex import attach_relation_index
    from gtos_amd.train import Trainer
    dev = torch.device("cpu")
    with DryRun() as rec:
        model = build_generator(Generator, "C1", dev, factored_relation=True, **kw).to(dev)
        model.set_compute_dtype(torch.bfloat16)
        model.train()
        trainer = Trainer(model, synth.CONFIGS["C1"]["d"], warmup_steps=2000, compute_dtype=torch.bfloat16, world_size=1, rank=0)
        batch, _ = synth.make_config_batch("C1", rank=0)
        attach_relation_index(attach_path_trie(batch))
        trainer.step(batch, sync=False)
        trainer.step(batch, sync=False)
        n = len(rec.calls)
        trainer.step(batch, sync=False)
    return rec, n


def test_dryrun_smoothed_step_takes_the_new_entry_points():
    rec, n = _dry_step(0.1, label_smoothing=0.1)
    hist = {}
    for name, _ in rec.calls[n:]:
        hist[name] = hist.get(name, 0) + 1
    assert hist["gtos_copy_nll_ls_prep"] == hist["gtos_copy_nll_ls_fwd"] == hist["gtos_copy_nll_ls_bwd"] == 1
    assert "gtos_copy_nll_fwd" not in hist and "gtos_copy_nll_bwd" not in hist and "gtos_copy_ll_fwd" not in hist


def test_dryrun_explicit_zero_keeps_the_launch_plan():
    from test_dryrun_launch_plan import _plan
    rec_a, na = _dry_step(None)
    rec_b, nb = _dry_step(0.0, label_smoothing=0.0)
    plan_a, plan_b = _plan(rec_a, na), _plan(rec_b, nb)
    assert plan_a == plan_b
    names = [p[0] for p in plan_a]
    assert names.count("gtos_copy_nll_fwd") == names.count("gtos_copy_nll_bwd") == 1
    assert not any(n.startswith("gtos_copy_nll_ls") for n in names)


# ------------------------------------------------------------------------------------------------ GPU
def dev():
    return torch.device("cuda")


def _dense_torch(logits, div, align, cp, tgt, eps, pad=PAD):
    """section 1 in float64 torch ops (differentiable): per-row loss [T,B]"""
    T, B, V = logits.shape
    S = cp.shape[0]
    C = max(V, 1 + int(cp.max()))
    s = torch.softmax(logits, -1)
    gc = torch.softmax(div, -1)
    p = torch.cat([gc[..., :1] * s, s.new_zeros(T, B, C - V)], -1)
    idx = cp.t().reshape(1, B, S).expand(T, -1, -1)
    p = p.scatter_add(-1, idx, gc[..., 1:] * align)
    ll = torch.log(p + 1e-12)
    nll = -ll.gather(-1, tgt.unsqueeze(-1)).squeeze(-1)
    loss = (1 - eps) * nll - eps / C * ll.sum(-1)
    return loss.masked_fill(tgt.eq(pad), 0.0)


def _gpu_case(T, B, V, S, wide, seed, dtype):
    rng = np.random.default_rng(seed)
    x, div, a, cp, y = make_case(rng, T, B, V, S, wide, peaked=True)
    d = dev()
    lg = torch.from_numpy(x).to(d).to(dtype).reshape(T, B, V)
    dv = torch.from_numpy(div).to(d).to(dtype).reshape(T, B, 2)
    al = torch.from_numpy(a).to(d).reshape(T, B, S)
    return lg, dv, al, torch.from_numpy(cp).to(d), torch.from_numpy(y).to(d).reshape(T, B)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,B,V,S,wide,eps", [(50, 64, 10000, 100, True, 0.1), (7, 5, 1001, 13, True, 0.5),
                                              (6, 3, 64, 9, False, 1.0), (5, 4, 100, 11, True, 0.0)])
def test_kernels_vs_float64_autograd(T, B, V, S, wide, eps, dtype, host_lib):
    from gtos_amd import ops
    from gtos_amd._lib import call, dt, stream
    from tests_support import NAN_BITS, guarded_operand, nan_buffer
    eps = float(np.float32(eps))
    lg, dv, al, cp, y = _gpu_case(T, B, V, S, wide, 7 + V + S, dtype)
    R = T * B
    ld = V + 24
    lg_g = guarded_operand(lg.reshape(R, V), ld=ld)
    dv_g = guarded_operand(dv.reshape(R, 2))
    al_g = guarded_operand(al.reshape(R, S))
    words = ops.ls_workspace_words(B, S, V)
    assert words == host_lib.ws_words(B, S, V)
    ws_buf = nan_buffer(words + 64, torch.float32, dev())
    ws = ws_buf.carve(32, 1, words, words).view(torch.int32)[0]
    f32 = nan_buffer(6 * R + 256, torch.float32, dev())
    loss, lse = f32.carve(32, 1, R, R)[0], f32.carve(64 + R, 1, R, R)[0]
    sums = f32.carve(96 + 2 * R, 1, 2 * R, 2 * R)[0]
    g_up = torch.from_numpy(np.random.default_rng(3).random(R).astype(np.float32) + 0.5).to(dev())
    call("gtos_copy_nll_ls_prep", B, S, V, cp.data_ptr(), ws.data_ptr(), words, stream())
    call("gtos_copy_nll_ls_fwd", dt(lg), T, B, V, S, lg_g.data_ptr(), ld, dv_g.data_ptr(), al_g.data_ptr(), y.data_ptr(), PAD, eps,
         ws.data_ptr(), words, loss.data_ptr(), lse.data_ptr(), sums.data_ptr(), stream())
    gout = nan_buffer(R * (V + 2) + 4096, dtype, dev())
    d_lg = gout.carve(512, R, V, V)
    d_dv = gout.carve(1024 + R * V, R, 2, 2)
    fout = nan_buffer(R * S + 1024, torch.float32, dev())
    d_al = fout.carve(256, R, S, S)
    call("gtos_copy_nll_ls_bwd", dt(lg), T, B, V, S, lg_g.data_ptr(), ld, dv_g.data_ptr(), al_g.data_ptr(), y.data_ptr(), PAD, eps,
         ws.data_ptr(), words, lse.data_ptr(), sums.data_ptr(), g_up.data_ptr(), d_lg.data_ptr(), d_dv.data_ptr(), d_al.data_ptr(),
         stream())
    torch.cuda.synchronize()
    for g_, what in ((ws_buf, "workspace"), (f32, "loss/lse/sums"), (gout, "d_logits/d_div"), (fout, "d_align")):
        g_.check(what)
    # the parallel grouping launch writes what the serial statement of the header does
    ref_ws = np.full(words, NAN_BITS[torch.float32], np.uint32).view(np.int32)     # (entries neither writes keep the band pattern)
    cpn = np.ascontiguousarray(cp.cpu().numpy())
    host_lib.build(_p(cpn), B, S, V, _p(ref_ws))
    assert np.array_equal(ws.cpu().numpy(), ref_ws)
    # float64 autograd of section 1 on the same (exactly upcast) inputs
    L64 = lg.double().requires_grad_(True)
    D64 = dv.double().requires_grad_(True)
    A64 = al.double().requires_grad_(True)
    ref = _dense_torch(L64, D64, A64, cp, y, eps)
    ref.backward(g_up.double().reshape(T, B))
    b16 = dtype == torch.bfloat16
    loss_within(loss.cpu().numpy(), ref.detach().reshape(-1).cpu().numpy())
    within("d_logits", d_lg.float().cpu().numpy(), L64.grad.reshape(R, V).cpu().numpy(), bf16_out=b16)
    within("d_div", d_dv.float().cpu().numpy(), D64.grad.reshape(R, 2).cpu().numpy(), bf16_out=b16)
    within("d_align", d_al.cpu().numpy(), A64.grad.reshape(R, S).cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_op_zero_smoothing_is_bitwise_the_plain_loss(dtype):
    from gtos_amd import ops
    lg, dv, al, cp, y = _gpu_case(9, 6, 1000, 17, True, 5, dtype)
    outs = []
    for kw in ({}, {"label_smoothing": 0.0}):
        L, D, A = (t.clone().requires_grad_(True) for t in (lg, dv, al))
        loss = ops.copy_nll(L, D, A, cp, y, PAD, **kw)
        loss.sum(0).sum().backward()
        outs.append((loss.detach(), L.grad, D.grad, A.grad))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.gpu
def test_model_zero_smoothing_matches_the_plain_model_c1_fp32():
    from gtos_amd import synth
    from gtos_amd.config import build_generator
    from gtos_amd.generator import Generator
    batch, _ = synth.make_config_batch("C1")
    batch = {k: v.to(dev()) for k, v in batch.items()}
    res = []
    for kw in ({}, {"label_smoothing": 0.0}):
        m = build_generator(Generator, "C1", dev(), dropout=0.0, **kw).to(dev())
        m.train()
        loss = m(batch)
        loss.backward()
        res.append((float(loss), {k: p.grad.detach().clone() for k, p in m.named_parameters()}))
    (la, ga), (lb, gb) = res
    assert abs(la - lb) <= 1e-5 * abs(la)
    for k in ga:
        assert float((ga[k] - gb[k]).abs().max()) <= 1e-5 * float(ga[k].abs().max()), k


def _smooth_oracle(ref, eps):
    """the oracle's DecodeLayer with its loss formed from the differentiable work=True row (label_smoothed_nll_loss)"""
    dec = ref.decoder
    plain = dec.forward
    pad = dec.vocabs['predictable_token'].padding_idx

    def forward(probe, graph_state, snt_state, graph_padding_mask, snt_padding_mask, attn_mask, copy_seq, target=None, work=False):
        ll = plain(probe, graph_state, snt_state, graph_padding_mask, snt_padding_mask, attn_mask, copy_seq, work=True)
        nll = -ll.gather(-1, target.unsqueeze(-1)).squeeze(-1)
        loss = (1.0 - eps) * nll + eps / ll.size(-1) * -ll.sum(-1)
        loss = loss.masked_fill(target.eq(pad), 0.0).sum(0)
        ntok = snt_padding_mask.shape[0] - snt_padding_mask.float().sum(0)
        return (loss / ntok).mean()
    dec.forward = forward
    return ref


@pytest.mark.gpu
@pytest.mark.parametrize("cfg_name,B", [("C1", 8), ("C3", 3)])
def test_full_model_vs_oracle_fp32(cfg_name, B):
    from gtos_amd.decoder import set_label_smoothing
    from tests_support import full_model_pair
    ref, m, batch, _ = full_model_pair(dev(), cfg_name, B, layers=2 if cfg_name == "C3" else None)
    _smooth_oracle(ref, 0.1)
    set_label_smoothing(m, 0.1)
    ref.train()
    m.train()
    loss_r = ref(batch)
    loss_r.backward()
    loss = m({k: v.to(dev()) for k, v in batch.items()})
    loss.backward()
    assert abs(loss.item() - loss_r.item()) < 1e-3 * max(1.0, abs(loss_r.item())), (loss.item(), loss_r.item())
    for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters()):
        err = (p.grad.cpu() - q.grad).abs().max().item()
        assert err < 1e-3 + 2e-3 * q.grad.abs().max().item(), (k, err, q.grad.abs().max().item())


@pytest.mark.gpu
def test_c2_slice_bf16_vs_oracle():
    from gtos_amd.decoder import set_label_smoothing
    from tests_support import full_model_pair
    ref, m, batch, _ = full_model_pair(dev(), "C2", 3)
    _smooth_oracle(ref, 0.1)
    set_label_smoothing(m, 0.1)
    m.set_compute_dtype(torch.bfloat16)
    ref.train()
    m.train()
    loss_r = ref(batch)
    loss_r.backward()
    loss = m({k: v.to(dev()) for k, v in batch.items()})
    loss.backward()
    torch.cuda.synchronize()
    assert abs(loss.item() - loss_r.item()) < 1e-2 * max(1.0, abs(loss_r.item())), (loss.item(), loss_r.item())
    grads = {k: q.grad for k, q in ref.named_parameters()}
    table = []
    num = den = 0.0
    for k, p in m.named_parameters():
        g, q = p.grad.cpu().double(), grads[k].double()
        num += float((g - q).pow(2).sum())
        den += float(q.pow(2).sum())
        table.append((k, float((g - q).norm() / max(float(q.norm()), 1e-30)), float(q.norm())))
    assert (num / den) ** 0.5 < 4e-2
    gmax = max(n for _, _, n in table)
    for k, e, n in table:
        if n >= 0.05 * gmax:
            assert e < 0.1, (k, e, n)
        elif n > 1e-4 * gmax:
            assert e < 0.25, (k, e, n)


@pytest.mark.gpu
def test_graph_capture_replays_on_another_batch():
    from gtos_amd import ops
    T, B, V, S = 8, 6, 1000, 15
    lg, dv, al, cp, y = _gpu_case(T, B, V, S, True, 11, torch.bfloat16)
    L, D, A = (t.clone().requires_grad_(True) for t in (lg, dv, al))
    cps, ys = cp.clone(), y.clone()
    up = torch.rand(T, B, device=dev()) + 0.5

    def run():
        out = ops.copy_nll(L, D, A, cps, ys, PAD, label_smoothing=0.1)
        return (out,) + torch.autograd.grad(out, (L, D, A), grad_outputs=up)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        static = run()
    lg2, dv2, al2, cp2, y2 = _gpu_case(T, B, V, S, True, 12, torch.bfloat16)
    cp2 = cp2 + torch.where(cp2 >= V, 40, 0)                  # another C
    y2 = torch.where(y2 >= V, y2 + 40, y2)
    assert int(cp2.max()) > int(cp.max())
    with torch.no_grad():
        for dst, src in ((L, lg2), (D, dv2), (A, al2), (cps, cp2), (ys, y2)):
            dst.copy_(src)
    graph.replay()
    torch.cuda.synchronize()
    got = [t.clone() for t in static]
    eager = run()
    for a, b in zip(got, eager):
        assert torch.equal(a, b)
    ref = _dense_torch(lg2.double(), dv2.double(), al2.double(), cp2, y2, 0.1)
    loss_within(got[0].detach().cpu().numpy(), ref.cpu().numpy())
