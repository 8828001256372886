"""Autograd's gradient contract on the paths that write parameter gradients themselves (ops._grad_target): gradients ACCUMULATE across
backward passes, a parameter may be used more than once, and ``p.grad`` is complete when ``backward()`` returns unless it is a view of a
flat gradient bucket (ops.attach_grad_view), whose readers call ops.join_side() first.

GPU tests (marked one by one) compare against float64 autograd on the same bf16-rounded operands, or against the oracle run in float64;
where the product is compared with itself the only differences are fp32 summation order and atomics.  The CPU tests run the GPU path's
Python glue under the dry-run recorder (tests/dryrun.py)."""
import ctypes

import pytest
import torch

from dryrun import DryRun
from gtos_amd import synth


def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


def rel_fro(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    return float((got - want).norm() / want.norm().clamp_min(1e-30))


def _tn_batch_call(jobs):
    """gtos_gemm_tn_batch on (dY, X, dW target, db target or None) tuples, as ops.flush_dw builds the table."""
    from gtos_amd._lib import call, stream
    n = len(jobs)
    vp, i64, i32 = ctypes.c_void_p * n, ctypes.c_int64 * n, ctypes.c_int * n
    A = vp(*[j[0].data_ptr() for j in jobs]); B = vp(*[j[1].data_ptr() for j in jobs]); C = vp(*[j[2].data_ptr() for j in jobs])
    bias = vp(*[(j[3].data_ptr() if j[3] is not None else None) for j in jobs])
    lda = i64(*[j[0].stride(0) for j in jobs]); ldb = i64(*[j[1].stride(0) for j in jobs]); ldc = i64(*[j[2].stride(0) for j in jobs])
    M_ = i32(*[j[2].shape[0] for j in jobs]); N_ = i32(*[j[2].shape[1] for j in jobs]); K_ = i32(*[j[0].shape[0] for j in jobs])
    call("gtos_gemm_tn_batch", n, ctypes.addressof(A), ctypes.addressof(lda), ctypes.addressof(M_), ctypes.addressof(B), ctypes.addressof(ldb),
         ctypes.addressof(N_), ctypes.addressof(K_), ctypes.addressof(C), ctypes.addressof(ldc), ctypes.addressof(bias), stream())


# ------------------------------------------------------------------------------------------------ A: the raw ABI, duplicate targets
@pytest.mark.gpu
def test_gemm_tn_batch_jobs_on_one_target_all_land():
    """48 jobs (one launch's whole table) on ONE dW [512, 512] and ONE db [512] at a C2 decoder layer's K = 3200: every contribution
    lands, against the float64 sum -- the bar of test_gemm_tn_batch_small_weight_gradients_vs_torch."""
    torch.manual_seed(21)
    K, M, N, n = 3200, 512, 512, 48
    dys = [(torch.randn(K, M, device=dev()) * 0.5).to(torch.bfloat16) for _ in range(n)]
    xs = [(torch.randn(K, N, device=dev()) * 0.5).to(torch.bfloat16) for _ in range(n)]
    base, bias0 = torch.randn(M, N, device=dev()), torch.randn(M, device=dev())
    dw, db = base.clone(), bias0.clone()
    _tn_batch_call([(dy, x, dw, db) for dy, x in zip(dys, xs)])
    torch.cuda.synchronize()
    want = base.double()
    want_b = bias0.double()
    for dy, x in zip(dys, xs):
        want = want + dy.double().t() @ x.double()
        want_b = want_b + dy.double().sum(0)
    print("MEASURED 48 jobs on one target: dW rel. Frobenius %.3e, db %.3e" % (rel_fro(dw, want), rel_fro(db, want_b)))
    torch.testing.assert_close(dw.double(), want, rtol=2e-3, atol=2e-3 * K ** 0.5)
    torch.testing.assert_close(db.double(), want_b, rtol=2e-3, atol=2e-3 * K ** 0.5)


@pytest.mark.gpu
@pytest.mark.parametrize("blocks", ["rows", "cols"])
def test_gemm_tn_batch_partly_overlapping_targets(blocks):
    """Jobs on partly overlapping blocks of one matrix: row blocks [0, 512) and [256, 768) of a [768, 512] matrix, or the same pair as
    column blocks of a [512, 768] matrix sharing its ldc -- several such pairs in one call, so that the overlapping tiles would be written
    by concurrent workgroups if they shared a launch."""
    torch.manual_seed(22 if blocks == "rows" else 23)
    K, pairs = 3200, 6
    base = torch.randn((768, 512) if blocks == "rows" else (512, 768), device=dev())
    out = base.clone()
    want = base.double().clone()
    jobs = []
    for q in range(2 * pairs):
        lo = 0 if q % 2 == 0 else 256
        dy = (torch.randn(K, 512, device=dev()) * 0.5).to(torch.bfloat16)
        x = (torch.randn(K, 512, device=dev()) * 0.5).to(torch.bfloat16)
        tgt = out[lo:lo + 512] if blocks == "rows" else out[:, lo:lo + 512]
        jobs.append((dy, x, tgt, None))
        prod = dy.double().t() @ x.double()
        if blocks == "rows":
            want[lo:lo + 512] += prod
        else:
            want[:, lo:lo + 512] += prod
    _tn_batch_call(jobs)
    torch.cuda.synchronize()
    print("MEASURED overlapping %s blocks: rel. Frobenius %.3e" % (blocks, rel_fro(out, want)))
    torch.testing.assert_close(out.double(), want, rtol=2e-3, atol=2e-3 * K ** 0.5)


# ------------------------------------------------------------------------------------------------ B: ops.linear, bf16, bucket views
def _linear_case(case, batched, monkeypatch, bucket=True):
    """{name: gradient} of one of three reuse patterns on bf16 ops.linear with its gradients in a flat fp32 bucket, and the float64
    autograd gradients of the same computation on the same bf16-rounded operands."""
    from gtos_amd import ops
    monkeypatch.setattr(ops, "DW_BATCH", batched)
    g = torch.Generator().manual_seed(31)
    rows = 3200
    if case == "rows":
        w0 = torch.randn(1536, 512, generator=g) / 512 ** 0.5
        b0 = torch.randn(1536, generator=g) * 0.1
    else:
        w0 = torch.randn(512, 512, generator=g) / 512 ** 0.5
        b0 = torch.randn(512, generator=g) * 0.1
    xs = [torch.randn(rows, 512, generator=g).to(torch.bfloat16) for _ in range(2)]
    gs = [torch.randn(rows, 1024 if case == "rows" else 512, generator=g) for _ in range(2)]

    def model(lin, w, b, x, cotangent):
        if case == "rows":             # two overlapping row blocks of one packed projection: rows 512..1023 are in both
            y = lin(x, w, b, (0, 1024)).float() + lin(x, w, b, (512, 1536)).float()
        elif case == "twice":           # one square layer applied twice in one forward
            y = lin(lin(x, w, b, None), w, b, None).float()
        else:                           # "two_backward": one use per forward, two forwards and backwards before the join
            y = lin(x, w, b, None).float()
        return (y * cotangent).sum()

    w = w0.to(dev()).requires_grad_()
    b = b0.to(dev()).requires_grad_()
    flat = torch.zeros(w.numel() + b.numel(), device=dev())
    if bucket:
        ops.attach_grad_view(w, flat[:w.numel()].view(w.shape))
        ops.attach_grad_view(b, flat[w.numel():].view(b.shape))

    def hip_lin(x, w_, b_, r):
        return ops.linear(x, w_, b_, rows=r)
    noted = []
    if case == "two_backward":
        for k in range(2):
            model(hip_lin, w, b, xs[k].to(dev()), gs[k].to(dev())).backward()
            noted.append(len(ops._DW_PENDING.get(dev(), [])))
    else:
        model(hip_lin, w, b, xs[0].to(dev()), gs[0].to(dev())).backward()
        noted.append(len(ops._DW_PENDING.get(dev(), [])))
    ops.join_side()
    torch.cuda.synchronize()
    got = {"weight": w.grad.detach().clone(), "bias": b.grad.detach().clone()}

    # float64 autograd: the operands the kernels saw (bf16 weight, bf16 input), no rounding inside
    w64 = w0.to(torch.bfloat16).double().requires_grad_()
    b64 = b0.double().requires_grad_()

    def ref_lin(x, w_, b_, r):
        if r is not None:
            w_, b_ = w_[r[0]:r[1]], b_[r[0]:r[1]]
        return x.double() @ w_.t() + b_
    for k in range(2 if case == "two_backward" else 1):
        model(ref_lin, w64, b64, xs[k], gs[k].double()).backward()
    want = {"weight": w64.grad, "bias": b64.grad}
    return got, want, noted


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["twice", "two_backward", "rows"])
def test_linear_reused_parameter_gradients_vs_fp64(case, monkeypatch):
    """A parameter used twice in one forward, two backward passes before one ops.join_side(), and overlapping ``rows=`` blocks of one
    in_proj weight: the bucket holds the SUM of all contributions.  Against float64 autograd: per-parameter relative Frobenius error at
    bf16 level (a lost contribution is ~0.5); against the same computation with DW_BATCH off: 1e-4."""
    got, want, noted = _linear_case(case, True, monkeypatch)
    assert min(noted) > 0                       # the batched path really took these jobs
    plain, _, noted0 = _linear_case(case, False, monkeypatch)
    assert max(noted0) == 0
    for k in got:
        e_ref, e_plain = rel_fro(got[k], want[k]), rel_fro(got[k], plain[k])
        print("MEASURED %s %s: vs fp64 %.3e, vs DW_BATCH off %.3e" % (case, k, e_ref, e_plain))
        assert e_ref < 2e-2, (case, k, e_ref)
        assert e_plain < 1e-4, (case, k, e_plain)


# ------------------------------------------------------------------------------------------------ C: the whole Generator at C1
def _force_side_paths(monkeypatch, trie):
    from gtos_amd import ops, gru
    monkeypatch.setattr(ops, "BWD_SIDE", True)
    monkeypatch.setattr(gru, "SIDE_STREAM", True)
    monkeypatch.setattr(gru, "TRIE_SIDE", True)
    monkeypatch.setattr(ops, "BWD_SIDE_MIN_ROWS", 0)          # C1 is below the size thresholds: force the side paths
    monkeypatch.setattr(gru, "SIDE_MIN_ROWS", 0)
    monkeypatch.setattr(gru, "TRIE", trie)


def _c1_model(device, dtype):
    from gtos_amd.config import build_generator
    from gtos_amd.generator import Generator
    m = build_generator(Generator, "C1", device, dropout=0.0).to(device)
    m.set_compute_dtype(dtype)
    m.train()
    return m


def _grads(m):
    return {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}


def _tight(got, want, scale, bar, what):
    """per parameter: |got - want|_F / scale (the summed norms of the parts of ``want``): fp32 order and atomics only"""
    assert set(got) == set(want), what
    worst = max((float((got[k].double() - want[k].double()).norm() / max(scale[k], 1e-30)), k) for k in want)
    print("MEASURED %s: worst per-parameter rel. Frobenius %.3e (%s)" % (what, worst[0], worst[1]))
    return [] if worst[0] < bar else [(what,) + worst]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,trie", [(torch.float32, False), (torch.bfloat16, True), (torch.bfloat16, False)],
                         ids=["fp32", "bf16-trie", "bf16-packed"])
@pytest.mark.parametrize("storage", ["plain", "bucket"])
def test_generator_gradients_accumulate(dtype, trie, storage, monkeypatch):
    """The product Generator at C1 with the side-stream paths forced on: (1) batch 1 backward, then batch 2 backward without zeroing ->
    g(batch 1) + g(batch 2); (2) zero_grad(set_to_none=False) after a step, then a second step -> a fresh gradient of that batch;
    (3) two forwards, one backward of loss1 + loss2 -> g(batch 1) + g(batch 2).  ``p.grad`` is read right after backward() -- a plain
    ``.grad`` is complete then; a bucket is read after ops.join_side(), as its contract says.  fp32: also against the oracle in float64."""
    from gtos_amd import ops
    from gtos_amd.flat import FlatParams
    _force_side_paths(monkeypatch, trie)
    b1, _ = synth.make_config_batch("C1", rank=0)
    b2, _ = synth.make_config_batch("C1", rank=1)
    d1, d2 = ({k: v.to(dev()) for k, v in b.items()} for b in (b1, b2))
    m = _c1_model(dev(), dtype)
    flat = FlatParams(m, mirror_dtype=dtype) if storage == "bucket" else None

    def reset():
        if flat is None:
            m.zero_grad(set_to_none=True)
        else:
            flat.zero_grad()

    left = []

    def done():
        if flat is not None:
            ops.join_side()
        elif ops._DW_PENDING or ops._PENDING_SIDE:                      # nothing may be deferred without a bucket
            left.append((sum(len(v) for v in ops._DW_PENDING.values()), sorted(map(str, ops._PENDING_SIDE))))
        torch.cuda.synchronize()
        return _grads(m)

    # the product's own per-batch gradients, each from an empty gradient
    reset(); m(d1).backward(); g1 = done()
    reset(); m(d2).backward(); g2 = done()
    assert float(max(t.abs().max() for t in g1.values())) > 0
    summed = {k: g1[k] + g2[k] for k in g1}
    n1 = {k: float(g1[k].double().norm()) for k in g1}
    n2 = {k: float(g2[k].double().norm()) for k in g2}
    n12 = {k: n1[k] + n2[k] for k in g1}
    # a lost contribution is of the order of one batch's gradient (0.3 .. 0.7 of the scale); fp32 sums in another order, and the atomics
    # (embedding scatter, bias partial sums), stay far below.  bf16: an atomic fp32 sum that is rounded to a bf16 operand can round the
    # other way, and that difference travels on.
    bar = 1e-5 if dtype == torch.float32 else 1e-4
    # (1) accumulation
    reset(); m(d1).backward(); m(d2).backward(); acc = done()
    bad = _tight(acc, summed, n12, bar, "accumulated %s %s" % (storage, dtype))
    # (3) two forwards, one backward
    reset(); (m(d1) + m(d2)).backward(); both = done()
    bad += _tight(both, summed, n12, bar, "two forwards %s %s" % (storage, dtype))
    # (2) a pre-set, zeroed gradient
    reset(); m(d1).backward(); done()
    if flat is None:
        m.zero_grad(set_to_none=False)
    else:
        flat.zero_grad()
    m(d2).backward(); pre = done()
    bad += _tight(pre, g2, n2, bar, "zeroed, not unset %s %s" % (storage, dtype))
    if dtype == torch.float32:
        from oracle import gtos_oracle as O
        from gtos_amd.config import generator_args
        torch.manual_seed(19940117)
        ref = O.Generator({k: O.VocabSpec(v, 0) for k, v in synth.DEFAULT_VOCAB.items()}, depth_size=32,
                          **dict(generator_args(synth.CONFIGS["C1"]), dropout=0.0))
        ref.load_state_dict({k: v.detach().cpu() for k, v in m.state_dict().items()})
        ref = ref.double()
        ref.train()
        ref(b1).backward()
        ref(b2).backward()
        for k, q in ref.named_parameters():
            err = (acc[k].cpu().double() - q.grad).abs().max().item()
            assert err < 1e-3 + 2e-3 * q.grad.abs().max().item(), (k, err, q.grad.abs().max().item())
    assert not left, "work outstanding after backward() returned: %s" % left
    assert not bad, bad


# ------------------------------------------------------------------------------------------------ D: an exception inside backward
class _RaiseInBackward(torch.autograd.Function):
    """Identity whose backward raises as soon as small weight-gradient jobs are waiting (and records how many)."""
    seen = []

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        from gtos_amd import ops
        waiting = sum(len(v) for v in ops._DW_PENDING.values())
        if not waiting:
            return g
        _RaiseInBackward.seen.append(waiting)
        raise RuntimeError("failing backward (test)")


def _arm_raise(monkeypatch):
    """Every ops.LinearFn input that needs a gradient passes _RaiseInBackward: backward raises at the first of them it reaches after a
    Linear downstream of it has noted its weight-gradient job."""
    from gtos_amd import ops
    real = ops.LinearFn.apply
    _RaiseInBackward.seen = []

    def apply(x, *a):
        return real(_RaiseInBackward.apply(x) if x.requires_grad else x, *a)
    monkeypatch.setattr(ops.LinearFn, "apply", apply)


def _failed_then_clean_step(device, batch, monkeypatch):
    """(trainer after a step whose backward raised + one clean step, fresh trainer after the same clean step with the failed step's
    counters).  A failed step's forward was counted (the device-side step control ran before backward), so the fresh trainer starts from
    those counters: the learning rate of its clean step is the same."""
    from gtos_amd import ops
    from gtos_amd.train import Trainer
    out = []
    counters = None
    for fail_first in (True, False):
        m = _c1_model(device, torch.bfloat16)
        tr = Trainer(m, 256, warmup_steps=100, compute_dtype=torch.bfloat16)
        if fail_first:
            with monkeypatch.context() as mp:
                _arm_raise(mp)
                with pytest.raises(RuntimeError, match="failing backward"):
                    tr.step(batch)
            assert _RaiseInBackward.seen and _RaiseInBackward.seen[0] > 0      # a Linear had noted its job when backward raised
            assert not ops._DW_PENDING                                          # ... and the failed step dropped it
            counters = tr.counters()
        else:
            tr.set_counters(counters[1], counters[0], counters[2])
        tr.step(batch)
        out.append(tr)
    return out


@pytest.mark.gpu
def test_exception_in_backward_leaves_nothing_for_the_next_step(monkeypatch):
    """D: a backward that raises part-way, caught, then one clean Trainer.step: parameters and Adam moments equal those of a fresh trainer
    that ran only the clean step."""
    batch, _ = synth.make_config_batch("C1", rank=0)
    batch = {k: v.to(dev()) for k, v in batch.items()}
    failed, fresh = _failed_then_clean_step(dev(), batch, monkeypatch)
    torch.cuda.synchronize()
    for name in ("param", "m", "v"):
        a, b = getattr(failed.flat, name), getattr(fresh.flat, name)
        err = float((a - b).abs().max())
        print("MEASURED exception then clean step, %s: max abs diff %.3e" % (name, err))
        assert err <= 1e-6, (name, err)


# ------------------------------------------------------------------------------------------------ CPU: the dry run (E, F, G)
def _dry_batch(cfg, B=None):
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.relindex import attach_relation_index
    batch, _ = synth.make_config_batch(cfg, rank=0, B=B)
    return attach_relation_index(attach_path_trie(batch))


@pytest.mark.parametrize("cfg", ["C1", "C2"])
def test_batched_weight_gradient_launches_have_disjoint_targets(cfg):
    """E: every gtos_gemm_tn_batch table a bf16 Trainer.step records has pairwise disjoint dW byte ranges within each 48-job launch, so
    the entry point's split at an overlapping target never adds a launch to these steps."""
    from gtos_amd.config import build_generator
    from gtos_amd.generator import Generator
    from gtos_amd.train import Trainer
    tables = []
    with DryRun() as rec:
        real = rec._check_other

        def check(name, a):
            if name == "gtos_gemm_tn_batch":           # the host arrays live only during the call: read them here
                n = a[0]
                M = list((ctypes.c_int * n).from_address(a[3]))
                N = list((ctypes.c_int * n).from_address(a[6]))
                C = list((ctypes.c_void_p * n).from_address(a[8]))
                ldc = list((ctypes.c_int64 * n).from_address(a[9]))
                tables.append([(C[j], C[j] + ((M[j] - 1) * ldc[j] + N[j]) * 4) for j in range(n)])
            return real(name, a)
        rec._check_other = check
        cpu = torch.device("cpu")
        m = build_generator(Generator, cfg, cpu).to(cpu)
        m.set_compute_dtype(torch.bfloat16)
        m.train()
        trainer = Trainer(m, synth.CONFIGS[cfg]["d"], warmup_steps=2000, compute_dtype=torch.bfloat16, world_size=1, rank=0)
        trainer.step(_dry_batch(cfg), sync=False)
    jobs = sum(len(t) for t in tables)
    print("E %s: %d gtos_gemm_tn_batch calls, %d jobs" % (cfg, len(tables), jobs))
    assert tables and jobs >= 20, [len(t) for t in tables]
    for t in tables:
        for c0 in range(0, len(t), 48):
            chunk = sorted(t[c0:c0 + 48])
            for (lo0, hi0), (lo1, hi1) in zip(chunk, chunk[1:]):
                assert hi0 <= lo1, "two jobs of one launch write the same bytes: [%x, %x) and [%x, %x)" % (lo0, hi0, lo1, hi1)


def test_plain_grad_leaves_no_deferred_work(monkeypatch):
    """F: a plain bf16 Generator (no bucket) whose ``.grad`` tensors exist -- zero_grad(set_to_none=False), gradient accumulation -- with
    the side-stream paths forced on: nothing is left outstanding when backward() returns, because only bucket views are written in place."""
    from gtos_amd import ops
    _force_side_paths(monkeypatch, True)
    with DryRun():
        try:
            m = _c1_model(torch.device("cpu"), torch.bfloat16)
            batch = _dry_batch("C1")
            m(batch).backward()                        # p.grad unset: autograd's
            assert not ops._DW_PENDING and not ops._PENDING_SIDE
            m.zero_grad(set_to_none=False)
            assert all(p.grad is not None for p in m.parameters() if p.requires_grad)
            m(batch).backward()
            pending = sum(len(v) for v in ops._DW_PENDING.values())
            assert pending == 0 and not ops._PENDING_SIDE, (pending, ops._PENDING_SIDE)
        finally:
            ops.discard_dw()
            ops.join_side()


def test_failed_backward_drops_noted_jobs_dry_run(monkeypatch):
    """G: scenario D under the dry run -- the small weight-gradient jobs a raising backward had noted are gone once Trainer.step re-raises."""
    from gtos_amd import ops
    with DryRun():
        try:
            _failed_then_clean_step(torch.device("cpu"), _dry_batch("C1"), monkeypatch)
        finally:
            ops.discard_dw()
            ops.join_side()
