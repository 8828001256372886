"""Distribution-shaped truncation of the sampling decode (Generator.work(search="sample", min_p=, typical_p=, epsilon_cutoff=,
eta_cutoff=), gtos_amd.search.sample_device, csrc/truncate.hip, csrc/truncate_kernels.h).

CPU: the rule header compiled with g++ against a numpy statement of the rule on random rows, Generator.work's argument checks, and
the launch plan under the dry run.  GPU: gtos_truncate_block against the same numpy statement inside sentinel columns, the law of
the draw after a truncation against the renormalised softmax on the kept set, and end to end on the C1 fp32 model.

Near ties.  The numpy statement sums in another order than the header (and the kernel in a third), and its exp / log may differ in
the last place, so a row is left out of a comparison when a decision of the rule hangs on less than NEAR = 1e-9 relative:
  * a column sits on the stage-1 threshold m + log(min_p): |x_c - thr| <= NEAR (|m| + |log min_p|), the magnitudes of the two terms the
    threshold is the sum of (only with min_p < 1: log 1 = 0 and x_c >= m are exact);
  * a cumulative mass sits on typical_p Z: |mass - typical_p Z| <= NEAR typical_p Z;
  * a deviation next to d* lies on an fp32 rounding boundary: dev_c = fp32(|a_c - H|) with a_c = -(x_c - m - log Z); a_c and H carry
    errors relative to their own size, so column c is "unstable" when fp32(|a_c - H| - tol_c) != fp32(|a_c - H| + tol_c) with
    tol_c = NEAR (|a_c| + |H|).  Moving one column by one fp32 step changes the kept set only if it meets or crosses ANOTHER column's
    deviation at the cut (with every deviation around d* more than a step apart the order, the cumulative masses and so the set stay
    what they are; columns with equal x move together).  So the row is flagged when an unstable column reaches [d* - 1 ulp, d* + 1 ulp]
    and a column with a different x reaches that interval too;
  * a p' sits on thr: |p'_c - thr| <= NEAR thr (the best survivor, which always stays, aside).
The cap on flagged rows is rows // 200."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver
from test_sample_decode import allowed_mask, random_row, random_tables, f32, np_kept, np_select, NEAR, UNK_


DRIVER = r"""
#include "truncate_kernels.h"
extern "C" int truncate_row(float* ll, int tot, int V, int b, int t, int min_t, const uint8_t* fs, const uint8_t* fl,
                            const uint8_t* owned, float T, float min_p, float typical_p, float eps, float eta) {
    return gtos_truncate::truncate_serial(ll, tot, V, b, t, min_t, fs, fl, owned, (double)T, (double)min_p, (double)typical_p,
                                          (double)eps, (double)eta);
}
// stage 2's threshold over n (deviation, weight) pairs: the plain bisection of truncate_serial, or the kernel's with narrow()
extern "C" float typical_dstar(const float* dev, const double* w, int n, double share, int narrowed, int* passes) {
    using namespace gtos_truncate;
    double Z = 0.0;
    float dmin = INFINITY, dmax = 0.0f;
    for (int i = 0; i < n; ++i) { Z += w[i]; dmin = dev[i] < dmin ? dev[i] : dmin; dmax = dev[i] > dmax ? dev[i] : dmax; }
    uint32_t klo = order_key(dmin) - 1, khi = order_key(dmax);
    for (*passes = 0; khi - klo > 1; ++*passes) {
        const uint32_t mid = bisect_mid(klo, khi);
        const float v = order_value(mid), vhi = order_value(khi);
        double mass = 0.0;
        float below = -INFINITY, above = INFINITY;
        for (int i = 0; i < n; ++i) {
            if (dev[i] <= v) { mass += w[i]; below = dev[i] > below ? dev[i] : below; }
            else if (dev[i] <= vhi) above = dev[i] < above ? dev[i] : above;
        }
        const bool enough = mass >= share * Z;
        if (narrowed) narrow(klo, khi, mid, enough, below, above);
        else if (enough) khi = mid;
        else klo = mid;
    }
    return order_value(khi);
}
"""

# (min_p, typical_p, epsilon_cutoff, eta_cutoff)
CUTS = [(0.05, 1.0, 0.0, 0.0), (0.5, 1.0, 0.0, 0.0), (1.0, 1.0, 0.0, 0.0), (0.0, 0.2, 0.0, 0.0), (0.0, 0.9, 0.0, 0.0),
        (0.0, 0.95, 0.0, 0.0), (0.0, 1.0, 3e-4, 0.0), (0.0, 1.0, 0.0, 2e-3), (0.0, 1.0, 0.02, 0.3), (0.1, 0.8, 1e-3, 4e-3),
        (0.02, 0.5, 0.0, 0.05)]
GRID = [(T, cut) for T in (0.3, 1.0, 2.5) for cut in CUTS]
OFF = (0.0, 1.0, 0.0, 0.0)


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = compile_host_driver(tmp_path_factory, "truncate_host", DRIVER)
    so.truncate_row.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 3 + [ctypes.c_float] * 5
    so.truncate_row.restype = ctypes.c_int
    so.typical_dstar.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_double, ctypes.c_int, ctypes.c_void_p]
    so.typical_dstar.restype = ctypes.c_float
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the rule, stated in numpy
def np_truncate(ll, allow, T, min_p, typical_p, eps, eta):
    """The rule of csrc/truncate_kernels.h on one row: ``allow`` its allowed set, the five settings as the fp32 values the kernel
    takes.  -> (mask of the survivors, near tie as the module docstring defines it)."""
    keep = allow.copy()
    if not allow.any():
        return keep, False
    near = False
    with np.errstate(divide="ignore", invalid="ignore"):
        x = ll.astype(np.float64) / T
    cols = np.nonzero(keep)[0]
    m = x[cols].max()
    if min_p > 0:
        L = math.log(min_p)
        thr = m + L
        if min_p < 1:
            near |= bool((np.abs(x[cols] - thr) <= NEAR * (abs(m) + abs(L))).any())
        keep[cols[x[cols] < thr]] = False
        cols = np.nonzero(keep)[0]
    if typical_p < 1:
        d = x[cols] - m
        w = np.exp(d)
        Z, E = w.sum(), (w * d).sum()
        logZ = math.log(Z)
        H = logZ - E / Z
        a = -(d - logZ)
        dd = np.abs(a - H)
        dev = dd.astype(np.float32)
        order = np.argsort(dev, kind="stable")
        dv, cum = dev[order], np.cumsum(w[order])
        ends = np.nonzero(np.r_[dv[1:] > dv[:-1], True])[0]            # last index of each run of equal deviations
        mass = cum[ends]
        near |= bool((np.abs(mass - typical_p * Z) <= NEAR * typical_p * Z).any())
        ok = mass >= typical_p * Z
        dstar = dv[ends[int(np.argmax(ok)) if ok.any() else -1]]
        tol = NEAR * (np.abs(a) + abs(H))
        lo, hi = np.maximum(dd - tol, 0.0).astype(np.float32), (dd + tol).astype(np.float32)
        reach = (hi >= np.nextafter(dstar, np.float32(-np.inf))) & (lo <= np.nextafter(dstar, np.float32(np.inf)))
        if (reach & (lo != hi)).any() and np.unique(x[cols][reach]).size > 1:
            near = True
        keep[cols[dev > dstar]] = False
        cols = np.nonzero(keep)[0]
    if eps > 0 or eta > 0:
        best = cols[np.lexsort((cols, -ll[cols].astype(np.float64)))[0]]
        d = x[cols] - x[cols].max()
        w = np.exp(d)
        Z, E = w.sum(), (w * d).sum()
        H = math.log(Z) - E / Z
        thr = max(eps if eps > 0 else 0.0, min(eta, math.sqrt(eta) * math.exp(-H)) if eta > 0 else 0.0)
        p = w / Z
        near |= bool(((np.abs(p - thr) <= NEAR * thr) & (cols != best)).any())
        keep[cols[(p < thr) & (cols != best)]] = False
    return keep, bool(near)


def check_row(tag, got, ll, allow, keep):
    """A truncated row against the statement: survivors and columns outside the allowed set keep their bits, the rest is -inf."""
    same = keep | ~allow
    assert np.array_equal(bits(got)[same], bits(ll)[same]), tag
    gone = got[allow & ~keep]
    assert np.isneginf(gone).all(), tag
    if allow.any():
        assert keep.any(), tag


# ------------------------------------------------------------------------------------------------ CPU
def test_rule_header_matches_numpy_rule(host_lib):
    rng = np.random.RandomState(20261020)
    rows = near = empty = cut_rows = 0
    for T, cut in GRID:
        Tf, (mp, tp, ep, et) = f32(T), [f32(v) for v in cut]
        for _ in range(300):
            tot = int(rng.choice([3, 8, 40, 117, 300, 5000]))
            V = int(rng.randint(1, tot + 1))
            B = int(rng.randint(1, 4))
            fs, fl, owned = random_tables(rng, B, V, tot, p_unk=float(rng.choice([0.04, 0.6])))
            ll = random_row(rng, tot)
            if rows % 97 == 0:
                ll[:] = -np.inf                                         # nothing allowed
            b, t, min_t = int(rng.randint(B)), int(rng.randint(6)), int(rng.randint(5))
            allow = allowed_mask(ll, V, fs, fl[b], owned[b], t, min_t)
            keep, amb = np_truncate(ll, allow, Tf, mp, tp, ep, et)
            got = ll.copy()
            n = host_lib.truncate_row(_p(got), tot, V, b, t, min_t, _p(fs), _p(fl), _p(owned), Tf, mp, tp, ep, et)
            rows += 1
            empty += not allow.any()
            if amb:
                near += 1
                continue
            tag = (T, cut, tot, V)
            assert n == (int(keep.sum()) if allow.any() else -1), tag
            check_row(tag, got, ll, allow, keep)
            cut_rows += bool((allow & ~keep).any())
    print("MEASURED truncate_serial vs numpy: %d rows, %d near ties, %d with nothing allowed, %d cut" % (rows, near, empty, cut_rows))
    assert rows == 9900 and near <= rows // 200, (rows, near)
    assert 0 < empty < rows // 20 and cut_rows > rows // 2, (empty, cut_rows)


def test_narrowed_search_finds_the_bisection_s_threshold(host_lib):
    """The kernel's search for d* (gtos_truncate::narrow after every pass) against the plain bisection on the same pairs: the same
    threshold, never more passes, and far fewer on a long row."""
    rng = np.random.RandomState(7)
    total = {0: 0, 1: 0}
    for case in range(400):
        n = int(rng.choice([1, 2, 3, 17, 300, 5000]))
        dev = np.abs(rng.randn(n) * 10.0 ** rng.randint(-6, 3)).astype(np.float32)
        if case % 4 == 0:
            dev = np.round(dev * 4) / np.float32(4)                     # ties, zeros
        if case % 7 == 0:
            dev[rng.randint(n)] = np.inf                                # a deviation past fp32
        w = np.exp(rng.randn(n) * 3.0)
        share = f32(rng.choice([0.2, 0.5, 0.9, 0.95, 0.999]))
        got = []
        for narrowed in (0, 1):
            passes = ctypes.c_int(0)
            got.append((host_lib.typical_dstar(_p(dev), _p(w), n, share, narrowed, ctypes.byref(passes)), passes.value))
            total[narrowed] += passes.value if n == 5000 else 0
        (d0, p0), (d1, p1) = got
        assert d0 == d1 and d0 in dev and p1 <= p0 <= 32, (case, n, got)
        order = np.argsort(dev, kind="stable")
        cum = np.cumsum(w[order])
        if not (np.abs(cum - share * w.sum()) <= NEAR * share * w.sum()).any():
            assert d0 == dev[order][np.argmax(cum >= share * w.sum())] or not (cum >= share * w.sum()).any(), (case, n)
    print("MEASURED passes on the 5000-pair cases: %d plain, %d narrowed" % (total[0], total[1]))
    assert total[1] * 3 < total[0] * 2


def test_work_checks_the_truncation_arguments():
    """No model needed: the checks run before anything is touched."""
    from gtos_amd.generator import Generator, check_truncation
    bad = [dict(min_p=-0.1), dict(min_p=1.5), dict(min_p=float("nan")), dict(min_p=1e-50), dict(min_p="0.1"), dict(min_p=True),
           dict(typical_p=0.0), dict(typical_p=-0.5), dict(typical_p=1.01), dict(typical_p=float("nan")), dict(typical_p=1 - 1e-12),
           dict(typical_p=None), dict(epsilon_cutoff=-1e-3), dict(epsilon_cutoff=1.0), dict(epsilon_cutoff=float("inf")),
           dict(epsilon_cutoff=1e-60), dict(eta_cutoff=-1e-3), dict(eta_cutoff=1.0), dict(eta_cutoff=2.0), dict(eta_cutoff=float("nan")),
           dict(eta_cutoff=1 - 1e-12)]
    for kw in bad:
        with pytest.raises(ValueError):
            Generator.work(None, {}, 4, 10, search="sample", **kw)
    for kw in (dict(min_p=0.05), dict(typical_p=0.9), dict(epsilon_cutoff=3e-4), dict(eta_cutoff=2e-3), dict(min_p=1.0)):
        for search in ("host", "device", "stochastic"):
            with pytest.raises(ValueError):
                Generator.work(None, {}, 4, 10, search=search, **kw)
        assert check_truncation("sample", **dict(dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0), **kw)) == kw
    for search in ("host", "device", "sample", "stochastic"):
        assert check_truncation(search, 0.0, 1.0, 0.0, 0.0) == {} == check_truncation(search, 0, 1, 0, 0)


def test_truncate_entry_point_refuses_bad_arguments():
    """-10 for settings outside the rule, -23 for null pointers, nothing launched, no device needed."""
    from gtos_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 33
    p = ctypes.c_void_p(16)

    def call(N=8, k=4, t=0, V=10, tot=12, T=1.0, cut=(0.1, 0.9, 1e-3, 1e-3), ld=12, ll=p, fs=p, fl=p, owned=p, state=p, active=p):
        return lib.gtos_truncate_block(N, k, t, V, tot, 0, T, *cut, ll, ld, fs, fl, owned, state, active, None)
    assert call(cut=OFF) == -10
    for i, values in enumerate(((-0.1, 1.5, float("nan")), (0.0, -0.1, 1.5, float("nan")), (-0.1, 1.0, float("nan")),
                                (-0.1, 1.0, float("nan")))):
        for v in values:
            assert call(cut=OFF[:i] + (v,) + (0.5,) * (3 - i)) == -10, (i, v)
    for T in (0.0, -1.0, float("inf"), float("nan")):
        assert call(T=T) == -10
    assert call(N=9) == -10 and call(k=0) == -10 and call(t=-1) == -10 and call(ld=11) == -10 and call(tot=9) == -10 and call(V=0) == -10
    for name in ("ll", "fs", "fl", "owned", "state", "active"):
        assert call(**{name: None}) == -23, name
    assert call(N=0, k=0, cut=OFF) == 0


def test_launch_plan_adds_one_truncate_block_per_step():
    from dryrun import DryRun
    from gtos_amd import synth
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.vocab import PAD, UNK, STR, END
    steps, k = 5, 4
    with DryRun() as rec:
        vocabs = synth.synth_vocabs()
        torch.manual_seed(1)
        model = Generator(vocabs, device=torch.device("cpu"), depth_size=32, **generator_args(synth.CONFIGS["C1"]))
        model.set_compute_dtype(torch.bfloat16)
        model.eval()
        batch, _ = synth.make_config_batch("C1", train=False)
        batch = attach_path_trie(batch)
        pv, cp = vocabs['predictable_token'], batch['cp_seq']
        batch['local_idx2token'] = [{int(i): "copy%d" % int(i) for i in cp[:, b].tolist() if i >= pv.size} for b in range(cp.shape[1])]
        B = batch['concept'].shape[1]

        def plan(**kw):
            n0 = len(rec.calls)
            assert len(model.work(batch, k, steps, search="sample", seed=3, **kw)) == B
            return rec.calls[n0:]
        base = [c[0] for c in plan()]
        assert base.count("gtos_sample_step") == steps and "gtos_truncate_block" not in base
        assert [c[0] for c in plan(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)] == base
        calls = plan(typical_p=0.9, temperature=0.7)
        names = [c[0] for c in calls]
        assert [x for x in names if x != "gtos_truncate_block"] == base
        at = [i for i, x in enumerate(names) if x == "gtos_truncate_block"]
        assert len(at) == steps and all(names[i + 1] == "gtos_sample_step" for i in at)
        for t, i in enumerate(at):
            a, s = calls[i][1], calls[i + 1][1]
            assert a[:6] == (B * k, k, t) + s[3:6] and a[6] == s[7] == 0.7                 # N, k, t, V, tot, min_t, temperature
            assert a[7:11] == (0.0, f32(0.9), 0.0, 0.0)
            assert a[11] == s[11] and a[12] == s[12] and a[13:16] == s[13:16]             # ll, ld, the three class tables
            assert a[16] == s[17] and a[17] == s[19]                                        # slot_state, active
        # after the bans, directly before the draw
        word = next(pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END))
        avoid = [[word] for _ in range(B)]
        names = [c[0] for c in plan(min_p=0.05, eta_cutoff=2e-3, no_repeat_ngram=3, avoid=avoid)]
        assert names.count("gtos_truncate_block") == steps == names.count("gtos_avoid_block") and names.count("gtos_ngram_block") == steps - 1
        for i, x in enumerate(names):
            if x == "gtos_truncate_block":
                assert names[i + 1] == "gtos_sample_step" and names[i - 1] == "gtos_avoid_block"
            elif x in ("gtos_avoid_block", "gtos_ngram_block"):
                assert names[i + 1] in ("gtos_truncate_block", "gtos_avoid_block")
            elif x == "gtos_sample_step":
                assert names[i - 1] == "gtos_truncate_block"


# ------------------------------------------------------------------------------------------------ GPU: the kernel
SENTINEL = 12345.0


def _run_truncate(t, k, V, tot, min_t, T, cut, ll, fs, fl, owned, state, active, pad=7):
    """One ops.truncate_block on numpy tables, ll inside a [N, tot + pad] buffer of sentinels -> the whole buffer after it"""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    buf = torch.full((ll.shape[0], tot + pad), SENTINEL, dtype=torch.float32, device=dev)
    buf[:, :tot] = D(ll)
    g_state, g_active = D(state), D(active)
    ops.truncate_block(t, k, V, tot, min_t, T, *cut, buf[:, :tot], D(fs), D(fl) if tot > V else None, D(owned) if tot > V else None,
                       g_state, g_active)
    assert np.array_equal(g_state.cpu().numpy(), state) and np.array_equal(g_active.cpu().numpy(), active)     # read only
    return buf.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("tot", [3, 32, 997, 20000])
def test_truncate_block_matches_numpy_rule(tot):
    rng = np.random.RandomState(1000 + tot)
    B, k = 3, 6
    N = B * k
    V = tot - max(1, tot // 8)
    rows = checked = near = cut_rows = 0
    for T, cut in GRID:
        Tf, cutf = f32(T), tuple(f32(v) for v in cut)
        fs, fl, owned = random_tables(rng, B, V, tot)
        ll = np.stack([random_row(rng, tot) for _ in range(N)])
        ll[0] = -np.inf                                                 # nothing allowed: the row is left alone
        t, min_t = int(rng.randint(9)), int(rng.randint(4))
        state = np.zeros((N, 3), dtype=np.int32)
        state[:, 0], state[:, 1] = t, -1
        dead = rng.rand(N) < 0.2
        dead[1] = True
        state[dead, 2] = 1
        active = np.zeros(3, dtype=np.int32)
        active[t % 3] = 1
        out = _run_truncate(t, k, V, tot, min_t, Tf, cutf, ll, fs, fl, owned, state, active)
        assert (out[:, tot:] == SENTINEL).all(), (T, cut)
        got = out[:, :tot]
        for s in range(N):
            tag = (T, cut, s)
            if dead[s]:
                assert np.array_equal(bits(got[s]), bits(ll[s])), tag
                continue
            allow = allowed_mask(ll[s], V, fs, fl[s // k], owned[s // k], t, min_t)
            keep, amb = np_truncate(ll[s], allow, Tf, *cutf)
            rows += 1
            if amb:
                near += 1
                continue
            checked += 1
            check_row(tag, got[s], ll[s], allow, keep)
            cut_rows += bool((allow & ~keep).any())
    print("MEASURED gtos_truncate_block vs numpy, tot = %d: %d live rows, %d near ties, %d cut" % (tot, rows, near, cut_rows))
    assert checked >= 300 and near <= rows // 200, (rows, checked, near)
    assert cut_rows > 0                                                 # not vacuous (three columns leave little to cut)
    # a launch whose flag is clear changes nothing
    state[:, 2] = 0
    for flags in ((0, 0, 0), (0, 1, 1)):
        active = np.array(flags, dtype=np.int32)
        out = _run_truncate(0, k, V, tot, 0, 1.0, (f32(0.5), f32(0.5), f32(0.01), f32(0.01)), ll, fs, fl, owned, state, active)
        assert np.array_equal(bits(out[:, :tot]), bits(ll)) and (out[:, tot:] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T,cut,top_p", [(1.0, (0.0, 0.8, 0.0, 0.0), 1.0), (0.7, (0.1, 1.0, 0.0, 0.0), 1.0),
                                         (1.5, (0.0, 1.0, 0.0, 0.05), 0.9)])
def test_truncated_draws_follow_the_renormalised_softmax(T, cut, top_p):
    """The fixed 40-column row of test_sample_step_draws_the_tempered_distribution in 4096 slots over 50 steps (no <END>), every step
    truncate_block then sample_step on a fresh copy of the row: 204,800 draws against softmax(ll / T) on the numpy kept set."""
    from torch.special import gammaincc
    from gtos_amd import ops
    rng = np.random.RandomState(40)
    B, k, max_t, tot, C = 64, 64, 50, 40, 2
    N = B * k
    V = tot
    Tf, pf, cutf = f32(T), f32(top_p), tuple(f32(v) for v in cut)
    row = (rng.randn(tot) * 1.2).astype(np.float32)
    row[7] = row[8]                                                     # a tie
    row = (row - np.log(np.exp(row.astype(np.float64)).sum())).astype(np.float32)
    fs = np.zeros(V, dtype=np.uint8)
    fs[1] = UNK_
    none = np.zeros(0, np.uint8)
    allow = allowed_mask(row, V, fs, none, none, 0, 0)
    keep, amb = np_truncate(row, allow, Tf, *cutf)
    assert not amb and 1 < keep.sum() < allow.sum()                     # the fixed row: a real cut, no decision on an edge
    cut_row = np.where(keep | ~allow, row, -np.inf).astype(np.float32)
    kept, v, amb = np_kept(cut_row, allowed_mask(cut_row, V, fs, none, none, 0, 0), Tf, 0, pf)
    assert not amb and set(kept) <= set(np.nonzero(keep)[0]) and (top_p == 1.0 or kept.size < keep.sum())
    dev = torch.device("cuda:0")
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)     # noqa: E731
    g_row, g_fs = D(np.broadcast_to(row, (N, tot)).copy()), D(fs)
    g_ll = torch.empty_like(g_row)
    state = np.zeros((N, 3), dtype=np.int32)
    state[:, 1] = -1
    g = [D(np.zeros(N)), D(state), D(np.full((max_t, N), -1, dtype=np.int32)), D(np.array([1, 0, 0], dtype=np.int32))]
    tok_shared, char_shared, dead_char = D(np.zeros(V, np.int64)), D(np.zeros((V, C), np.int64)), D(np.zeros(C, np.int64))
    tok_out = torch.empty(N, dtype=torch.int64, device=dev)
    char_out = torch.empty((N, C), dtype=torch.int64, device=dev)
    for t in range(max_t):
        g_ll.copy_(g_row)
        ops.truncate_block(t, k, V, tot, 0, Tf, *cutf, g_ll, g_fs, None, None, g[1], g[3])
        ops.sample_step(t, k, V, tot, 0, max_t, Tf, 0, pf, 123456789, g_ll, g_fs, None, None, *g, tok_shared, None, char_shared, None, 0,
                        dead_char, tok_out, char_out)
    assert np.array_equal(bits(g_ll[0].cpu().numpy()), bits(cut_row))
    drawn = g[2].cpu().numpy().ravel()
    assert (drawn >= 0).all() and drawn.size == N * max_t
    counts = np.bincount(drawn, minlength=tot)
    outside = np.setdiff1d(np.arange(tot), kept)
    assert counts[outside].sum() == 0, (outside, counts[outside])
    p = np.exp(v.astype(np.float64) / Tf - (v.astype(np.float64) / Tf).max())
    p /= p.sum()
    expect = p * drawn.size
    chi2 = float(((counts[kept] - expect) ** 2 / expect).sum())
    df = kept.size - 1
    assert df >= 1
    pval = float(gammaincc(torch.tensor(df / 2.0, dtype=torch.float64), torch.tensor(chi2 / 2.0, dtype=torch.float64)))
    print("MEASURED T=%g cut=%r top_p=%g: %d of %d allowed columns kept, chi2 %.2f on %d df, p = %.3g" % (
        T, cut, top_p, kept.size, int(allow.sum()), chi2, df, pval))
    assert pval > 1e-6, (chi2, df, pval)


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
def test_truncated_sampling_end_to_end_fp32(monkeypatch):
    """C1 fp32, 4 samples, 12 steps, typical_p = 0.9 and min_p = 0.02: seeds, sync_every, every draw re-scored by a teacher-forced
    host loop against the numpy statement (np_truncate, then the sampler's np_select on what is left: the drawn token lies in the kept
    set because it IS the restatement's draw), min_p = 1 against greedy, and the bans in front of the cuts."""
    from test_device_beam_search import _synth_model
    from test_sample_decode import _capture_memory, _fresh, _host_decode, _ids_of, _samples
    from test_avoid_block import most_seen_and_first_bigram, holds_entry
    from gtos_amd import search
    from gtos_amd.vocab import END
    model, batch = _synth_model("C1", torch.float32)
    memory = _capture_memory(model, batch, monkeypatch)
    B = len(memory['local_idx2token'])
    k, max_t, min_t = 4, 12, 3
    cuts = dict(typical_p=0.9, min_p=0.02)
    key = lambda beams: [(b.steps, _samples(b)) for b in beams]        # noqa: E731
    work = lambda seed, **kw: model.work(batch, k, max_t, min_t, search="sample", seed=seed, **kw)      # noqa: E731
    a = work(5, **cuts)
    assert key(a) == key(work(5, **cuts)) and key(a) != key(work(6, **cuts))
    assert key(a) != key(work(5))                                       # the cuts changed the draw
    for sync in (1, 8):
        beams = search.sample_device(model, memory, _fresh(B, k, max_t, min_t), 1.0, 0, 1.0, 5, sync_every=sync, **cuts)
        assert key(beams) == key(a), sync
    # draw by draw against the restatement
    near, removed, rows = set(), [0], [0]

    def choose(s, t, row, allow):
        b, j = divmod(s, k)
        keep, amb = np_truncate(row, allow, 1.0, f32(0.02), f32(0.9), 0.0, 0.0)
        rows[0] += 1
        removed[0] += int((allow & ~keep).sum())
        w, tie = np_select(np.where(keep, row, -np.inf).astype(np.float32), keep, 1.0, 0, 1.0, 5, b, j, t)
        if amb or tie:
            near.add(s)
        return None if w < 0 else w
    seqs, scores = _host_decode(model, memory, k, max_t, min_t, choose)
    assert removed[0] > rows[0]                                         # not vacuous: more than a column a row went
    compared = 0
    for b, beam in enumerate(a):
        if any(b * k + j in near for j in range(k)):
            continue
        got = sorted((_ids_of(model, memory, b, seq), score) for seq, score in _samples(beam))
        want = sorted((seqs[b * k + j], scores[b * k + j]) for j in range(k))
        assert [g[0] for g in got] == [w[0] for w in want], b
        for (_, x), (_, y) in zip(got, want):
            assert abs(x - y) <= 1e-4 * max(1.0, abs(y)), (b, x, y)
        compared += 1
    print("MEASURED truncated sampling: %d of %d graphs compared draw by draw, %d slots with a near tie, %.1f of the allowed columns "
          "removed per row" % (compared, B, len(near), removed[0] / max(1, rows[0])))
    assert compared >= (B + 1) // 2
    # min_p = 1 keeps the columns at the maximum: greedy, unless a row has an exact tie there
    tied = set()

    def greedy(s, t, row, allow):
        best = np.where(allow, row, -np.inf)
        if (best == best.max()).sum() > 1:
            tied.add(s // k)
        return int(np.argmax(best))
    seqs, scores = _host_decode(model, memory, k, max_t, min_t, greedy)
    one, top1 = work(11, min_p=1.0), work(11, top_k=1)
    for b in range(B):
        if b in tied:
            continue
        assert key([one[b]]) == key([top1[b]]), b
        got = {tuple(_ids_of(model, memory, b, seq)): score for seq, score in _samples(one[b])}
        assert set(got) == {tuple(seqs[b * k])} and got[tuple(seqs[b * k])] == scores[b * k], b
    assert len(tied) < B
    # the bans act before the cuts
    avoid = [most_seen_and_first_bigram(_samples(beam)[0][0]) for beam in a]
    assert any(avoid)
    beams = work(5, no_repeat_ngram=2, avoid=avoid, **cuts)
    for b, beam in enumerate(beams):
        hyps = beam.completed_hypotheses + beam.hypotheses
        assert len(hyps) == k
        for h in hyps:
            assert not holds_entry(h.seq, avoid[b]), (b, h.seq, avoid[b])
            y = [w for w in h.seq[1:] if w != END]
            assert len(set(zip(y, y[1:]))) == max(len(y) - 1, 0), h.seq
