"""Coverage-penalised beam search (Generator.work(..., coverage_penalty=beta), Generator.coverage, gtos_amd.search.CoverageBeam,
csrc/coverage.hip, csrc/coverage_kernels.h).

CPU: the rule header compiled with g++ is driven through random multi-step searches next to the Python statement of the rule
(CoverageBeam.advance, fed the same candidate lists and the same random penalty per live slot): parents, sequences, fp64 scores,
recorded penalties, completion order, the state words and the continue flag must agree exactly; beta = 0 gives the tables of
gtos_beam::advance_serial; a large beta hands the whole cut to the best-covered parent; get_k_best; the argument checks; the launch
plan under the dry run.
GPU: gtos_coverage_step against a torch statement (bitwise coverage, bounded penalty, reproducible across slots and batches, guard
bands), gtos_coverage_advance against the g++ driver (exact, guard bands), work(search="device") against work(search="host"), the
row-sum invariant, and the search's coverage against the teacher-forced Generator.coverage on the golden beam models."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver, Guarded, GuardedFlat

DRIVER = r"""
#include "coverage_kernels.h"
// what one gtos_coverage_advance launch does to the search tables, serially
extern "C" void coverage_all(int B, int k, double beta, int t, int V, int tot, int min_t, int max_t, const float* topv, const int* topi,
                             const uint8_t* fs, const uint8_t* fl, double* slot_score, int* state, int* bp_parent, int* bp_token,
                             int* comp_step, int* comp_parent, double* comp_score, int* active, const double* cp, double* slot_cp,
                             double* comp_cp) {
    using namespace gtos_coverage;
    static double ps[MAX_K * MAX_K], pk[MAX_K * MAX_K];
    static int pt[MAX_K * MAX_K], order[MAX_K];
    static uint8_t pf[MAX_K * MAX_K];
    const long N = (long)B * k;
    active[active_clear(t)] = 0;
    if (!active[active_read(t)]) return;
    for (int b = 0; b < B; ++b)
        if (advance_serial(b, k, beta, t, V, tot, min_t, max_t, topv, topi, fs, fl, slot_score, state, bp_parent + t * N, bp_token + t * N,
                           comp_step, comp_parent, comp_score, cp, slot_cp, comp_cp, ps, pk, pt, pf, order))
            active[active_set(t)] |= 1;
}
// ... and one gtos_beam_advance launch (csrc/beam_kernels.h), for the beta = 0 identity
extern "C" void plain_all(int B, int k, int t, int V, int tot, int min_t, int max_t, const float* topv, const int* topi,
                          const uint8_t* fs, const uint8_t* fl, double* slot_score, int* state, int* bp_parent, int* bp_token,
                          int* comp_step, int* comp_parent, double* comp_score, int* active) {
    using namespace gtos_beam;
    static double ps[MAX_K * MAX_K];
    static int pt[MAX_K * MAX_K], order[MAX_K];
    static uint8_t pf[MAX_K * MAX_K];
    const long N = (long)B * k;
    active[active_clear(t)] = 0;
    if (!active[active_read(t)]) return;
    for (int b = 0; b < B; ++b)
        if (advance_serial(b, k, t, V, tot, min_t, max_t, topv, topi, fs, fl, slot_score, state, bp_parent + t * N, bp_token + t * N,
                           comp_step, comp_parent, comp_score, ps, pt, pf, order))
            active[active_set(t)] |= 1;
}
extern "C" int beta_fine(double beta) { return gtos_coverage::beta_ok(beta); }
extern "C" double term(float cov) { return (double)gtos_coverage::cp_term(cov); }
"""

PAD, UNK, STR, END = "<PAD>", "<UNK>", "<STR>", "<END>"
KS = [4, 6, 8, 32]
BETAS = [0.0, 0.2, 1e4]
B, V, N_LOCAL, MAX_T = 3, 40, 6, 12


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = compile_host_driver(tmp_path_factory, "coverage_host", DRIVER)
    lib.coverage_all.argtypes = [ctypes.c_int] * 2 + [ctypes.c_double] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 15
    lib.coverage_all.restype = None
    lib.plain_all.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 12
    lib.plain_all.restype = None
    lib.beta_fine.argtypes = [ctypes.c_double]
    lib.term.argtypes = [ctypes.c_float]
    lib.term.restype = ctypes.c_double
    return lib


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


class Tables(object):
    """The tables of a covered device search as numpy arrays: the plain search's, then slot_cp / comp_cp; with n also the coverage
    tables of the kernel (cov_cur is an input of a step, like cp)."""

    def __init__(self, B, k, max_t, n=0):
        from test_device_beam_search import Tables as Plain
        self.plain = Plain(B, k, max_t)
        self.B, self.k, self.N, self.max_t, self.n = B, k, B * k, max_t, n
        self.slot_cp = np.zeros(B * k, dtype=np.float64)
        self.comp_cp = np.zeros((B, k), dtype=np.float64)
        self.comp_cov = np.zeros((B, k, max(n, 1)), dtype=np.float32)
        self.slot_cov = np.zeros((B * k, max(n, 1)), dtype=np.float32)

    def __getattr__(self, name):
        return getattr(self.plain, name)

    def arrays(self):
        return self.plain.arrays() + [self.slot_cp, self.comp_cp] + ([self.comp_cov, self.slot_cov] if self.n else [])

    def names(self):
        return ["slot_score", "state", "bp_parent", "bp_token", "comp_step", "comp_parent", "comp_score", "active", "slot_cp", "comp_cp",
                "comp_cov", "slot_cov"]

    def beams(self, strings, min_t):
        return self.plain.beams(strings, min_t)


def host_step(lib):
    def step(tab, beta, t, V_, tot, min_t, topv, topi, fs, fl, cp, cov=None):
        lib.coverage_all(tab.B, tab.k, beta, t, V_, tot, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(fs), _np_ptr(fl),
                         *[_np_ptr(a) for a in tab.plain.arrays()], _np_ptr(cp), _np_ptr(tab.slot_cp), _np_ptr(tab.comp_cp))
    return step


def plain_step(lib):
    def step(tab, beta, t, V_, tot, min_t, topv, topi, fs, fl, cp, cov=None):
        lib.plain_all(tab.B, tab.k, t, V_, tot, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(fs), _np_ptr(fl),
                      *[_np_ptr(a) for a in tab.arrays()])
    return step


def gpu_step(tab, beta, t, V_, tot, min_t, topv, topi, fs, fl, cp, cov):
    """The same step on the device kernel: tables up (each inside guard bands), one gtos_coverage_advance, tables down."""
    from gtos_amd import ops
    from test_diverse_beam import Banded
    dev = torch.device("cuda:0")
    D = lambda a: torch.from_numpy(a).to(dev)
    g = [Banded(a, dev) for a in tab.arrays()]
    p, (slot_cp, comp_cp, comp_cov, slot_cov) = [x.view for x in g[:8]], [x.view for x in g[8:]]
    ops.coverage_advance(t, tab.k, beta, V_, tot, min_t, tab.max_t, D(topv), D(topi), D(fs), D(fl) if fl.size else None, *p[:7], D(cp),
                         D(cov), slot_cp, comp_cp, comp_cov, slot_cov, p[7])
    for a, x, name in zip(tab.arrays(), g, tab.names()):
        x.check("gtos_coverage_advance %s, step %d" % (name, t))
        a[...] = x.view.cpu().numpy()


def random_search(rng, step_fn, k, beta, min_t, twin=None, n=0):
    """One multi-step covered search of B graphs: the Python rule (search.CoverageBeam) and step_fn (the fixed-slot tables) fed the
    same candidate lists and the same penalty per live slot.  Every token class occurs (<UNK> as a vocabulary id, <END> as a vocabulary
    id and as copy strings, <END> before min_t), values lie on a coarse grid so that ties occur -- of scores and, the penalties lying on
    a grid as well, of keys -- and some are -inf.
    beta = 1e4: the live slots' penalties are at least 1 apart, log-likelihoods stay in [-20, 0] (steps of at most 1.5, 12 steps) and
    the best-covered parent offers k finite candidates that are not <UNK>: every survivor of the cut must descend from it.
    ``twin`` = (step function, tables): a second implementation fed the same steps whose (plain) tables must stay equal.
    ``n`` > 0: random coverage rows [N, n] go in as well, and the rows recorded must be the parents'.
    Returns the number of beam advances compared."""
    from gtos_amd.search import CoverageBeam
    large = beta == 1e4
    tot = V + N_LOCAL
    words = [PAD, UNK, END] + ["w%d" % i for i in range(V - 3)]
    strings = [words + [END if rng.rand() < 0.3 else "c%d" % j for j in range(N_LOCAL)] for _ in range(B)]
    cls = lambda w: 1 if w == UNK else 2 if w == END else 0
    fs = np.array([cls(w) for w in words], dtype=np.uint8)
    fl = np.array([[cls(w) for w in s[V:]] for s in strings], dtype=np.uint8).reshape(B, N_LOCAL)
    tab = Tables(B, k, MAX_T, n)
    beams = [CoverageBeam(k, min_t, MAX_T, beta) for _ in range(B)]
    n_adv, t = 0, 0
    while True:
        got = tab.beams(strings, min_t)
        for b, (g, w) in enumerate(zip(got, beams)):
            assert g.steps == w.steps and g.completed() == w.completed(), (t, b)
            assert [(h.seq, h.score) for h in g.hypotheses] == [(h.seq, h.score) for h in w.hypotheses], (t, b)
            assert [(h.seq, h.score) for h in g.completed_hypotheses] == [(h.seq, h.score) for h in w.completed_hypotheses], (t, b)
            assert tab.slot_cp[b * k:b * k + len(w.hypotheses)].tolist() == [h.cp for h in w.hypotheses] or t == 0, (t, b)
            assert tab.comp_cp[b, :len(w.completed_hypotheses)].tolist() == [h.cp for h in w.completed_hypotheses], (t, b)
        if all(beam.completed() or not beam.hypotheses for beam in beams):
            break
        assert t < MAX_T
        cp = -0.25 * rng.randint(0, 8, size=B * k).astype(np.float64)
        best = [0] * B
        if large:
            for b in range(B):
                cp[b * k:(b + 1) * k] = -1.5 * rng.permutation(k) - rng.rand(k) * 0.25
                nl = len(beams[b].hypotheses)
                best[b] = int(np.argmax(cp[b * k:b * k + nl])) if nl else 0
        cov = rng.rand(B * k, n).astype(np.float32) * 2 if n else None
        topv = np.full((B * k, k), np.nan, dtype=np.float32)
        topi = np.zeros((B * k, k), dtype=np.int32)
        for s in range(B * k):
            if large and s % k == best[s // k]:
                ok = [i for i, w in enumerate(strings[s // k]) if w not in (UNK, PAD)]
                ids = rng.choice(ok, size=k, replace=False)
                vals = rng.choice([-0.5, -1.0, -1.5], size=k).astype(np.float32)
            else:
                ids = rng.choice(tot, size=k, replace=False)
                grid = [-0.5, -1.0, -1.5, -0.25, -0.75, -np.inf] if large else [-0.5, -1.0, -1.5, -2.0, -3.0, -np.inf]
                vals = rng.choice(grid, size=k, p=[.25, .25, .2, .15, .1, .05]).astype(np.float32)
                if rng.rand() < 0.5 and not large:
                    vals = (vals + rng.randn(k).astype(np.float32) * 0.01).astype(np.float32)
            order = np.lexsort((ids, -vals.astype(np.float64)))       # descending value, lower id first
            topv[s], topi[s] = vals[order], ids[order]
        was = [(beam.completed(), len(beam.hypotheses), len(beam.completed_hypotheses)) for beam in beams]
        parents = [None] * B
        for b, beam in enumerate(beams):
            if beam.completed():
                continue
            nl = len(beam.hypotheses)
            rows = [[(strings[b][int(i)], float(v)) for v, i in zip(topv[s], topi[s])] for s in range(b * k, b * k + nl)]
            parents[b] = beam.advance(rows, cp[b * k:b * k + nl].tolist(), [[b * k + j] for j in range(nl)])
        step_fn(tab, beta, t, V, tot, min_t, topv, topi, fs, fl, cp, cov)
        if twin:
            twin[0](twin[1], beta, t, V, tot, min_t, topv, topi, fs, fl, cp, cov)
            for a, a2 in zip(tab.plain.arrays(), twin[1].arrays()[:8]):
                assert np.array_equal(a.ravel(), a2.ravel(), equal_nan=True), ("twin tables", t)
            if len(twin[1].arrays()) > 8:
                assert np.array_equal(tab.slot_cp, twin[1].slot_cp) and np.array_equal(tab.comp_cp, twin[1].comp_cp), ("twin cp", t)
        go = False
        for b, beam in enumerate(beams):
            par = parents[b]
            if par is None:
                assert (tab.bp_parent[t, b * k:(b + 1) * k] == -1).all(), ("a done beam's row", t, b)
                continue
            n_adv += 1
            assert tab.state[b].tolist() == [beam.steps, len(beam.completed_hypotheses), len(beam.hypotheses), int(beam.completed())], (t, b)
            assert [int(p) - b * k for p in tab.bp_parent[t, b * k:b * k + len(par)]] == list(par), ("parents", t, b)
            assert (tab.bp_parent[t, b * k + len(par):(b + 1) * k] == -1).all(), ("dead slots", t, b)
            assert [strings[b][int(i)] for i in tab.bp_token[t, b * k:b * k + len(par)]] == [h.seq[-1] for h in beam.hypotheses]
            assert tab.slot_cp[b * k:b * k + len(par)].tolist() == [h.cp for h in beam.hypotheses] == [cp[b * k + p] for p in par], (t, b)
            new = range(was[b][2], len(beam.completed_hypotheses))
            assert [tab.comp_cp[b, j] for j in new] == [beam.completed_hypotheses[j].cp for j in new], (t, b)
            assert [int(tab.comp_parent[b, j]) for j in new] == [beam.completed_hypotheses[j].coverage[0] for j in new], (t, b)
            assert [[b * k + p] for p in par] == [h.coverage for h in beam.hypotheses]
            if n:
                for j in new:
                    assert np.array_equal(tab.comp_cov[b, j], cov[tab.comp_parent[b, j]]), ("comp_cov", t, b, j)
                for j, p in enumerate(par):
                    assert np.array_equal(tab.slot_cov[b * k + j], cov[b * k + p]), ("slot_cov", t, b, j)
            if large and was[b][1]:
                assert all(p == best[b] for p in par), ("large beta: a survivor of another parent", t, b, par, best[b])
                assert all(int(tab.comp_parent[b, j]) == b * k + best[b] for j in new), ("large beta: completions", t, b)
                assert all(-20.0 <= h.score <= 0.0 for h in beam.hypotheses + beam.completed_hypotheses), "scores are plain sums"
            go |= not beam.completed() and len(beam.hypotheses) > 0
        assert int(tab.active[(t + 1) % 3]) == int(go) and int(tab.active[(t + 2) % 3]) == 0, ("continue flag", t)
        t += 1
    snap = [a.copy() for a in tab.arrays() if a is not tab.plain.active]
    for t2 in range(t, MAX_T):                               # the device loop keeps launching steps up to max_t: they change nothing
        step_fn(tab, beta, t2, V, tot, min_t, np.zeros((B * k, k), np.float32), np.zeros((B * k, k), np.int32), fs, fl,
                np.zeros(B * k), np.zeros((B * k, n), np.float32) if n else None)
    for a, b_ in zip([a for a in tab.arrays() if a is not tab.plain.active], snap):
        assert np.array_equal(a, b_, equal_nan=True), "a step after the end changed the tables"
    return n_adv


# ------------------------------------------------------------------------------------------------ CPU: the header
@pytest.mark.parametrize("k", KS)
def test_rule_header_matches_the_python_rule(host_lib, k):
    step = host_step(host_lib)
    n = 0
    for li, beta in enumerate(BETAS):
        rng = np.random.RandomState(20261019 + 1000 * k + li)
        for rep in range(4):
            n += random_search(rng, step, k, beta, min_t=rep % 4)
    assert n >= 36, n
    assert [host_lib.beta_fine(x) for x in (0.0, 0.2, 1e4, -1e-300, float("inf"), float("nan"))] == [1, 1, 1, 0, 0, 0]


def test_without_penalty_the_tables_are_the_plain_search(host_lib):
    """beta = 0: the tables of gtos_coverage::advance_serial equal those of gtos_beam::advance_serial bit for bit, step by step."""
    from test_device_beam_search import Tables as PlainTables
    for k in (8, 6, 32):
        rng = np.random.RandomState(77 + 10 * k)
        for min_t in (0, 2):
            assert random_search(rng, host_step(host_lib), k, 0.0, min_t, twin=(plain_step(host_lib), PlainTables(B, k, MAX_T))) > 0


@pytest.mark.parametrize("k", KS)
def test_a_large_penalty_hands_the_cut_to_the_best_covered_parent(host_lib, k):
    """(the assertions sit in random_search, at every step of a beta = 1e4 search)"""
    rng = np.random.RandomState(99 + 100 * k)
    for min_t in (0, 2):
        assert random_search(rng, host_step(host_lib), k, 1e4, min_t) > 0


def test_the_penalty_term(host_lib):
    """A saturated node contributes exactly 0; an untouched one the floor's logarithm; the term is an fp32 logf."""
    assert host_lib.term(1.0) == 0.0 and host_lib.term(1.5) == 0.0 and host_lib.term(37.0) == 0.0
    assert abs(host_lib.term(0.0) - math.log(1e-12)) < 1e-5 and abs(host_lib.term(0.5) - math.log(0.5)) < 1e-7
    assert host_lib.term(0.25) == float(np.float32(host_lib.term(0.25)))


def test_get_k_best_ranks_by_the_gnmt_score():
    from gtos_amd.search import CoverageBeam, CoveredHypothesis
    rng = np.random.RandomState(5)
    for beta in BETAS:
        for alpha in (0.0, 0.6, 1.0):
            beam = CoverageBeam(8, 1, 20, beta)
            hyps = [CoveredHypothesis([STR] + ["w"] * int(rng.randint(1, 9)) + [END], -float(rng.randint(1, 30)) / 4,
                                      -float(rng.randint(0, 12)) / 4, []) for _ in range(8)]
            beam.completed_hypotheses = list(hyps)
            want = sorted(hyps, key=lambda h: h.score / (1 + len(h.seq)) ** alpha + beta * h.cp, reverse=True)
            assert [id(h) for h in beam.get_k_best(5, alpha)] == [id(h) for h in want[:5]]
            live = CoverageBeam(8, 1, 20, beta)             # nothing completed: the live hypotheses
            live.hypotheses = [CoveredHypothesis(h.seq[:-1], h.score, h.cp, []) for h in hyps]
            want = sorted(live.hypotheses, key=lambda h: h.score / (1 + len(h.seq)) ** alpha + beta * h.cp, reverse=True)
            assert [id(h) for h in live.get_k_best(8, alpha)] == [id(h) for h in want]
    beam = CoverageBeam(2, 0, 5, 2.0)                        # the penalty steers, the score stays the log-likelihood
    assert beam.advance([[("a", -1.0), ("b", -2.0)]], [-3.0], [[0.5]]) == [0, 0]
    assert [(h.seq, h.score, h.cp, h.coverage) for h in beam.hypotheses] == [([STR, "a"], -1.0, -3.0, [0.5]), ([STR, "b"], -2.0, -3.0, [0.5])]
    assert beam.advance([[("c", -1.0), ("d", -1.5)], [("e", -0.25), ("f", -9.0)]], [-4.0, -1.0], [[1.], [2.]]) == [1, 0]
    assert [(h.seq[-1], h.score, h.cp, h.coverage) for h in beam.hypotheses] == [("e", -2.25, -1.0, [2.]), ("c", -2.0, -4.0, [1.])]


# ------------------------------------------------------------------------------------------------ CPU: argument checks
def test_work_checks_the_coverage_penalty():
    """No model needed: the checks run before anything is touched."""
    from gtos_amd.generator import Generator, check_coverage
    for search in ("host", "device"):
        for bad in (True, False, "0.2", 1j, [0.2], -0.1, float("inf"), float("-inf"), float("nan")):
            with pytest.raises(ValueError):
                Generator.work(None, {}, 4, 10, search=search, coverage_penalty=bad)
        with pytest.raises(ValueError):
            Generator.work(None, {}, 4, 10, search=search, coverage_penalty=0.2, groups=2)
        with pytest.raises(ValueError):
            Generator.work(None, {}, 4, 10, search=search, coverage_penalty=0.2, constraints=[["w1"]])
    with pytest.raises(ValueError):
        Generator.work(None, {}, 4, 10, search="sample", seed=1, coverage_penalty=0.2)
    assert check_coverage(None, "sample", 2, [[]]) is None
    assert check_coverage(0, "host", 1, None) == 0.0 and check_coverage(0.2, "device", 1, None) == 0.2
    assert isinstance(check_coverage(1, "host", 1, None), float)


def test_coverage_entry_points_refuse_bad_arguments():
    """-10 outside the shapes, -23 for null pointers; nothing launched, no device needed."""
    from gtos_amd import _lib
    lib = _lib.load()
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(32)

    def stp(N=8, k=4, t=0, n=5, ptrs=None):
        return lib.gtos_coverage_step(N, k, t, n, *(ptrs or [p, p, p, p, q, p, p]), None)
    assert stp(N=9) == -10 and stp(k=0) == -10 and stp(t=-1) == -10 and stp(n=0) == -10
    assert stp(ptrs=[p] * 7) == -10                          # the two coverage buffers alternate
    for i in (0, 1, 3, 4, 5, 6):
        ptrs = [p, p, p, p, q, p, p]
        ptrs[i] = None
        assert stp(ptrs=ptrs) == -23, i
    assert stp(N=0, k=0) == 0

    def adv(B_=2, k=4, t=0, V_=10, tot=10, max_t=5, beta=0.2, n=5, ptrs=None):
        return lib.gtos_coverage_advance(B_, k, t, V_, tot, 0, max_t, _bits(beta), n, *(ptrs or [p] * 18), None)
    assert adv(k=33) == -10 and adv(k=0) == -10 and adv(t=5) == -10 and adv(t=-1) == -10 and adv(tot=9) == -10 and adv(n=0) == -10
    assert adv(beta=-0.5) == -10 and adv(beta=float("inf")) == -10 and adv(beta=float("nan")) == -10
    for i in range(18):
        ptrs = [p] * 18
        ptrs[i] = None
        assert adv(ptrs=ptrs, tot=12) == -23, i
    assert adv(B_=0, k=99) == 0


def test_ops_check_shapes_under_the_dry_run():
    from dryrun import DryRun
    from gtos_amd import ops
    from gtos_amd._lib import GtosHipError
    with DryRun() as rec:
        B_, k, max_t, V_, tot, n = 2, 6, 5, 10, 13, 7
        N = B_ * k
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
        f32 = lambda *s: torch.zeros(*s, dtype=torch.float32)
        pad = torch.zeros(n, N, dtype=torch.bool)
        cov = [f32(N, n), f32(N, n)]
        ops.coverage_step(1, k, f32(N, n), pad, i32(N), cov[0], cov[1], f64(N), i32(3))
        ops.coverage_step(0, k, f32(N, n), pad.to(torch.uint8), None, cov[1], cov[0], f64(N), i32(3))
        for bad in (f64(N, n), f32(N, n).t(), f32(N), f32(N, 0)):
            with pytest.raises(GtosHipError):
                ops.coverage_step(1, k, bad, pad, i32(N), cov[0], cov[1], f64(N), i32(3))
        with pytest.raises(AssertionError):
            ops.coverage_step(1, k, f32(N, n), pad, i32(N), cov[0], cov[0], f64(N), i32(3))
        with pytest.raises(AssertionError):
            ops.coverage_step(1, k, f32(N, n), pad.t(), i32(N), cov[0], cov[1], f64(N), i32(3))
        with pytest.raises(AssertionError):
            ops.coverage_step(1, k, f32(N, n), pad, i32(N).long(), cov[0], cov[1], f64(N), i32(3))
        with pytest.raises(AssertionError):
            ops.coverage_step(1, k, f32(N, n), pad, i32(N), cov[0], cov[1], f32(N), i32(3))
        with pytest.raises(AssertionError):
            ops.coverage_step(1, 5, f32(N, n), pad, i32(N), cov[0], cov[1], f64(N), i32(3))
        tabs = [f64(N), i32(B_, 4), i32(max_t, N), i32(max_t, N), i32(B_, k), i32(B_, k), f64(B_, k)]
        flags = [torch.zeros(V_, dtype=torch.uint8), torch.zeros(B_, tot - V_, dtype=torch.uint8)]
        more = [f64(N), cov[0], f64(N), f64(B_, k), f32(B_, k, n), f32(N, n), i32(3)]
        ops.coverage_advance(1, k, 0.2, V_, tot, 0, max_t, f32(N, k), i32(N, k), *flags, *tabs, *more)
        for i, bad in ((0, f32(N)), (1, f32(N, n).double()), (3, f64(B_, k + 1)), (4, f32(B_, k, n + 1)), (5, f32(N, n + 1))):
            with pytest.raises(AssertionError):
                ops.coverage_advance(1, k, 0.2, V_, tot, 0, max_t, f32(N, k), i32(N, k), *flags, *tabs, *more[:i], bad, *more[i + 1:])
        for bad in (-0.2, float("inf"), float("nan"), 1):
            with pytest.raises(AssertionError):
                ops.coverage_advance(1, k, bad, V_, tot, 0, max_t, f32(N, k), i32(N, k), *flags, *tabs, *more)
    assert rec.names() == ["gtos_coverage_step", "gtos_coverage_step", "gtos_coverage_advance"]
    assert rec.calls[0][1][:4] == (N, k, 1, n) and rec.calls[1][1][6] is None
    assert rec.calls[2][1][:9] == (B_, k, 1, V_, tot, 0, max_t, _bits(0.2), n)


# ------------------------------------------------------------------------------------------------ CPU: launch plans
def test_covered_device_search_launch_plan():
    from dryrun import DryRun
    from gtos_amd import synth
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.search import CoverageBeam
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
        n_graphs, n = batch['concept'].shape[1], batch['concept'].shape[0] - 1

        def plan(**kw):
            n0 = len(rec.calls)
            beams = model.work(batch, k, steps, search="device", **kw)
            assert len(beams) == n_graphs
            return beams, rec.calls[n0:]
        names = [c[0] for c in plan()[1]]
        assert not [x for x in names if x.startswith("gtos_coverage")]
        assert [c[0] for c in plan(coverage_penalty=None)[1]] == names                         # None: the plan of today
        search = ("gtos_ngram_block", "gtos_coverage_step", "gtos_beam_topk", "gtos_coverage_advance", "gtos_beam_reorder")
        for ngram in (0, 3):
            beams, calls = plan(coverage_penalty=0.2, no_repeat_ngram=ngram)
            got = [c[0] for c in calls]
            per_step = []
            for t in range(steps):
                per_step += [x for x in search if x != "gtos_ngram_block" or (ngram and t)]
            assert [x for x in got if x in search] == per_step
            assert "gtos_beam_advance" not in got
            first = [i for i, x in enumerate(got) if x == "gtos_coverage_step"]
            for t, i in enumerate(first):                    # straight after the decoder (and the n-gram kernel)
                assert got[i - 1] == ("gtos_ngram_block" if ngram and t else "gtos_copy_ll_fwd"), (t, got[i - 1])
            # the decoder's own launches are those of the plain search
            swap = {"gtos_coverage_advance": "gtos_beam_advance"}
            plain = [c[0] for c in plan(no_repeat_ngram=ngram)[1]]
            assert [swap.get(x, x) for x in got if x != "gtos_coverage_step"] == plain
            stp = [c[1] for c in calls if c[0] == "gtos_coverage_step"]
            assert [a[:4] for a in stp] == [(n_graphs * k, k, t, n) for t in range(steps)]
            assert stp[0][6] is None and all(a[6] is not None for a in stp[1:])
            assert all(a[7] != a[8] for a in stp) and all(x[8] == y[7] for x, y in zip(stp, stp[1:]))     # the buffers alternate
            adv = [c[1] for c in calls if c[0] == "gtos_coverage_advance"]
            assert [(a[0], a[1], a[2], a[7], a[8]) for a in adv] == [(n_graphs, k, t, _bits(0.2), n) for t in range(steps)]
            assert all(isinstance(b_, CoverageBeam) and b_.beta == 0.2 for b_ in beams)
        beams, calls = plan(coverage_penalty=0.0)
        assert [c[1][7] for c in calls if c[0] == "gtos_coverage_advance"] == [_bits(0.0)] * steps
        # the host search: the same step kernel, a hypothesis its own parent
        n0 = len(rec.calls)
        model.work(batch, k, 2, search="host", coverage_penalty=0.2)
        host = [c for c in rec.calls[n0:] if c[0].startswith("gtos_coverage")]
        assert [c[0] for c in host] == ["gtos_coverage_step"] * len(host) and host and all(c[1][6] is None and c[1][1] == 1 for c in host)
        # Generator.coverage: one launch on a zero coverage
        n0 = len(rec.calls)
        out = model.coverage(batch)
        cov_calls = [c for c in rec.calls[n0:] if c[0].startswith("gtos_coverage")]
        assert [c[0] for c in cov_calls] == ["gtos_coverage_step"] and cov_calls[0][1][:4] == (n_graphs, 1, 0, n)
        assert out.coverage.shape == (n_graphs, n) and out.cp.shape == (n_graphs,) and out.cp.dtype == torch.float64
        assert out.tokens.shape == (n_graphs,) and out.graph_of.tolist() == list(range(n_graphs))


# ------------------------------------------------------------------------------------------------ GPU: the step kernel
F64_BAND = 0x7FF8A5A5A5A5A5A5                                 # a NaN pattern for the fp64 bands


def _step_case(rng, N, k, n, t):
    """Operands of one gtos_coverage_step: t = 0 with no parent row; t >= 1 a permuted parent row with two children of one parent and
    several dead slots.  Padding: every graph another non-trailing pattern, one graph all but one node padded."""
    align = torch.from_numpy(rng.dirichlet(np.ones(n), size=N).astype(np.float32))
    prev = torch.from_numpy((rng.rand(N, n) * rng.choice([0.0, 0.3, 1.2], size=(N, 1))).astype(np.float32))
    pad = torch.from_numpy(rng.rand(n, N // k) < 0.3)
    pad[:, 0] = True
    pad[n // 2, 0] = False                                   # all but one
    if n > 1:
        pad[0, 1], pad[n - 1, 1] = True, False               # not trailing
    pad = pad.repeat_interleave(k, dim=1).contiguous()
    parent = None
    if t:
        parent = torch.from_numpy(rng.permutation(N).astype(np.int32))
        parent[1] = parent[0]
        parent[rng.choice(np.arange(2, N), size=max(1, N // 4), replace=False)] = -1
    return align, pad, parent, prev


def _step_launch(dev, t, k, align, pad, parent, prev, active=None, what="gtos_coverage_step"):
    from gtos_amd import ops
    N, n = align.shape
    cov = Guarded(N, n, torch.float32, dev, lead=8, trail=8)
    cp = GuardedFlat(N, torch.float64, dev, band=F64_BAND)
    cov.view.fill_(-3.0)
    cp.view.fill_(-3.0)
    act = torch.ones(3, dtype=torch.int32) if active is None else active
    ops.coverage_step(t, k, align.to(dev), pad.to(dev), None if parent is None else parent.to(dev), prev.to(dev), cov.view, cp.view,
                      act.to(dev))
    cov.check(what + " cov_cur")
    cp.check(what + " cp")
    return cov.view.cpu(), cp.view.cpu()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 65, 300])
@pytest.mark.parametrize("N,k", [(18, 6), (64, 32)])
def test_coverage_step_kernel(n, N, k):
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1000 * n + N)
    worst = 0.0
    for t in (0, 1, 4):
        align, pad, parent, prev = _step_case(rng, N, k, n, t)
        if t == 0:
            prev.zero_()
        cov, cp = _step_launch(dev, t, k, align, pad, parent, prev)
        live = torch.ones(N, dtype=torch.bool) if parent is None else parent >= 0
        src = prev if parent is None else prev[parent.clamp(min=0).long()]
        want = torch.where(live[:, None], src + align, torch.zeros(()))
        assert torch.equal(cov, want), (t, "cov_cur is not cov_prev[parent] + align bitwise")
        keep = ~pad.t()
        terms = torch.log(want.clamp(max=1.0).double() + 1e-12) * keep
        ref = torch.where(live, terms.sum(1), torch.zeros((), dtype=torch.float64))
        assert bool((cp[~live] == 0).all()) and bool((cov[~live] == 0).all())
        err = (cp - ref).abs()
        bound = keep.sum(1).double() * 2.0 ** -18
        worst = max(worst, float((err / bound.clamp(min=2.0 ** -18)).max()))
        assert bool((err <= bound).all()), (t, float(err.max()), float(bound.min()))
        # the same rows at other slot indices of a batch of another N: the same bits
        take = torch.nonzero(live).flatten()[:5].flip(0)
        N2 = 2 * k if N != 2 * k else 3 * k
        a2, pv2, pd2 = torch.zeros(N2, n), torch.zeros(N2, n), torch.zeros(n, N2, dtype=torch.bool)
        at = [N2 - 1 - 2 * i for i in range(len(take))]
        a2[at], pv2[at], pd2[:, at] = align[take], src[take], pad[:, take]
        _, cp2 = _step_launch(dev, 0, k, a2, pd2, None, pv2)
        assert torch.equal(cp2[at], cp[take]), (t, "the penalty of a row depends on where the row sits")
        # the read flag at 0: nothing is written
        off = torch.ones(3, dtype=torch.int32)
        off[t % 3] = 0
        cov0, cp0 = _step_launch(dev, t, k, align, pad, parent, prev, active=off)
        assert bool((cov0 == -3.0).all()) and bool((cp0 == -3.0).all())
    print("MEASURED gtos_coverage_step n=%d N=%d: max |cp - fp64| / (n_nonpad * 2**-18) = %.3e" % (n, N, worst))


# ------------------------------------------------------------------------------------------------ GPU: the advance kernel
@pytest.mark.gpu
@pytest.mark.parametrize("k", [32, 6, 8])
def test_coverage_advance_kernel_matches_the_header(host_lib, k):
    """The kernel (every table inside guard bands) and the g++ driver over the same random searches: every table equal after every
    step (the twin), both equal to the Python rule, and the coverage rows recorded are the parents'."""
    n = 0
    for li, beta in enumerate(BETAS):
        rng = np.random.RandomState(31 + 1000 * k + li)
        for min_t in (0, 2):
            n += random_search(rng, gpu_step, k, beta, min_t, twin=(host_step(host_lib), Tables(B, k, MAX_T)), n=70 if k != 32 else 300)
    assert n >= 18


# ------------------------------------------------------------------------------------------------ GPU: end to end
def _steps_of(h):
    return len(h.seq) - 1


@pytest.mark.gpu
@pytest.mark.parametrize("k,beta,ngram", [(8, 0.2, 0), (6, 5.0, 0), (8, 0.2, 2)])
def test_covered_device_search_equals_covered_host_search_fp32(k, beta, ngram):
    from test_diverse_beam import synth_c1, _close
    model, batch = synth_c1()
    max_t, min_t = 10, 1
    kw = dict(coverage_penalty=beta, no_repeat_ngram=ngram)
    host = model.work(batch, k, max_t, min_t, **kw)
    dev = model.work(batch, k, max_t, min_t, search="device", **kw)
    pad = batch['concept'][1:].eq(model.vocabs['concept'].padding_idx).cpu()
    n = pad.shape[0]
    worst, compared = 0.0, 0
    for b, (h, d) in enumerate(zip(host, dev)):
        assert h.steps == d.steps and h.beta == d.beta == beta, b
        for hl, dl in ((h.hypotheses, d.hypotheses), (h.completed_hypotheses, d.completed_hypotheses)):
            assert [x.seq for x in hl] == [x.seq for x in dl], b
            for x, y in zip(hl, dl):
                assert _close(x.score, y.score) and _close(x.cp, y.cp), (b, x.seq, x.score, y.score, x.cp, y.cp)
                assert len(x.coverage) == len(y.coverage) == n
                diff = max(abs(p - q) for p, q in zip(x.coverage, y.coverage))
                worst = max(worst, diff)
                assert diff <= 1e-5, (b, x.seq, diff)
                assert all(c == 0 for c, m in zip(y.coverage, pad[:, b].tolist()) if m), "coverage at a padded node"
                # the invariant: every step's row is an fp32 softmax over the graph's nodes
                for z in (x, y):
                    steps = _steps_of(z)
                    assert abs(sum(z.coverage) - steps) <= steps * n * 2.0 ** -23, (b, z.seq, sum(z.coverage), steps)
                compared += 1
        assert [x.seq for x in h.get_k_best(k, 0.6)] == [x.seq for x in d.get_k_best(k, 0.6)], b
    assert compared >= len(dev)
    print("MEASURED k=%d beta=%g ngram=%d: %d hypotheses, max |coverage host - device| %.3e" % (k, beta, ngram, compared, worst))


@pytest.mark.gpu
def test_zero_penalty_is_the_plain_device_search_with_coverage_reported():
    from test_diverse_beam import synth_c1
    model, batch = synth_c1()
    k, max_t, min_t = 8, 10, 1
    plain = model.work(batch, k, max_t, min_t, search="device")
    zero = model.work(batch, k, max_t, min_t, search="device", coverage_penalty=0.0)
    n = batch['concept'].shape[0] - 1
    worst = 0.0
    for b, (p, z) in enumerate(zip(plain, zero)):
        assert p.steps == z.steps, b
        for pl, zl in ((p.hypotheses, z.hypotheses), (p.completed_hypotheses, z.completed_hypotheses)):
            assert [(x.seq, x.score) for x in pl] == [(x.seq, x.score) for x in zl], b
            for x in zl:
                assert x.cp <= 0 and len(x.coverage) == n, (b, x.seq)
                steps = _steps_of(x)
                worst = max(worst, abs(sum(x.coverage) - steps) / (steps * n * 2.0 ** -23))
                assert abs(sum(x.coverage) - steps) <= steps * n * 2.0 ** -23, (b, x.seq, sum(x.coverage), steps)
        assert [x.seq for x in p.get_k_best(k, 0.6)] == [x.seq for x in z.get_k_best(k, 0.6)], b
    print("MEASURED sum(coverage) - steps: worst %.3f of the bound steps * n * 2**-23" % worst)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["beam_smatch", "beam_dep_dev"])
def test_search_coverage_agrees_with_the_teacher_forced_pass(case, tmp_path):
    """Per step the incremental decoder and the full-sequence pass attend alike: the coverage a finished hypothesis of the device
    search carries equals Generator.coverage of its string, per node within 1e-3 (tokens + 1)."""
    from test_score_eval_model import _beam_model
    model, batch, meta, _ = _beam_model(case, tmp_path)
    alpha = meta["cfg"]["alpha"]
    compared, worst = 0, 0.0
    for run in meta["runs"]:
        beams = model.work(batch, run["beam"], run["max_step"], run["min_step"], search="device", coverage_penalty=0.2)
        hyps = [[h for h in beam.get_k_best(run["beam"], alpha) if h.seq[-1] == END] for beam in beams]
        targets = [[list(h.seq[1:-1]) for h in hs] for hs in hyps]
        out = model.coverage(batch, targets)
        cov, cp, tokens, owner = out.coverage.cpu(), out.cp.cpu(), out.tokens.cpu().tolist(), out.graph_of.cpu().tolist()
        flat = [(b, h) for b, hs in enumerate(hyps) for h in hs]
        assert len(flat) == cov.shape[0] == cp.shape[0] and owner == [b for b, _ in flat]
        assert tokens == [len(h.seq) - 1 for _, h in flat]                                      # the tokens and <END>
        for (b, h), row, n_tok in zip(flat, cov, tokens):
            diff = float((torch.tensor(h.coverage, dtype=torch.float64) - row.double()).abs().max())
            worst = max(worst, diff / (n_tok + 1))
            assert diff <= 1e-3 * (n_tok + 1), (b, h.seq, diff)
            compared += 1
    assert compared > 0
    print("MEASURED %s: %d hypotheses, max per-node |coverage search - teacher| / (tokens + 1) = %.3e" % (case, compared, worst))
