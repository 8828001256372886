"""Diverse (group) beam search (Generator.work(..., groups=G, diversity=lambda), gtos_amd.search.GroupBeam, csrc/diverse.hip,
csrc/diverse_kernels.h).

CPU: the rule header compiled with g++ is driven through random multi-step searches next to the Python statement of the rule
(GroupBeam.advance, fed the same candidate lists): parents, sequences, fp64 scores, completion order, per-group counters and the
continue flag must agree exactly; three identities on the same driver (G = 1 is the plain search's tables, lambda = 0 is G independent
searches, a large lambda gives every group other first tokens); the argument checks; the launch plan under the dry run.
GPU: gtos_diverse_advance against the g++ driver (exact), both new kernels' stores inside guard bands, gtos_diverse_reorder against an
index_select statement, and work(search="device") against work(search="host") with groups, plus the identities end to end."""
import ctypes
import struct

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver, Guarded

DRIVER = r"""
#include "diverse_kernels.h"
// what one gtos_diverse_advance launch does, serially: the flag rotation, every graph's groups by gtos_diverse::advance_serial
extern "C" void diverse_all(int B, int k, int G, double lambda, int t, int V, int tot, int min_t, int max_t, const float* topv,
                            const int* topi, const uint8_t* fs, const uint8_t* fl, double* slot_score, int* state, int* bp_parent,
                            int* bp_token, int* comp_step, int* comp_parent, double* comp_score, int* active) {
    using namespace gtos_diverse;
    static double pm[MAX_POOL], pk[MAX_POOL];
    static int pt[MAX_POOL], order[MAX_K], chosen[MAX_K];
    static uint8_t pf[MAX_POOL];
    const long N = (long)B * k;
    active[active_clear(t)] = 0;
    if (!active[active_read(t)]) return;
    for (int b = 0; b < B; ++b)
        if (advance_serial(b, k, G, lambda, t, V, tot, min_t, max_t, topv, topi, fs, fl, slot_score, state, bp_parent + t * N,
                           bp_token + t * N, comp_step, comp_parent, comp_score, pm, pk, pt, pf, order, chosen))
            active[active_set(t)] |= 1;
}
// ... and one gtos_beam_advance launch (csrc/beam_kernels.h), for the G = 1 identity
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
extern "C" int lambda_fine(double lambda) { return gtos_diverse::lambda_ok(lambda); }
"""

PAD, UNK, STR, END = "<PAD>", "<UNK>", "<STR>", "<END>"
SHAPES = [(4, 2), (6, 3), (32, 4), (32, 32), (32, 2), (8, 1)]           # (k, G)
GPU_SHAPES = [(32, 2), (32, 32), (6, 3), (8, 1)]     # a pool larger than the workgroup, 32 phases, a width that is no power of two, 1024 entries
LAMBDAS = [0.0, 0.5, 1e4]
B, V, N_LOCAL, MAX_T = 3, 40, 6, 12


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = compile_host_driver(tmp_path_factory, "diverse_host", DRIVER)
    lib.diverse_all.argtypes = [ctypes.c_int] * 3 + [ctypes.c_double] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 12
    lib.diverse_all.restype = None
    lib.plain_all.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 12
    lib.plain_all.restype = None
    lib.lambda_fine.argtypes = [ctypes.c_double]
    return lib


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Tables(object):
    """The tables of a grouped device search as numpy arrays: state [B*G, 4], the rest as the plain search's."""

    def __init__(self, B, k, G, max_t):
        N = B * k
        self.B, self.k, self.G, self.N, self.max_t = B, k, G, N, max_t
        self.active = np.array([1, 0, 0], dtype=np.int32)
        self.state = np.zeros((B * G, 4), dtype=np.int32)
        self.state[:, 2] = 1
        self.bp_parent = np.full((max_t, N), -1, dtype=np.int32)
        self.bp_token = np.full((max_t, N), -1, dtype=np.int32)
        self.comp_step = np.zeros((B, k), dtype=np.int32)
        self.comp_parent = np.zeros((B, k), dtype=np.int32)
        self.slot_score = np.zeros(N, dtype=np.float64)
        self.comp_score = np.zeros((B, k), dtype=np.float64)

    def arrays(self):
        return [self.slot_score, self.state, self.bp_parent, self.bp_token, self.comp_step, self.comp_parent, self.comp_score,
                self.active]

    def beams(self, strings, min_t):
        from gtos_amd.search import Beam, fill_beams
        beams = [Beam(self.k, min_t, self.max_t) for _ in range(self.B)]
        return fill_beams(beams, self.k, self.state.ravel().tolist(), self.bp_parent.ravel().tolist(), self.bp_token.ravel().tolist(),
                          self.comp_step.ravel().tolist(), self.comp_parent.ravel().tolist(), self.slot_score.tolist(),
                          self.comp_score.ravel().tolist(), lambda b, i: strings[b][i], groups=self.G)


def host_step(lib):
    def step(tab, lam, t, V_, tot, min_t, topv, topi, fs, fl):
        lib.diverse_all(tab.B, tab.k, tab.G, lam, t, V_, tot, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(fs), _np_ptr(fl),
                        *[_np_ptr(a) for a in tab.arrays()])
    return step


def plain_step(lib):
    def step(tab, lam, t, V_, tot, min_t, topv, topi, fs, fl):
        lib.plain_all(tab.B, tab.k, t, V_, tot, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(fs), _np_ptr(fl),
                      *[_np_ptr(a) for a in tab.arrays()])
    return step


def gpu_step(tab, lam, t, V_, tot, min_t, topv, topi, fs, fl):
    """The same step on the device kernel: tables up, one gtos_diverse_advance, tables down."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    g = [torch.from_numpy(a).to(dev) for a in tab.arrays()]
    ops.diverse_advance(t, tab.k, tab.G, lam, V_, tot, min_t, tab.max_t, torch.from_numpy(topv).to(dev), torch.from_numpy(topi).to(dev),
                        torch.from_numpy(fs).to(dev), torch.from_numpy(fl).to(dev) if fl.size else None, *g)
    for a, x in zip(tab.arrays(), g):
        a[...] = x.cpu().numpy()


def pairs(hyps):
    return [(h.seq, h.score) for h in hyps]


def compare(got, want, what):
    """Beam objects filled from the tables against the Python rule's: per group and on the union."""
    for b, (g, w) in enumerate(zip(got, want)):
        tag = "%s, graph %d" % (what, b)
        assert len(g.groups) == len(w.groups), tag
        for j, (gg, wg) in enumerate(zip(g.groups, w.groups)):
            gt = "%s group %d" % (tag, j)
            assert gg.beam_size == wg.beam_size and gg.steps == wg.steps, gt
            assert pairs(gg.hypotheses) == pairs(wg.hypotheses), gt + " alive"
            assert pairs(gg.completed_hypotheses) == pairs(wg.completed_hypotheses), gt + " completed"
            assert gg.completed() == wg.completed(), gt
        assert g.steps == w.steps and pairs(g.hypotheses) == pairs(w.hypotheses), tag
        assert pairs(g.completed_hypotheses) == pairs(w.completed_hypotheses), tag


def random_search(rng, step_fn, k, G, lam, min_t, twin=None, independent=False):
    """One multi-step grouped search of B graphs: the Python rule (search.GroupBeam) and step_fn (the fixed-slot tables) fed the same
    candidate lists.  Every token class occurs (<UNK> as a vocabulary id, <END> as a vocabulary id and as copy strings), values lie on
    a coarse grid so that ties occur, some are -inf.  The strings of a graph's tokens that can survive are unique, so comparing ids
    (the tables) and strings (the rule) coincide: only <END> is spelled by several ids, and an <END> never joins the chosen list.
    With lam = 1e4 the candidates of step 0 are k finite plain tokens (at least G, as the identity asks; all k, so that it holds for
    every hypothesis of a group of any width): the first tokens of a graph's groups must then be pairwise distinct.
    ``twin`` = (step function, Tables): a second implementation fed the same steps whose tables must stay equal to the first's.
    ``independent``: lam = 0, every group next to a plain Beam of width g fed the group's candidates.
    Returns the number of group advances compared."""
    from gtos_amd.search import Beam, GroupBeam
    g = k // G
    tot = V + N_LOCAL
    words = [PAD, UNK, END] + ["w%d" % i for i in range(V - 3)]
    strings = [words + [END if rng.rand() < 0.3 else "c%d" % j for j in range(N_LOCAL)] for _ in range(B)]
    for s in strings:
        plain = [w for w in s if w != END]
        assert len(plain) == len(set(plain))
    cls = lambda w: 1 if w == UNK else 2 if w == END else 0
    fs = np.array([cls(w) for w in words], dtype=np.uint8)
    fl = np.array([[cls(w) for w in s[V:]] for s in strings], dtype=np.uint8).reshape(B, N_LOCAL)
    tab = Tables(B, k, G, MAX_T)
    beams = [GroupBeam(k, min_t, MAX_T, G, lam) for _ in range(B)]
    solo = [[Beam(g, min_t, MAX_T) for _ in range(G)] for _ in range(B)] if independent else None
    n_adv, t = 0, 0
    while True:
        compare(tab.beams(strings, min_t), beams, "before step %d" % t)
        live = [beam.live_hypotheses() if not beam.completed() else [] for beam in beams]
        if not any(live):
            break
        assert t < MAX_T
        topv = np.full((B * k, k), np.nan, dtype=np.float32)
        topi = np.zeros((B * k, k), dtype=np.int32)
        for s in range(B * k):
            if lam == 1e4 and t == 0:
                ok = [i for i, w in enumerate(strings[s // k]) if cls(w) == 0 and w != PAD]
                ids = rng.choice(ok, size=k, replace=False)
                vals = rng.choice([-0.5, -1.0, -1.5, -2.0, -3.0], size=k).astype(np.float32)
            else:
                ids = rng.choice(tot, size=k, replace=False)
                vals = rng.choice([-0.5, -1.0, -1.5, -2.0, -3.0, -np.inf], size=k, p=[.25, .25, .2, .15, .1, .05]).astype(np.float32)
                if rng.rand() < 0.5:
                    vals = (vals + rng.randn(k).astype(np.float32) * 0.01).astype(np.float32)
            order = np.lexsort((ids, -vals.astype(np.float64)))       # descending value, lower id first
            topv[s], topi[s] = vals[order], ids[order]
        before = [[(grp.completed(), len(grp.hypotheses)) for grp in beam.groups] for beam in beams]
        for b, beam in enumerate(beams):
            beam.last_parents = [None] * G
            if beam.completed():
                continue
            results, cuts = [], []
            for j, grp in enumerate(beam.groups):
                if grp.completed():
                    continue
                rows = [[(strings[b][int(i)], float(v)) for v, i in zip(topv[s], topi[s])]
                        for s in range(b * k + j * g, b * k + j * g + len(grp.hypotheses))]
                cuts.append((j, rows))
                results += rows
            keep = beam.advance(results)
            assert len(keep) == len(beam.live_hypotheses())
            if solo:
                for j, rows in cuts:
                    solo[b][j].advance(rows)
        step_fn(tab, lam, t, V, tot, min_t, topv, topi, fs, fl)
        if twin:
            twin[0](twin[1], lam, t, V, tot, min_t, topv, topi, fs, fl)
            for a, a2 in zip(tab.arrays(), twin[1].arrays()):
                assert np.array_equal(a.ravel(), a2.ravel(), equal_nan=True), ("twin tables", t)
        # parents, per-group counters and the continue flag of this step
        go = False
        for b, beam in enumerate(beams):
            for j, grp in enumerate(beam.groups):
                q, at = b * G + j, b * k + j * g
                was_done, _ = before[b][j]
                par = beam.last_parents[j]
                assert (par is None) == was_done, (t, b, j)
                assert tab.state[q].tolist() == [grp.steps, len(grp.completed_hypotheses), len(grp.hypotheses), int(grp.completed())], (t, b, j)
                if par is not None:
                    n_adv += 1
                    assert [int(p) - at for p in tab.bp_parent[t, at:at + len(par)]] == list(par), ("parents", t, b, j)
                    assert (tab.bp_parent[t, at + len(par):at + g] == -1).all(), ("dead slots", t, b, j)
                    assert [strings[b][int(i)] for i in tab.bp_token[t, at:at + len(par)]] == [h.seq[-1] for h in grp.hypotheses]
                else:
                    assert (tab.bp_parent[t, at:at + g] == -1).all(), ("a done group's row", t, b, j)
                go |= not grp.completed() and len(grp.hypotheses) > 0
        assert int(tab.active[(t + 1) % 3]) == int(go) and int(tab.active[(t + 2) % 3]) == 0, ("continue flag", t)
        if lam == 1e4 and t == 0:
            for b, beam in enumerate(beams):
                first = [[h.seq[1] for h in grp.hypotheses] for grp in beam.groups]
                flat = [w for f in first for w in f]
                assert all(len(f) == g for f in first) and len(set(flat)) == k, ("first tokens", b, first)
        if solo:
            for b, beam in enumerate(beams):
                for j, grp in enumerate(beam.groups):
                    assert pairs(grp.hypotheses) == pairs(solo[b][j].hypotheses), ("independent", t, b, j)
                    assert pairs(grp.completed_hypotheses) == pairs(solo[b][j].completed_hypotheses), ("independent", t, b, j)
                    assert grp.steps == solo[b][j].steps
        t += 1
    # the device loop keeps launching steps up to max_t: they must change nothing
    snap = [a.copy() for a in tab.arrays()[:-1]]
    for t2 in range(t, MAX_T):
        step_fn(tab, lam, t2, V, tot, min_t, np.zeros((B * k, k), np.float32), np.zeros((B * k, k), np.int32), fs, fl)
    for a, b_ in zip(tab.arrays()[:-1], snap):
        assert np.array_equal(a, b_, equal_nan=True), "a step after the end changed the tables"
    compare(tab.beams(strings, min_t), beams, "end")
    return n_adv


# ------------------------------------------------------------------------------------------------ CPU: the header
@pytest.mark.parametrize("k,G", SHAPES)
def test_rule_header_matches_the_python_rule(host_lib, k, G):
    step = host_step(host_lib)
    n = 0
    for li, lam in enumerate(LAMBDAS):
        rng = np.random.RandomState(20261018 + 1000 * k + 10 * G + li)
        for rep in range(4):
            n += random_search(rng, step, k, G, lam, min_t=rep % 4)
    assert n >= 12 * G, n


def test_one_group_is_the_plain_beam_search(host_lib):
    """G = 1: the tables of gtos_diverse::advance_serial equal those of gtos_beam::advance_serial step by step, whatever lambda is."""
    from test_device_beam_search import Tables as PlainTables
    for li, lam in enumerate(LAMBDAS):
        for k in (8, 5, 32):
            rng = np.random.RandomState(77 + 10 * k + li)
            for min_t in (0, 2):
                assert random_search(rng, host_step(host_lib), k, 1, lam, min_t, twin=(plain_step(host_lib), PlainTables(B, k, MAX_T))) > 0


@pytest.mark.parametrize("k,G", SHAPES)
def test_without_penalty_the_groups_are_independent_searches(host_lib, k, G):
    rng = np.random.RandomState(4242 + 100 * k + G)
    for min_t in (0, 1, 3):
        assert random_search(rng, host_step(host_lib), k, G, 0.0, min_t, independent=True) > 0


@pytest.mark.parametrize("k,G", [s for s in SHAPES if s[1] > 1])
def test_a_large_penalty_separates_the_first_tokens(host_lib, k, G):
    """(the assertion sits in random_search, at step 0 of every lam = 1e4 search)"""
    rng = np.random.RandomState(99 + 100 * k + G)
    for min_t in (0, 2):
        assert random_search(rng, host_step(host_lib), k, G, 1e4, min_t) > 0


def test_scores_are_model_scores_not_keys(host_lib):
    """With lam = 1e4 a penalised candidate that is kept carries its log-likelihood: every stored score stays above -100."""
    from gtos_amd.search import GroupBeam
    beam = GroupBeam(4, 0, 5, 2, 1e4)
    rows = [[("a", -1.0), ("b", -2.0), ("x", float("-inf")), ("y", float("-inf"))]] * 2
    assert beam.advance(rows) == [0, 0, 1, 1]
    assert pairs(beam.groups[0].hypotheses) == [([STR, "a"], -1.0), ([STR, "b"], -2.0)]
    assert pairs(beam.groups[1].hypotheses) == [([STR, "a"], -1.0), ([STR, "b"], -2.0)]        # keys -10001, -10002 beat -inf
    assert beam.last_parents == [[0, 0], [0, 0]] and beam.steps == 1 and len(beam.hypotheses) == 4


# ------------------------------------------------------------------------------------------------ CPU: argument checks
def test_work_checks_groups_and_diversity():
    """No model needed: the checks run before anything is touched."""
    from gtos_amd.generator import Generator
    for search in ("host", "device"):
        for bad in (0, -1, 3, 1.5, True, "2", None):                      # 3 does not divide 4
            with pytest.raises(ValueError):
                Generator.work(None, {}, 4, 10, search=search, groups=bad, diversity=0.0)
        for bad in (-0.5, float("inf"), float("nan"), "1", True, None):
            with pytest.raises(ValueError):
                Generator.work(None, {}, 4, 10, search=search, groups=2, diversity=bad)
        with pytest.raises(ValueError):
            Generator.work(None, {}, 4, 10, search=search, diversity=0.5)                 # groups = 1: would do nothing
    for kw in (dict(groups=2), dict(diversity=0.5), dict(groups=2, diversity=0.5)):
        with pytest.raises(ValueError):
            Generator.work(None, {}, 4, 10, search="sample", seed=1, **kw)


def _bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def test_diverse_entry_points_refuse_bad_arguments(host_lib):
    """-10 outside the shapes, -23 for null pointers; nothing launched, no device needed."""
    from gtos_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def adv(B_=2, k=4, G=2, lam=0.5, t=0, V_=10, tot=10, max_t=5, ptrs=None):
        return lib.gtos_diverse_advance(B_, k, G, _bits(lam), t, V_, tot, 0, max_t, *(ptrs or [p] * 12), None)
    assert adv(k=33, G=1) == -10 and adv(k=0) == -10
    assert adv(G=0) == -10 and adv(G=3) == -10 and adv(k=32, G=5) == -10
    assert adv(lam=-0.5) == -10 and adv(lam=float("inf")) == -10 and adv(lam=float("nan")) == -10 and adv(lam=-float("inf")) == -10
    assert adv(t=5) == -10 and adv(t=-1) == -10 and adv(tot=9) == -10 and adv(V_=0, tot=0) == -10
    for i in range(12):
        ptrs = [p] * 12
        ptrs[i] = None
        assert adv(ptrs=ptrs, tot=12) == -23, i
    assert adv(B_=0, k=99) == 0
    assert [host_lib.lambda_fine(x) for x in (0.0, 0.5, 1e4, -1e-300, float("inf"), float("nan"))] == [1, 1, 1, 0, 0, 0]

    def reo(row_bytes=32, N=8, k=4, g=2, t=0, state=p, active=p, bp=p):
        return lib.gtos_diverse_reorder(1, p, p, row_bytes, N, k, g, t, 5, bp, p, state, active, 10, 10, p, p, p, p, 22, 0, p, p, p, None)
    assert reo(row_bytes=24) == -10 and reo(N=9) == -10 and reo(t=5) == -10 and reo(k=33, g=33, N=33) == -10
    assert reo(g=0) == -10 and reo(g=3) == -10 and reo(g=8) == -10
    assert reo(state=None) == -23 and reo(active=None) == -23 and reo(bp=None) == -23
    assert reo(N=0, g=0) == 0


def test_ops_check_shapes_under_the_dry_run():
    from dryrun import DryRun
    from gtos_amd import ops
    with DryRun() as rec:
        B_, k, G, max_t, V_, tot, C = 2, 6, 3, 5, 10, 13, 4
        N = B_ * k
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
        f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
        tabs = [f64(N), i32(B_ * G, 4), i32(max_t, N), i32(max_t, N), i32(B_, k), i32(B_, k), f64(B_, k), i32(3)]
        flags = [torch.zeros(V_, dtype=torch.uint8), torch.zeros(B_, tot - V_, dtype=torch.uint8)]
        ops.diverse_advance(1, k, G, 0.5, V_, tot, 0, max_t, torch.zeros(N, k), i32(N, k), *flags, *tabs)
        with pytest.raises(AssertionError):
            ops.diverse_advance(1, k, 4, 0.5, V_, tot, 0, max_t, torch.zeros(N, k), i32(N, k), *flags, *tabs)      # 4 does not divide 6
        with pytest.raises(AssertionError):
            ops.diverse_advance(1, k, G, 0.5, V_, tot, 0, max_t, torch.zeros(N, k), i32(N, k), *flags, tabs[0], i32(B_, 4), *tabs[2:])
        i64 = lambda *s: torch.zeros(*s, dtype=torch.int64)
        src, dst = [torch.zeros(max_t, N, 8)], [torch.zeros(max_t, N, 8)]
        nxt = [i64(V_), i64(B_, tot - V_), i64(V_, C), i64(B_, tot - V_, C), 0, i64(C), i64(N), i64(N, C)]
        ops.diverse_reorder(src, dst, 1, k, k // G, tabs[2], tabs[3], tabs[1], tabs[7], V_, tot, *nxt)
        with pytest.raises(AssertionError):
            ops.diverse_reorder(src, dst, 1, k, 4, tabs[2], tabs[3], tabs[1], tabs[7], V_, tot, *nxt)
    assert rec.names() == ["gtos_diverse_advance", "gtos_diverse_reorder"]
    assert rec.calls[0][1][:9] == (B_, k, G, _bits(0.5), 1, V_, tot, 0, max_t)
    assert rec.calls[1][1][3:9] == (32, N, k, k // G, 1, max_t)


# ------------------------------------------------------------------------------------------------ CPU: launch plans
def test_grouped_device_search_launches_the_diverse_kernels():
    from dryrun import DryRun
    from gtos_amd import synth
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
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
        n_graphs = batch['concept'].shape[1]

        def plan(**kw):
            n0 = len(rec.calls)
            beams = model.work(batch, k, steps, search="device", **kw)
            assert len(beams) == n_graphs
            return beams, rec.calls[n0:]
        _, base = plan()
        names = [c[0] for c in base]
        assert names.count("gtos_beam_topk") == names.count("gtos_beam_advance") == names.count("gtos_beam_reorder") == steps
        assert not [x for x in names if x.startswith("gtos_diverse")]
        assert [c[0] for c in plan(groups=1, diversity=0.0)[1]] == names                       # the defaults: the plan of today
        beams, calls = plan(groups=2, diversity=0.5)
        got = [c[0] for c in calls]
        swap = {"gtos_beam_advance": "gtos_diverse_advance", "gtos_beam_reorder": "gtos_diverse_reorder"}
        assert got == [swap.get(x, x) for x in names]                                          # launch for launch, two of them swapped
        assert got.count("gtos_beam_topk") == got.count("gtos_diverse_advance") == got.count("gtos_diverse_reorder") == steps
        adv = [c[1] for c in calls if c[0] == "gtos_diverse_advance"]
        assert [a[:5] for a in adv] == [(n_graphs, k, 2, _bits(0.5), t) for t in range(steps)]
        reo = [c[1] for c in calls if c[0] == "gtos_diverse_reorder"]
        assert [a[4:8] for a in reo] == [(n_graphs * k, k, 2, t) for t in range(steps)]
        topk = [c[1] for c in calls if c[0] == "gtos_beam_topk"]
        assert all(a[0] == n_graphs * k and a[2] == k for a in topk)                           # the whole k per slot, not g
        for beam in beams:
            assert len(beam.groups) == 2 and all(grp.beam_size == 2 for grp in beam.groups)
        _, blocked = plan(groups=2, diversity=0.5, no_repeat_ngram=3)
        assert [c[0] for c in blocked if c[0] != "gtos_ngram_block"] == got
        assert [c[0] for c in blocked].count("gtos_ngram_block") == steps - 1


# ------------------------------------------------------------------------------------------------ GPU: the advance kernel
@pytest.mark.gpu
@pytest.mark.parametrize("k,G", GPU_SHAPES)
def test_diverse_advance_kernel_matches_the_header(host_lib, k, G):
    """The kernel and the g++ driver over the same random searches: every table equal after every step (the twin), and both equal to
    the Python rule."""
    n = 0
    for li, lam in enumerate(LAMBDAS):
        rng = np.random.RandomState(31 + 1000 * k + 10 * G + li)
        for min_t in (0, 2):
            n += random_search(rng, gpu_step, k, G, lam, min_t, twin=(host_step(host_lib), Tables(B, k, G, MAX_T)))
    assert n >= 6 * G


POISON = -7


class Banded(object):
    """A table carved from the middle of a poisoned allocation (any dtype): ``.view`` is the table, ``.check()`` asserts that the
    bands on both sides still hold the poison."""

    def __init__(self, init, dev, margin=4096):
        flat = torch.from_numpy(np.ascontiguousarray(init)).reshape(-1)
        self.whole = torch.full((2 * margin + flat.numel(),), POISON, dtype=flat.dtype, device=dev)
        self.view = self.whole[margin:margin + flat.numel()].view(*init.shape)
        self.view.copy_(flat.view(*init.shape))
        self.margin = margin

    def check(self, what):
        w = self.whole.cpu()
        n = w.numel() - 2 * self.margin
        assert bool((w[:self.margin] == POISON).all()) and bool((w[self.margin + n:] == POISON).all()), what + ": a store outside the table"


@pytest.mark.gpu
@pytest.mark.parametrize("k,G", [(32, 1), (32, 32), (6, 3)])
def test_diverse_advance_stores_inside_its_outputs(host_lib, k, G):
    """Three steps of a search on tables carved from poisoned allocations: the bands stay, and the tables equal the g++ driver's, so
    nothing inside them changed that the rule does not write."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(5 + k + G)
    tot = V + N_LOCAL
    fs = np.zeros(V, dtype=np.uint8)
    fs[1], fs[2] = 1, 2
    fl = np.zeros((B, N_LOCAL), dtype=np.uint8)
    fl[:, 0] = 2
    host = Tables(B, k, G, MAX_T)
    band = [Banded(a, dev) for a in Tables(B, k, G, MAX_T).arrays()]
    D = lambda a: torch.from_numpy(a).to(dev)
    for t in range(3):
        topi = np.stack([np.sort(rng.choice(tot, size=k, replace=False)) for _ in range(B * k)]).astype(np.int32)
        topv = -np.sort(rng.choice([0.5, 1.0, 1.5, 2.0], size=(B * k, k)), axis=1).astype(np.float32)
        host_step(host_lib)(host, 0.5, t, V, tot, 1, topv, topi, fs, fl)
        ops.diverse_advance(t, k, G, 0.5, V, tot, 1, MAX_T, D(topv), D(topi), D(fs), D(fl), *[x.view for x in band])
        for x, a, name in zip(band, host.arrays(), ("slot_score", "state", "bp_parent", "bp_token", "comp_step", "comp_parent", "comp_score", "active")):
            x.check("gtos_diverse_advance %s, step %d" % (name, t))
            assert np.array_equal(x.view.cpu().numpy(), a), (name, t)
    assert int(host.state[:, 0].max()) == 3 and int(host.state[:, 2].sum()) > 0          # (a group of width 1 may be done after two steps)


# ------------------------------------------------------------------------------------------------ GPU: the reorder kernel
@pytest.mark.gpu
@pytest.mark.parametrize("dtype,width", [(torch.bfloat16, 1024), (torch.float32, 72)])
def test_diverse_reorder_gathers_exactly_and_inside_its_outputs(dtype, width):
    """G = 2 with, per graph, one group done and one live (and a graph with both live): the done group's slots get zero rows and the
    padding input, copy ids resolve through the table of the GRAPH (the local tables differ between graphs), and nothing outside the
    caches' rows [0, t] or the input rows is stored (guard bands)."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(width)
    B_, k, G, T, V_, tot, C = 3, 6, 2, 7, 30, 37, 22
    g, N = k // G, B_ * k
    src = [torch.randn(T, N, width, generator=gen).to(dtype).to(dev) for _ in range(2)]
    bp_parent = torch.randint(-1, N, (T, N), generator=gen, dtype=torch.int32)
    bp_token = torch.randint(0, tot, (T, N), generator=gen, dtype=torch.int32)
    bp_token[:, ::2] = torch.randint(V_, tot, (T, (N + 1) // 2), generator=gen, dtype=torch.int32)      # many copy ids
    state = torch.zeros(B_ * G, 4, dtype=torch.int32)
    state[0, 3] = 1                                          # graph 0: group 0 done, group 1 live
    state[3, 3] = 1                                          # graph 1: group 1 done, group 0 live; graph 2: both live
    tok_shared = torch.randint(0, 1000, (V_,), generator=gen)
    char_shared = torch.randint(0, 100, (V_, C), generator=gen)
    tok_local = torch.randint(1000, 2000, (B_, tot - V_), generator=gen)
    char_local = torch.randint(100, 200, (B_, tot - V_, C), generator=gen)
    assert not torch.equal(tok_local[0], tok_local[1]) and not torch.equal(tok_local[1], tok_local[2])
    dead_char = torch.randint(0, 100, (C,), generator=gen)
    D = lambda x: x.to(dev)
    for t, act in ((0, 1), (4, 1), (T - 1, 1), (3, 0)):
        active = torch.zeros(3, dtype=torch.int32)
        active[t % 3] = act
        dst = [Guarded(T * N, width, dtype, dev, lead=8, trail=8, init=7.0) for _ in src]
        tok_out = Banded(np.full((N,), -5, dtype=np.int64), dev)
        char_out = Banded(np.full((N, C), -5, dtype=np.int64), dev)
        ops.diverse_reorder(src, [d.view.view(T, N, width) for d in dst], t, k, g, D(bp_parent), D(bp_token), D(state), D(active), V_, tot,
                            D(tok_shared), D(tok_local), D(char_shared), D(char_local), 3, D(dead_char), tok_out.view, char_out.view)
        par = bp_parent[t].long()
        live = (par >= 0) & (state[torch.arange(N) // g, 3] == 0) & bool(act)
        assert not live[:g].any() and not live[k + g:2 * k].any()                      # the done groups
        if act:
            assert live[g:k].any() and live[k:k + g].any() and live[2 * k:].any()
        for s_, d_ in zip(src, dst):
            d_.check("gtos_diverse_reorder cache, t = %d" % t)
            want = torch.full((T, N, width), 7.0).to(dtype)
            if act:
                rows = s_.cpu()[: t + 1].index_select(1, par.clamp(min=0))
                rows[:, ~live] = 0
                want[: t + 1] = rows
            assert torch.equal(d_.view.view(T, N, width).cpu(), want), (t, act)
        ids = bp_token[t].long()
        wt = torch.full((N,), 3, dtype=torch.int64)
        wc = dead_char.expand(N, C).clone()
        for s in range(N):
            if live[s]:
                i, b = int(ids[s]), s // k
                wt[s] = tok_shared[i] if i < V_ else tok_local[b, i - V_]
                wc[s] = char_shared[i] if i < V_ else char_local[b, i - V_]
        tok_out.check("gtos_diverse_reorder tok_out")
        char_out.check("gtos_diverse_reorder char_out")
        assert torch.equal(tok_out.view.cpu(), wt) and torch.equal(char_out.view.cpu(), wc), (t, act)


# ------------------------------------------------------------------------------------------------ GPU: end to end
def _synth_model(config, dtype):
    """(the construction of test_device_beam_search.py::_synth_model)"""
    from gtos_amd import synth
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    dev = torch.device("cuda:0")
    cfg = synth.CONFIGS[config]
    vocabs = synth.synth_vocabs()
    torch.manual_seed(19940117)
    model = Generator(vocabs, device=dev, depth_size=256 if cfg["kind"] == "dep" else 32, **generator_args(cfg)).to(dev)
    model.set_compute_dtype(dtype)
    model.eval()
    batch, _ = synth.make_config_batch(config, train=False)
    batch_dev = {k: v.to(dev) for k, v in attach_path_trie(batch).items()}
    pv, cp = vocabs['predictable_token'], batch['cp_seq']
    batch_dev['local_idx2token'] = [{int(i): "copy%d" % int(i) for i in cp[:, b].tolist() if i >= pv.size} for b in range(cp.shape[1])]
    return model, batch_dev


_model = {}


def synth_c1():
    if not _model:
        _model["c1"] = _synth_model("C1", torch.float32)
    return _model["c1"]


def _close(x, y):
    return x == y or abs(x - y) <= 1e-5 * abs(x)               # the tolerance of test_device_search_equals_host_search_fp32


@pytest.mark.gpu
@pytest.mark.parametrize("k,G,lam,ngram", [(8, 4, 0.5, 0), (6, 2, 1e4, 0), (8, 4, 0.5, 2), (6, 2, 1e4, 2)])
def test_grouped_device_search_equals_grouped_host_search_fp32(k, G, lam, ngram):
    """C1-sized fp32 batch (every row of the decoder's launches is computed the same whatever the row count): the two searches pick
    the same hypotheses, group by group."""
    model, batch = synth_c1()
    max_t, min_t = 10, 1
    kw = dict(groups=G, diversity=lam, no_repeat_ngram=ngram)
    host = model.work(batch, k, max_t, min_t, **kw)
    dev = model.work(batch, k, max_t, min_t, search="device", **kw)
    distinct = 0
    for b, (h, d) in enumerate(zip(host, dev)):
        assert h.steps == d.steps and len(h.groups) == len(d.groups) == G, b
        for j, (hg, dg) in enumerate(zip(h.groups, d.groups)):
            assert hg.beam_size == dg.beam_size == k // G and hg.steps == dg.steps, (b, j)
            for hl, dl in ((hg.hypotheses, dg.hypotheses), (hg.completed_hypotheses, dg.completed_hypotheses)):
                assert [x.seq for x in hl] == [x.seq for x in dl], (b, j)
                assert all(_close(x.score, y.score) for x, y in zip(hl, dl)), (b, j)
        assert [x.seq for x in h.hypotheses] == [x.seq for g_ in h.groups for x in g_.hypotheses]
        assert [x.seq for x in d.completed_hypotheses] == [x.seq for g_ in d.groups for x in g_.completed_hypotheses]
        hb, db = h.get_k_best(k, 0.6), d.get_k_best(k, 0.6)
        assert [x.seq for x in hb] == [x.seq for x in db], b
        firsts = [g_.hypotheses[0].seq[1] for g_ in d.groups if g_.hypotheses]
        distinct += len(set(firsts)) == len(firsts)
        if ngram:
            for x in d.hypotheses + d.completed_hypotheses:
                y = [w for w in x.seq[1:] if w != END]
                grams = [tuple(y[i:i + ngram]) for i in range(len(y) - ngram + 1)]
                assert len(grams) == len(set(grams)), x.seq
    print("MEASURED k=%d G=%d lambda=%g: %d of %d graphs whose groups' best live hypotheses start on distinct tokens" % (k, G, lam, distinct, len(dev)))


def _capture_memory(model, batch, monkeypatch):
    """Generator.work's per-graph memory (encoder run once), by stopping work before its search."""
    import gtos_amd.generator as Gm
    box = {}
    monkeypatch.setattr(Gm, "sample_device", lambda m, memory, beams, *a, **kw: box.update(memory=memory) or beams)
    model.work(batch, 1, 1, search="sample", seed=0)
    monkeypatch.undo()
    return box["memory"]


@pytest.mark.gpu
def test_one_group_through_the_new_kernels_is_the_plain_device_search(monkeypatch):
    from gtos_amd import search
    model, batch = synth_c1()
    memory = _capture_memory(model, batch, monkeypatch)
    for k, max_t, min_t, ngram in ((4, 12, 1, 0), (6, 9, 3, 0), (8, 10, 1, 3)):
        out = []
        for kw in (dict(), dict(grouped=True), dict(grouped=True, diversity=0.5)):
            beams = [search.Beam(k, min_t, max_t) for _ in memory['local_idx2token']]
            stats = {}
            with torch.no_grad():
                search.beam_search_device(model, memory, beams, stats=stats, no_repeat_ngram=ngram, **kw)
            out.append([(b.steps, pairs(b.hypotheses), pairs(b.completed_hypotheses)) for b in beams] + [stats])
            if kw:
                assert all(len(b.groups) == 1 and pairs(b.groups[0].hypotheses) == pairs(b.hypotheses) for b in beams)
        assert out[0] == out[1] == out[2], (k, max_t, min_t)


@pytest.mark.gpu
def test_without_penalty_two_groups_are_two_plain_device_searches():
    """lambda = 0, G = 2, k = 8: each group equals the plain k = 4 device search (a width-4 cut never reaches below a slot's fourth
    candidate, so the top-8 the groups see changes nothing)."""
    model, batch = synth_c1()
    max_t, min_t = 10, 1
    plain = model.work(batch, 4, max_t, min_t, search="device")
    two = model.work(batch, 8, max_t, min_t, search="device", groups=2, diversity=0.0)
    for b, (p, d) in enumerate(zip(plain, two)):
        assert len(d.groups) == 2 and d.steps == p.steps, b
        for j, grp in enumerate(d.groups):
            assert grp.steps == p.steps, (b, j)
            for gl, pl in ((grp.hypotheses, p.hypotheses), (grp.completed_hypotheses, p.completed_hypotheses)):
                assert [x.seq for x in gl] == [x.seq for x in pl], (b, j)
                assert all(_close(x.score, y.score) for x, y in zip(gl, pl)), (b, j)
