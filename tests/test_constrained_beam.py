"""Lexically constrained beam search (Generator.work(..., constraints=[...]), gtos_amd.search.ConstrainedBeam, csrc/constrain.hip,
csrc/constrain_kernels.h).

CPU: the rule header compiled with g++ is driven through random multi-step searches next to the Python statement of the rule
(ConstrainedBeam.advance, fed the same candidate lists and forced log-likelihoods): tables, met rows, state words and the continue flag
must agree exactly; identities on the same driver (no constraints: the tables of gtos_beam::advance_serial; k = 1: the first c tokens
are the constraints; a completion holds every constraint; a slot's mask is its sequence's; a beam ends holding a hypothesis with every
constraint); the argument checks; the launch plan under the dry run.
GPU: gtos_constrain_advance against the g++ driver (exact), its stores inside guard bands, work(search="device") against
work(search="host") with constraints, and the route without constraints against the plain device search."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver, Guarded

DRIVER = r"""
#include "constrain_kernels.h"
// what one gtos_constrain_advance launch does, serially: the flag rotation, every beam by gtos_constrain::advance_serial
extern "C" void constrain_all(int B, int k, int Cw, int t, int V, int tot, int min_t, int max_t, const float* topv, const int* topi,
                              const float* ll, long ld, const int* cons, const uint8_t* fs, const uint8_t* fl, double* slot_score,
                              int* state, int* bp_parent, int* bp_token, int* comp_step, int* comp_parent, double* comp_score, int* met,
                              int* active) {
    using namespace gtos_constrain;
    static double ps[MAX_POOL];
    static int pt[MAX_POOL], pm[MAX_POOL], pq[MAX_POOL], order[MAX_K];
    static uint8_t pf[MAX_POOL];
    static signed char pb[MAX_POOL];
    const long N = (long)B * k;
    active[active_clear(t)] = 0;
    if (!active[active_read(t)]) return;
    for (int b = 0; b < B; ++b)
        if (advance_serial(b, k, Cw, t, V, tot, min_t, max_t, topv, topi, ll, ld, cons, fs, fl, slot_score, state, bp_parent + t * N,
                           bp_token + t * N, comp_step, comp_parent, comp_score, met + (t % 2) * N, met + ((t + 1) % 2) * N, ps, pt, pf,
                           pm, pb, pq, order))
            active[active_set(t)] |= 1;
}
// ... and one gtos_beam_advance launch (csrc/beam_kernels.h), for the identity without constraints
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
extern "C" int max_cons() { return gtos_constrain::MAX_CONS; }
"""

PAD, UNK, STR, END = "<PAD>", "<UNK>", "<STR>", "<END>"
SHAPES = [(1, 1), (4, 3), (6, 0), (8, 16), (32, 16)]        # (k, c)
GPU_SHAPES = [(1, 1), (6, 2), (8, 16), (32, 16)]            # ... (32, 16): a pool of up to 1536 entries, six per thread
B, V, TOT, MAX_T = 3, 23, 57, 18
NAMES = ("slot_score", "state", "bp_parent", "bp_token", "comp_step", "comp_parent", "comp_score", "met", "active")


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = compile_host_driver(tmp_path_factory, "constrain_host", DRIVER)
    lib.constrain_all.argtypes = [ctypes.c_int] * 8 + [ctypes.c_void_p] * 3 + [ctypes.c_long] + [ctypes.c_void_p] * 12
    lib.constrain_all.restype = None
    lib.plain_all.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 12
    lib.plain_all.restype = None
    return lib


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


class Tables(object):
    """The tables of a constrained device search as numpy arrays: the plain search's plus met [2, N]."""

    def __init__(self, B_, k, max_t):
        N = B_ * k
        self.B, self.k, self.N, self.max_t = B_, k, N, max_t
        self.active = np.array([1, 0, 0], dtype=np.int32)
        self.state = np.zeros((B_, 4), dtype=np.int32)
        self.state[:, 2] = 1
        self.bp_parent = np.full((max_t, N), -1, dtype=np.int32)
        self.bp_token = np.full((max_t, N), -1, dtype=np.int32)
        self.comp_step = np.zeros((B_, k), dtype=np.int32)
        self.comp_parent = np.zeros((B_, k), dtype=np.int32)
        self.slot_score = np.zeros(N, dtype=np.float64)
        self.comp_score = np.zeros((B_, k), dtype=np.float64)
        self.met = np.zeros((2, N), dtype=np.int32)

    def arrays(self):
        return [self.slot_score, self.state, self.bp_parent, self.bp_token, self.comp_step, self.comp_parent, self.comp_score, self.met,
                self.active]

    def plain_arrays(self):
        return [a for a, n in zip(self.arrays(), NAMES) if n != "met"]

    def beams(self, strings, min_t):
        from gtos_amd.search import Beam, fill_beams
        beams = [Beam(self.k, min_t, self.max_t) for _ in range(self.B)]
        return fill_beams(beams, self.k, self.state.ravel().tolist(), self.bp_parent.ravel().tolist(), self.bp_token.ravel().tolist(),
                          self.comp_step.ravel().tolist(), self.comp_parent.ravel().tolist(), self.slot_score.tolist(),
                          self.comp_score.ravel().tolist(), lambda b, i: strings[b][i])


def host_step(lib):
    def step(tab, cons, t, min_t, topv, topi, ll, fs, fl):
        lib.constrain_all(tab.B, tab.k, cons.shape[1], t, V, TOT, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(ll), ll.shape[1],
                          _np_ptr(cons), _np_ptr(fs), _np_ptr(fl), *[_np_ptr(a) for a in tab.arrays()])
    return step


def plain_step(lib):
    def step(tab, cons, t, min_t, topv, topi, ll, fs, fl):
        lib.plain_all(tab.B, tab.k, t, V, TOT, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(fs), _np_ptr(fl),
                      *[_np_ptr(a) for a in tab.plain_arrays()])
    return step


def gpu_step(tab, cons, t, min_t, topv, topi, ll, fs, fl):
    """The same step on the device kernel: tables up, one gtos_constrain_advance (ll with a leading dimension above its width), tables
    down."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    g = [torch.from_numpy(a).to(dev) for a in tab.arrays()]
    wide = torch.full((ll.shape[0], TOT + 5), float("nan"), dtype=torch.float32, device=dev)
    wide[:, :TOT] = torch.from_numpy(ll).to(dev)
    ops.constrain_advance(t, tab.k, V, TOT, min_t, tab.max_t, torch.from_numpy(topv).to(dev), torch.from_numpy(topi).to(dev),
                          wide[:, :TOT], torch.from_numpy(cons).to(dev), torch.from_numpy(fs).to(dev), torch.from_numpy(fl).to(dev), *g)
    for a, x in zip(tab.arrays(), g):
        a[...] = x.cpu().numpy()


def pairs(hyps):
    return [(h.seq, h.score) for h in hyps]


def mask_of(seq, constraints):
    return sum(1 << i for i, w in enumerate(constraints) if w in seq)


def topk_rows(ll, k):
    """(values, columns) [N, k] of ll's rows, descending, equal values lower column first: what gtos_beam_topk returns."""
    order = np.lexsort((np.broadcast_to(np.arange(ll.shape[1]), ll.shape), -ll.astype(np.float64)), axis=1)[:, :k]
    return np.take_along_axis(ll, order, 1).astype(np.float32), order.astype(np.int32)


def make_world(rng, c, none_for=()):
    """Strings and classes of B graphs' output ids (every class occurs: <UNK> and <END> as vocabulary ids, <END> also as copy strings;
    the strings that can survive are unique within a graph) and their constraints: graph 0 has c, the others a random number up to c
    (``none_for``: graphs without any), drawn from the plain ids other than <PAD>.  -> strings, fs, fl, cons int32 [B, c], cons strings"""
    words = [PAD, UNK, END] + ["w%d" % i for i in range(V - 3)]
    strings = [words + [END if rng.rand() < 0.3 else "c%d" % j for j in range(TOT - V)] for _ in range(B)]
    cls = lambda w: 1 if w == UNK else 2 if w == END else 0         # noqa: E731
    fs = np.array([cls(w) for w in words], dtype=np.uint8)
    fl = np.array([[cls(w) for w in s[V:]] for s in strings], dtype=np.uint8).reshape(B, TOT - V)
    cons = np.full((B, c), -1, dtype=np.int32)
    for b in range(B):
        n = 0 if b in none_for else c if b == 0 else int(rng.randint(0, c + 1))
        ok = [i for i, w in enumerate(strings[b]) if cls(w) == 0 and w != PAD]
        cons[b, :n] = rng.choice(ok, size=n, replace=False)
    return strings, fs, fl, cons, [[strings[b][i] for i in cons[b] if i >= 0] for b in range(B)]


def random_search(rng, step_fn, k, c, min_t, twin=None, finite=False, none_for=(), plain_twin=None):
    """One multi-step constrained search of B graphs: the Python rule (search.ConstrainedBeam) and step_fn (the fixed-slot tables) fed
    the same ll rows [N, TOT] -- multiples of 0.25 so that ties occur, some columns -inf (``finite``: never a constraint's) -- their
    top-k and, per constraint, the ll of its column.
    ``twin`` = (step function, Tables): a second implementation whose tables must stay equal.  ``plain_twin`` = (plain step function,
    Tables): gtos_beam's advance fed the same top-k; the graphs without constraints must get its tables.
    Asserts after every step: state words, back-pointer rows, the met row written, the continue flag, the beams rebuilt from the
    tables, a live mask is its sequence's, a completion holds every constraint.  At the end: with k = 1 and finite lls the first c_b
    tokens are a permutation of the constraints; with finite lls and min_t <= c_b <= MAX_T the beam holds a hypothesis with all of them.
    Returns the number of beam advances compared."""
    from gtos_amd.search import ConstrainedBeam, constraints_met
    strings, fs, fl, cons, cons_str = make_world(rng, c, none_for)
    tab = Tables(B, k, MAX_T)
    beams = [ConstrainedBeam(k, min_t, MAX_T, cons_str[b]) for b in range(B)]
    N = B * k
    n_adv, t = 0, 0
    while True:
        got = tab.beams(strings, min_t)
        for b, (g, w) in enumerate(zip(got, beams)):
            assert g.steps == w.steps and pairs(g.hypotheses) == pairs(w.hypotheses), ("alive before step %d" % t, b)
            assert pairs(g.completed_hypotheses) == pairs(w.completed_hypotheses), ("completed before step %d" % t, b)
        if not any(beam.hypotheses for beam in beams if not beam.completed()):
            break
        assert t < MAX_T
        ll = (-0.25 * rng.randint(0, 25, size=(N, TOT))).astype(np.float32)
        ll[rng.rand(N, TOT) < 0.1] = -np.inf
        if finite:
            for s in range(N):
                ids = cons[s // k][cons[s // k] >= 0]
                ll[s, ids] = np.where(np.isinf(ll[s, ids]), np.float32(-6.25), ll[s, ids])
        topv, topi = topk_rows(ll, k)
        was = [(beam.completed(), len(beam.hypotheses)) for beam in beams]
        for b, beam in enumerate(beams):
            if beam.completed():
                continue
            slots = range(b * k, b * k + len(beam.hypotheses))
            rows = [[(strings[b][int(i)], float(v)) for v, i in zip(topv[s], topi[s])] for s in slots]
            forced = [[(w, float(ll[s, i])) for w, i in zip(cons_str[b], cons[b])] for s in slots]
            beam.last_parents = beam.advance(rows, forced)
            n_adv += 1
        flags = tab.active.copy()
        step_fn(tab, cons, t, min_t, topv, topi, ll, fs, fl)
        if twin:
            twin[0](twin[1], cons, t, min_t, topv, topi, ll, fs, fl)
            for a, a2, name in zip(tab.arrays(), twin[1].arrays(), NAMES):
                assert np.array_equal(a.ravel(), a2.ravel(), equal_nan=True), ("twin tables", name, t)
        if plain_twin:
            other = plain_twin[1]
            other.active[:] = flags                                 # (the flag is shared by the graphs: the plain search follows ours)
            plain_twin[0](other, cons, t, min_t, topv, topi, ll, fs, fl)
            free = [b for b in range(B) if not cons_str[b]]
            assert free
            for b in free:
                own = slice(b * k, b * k + k)
                for name in ("state", "comp_step", "comp_parent", "comp_score"):
                    assert np.array_equal(getattr(tab, name)[b], getattr(other, name)[b]), ("plain tables", name, b, t)
                for name in ("bp_parent", "bp_token"):
                    assert np.array_equal(getattr(tab, name)[:, own], getattr(other, name)[:, own]), ("plain tables", name, b, t)
                assert np.array_equal(tab.slot_score[own], other.slot_score[own]), ("plain tables", "slot_score", b, t)
                assert not tab.met[:, own].any()
            if len(free) == B:
                assert np.array_equal(tab.active, other.active)
        go = False
        for b, beam in enumerate(beams):
            at = b * k
            done_before, _ = was[b]
            assert tab.state[b].tolist() == [beam.steps, len(beam.completed_hypotheses), len(beam.hypotheses), int(beam.completed())], (t, b)
            if not done_before:
                par = beam.last_parents
                assert [int(p) - at for p in tab.bp_parent[t, at:at + len(par)]] == list(par), ("parents", t, b)
                assert (tab.bp_parent[t, at + len(par):at + k] == -1).all(), ("dead slots", t, b)
                assert [strings[b][int(i)] for i in tab.bp_token[t, at:at + len(par)]] == [h.seq[-1] for h in beam.hypotheses]
                assert tab.met[(t + 1) % 2, at:at + len(par)].tolist() == beam.met, ("met", t, b)
                assert not tab.met[(t + 1) % 2, at + len(par):at + k].any(), ("met of dead slots", t, b)
            else:
                assert (tab.bp_parent[t, at:at + k] == -1).all(), ("a done beam's row", t, b)
            assert [mask_of(h.seq, cons_str[b]) for h in beam.hypotheses] == beam.met, ("mask recomputed", t, b)
            for h in beam.completed_hypotheses:
                assert constraints_met(h.seq, cons_str[b]) == len(cons_str[b]), ("a completion lacks a constraint", t, b, h.seq)
            go |= not beam.completed() and len(beam.hypotheses) > 0
        assert int(tab.active[(t + 1) % 3]) == int(go) and int(tab.active[(t + 2) % 3]) == 0, ("continue flag", t)
        t += 1
    # the device loop keeps launching steps up to max_t: they must change nothing
    snap = [a.copy() for a in tab.arrays()[:-1]]
    for t2 in range(t, MAX_T):
        step_fn(tab, cons, t2, min_t, np.zeros((N, k), np.float32), np.zeros((N, k), np.int32), np.zeros((N, TOT), np.float32), fs, fl)
    for a, b_ in zip(tab.arrays()[:-1], snap):
        assert np.array_equal(a, b_, equal_nan=True), "a step after the end changed the tables"
    if finite:
        for b, beam in enumerate(beams):
            cb = len(cons_str[b])
            held = beam.hypotheses + beam.completed_hypotheses
            if k == 1 and held:
                h = held[0]
                assert sorted(h.seq[1:1 + cb]) == sorted(cons_str[b]), ("k = 1: the constraints come first", b, h.seq)
            if min_t <= cb <= MAX_T:
                assert any(constraints_met(h.seq, cons_str[b]) == cb for h in held), ("no hypothesis holds every constraint", b)
    return n_adv


# ------------------------------------------------------------------------------------------------ CPU: the header
@pytest.mark.parametrize("k,c", SHAPES)
def test_rule_header_matches_the_python_rule(host_lib, k, c):
    step = host_step(host_lib)
    rng = np.random.RandomState(20261019 + 100 * k + c)
    n = 0
    for rep in range(6):
        n += random_search(rng, step, k, c, min_t=rep % 4)
    assert n >= 6 * B


@pytest.mark.parametrize("k", [1, 5, 8, 32])
def test_without_constraints_the_tables_are_the_plain_search_s(host_lib, k):
    """Cw = 0, and Cw > 0 with graphs whose row is all -1: those graphs get the tables of gtos_beam::advance_serial step by step."""
    rng = np.random.RandomState(404 + k)
    for min_t in (0, 2):
        assert random_search(rng, host_step(host_lib), k, 0, min_t, none_for=(0, 1, 2), plain_twin=(plain_step(host_lib), Tables(B, k, MAX_T))) > 0
        assert random_search(rng, host_step(host_lib), k, 3, min_t, none_for=(1,), plain_twin=(plain_step(host_lib), Tables(B, k, MAX_T))) > 0


@pytest.mark.parametrize("k,c", [(1, 1), (1, 5), (1, 16), (4, 3), (8, 16), (32, 16), (6, 2)])
def test_constraints_are_met_when_their_lls_are_finite(host_lib, k, c):
    """(the assertions sit at the end of random_search: k = 1 produces the constraints first; every beam with min_t <= c_b <= max_t ends
    holding a hypothesis, live or completed, with all of them)"""
    rng = np.random.RandomState(777 + 100 * k + c)
    for min_t in (0, 1):
        assert random_search(rng, host_step(host_lib), k, c, min_t, finite=True) > 0


def test_python_rule_by_hand():
    """k = 2, constraints (x, y): the fullest bank's best goes first, then the next bank's best; <END> is held back until both are met."""
    from gtos_amd.search import ConstrainedBeam, constraints_met
    ninf = float("-inf")
    beam = ConstrainedBeam(2, 0, 9, ["x", "y"])
    assert beam.advance([[("a", -1.0), (END, -1.5)]], [[("x", -5.0), ("y", ninf)]]) == [0, 0]
    assert pairs(beam.hypotheses) == [([STR, "x"], -5.0), ([STR, "a"], -1.0)] and beam.met == [1, 0]      # <END> absent, y not forced
    # slot 0 (met x): top-k (y, b); slot 1 (nothing met): top-k (a, b), x and y forced
    assert beam.advance([[("y", -2.0), ("b", -0.5)], [("a", -0.1), ("b", -0.2)]], [[("x", -9.0), ("y", -2.0)], [("x", -1.0), ("y", -3.0)]]) == [0, 1]
    # bank 2: x y (-7); bank 1: a x (-2), a y (-4), x b (-5.5); bank 0: a a, a b -- the best of bank 2, then the best of bank 1
    assert pairs(beam.hypotheses) == [([STR, "x", "y"], -7.0), ([STR, "a", "x"], -2.0)] and beam.met == [3, 1]
    assert beam.advance([[(END, -1.0), ("c", -2.0)], [(END, -0.1), ("y", -4.0)]], [[("x", 0.0), ("y", 0.0)]] * 2) == [1]
    assert pairs(beam.completed_hypotheses) == [([STR, "x", "y", END], -8.0)]                            # the other <END> lacks y
    assert pairs(beam.hypotheses) == [([STR, "a", "x", "y"], -6.0)] and beam.met == [3]
    assert constraints_met([STR, "x", "x", "q"], ["x", "y"]) == 1 and constraints_met([], []) == 0
    assert constraints_met(["y", "x"], ["x", "y", "x"]) == 2


# ------------------------------------------------------------------------------------------------ CPU: argument checks
def test_check_constraints():
    from gtos_amd import ops, synth
    from gtos_amd.generator import Generator, check_constraints
    pv = synth.synth_vocabs()['predictable_token']
    word = next(pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END))
    local = [{pv.size: "copy0", pv.size + 1: "copy1"}, {pv.size: "other"}]
    ok = lambda c, search="device", groups=1: check_constraints(c, search, groups, local, pv)      # noqa: E731
    assert ok(None) is None and ok(None, "sample", 2) is None
    assert ok([["copy0", word], []]) == [["copy0", word], []] and ok((("copy1",), ["other"]), "host") == [["copy1"], ["other"]]
    assert ops.CONSTRAIN_MAX == 16
    many = [pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END)][:17]
    assert len(many) == 17 and ok([many[:16], []]) == [many[:16], []]
    bad = [[["copy0"]], [["copy0"], [], []], "ab", [["copy0"], "other"], [[3], []], [["copy0", None], []],      # outer length, non-strings
           [[PAD], []], [[STR], []], [[END], []], [[UNK], []],
           [["other"], []], [[], ["copy0"]], [["no-such-word"], []],                                   # another graph's copy token
           [["copy0", "copy0"], []], [[word, "copy1", word], []], [many, []]]
    for c in bad:
        with pytest.raises(ValueError):
            ok(c)
        with pytest.raises(ValueError):
            ok(c, "host")
    for search, groups in (("sample", 1), ("device", 2), ("host", 4)):
        with pytest.raises(ValueError):
            ok([["copy0"], []], search, groups)
    # through work: the checks run before anything of the model is touched
    me = types.SimpleNamespace(vocabs={'predictable_token': pv})
    data = {'local_idx2token': local}
    for kw in (dict(search="sample", seed=1), dict(search="device", groups=2), dict(search="host", groups=2, diversity=0.5)):
        with pytest.raises(ValueError):
            Generator.work(me, data, 4, 10, constraints=[["copy0"], []], **kw)
    for c in bad:
        with pytest.raises(ValueError):
            Generator.work(me, data, 4, 10, search="device", constraints=c)


def test_constrain_entry_point_refuses_bad_arguments(host_lib):
    """-10 outside the shapes, -23 for null pointers; nothing launched, no device needed."""
    from gtos_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert host_lib.max_cons() == ops.CONSTRAIN_MAX

    def adv(B_=2, k=4, Cw=2, t=0, V_=10, tot=10, max_t=5, ld=None, ptrs=None):
        ptrs = ptrs or [p] * 15
        return lib.gtos_constrain_advance(B_, k, Cw, t, V_, tot, 0, max_t, ptrs[0], ptrs[1], ptrs[2], tot if ld is None else ld, *ptrs[3:], None)
    assert adv(k=33) == -10 and adv(k=0) == -10 and adv(Cw=-1) == -10 and adv(Cw=17) == -10
    assert adv(t=5) == -10 and adv(t=-1) == -10 and adv(tot=9) == -10 and adv(V_=0, tot=0) == -10 and adv(ld=9) == -10
    for i in range(15):
        ptrs = [p] * 15
        ptrs[i] = None
        assert adv(ptrs=ptrs, tot=12) == -23, i
    assert adv(B_=0, k=99) == 0


def _dry_tables(B_, k, max_t):
    N = B_ * k
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)         # noqa: E731
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)       # noqa: E731
    return [f64(N), i32(B_, 4), i32(max_t, N), i32(max_t, N), i32(B_, k), i32(B_, k), f64(B_, k), i32(2, N), i32(3)]


def test_ops_check_shapes_under_the_dry_run():
    from dryrun import DryRun
    from gtos_amd import ops, _lib
    with DryRun() as rec:
        B_, k, Cw, max_t, V_, tot = 2, 6, 3, 5, 10, 13
        N = B_ * k
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)     # noqa: E731
        tabs = _dry_tables(B_, k, max_t)
        flags = [torch.zeros(V_, dtype=torch.uint8), torch.zeros(B_, tot - V_, dtype=torch.uint8)]
        top = [torch.zeros(N, k), i32(N, k)]
        ll = torch.zeros(N, tot + 3)[:, :tot]
        ops.constrain_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_, Cw), *flags, *tabs)
        ops.constrain_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_, 0), *flags, *tabs)
        with pytest.raises(AssertionError):
            ops.constrain_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_, 17), *flags, *tabs)
        with pytest.raises(AssertionError):
            ops.constrain_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_ + 1, Cw), *flags, *tabs)
        with pytest.raises(AssertionError):
            ops.constrain_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_, Cw).long(), *flags, *tabs)
        with pytest.raises(AssertionError):
            ops.constrain_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_, Cw), *flags, *tabs[:7], i32(N), tabs[8])          # met [2, N]
        with pytest.raises(_lib.GtosHipError):
            ops.constrain_advance(1, k, V_, tot, 0, max_t, *top, torch.zeros(N, tot + 1), i32(B_, Cw), *flags, *tabs)
        with pytest.raises(_lib.GtosHipError):
            ops.constrain_advance(1, k, V_, tot, 0, max_t, *top, torch.zeros(N, tot).double(), i32(B_, Cw), *flags, *tabs)
    assert rec.names() == ["gtos_constrain_advance"] * 2
    assert rec.calls[0][1][:8] == (B_, k, Cw, 1, V_, tot, 0, max_t) and rec.calls[0][1][11] == tot + 3 and rec.calls[0][1][12] is not None
    assert rec.calls[1][1][2] == 0 and rec.calls[1][1][12] is None


# ------------------------------------------------------------------------------------------------ CPU: launch plans
def test_constrained_device_search_launches_the_new_advance():
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
        word = next(pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END))
        cons = [sorted(local.values())[:2] + [word] if b % 2 else [] for b, local in enumerate(batch['local_idx2token'])]
        width = max(len(c) for c in cons)
        assert width >= 1

        def plan(**kw):
            n0 = len(rec.calls)
            beams = model.work(batch, k, steps, search="device", **kw)
            assert len(beams) == n_graphs
            return beams, rec.calls[n0:]
        _, base = plan()
        names = [c[0] for c in base]
        assert names.count("gtos_beam_topk") == names.count("gtos_beam_advance") == names.count("gtos_beam_reorder") == steps
        assert "gtos_constrain_advance" not in names
        assert [c[0] for c in plan(constraints=None)[1]] == names                               # the default: the plan of today
        beams, calls = plan(constraints=cons)
        got = [c[0] for c in calls]
        assert got == [{"gtos_beam_advance": "gtos_constrain_advance"}.get(x, x) for x in names]   # launch for launch, one of them swapped
        assert got.count("gtos_beam_topk") == got.count("gtos_constrain_advance") == got.count("gtos_beam_reorder") == steps
        adv = [c[1] for c in calls if c[0] == "gtos_constrain_advance"]
        assert [a[:4] for a in adv] == [(n_graphs, k, width, t) for t in range(steps)]
        assert all(hasattr(b, "met") for b in beams)
        _, empty = plan(constraints=[[] for _ in cons])
        assert [c[0] for c in empty] == got and all(c[1][2] == 0 for c in empty if c[0] == "gtos_constrain_advance")
        _, blocked = plan(constraints=cons, no_repeat_ngram=3)
        assert [c[0] for c in blocked if c[0] != "gtos_ngram_block"] == got
        assert [c[0] for c in blocked].count("gtos_ngram_block") == steps - 1
        at = [c[0] for c in blocked]
        assert at.index("gtos_ngram_block") < at.index("gtos_constrain_advance", at.index("gtos_ngram_block"))    # ll is read after the bans
        # the host search through the same glue (numbers mean nothing under the dry run): no device selection kernel, ``met`` per beam
        for kw in (dict(), dict(no_repeat_ngram=2)):
            n0 = len(rec.calls)
            host = model.work(batch, k, steps, constraints=cons, **kw)
            assert len(host) == n_graphs and all(len(b.met) == len(b.hypotheses) for b in host)
            assert not [c[0] for c in rec.calls[n0:] if c[0].startswith(("gtos_beam", "gtos_constrain", "gtos_ngram"))]


# ------------------------------------------------------------------------------------------------ GPU: the advance kernel
@pytest.mark.gpu
@pytest.mark.parametrize("k,c", GPU_SHAPES)
def test_constrain_advance_kernel_matches_the_header(host_lib, k, c):
    """The kernel and the g++ driver over the same random searches: every table equal after every step (the twin), and both equal to
    the Python rule."""
    rng = np.random.RandomState(31 + 100 * k + c)
    n = 0
    for min_t, finite in ((0, False), (2, False), (1, True)):
        n += random_search(rng, gpu_step, k, c, min_t, twin=(host_step(host_lib), Tables(B, k, MAX_T)), finite=finite)
    assert n >= 3 * B


F64_BAND = 0x7FF8A5A5A5A5A5A5


class GuardedTable(object):
    """A table of the advance inside a Guarded allocation: int32 tables live in an fp32 one (the same bits), fp64 ones in their own."""

    def __init__(self, a, dev):
        a2 = np.ascontiguousarray(a).reshape(-1, a.shape[-1])
        init = torch.from_numpy(a2)
        if a.dtype == np.int32:
            self.g = Guarded(a2.shape[0], a2.shape[1], torch.float32, dev, lead=64, trail=64, init=init.view(torch.float32))
            self.view = self.g.view.view(torch.int32).view(*a.shape)
        else:
            self.g = Guarded(a2.shape[0], a2.shape[1], torch.float64, dev, lead=64, trail=64, init=init, band=F64_BAND)
            self.view = self.g.view.view(*a.shape)


@pytest.mark.gpu
@pytest.mark.parametrize("k,c", [(32, 16), (6, 0)])
def test_constrain_advance_stores_inside_its_outputs(host_lib, k, c):
    """Two steps from a state with every slot live (the largest pool: k x (k + c) entries) on tables inside guard bands: the bands
    stay, and the tables equal the g++ driver's, so nothing inside them changed that the rule does not write."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(5 + k + c)
    strings, fs, fl, cons, cons_str = make_world(rng, c)
    host = Tables(B, k, MAX_T)
    t0, N = 3, B * k
    host.active[:] = 0
    host.active[t0 % 3] = 1
    host.state[:] = (t0, 0, k, 0)
    host.slot_score[:] = -0.25 * rng.randint(0, 40, size=N)
    full = np.array([(1 << int((cons[b] >= 0).sum())) - 1 for b in range(B)]).repeat(k)
    host.met[t0 % 2] = rng.randint(0, 1 << 16, size=N) & full
    band = [GuardedTable(a, dev) for a in host.arrays()]
    D = lambda a: torch.from_numpy(a).to(dev)                   # noqa: E731
    for t in (t0, t0 + 1):
        ll = (-0.25 * rng.randint(0, 25, size=(N, TOT))).astype(np.float32)
        ll[rng.rand(N, TOT) < 0.1] = -np.inf
        topv, topi = topk_rows(ll, k)
        host_step(host_lib)(host, cons, t, 1, topv, topi, ll, fs, fl)
        ops.constrain_advance(t, k, V, TOT, 1, MAX_T, D(topv), D(topi), D(ll), D(cons), D(fs), D(fl), *[x.view for x in band])
        for x, a, name in zip(band, host.arrays(), NAMES):
            x.g.check("gtos_constrain_advance %s, step %d" % (name, t))
            assert np.array_equal(x.view.cpu().numpy(), a), (name, t)
    assert int(host.state[:, 0].min()) == t0 + 2 and int(host.state[:, 2].sum()) > 0
    if c:
        assert host.met[(t0 + 2) % 2].any()


# ------------------------------------------------------------------------------------------------ GPU: end to end
def _fixed_word(pv):
    return next(pv.idx2token(i) for i in range(pv.size - 1, -1, -1) if pv.idx2token(i) not in (PAD, UNK, STR, END))


_plain = {}


def plain_and_constraints(k, max_t, min_t):
    """The plain device search of the synthetic C1 fp32 model (once per k) and, per graph, its constraints: two of the graph's copy
    tokens that the plain search's best hypothesis lacks (fewer where it has fewer) plus one fixed vocabulary word."""
    from test_diverse_beam import synth_c1
    if k not in _plain:
        model, batch = synth_c1()
        plain = model.work(batch, k, max_t, min_t, search="device")
        word = _fixed_word(model.vocabs['predictable_token'])
        cons, best = [], []
        for b, beam in enumerate(plain):
            top = beam.get_k_best(1, 0.6)[0]
            copies = [w for _, w in sorted(batch['local_idx2token'][b].items()) if w not in top.seq]
            cons.append(copies[:2] + [word])
            best.append(top)
        _plain[k] = (cons, best)
    return _plain[k]


@pytest.mark.gpu
@pytest.mark.parametrize("k,ngram", [(1, 0), (6, 0), (8, 0), (1, 2), (6, 2), (8, 2)])
def test_constrained_device_search_equals_constrained_host_search_fp32(k, ngram):
    """C1-sized fp32 batch: the two searches pick the same hypotheses in the same order, and the identities of the CPU driver hold
    on what they return."""
    from gtos_amd.search import constraints_met
    from test_diverse_beam import synth_c1, _close
    model, batch = synth_c1()
    max_t, min_t = 12, 1
    cons, best = plain_and_constraints(k, max_t, min_t)
    assert any(len(c) == 3 for c in cons)
    kw = dict(constraints=cons, no_repeat_ngram=ngram)
    host = model.work(batch, k, max_t, min_t, **kw)
    dev = model.work(batch, k, max_t, min_t, search="device", **kw)
    n_full, gaps = 0, []
    for b, (h, d) in enumerate(zip(host, dev)):
        assert h.steps == d.steps, b
        for hl, dl in ((h.hypotheses, d.hypotheses), (h.completed_hypotheses, d.completed_hypotheses)):
            assert [x.seq for x in hl] == [x.seq for x in dl], b
            assert all(_close(x.score, y.score) for x, y in zip(hl, dl)), b
        assert list(h.met) == list(d.met) == [mask_of(x.seq, cons[b]) for x in d.hypotheses], b
        for x in d.completed_hypotheses:
            assert constraints_met(x.seq, cons[b]) == len(cons[b]), (b, x.seq)
        held = d.hypotheses + d.completed_hypotheses
        if not ngram:
            assert any(constraints_met(x.seq, cons[b]) == len(cons[b]) for x in held), b          # min_t = 1 <= c_b <= max_t, finite lls
            if k == 1:
                assert sorted(held[0].seq[1:1 + len(cons[b])]) == sorted(cons[b]), (b, held[0].seq)
        else:
            for x in held:
                y = [w for w in x.seq[1:] if w != END]
                grams = [tuple(y[i:i + ngram]) for i in range(len(y) - ngram + 1)]
                assert len(grams) == len(set(grams)), x.seq
        n_full += any(constraints_met(x.seq, cons[b]) == len(cons[b]) for x in d.completed_hypotheses)
        gaps.append(best[b].score - d.get_k_best(1, 0.6)[0].score)
    print("MEASURED k=%d ngram=%d: %d of %d graphs hold a completed hypothesis with all constraints" % (k, ngram, n_full, len(dev)))
    print("MEASURED k=%d ngram=%d: mean score gap to the plain search's best %.4f" % (k, ngram, sum(gaps) / len(gaps)))


@pytest.mark.gpu
def test_without_constraints_the_new_route_is_the_plain_device_search(monkeypatch):
    from gtos_amd import search
    from test_diverse_beam import synth_c1, _capture_memory
    model, batch = synth_c1()
    memory = _capture_memory(model, batch, monkeypatch)
    n = len(memory['local_idx2token'])
    for k, max_t, min_t, ngram in ((4, 12, 1, 0), (6, 9, 3, 0), (8, 10, 1, 3)):
        out = []
        for kw in (dict(), dict(constrained=True), dict(constraints=[[] for _ in range(n)])):
            beams = [search.Beam(k, min_t, max_t) for _ in range(n)]
            stats = {}
            with torch.no_grad():
                search.beam_search_device(model, memory, beams, stats=stats, no_repeat_ngram=ngram, **kw)
            out.append([(b.steps, pairs(b.hypotheses), pairs(b.completed_hypotheses)) for b in beams] + [stats])
            if kw:
                assert all(not any(b.met) for b in beams)
        assert out[0] == out[1] == out[2], (k, max_t, min_t)
