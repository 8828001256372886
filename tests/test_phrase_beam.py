"""Phrase-constrained beam search (Generator.work(..., phrases=[...]), gtos_amd.search.PhraseBeam, csrc/phrase.hip,
csrc/phrase_kernels.h).

CPU: the rule header compiled with g++ is driven through random multi-step searches next to the Python statement of the rule
(PhraseBeam.advance, fed the same candidate lists and forced log-likelihoods): tables, packed state rows, state words and the continue
flag must agree exactly; identities on the same driver (single-token phrases: the tables of gtos_constrain::advance_serial; no phrases:
those of gtos_beam::advance_serial; a completion holds every phrase; a slot's state is its sequence's replayed; under the stated
conditions a beam ends holding a hypothesis with every phrase, and k = 1 produces the phrases first, each contiguous); a case by hand;
the argument checks; the launch plan under the dry run.
GPU: gtos_phrase_advance against the g++ driver (exact), its stores inside guard bands, work(search="device") against
work(search="host") with phrases, single-token phrases against constraints=, and the route without phrases against the plain device
search."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver, Guarded

DRIVER = r"""
#include "phrase_kernels.h"
// what one gtos_phrase_advance launch does, serially: the flag rotation, every beam by gtos_phrase::advance_serial
extern "C" void phrase_all(int B, int k, int Cw, int Lw, int t, int V, int tot, int min_t, int max_t, const float* topv, const int* topi,
                           const float* ll, long ld, const int* phr, const uint8_t* fs, const uint8_t* fl, double* slot_score,
                           int* state, int* bp_parent, int* bp_token, int* comp_step, int* comp_parent, double* comp_score, int* pst,
                           int* active) {
    using namespace gtos_phrase;
    static double ps[MAX_POOL];
    static int pt[MAX_POOL], pn[MAX_POOL], pq[MAX_POOL], order[MAX_K];
    static uint8_t pf[MAX_POOL];
    static signed char pb[MAX_POOL];
    const long N = (long)B * k;
    active[active_clear(t)] = 0;
    if (!active[active_read(t)]) return;
    for (int b = 0; b < B; ++b)
        if (advance_serial(b, k, Cw, Lw, t, V, tot, min_t, max_t, topv, topi, ll, ld, phr, fs, fl, slot_score, state, bp_parent + t * N,
                           bp_token + t * N, comp_step, comp_parent, comp_score, pst + (t % 2) * N, pst + ((t + 1) % 2) * N, ps, pt, pf,
                           pn, pb, pq, order))
            active[active_set(t)] |= 1;
}
// ... one gtos_constrain_advance launch (csrc/constrain_kernels.h), for the identity with single-token phrases
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
// ... and one gtos_beam_advance launch (csrc/beam_kernels.h), for the identity without phrases
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
// how the rule reads one graph's rows: c, T and the lengths
extern "C" int read_phrases(const int* phr_b, int Cw, int Lw, int tot, int* total, int* len) {
    gtos_phrase::PhraseSet s;
    gtos_phrase::load_phrases(&s, phr_b, Cw, Lw, tot);
    *total = s.total;
    for (int i = 0; i < s.c; ++i) len[i] = s.len[i];
    return s.c;
}
extern "C" int max_phr() { return gtos_phrase::MAX_PHR; }
extern "C" int max_len() { return gtos_phrase::MAX_LEN; }
extern "C" int max_tokens() { return gtos_phrase::MAX_TOKENS; }
"""

PAD, UNK, STR, END = "<PAD>", "<UNK>", "<STR>", "<END>"
SHAPES = [(1, 1, 1), (4, 3, 3), (6, 0, 1), (8, 16, 4), (32, 16, 4)]      # (k, phrases, longest phrase)
GPU_SHAPES = [(1, 1, 1), (6, 2, 3), (8, 16, 4), (32, 16, 4)]             # ... (32, 16, 4): a pool of up to 1536 entries, 64 bank levels
B, V, TOT, MAX_T = 3, 23, 57, 18
LONG_T = 70                                                              # above the 64 tokens a graph's phrases may hold together
NAMES = ("slot_score", "state", "bp_parent", "bp_token", "comp_step", "comp_parent", "comp_score", "pst", "active")


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = compile_host_driver(tmp_path_factory, "phrase_host", DRIVER)
    lib.phrase_all.argtypes = [ctypes.c_int] * 9 + [ctypes.c_void_p] * 3 + [ctypes.c_long] + [ctypes.c_void_p] * 12
    lib.phrase_all.restype = None
    lib.constrain_all.argtypes = [ctypes.c_int] * 8 + [ctypes.c_void_p] * 3 + [ctypes.c_long] + [ctypes.c_void_p] * 12
    lib.constrain_all.restype = None
    lib.plain_all.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 12
    lib.plain_all.restype = None
    return lib


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a.size else None


def pack(met, open_, pos):
    """the packed state word of csrc/phrase_kernels.h"""
    return met | (open_ + 1) << 16 | pos << 21


class Tables(object):
    """The tables of a phrase-constrained device search as numpy arrays: the plain search's plus pst [2, N]."""

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
        self.pst = np.zeros((2, N), dtype=np.int32)

    def arrays(self):
        return [self.slot_score, self.state, self.bp_parent, self.bp_token, self.comp_step, self.comp_parent, self.comp_score, self.pst,
                self.active]

    def plain_arrays(self):
        return [a for a, n in zip(self.arrays(), NAMES) if n != "pst"]

    def beams(self, strings, min_t):
        from gtos_amd.search import Beam, fill_beams
        beams = [Beam(self.k, min_t, self.max_t) for _ in range(self.B)]
        return fill_beams(beams, self.k, self.state.ravel().tolist(), self.bp_parent.ravel().tolist(), self.bp_token.ravel().tolist(),
                          self.comp_step.ravel().tolist(), self.comp_parent.ravel().tolist(), self.slot_score.tolist(),
                          self.comp_score.ravel().tolist(), lambda b, i: strings[b][i])


def host_step(lib):
    def step(tab, phr, t, min_t, topv, topi, ll, fs, fl):
        lib.phrase_all(tab.B, tab.k, phr.shape[1], phr.shape[2], t, V, TOT, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(ll),
                       ll.shape[1], _np_ptr(phr), _np_ptr(fs), _np_ptr(fl), *[_np_ptr(a) for a in tab.arrays()])
    return step


def constrain_step(lib):
    """gtos_constrain's advance on the phrases' first ids (the twin of a search whose phrases hold one token each)"""
    def step(tab, phr, t, min_t, topv, topi, ll, fs, fl):
        cons = np.ascontiguousarray(phr[:, :, 0])
        lib.constrain_all(tab.B, tab.k, cons.shape[1], t, V, TOT, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(ll), ll.shape[1],
                          _np_ptr(cons), _np_ptr(fs), _np_ptr(fl), *[_np_ptr(a) for a in tab.arrays()])
    return step


def plain_step(lib):
    def step(tab, phr, t, min_t, topv, topi, ll, fs, fl):
        lib.plain_all(tab.B, tab.k, t, V, TOT, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(fs), _np_ptr(fl),
                      *[_np_ptr(a) for a in tab.plain_arrays()])
    return step


def gpu_step(tab, phr, t, min_t, topv, topi, ll, fs, fl):
    """The same step on the device kernel: tables up, one gtos_phrase_advance (ll with a leading dimension above its width), tables
    down."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    g = [torch.from_numpy(a).to(dev) for a in tab.arrays()]
    wide = torch.full((ll.shape[0], TOT + 5), float("nan"), dtype=torch.float32, device=dev)
    wide[:, :TOT] = torch.from_numpy(ll).to(dev)
    ops.phrase_advance(t, tab.k, V, TOT, min_t, tab.max_t, torch.from_numpy(topv).to(dev), torch.from_numpy(topi).to(dev),
                       wide[:, :TOT], torch.from_numpy(phr).to(dev), torch.from_numpy(fs).to(dev), torch.from_numpy(fl).to(dev), *g)
    for a, x in zip(tab.arrays(), g):
        a[...] = x.cpu().numpy()


def pairs(hyps):
    return [(h.seq, h.score) for h in hyps]


def topk_rows(ll, k):
    """(values, columns) [N, k] of ll's rows, descending, equal values lower column first: what gtos_beam_topk returns."""
    order = np.lexsort((np.broadcast_to(np.arange(ll.shape[1]), ll.shape), -ll.astype(np.float64)), axis=1)[:, :k]
    return np.take_along_axis(ll, order, 1).astype(np.float32), order.astype(np.int32)


def make_world(rng, c, L, none_for=(), single=False):
    """Strings and classes of B graphs' output ids (every class occurs: <UNK> and <END> as vocabulary ids, <END> also as copy strings;
    the strings that can survive are unique within a graph) and their phrases: graph 0 has c, its first of L tokens, the others a random
    number up to c (``none_for``: graphs without any) of 1 .. L tokens.  A phrase's tokens come from six plain ids of the graph, so that
    phrases share first tokens and repeat tokens inside; one phrase in four repeats an earlier one (``single``: one distinct token each
    instead).  -> strings, fs, fl, phr int32 [B, c, L], the phrases as strings"""
    words = [PAD, UNK, END] + ["w%d" % i for i in range(V - 3)]
    strings = [words + [END if rng.rand() < 0.3 else "c%d" % j for j in range(TOT - V)] for _ in range(B)]
    cls = lambda w: 1 if w == UNK else 2 if w == END else 0         # noqa: E731
    fs = np.array([cls(w) for w in words], dtype=np.uint8)
    fl = np.array([[cls(w) for w in s[V:]] for s in strings], dtype=np.uint8).reshape(B, TOT - V)
    phr = np.full((B, c, L), -1, dtype=np.int32)
    for b in range(B):
        n = 0 if b in none_for else c if b == 0 else int(rng.randint(0, c + 1))
        ok = [i for i, w in enumerate(strings[b]) if cls(w) == 0 and w != PAD]
        if single:
            phr[b, :n, 0] = rng.choice(ok, size=n, replace=False)
            continue
        alphabet = rng.choice(ok, size=6, replace=False)
        for i in range(n):
            if i and rng.rand() < 0.25:
                phr[b, i] = phr[b, rng.randint(0, i)]
            else:
                length = L if (b == 0 and i == 0) else int(rng.randint(1, L + 1))
                phr[b, i, :length] = rng.choice(alphabet, size=length)
    return strings, fs, fl, phr, [[[strings[b][i] for i in row if i >= 0] for row in phr[b] if row[0] >= 0] for b in range(B)]


def bank_of(phrases, met, open_, pos):
    return sum(len(p) for i, p in enumerate(phrases) if (met >> i) & 1) + pos


def random_search(rng, step_fn, k, c, L, min_t, max_t=MAX_T, twin=None, finite=False, none_for=(), plain_twin=None, single=False):
    """One multi-step phrase-constrained search of B graphs: the Python rule (search.PhraseBeam) and step_fn (the fixed-slot tables) fed
    the same ll rows [N, TOT] -- multiples of 0.25 so that ties occur, some columns -inf (``finite``: never a phrase token's) -- their
    top-k and, per phrase token, the ll of its column.
    ``twin`` = (step function, Tables): a second implementation whose tables must stay equal.  ``plain_twin`` = (plain step function,
    Tables): gtos_beam's advance fed the same top-k; the graphs without phrases must get its tables.
    Asserts after every step: state words, back-pointer rows, the state row written, the continue flag, the beams rebuilt from the
    tables, a live state is its sequence's replayed (phrase_state), a completion replays to a full mask.  At the end, with finite lls
    and min_t <= T_b <= max_t (T_b: the tokens of the graph's phrases): the beam holds a hypothesis whose replay is full, and with k = 1
    the first T_b tokens raise the bank by one each -- they are the phrases, each contiguous.
    Returns the number of beam advances compared."""
    from gtos_amd.search import PhraseBeam, phrase_state
    strings, fs, fl, phr, phr_str = make_world(rng, c, L, none_for, single)
    tab = Tables(B, k, max_t)
    beams = [PhraseBeam(k, min_t, max_t, phr_str[b]) for b in range(B)]
    full = [(1 << len(p)) - 1 for p in phr_str]
    tokens = [sorted(set(int(i) for i in phr[b].ravel() if i >= 0)) for b in range(B)]
    N = B * k
    n_adv, t = 0, 0
    while True:
        got = tab.beams(strings, min_t)
        for b, (g, w) in enumerate(zip(got, beams)):
            assert g.steps == w.steps and pairs(g.hypotheses) == pairs(w.hypotheses), ("alive before step %d" % t, b)
            assert pairs(g.completed_hypotheses) == pairs(w.completed_hypotheses), ("completed before step %d" % t, b)
        if not any(beam.hypotheses for beam in beams if not beam.completed()):
            break
        assert t < max_t
        ll = (-0.25 * rng.randint(0, 25, size=(N, TOT))).astype(np.float32)
        ll[rng.rand(N, TOT) < 0.1] = -np.inf
        if finite:
            for s in range(N):
                ids = tokens[s // k]
                ll[s, ids] = np.where(np.isinf(ll[s, ids]), np.float32(-6.25), ll[s, ids])
        topv, topi = topk_rows(ll, k)
        was = [(beam.completed(), len(beam.hypotheses)) for beam in beams]
        for b, beam in enumerate(beams):
            if beam.completed():
                continue
            slots = range(b * k, b * k + len(beam.hypotheses))
            rows = [[(strings[b][int(i)], float(v)) for v, i in zip(topv[s], topi[s])] for s in slots]
            forced = [{strings[b][i]: float(ll[s, i]) for i in tokens[b]} for s in slots]
            beam.last_parents = beam.advance(rows, forced)
            n_adv += 1
        flags = tab.active.copy()
        step_fn(tab, phr, t, min_t, topv, topi, ll, fs, fl)
        if twin:
            twin[0](twin[1], phr, t, min_t, topv, topi, ll, fs, fl)
            for a, a2, name in zip(tab.arrays(), twin[1].arrays(), NAMES):
                assert np.array_equal(a.ravel(), a2.ravel(), equal_nan=True), ("twin tables", name, t)
        if plain_twin:
            other = plain_twin[1]
            other.active[:] = flags                                 # (the flag is shared by the graphs: the plain search follows ours)
            plain_twin[0](other, phr, t, min_t, topv, topi, ll, fs, fl)
            free = [b for b in range(B) if not phr_str[b]]
            assert free
            for b in free:
                own = slice(b * k, b * k + k)
                for name in ("state", "comp_step", "comp_parent", "comp_score"):
                    assert np.array_equal(getattr(tab, name)[b], getattr(other, name)[b]), ("plain tables", name, b, t)
                for name in ("bp_parent", "bp_token"):
                    assert np.array_equal(getattr(tab, name)[:, own], getattr(other, name)[:, own]), ("plain tables", name, b, t)
                assert np.array_equal(tab.slot_score[own], other.slot_score[own]), ("plain tables", "slot_score", b, t)
                assert not tab.pst[:, own].any()
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
                want = [pack(m, o, p) for m, (o, p) in zip(beam.met, beam.progress)]
                assert tab.pst[(t + 1) % 2, at:at + len(par)].tolist() == want, ("packed states", t, b)
                assert not tab.pst[(t + 1) % 2, at + len(par):at + k].any(), ("states of dead slots", t, b)
            else:
                assert (tab.bp_parent[t, at:at + k] == -1).all(), ("a done beam's row", t, b)
            assert [phrase_state(h.seq, phr_str[b]) for h in beam.hypotheses] == [(m,) + tuple(p) for m, p in zip(beam.met, beam.progress)], \
                ("state replayed", t, b)
            for h in beam.completed_hypotheses:
                assert phrase_state(h.seq, phr_str[b])[0] == full[b], ("a completion lacks a phrase", t, b, h.seq)
            go |= not beam.completed() and len(beam.hypotheses) > 0
        assert int(tab.active[(t + 1) % 3]) == int(go) and int(tab.active[(t + 2) % 3]) == 0, ("continue flag", t)
        t += 1
    # the device loop keeps launching steps up to max_t: they must change nothing
    snap = [a.copy() for a in tab.arrays()[:-1]]
    for t2 in range(t, min(max_t, t + 3)):
        step_fn(tab, phr, t2, min_t, np.zeros((N, k), np.float32), np.zeros((N, k), np.int32), np.zeros((N, TOT), np.float32), fs, fl)
    for a, b_ in zip(tab.arrays()[:-1], snap):
        assert np.array_equal(a, b_, equal_nan=True), "a step after the end changed the tables"
    if finite:
        for b, beam in enumerate(beams):
            T = sum(len(p) for p in phr_str[b])
            held = beam.hypotheses + beam.completed_hypotheses
            if not min_t <= T <= max_t:
                continue
            assert any(phrase_state(h.seq, phr_str[b])[0] == full[b] for h in held), ("no hypothesis holds every phrase", b)
            if k == 1:
                h = held[0]
                for j in range(T + 1):
                    assert bank_of(phr_str[b], *phrase_state(h.seq[1:1 + j], phr_str[b])) == j, ("k = 1: the phrases come first", b, h.seq)
    return n_adv


# ------------------------------------------------------------------------------------------------ CPU: the header
@pytest.mark.parametrize("k,c,L", SHAPES)
def test_rule_header_matches_the_python_rule(host_lib, k, c, L):
    step = host_step(host_lib)
    rng = np.random.RandomState(20261019 + 100 * k + 10 * c + L)
    n = 0
    for rep in range(4 if k == 32 else 6):
        n += random_search(rng, step, k, c, L, min_t=rep % 4)
    assert n >= 4 * B


def test_the_random_phrases_cover_the_hard_cases():
    """What make_world promises: duplicates, shared first tokens and repeated tokens inside a phrase all occur."""
    rng = np.random.RandomState(1)
    dup = shared = inside = 0
    for _ in range(5):
        phr_str = make_world(rng, 16, 4)[4]
        for ps in phr_str:
            t = [tuple(p) for p in ps]
            dup += len(set(t)) < len(t)
            shared += len(set(p[0] for p in set(t))) < len(set(t))
            inside += any(len(set(p)) < len(p) for p in t)
    assert dup and shared and inside


@pytest.mark.parametrize("k,c", [(1, 1), (4, 3), (8, 16), (32, 16)])
def test_single_token_phrases_give_the_constrained_search_s_tables(host_lib, k, c):
    """Lw = 1, distinct ids: every table equals gtos_constrain::advance_serial's step by step, the packed state being the mask."""
    rng = np.random.RandomState(909 + 100 * k + c)
    for min_t in (0, 2):
        assert random_search(rng, host_step(host_lib), k, c, 1, min_t, twin=(constrain_step(host_lib), Tables(B, k, MAX_T)), single=True) > 0


@pytest.mark.parametrize("k", [1, 5, 8, 32])
def test_without_phrases_the_tables_are_the_plain_search_s(host_lib, k):
    """Cw = 0, and Cw > 0 with graphs whose rows are all -1: those graphs get the tables of gtos_beam::advance_serial step by step."""
    rng = np.random.RandomState(404 + k)
    for min_t in (0, 2):
        assert random_search(rng, host_step(host_lib), k, 0, 1, min_t, none_for=(0, 1, 2), plain_twin=(plain_step(host_lib), Tables(B, k, MAX_T))) > 0
        assert random_search(rng, host_step(host_lib), k, 3, 3, min_t, none_for=(1,), plain_twin=(plain_step(host_lib), Tables(B, k, MAX_T))) > 0


@pytest.mark.parametrize("k,c,L", [(1, 1, 1), (1, 5, 3), (1, 16, 4), (4, 3, 3), (8, 16, 4), (32, 16, 4), (6, 2, 3), (2, 4, 2), (5, 5, 4)])
def test_phrases_are_met_when_their_lls_are_finite(host_lib, k, c, L):
    """(the assertions sit in random_search: every completion replays to a full mask; under min_t <= T_b <= max_t every beam ends
    holding a hypothesis, live or completed, with every phrase, and k = 1 produces the phrases first, each contiguous)"""
    rng = np.random.RandomState(777 + 100 * k + 10 * c + L)
    for min_t in (0, 1):
        assert random_search(rng, host_step(host_lib), k, c, L, min_t, max_t=LONG_T if c * L > MAX_T else MAX_T, finite=True) > 0


def test_how_the_header_reads_a_graph_s_rows(host_lib):
    """-1 or an id outside [0, tot) ends a phrase, an empty phrase ends the list, and so does the phrase that would take the graph past
    MAX_TOKENS ids: the bank of any state the kernel can reach fits the pool's signed byte."""
    def read(rows, tot=50):
        phr = np.array(rows, dtype=np.int32)
        total, lens = ctypes.c_int(0), (ctypes.c_int * 16)()
        c = host_lib.read_phrases(_np_ptr(phr), phr.shape[0], phr.shape[1], tot, ctypes.byref(total), lens)
        return c, total.value, list(lens[:c])
    assert read([[3, 4, -1], [5, -1, 7], [8, 9, 10]]) == (3, 6, [2, 1, 3])
    assert read([[3, 50, 4], [49, 0, -1]]) == (2, 3, [1, 2])                     # 50 is outside [0, 50)
    assert read([[3, 4], [-1, 5], [6, 7]]) == (1, 2, [2])                        # an empty phrase ends the list
    assert read([[60, 1], [2, 3]]) == (0, 0, [])
    assert read([[1] * 5] * 16) == (12, 60, [5] * 12)                            # the 13th would make 65
    assert read([[1] * 4] * 16) == (16, 64, [4] * 16)
    assert read([[1] * 16] * 5) == (4, 64, [16] * 4)


def test_python_rule_by_hand():
    """k = 1, one phrase (x, y): x is forced; y is not available, so the next token drops the open phrase and the bank falls from 1 to
    0; the phrase starts again, finishes, and only then may the hypothesis end.  No failure links."""
    from gtos_amd.search import PhraseBeam, phrase_state, phrase_step
    ninf = float("-inf")
    beam = PhraseBeam(1, 0, 9, [["x", "y"]])
    assert beam.advance([[("a", -1.0)]], [{"x": -5.0, "y": -1.0}]) == [0]
    assert pairs(beam.hypotheses) == [([STR, "x"], -5.0)] and beam.met == [0] and beam.progress == [(0, 1)]       # bank 1 beats bank 0
    assert beam.bank(0, 0, 1) == 1
    assert beam.advance([[("c", -0.5)]], [{"x": -1.0, "y": ninf}]) == [0]                                         # y = -inf: not forced
    assert pairs(beam.hypotheses) == [([STR, "x", "c"], -5.5)] and beam.met == [0] and beam.progress == [(-1, 0)]
    assert beam.bank(0, -1, 0) == 0                                                                                  # ... the bank fell
    assert beam.advance([[(END, -0.1)]], [{"x": -2.0, "y": -1.0}]) == [0]                                         # <END> held back, x forced
    assert pairs(beam.hypotheses) == [([STR, "x", "c", "x"], -7.5)] and beam.progress == [(0, 1)]
    assert beam.advance([[("y", -0.25)]], [{"x": -2.0, "y": -0.25}]) == [0]                                       # y in the top-k: not twice
    assert pairs(beam.hypotheses) == [([STR, "x", "c", "x", "y"], -7.75)] and beam.met == [1] and beam.progress == [(-1, 0)]
    assert beam.advance([[(END, -0.25)]], [{"x": -2.0, "y": -2.0}]) == []
    assert pairs(beam.completed_hypotheses) == [([STR, "x", "c", "x", "y", END], -8.0)]
    # k = 2, a phrase listed twice and a phrase sharing its first token: one forced candidate per token; the lowest unmet index starts
    beam = PhraseBeam(2, 0, 9, [["x", "y"], ["x", "y"], ["x"]])
    assert beam.advance([[("a", -1.0), ("b", -2.0)]], [{"x": -5.0, "y": -1.0}]) == [0, 0]
    assert pairs(beam.hypotheses) == [([STR, "x"], -5.0), ([STR, "a"], -1.0)] and beam.progress == [(0, 1), (-1, 0)]
    assert beam.advance([[("b", -1.0), ("a", -2.0)], [("b", -1.0), ("a", -2.0)]], [{"x": -9.0, "y": -1.0}] * 2) == [0, 1]
    assert pairs(beam.hypotheses) == [([STR, "x", "y"], -6.0), ([STR, "a", "x"], -10.0)] and beam.met == [1, 0]
    assert beam.progress == [(-1, 0), (0, 1)]
    # the transition on its own
    assert phrase_state(["a", "a", "a", "b"], [["a", "a", "b"]]) == (0, -1, 0)                  # no failure links: not found
    assert phrase_state(["a", "a", "b"], [["a", "a", "b"]]) == (1, -1, 0)
    assert phrase_state([STR, "x", "y", "x", "y", "x"], [["x", "y"], ["x", "y"], ["x"]]) == (7, -1, 0)
    assert phrase_state([STR, "x", "y", "x"], [["x", "y"], ["x", "y"], ["x"]]) == (1, 1, 1)
    assert phrase_state([], []) == (0, -1, 0) and phrase_step([["q"]], 0, -1, 0, "q") == (1, -1, 0)


# ------------------------------------------------------------------------------------------------ CPU: argument checks
def test_check_phrases():
    from gtos_amd import ops, synth
    from gtos_amd.generator import Generator, check_phrases
    pv = synth.synth_vocabs()['predictable_token']
    plain = [pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END)]
    word = plain[0]
    local = [{pv.size: "copy0", pv.size + 1: "copy1"}, {pv.size: "other"}]
    ok = lambda p, search="device", groups=1, cons=None, cov=None: check_phrases(p, search, groups, cons, cov, local, pv)      # noqa: E731
    assert ok(None) is None and ok(None, "sample", 2, [["copy0"], []], 0.5) is None
    assert ok([[["copy0", word], ["copy1"]], []]) == [[["copy0", word], ["copy1"]], []]
    assert ok(([("copy1", "copy1")], [["other"], ["other"]]), "host") == [[["copy1", "copy1"]], [["other"], ["other"]]]      # twice: allowed
    assert (ops.PHRASE_MAX, ops.PHRASE_LEN_MAX, ops.PHRASE_TOKENS_MAX) == (16, 16, 64)
    assert ok([[[word]] * 16, []]) and ok([[[word] * 16] * 4, []]) and ok([[plain[:16]], []])
    bad = [[[["copy0"]]], [[["copy0"]], [], []], "ab",                                                 # outer length
           [[["copy0"]], "other"], [{"copy0": 1}, []], [[["copy0"]], None],                            # a graph entry that is no list
           [["copy0"], []], [[["copy0"], "copy1"], []], [[[]], []], [[()], []], [[["copy0", 3]], []], [[[None]], []], [[3], []],
           [[[PAD]], []], [[["copy0", STR]], []], [[[END]], []], [[[word, UNK]], []],
           [[["other"]], []], [[], [["copy0"]]], [[["copy0", "no-such-word"]], []],                    # another graph's copy token
           [[[word]] * 17, []], [[[word] * 17], []], [[[word] * 13] * 5, []]]                          # 17 phrases, 17 tokens, 65 in total
    for p in bad:
        with pytest.raises(ValueError):
            ok(p)
        with pytest.raises(ValueError):
            ok(p, "host")
    good = [[["copy0"]], []]
    for search, groups, cons, cov in (("sample", 1, None, None), ("device", 2, None, None), ("host", 4, None, None),
                                      ("device", 1, [["copy0"], []], None), ("host", 1, [[], []], None), ("device", 1, None, 0.0),
                                      ("host", 1, None, 0.5)):
        with pytest.raises(ValueError):
            ok(good, search, groups, cons, cov)
    # through work: the checks run before anything of the model is touched
    me = types.SimpleNamespace(vocabs={'predictable_token': pv})
    data = {'local_idx2token': local}
    for kw in (dict(search="sample", seed=1), dict(search="device", groups=2), dict(search="host", groups=2, diversity=0.5),
               dict(search="device", constraints=[["copy0"], []]), dict(search="host", coverage_penalty=0.2)):
        with pytest.raises(ValueError):
            Generator.work(me, data, 4, 10, phrases=good, **kw)
    for p in bad:
        with pytest.raises(ValueError):
            Generator.work(me, data, 4, 10, search="device", phrases=p)


def test_phrase_entry_point_refuses_bad_arguments(host_lib):
    """-10 outside the shapes, -23 for null pointers; nothing launched, no device needed."""
    from gtos_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert (host_lib.max_phr(), host_lib.max_len(), host_lib.max_tokens()) == (ops.PHRASE_MAX, ops.PHRASE_LEN_MAX, ops.PHRASE_TOKENS_MAX)
    assert _lib.ABI_VERSION >= 30

    def adv(B_=2, k=4, Cw=2, Lw=3, t=0, V_=10, tot=10, max_t=5, ld=None, ptrs=None):
        ptrs = ptrs or [p] * 15
        return lib.gtos_phrase_advance(B_, k, Cw, Lw, t, V_, tot, 0, max_t, ptrs[0], ptrs[1], ptrs[2], tot if ld is None else ld, *ptrs[3:], None)
    assert adv(k=33) == -10 and adv(k=0) == -10 and adv(Cw=-1) == -10 and adv(Cw=17) == -10
    assert adv(Lw=17) == -10 and adv(Lw=-1) == -10 and adv(Lw=0) == -10
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
        B_, k, Cw, Lw, max_t, V_, tot = 2, 6, 3, 4, 5, 10, 13
        N = B_ * k
        i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)     # noqa: E731
        tabs = _dry_tables(B_, k, max_t)
        flags = [torch.zeros(V_, dtype=torch.uint8), torch.zeros(B_, tot - V_, dtype=torch.uint8)]
        top = [torch.zeros(N, k), i32(N, k)]
        ll = torch.zeros(N, tot + 3)[:, :tot]
        ops.phrase_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_, Cw, Lw), *flags, *tabs)
        ops.phrase_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_, 0, 1), *flags, *tabs)
        for phr in (i32(B_, 17, Lw), i32(B_, Cw, 17), i32(B_, Cw, 0), i32(B_ + 1, Cw, Lw), i32(B_, Cw), i32(B_, Cw, Lw).long()):
            with pytest.raises(AssertionError):
                ops.phrase_advance(1, k, V_, tot, 0, max_t, *top, ll, phr, *flags, *tabs)
        with pytest.raises(AssertionError):
            ops.phrase_advance(1, k, V_, tot, 0, max_t, *top, ll, i32(B_, Cw, Lw), *flags, *tabs[:7], i32(N), tabs[8])         # pst [2, N]
        with pytest.raises(_lib.GtosHipError):
            ops.phrase_advance(1, k, V_, tot, 0, max_t, *top, torch.zeros(N, tot + 1), i32(B_, Cw, Lw), *flags, *tabs)
        with pytest.raises(_lib.GtosHipError):
            ops.phrase_advance(1, k, V_, tot, 0, max_t, *top, torch.zeros(N, tot).double(), i32(B_, Cw, Lw), *flags, *tabs)
    assert rec.names() == ["gtos_phrase_advance"] * 2
    assert rec.calls[0][1][:9] == (B_, k, Cw, Lw, 1, V_, tot, 0, max_t) and rec.calls[0][1][12] == tot + 3 and rec.calls[0][1][13] is not None
    assert rec.calls[1][1][2] == 0 and rec.calls[1][1][13] is None


# ------------------------------------------------------------------------------------------------ CPU: launch plans
def test_phrase_device_search_launches_the_new_advance():
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
        own = [sorted(local.values()) + [word, word] for local in batch['local_idx2token']]         # (a graph may have no copy token)
        phrases = [[cp_[:2], [word], [word, cp_[0], word]] if b % 2 else [] for b, cp_ in enumerate(own)]
        Cw, Lw = 3, 3
        assert any(phrases)

        def plan(**kw):
            n0 = len(rec.calls)
            beams = model.work(batch, k, steps, search="device", **kw)
            assert len(beams) == n_graphs
            return beams, rec.calls[n0:]
        _, base = plan()
        names = [c[0] for c in base]
        assert names.count("gtos_beam_topk") == names.count("gtos_beam_advance") == names.count("gtos_beam_reorder") == steps
        assert "gtos_phrase_advance" not in names
        assert [c[0] for c in plan(phrases=None)[1]] == names                                    # the default: the plan of today
        beams, calls = plan(phrases=phrases)
        got = [c[0] for c in calls]
        assert got == [{"gtos_beam_advance": "gtos_phrase_advance"}.get(x, x) for x in names]    # launch for launch, one of them swapped
        assert got.count("gtos_beam_topk") == got.count("gtos_phrase_advance") == got.count("gtos_beam_reorder") == steps
        for t in range(steps):                                                                   # between the plain top-k and reorder
            at = [i for i, x in enumerate(got) if x == "gtos_phrase_advance"][t]
            assert got[at - 1] == "gtos_beam_topk" and got[at + 1] == "gtos_beam_reorder"
        adv = [c[1] for c in calls if c[0] == "gtos_phrase_advance"]
        assert [a[:5] for a in adv] == [(n_graphs, k, Cw, Lw, t) for t in range(steps)]
        assert all(len(b.met) == len(b.progress) == len(b.hypotheses) for b in beams)
        _, empty = plan(phrases=[[] for _ in phrases])
        assert [c[0] for c in empty] == got and all(c[1][2] == 0 and c[1][13] is None for c in empty if c[0] == "gtos_phrase_advance")
        _, blocked = plan(phrases=phrases, no_repeat_ngram=3)
        assert [c[0] for c in blocked if c[0] != "gtos_ngram_block"] == got
        assert [c[0] for c in blocked].count("gtos_ngram_block") == steps - 1
        at = [c[0] for c in blocked]
        assert at.index("gtos_ngram_block") < at.index("gtos_phrase_advance", at.index("gtos_ngram_block"))      # ll is read after the bans
        # the host search through the same glue (numbers mean nothing under the dry run): no device selection kernel, states per beam
        for kw in (dict(), dict(no_repeat_ngram=2)):
            n0 = len(rec.calls)
            host = model.work(batch, k, steps, phrases=phrases, **kw)
            assert len(host) == n_graphs and all(len(b.met) == len(b.progress) == len(b.hypotheses) for b in host)
            assert not [c[0] for c in rec.calls[n0:] if c[0].startswith(("gtos_beam", "gtos_constrain", "gtos_phrase", "gtos_ngram"))]


# ------------------------------------------------------------------------------------------------ GPU: the advance kernel
@pytest.mark.gpu
@pytest.mark.parametrize("k,c,L", GPU_SHAPES)
def test_phrase_advance_kernel_matches_the_header(host_lib, k, c, L):
    """The kernel and the g++ driver over the same random searches: every table equal after every step (the twin), and both equal to
    the Python rule."""
    rng = np.random.RandomState(31 + 100 * k + 10 * c + L)
    n = 0
    for min_t, finite in ((0, False), (2, False), (1, True)):
        n += random_search(rng, gpu_step, k, c, L, min_t, twin=(host_step(host_lib), Tables(B, k, MAX_T)), finite=finite)
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


def random_states(rng, phr, k):
    """A valid packed state per slot: a random mask of the graph's phrases and, for half of the slots, an unmet phrase of more than one
    token open at a random position"""
    out = np.zeros(phr.shape[0] * k, dtype=np.int32)
    for s in range(out.size):
        rows = phr[s // k]
        lens = [int((r >= 0).sum()) for r in rows if r[0] >= 0]
        met = int(rng.randint(0, 1 << 16)) & ((1 << len(lens)) - 1)
        can = [i for i, n in enumerate(lens) if n > 1 and not (met >> i) & 1]
        if can and rng.rand() < 0.5:
            i = can[rng.randint(len(can))]
            out[s] = pack(met, i, int(rng.randint(1, lens[i])))
        else:
            out[s] = pack(met, -1, 0)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("k,c,L", [(32, 16, 4), (6, 0, 1)])
def test_phrase_advance_stores_inside_its_outputs(host_lib, k, c, L):
    """Two steps from a state with every slot live (the largest pool: k x (k + c) entries) on tables inside guard bands: the bands
    stay, and the tables equal the g++ driver's, so nothing inside them changed that the rule does not write."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(5 + k + c)
    strings, fs, fl, phr, phr_str = make_world(rng, c, L)
    host = Tables(B, k, MAX_T)
    t0, N = 3, B * k
    host.active[:] = 0
    host.active[t0 % 3] = 1
    host.state[:] = (t0, 0, k, 0)
    host.slot_score[:] = -0.25 * rng.randint(0, 40, size=N)
    host.pst[t0 % 2] = random_states(rng, phr, k)
    band = [GuardedTable(a, dev) for a in host.arrays()]
    D = lambda a: torch.from_numpy(a).to(dev)                   # noqa: E731
    for t in (t0, t0 + 1):
        ll = (-0.25 * rng.randint(0, 25, size=(N, TOT))).astype(np.float32)
        ll[rng.rand(N, TOT) < 0.1] = -np.inf
        topv, topi = topk_rows(ll, k)
        host_step(host_lib)(host, phr, t, 1, topv, topi, ll, fs, fl)
        ops.phrase_advance(t, k, V, TOT, 1, MAX_T, D(topv), D(topi), D(ll), D(phr), D(fs), D(fl), *[x.view for x in band])
        for x, a, name in zip(band, host.arrays(), NAMES):
            x.g.check("gtos_phrase_advance %s, step %d" % (name, t))
            assert np.array_equal(x.view.cpu().numpy(), a), (name, t)
    assert int(host.state[:, 0].min()) == t0 + 2 and int(host.state[:, 2].sum()) > 0
    if c:
        assert host.pst[(t0 + 2) % 2].any() and (host.pst[(t0 + 2) % 2] >> 16).any()           # masks, and phrases in progress


# ------------------------------------------------------------------------------------------------ GPU: end to end
def _fixed_words(pv):
    return [pv.idx2token(i) for i in range(pv.size - 1, -1, -1) if pv.idx2token(i) not in (PAD, UNK, STR, END)][:2]


_plain = {}


def plain_and_phrases(k, max_t, min_t):
    """The plain device search of the synthetic C1 fp32 model (once per k) and, per graph, its three phrases (six tokens): two of the
    graph's copy tokens that the plain search's best hypothesis lacks (topped up with its other copy tokens); a vocabulary word between
    two copy tokens; one single vocabulary word."""
    from test_diverse_beam import synth_c1
    if k not in _plain:
        model, batch = synth_c1()
        plain = model.work(batch, k, max_t, min_t, search="device")
        w0, w1 = _fixed_words(model.vocabs['predictable_token'])
        phrases, best = [], []
        for b, beam in enumerate(plain):
            top = beam.get_k_best(1, 0.6)[0]
            copies = [w for _, w in sorted(batch['local_idx2token'][b].items())]
            assert len(copies) >= 2
            lacking = [w for w in copies if w not in top.seq] + [w for w in copies if w in top.seq]
            phrases.append([lacking[:2], [copies[-1], w0, copies[0]], [w1]])
            best.append(top)
        _plain[k] = (phrases, best)
    return _plain[k]


@pytest.mark.gpu
@pytest.mark.parametrize("k,ngram", [(1, 0), (6, 0), (8, 0), (1, 2), (6, 2), (8, 2)])
def test_phrase_device_search_equals_phrase_host_search_fp32(k, ngram):
    """C1-sized fp32 batch: the two searches pick the same hypotheses in the same order, their states agree with each other and with
    the strings replayed, and every finished hypothesis holds every phrase."""
    from gtos_amd.search import phrase_state
    from test_diverse_beam import synth_c1, _close
    model, batch = synth_c1()
    max_t, min_t = 12, 1
    phrases, best = plain_and_phrases(k, max_t, min_t)
    assert all([len(p) for p in ps] == [2, 3, 1] for ps in phrases)
    kw = dict(phrases=phrases, no_repeat_ngram=ngram)
    host = model.work(batch, k, max_t, min_t, **kw)
    dev = model.work(batch, k, max_t, min_t, search="device", **kw)
    n_full, gaps = 0, []
    for b, (h, d) in enumerate(zip(host, dev)):
        assert h.steps == d.steps, b
        for hl, dl in ((h.hypotheses, d.hypotheses), (h.completed_hypotheses, d.completed_hypotheses)):
            assert [x.seq for x in hl] == [x.seq for x in dl], b
            assert all(_close(x.score, y.score) for x, y in zip(hl, dl)), b
        replay = [phrase_state(x.seq, phrases[b]) for x in d.hypotheses]
        assert list(h.met) == list(d.met) == [r[0] for r in replay], b
        assert [tuple(p) for p in h.progress] == [tuple(p) for p in d.progress] == [r[1:] for r in replay], b
        for x in d.completed_hypotheses:
            assert phrase_state(x.seq, phrases[b])[0] == 7, (b, x.seq)
        held = d.hypotheses + d.completed_hypotheses
        if not ngram:
            assert any(phrase_state(x.seq, phrases[b])[0] == 7 for x in held), b                  # min_t = 1 <= T = 6 <= max_t, finite lls
            if k == 1:
                assert phrase_state(held[0].seq[1:7], phrases[b])[0] == 7, (b, held[0].seq)
        else:
            for x in held:
                y = [w for w in x.seq[1:] if w != END]
                grams = [tuple(y[i:i + ngram]) for i in range(len(y) - ngram + 1)]
                assert len(grams) == len(set(grams)), x.seq
        n_full += any(phrase_state(x.seq, phrases[b])[0] == 7 for x in d.completed_hypotheses)
        gaps.append(best[b].score - d.get_k_best(1, 0.6)[0].score)
    print("MEASURED k=%d ngram=%d: %d of %d graphs hold a completed hypothesis with all phrases" % (k, ngram, n_full, len(dev)))
    print("MEASURED k=%d ngram=%d: mean score gap to the plain search's best %.4f" % (k, ngram, sum(gaps) / len(gaps)))


@pytest.mark.gpu
@pytest.mark.parametrize("k,ngram", [(1, 0), (6, 2), (8, 0)])
def test_single_token_phrases_equal_the_constrained_device_search(k, ngram):
    """phrases=[[w], ...] gives the beams of constraints=[w, ...]: sequences, scores and masks, exactly"""
    from test_diverse_beam import synth_c1
    model, batch = synth_c1()
    max_t, min_t = 12, 1
    phrases, _ = plain_and_phrases(k, max_t, min_t)
    cons = [ps[0] + ps[2] for ps in phrases]                     # three distinct single tokens
    assert all(len(set(c)) == 3 for c in cons)
    a = model.work(batch, k, max_t, min_t, search="device", no_repeat_ngram=ngram, constraints=cons)
    p = model.work(batch, k, max_t, min_t, search="device", no_repeat_ngram=ngram, phrases=[[[w] for w in c] for c in cons])
    for b, (x, y) in enumerate(zip(a, p)):
        assert x.steps == y.steps and pairs(x.hypotheses) == pairs(y.hypotheses), b
        assert pairs(x.completed_hypotheses) == pairs(y.completed_hypotheses), b
        assert list(x.met) == list(y.met) and all(tuple(q) == (-1, 0) for q in y.progress), b


@pytest.mark.gpu
def test_without_phrases_the_new_route_is_the_plain_device_search(monkeypatch):
    from gtos_amd import search
    from test_diverse_beam import synth_c1, _capture_memory
    model, batch = synth_c1()
    memory = _capture_memory(model, batch, monkeypatch)
    n = len(memory['local_idx2token'])
    for k, max_t, min_t, ngram in ((4, 12, 1, 0), (6, 9, 3, 0), (8, 10, 1, 3)):
        out = []
        for kw in (dict(), dict(phrased=True), dict(phrases=[[] for _ in range(n)])):
            beams = [search.Beam(k, min_t, max_t) for _ in range(n)]
            stats = {}
            with torch.no_grad():
                search.beam_search_device(model, memory, beams, stats=stats, no_repeat_ngram=ngram, **kw)
            out.append([(b.steps, pairs(b.hypotheses), pairs(b.completed_hypotheses)) for b in beams] + [stats])
            if kw:
                assert all(not any(b.met) and all(tuple(q) == (-1, 0) for q in b.progress) for b in beams)
        assert out[0] == out[1] == out[2], (k, max_t, min_t)
