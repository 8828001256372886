"""Stochastic beam search (Generator.work(..., search="stochastic"), gtos_amd.search.stochastic_beam_search_device, csrc/sbs.hip,
csrc/sbs_kernels.h): k distinct sequences per graph, drawn without replacement.

CPU: the rule header compiled with g++ against a numpy statement of rules 1-7 on random tables; the law of the draw on a toy tree
(ordered first / second pair against Plackett-Luce, first alone against one sample's law); the importance weights; work's argument
checks; the entry points' refusals.  GPU: the two kernels against the same numpy statement, the law through the real kernels, and end
to end on C1 (fp32) and C2 (bf16) models against a host loop that applies the numpy rule."""
import ctypes
import math
import types

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver
from test_sample_decode import END_, NEAR, _p, allowed_mask, f32, random_row, random_tables, uniforms


DRIVER = r"""
#include "sbs_kernels.h"
using namespace gtos_sbs;
extern "C" int max_k() { return MAX_K; }
extern "C" void roots(uint64_t seed, int B, double* out) {
    for (int b = 0; b < B; ++b) out[b] = root_gumbel(seed, b);
}
extern "C" void sbs_step(int N, int k, int t, int V, int tot, int min_t, double T, uint64_t seed, const float* ll, int64_t ld,
                         const uint8_t* fs, const uint8_t* fl, const uint8_t* owned, const double* slot_logq, const double* slot_gumbel,
                         const int* state, const int* active, int* cand_tok, float* cand_ll, double* cand_logq, double* cand_gumbel) {
    if (!active[active_read(t)]) return;
    double kk[MAX_K];
    for (int s = 0; s < N; ++s) {
        const int b = s / k, j = s % k;
        if (!slot_is_live(state + (int64_t)b * BS_WORDS, j)) continue;
        const int64_t at = (int64_t)s * k;
        row_serial(ll + s * ld, tot, V, b, j, t, min_t, fs, fl, owned, T, seed, k, slot_logq[s], slot_gumbel[s], cand_tok + at,
                   cand_ll + at, cand_logq + at, cand_gumbel + at, kk);
    }
}
extern "C" void sbs_advance(int B, int k, int t, int V, int tot, int min_t, int max_t, const int* cand_tok, const float* cand_ll,
                            const double* cand_logq, const double* cand_gumbel, const uint8_t* fs, const uint8_t* fl,
                            double* slot_score, double* slot_logq, double* slot_gumbel, int* state, int* bp_parent, int* bp_token,
                            int* comp_step, int* comp_parent, double* comp_score, double* comp_logq, double* comp_gumbel, int* active) {
    const Tables a{B, k, t, V, tot, min_t, max_t, cand_tok, cand_ll, cand_logq, cand_gumbel, fs, fl, slot_score, slot_logq, slot_gumbel,
                   state, bp_parent, bp_token, comp_step, comp_parent, comp_score, comp_logq, comp_gumbel, active};
    static double G[MAX_POOL];
    static uint8_t present[MAX_POOL];
    int order[MAX_K], c_step[MAX_K], c_parent[MAX_K];
    double c_score[MAX_K], c_logq[MAX_K], s_score[MAX_K];
    active[active_clear(t)] = 0;
    if (!active[active_read(t)]) return;
    for (int b = 0; b < B; ++b)
        if (advance_serial(a, b, G, present, order, Stage{c_step, c_parent, c_score, c_logq, s_score})) active[active_set(t)] |= 1;
}
"""

# logq and G: |got - want| <= TOL * max(1, |want|).  The largest such gap between the g++ build of the header and the numpy statement
# over the cases of test_rule_header_matches_numpy is 3.1e-14: numpy sums a row's weights pairwise, the header serially, and the two
# libms differ in the last place, which leaves the keys an ulp or two apart (values up to ~100); rule 5 then takes log(1 - exp(key - Z)),
# which magnifies that by 1 / (Z - key) for a candidate close under its row's best.  The bar carries a factor 8 on top because the
# device's log / exp are accurate to an ulp or two rather than correctly rounded.  The GPU tests use the same bar.
TOL = 8 * 3.1e-14
CHI2_239 = 312.3          # 0.999 quantile of chi-square with 239 degrees of freedom (240 ordered pairs of 16 leaves)
CHI2_15 = 37.70           # the same for 15 (the 16 leaves)
UNK_STRING = "<UNK>"
INT_TABLES = ("state", "bp_parent", "bp_token", "comp_step", "comp_parent", "active")
DBL_TABLES = ("slot_score", "slot_logq", "slot_gumbel", "comp_score", "comp_logq", "comp_gumbel")


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = compile_host_driver(tmp_path_factory, "sbs_host", DRIVER)
    c_i, c_p = ctypes.c_int, ctypes.c_void_p
    so.sbs_step.argtypes = [c_i] * 6 + [ctypes.c_double, ctypes.c_uint64, c_p, ctypes.c_int64] + [c_p] * 11
    so.sbs_step.restype = None
    so.sbs_advance.argtypes = [c_i] * 7 + [c_p] * 18
    so.sbs_advance.restype = None
    so.max_k.restype = c_i
    so.roots.argtypes = [ctypes.c_uint64, c_i, c_p]
    so.roots.restype = None
    return so


# ------------------------------------------------------------------------------------------------ the rule, stated in numpy
def fresh_tables(B, k, max_t, roots=0.0):
    """The tables of a search before its first step: slot 0 of every graph live with score = logq = 0 and G = its root value"""
    N = B * k
    S = dict(state=np.tile(np.array([0, 0, 1, 0], np.int32), (B, 1)), bp_parent=np.full((max_t, N), -1, np.int32),
             bp_token=np.full((max_t, N), -1, np.int32), comp_step=np.zeros((B, k), np.int32), comp_parent=np.zeros((B, k), np.int32),
             active=np.array([1, 0, 0], np.int32))
    S.update({name: np.zeros((B, k) if name.startswith("comp") else N) for name in DBL_TABLES})
    S["slot_gumbel"][::k] = roots
    return S


def close_pair(a, b):
    return abs(a - b) <= NEAR * max(abs(a), abs(b))


def np_row(row, allow, T, seed, b, j, t, k, logq_s, G_s):
    """Rules 2-5 for one live row -> ([(column, ll, logq, G'), ...] in key order, some decision of the cut was a near tie)."""
    cols = np.nonzero(allow)[0]
    if not cols.size:
        return [], False
    v = row[cols].astype(np.float64)
    x = (v - v.max()) / T
    logq = logq_s + x - np.log(np.exp(x).sum())
    key = logq - np.log(-np.log(uniforms(seed, b, j, t, cols)))
    order = np.lexsort((cols, -key))
    near = any(close_pair(key[order[i]], key[order[i + 1]]) for i in range(min(k, cols.size - 1)))
    order = order[:k]
    Z = key[order[0]]
    out = []
    for i in order:
        if key[i] == Z:
            G = G_s
        else:
            u = G_s - key[i] + np.log1p(-np.exp(key[i] - Z))
            G = G_s - max(0.0, u) - np.log1p(np.exp(-abs(u)))
        out.append((int(cols[i]), row[cols[i]], float(logq[i]), float(G)))
    return out, near


def np_rule(S, t, k, V, tot, min_t, max_t, T, seed, ll, fs, fl, owned):
    """Rules 1-7: one step and advance of every graph on a copy of the tables S -> (tables, per graph: a decision was a near tie)."""
    S = {name: x.copy() for name, x in S.items()}
    B = S["state"].shape[0]
    near = np.zeros(B, bool)
    S["active"][(t + 2) % 3] = 0
    if not S["active"][t % 3]:
        return S, near
    for b in range(B):
        steps, ncomp, nlive, done = S["state"][b]
        if done:
            continue
        pool = [("comp", i, float(S["comp_gumbel"][b, i])) for i in range(ncomp)]
        for j in range(nlive):
            s = b * k + j
            allow = allowed_mask(ll[s], V, fs, fl[b], owned[b], t, min_t)
            cands, amb = np_row(ll[s], allow, T, seed, b, j, t, k, float(S["slot_logq"][s]), float(S["slot_gumbel"][s]))
            near[b] |= amb
            pool += [("cand", (s, c), c[3]) for c in cands]
        pool.sort(key=lambda e: -e[2])                                  # stable: ties keep pool order
        near[b] |= any(close_pair(pool[i][2], pool[i + 1][2]) for i in range(min(k, len(pool) - 1)))
        old = {name: S[name][b].copy() for name in ("comp_step", "comp_parent", "comp_score", "comp_logq", "comp_gumbel")}
        old_score = S["slot_score"][b * k:b * k + k].copy()
        S["bp_parent"][t, b * k:b * k + k] = -1
        S["bp_token"][t, b * k:b * k + k] = -1
        ncomp = nlive = 0
        for kind, what, G in pool[:k]:
            if kind == "comp":
                row = [old[name][what] for name in ("comp_step", "comp_parent", "comp_score", "comp_logq")]
            else:
                s, (c, llc, logq, _) = what
                score = old_score[s - b * k] + np.float64(llc)
                if (fs[c] if c < V else fl[b, c - V]) == END_:
                    row = [t, s, score, logq]
                else:
                    at = b * k + nlive
                    S["bp_parent"][t, at], S["bp_token"][t, at] = s, c
                    S["slot_score"][at], S["slot_logq"][at], S["slot_gumbel"][at] = score, logq, G
                    nlive += 1
                    continue
            for name, x in zip(("comp_step", "comp_parent", "comp_score", "comp_logq", "comp_gumbel"), row + [G]):
                S[name][b, ncomp] = x
            ncomp += 1
        S["state"][b] = [steps + 1, ncomp, nlive, int(nlive == 0 or steps + 1 >= max_t)]
        if not S["state"][b, 3]:
            S["active"][(t + 1) % 3] = 1
    return S, near


def gap(got, want):
    """max |got - want| / max(1, |want|) over two arrays"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(1.0, np.abs(want)))) if got.size else 0.0


def compare_tables(got, want, before, near, t, k, tag):
    """The tables after a step against the numpy statement's, graph by graph; a graph with a near tie is only counted.  Tokens, parents,
    table order and scores equal, logq and G within TOL.  -> (graphs compared, the largest logq / G gap seen)."""
    B = want["state"].shape[0]
    checked, worst = 0, 0.0
    for b in range(B):
        if near[b]:
            continue
        checked += 1
        sl = slice(b * k, b * k + k)
        assert got["state"][b].tolist() == want["state"][b].tolist(), (tag, b)
        _, ncomp, nlive, _ = want["state"][b]
        if before["state"][b, 3] or not before["active"][t % 3]:        # a done graph, or a step that does not run: nothing changes
            for name in ("bp_parent", "bp_token"):
                assert np.array_equal(got[name][t, sl], before[name][t, sl]), (tag, b, name)
            for name in ("slot_score", "slot_logq", "slot_gumbel"):
                assert np.array_equal(got[name][sl], before[name][sl]), (tag, b, name)
            for name in ("comp_step", "comp_parent", "comp_score", "comp_logq", "comp_gumbel"):
                assert np.array_equal(got[name][b], before[name][b]), (tag, b, name)
            continue
        for name in ("bp_parent", "bp_token"):
            assert got[name][t, sl].tolist() == want[name][t, sl].tolist(), (tag, b, name)
        assert np.array_equal(got["slot_score"][sl][:nlive], want["slot_score"][sl][:nlive]), (tag, b)
        for name in ("comp_step", "comp_parent", "comp_score"):
            assert np.array_equal(got[name][b, :ncomp], want[name][b, :ncomp]), (tag, b, name)
        for g, w in ((got[name][sl][:nlive], want[name][sl][:nlive]) for name in ("slot_logq", "slot_gumbel")):
            worst = max(worst, gap(g, w))
        for g, w in ((got[name][b, :ncomp], want[name][b, :ncomp]) for name in ("comp_logq", "comp_gumbel")):
            worst = max(worst, gap(g, w))
        assert worst <= TOL, (tag, b, worst)
    others = [r for r in range(want["bp_parent"].shape[0]) if r != t]
    for name in ("bp_parent", "bp_token"):
        assert np.array_equal(got[name][others], before[name][others]), (tag, name)
    if not near.any():
        assert got["active"].tolist() == want["active"].tolist(), tag
    assert got["active"][(t + 2) % 3] == 0 and got["active"][t % 3] == before["active"][t % 3], tag
    return checked, worst


def random_case(rng, B, k, tot, T, max_t=9):
    """Random tables in front of step t with every hazard of the rule: dead slots, done graphs, rows with fewer than k (or no) allowed
    columns, <END> on both sides of min_time_step, completions above and below the live slots' values, and (graph 0, when asked by the
    caller through ``all_done``) a graph whose first k will all be completions."""
    N = B * k
    V = tot - max(1, tot // 8) if tot > 8 else int(rng.randint(1, tot + 1))
    fs, fl, owned = random_tables(rng, B, V, tot, p_end=float(rng.choice([0.04, 0.3])))
    t, min_t = int(rng.randint(max_t)), int(rng.randint(max_t))
    ll = np.stack([random_row(rng, tot) for _ in range(N)])
    S = fresh_tables(B, k, max_t)
    S["active"][:] = 0
    S["active"][[t % 3, (t + 2) % 3]] = 1
    S["bp_parent"][:] = rng.randint(-1, N, size=(max_t, N))
    S["bp_token"][:] = rng.randint(-1, tot, size=(max_t, N))
    S["bp_parent"][t], S["bp_token"][t] = -1, -1
    for b in range(B):
        nlive = int(rng.randint(0, k + 1))
        ncomp = int(rng.randint(0, k - nlive + 1))
        S["state"][b] = [t, ncomp, nlive, int(nlive == 0 or rng.rand() < 0.1)]
        S["comp_gumbel"][b, :ncomp] = np.sort(-rng.rand(ncomp) * rng.choice([3.0, 12.0]))[::-1]
        S["comp_step"][b, :ncomp] = rng.randint(0, t + 1, ncomp)
        S["comp_parent"][b, :ncomp] = rng.randint(b * k, b * k + k, ncomp)
    S["comp_score"][:], S["comp_logq"][:] = -rng.rand(B, k) * 30, -rng.rand(B, k) * 30
    S["slot_score"][:], S["slot_logq"][:], S["slot_gumbel"][:] = -rng.rand(N) * 30, -rng.rand(N) * 30, -rng.rand(N) * 4
    for s in rng.choice(N, size=max(1, N // 4), replace=False):        # rows with few allowed columns, and one with none
        keep = rng.choice(tot, size=min(tot, int(rng.randint(1, 4))), replace=False)
        row = np.full(tot, -np.inf, np.float32)
        row[keep] = ll[s, keep]
        ll[s] = row
    ll[int(rng.randint(N))] = -np.inf
    return dict(V=V, fs=fs, fl=fl, owned=owned, t=t, min_t=min_t, max_t=max_t, ll=ll, S=S, T=f32(T),
                seed=int(rng.randint(0, 2 ** 62)) * 4 + 1)


def all_completions_case(rng, case, k):
    """Graph 0 of ``case`` rewritten so that its first k are all completions: k - 1 of them retained above its one live slot's value,
    and that slot's row all but certain to draw <END> first, whose value is then the slot's own."""
    S, V, t = case["S"], case["V"], case["t"]
    case["min_t"] = 0
    case["fs"][2 % V] = END_
    S["state"][0] = [t, k - 1, 1, 0]
    S["comp_gumbel"][0, :k - 1] = np.sort(-rng.rand(k - 1))[::-1]
    S["slot_gumbel"][0] = -2.0
    case["ll"][0] = -60.0
    case["ll"][0, 2 % V] = -0.01
    return case


def host_step(lib, case, k):
    """One step + advance of the g++ build of the header on a copy of the case's tables"""
    S = {name: x.copy() for name, x in case["S"].items()}
    B = S["state"].shape[0]
    N, tot = case["ll"].shape
    cand = [np.full((N, k), -7, np.int32), np.zeros((N, k), np.float32), np.zeros((N, k)), np.zeros((N, k))]
    V, t, min_t, max_t = case["V"], case["t"], case["min_t"], case["max_t"]
    lib.sbs_step(N, k, t, V, tot, min_t, case["T"], case["seed"], _p(case["ll"]), tot, _p(case["fs"]), _p(case["fl"]), _p(case["owned"]),
                 _p(S["slot_logq"]), _p(S["slot_gumbel"]), _p(S["state"]), _p(S["active"]), *[_p(x) for x in cand])
    lib.sbs_advance(B, k, t, V, tot, min_t, max_t, *[_p(x) for x in cand], _p(case["fs"]), _p(case["fl"]), _p(S["slot_score"]),
                    _p(S["slot_logq"]), _p(S["slot_gumbel"]), _p(S["state"]), _p(S["bp_parent"]), _p(S["bp_token"]), _p(S["comp_step"]),
                    _p(S["comp_parent"]), _p(S["comp_score"]), _p(S["comp_logq"]), _p(S["comp_gumbel"]), _p(S["active"]))
    return S


def want_of(case, k):
    return np_rule(case["S"], case["t"], k, case["V"], case["ll"].shape[1], case["min_t"], case["max_t"], case["T"], case["seed"],
                   case["ll"], case["fs"], case["fl"], case["owned"])


def census(case, want, k, seen):
    """Which of the hazards the issue lists this case exercised"""
    S, t = case["S"], case["t"]
    for b in range(S["state"].shape[0]):
        _, ncomp, nlive, done = S["state"][b]
        if done:
            seen["done graph"] += 1
            continue
        seen["dead slots"] += nlive < k
        n_allowed = [int(allowed_mask(case["ll"][b * k + j], case["V"], case["fs"], case["fl"][b], case["owned"][b], t, case["min_t"]).sum())
                     for j in range(nlive)]
        seen["fewer than k allowed"] += any(0 < n < k for n in n_allowed)
        seen["none allowed"] += any(n == 0 for n in n_allowed)
        seen["<END> before min_time_step"] += t < case["min_t"]
        seen["<END> allowed"] += t >= case["min_t"]
        kept = set(want["comp_gumbel"][b, :want["state"][b, 1]].tolist()) & set(S["comp_gumbel"][b, :ncomp].tolist())
        seen["completions that stay"] += len(kept) > 0
        seen["completions evicted"] += len(kept) < ncomp
        seen["new completion"] += bool((want["comp_step"][b, :want["state"][b, 1]] == t).any())
        seen["first k all completions"] += want["state"][b, 1] == k


# ------------------------------------------------------------------------------------------------ CPU
def test_rule_header_matches_numpy(host_lib):
    from gtos_amd import ops
    assert host_lib.max_k() == ops.SBS_MAX_K == 32
    rng = np.random.RandomState(20261020)
    checked = near = 0
    worst = 0.0
    seen = {name: 0 for name in ("done graph", "dead slots", "fewer than k allowed", "none allowed", "<END> before min_time_step",
                                 "<END> allowed", "completions that stay", "completions evicted", "new completion",
                                 "first k all completions")}
    for tot in (5, 32, 997):
        for k in (1, 3, 6, 32):
            for T in (0.5, 1.0, 2.5):
                for rep in range(6 if tot < 997 else 3):
                    case = random_case(rng, 3, k, tot, T)
                    if rep == 0:
                        all_completions_case(rng, case, k)
                    want, amb = want_of(case, k)
                    got = host_step(host_lib, case, k)
                    n, w = compare_tables(got, want, case["S"], amb, case["t"], k, (tot, k, T, rep))
                    checked, near, worst = checked + n, near + int(amb.sum()), max(worst, w)
                    census(case, want, k, seen)
    print("graphs compared %d, near ties %d, largest logq / G gap %.3g (bar %.3g)" % (checked, near, worst, TOL))
    assert checked >= 400 and near <= checked // 50, (checked, near)
    assert near == 0, near                                              # continuous fp64 keys: the numpy statement leaves none out
    assert all(seen.values()), seen
    # a step whose active word is clear changes nothing
    case = random_case(rng, 3, 6, 32, 1.0)
    case["S"]["active"][:] = 0
    got = host_step(host_lib, case, 6)
    for name in INT_TABLES + DBL_TABLES:
        assert np.array_equal(got[name], case["S"][name]), name


# the toy tree of the law tests: 4 plain tokens, two steps, T = 1.3; the rows carry masked mass (they do not sum to 1)
TOY_T, TOY_K = f32(1.3), 3
TOY_ROOT = np.log(0.7 * np.array([.4, .3, .2, .1]))
TOY_SECOND = np.log(np.array([[.25, .25, .25, .25], [.5, .2, .2, .1], [.1, .2, .3, .4], [.4, .4, .1, .1]]) * np.array([[.9], [.5], [.8], [.6]]))


def toy_leaf_law():
    """p[4 * first + second] under the distribution drawn from: every row tempered and normalised on its own"""
    norm = lambda row: np.exp(row / TOY_T) / np.exp(row / TOY_T).sum()
    return (norm(TOY_ROOT)[:, None] * np.stack([norm(r) for r in TOY_SECOND])).ravel()


def law_statistics(leaves):
    """leaves int [trials, 3] in rank order -> (chi-square of the ordered (first, second) pair against p_i p_j / (1 - p_i) over the
    240 cells, chi-square of the first alone over its 16 cells, the smallest expectation of a pair cell)"""
    p = toy_leaf_law()
    n = leaves.shape[0]
    pair = np.zeros((16, 16))
    np.add.at(pair, (leaves[:, 0], leaves[:, 1]), 1)
    expect = n * p[:, None] * p[None, :] / (1 - p[:, None])
    off = ~np.eye(16, dtype=bool)
    assert pair[~off].sum() == 0
    first = np.bincount(leaves[:, 0], minlength=16)
    return (float(((pair - expect) ** 2 / expect)[off].sum()), float(((first - n * p) ** 2 / (n * p)).sum()), float(expect[off].min()))


def check_trials(leaves, G, parent_G, roots):
    """Every trial: k distinct leaves, in descending G, every child's G <= its parent's, the first's the root's own"""
    assert (parent_G <= roots[:, None]).all() and (G[:, 0] == roots).all()
    assert leaves.shape[1] == TOY_K and (leaves >= 0).all() and (leaves < 16).all()
    srt = np.sort(leaves, axis=1)
    assert (srt[:, 1:] != srt[:, :-1]).all()
    assert (G[:, 1:] <= G[:, :-1]).all()
    assert (G <= parent_G).all()


@pytest.fixture(scope="module")
def toy_trials(host_lib):
    """40,000 trials (one graph each) of the toy tree through the g++ build of the header, for each of seeds 1, 2, 3 ->
    {seed: (leaves [n,3], logq [n,3], G [n,3], parent G [n,3], root G [n])}.  The roots are the header's root_gumbel, which
    gtos_amd.search.stochastic_roots restates."""
    from gtos_amd.search import stochastic_roots
    B, k, tot = 40000, TOY_K, 4
    N = B * k
    fs, none = np.zeros(4, np.uint8), np.zeros((B, 0), np.uint8)
    out = {}
    for seed in (1, 2, 3):
        roots = np.zeros(B)
        host_lib.roots(seed, B, _p(roots))
        assert np.allclose(roots[:300], stochastic_roots(seed, 300), rtol=1e-15, atol=0) and abs(roots.mean() - 0.5772) < 0.03
        S = fresh_tables(B, k, 2, roots)
        case = dict(V=4, fs=fs, fl=none, owned=none, t=0, min_t=0, max_t=2, T=TOY_T, seed=seed, S=S,
                    ll=np.tile(TOY_ROOT.astype(np.float32), (N, 1)))
        S = host_step(host_lib, case, k)
        parent_G = S["slot_gumbel"].copy()
        case.update(t=1, S=S, ll=np.ascontiguousarray(TOY_SECOND.astype(np.float32)[np.maximum(S["bp_token"][0], 0)]))
        S = host_step(host_lib, case, k)
        assert (S["state"] == [2, 0, k, 1]).all()
        leaves = 4 * S["bp_token"][0][S["bp_parent"][1]] + S["bp_token"][1]
        out[seed] = (leaves.reshape(B, k), S["slot_logq"].reshape(B, k), S["slot_gumbel"].reshape(B, k),
                     parent_G[S["bp_parent"][1]].reshape(B, k), roots)
    return out


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_law_of_the_draw(toy_trials, seed):
    """The ordered (first, second) pair follows the without-replacement law of the leaf distribution, the first alone that
    distribution.  The numpy simulation of the rule gave 200-239 for the pair statistic; without the local normalisation of rule 2, 505."""
    leaves, logq, G, parent_G, roots = toy_trials[seed]
    check_trials(leaves, G, parent_G, roots)
    assert gap(logq, np.log(toy_leaf_law())[leaves]) <= 1e-6           # the header saw the fp32 rows
    pair, first, smallest = law_statistics(leaves)
    print("seed %d: chi-square of the pair %.1f (bound %.1f), of the first %.1f (bound %.2f)" % (seed, pair, CHI2_239, first, CHI2_15))
    assert 10.0 < smallest < 11.0, smallest
    assert pair <= CHI2_239 and first <= CHI2_15, (pair, first)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_stochastic_weights_estimate_the_leaf_probabilities(toy_trials, seed):
    """mean over the trials of sum_i w_i [leaf_i == l] is p_l within 4 standard errors (taken from the trials), for every leaf"""
    from gtos_amd.search import StochasticHypothesis, stochastic_weights
    leaves, logq, G, _, _ = toy_trials[seed]
    n = leaves.shape[0]
    est = np.zeros((n, 16))
    for i, (lv, lq, g) in enumerate(zip(leaves.tolist(), logq.tolist(), G.tolist())):
        beam = types.SimpleNamespace(completed_hypotheses=[StochasticHypothesis([lv[0]], 0.0, lq[0], g[0])],
                                     hypotheses=[StochasticHypothesis([lv[r]], 0.0, lq[r], g[r]) for r in (1, 2)])
        weights, kappa = stochastic_weights(beam)
        assert kappa == g[2] and [h.seq[0] for h, _ in weights] == lv[:2]
        for h, w in weights:
            assert w >= math.exp(h.logq)
            est[i, h.seq[0]] += w
    p = toy_leaf_law()
    mean, se = est.mean(0), est.std(0, ddof=1) / math.sqrt(n)
    assert (se > 0).all() and (np.abs(mean - p) <= 4 * se).all(), ((mean - p) / se).tolist()
    # the helper's edges: one hypothesis has nothing below it; an empty beam
    one = types.SimpleNamespace(completed_hypotheses=[], hypotheses=[StochasticHypothesis(["a"], -1.0, -1.0, -0.5)])
    assert stochastic_weights(one) == ([], -0.5)
    assert stochastic_weights(types.SimpleNamespace(completed_hypotheses=[], hypotheses=[]))[0] == []


def test_work_checks_the_stochastic_arguments():
    """No model needed: the checks run before anything is touched."""
    from gtos_amd import synth
    from gtos_amd.generator import Generator
    pv = synth.synth_vocabs()['predictable_token']
    word = next(pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i)[0] != "<")
    me = types.SimpleNamespace(vocabs={'predictable_token': pv})
    data = {'local_idx2token': [{pv.size: "copy0"}, {}]}
    refused = [dict(top_k=5), dict(top_p=0.9), dict(top_k=1, top_p=0.5), dict(groups=2), dict(groups=2, diversity=0.5),
               dict(constraints=[["copy0"], []]), dict(phrases=[[["copy0", word]], []]), dict(coverage_penalty=0.2),
               dict(coverage_penalty=0.0)]
    for kw in refused:
        with pytest.raises(ValueError):
            Generator.work(me, data, 4, 10, search="stochastic", seed=1, **kw)
    bad = [dict(temperature=0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
           dict(temperature=1e300), dict(temperature=True), dict(seed=1.5), dict(seed="7"), dict(top_k=-1), dict(top_p=0.0)]
    for kw in bad:
        with pytest.raises(ValueError):
            Generator.work(me, data, 4, 10, search="stochastic", **kw)
    for beam_size in (0, 33, 2.0):
        with pytest.raises(ValueError):
            Generator.work(me, data, beam_size, 10, search="stochastic")
    for kw in (dict(no_repeat_ngram=-1), dict(avoid=[["copy0"]]), dict(avoid=[[UNK_STRING], []])):
        with pytest.raises(ValueError):
            Generator.work(me, data, 4, 10, search="stochastic", **kw)
    for kw in (dict(temperature=0.7), dict(seed=3)):                    # the beam searches still refuse the sampling keywords
        for search in ("host", "device"):
            with pytest.raises(ValueError):
                Generator.work(me, data, 4, 10, search=search, **kw)
    with pytest.raises(ValueError, match="stochastic"):
        Generator.work(me, data, 4, 10, search="stochastic-beam")



def test_sbs_entry_points_refuse_bad_arguments():
    """-10 for settings outside the rule, -23 for null pointers; nothing launched, no device needed."""
    from gtos_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def step(N=8, k=4, t=0, V=10, tot=12, max_t=5, T=1.0, ld=12, ptrs=None):
        ptrs = ptrs or [p] * 12
        return lib.gtos_sbs_step(N, k, t, V, tot, 0, max_t, T, 7, ptrs[0], ld, *ptrs[1:], None)

    def advance(B=2, k=4, t=0, V=10, tot=12, max_t=5, ptrs=None):
        return lib.gtos_sbs_advance(B, k, t, V, tot, 0, max_t, *(ptrs or [p] * 18), None)
    for kw in (dict(k=0), dict(k=33, N=66), dict(N=9), dict(t=-1), dict(t=5), dict(V=0), dict(tot=9), dict(ld=11), dict(T=0.0),
               dict(T=-1.0), dict(T=float("inf")), dict(T=float("nan"))):
        assert step(**kw) == -10, kw
    for kw in (dict(k=0), dict(k=33), dict(t=-1), dict(t=5), dict(V=0), dict(tot=9)):
        assert advance(**kw) == -10, kw
    for i in range(12):                                                 # ll, the two flag tables, owned_local, ... in the entry point's order
        ptrs = [None if q == i else p for q in range(12)]
        assert step(ptrs=ptrs) == -23, i
        if i not in (2, 3):                                             # flag_local and owned_local may be null when tot == V
            assert step(tot=10, ld=10, ptrs=ptrs) == -23, i
    for i in range(18):
        ptrs = [None if q == i else p for q in range(18)]
        assert advance(ptrs=ptrs) == -23, i
        if i != 5:                                                      # flag_local
            assert advance(tot=10, ptrs=ptrs) == -23, i
    assert step(N=0) == 0 and advance(B=0) == 0


# ------------------------------------------------------------------------------------------------ GPU: the kernels
def device_step(case, k, inputs=None):
    """One ops.sbs_step + ops.sbs_advance (+ ops.beam_reorder without caches, for the next inputs) on a copy of the case's tables"""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    N, tot = case["ll"].shape
    V, t, min_t, max_t = case["V"], case["t"], case["min_t"], case["max_t"]
    S = {name: D(x) for name, x in case["S"].items()}
    fs, fl, owned = D(case["fs"]), D(case["fl"]) if tot > V else None, D(case["owned"]) if tot > V else None
    cand = [torch.full((N, k), -7, dtype=torch.int32, device=dev), torch.zeros((N, k), dtype=torch.float32, device=dev),
            torch.zeros((N, k), dtype=torch.float64, device=dev), torch.zeros((N, k), dtype=torch.float64, device=dev)]
    ops.sbs_step(t, k, V, tot, min_t, max_t, case["T"], case["seed"], D(case["ll"]), fs, fl, owned, S["slot_logq"], S["slot_gumbel"],
                 S["state"], S["active"], *cand)
    ops.sbs_advance(t, k, V, tot, min_t, max_t, *cand, fs, fl, S["slot_score"], S["slot_logq"], S["slot_gumbel"], S["state"],
                    S["bp_parent"], S["bp_token"], S["comp_step"], S["comp_parent"], S["comp_score"], S["comp_logq"], S["comp_gumbel"],
                    S["active"])
    out = {name: x.cpu().numpy() for name, x in S.items()}
    if inputs is not None:
        tok_shared, tok_local, char_shared, char_local, dead_tok, dead_char = inputs
        C = dead_char.shape[0]
        tok_out = torch.full((N,), -5, dtype=torch.int64, device=dev)
        char_out = torch.full((N, C), -5, dtype=torch.int64, device=dev)
        ops.beam_reorder([], [], t, k, S["bp_parent"], S["bp_token"], S["state"], S["active"], V, tot, D(tok_shared),
                         D(tok_local) if tot > V else None, D(char_shared), D(char_local) if tot > V else None, dead_tok, D(dead_char),
                         tok_out, char_out)
        out["tok_out"], out["char_out"] = tok_out.cpu().numpy(), char_out.cpu().numpy()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("tot,k", [(32, 6), (997, 6), (20000, 6), (65536, 6), (997, 32), (32, 1)])
def test_sbs_kernels_match_numpy_rule(tot, k):
    rng = np.random.RandomState(tot * 64 + k)
    B, C = 3, 5
    N = B * k
    checked = near = 0
    worst = 0.0
    for T in (0.5, 1.0, 2.5):
        for rep in range(4):
            case = random_case(rng, B, k, tot, T)
            if rep == 0:
                all_completions_case(rng, case, k)
            V = case["V"]
            inputs = (rng.randint(0, 1000, V), rng.randint(0, 1000, (B, tot - V)), rng.randint(0, 100, (V, C)),
                      rng.randint(0, 100, (B, tot - V, C)), 77, rng.randint(0, 100, C))
            want, amb = want_of(case, k)
            got = device_step(case, k, inputs)
            n, w = compare_tables(got, want, case["S"], amb, case["t"], k, (tot, k, T, rep))
            checked, near, worst = checked + n, near + int(amb.sum()), max(worst, w)
            tok_shared, tok_local, char_shared, char_local, dead_tok, dead_char = inputs
            for s in range(N):
                b = s // k
                if amb[b]:
                    continue
                w = want["bp_token"][case["t"], s]
                if w >= 0 and not want["state"][b, 3] and not case["S"]["state"][b, 3]:
                    assert got["tok_out"][s] == (tok_shared[w] if w < V else tok_local[b, w - V]), (tot, k, T, rep, s)
                    assert (got["char_out"][s] == (char_shared[w] if w < V else char_local[b, w - V])).all(), (tot, k, T, rep, s)
                else:
                    assert got["tok_out"][s] == dead_tok and (got["char_out"][s] == dead_char).all(), (tot, k, T, rep, s)
    print("graphs compared %d, near ties %d, largest logq / G gap %.3g (bar %.3g)" % (checked, near, worst, TOL))
    assert checked >= 30 and near <= checked // 50, (checked, near)
    # a step whose active word is clear changes no table and hands every slot the padding input
    case["S"]["active"][:] = 0
    got = device_step(case, k, inputs)
    for name in INT_TABLES + DBL_TABLES:
        assert np.array_equal(got[name], case["S"][name]), name
    assert (got["tok_out"] == inputs[4]).all() and (got["char_out"] == inputs[5]).all()


@pytest.mark.gpu
def test_law_of_the_draw_on_the_device():
    """The toy tree through the real kernels: 8,192 graphs per launch x 5 seeds, the second step's rows gathered on the device by
    the first step's bp_token; the statistic and the bound of test_law_of_the_draw over the 40,960 trials together.  The roots are
    left at 0 here: the order of a draw does not depend on the root's value."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    B, k, tot, max_t = 8192, TOY_K, 4, 2
    N = B * k
    fs = torch.zeros(4, dtype=torch.uint8, device=dev)
    root = torch.from_numpy(TOY_ROOT.astype(np.float32)).to(dev).expand(N, tot).contiguous()
    second = torch.from_numpy(TOY_SECOND.astype(np.float32)).to(dev)
    leaves, Gs, parents = [], [], []
    for seed in (1, 2, 3, 4, 5):
        S = {name: torch.from_numpy(x).to(dev) for name, x in fresh_tables(B, k, max_t).items()}
        cand = [torch.full((N, k), -7, dtype=torch.int32, device=dev), torch.zeros((N, k), dtype=torch.float32, device=dev),
                torch.zeros((N, k), dtype=torch.float64, device=dev), torch.zeros((N, k), dtype=torch.float64, device=dev)]
        for t in range(max_t):
            ll = root if t == 0 else second.index_select(0, S["bp_token"][0].clamp(min=0).long()).contiguous()
            if t == 1:
                parent_G = S["slot_gumbel"].clone()
            ops.sbs_step(t, k, tot, tot, 0, max_t, TOY_T, seed, ll, fs, None, None, S["slot_logq"], S["slot_gumbel"], S["state"],
                         S["active"], *cand)
            ops.sbs_advance(t, k, tot, tot, 0, max_t, *cand, fs, None, S["slot_score"], S["slot_logq"], S["slot_gumbel"], S["state"],
                            S["bp_parent"], S["bp_token"], S["comp_step"], S["comp_parent"], S["comp_score"], S["comp_logq"],
                            S["comp_gumbel"], S["active"])
        H = {name: x.cpu().numpy() for name, x in S.items()}
        assert (H["state"] == [2, 0, k, 1]).all()
        leaves.append((4 * H["bp_token"][0][H["bp_parent"][1]] + H["bp_token"][1]).reshape(B, k))
        Gs.append(H["slot_gumbel"].reshape(B, k))
        parents.append(parent_G.cpu().numpy()[H["bp_parent"][1]].reshape(B, k))
    leaves, Gs, parents = np.concatenate(leaves), np.concatenate(Gs), np.concatenate(parents)
    check_trials(leaves, Gs, parents, np.zeros(leaves.shape[0]))
    pair, first, _ = law_statistics(leaves)
    print("chi-square of the pair %.1f (bound %.1f), of the first %.1f (bound %.2f)" % (pair, CHI2_239, first, CHI2_15))
    assert pair <= CHI2_239 and first <= CHI2_15, (pair, first)


# ------------------------------------------------------------------------------------------------ GPU: end to end
def _host_search(model, memory, k, max_t, min_t, T, seed, no_repeat_ngram=0, avoid=None):
    """A host loop over Generator.decode_slots that applies the numpy statement of the rule (np_rule) every step, bans what
    ``no_repeat_ngram`` / ``avoid`` (per graph lists of output-id lists) ban, and reorders the caches with index_select.
    -> (the Beam objects, filled from the numpy tables; graphs in which some decision was a near tie)."""
    from gtos_amd.search import avoided_tokens, banned_tokens, fill_stochastic, slot_memory, stochastic_roots
    from test_sample_decode import _fresh
    B = len(memory['local_idx2token'])
    N = B * k
    dev = memory['probe'].device
    mem = slot_memory(memory, B, k)
    local = memory['local_idx2token']
    pv = model.vocabs['predictable_token']
    V = pv.size
    tot = max(int(memory['tot_ext']), V)
    tab = model.search_tables(local, tot)
    owned = model.sample_tables(local, tot)
    fs = tab['flag_shared'].cpu().numpy()
    fl = tab['flag_local'].cpu().numpy() if tot > V else np.zeros((B, 0), np.uint8)
    ow = owned.cpu().numpy() if tot > V else np.zeros((B, 0), np.uint8)
    caches = [c[0] for c in model.slot_caches(max_t, N, copies=1)]
    tok = torch.full((1, N), tab['dead_tok'], dtype=torch.int64, device=dev)
    chars = tab['dead_char'].expand(1, N, tab['C']).contiguous()
    tok[0, ::k] = tab['start_tok']
    chars[0, ::k] = tab['start_char']
    S = fresh_tables(B, k, max_t, stochastic_roots(seed, B))
    near = np.zeros(B, bool)

    def ids_of(s, t):
        """the output ids slot s holds after step t"""
        ids = []
        while t >= 0:
            ids.append(int(S["bp_token"][t, s]))
            s, t = int(S["bp_parent"][t, s]), t - 1
        return ids[::-1]
    for t in range(max_t):
        if not S["active"][t % 3]:
            break
        ll = model.decode_slots((tok, chars), caches, mem, t).cpu().numpy()
        for b in range(B):
            for j in range(S["state"][b, 2] if not S["state"][b, 3] else 0):
                have = ids_of(b * k + j, t - 1)
                bans = banned_tokens(have, no_repeat_ngram) if no_repeat_ngram else []
                if avoid is not None:
                    bans = bans + avoided_tokens(have, avoid[b])
                ll[b * k + j, bans] = -np.inf
        S, amb = np_rule(S, t, k, V, tot, min_t, max_t, T, seed, ll, fs, fl, ow)
        near |= amb
        parent, token = S["bp_parent"][t], S["bp_token"][t]
        live = (parent >= 0) & ~np.repeat(S["state"][:, 3].astype(bool), k)
        idx = torch.from_numpy(np.where(live, parent, 0).astype(np.int64)).to(dev)
        caches = [c.index_select(1, idx) for c in caches]
        tok = torch.full((1, N), tab['dead_tok'], dtype=torch.int64, device=dev)
        chars = tab['dead_char'].expand(1, N, tab['C']).contiguous()
        for s in np.nonzero(live)[0]:
            b, w = s // k, int(token[s])
            tok[0, s] = tab['tok_shared'][w] if w < V else tab['tok_local'][b, w - V]
            chars[0, s] = tab['char_shared'][w] if w < V else tab['char_local'][b, w - V]
    flat = {name: S[name].ravel().tolist() for name in INT_TABLES[:5] + DBL_TABLES}
    beams = fill_stochastic(_fresh(B, k, max_t, min_t), k, token_string=lambda b, i: local[b][i] if i in local[b] else pv.idx2token(i),
                            **flat)
    return beams, near


def _hyps(beam):
    return list(beam.completed_hypotheses) + list(beam.hypotheses)


def _key(beams):
    return [(b.steps, [(h.seq, h.score, h.logq, h.gumbel) for h in b.completed_hypotheses],
             [(h.seq, h.score, h.logq, h.gumbel) for h in b.hypotheses]) for b in beams]


def _same_as_host(got, want, near):
    """Same sequences in the same order, scores exactly equal, logq and G within the bar; a graph with a near tie is only counted"""
    checked = 0
    for b, (g, w) in enumerate(zip(got, want)):
        if near[b]:
            continue
        checked += 1
        assert g.steps == w.steps, b
        for gl, wl in ((g.completed_hypotheses, w.completed_hypotheses), (g.hypotheses, w.hypotheses)):
            assert [h.seq for h in gl] == [h.seq for h in wl], b
            assert [h.score for h in gl] == [h.score for h in wl], b
            assert gap([h.logq for h in gl], [h.logq for h in wl]) <= TOL and gap([h.gumbel for h in gl], [h.gumbel for h in wl]) <= TOL, b
    assert checked >= 1 and len(got) - checked <= checked // 50, (checked, len(got))


def _check_stochastic(model, memory, beams, k, max_t, min_t, seed):
    """The sampling decode's invariants (k hypotheses, no <UNK>, only the graph's own copies, min_time_step) and this search's: k
    distinct sequences in descending G, logq <= 0, the best G the root's and none above it"""
    from gtos_amd.search import stochastic_roots
    from test_sample_decode import _check_invariants
    roots = stochastic_roots(seed, len(beams))
    _check_invariants(model, memory, beams, k, max_t, min_t)
    for b, beam in enumerate(beams):
        seqs = [tuple(h.seq) for h in _hyps(beam)]
        assert len(set(seqs)) == len(seqs) == k, b
        for part in (beam.completed_hypotheses, beam.hypotheses):
            assert all(x.gumbel >= y.gumbel for x, y in zip(part, part[1:])), b
        assert max(h.gumbel for h in _hyps(beam)) == roots[b], b
        for h in _hyps(beam):
            assert h.logq <= 0.0 and h.gumbel <= roots[b] and math.isfinite(h.logq) and math.isfinite(h.gumbel), (b, h.seq)


@pytest.mark.gpu
def test_stochastic_end_to_end_fp32(monkeypatch):
    from test_device_beam_search import _synth_model
    from test_sample_decode import _capture_memory, _fresh, _samples, _teacher_forced
    from gtos_amd import search
    model, batch = _synth_model("C1", torch.float32)
    memory = _capture_memory(model, batch, monkeypatch)
    B = len(memory['local_idx2token'])
    k, max_t, min_t = 4, 12, 3
    run = lambda seed, sync=8, T=1.0: search.stochastic_beam_search_device(model, memory, _fresh(B, k, max_t, min_t), T, seed,
                                                                           sync_every=sync)
    for T, seed in ((1.0, 5), (f32(0.6), 17)):
        got = model.work(batch, k, max_t, min_t, search="stochastic", temperature=T, seed=seed)
        want, near = _host_search(model, memory, k, max_t, min_t, T, seed)
        _same_as_host(got, want, near)
        _check_stochastic(model, memory, got, k, max_t, min_t, seed)
        _teacher_forced(model, memory, got, k, max_t, min_t)
        assert _key(got) == _key(run(seed, T=T))
        for sync in (1, 64):
            assert _key(got) == _key(run(seed, sync, T=T)), sync
        for beam in got:
            best = beam.get_k_best(2, 0.6)
            assert 1 <= len(best) <= 2 and all(hasattr(h, "logq") for h in best)
    assert _key(run(5)) != _key(run(6))
    # one slot: the draw of the sampling decode for the same seed (the per-row constants do not move the arg-max over the same keys)
    for T in (1.0, f32(0.6)):
        one = model.work(batch, 1, max_t, min_t, search="stochastic", temperature=T, seed=41)
        ref = model.work(batch, 1, max_t, min_t, search="sample", temperature=T, seed=41)
        for b, (x, y) in enumerate(zip(one, ref)):
            assert [(h.seq, h.score) for h in _hyps(x)] == _samples(y), (T, b)
            assert x.steps == y.steps and len(x.completed_hypotheses) == len(y.completed_hypotheses), (T, b)


@pytest.mark.gpu
def test_stochastic_with_bans(monkeypatch):
    """no_repeat_ngram = 2 and an avoid list: no output repeats a bigram or holds an entry, and the run is the host loop's with the
    same bans"""
    from test_device_beam_search import _synth_model
    from test_sample_decode import _capture_memory, _ids_of
    from gtos_amd import search
    model, batch = _synth_model("C1", torch.float32)
    memory = _capture_memory(model, batch, monkeypatch)
    B = len(memory['local_idx2token'])
    k, max_t, min_t, T, seed = 4, 12, 3, 1.0, 23
    plain = model.work(batch, k, max_t, min_t, search="stochastic", temperature=T, seed=seed)
    # avoid, per graph: the first token of its first hypothesis (a word) and the first bigram of its second (a phrase)
    avoid = [[_hyps(beam)[0].seq[1], list(_hyps(beam)[1].seq[1:3])] for beam in plain]
    got = model.work(batch, k, max_t, min_t, search="stochastic", temperature=T, seed=seed, no_repeat_ngram=2, avoid=avoid)
    entries = [[[e] if isinstance(e, str) else e for e in row] for row in avoid]
    ids = search.avoid_ids(model, memory['local_idx2token'], entries)
    want, near = _host_search(model, memory, k, max_t, min_t, T, seed, no_repeat_ngram=2, avoid=ids)
    _same_as_host(got, want, near)
    _check_stochastic(model, memory, got, k, max_t, min_t, seed)
    for b, beam in enumerate(got):
        assert beam.avoid == entries[b]
        for h in _hyps(beam):
            words = h.seq[1:]
            grams = list(zip(words, words[1:]))
            assert len(set(grams)) == len(grams), (b, h.seq)
            for e in entries[b]:
                assert all(words[i:i + len(e)] != e for i in range(len(words) - len(e) + 1)), (b, e, h.seq)
    assert _key(got) != _key(plain)


@pytest.mark.gpu
def test_stochastic_end_to_end_bf16_c2(monkeypatch):
    """C2-shaped eval batch in bf16, 8 slots, 50 steps: the invariants, teacher-forced scores, and no host read inside the loop but
    the flag every sync_every steps (stats counts them and the two final tables)."""
    from test_device_beam_search import _synth_model
    from test_sample_decode import _capture_memory, _fresh, _teacher_forced
    from gtos_amd import search, ops
    model, batch = _synth_model("C2", torch.bfloat16)
    memory = _capture_memory(model, batch, monkeypatch)
    B = len(memory['local_idx2token'])
    k, max_t, min_t, sync = 8, 50, 2, 8
    reads, flags, inside = [0], [0], [False]

    def spy(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **kw):
            if self.is_cuda:
                if inside[0]:
                    reads[0] += 1
                elif name == "item":
                    flags[0] += 1
            return orig(self, *a, **kw)
        monkeypatch.setattr(torch.Tensor, name, f)
    for name in ("item", "cpu", "tolist", "numpy", "__bool__", "__int__", "__float__"):
        spy(name)

    def inside_of(fn):
        def f(*a, **kw):
            inside[0] = True
            try:
                return fn(*a, **kw)
            finally:
                inside[0] = False
        return f
    monkeypatch.setattr(model, "decode_slots", inside_of(model.decode_slots))
    for name in ("sbs_step", "sbs_advance", "beam_reorder"):
        monkeypatch.setattr(ops, name, inside_of(getattr(ops, name)))
    stats = {}
    beams = search.stochastic_beam_search_device(model, memory, _fresh(B, k, max_t, min_t), 0.9, 2026, sync_every=sync, stats=stats)
    monkeypatch.undo()
    assert reads[0] == 0
    assert stats["host_reads"] == flags[0] + 2 and flags[0] <= (max_t - 1) // sync and stats["steps"] <= max_t
    _check_stochastic(model, memory, beams, k, max_t, min_t, 2026)
    _teacher_forced(model, memory, beams, k, max_t, min_t)
