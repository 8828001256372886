"""Token-level attribution, kernel level and host glue (gtos_copy_explain_fwd, csrc/copy_explain.hip, the rule in
csrc/copy_explain_kernels.h, ops.copy_explain, Generator.explain, Explained.rows).  The model-level GPU tests are in
tests/test_score_explain_model.py.

Row r = (t, b):  q_k = g softmax(x)_k [k < V],  p_k = q_k + c sum_{s: cp_seq[s,b] == k} a_s over the row's universe (the columns [0, V)
and the distinct non-negative copy ids of graph b).  entropy = -sum p ln p, gate = c, copy_share = c mass_y / p_y, source / focus the
alignment argmaxes (lowest position among equals), rank = #{k != y: p_k > p_y} (strict; -1 for a y outside the universe).
``reference_explain`` states this in float64 on the dense row of test_score_eval.reference_eval.

Bars.  nll: exact (the header against gtos_eval::row_serial, the kernel against ops.copy_eval).  source / focus: equal on every row
(argmaxes over input values).  gate, copy_share, source_weight, focus_weight: rtol 1e-5 on the CPU, 1e-4 on the GPU, atol 1e-12 --
test_score_eval's bars for p_pred, the diverter drawn as there.  rank: |rank - ref| <= slack(row), slack = the number of universe columns
k != y with 0 < |p_k - p_y| <= 1e-5 p_y in float64; rows with slack > 0 may be at most 2 % of a case, asserted on the statement alone.
An EXACT tie gets no slack: rank is strict, equal inputs give equal p in the statement and in the kernel alike, so such a column must
be counted for neither -- and bf16-rounded logits tie exactly with the target's on 25-45 % of the rows at V ~ 10000, which a slack that
counted them would excuse wholesale.
entropy: |H - H_ref| <= eps * max(H_ref, max_k |x_k|): H is formed from differences and quotients of numbers of the logits' magnitude
(ln Z, E / Z), as test_score_eval's docstring says of nll.  eps is 4 x the worst ratio measured over the cases, rounded up to one digit:
  CPU (g++, the header):   worst ratio 1.3e-07 -> EPS_CPU = 6e-7  (cap 1e-5)
  GPU (MI355X, fp32/bf16): worst ratio 5.6e-08 -> EPS_GPU = 3e-7  (cap 1e-4); against the product's dense ll row the same bar plus the
                           1e-12 floor's contribution (V + copies) * 1e-12 * 27."""
import ctypes

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver
from test_score_eval import GPU_SHAPES, PAD, _c1, _p, dev, make_case, reference_eval

NEAR = 1e-5
SLACK_SHARE = 0.02
EPS_CPU = 6e-7
EPS_GPU = 3e-7
NAMES = ("nll", "entropy", "gate", "copy_share", "source", "source_weight", "focus", "focus_weight", "rank")
INT = ("source", "focus", "rank")

DRIVER = r"""
#include "copy_explain_kernels.h"
extern "C" void row(const float* x, int V, float d0, float d1, const float* a, int S, const int64_t* cp, int B, int b, int64_t y,
                    int64_t pad, float* f, int* i) {
    gtos_explain::row_serial(x, V, d0, d1, a, S, cp, B, b, y, pad, f, f + 1, f + 2, f + 3, i, f + 4, i + 1, f + 5, i + 2);
}
extern "C" void eval_nll(const float* x, int V, float d0, float d1, const float* a, int S, const int64_t* cp, int B, int b, int64_t y,
                         int64_t pad, float* nll) {
    int pred;
    float pp;
    gtos_eval::row_serial(x, V, d0, d1, a, S, cp, B, b, y, pad, nll, &pred, &pp);
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = compile_host_driver(tmp_path_factory, "explain_host", DRIVER)
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    so.row.argtypes, so.row.restype = [P, I, F, F, P, I, P, I, I, L, L, P, P], None
    so.eval_nll.argtypes, so.eval_nll.restype = [P, I, F, F, P, I, P, I, I, L, L, P], None
    return so


def host_rows(lib, x, div, a, cp, y, pad=PAD):
    """gtos_explain::row_serial on every row -> dict of [R] arrays, plus gtos_eval::row_serial's nll"""
    R, V = x.shape
    S, B = cp.shape
    out = {n: np.zeros(R, np.int32 if n in INT else np.float32) for n in NAMES}
    eval_nll = np.zeros(R, np.float32)
    cpc = np.ascontiguousarray(cp)
    for r in range(R):
        xr, ar = np.ascontiguousarray(x[r]), np.ascontiguousarray(a[r])
        f, i, n = np.zeros(6, np.float32), np.zeros(3, np.int32), np.zeros(1, np.float32)
        args = (_p(xr), V, float(div[r, 0]), float(div[r, 1]), _p(ar), S, _p(cpc), B, r % B, int(y[r]), pad)
        lib.row(*args, _p(f), _p(i))
        lib.eval_nll(*args, _p(n))
        for k, name in enumerate(("nll", "entropy", "gate", "copy_share", "source_weight", "focus_weight")):
            out[name][r] = f[k]
        out["source"][r], out["focus"][r], out["rank"][r] = i
        eval_nll[r] = n[0]
    return out, eval_nll


# ------------------------------------------------------------------------------------------------ the rule, stated in float64
def entropy_of(p):
    p = np.asarray(p, np.float64)
    return -(p * np.log(np.where(p > 0, p, 1.0))).sum(-1)


def reference_explain(x, div, a, cp, y, pad=PAD):
    """x [R,V], div [R,2], a [R,S], cp [S,B] (row r belongs to graph r % B), y [R] -> dict of the nine outputs [R] in float64 / int64
    plus ``slack`` [R] (universe columns k != y within 1e-5 relative of p_y without being equal to it), ``reachable`` [R] and the dense row ``p`` [R,C]."""
    nll, _, _, _, p = reference_eval(x, div, a, cp, y, pad)
    div, a = np.asarray(div, np.float64), np.asarray(a, np.float64)
    R, V = x.shape
    S, B = cp.shape
    C = p.shape[1]
    rows = np.arange(R)
    e = np.exp(div - div.max(1, keepdims=True))
    c = (e / e.sum(1, keepdims=True))[:, 1]
    universe = np.zeros((R, C), bool)
    universe[:, :V] = True
    ids = cp[:, rows % B].T if S else np.zeros((R, 0), np.int64)               # [R, S]
    for r in range(R):
        universe[r, ids[r][ids[r] >= 0]] = True
    live = (y != pad) & (y >= 0)
    inside = live & (y < C)
    yc = np.where(inside, y, 0)
    reach = inside & universe[rows, yc]
    p_y = np.where(reach, p[rows, yc], 0.0)
    holds = (ids == y[:, None]) & live[:, None]                                # positions whose copy id is the target
    cm = c * (a * holds).sum(1)
    share = np.where(reach & (p_y > 0), cm / np.where(p_y > 0, p_y, 1.0), 0.0)
    if S:
        masked = np.where(holds, a, -1.0)
        source = np.where(holds.any(1), masked.argmax(1), -1)                  # numpy: the first (lowest) among equals
        focus = a.argmax(1)
    else:
        source, focus = np.full(R, -1), np.full(R, -1)
    weight = lambda pos: np.where(pos >= 0, a[rows, np.maximum(pos, 0)], 0.0) if S else np.zeros(R)      # noqa: E731
    cols = np.arange(C)[None, :]
    rank = np.where(reach, ((p > p_y[:, None]) & universe).sum(1), -1)         # strict: the target's own column never counts
    near = (np.abs(p - p_y[:, None]) <= NEAR * p_y[:, None]) & (p != p_y[:, None])      # (an exact tie needs no slack: see the docstring)
    slack = np.where(reach, (near & universe & (cols != y[:, None])).sum(1), 0)
    return dict(nll=nll, entropy=entropy_of(p), gate=c, copy_share=share, source=source, source_weight=weight(source), focus=focus,
                focus_weight=weight(focus), rank=rank, slack=slack, reachable=reach, p=p)


def slack_share_ok(name, ref):
    share = float((ref["slack"] > 0).mean())
    assert share <= SLACK_SHARE, "%s: %.1f %% of the rows have a column within 1e-5 of the target's p" % (name, 100 * share)


def check_outputs(name, got, ref, x, rtol, eps):
    """``got``: dict of [R] arrays (nll is checked by the caller).  Returns the worst entropy ratio (err / scale)."""
    for k in ("source", "focus"):
        bad = np.nonzero(got[k] != ref[k])[0]
        assert bad.size == 0, "%s: %s differs on %d row(s), e.g. row %d: %d vs %d" % (name, k, bad.size, bad[0], got[k][bad[0]], ref[k][bad[0]])
    for k in ("gate", "copy_share", "source_weight", "focus_weight"):
        assert np.allclose(got[k], ref[k], rtol=rtol, atol=1e-12), "%s: %s off by %.3e" % (name, k, np.abs(got[k] - ref[k]).max())
    off = np.abs(got["rank"].astype(np.int64) - ref["rank"])
    bad = np.nonzero(off > ref["slack"])[0]
    assert bad.size == 0, "%s: rank differs on %d row(s) beyond the slack, e.g. row %d: %d vs %d (slack %d)" % (
        name, bad.size, bad[0], got["rank"][bad[0]], ref["rank"][bad[0]], ref["slack"][bad[0]])
    assert ((got["rank"] == -1) == ~ref["reachable"]).all(), name + ": rank is -1 exactly for an unreachable target"
    scale = np.maximum(ref["entropy"], np.abs(x).max(1).astype(np.float64))
    ratio = np.abs(got["entropy"].astype(np.float64) - ref["entropy"]) / scale
    print("MEASURED %s: entropy worst err/scale %.3e (max err %.3e, H in [%.3f, %.3f]), rows with slack %d" % (
        name, ratio.max(), np.abs(got["entropy"] - ref["entropy"]).max(), ref["entropy"].min(), ref["entropy"].max(),
        int((ref["slack"] > 0).sum())))
    assert (ratio <= eps).all(), "%s: entropy off by %.3e of its scale at row %d, bar %.1e" % (name, ratio.max(), ratio.argmax(), eps)
    return float(ratio.max())


def cpu_cases(rng):
    """(name, x, div, a, cp, y): V x S at T*B = 96, more positions than threads, and graphs whose positions all share one id"""
    for V in (7, 64, 1000):
        for S in (0, 1, 37):
            yield ("V=%d S=%d" % (V, S),) + make_case(rng, 24, 4, V, S, plant=False)[:5]
    yield ("V=130 S=300",) + make_case(rng, 24, 4, 130, 300, plant=False)[:5]
    x, div, a, cp, y, _ = make_case(rng, 24, 4, 64, 37, plant=False)
    cp[:, 1] = 5                                               # every position of graph 1 holds id 5 (< V), of graph 2 id 70 (>= V)
    cp[:, 2] = 70
    for r in range(96):
        if r % 4 == 1 and r % 3 == 0:
            y[r] = 5
        if r % 4 == 2 and r % 3 == 0:
            y[r] = 70
    yield ("one id per graph", x, div, a, cp, y)


# ------------------------------------------------------------------------------------------------ CPU
def test_header_rows_match_float64_statement(host_lib):
    """Measured with g++ -O2: worst entropy err/scale 1.275e-07 over these cases (V=1000, S=37) -> EPS_CPU = 6e-7."""
    rng = np.random.default_rng(20261020)
    seen = dict(pad=0, vocab=0, copy_lo=0, copy_hi=0, unreachable=0, share_between=0, source_none=0, shared_id=0, one_id_graph=0)
    worst = 0.0
    for name, x, div, a, cp, y in cpu_cases(rng):
        R, V = x.shape
        S, B = cp.shape
        ref = reference_explain(x, div, a, cp, y)
        slack_share_ok(name, ref)                             # a property of the case, judged on the float64 statement alone
        got, eval_nll = host_rows(host_lib, x, div, a, cp, y)
        assert np.array_equal(got["nll"].view(np.int32), eval_nll.view(np.int32)), name + ": nll is not gtos_eval::row_serial's"
        assert (got["nll"][y == PAD] == 0).all()
        worst = max(worst, check_outputs(name, got, ref, x, 1e-5, EPS_CPU))
        pad = y == PAD
        assert (got["copy_share"][pad] == 0).all() and (got["source"][pad] == -1).all() and (got["source_weight"][pad] == 0).all()
        assert (got["rank"][pad] == -1).all() and (got["entropy"][pad] > 0).all() and (got["gate"][pad] > 0).all()
        if S == 0:
            assert (got["focus"] == -1).all() and (got["focus_weight"] == 0).all()
        seen["shared_id"] += sum(len(set(cp[:, b])) < S for b in range(B))
        seen["one_id_graph"] += sum(S > 1 and len(set(cp[:, b])) == 1 for b in range(B))
        for r in range(R):
            own, yb = set(cp[:, r % B].tolist()), int(y[r])
            seen["pad" if yb == PAD else "copy_lo" if yb in own and yb < V else "copy_hi" if yb in own
                 else "unreachable" if yb >= V else "vocab"] += 1
        seen["share_between"] += int(((got["copy_share"] > 0) & (got["copy_share"] < 1)).sum())
        seen["source_none"] += int(((got["source"] == -1) & ~pad).sum())
    print("MEASURED header: worst entropy err/scale %.3e, EPS_CPU %.1e" % (worst, EPS_CPU))
    assert EPS_CPU <= 1e-5
    assert all(v > 0 for v in seen.values()), seen


def test_header_planted_rows(host_lib):
    V, S, B = 8, 4, 1
    x = np.array([[0, 1, 5, 1, 5, 0, -1, 2]], np.float32)
    cp = np.array([[3], [9], [9], [3]], np.int64)
    zero = np.zeros((1, S), np.float32)

    def run(a, y, d=(0.0, 0.0)):
        got, _ = host_rows(host_lib, x, np.array([d], np.float32), np.asarray(a, np.float32).reshape(1, S), cp, np.array([y], np.int64))
        return {k: v[0] for k, v in got.items()}
    # two equal largest logits, no copy mass: nothing beats the target on either column; the runner-up has both above it
    assert run(zero, 2)["rank"] == 0 and run(zero, 4)["rank"] == 0
    assert run(zero, 7)["rank"] == 2 and run(zero, 6)["rank"] == 7
    # a copy id >= V with positive mass: all of its probability was copied, exactly
    r = run([[0.1, 0.3, 0.2, 0.0]], 9)
    assert r["copy_share"] == 1.0 and r["source"] == 1 and abs(r["source_weight"] - 0.3) < 1e-7
    assert r["rank"] == 0                                      # p = c * 0.5 = 0.25 against g * s_2 = 0.238
    assert run([[0.1, 0.2, 0.2, 0.0]], 9)["rank"] == 2         # ... and 0.2 against it: columns 2 and 4 are above
    r = run(zero, 9)                                           # without mass: p_y = 0, every vocabulary column is above it
    assert r["copy_share"] == 0.0 and r["rank"] == 8 and r["source"] == 1 and r["source_weight"] == 0.0
    # held by two positions with equal weights: the lower position; focus likewise
    r = run([[0.25, 0.1, 0.1, 0.25]], 3)
    assert r["source"] == 0 and r["focus"] == 0 and 0 < r["copy_share"] < 1
    r = run([[0.0, 0.2, 0.2, 0.0]], 9)
    assert r["source"] == 1 and r["focus"] == 1
    # a target nobody owns, a padded row
    r = run([[0.1, 0.3, 0.2, 0.0]], 77)
    assert r["rank"] == -1 and r["source"] == -1 and r["copy_share"] == 0 and abs(r["nll"] - 27.631021) < 1e-4
    r = run([[0.1, 0.3, 0.2, 0.0]], PAD)
    assert r["nll"] == 0 and r["rank"] == -1 and r["source"] == -1 and r["focus"] == 1 and r["entropy"] > 0 and r["gate"] == 0.5


def test_argument_checks_abi_and_exports():
    from dryrun import DryRun
    from gtos_amd import _lib, build, ops
    from gtos_amd._lib import GtosHipError
    assert _lib.ABI_VERSION >= 34
    assert len(_lib.SIGNATURES["gtos_copy_explain_fwd"]) == 22 and len(ops.EXPLAIN_OUTPUTS) == 9
    lg, dv, al = torch.zeros(2, 3, 8), torch.zeros(2, 3, 2), torch.zeros(2, 3, 4)
    cp, y = torch.zeros(4, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(GtosHipError, match="GPU only"):
        ops.copy_explain(lg, dv, al, cp, y, PAD)
    with DryRun() as rec:
        out = ops.copy_explain(lg, dv, al, cp, y, PAD)
        assert [t.dtype for t in out] == [d for _, d in ops.EXPLAIN_OUTPUTS] and all(t.shape == (2, 3) for t in out)
        name, args = rec.calls[-1]
        assert name == "gtos_copy_explain_fwd" and args[:5] == (0, 2, 3, 8, 4) and args[6] == 8 and args[11] == PAD
        assert list(args[12:21]) == [t.data_ptr() for t in out]
        assert ops.copy_explain(lg, dv, al, cp, y, PAD, out=out)[4] is out[4]
        with pytest.raises(GtosHipError, match="int64"):
            ops.copy_explain(lg, dv, al, cp.int(), y, PAD)
        with pytest.raises(GtosHipError, match="int64"):
            ops.copy_explain(lg, dv, al, cp, y[:1], PAD)
        with pytest.raises(GtosHipError, match="one per output"):
            ops.copy_explain(lg, dv, al, cp, y, PAD, out=out[:3])
        with pytest.raises(GtosHipError, match=r"out\[source\]"):
            ops.copy_explain(lg, dv, al, cp, y, PAD, out=out[:4] + (out[0],) + out[5:])
        with pytest.raises(GtosHipError, match=r"out\[rank\]"):
            ops.copy_explain(lg, dv, al, cp, y, PAD, out=out[:8] + (torch.zeros(3, 2, dtype=torch.int32),))
    # the C entry refuses before it launches: none of these calls reaches the device
    lib = ctypes.CDLL(build.build(verbose=False))
    fn = lib.gtos_copy_explain_fwd
    fn.argtypes, fn.restype = _lib.SIGNATURES["gtos_copy_explain_fwd"], ctypes.c_int
    ok = [0, 2, 3, 8, 4, 64, 8, 64, 64, 64, 64, PAD] + [64] * 9 + [None]          # (64: a pointer that is not null; never followed)

    def with_(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return fn(*a)
    assert with_(a1=0) == 0 and with_(a2=0) == 0 and with_(a1=-1) == 0             # T * B <= 0: nothing to do
    assert with_(a3=0) == -24 and with_(a4=-1) == -24 and with_(a4=4097) == -24 and with_(a6=7) == -24
    for k in (5, 7, 8, 9, 10) + tuple(range(12, 21)):
        assert with_(**{"a%d" % k: None}) == -23, k
    assert with_(a4=0, a8=None, a9=None, a3=0) == -24                              # shapes are judged first


def test_dry_run_launch_plans():
    from dryrun import DryRun
    from gtos_amd import ops
    from gtos_amd.generator import Explained
    with DryRun() as rec:
        trainer, batch = _c1()
        model = trainer.model
        B, T = batch['concept'].size(1), batch['token_out'].size(0)
        seed = ops._seed_state[0]
        model.relation_encoder.trie_in_eval = "as found"
        n0 = len(rec.calls)
        ex = model.explain(batch)
        names = [n for n, _ in rec.calls[n0:]]
        assert names.count("gtos_copy_explain_fwd") == 1
        assert not any(n in ("gtos_copy_eval_fwd", "gtos_copy_ll_fwd", "gtos_eval_accumulate") or n.startswith("gtos_copy_nll") or "bwd" in n
                       for n in names), sorted(set(names))
        assert isinstance(ex, Explained) and ex._fields == ("token_ll", "entropy", "copy_gate", "copy_share", "source", "source_weight",
                                                            "focus", "focus_weight", "rank", "tokens", "graph_of")
        for k in ex._fields[:9]:
            assert getattr(ex, k).shape == (T, B) and getattr(ex, k).dtype == (torch.int32 if k in INT else torch.float32), k
        assert ex.tokens.dtype == torch.int32 and ex.tokens.tolist() == batch['token_out'].ne(PAD).sum(0).tolist()
        assert ex.graph_of.tolist() == list(range(B))
        assert model.training and ops._seed_state[0] == seed and not ops._DW_PENDING.get(batch['concept'].device)
        assert model.relation_encoder.trie_in_eval == "as found"
        model.relation_encoder.trie_in_eval = True
        # the same launches as score, but for its last
        n1 = len(rec.calls)
        model.score(batch)
        score_names = [n for n, _ in rec.calls[n1:]]
        assert "gtos_copy_explain_fwd" not in score_names
        assert [n for n in names if n != "gtos_copy_explain_fwd"] == [n for n in score_names if n != "gtos_copy_eval_fwd"]
        # an n-best list per graph: one string list, a list of them, an empty list
        n0 = len(rec.calls)
        targets = [["w1", "w2"], [["w3"], ["w1", "copy-me", "w2", "w2"]]] + [[] for _ in range(B - 2)]
        en = model.explain(batch, targets)
        name, args = [c for c in rec.calls[n0:] if c[0] == "gtos_copy_explain_fwd"][0]
        assert [n for n, _ in rec.calls[n0:]].count("gtos_copy_explain_fwd") == 1
        assert en.graph_of.tolist() == [0, 1, 1] and en.tokens.tolist() == [3, 2, 5] and en.rank.shape == (5, 3)
        assert args[1:3] == (5, 3) and args[4] == batch['cp_seq'].size(0)
        assert [len(s) for s in en.rows(batch)] == [3, 2, 5]
        # all n-best lists empty: nothing is launched
        n0 = len(rec.calls)
        none = model.explain(batch, [[] for _ in range(B)])
        assert len(rec.calls) == n0 and none.rank.shape == (0, 0) and none.rank.dtype == torch.int32 and none.graph_of.shape == (0,)
        assert none.rows(batch) == []
        with pytest.raises(ValueError, match="one entry per graph"):
            model.explain(batch, [["a"]] * (B + 1))
        # eval mode is left as found, too
        model.eval()
        model.explain(batch)
        assert not model.training and not any(m.training for m in model.modules())
        model.train()
        # evaluate and a training step hold no explain launch
        n0 = len(rec.calls)
        trainer.evaluate([batch])
        ops.set_seed(12345)
        trainer.step(batch, sync=False)
        names = [n for n, _ in rec.calls[n0:]]
        assert "gtos_copy_explain_fwd" not in names and "gtos_copy_eval_fwd" in names and "gtos_copy_nll_fwd" in names


def test_explained_rows_by_hand():
    """Two sequences against graphs 1 and 0, T = 3: padded positions are skipped, copy ids resolve through the graph's table, the
    rest through the vocabulary, the nodes through the concept vocabulary (position s is row s + 1 of data['concept'])."""
    from gtos_amd.generator import Explained

    class Vocab:
        def __init__(self, words):
            self.words = words

        def idx2token(self, i):
            return self.words[i]
    f = lambda *v: torch.tensor(v, dtype=torch.float32).t()        # noqa: E731   (written per sequence, stored [T, N])
    i = lambda *v: torch.tensor(v, dtype=torch.int32).t()          # noqa: E731
    ex = Explained(token_ll=f([-0.5, -1.5, 0.0], [-0.25, -2.0, -3.0]), entropy=f([1.0, 2.0, 9.0], [0.5, 0.25, 0.125]),
                   copy_gate=f([0.5, 0.25, 9.0], [0.75, 0.5, 0.25]), copy_share=f([1.0, 0.0, 0.0], [0.5, 0.0, 0.0]),
                   source=i([1, -1, -1], [0, -1, -1]), source_weight=f([0.75, 0.0, 0.0], [0.5, 0.0, 0.0]),
                   focus=i([1, 0, 0], [0, 1, 1]), focus_weight=f([0.75, 0.5, 9.0], [0.5, 0.5, 0.5]), rank=i([0, 3, -1], [1, 0, -1]),
                   tokens=torch.tensor([2, 3], dtype=torch.int32), graph_of=torch.tensor([1, 0]))
    ex.target = torch.tensor([[5, 2, PAD], [4, 1, 3]]).t()
    ex.vocab, ex.concept_vocab = Vocab(["<pad>", "a", "b", "c"]), Vocab(["<pad>", "<cls>", "boy", "want-01", "Paris"])
    data = {'local_idx2token': [{4: "want", 5: "never"}, {4: "wrong", 5: "Paris"}],
            'concept': torch.tensor([[1, 3, 2], [1, 2, 4]]).t()}
    rows = ex.rows(data)
    assert [len(r) for r in rows] == [2, 3]
    assert [d["token"] for d in rows[0]] == ["Paris", "b"] and [d["token"] for d in rows[1]] == ["want", "a", "c"]
    assert rows[0][0] == {"token": "Paris", "ll": -0.5, "entropy": 1.0, "copy_gate": 0.5, "copy_share": 1.0, "rank": 0, "source": 1,
                          "focus": 1, "source_concept": "Paris", "focus_concept": "Paris"}
    assert rows[0][1]["source"] == -1 and rows[0][1]["source_concept"] is None and rows[0][1]["focus_concept"] == "boy"
    assert rows[1][0]["token"] == "want" and rows[1][0]["source_concept"] == "want-01" and rows[1][1]["focus_concept"] == "boy"
    # without the concept ids there are no node strings; an explicit vocabulary overrides the instance's
    bare = ex.rows({'local_idx2token': data['local_idx2token']}, vocab=Vocab(["P", "A", "B", "C"]))
    assert "source_concept" not in bare[0][0] and bare[0][1]["token"] == "B" and bare[0][0]["token"] == "Paris"


# ------------------------------------------------------------------------------------------------ GPU: the kernel
EXPLAIN_SHAPES = GPU_SHAPES + [(4, 3, 130, 300)]
_CASES = {}


def gpu_case(T, B, V, S, dtype):
    """The inputs on the device and the float64 statement on the SAME inputs (bf16-rounded where the kernel reads bf16).  The host
    side is built once per (shape, dtype), shared by the tests below and left unchanged; the device copies are made per call, so that
    no device memory stays allocated after a test."""
    key = (T, B, V, S, dtype)
    if key not in _CASES:
        rng = np.random.default_rng(31 + V + S)
        x, div, a, cp, y, _ = make_case(rng, T, B, V, S, plant=False)
        lg = torch.from_numpy(x).to(dtype).reshape(T, B, V)
        dv = torch.from_numpy(div).to(dtype).reshape(T, B, 2)
        R = T * B
        xr = lg.float().numpy().reshape(R, V)
        ref = reference_explain(xr, dv.float().numpy().reshape(R, 2), a, cp, y)
        ref.pop("p")                                           # (the dense float64 row: 257 MB at the largest shape)
        _CASES[key] = ((lg, dv, torch.from_numpy(a).reshape(T, B, S), torch.from_numpy(cp), torch.from_numpy(y).reshape(T, B)), xr, ref)
    host, xr, ref = _CASES[key]
    return tuple(t.to(dev()) for t in host) + (xr, ref)


def as_numpy(out):
    return {n: t.cpu().numpy().reshape(-1) for n, t in zip(NAMES, out)}


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,B,V,S", EXPLAIN_SHAPES)
def test_copy_explain_vs_float64_statement_guarded(T, B, V, S, dtype):
    """Measured on the MI355X: worst entropy err/scale 5.618e-08 over these shapes and both dtypes (fp32, V=10000, S=101) ->
    EPS_GPU = 3e-7."""
    from gtos_amd import ops
    from tests_support import nan_buffer
    lg, dv, al, cp, y, xr, ref = gpu_case(T, B, V, S, dtype)
    R = T * B
    slack_share_ok("T*B=%d V=%d S=%d" % (R, V, S), ref)
    buf = nan_buffer(9 * (R + 128) + 128, torch.float32, dev())
    out = tuple(buf.carve(128 + k * (R + 128), T, B, B) for k in range(9))
    out = tuple(t.view(torch.int32) if n in INT else t for n, t in zip(NAMES, out))
    ret = ops.copy_explain(lg, dv, al, cp, y, PAD, out=out)
    torch.cuda.synchronize()
    buf.check("the nine outputs")
    assert all(r.data_ptr() == o.data_ptr() for r, o in zip(ret, out))
    nll = ops.copy_eval(lg, dv, al, cp, y, PAD)[0]
    assert torch.equal(out[0].view(torch.int32), nll.view(torch.int32)), "nll is not bitwise gtos_copy_eval_fwd's"
    got = as_numpy(out)
    check_outputs("copy_explain %s T*B=%d V=%d S=%d" % (dtype, R, V, S), got, ref, xr, 1e-4, EPS_GPU)
    pad = y.cpu().numpy().reshape(R) == PAD
    assert (got["nll"][pad] == 0).all() and (got["copy_share"][pad] == 0).all() and (got["source"][pad] == -1).all()
    assert (got["source_weight"][pad] == 0).all() and (got["rank"][pad] == -1).all()
    assert EPS_GPU <= 1e-4
    # the plain call allocates its own outputs; a second launch gives the same bits in all nine
    again = ops.copy_explain(lg, dv, al, cp, y, PAD)
    for n, t, u in zip(NAMES, out, again):
        assert torch.equal(t.view(torch.int32), u.view(torch.int32)), n + " differs between two launches"


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,B,V,S", EXPLAIN_SHAPES)
def test_copy_explain_vs_the_dense_ll_row(T, B, V, S, dtype):
    """p = exp(copy_log_likelihood) - 1e-12, clamped at 0, is the product's own dense row: its entropy and the rank it gives the
    target are the kernel's, within the bar of the test above plus what the floor can add, (V + copies) * 1e-12 * 27."""
    from gtos_amd import ops
    lg, dv, al, cp, y, xr, ref = gpu_case(T, B, V, S, dtype)
    R = T * B
    got = as_numpy(ops.copy_explain(lg, dv, al, cp, y, PAD))
    tot = max(V, 1 + int(cp.max())) if S else V
    ll = ops.copy_log_likelihood(lg, dv, al, cp, tot).reshape(R, tot)
    p = (torch.exp(ll.double()) - 1e-12).clamp(min=0).cpu().numpy()
    H = entropy_of(p)
    scale = np.maximum(ref["entropy"], np.abs(xr).max(1).astype(np.float64))
    bar = EPS_GPU * scale + tot * 1e-12 * 27
    err = np.abs(got["entropy"] - H)
    print("MEASURED dense row %s T*B=%d V=%d S=%d: entropy max err %.3e, worst err / bar %.3f" % (
        dtype, R, V, S, err.max(), (err / bar).max()))
    assert (err <= bar).all(), "entropy off the dense row's by %.3e at a bar of %.3e" % (err.max(), bar[err.argmax()])
    yv = y.cpu().numpy().reshape(R)
    reach = ref["reachable"]
    p_y = p[np.arange(R), np.where(reach, yv, 0)]
    rank = (p > p_y[:, None]).sum(1)
    off = np.abs(got["rank"].astype(np.int64) - rank)
    bad = np.nonzero(reach & (off > ref["slack"]))[0]
    assert bad.size == 0, "rank differs from the dense row's on %d row(s) beyond the slack, e.g. row %d: %d vs %d (p_y %.3e)" % (
        bad.size, bad[0], got["rank"][bad[0]], rank[bad[0]], p_y[bad[0]])
