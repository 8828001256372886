"""Teacher-forced scoring, kernel level and host glue (gtos_copy_eval_fwd / gtos_eval_accumulate, csrc/copy_eval.hip, the rule in
csrc/copy_eval_kernels.h, ops.copy_eval / ops.eval_accumulate, Generator.score, Trainer.evaluate).

Row r = (t, b):  p_k = g softmax(x)_k [k < V] + c sum_{s: cp_seq[s,b] == k} a_s,  nll = -log(p_y + 1e-12) (0 at y == pad),
pred = argmax_k p_k with equal values to the LOWER column, p_pred = p_pred's value.
CPU: the rule header compiled with g++ against a float64 numpy statement, the argument checks, the dry-run launch plans and the one
collective of a two-rank evaluation.  GPU: the kernels against the float64 statement inside NaN guard bands, bitwise against
gtos_copy_nll_fwd, and the accumulation.  The model-level GPU tests are in tests/test_score_eval_model.py.

Bars.  ``pred`` must be equal on every row that is not a NEAR TIE (the two largest float64 p differ by less than 1e-5 relative without
being equal); near ties may be at most 1 % of a case's rows, asserted on the float64 statement before the output is looked at.
``nll`` on the CPU: 1e-6 relative.  nll = lse - x_y - log(g) (or the log of a copy mass) is a DIFFERENCE of fp32 numbers of the
logits' magnitude, and the kernel's arithmetic is pinned bitwise to gtos_copy_nll_fwd, so "relative" is taken to the larger of
|nll| and max_k |x_k| of the row: a confident row's nll ~ 1e-2 cannot be resolved to 1e-8 by an lse ~ 13 that fp32 holds to 5e-7.
The diverter scores are drawn with |d0 - d1| <= 3: gtos_copy_nll_fwd forms c = 1 - g, whose absolute error 2^-24 is a relative error
2^-24 / c of a copy target's p, inside the bar for c >= 0.047 and not below (a property of the existing kernel, kept bitwise).
On the GPU nll is held to test_label_smoothing.within() as the kernels of the smoothed loss are."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver

PAD = 0
NEAR = 1e-5
NEAR_SHARE = 0.01

DRIVER = r"""
#include "copy_eval_kernels.h"
extern "C" void row(const float* x, int V, float d0, float d1, const float* a, int S, const int64_t* cp, int B, int b, int64_t y,
                    int64_t pad, float* nll, int* pred, float* p_pred) {
    gtos_eval::row_serial(x, V, d0, d1, a, S, cp, B, b, y, pad, nll, pred, p_pred);
}
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = compile_host_driver(tmp_path_factory, "eval_host", DRIVER)
    P, I, L, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
    so.row.argtypes, so.row.restype = [P, I, F, F, P, I, P, I, I, L, L, P, P, P], None
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


# ------------------------------------------------------------------------------------------------ the rule, stated in float64
def reference_eval(x, div, a, cp, y, pad=PAD):
    """x [R,V], div [R,2], a [R,S], cp [S,B] (row r belongs to graph r % B), y [R] -> nll [R], pred [R], p_pred [R], near [R] (bool):
    the dense row p [R,C], C = max(V, 1 + max(cp)), its gather at y (p = 0 for a y outside [0, C)), its argmax with the lowest column
    among equals, and whether the row's two largest p are a near tie."""
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
    if S:
        ids = cp[:, np.arange(R) % B].T                                      # [R, S]
        keep = ids >= 0
        rows = np.repeat(np.arange(R), S).reshape(R, S)
        np.add.at(p, (rows[keep], ids[keep]), (c * a)[keep])
    inside = (y >= 0) & (y < C)
    py = np.where(inside, p[np.arange(R), np.where(inside, y, 0)], 0.0)
    nll = np.where(y != pad, -np.log(py + 1e-12), 0.0)
    pred = p.argmax(1)                                                       # numpy: the first (lowest) among equals
    if C > 1:
        top2 = -np.partition(-p, 1, axis=1)[:, :2]
        near = (top2[:, 0] != top2[:, 1]) & (top2[:, 0] - top2[:, 1] < NEAR * top2[:, 0])
    else:
        near = np.zeros(R, bool)
    return nll, pred, p[np.arange(R), pred], near, p


def make_case(rng, T, B, V, S, plant=True):
    """Random rows for the rule.  Logits 4 randn; diverter scores uniform in [-1.5, 1.5]; alignment rows normalised, half of them
    peaked on one position (so that a copy group can beat the best vocabulary column) and some with zeros; copy ids below V (repeated
    within a graph) and above V; targets <pad>, vocabulary ids, the graph's own copy ids and ids nobody owns.  With ``plant``: rows
    with two EQUAL largest logits and no copy mass (the lower column must win), the higher of the two being a copy id of the graph
    where it has one (a copy group on a column whose c * mass is 0 ties with the vocabulary candidate), and rows whose largest logit
    sits on a copy id with zero mass.  Returns x, div, a, cp, y and the planted rows."""
    R = T * B
    x = (rng.standard_normal((R, V)) * 4).astype(np.float32)
    div = rng.uniform(-1.5, 1.5, (R, 2)).astype(np.float32)
    a = rng.random((R, S)).astype(np.float32)
    a[rng.random((R, S)) < 0.2] = 0.0
    if S:
        pk = np.nonzero(rng.random(R) < 0.5)[0]
        a[pk, rng.integers(0, S, len(pk))] += 6.0
    a /= np.maximum(a.sum(1, keepdims=True), 1e-6)
    cp = np.empty((S, B), np.int64)
    nxt = V
    for b in range(B):
        for s in range(S):
            r = rng.random()
            if r < 0.35:
                cp[s, b] = nxt + rng.integers(0, 3)              # ids >= V, repeated
            elif r < 0.7 or s == 0:
                cp[s, b] = rng.integers(1, V)
            else:
                cp[s, b] = cp[rng.integers(0, s), b]             # several positions share an id
        nxt += 3
    y = rng.integers(1, V, R).astype(np.int64)
    for r in range(R):
        k = rng.random()
        if k < 0.1:
            y[r] = PAD
        elif k < 0.45 and S:
            y[r] = cp[rng.integers(0, S), r % B]
        elif k < 0.55:
            y[r] = V + rng.integers(0, nxt - V + 4)              # another graph's id, or an id nobody owns (possibly >= C)
    planted = []
    if plant and V >= 3:
        for r in rng.choice(R, size=min(R, 6), replace=False):
            b = r % B
            own_lo = sorted(int(i) for i in cp[:, b] if 1 <= i < V) if S else []
            top = float(x[r].max())
            if len(planted) % 2 == 0:                            # two equal largest logits, no copy mass
                j2 = own_lo[-1] if own_lo else int(rng.integers(1, V))
                j1 = int(rng.integers(0, j2))
                x[r, j1] = x[r, j2] = np.float32(top + 6.0)
            elif own_lo:                                         # the largest logit on a copy id with zero mass
                x[r, own_lo[0]] = np.float32(top + 6.0)
            a[r] = 0.0
            planted.append(int(r))
    return x, div, a, cp, y, planted


def check_pred(name, pred, ref_pred, near):
    pred, ref_pred = np.asarray(pred).reshape(-1), np.asarray(ref_pred).reshape(-1)
    bad = (pred != ref_pred) & ~near
    assert not bad.any(), "%s: pred differs on %d row(s) that are no near tie, e.g. row %d: %d vs %d" % (
        name, int(bad.sum()), int(np.nonzero(bad)[0][0]), int(pred[bad][0]), int(ref_pred[bad][0]))


# ------------------------------------------------------------------------------------------------ CPU
def test_header_rows_match_float64_statement(host_lib):
    rng = np.random.default_rng(20261016)
    seen = dict(pad=0, vocab=0, copy_lo=0, copy_hi=0, unreachable=0, copy_wins=0, vocab_wins=0, exact_tie=0, shared_id=0)
    worst = 0.0
    for V in (7, 64, 1000):
        for S in (0, 1, 37):
            T, B = 24, 4
            R = T * B
            x, div, a, cp, y, planted = make_case(rng, T, B, V, S)
            nll_ref, pred_ref, pp_ref, near, p = reference_eval(x, div, a, cp, y)
            # the share of near ties is a property of the case, judged on the float64 statement alone
            assert near.mean() <= NEAR_SHARE, "V=%d S=%d: %d of %d rows are near ties" % (V, S, int(near.sum()), R)
            top2 = -np.partition(-p, 1, axis=1)[:, :2]
            seen["exact_tie"] += int((top2[:, 0] == top2[:, 1]).sum())
            assert not planted or (top2[planted[0], 0] == top2[planted[0], 1]), "the planted tie is not exact in float64"
            seen["shared_id"] += sum(len(set(cp[:, b])) < S for b in range(B))
            nll, pred, pp = np.zeros(R, np.float32), np.zeros(R, np.int32), np.zeros(R, np.float32)
            cpc = np.ascontiguousarray(cp)
            for r in range(R):
                xr, ar = np.ascontiguousarray(x[r]), np.ascontiguousarray(a[r])
                o1, o2, o3 = np.zeros(1, np.float32), np.zeros(1, np.int32), np.zeros(1, np.float32)
                host_lib.row(_p(xr), V, float(div[r, 0]), float(div[r, 1]), _p(ar), S, _p(cpc), B, r % B, int(y[r]), PAD,
                             _p(o1), _p(o2), _p(o3))
                nll[r], pred[r], pp[r] = o1[0], o2[0], o3[0]
                own = set(cp[:, r % B].tolist())
                yb = int(y[r])
                seen["pad" if yb == PAD else "copy_lo" if yb in own and yb < V else "copy_hi" if yb in own
                     else "unreachable" if yb >= V else "vocab"] += 1
                if S and not near[r]:
                    seen["copy_wins" if (int(pred_ref[r]) in own and a[r].sum() > 0) else "vocab_wins"] += 1
            bound = 1e-6 * np.maximum(np.abs(nll_ref), np.abs(x).max(1).astype(np.float64))
            err = np.abs(nll.astype(np.float64) - nll_ref)
            worst = max(worst, float((err / bound).max()))
            print("MEASURED V=%d S=%d: nll max err %.3e, max err/bound %.3f, near ties %d" % (V, S, err.max(), (err / bound).max(),
                                                                                               int(near.sum())))
            assert (err <= bound).all(), "V=%d S=%d: nll off by %.3e at a bound of %.3e" % (
                V, S, float(err[np.argmax(err / bound)]), float(bound[np.argmax(err / bound)]))
            assert (nll[y == PAD] == 0).all()
            check_pred("V=%d S=%d" % (V, S), pred, pred_ref, near)
            ok = ~near
            assert np.allclose(pp[ok], pp_ref[ok], rtol=1e-5, atol=1e-12)
    assert all(v > 0 for v in seen.values()), seen


def test_header_planted_ties_take_the_lower_column(host_lib):
    """Exact ties, by hand: two equal logits, a copy id ON the higher of them with zero mass (lower column), with mass (it wins);
    a copy group above V that loses / wins; eight equal logits; a padded row; a target nobody owns."""
    V, S, B = 8, 3, 1
    x = np.array([0, 1, 5, 1, 5, 0, -1, 2], np.float32)
    cp = np.array([[4], [9], [9]], np.int64)

    def run(xr, a, d=(0.0, 0.0), y=3):
        o1, o2, o3 = np.zeros(1, np.float32), np.zeros(1, np.int32), np.zeros(1, np.float32)
        ar = np.asarray(a, np.float32)
        host_lib.row(_p(np.ascontiguousarray(xr)), V, d[0], d[1], _p(ar), S, _p(cp), B, 0, y, PAD, _p(o1), _p(o2), _p(o3))
        return float(o1[0]), int(o2[0]), float(o3[0])
    assert run(x, [0, 0, 0])[1] == 2                       # columns 2 and 4 tie, column 4 is a copy id with c * mass = 0
    assert run(x, [0.5, 0, 0])[1] == 4                     # ... and with mass it wins
    assert run(x, [0, 0.2, 0.2])[1] == 2                   # group 9: c * 0.4 = 0.2 < g * s_2 = 0.238
    assert run(x, [0, 0.3, 0.3])[1] == 9                   # ... and 0.3 beats it: a column above V
    x1 = np.zeros(8, np.float32)                           # eight equal logits: the lowest column, p = g / 8
    nll, pred, pp = run(x1, [0, 0, 0])
    assert pred == 0 and abs(pp - 0.0625) < 1e-7
    assert run(x1, [0, 0.125, 0.125])[1] == 9              # c * 0.25 = 1/8 > 1/16
    assert run(x1, [0, 0, 0], y=PAD)[0] == 0.0 and run(x1, [0, 0, 0], y=PAD)[1] == 0      # a padded row: nll 0, pred still the argmax
    assert abs(run(x1, [0, 0, 0], y=77)[0] - 27.631021) < 1e-4                           # an id nobody owns: -log(1e-12)


def test_argument_checks():
    from gtos_amd import ops
    from gtos_amd._lib import GtosHipError
    from gtos_amd.data import batchify_targets
    lg, dv, al = torch.zeros(2, 3, 8), torch.zeros(2, 3, 2), torch.zeros(2, 3, 4)
    cp, y = torch.zeros(4, 3, dtype=torch.int64), torch.zeros(2, 3, dtype=torch.int64)
    with pytest.raises(GtosHipError, match="GPU only"):
        ops.copy_eval(lg, dv, al, cp, y, PAD)
    with pytest.raises(GtosHipError, match="GPU only"):
        ops.eval_accumulate(torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.int32), y, PAD, torch.zeros(5, dtype=torch.float64))
    with pytest.raises(ValueError):
        batchify_targets([["a"], ["b"]], {}, [{}])
    with pytest.raises(ValueError):
        batchify_targets([["a", 3]], {}, [{}])


def _c1():
    from gtos_amd import synth
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.relindex import attach_relation_index
    from gtos_amd.train import Trainer
    cpu = torch.device("cpu")
    cfg = synth.CONFIGS["C1"]
    model = Generator(synth.synth_vocabs(), device=cpu, **generator_args(cfg)).to(cpu)       # (real vocabularies: targets are strings)
    model.set_compute_dtype(torch.bfloat16)
    model.train()
    trainer = Trainer(model, cfg["d"], warmup_steps=2000, compute_dtype=torch.bfloat16, world_size=1, rank=0)
    batch, _ = synth.make_config_batch("C1", rank=0)
    attach_relation_index(attach_path_trie(batch))
    pv = trainer.model.vocabs['predictable_token']
    cp = batch['cp_seq']
    batch['local_idx2token'] = [{int(i): "copy%d" % int(i) for i in cp[:, b].tolist() if i >= pv.size} for b in range(cp.shape[1])]
    return trainer, batch


def test_score_argument_checks_under_dry_run():
    from dryrun import DryRun
    with DryRun():
        trainer, batch = _c1()
        B = batch['concept'].size(1)
        with pytest.raises(ValueError, match="one entry per graph"):
            trainer.model.score(batch, [["a"]] * (B + 1))
        with pytest.raises(ValueError, match="token strings"):
            trainer.model.score(batch, [["a", 5]] + [[]] * (B - 1))
        with pytest.raises(ValueError, match="token strings"):
            trainer.model.score(batch, [[["a"], "b"]] + [[]] * (B - 1))
        bare = {k: v for k, v in batch.items() if k != 'local_idx2token'}
        with pytest.raises(ValueError, match="copy table"):
            trainer.model.score(bare, [["a"]] * B)


def test_dry_run_launch_plans():
    from dryrun import DryRun
    from gtos_amd import ops
    with DryRun() as rec:
        trainer, batch = _c1()
        model = trainer.model
        B = batch['concept'].size(1)
        seed = ops._seed_state[0]
        n0 = len(rec.calls)
        sc = model.score(batch)
        names = [n for n, _ in rec.calls[n0:]]
        assert names.count("gtos_copy_eval_fwd") == 1
        assert not any(n == "gtos_copy_ll_fwd" or n.startswith("gtos_copy_nll") or "bwd" in n or n == "gtos_eval_accumulate"
                       for n in names), sorted(set(names))
        T = batch['token_out'].size(0)
        assert sc.sentence_ll.shape == (B,) and sc.sentence_ll.dtype == torch.float64
        assert sc.tokens.dtype == sc.correct.dtype == sc.pred.dtype == torch.int32 and sc.token_ll.dtype == torch.float32
        assert sc.token_ll.shape == sc.pred.shape == (T, B) and sc.graph_of.tolist() == list(range(B))
        assert sc.tokens.tolist() == batch['token_out'].ne(PAD).sum(0).tolist()
        assert model.training and ops._seed_state[0] == seed and not ops._DW_PENDING.get(batch['concept'].device)
        # an n-best list per graph: one string list, a list of them, an empty list
        n0 = len(rec.calls)
        targets = [["w1", "w2"], [["w3"], ["w1", "copy-me", "w2", "w2"]]] + [[] for _ in range(B - 2)]
        sn = model.score(batch, targets)
        names = [n for n, _ in rec.calls[n0:]]
        assert names.count("gtos_copy_eval_fwd") == 1 and sn.graph_of.tolist() == [0, 1, 1]
        assert sn.tokens.tolist() == [3, 2, 5] and sn.pred.shape == (5, 3)
        assert [len(s) for s in sn.strings(batch)] == [3, 2, 5]
        name, args = [c for c in rec.calls[n0:] if c[0] == "gtos_copy_eval_fwd"][0]
        assert args[1:3] == (5, 3) and args[4] == batch['cp_seq'].size(0)         # T, N and S of the gathered graph memory
        model.eval()
        model.score(batch)
        assert not model.training and not any(m.training for m in model.modules())
        model.train()
        # evaluate over two batches: score + accumulate per batch, nothing else new
        n0 = len(rec.calls)
        res = trainer.evaluate([batch, batch])
        names = [n for n, _ in rec.calls[n0:]]
        assert names.count("gtos_copy_eval_fwd") == 2 and names.count("gtos_eval_accumulate") == 2
        assert not any("bwd" in n or n.startswith("gtos_adam") or n == "gtos_step_control" for n in names)
        assert set(res) == {"nll_per_token", "perplexity", "accuracy", "tokens", "sentences", "loss"}
        assert model.training and ops._seed_state[0] == seed
    # a training step launches the same entries with and without an evaluation in front of it
    plans = []
    for with_eval in (False, True):
        with DryRun() as rec:
            trainer, batch = _c1()
            ops.set_seed(12345)
            trainer.step(batch, sync=False)
            if with_eval:
                trainer.evaluate([batch, batch])
            n0 = len(rec.calls)
            trainer.step(batch, sync=False)
            plans.append([n for n, _ in rec.calls[n0:]])
    assert plans[0] == plans[1] and "gtos_copy_nll_fwd" in plans[0] and "gtos_copy_eval_fwd" not in plans[0]


def test_eval_metrics_from_totals():
    import math
    from gtos_amd.train import eval_metrics
    m = eval_metrics([30.0, 12.0, 9.0, 4.0, 10.0])
    assert m == {"nll_per_token": 2.5, "perplexity": math.exp(2.5), "accuracy": 0.75, "tokens": 12, "sentences": 4, "loss": 2.5}
    z = eval_metrics([0.0] * 5)
    assert z["tokens"] == 0 and math.isnan(z["loss"]) and math.isnan(z["perplexity"])


# ------------------------------------------------------------------------------------------------ two gloo ranks, dry run
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _eval_worker(rank, world, port, q):
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import torch.distributed as dist
    from dryrun import DryRun
    import gtos_amd.train as train_mod
    from gtos_amd import synth
    from gtos_amd.config import build_generator
    from gtos_amd.generator import Generator
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    log = []
    real_ar = dist.all_reduce

    def logged_all_reduce(t, op=dist.ReduceOp.SUM, async_op=False, **kw):
        log.append(("all_reduce", t.numel(), str(t.dtype), "sum" if op == dist.ReduceOp.SUM else "other", bool(async_op), len(rec.calls)))
        return real_ar(t, op=op, async_op=async_op, **kw)
    dev = torch.device("cpu")
    with DryRun() as rec:
        torch.manual_seed(19940117)
        model = build_generator(Generator, "C1", dev, factored_relation=True).to(dev)
        model.set_compute_dtype(torch.bfloat16)
        model.train()
        trainer = train_mod.Trainer(model, synth.CONFIGS["C1"]["d"], warmup_steps=1, compute_dtype=torch.bfloat16, world_size=world, rank=rank)
        train_mod.dist.all_reduce = logged_all_reduce            # (after construction: the parameter broadcast is not the subject)
        batches = [synth.make_config_batch("C1", rank=rank, B=2 + rank)[0] for _ in range(2 + rank)]      # shards of different sizes
        # no kernel runs under the dry run, so the totals are filled by hand: rank r has scored (sum nll, tokens, correct, sentences, norm)
        totals = torch.tensor([[30.0, 12.0, 9.0, 4.0, 10.0], [10.0, 8.0, 3.0, 2.0, 3.0]][rank], dtype=torch.float64)
        res = trainer.evaluate(batches, totals=totals)
        q.put((rank, log, len(rec.calls), res, rec.histogram().get("gtos_eval_accumulate", 0)))
    dist.destroy_process_group()


def test_evaluate_two_ranks_one_collective_under_dry_run():
    import math
    import torch.multiprocessing as mp
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_eval_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted((q.get(timeout=600) for _ in range(world)), key=lambda r: r[0])
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    want = {"nll_per_token": 2.0, "perplexity": math.exp(2.0), "accuracy": 0.6, "tokens": 20, "sentences": 6, "loss": 13.0 / 6.0}
    for rank, log, n_calls, out, n_acc in res:
        assert len(log) == 1, log                                   # exactly ONE collective ...
        _, numel, dtype, op, async_op, at = log[0]
        assert (numel, dtype, op, async_op) == (5, "torch.float64", "sum", False)
        assert at == n_calls and n_acc == 2 + rank                  # ... after the last batch's last launch
        assert out == want, (rank, out)


# ------------------------------------------------------------------------------------------------ GPU: the kernels
def dev():
    assert torch.cuda.is_available(), "gpu-marked tests need the MI355X"
    return torch.device("cuda:0")


def _gpu_case(T, B, V, S, seed, dtype, plant=True):
    rng = np.random.default_rng(seed)
    x, div, a, cp, y, _ = make_case(rng, T, B, V, S, plant)
    d = dev()
    lg = torch.from_numpy(x).to(d).to(dtype).reshape(T, B, V)
    dv = torch.from_numpy(div).to(d).to(dtype).reshape(T, B, 2)
    al = torch.from_numpy(a).to(d).reshape(T, B, S)
    return lg, dv, al, torch.from_numpy(cp).to(d), torch.from_numpy(y).to(d).reshape(T, B)


GPU_SHAPES = [(3, 4, 7, 0), (12, 5, 1000, 37), (50, 64, 10000, 101), (8, 5, 9999, 23)]


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,B,V,S", GPU_SHAPES)
def test_copy_eval_vs_float64_statement_guarded(T, B, V, S, dtype):
    from gtos_amd import ops
    from tests_support import nan_buffer
    from test_label_smoothing import within
    lg, dv, al, cp, y = _gpu_case(T, B, V, S, 11 + V + S, dtype)
    R = T * B
    # the float64 statement on the SAME inputs (bf16-rounded where the kernel reads bf16)
    nll_ref, pred_ref, pp_ref, near, _ = reference_eval(lg.float().cpu().numpy().reshape(R, V), dv.float().cpu().numpy().reshape(R, 2),
                                                        al.cpu().numpy().reshape(R, S), cp.cpu().numpy(), y.cpu().numpy().reshape(R))
    assert near.mean() <= NEAR_SHARE, "%d of %d rows are near ties" % (int(near.sum()), R)
    f32 = nan_buffer(3 * R + 512, torch.float32, dev())
    nll = f32.carve(64, T, B, B)
    pred = f32.carve(192 + R, T, B, B).view(torch.int32)
    pp = f32.carve(320 + 2 * R, T, B, B)
    out = ops.copy_eval(lg, dv, al, cp, y, PAD, out=(nll, pred, pp))
    torch.cuda.synchronize()
    f32.check("nll / pred / p_pred")
    assert out[0].data_ptr() == nll.data_ptr()
    got_nll, got_pred, got_pp = nll.cpu().numpy().reshape(R), pred.cpu().numpy().reshape(R), pp.cpu().numpy().reshape(R)
    err = np.abs(got_nll - nll_ref)
    print("MEASURED copy_eval %s T*B=%d V=%d S=%d: nll max err %.3e (max |ref| %.3f), near ties %d" % (
        dtype, R, V, S, err.max(), np.abs(nll_ref).max(), int(near.sum())))
    within("nll", got_nll, nll_ref)
    assert (got_nll[y.cpu().numpy().reshape(R) == PAD] == 0).all()
    check_pred("pred", got_pred, pred_ref, near)
    ok = ~near
    assert np.allclose(got_pp[ok], pp_ref[ok], rtol=1e-4, atol=1e-12)
    # the plain call allocates its own outputs and gives the same bits
    nll2, pred2, pp2 = ops.copy_eval(lg, dv, al, cp, y, PAD)
    assert torch.equal(nll2, nll) and torch.equal(pred2, pred) and torch.equal(pp2, pp)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("T,B,V,S", GPU_SHAPES)
def test_copy_eval_nll_is_bitwise_copy_nll_and_pred_is_the_argmax_of_the_ll_row(T, B, V, S, dtype):
    from gtos_amd import ops
    lg, dv, al, cp, y = _gpu_case(T, B, V, S, 5 + V + S, dtype, plant=False)
    nll, pred, pp = ops.copy_eval(lg, dv, al, cp, y, PAD)
    plain = ops.copy_nll(lg, dv, al, cp, y, PAD, label_smoothing=0.0)
    assert torch.equal(nll.view(torch.int32), plain.view(torch.int32)), "nll is not bitwise gtos_copy_nll_fwd's"
    tot = max(V, 1 + int(cp.max())) if S else V
    ll = ops.copy_log_likelihood(lg, dv, al, cp, tot).reshape(T * B, tot)
    top2 = ll.topk(2, dim=1).values
    # rows whose top two ll values do not differ by more than 1e-5 may be skipped -- but not the EXACTLY equal ones (bf16 logits tie
    # in their top two on ~1 % of such rows): two equal logits give the same ll bits, and there the lower column must come out
    near = (((top2[:, 0] - top2[:, 1]) <= NEAR) & (top2[:, 0] != top2[:, 1])).cpu().numpy()
    assert near.mean() <= NEAR_SHARE, "%d of %d ll rows have their top two within %g" % (int(near.sum()), T * B, NEAR)
    # (torch.argmax does not promise the lowest column among equals: take it explicitly)
    cols = torch.arange(tot, device=ll.device).expand_as(ll)
    want = torch.where(ll == ll.max(1, keepdim=True).values, cols, tot).min(1).values
    check_pred("pred vs ll argmax", pred.reshape(-1).cpu().numpy(), want.cpu().numpy(), near)
    got_ll = torch.log(pp.reshape(-1) + 1e-12)
    assert torch.allclose(got_ll, ll.max(1).values, rtol=0, atol=1e-4)


@pytest.mark.gpu
def test_eval_accumulate_sums_counts_and_determinism():
    from gtos_amd import ops
    d = dev()
    runs = []
    for rep in range(2):
        totals = torch.zeros(5, dtype=torch.float64, device=d)
        want = np.zeros(5)
        per_call = []
        r2 = np.random.default_rng(17)
        for T, B in ((50, 64), (7, 300), (1, 1)):
            nll = (r2.random((T, B)) * 9).astype(np.float32)
            y = r2.integers(0, 40, (T, B)).astype(np.int64)
            y[r2.random((T, B)) < 0.3] = PAD
            if B > 2:
                y[:, 1] = PAD                                         # a column without a target: no sentence
            pred = np.where(r2.random((T, B)) < 0.5, y, y + 1).astype(np.int32)
            nll[y == PAD] = 0.0
            sn, st, sc = ops.eval_accumulate(torch.from_numpy(nll).to(d), torch.from_numpy(pred).to(d), torch.from_numpy(y).to(d),
                                             PAD, totals)
            live = y != PAD
            ref_n = (nll.astype(np.float64) * live).sum(0)
            ref_t = live.sum(0)
            ref_c = ((pred == y) & live).sum(0)
            assert np.allclose(sn.cpu().numpy(), ref_n, rtol=1e-12, atol=0)
            assert np.array_equal(st.cpu().numpy(), ref_t) and np.array_equal(sc.cpu().numpy(), ref_c)
            has = ref_t > 0
            want += [ref_n.sum(), ref_t.sum(), ref_c.sum(), has.sum(), (ref_n[has] / ref_t[has]).sum()]
            per_call.append((sn.clone(), st.clone(), sc.clone()))
        got = totals.cpu().numpy()
        assert np.allclose(got, want, rtol=1e-12, atol=0), (got, want)
        assert got[1] == want[1] and got[2] == want[2] and got[3] == want[3]
        runs.append((totals.clone(), per_call))
    assert torch.equal(runs[0][0].view(torch.int64), runs[1][0].view(torch.int64))
    for (a, b, c), (a2, b2, c2) in zip(runs[0][1], runs[1][1]):
        assert torch.equal(a.view(torch.int64), a2.view(torch.int64)) and torch.equal(b, b2) and torch.equal(c, c2)
