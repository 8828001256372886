"""Repeat-n-gram blocking (Generator.work(..., no_repeat_ngram=n), gtos_amd.search, csrc/ngram.hip, csrc/ngram_kernels.h).

CPU: the rule header compiled with g++ against a brute-force statement of the rule, the argument checks, and the launch plans of both
device decoders under the dry run.  GPU: gtos_ngram_block against a numpy statement (exact), its stores inside guard bands, and
work() with all three searches on the two golden models against a blocked restatement of the search around the oracle's next-token
log-likelihoods."""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver, Guarded

NEG_INF = float("-inf")
NS = [1, 2, 3, 4, 8]

DRIVER = r"""
#include "ngram_kernels.h"
using namespace gtos_ngram;
extern "C" int banned_row(const int* y, int t, int n, int* out) { return banned_serial(y, t, n, out); }
extern "C" int ban_pos(const int* y, int t, int n, int i) { return ban_at(y, t, n, i); }
extern "C" int max_t() { return MAX_T; }
"""


def brute_banned(y, n):
    """The rule, stated without positions: w is banned iff the n-gram (the last n - 1 tokens of y) + [w] occurs in y."""
    y = list(y)
    t = len(y)
    if t < n - 1:
        return set()
    suffix = y[t - n + 1:] if n > 1 else []
    return {w for w in set(y) if any(y[i:i + n] == suffix + [w] for i in range(t - n + 1))}


def has_repeat(y, n):
    grams = [tuple(y[i:i + n]) for i in range(len(y) - n + 1)]
    return len(grams) != len(set(grams))


# ------------------------------------------------------------------------------------------------ CPU: the header
@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = compile_host_driver(tmp_path_factory, "ngram_host", DRIVER)
    lib.banned_row.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    lib.ban_pos.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int]
    return lib


def test_rule_header_matches_brute_force(host_lib):
    from gtos_amd import ops
    from gtos_amd.search import banned_tokens
    assert host_lib.max_t() == ops.NGRAM_MAX_T >= 1024
    rng = np.random.RandomState(20261017)
    rows = 0
    out = np.zeros(80, dtype=np.int32)

    def check(y, n):
        y = np.ascontiguousarray(y, dtype=np.int32)
        t = len(y)
        m = host_lib.banned_row(y.ctypes.data, t, n, out.ctypes.data)
        want = brute_banned(y.tolist(), n)
        assert 0 <= m <= t and set(out[:m].tolist()) == want, (y.tolist(), n)
        per_pos = [host_lib.ban_pos(y.ctypes.data, t, n, i) for i in range(-1, t + 2)]
        assert [w for w in per_pos if w >= 0] == out[:m].tolist(), (y.tolist(), n)
        assert banned_tokens(y.tolist(), n) == out[:m].tolist()           # the host search's list form
    for rep in range(5):
        for alphabet in (2, 3, 50):
            for t in range(0, 71):
                for n in NS:
                    check(rng.randint(0, alphabet, size=t), n)
                    rows += 1
    for t in range(0, 71):
        for n in NS:
            check(np.full(t, 7), n)                                        # all equal
            check(rng.permutation(100)[:t], n)                             # all distinct
            rows += 2
    assert rows >= 5000, rows
    # what the rule promises: a history without a repeated n-gram stays so exactly under the tokens that are not banned
    for _ in range(300):
        n = int(rng.choice([1, 2, 3]))
        y = []
        for _step in range(12):
            free = [w for w in range(4) if w not in brute_banned(y, n)]
            if not free:
                break
            y.append(int(rng.choice(free)))
            assert not has_repeat(y, n)
        for w in brute_banned(y, n):
            assert has_repeat(y + [w], n)


# ------------------------------------------------------------------------------------------------ CPU: argument checks
def test_work_checks_no_repeat_ngram():
    """No model needed: the check runs before anything is touched."""
    from gtos_amd.generator import Generator
    from gtos_amd import ops
    for search in ("host", "device", "sample"):
        for bad in (-1, 1.5, True, "3"):
            with pytest.raises(ValueError):
                Generator.work(None, {}, 4, 10, search=search, no_repeat_ngram=bad)
    for search in ("device", "sample"):
        with pytest.raises(ValueError):
            Generator.work(None, {}, 4, 10, search=search, no_repeat_ngram=ops.NGRAM_MAX_T + 1)
        with pytest.raises(ValueError):
            Generator.work(None, {}, 4, ops.NGRAM_MAX_T + 1, search=search, no_repeat_ngram=2)


def test_ngram_entry_point_refuses_bad_arguments():
    """-10 outside the shapes, -23 for null pointers; nothing launched, no device needed."""
    from gtos_amd import _lib, ops
    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def call(N=8, k=4, t=2, max_t=5, n=3, tot=12, ld=12, ll=p, parent=p, token=p, prev=p, cur=p, active=p):
        return lib.gtos_ngram_block(N, k, t, max_t, n, tot, ll, ld, parent, token, prev, cur, active, None)
    assert call(n=0) == -10
    assert call(t=0) == -10
    assert call(t=5) == -10
    assert call(tot=0) == -10
    assert call(ld=11) == -10
    assert call(N=9) == -10
    assert call(t=1, max_t=ops.NGRAM_MAX_T + 1) == -10
    for name in ("ll", "token", "prev", "cur", "active"):
        assert call(**{name: None}) == -23, name
    assert call(N=0, n=0) == 0


def test_ops_ngram_block_passes_the_signature_check():
    from dryrun import DryRun
    from gtos_amd import ops
    with DryRun() as rec:
        N, max_t, tot = 6, 9, 20
        ll = torch.zeros(N, tot)
        hist = [torch.zeros(N, max_t, dtype=torch.int32) for _ in range(2)]
        tok = torch.zeros(max_t, N, dtype=torch.int32)
        active = torch.zeros(3, dtype=torch.int32)
        ops.ngram_block(4, 3, 2, ll, None, tok[3], hist[1], hist[0], active)
        ops.ngram_block(5, 3, 2, ll, tok[4], tok[4], hist[0], hist[1], active)
        with pytest.raises(AssertionError):
            ops.ngram_block(5, 3, 2, ll, None, tok[4], hist[0], hist[0], active)
    assert rec.names() == ["gtos_ngram_block"] * 2
    assert rec.calls[0][1][:6] == (N, 3, 4, max_t, 2, tot) and rec.calls[0][1][8] is None


# ------------------------------------------------------------------------------------------------ CPU: launch plans
def test_launch_plans_differ_by_one_ngram_block_per_step():
    from dryrun import DryRun
    from gtos_amd import synth
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    steps = 5
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

        def plan(**kw):
            n0 = len(rec.calls)
            beams = model.work(batch, 4, steps, **kw)
            assert len(beams) == batch['concept'].shape[1]
            return rec.calls[n0:]
        for kw, select in ((dict(search="device"), "gtos_beam_topk"), (dict(search="sample", seed=3), "gtos_sample_step")):
            base = [c[0] for c in plan(**kw)]
            assert base.count(select) == steps and "gtos_ngram_block" not in base
            assert [c[0] for c in plan(no_repeat_ngram=0, **kw)] == base
            calls = plan(no_repeat_ngram=3, **kw)
            names = [c[0] for c in calls]
            assert [x for x in names if x != "gtos_ngram_block"] == base
            at = [i for i, x in enumerate(names) if x == "gtos_ngram_block"]
            assert len(at) == steps - 1 and all(names[i + 1] == select for i in at)
            N = 4 * batch['concept'].shape[1]
            assert [calls[i][1][:5] for i in at] == [(N, 4, t, steps, 3) for t in range(1, steps)]


# ------------------------------------------------------------------------------------------------ GPU: the kernel
POISON = -7


def _expect(ll, hist_prev, hist_cur, parent, token, t, n, act):
    """The numpy statement of one gtos_ngram_block launch: (ll, hist_cur) after it."""
    ll, hist_cur = ll.copy(), hist_cur.copy()
    if not act:
        return ll, hist_cur
    for s in range(ll.shape[0]):
        p = s if parent is None else int(parent[s])
        if p < 0 or token[s] < 0:
            continue
        y = hist_prev[p, :t - 1].tolist() + [int(token[s])]
        hist_cur[s, :t] = y
        for w in brute_banned(y, n):
            ll[s, w] = -np.inf
    return ll, hist_cur


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("k", [1, 3, 32])
def test_ngram_block_matches_numpy_rule(k, n):
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(1000 * k + n)
    B, max_t = 3, 260
    N = B * k
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    launches = bans = 0
    for t in sorted({t for t in (1, n - 2, n - 1, n, 63, 64, 65, 257) if 1 <= t < max_t}):
        for tot in (40, 1000):
            alphabet = np.array([0, 7, tot - 1], dtype=np.int32)        # few ids: matches are frequent; the last column is one
            for ld in (tot, tot + 3):
                for variant in ("beam", "sample", "inactive"):
                    hist_prev = alphabet[rng.randint(0, 3, size=(N, max_t))]
                    hist_prev[N - 1] = 7                                   # an all-equal row
                    hist_cur = np.full((N, max_t), POISON, dtype=np.int32)
                    token = alphabet[rng.randint(0, 3, size=N)]
                    token[N - 1] = 7
                    parent = (np.arange(N) // k) * k + rng.randint(0, k, size=N)      # any slot of the same graph
                    if k >= 3:
                        parent[1] = parent[0]                              # two children of one parent
                        parent[2::4] = -1                                  # dead slots, interleaved
                        token[4::5] = -1
                    else:
                        parent[1] = -1
                        if variant == "beam":
                            token[0] = -1
                    parent = parent.astype(np.int32)
                    buf = rng.randn(N * ld).astype(np.float32)
                    buf.reshape(N, ld)[:, tot:] = np.nan                   # the stride gap is no column
                    ll = buf.reshape(N, ld)[:, :tot]
                    active = np.zeros(3, dtype=np.int32)
                    active[t % 3] = variant != "inactive"
                    if variant == "sample":                                # parent = NULL, the token row cut from a [max_t, N] table
                        table = rng.randint(0, 3, size=(max_t, N)).astype(np.int32)
                        table[t - 1] = token
                        g_par, g_tok, parent = None, D(table)[t - 1], None
                    else:
                        g_par, g_tok = D(parent), D(token)
                    g_buf, g_prev, g_cur, g_act = D(buf), D(hist_prev), D(hist_cur), D(active)
                    ops.ngram_block(t, k, n, g_buf.view(N, ld)[:, :tot], g_par, g_tok, g_prev, g_cur, g_act)
                    want_ll, want_cur = _expect(ll, hist_prev, hist_cur, parent, token, t, n, variant != "inactive")
                    want_buf = buf.copy()
                    want_buf.reshape(N, ld)[:, :tot] = want_ll
                    what = (t, tot, ld, variant)
                    assert np.array_equal(g_buf.cpu().numpy().view(np.int32), want_buf.view(np.int32)), what      # bit for bit
                    assert np.array_equal(g_cur.cpu().numpy(), want_cur), what
                    assert np.array_equal(g_prev.cpu().numpy(), hist_prev) and np.array_equal(g_act.cpu().numpy(), active), what
                    launches += 1
                    bans += int(np.isneginf(want_ll).sum())
    assert launches >= 12 * 5 and bans > 0, (launches, bans)


@pytest.mark.gpu
@pytest.mark.parametrize("k,n,t", [(3, 1, 1), (3, 2, 65), (32, 3, 257), (1, 8, 64)])
def test_ngram_block_stores_inside_its_outputs(k, n, t):
    """ll and both history buffers carved from poisoned allocations: nothing outside ll's columns and hist_cur[live, :t] changes."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(77 + t)
    B, max_t, tot = 3, 258, 40
    N = B * k
    alphabet = np.array([0, 7, tot - 1], dtype=np.int32)
    ll0 = torch.from_numpy(rng.randn(N, tot).astype(np.float32))
    g_ll = Guarded(N, tot, torch.float32, dev, ld=tot + 3, init=ll0.to(dev))
    margin = 4 * max_t
    hist = []
    for fill in (alphabet[rng.randint(0, 3, size=(N, max_t))], np.full((N, max_t), POISON, dtype=np.int32)):
        whole = torch.full((2 * margin + N * max_t,), POISON - 1, dtype=torch.int32, device=dev)
        view = whole[margin:margin + N * max_t].view(N, max_t)
        view.copy_(torch.from_numpy(fill))
        hist.append((whole, view, fill))
    parent = ((np.arange(N) // k) * k + rng.randint(0, k, size=N)).astype(np.int32)
    token = alphabet[rng.randint(0, 3, size=N)]
    parent[1::3] = -1
    token[2::7] = -1
    active = np.zeros(3, dtype=np.int32)
    active[t % 3] = 1
    D = lambda a: torch.from_numpy(a).to(dev)
    ops.ngram_block(t, k, n, g_ll.view, D(parent), D(token), hist[0][1], hist[1][1], D(active))
    g_ll.check("gtos_ngram_block ll")
    want_ll, want_cur = _expect(ll0.numpy(), hist[0][2], hist[1][2], parent, token, t, n, True)
    assert np.array_equal(g_ll.view.contiguous().cpu().numpy().view(np.int32), np.ascontiguousarray(want_ll).view(np.int32))
    for whole, view, fill in hist:
        w = whole.cpu().numpy()
        assert (w[:margin] == POISON - 1).all() and (w[margin + N * max_t:] == POISON - 1).all()
    assert np.array_equal(hist[0][1].cpu().numpy(), hist[0][2])
    cur = hist[1][1].cpu().numpy()
    assert np.array_equal(cur, want_cur)
    dead = (parent < 0) | (token < 0)
    assert dead.any() and (~dead).any() and (cur[dead] == POISON).all() and (cur[:, t:] == POISON).all()


# ------------------------------------------------------------------------------------------------ GPU: end to end
NEAR = 5e-5              # a selection gap of the restatement below this leaves its sentence out of the exact comparison
_restated = {}
_left_out = set()


def _gap(a, b):
    d = a - b
    return d if math.isfinite(d) else float("inf")


def restate_sentence(O, model, graph, gmask, probe, cp_seq, local, vocabs, k, max_t, min_t, n, alpha):
    """The reference's search (oracle.beam_search_sentence: torch.topk, the pool rule) with the ban in front of the top-k ->
    (finished, alive, k-best, steps, the smallest selection gap)."""
    pv = vocabs['predictable_token']
    inv = {w: i for i, w in local.items()}
    alive, fin, steps, gap = [(['<STR>'], 0.0)], [], 0, float("inf")
    while len(fin) < k and steps < max_t and alive:
        ll = O.next_token_ll(model, graph, gmask, probe, cp_seq, [s for s, _ in alive], vocabs).clone()
        for h, (seq, _) in enumerate(alive):
            for w in brute_banned(seq[1:], n) if n else ():
                ll[h, inv[w] if w in inv else pv.token2idx(w)] = NEG_INF
        top_s, top_i = torch.topk(ll, min(k + 1, ll.shape[1]), 1)
        pool = []
        for h, (seq, score) in enumerate(alive):
            row = top_s[h].tolist()
            if len(row) > k:
                gap = min(gap, _gap(row[k - 1], row[k]))
            for s, i in zip(row[:k], top_i[h].tolist()[:k]):
                word = local[i] if i in local else pv.idx2token(i)
                pool.append((seq + [word], NEG_INF if word == '<UNK>' else score + s))
        pool = sorted(pool, key=lambda c: -c[1])
        cut = k - len(fin)
        if 0 < cut < len(pool):
            gap = min(gap, _gap(pool[cut - 1][1], pool[cut][1]))
        alive = []
        for seq, score in pool[:cut]:
            if seq[-1] == '<END>':
                if len(seq) - 2 >= min_t:
                    fin.append((seq, score))
            else:
                alive.append((seq, score))
        steps += 1
    best = O.k_best(fin, alive, k, alpha)
    norm = [s / ((1 + len(q)) ** alpha) for q, s in sorted(fin if fin else alive, key=lambda c: -(c[1] / ((1 + len(c[0])) ** alpha)))]
    for a, b in zip(norm, norm[1:]):
        gap = min(gap, _gap(a, b))
    return fin, alive, best, steps, gap


def restated(case, tmp_path):
    """The restatement of every (run, n, sentence) of a golden case, computed once on the CPU and shared."""
    if case in _restated:
        return _restated[case]
    from oracle import gtos_oracle as O
    from test_beam_and_vocab import load_case, make_vocabs, batch_of, state_dict_of
    meta, arrs = load_case(case)
    vocabs = make_vocabs(meta, tmp_path)
    cfg = meta["cfg"]
    ga = [[tuple(f) for f in a] if isinstance(a, list) else a for a in cfg["gen_args"]]
    ref = O.Generator(vocabs, *ga, cfg["d"], cfg["ff"], cfg["H"], 0.0, cfg["snt_layers"], cfg["graph_layers"],
                      cfg["inference_layers"], depth_size=cfg.get("depth_size", 32))
    ref.load_state_dict(state_dict_of(arrs))
    ref.eval()
    batch = batch_of(meta, arrs)
    out = {}
    with torch.no_grad():
        graph, gmask, probe = ref.encode_step(batch, train=False)
        for r, run in enumerate(meta["runs"]):
            for n in (1, 2, 3):
                out[r, n] = [restate_sentence(O, ref, graph[:, b:b + 1], gmask[:, b:b + 1], probe[:, b:b + 1], batch['cp_seq'][:, b:b + 1],
                                              batch['local_idx2token'][b], vocabs, run["beam"], run["max_step"], run["min_step"], n,
                                              cfg["alpha"]) for b in range(graph.shape[1])]
    _restated[case] = out
    return out


def _golden_model(case, tmp_path):
    from test_beam_and_vocab import load_case, make_vocabs, batch_of, state_dict_of
    from gtos_amd.generator import Generator
    meta, arrs = load_case(case)
    dev = torch.device("cuda:0")
    vocabs = make_vocabs(meta, tmp_path)
    cfg = meta["cfg"]
    ga = [[tuple(f) for f in a] if isinstance(a, list) else a for a in cfg["gen_args"]]
    model = Generator(vocabs, *ga, cfg["d"], cfg["ff"], cfg["H"], 0.0, cfg["snt_layers"], cfg["graph_layers"],
                      cfg["inference_layers"], None, dev, depth_size=cfg.get("depth_size", 32)).to(dev)
    model.load_state_dict(state_dict_of(arrs))
    model.eval()
    return meta, model, batch_of(meta, arrs, dev)


def _pairs(hyps):
    return [(h.seq, h.score) for h in hyps]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["beam_smatch", "beam_dep_dev"])
def test_blocked_search_matches_the_restatement(case, tmp_path):
    """work(search="device") and work(search="host") with n in {1, 2, 3} against the blocked restatement, at the fixture's own runs.
    A sentence is left out of the exact comparison only when one of the restatement's own selection gaps is below 5e-5; over both
    cases at most 9 of the 90 (case, run, n, sentence) combinations and at most 6 sentences may be."""
    from test_beam_and_vocab import check_hyps
    meta, model, batch = _golden_model(case, tmp_path)
    want_all = restated(case, tmp_path)
    alpha = meta["cfg"]["alpha"]
    compared = 0
    for r, run in enumerate(meta["runs"]):
        k, max_t, min_t = run["beam"], run["max_step"], run["min_step"]
        plain = model.work(batch, k, max_t, min_t, search="device")
        zero = model.work(batch, k, max_t, min_t, search="device", no_repeat_ngram=0)
        for a, b in zip(plain, zero):
            assert (a.steps, _pairs(a.hypotheses), _pairs(a.completed_hypotheses)) == (b.steps, _pairs(b.hypotheses), _pairs(b.completed_hypotheses))
        for n in (1, 2, 3):
            for search in ("device", "host"):
                beams = model.work(batch, k, max_t, min_t, search=search, no_repeat_ngram=n)
                for b, (beam, (fin, alive, best, steps, gap)) in enumerate(zip(beams, want_all[r, n])):
                    tag = "%s run %s n %d sentence %d (%s)" % (case, (k, max_t, min_t), n, b, search)
                    got_best = _pairs(beam.get_k_best(k, alpha))      # (with nothing finished this moves the alive list, as the reference does)
                    for seq, _ in _pairs(beam.completed_hypotheses) + _pairs(beam.hypotheses):
                        assert not has_repeat([w for w in seq[1:] if w != '<END>'], n), (tag, seq)
                    if n == 1:
                        assert [list(s) for s, _ in got_best] != [list(s) for s, _ in run["expect"][b]["k_best"]], tag
                    print("MEASURED %s: smallest selection gap of the restatement %.3e" % (tag, gap))
                    if gap < NEAR:
                        _left_out.add((case, r, n, b))
                        continue
                    compared += 1
                    assert beam.steps == steps, tag
                    if fin:
                        check_hyps(_pairs(beam.completed_hypotheses), fin, tag + " finished")
                        check_hyps(_pairs(beam.hypotheses), alive, tag + " alive")
                    else:
                        check_hyps(got_best, sorted(alive, key=lambda c: -(c[1] / ((1 + len(c[0])) ** alpha))), tag + " alive")
                    check_hyps(got_best, best, tag + " k-best")
    assert len(_left_out) <= 9 and len({(c, r, b) for c, r, n, b in _left_out}) <= 6, sorted(_left_out)
    assert compared >= 2 * 3 * 6 * len(meta["runs"]) - 2 * 9


@pytest.mark.gpu
def test_blocked_device_search_is_independent_of_sync_every(tmp_path, monkeypatch):
    from gtos_amd import search
    from test_sample_decode import _capture_memory
    meta, model, batch = _golden_model("beam_smatch", tmp_path)
    run = meta["runs"][0]
    memory = _capture_memory(model, batch, monkeypatch)
    out = []
    for sync in (1, 8):
        beams = [search.Beam(run["beam"], run["min_step"], run["max_step"]) for _ in memory['local_idx2token']]
        with torch.no_grad():
            search.beam_search_device(model, memory, beams, sync_every=sync, no_repeat_ngram=3)
        out.append([(b.steps, _pairs(b.hypotheses), _pairs(b.completed_hypotheses)) for b in beams])
    assert out[0] == out[1]


@pytest.mark.gpu
def test_blocked_sampling_end_to_end_fp32():
    """n = 1 on a C1-sized fp32 batch: no sample holds a token twice, one seed gives one result, every recorded score is the
    model's teacher-forced log-likelihood of the sample (the bar of test_sample_decode.py), and n = 0 is the call without the keyword."""
    from test_device_beam_search import _synth_model
    model, batch = _synth_model("C1", torch.float32)
    k, max_t = 4, 12
    key = lambda beams: [(b.steps, _pairs(b.completed_hypotheses), _pairs(b.hypotheses)) for b in beams]
    for kw in (dict(), dict(top_k=2)):                   # the whole row, and a top-k narrow enough that unblocked samples repeat tokens
        _check_blocked_samples(model, batch, k, max_t, key, kw)


def _check_blocked_samples(model, batch, k, max_t, key, kw):
    a = model.work(batch, k, max_t, search="sample", seed=5, no_repeat_ngram=1, **kw)
    assert key(a) == key(model.work(batch, k, max_t, search="sample", seed=5, no_repeat_ngram=1, **kw))
    plain = model.work(batch, k, max_t, search="sample", seed=5, **kw)
    assert key(plain) == key(model.work(batch, k, max_t, search="sample", seed=5, no_repeat_ngram=0, **kw))
    print("MEASURED %r: %d of %d unblocked samples hold a token twice" % (
        kw, sum(has_repeat(h.seq[1:], 1) for b in plain for h in b.completed_hypotheses + b.hypotheses), k * len(plain)))
    targets, scores = [], []
    for beam in a:
        hyps = beam.completed_hypotheses + beam.hypotheses
        assert len(hyps) == k
        for h in hyps:
            assert not has_repeat(h.seq[1:], 1), h.seq
        targets.append([[w for w in h.seq[1:] if w != '<END>'] for h in hyps])
        scores += [(h.score, len(h.seq) - 1) for h in hyps]
    token_ll = model.score(batch, targets).token_ll.double().cpu()
    assert token_ll.shape[1] == len(scores)
    for j, (score, length) in enumerate(scores):
        want = float(token_ll[:length, j].sum())
        assert abs(want - score) <= 1e-4 * max(1.0, abs(score)), (j, want, score)
