"""Device-resident sampling decode (Generator.work(..., search="sample"), gtos_amd.search.sample_device, csrc/sample.hip,
csrc/sample_kernels.h).

CPU: the selection header compiled with g++ against a numpy statement of the rule on random rows, the counter hash against its
Python restatement, and Generator.work's argument checks.  GPU: gtos_sample_step against the same numpy statement (winner, score,
state words, token table, next input), the sampled distribution against softmax(ll / T) on the kept set, and end to end on C1 (fp32)
and C2 (bf16) models: greedy equality with a host loop, seeds, sync_every, vocabulary invariants and teacher-forced scores."""
import ctypes

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver


DRIVER = r"""
#include "sample_kernels.h"
using namespace gtos_sample;
extern "C" int select_row(const float* ll, int tot, int V, int b, int j, int t, int min_t, const uint8_t* fs, const uint8_t* fl,
                          const uint8_t* owned, double T, int top_k, double top_p, uint64_t seed) {
    float kv[MAX_TOPK];
    int kc[MAX_TOPK];
    return select_serial(ll, tot, V, b, j, t, min_t, fs, fl, owned, T, top_k, top_p, seed, kv, kc);
}
extern "C" void row_bits(uint64_t seed, int g, int j, int t, int n, uint64_t* out) {
    const uint64_t key = row_key(seed, g, j, t);
    for (int c = 0; c < n; ++c) out[c] = draw(key, (uint64_t)c);
}
"""

PLAIN, UNK_, END_ = 0, 1, 2
NEAR = 1e-9
GRID = [(T, k, p) for T in (0.3, 1.0, 2.5) for k in (0, 1, 5, 32) for p in (0.3, 0.9, 1.0)]


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    so = compile_host_driver(tmp_path_factory, "sample_host", DRIVER)
    so.select_row.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                              ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_int, ctypes.c_double,
                              ctypes.c_uint64]
    so.select_row.restype = ctypes.c_int
    so.row_bits.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    so.row_bits.restype = None
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def f32(x):
    """The kernel takes temperature and top_p as fp32."""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ the rule, stated in numpy
def allowed_mask(ll, V, fs, fl_b, owned_b, t, min_t):
    """Rule 1 for one row of graph b: fl_b / owned_b are that graph's [tot - V] copy tables."""
    tot = ll.shape[0]
    cls = np.concatenate([fs[:V], fl_b[:tot - V]]).astype(np.int64)
    own = np.concatenate([np.ones(V, bool), owned_b[:tot - V].astype(bool)])
    return np.isfinite(ll) & own & ((cls == PLAIN) | ((cls == END_) & (t >= min_t)))


def uniforms(seed, g, j, t, cols):
    from gtos_amd.search import sample_bits
    m = (sample_bits(seed, g, j, t, cols) >> np.uint64(11)).astype(np.float64)
    u = (m + 0.5) * 2.0 ** -53
    return np.where(u < 1.0, u, 1.0 - 2.0 ** -53)


def np_kept(ll, allow, T, top_k, top_p):
    """Rules 2 and 3: the kept columns (ll descending, column ascending) and whether the top-p cut is a near tie."""
    cols = np.nonzero(allow)[0]
    v = ll[cols]
    order = np.lexsort((cols, -v.astype(np.float64)))
    cols, v = cols[order], v[order]
    if top_k:
        cols, v = cols[:top_k], v[:top_k]
    near = False
    if top_p < 1.0 and cols.size > 1:
        w = np.exp((v.astype(np.float64) - float(v[0])) / T)
        Z, cum = w.sum(), np.cumsum(w)
        ends = np.nonzero(np.r_[v[1:] < v[:-1], True])[0]          # last index of each run of equal values
        mass = cum[ends]
        near = bool((np.abs(mass - top_p * Z) <= NEAR * top_p * Z).any())
        n = ends[np.argmax(mass >= top_p * Z)] + 1
        cols, v = cols[:n], v[:n]
    return cols, v, near


def np_select(ll, allow, T, top_k, top_p, seed, g, j, t):
    """Rules 2-4 -> (winner or -1, near tie)."""
    cols, v, near = np_kept(ll, allow, T, top_k, top_p)
    if not cols.size:
        return -1, False
    keys = v.astype(np.float64) / T - np.log(-np.log(uniforms(seed, g, j, t, cols)))
    order = np.lexsort((cols, -keys))
    if cols.size > 1:
        a, b = keys[order[0]], keys[order[1]]
        near |= abs(a - b) <= NEAR * max(abs(a), abs(b))
    return int(cols[order[0]]), near


def random_tables(rng, B, V, tot, p_unk=0.04, p_end=0.04):
    """Token classes of the shared ids and of every graph's copy ids, and which copy ids each graph owns."""
    classes = lambda n: rng.choice([PLAIN, UNK_, END_], size=n, p=[1 - p_unk - p_end, p_unk, p_end]).astype(np.uint8)
    fs = classes(V)
    fs[:3] = [PLAIN, UNK_, END_][:min(V, 3)]
    fl = classes(B * (tot - V)).reshape(B, tot - V)
    owned = (rng.rand(B, tot - V) < 0.5).astype(np.uint8)
    return fs, fl, owned


def random_row(rng, tot):
    """Log-likelihood-like values with every hazard: coarse grids (ties), -inf entries, one dominant column sometimes."""
    kind = rng.randint(4)
    if kind == 0:
        x = rng.randn(tot) * 2.0 - 8.0
    elif kind == 1:
        x = np.round(rng.randn(tot) * 2.0) / 4.0 - 5.0                 # many ties
    elif kind == 2:
        x = rng.randn(tot) * 0.01 - 9.0                                 # near uniform
    else:
        x = rng.randn(tot) * 3.0 - 12.0
        x[rng.randint(tot)] = -0.05                                     # one likely column
    x[rng.rand(tot) < 0.05] = -np.inf
    return x.astype(np.float32)


# ------------------------------------------------------------------------------------------------ CPU
def test_selection_header_matches_numpy_rule(host_lib):
    rng = np.random.RandomState(20261016)
    rows = near = empty = 0
    for T, top_k, top_p in GRID:
        Tf, pf = f32(T), f32(top_p)
        for _ in range(300):
            tot = int(rng.choice([3, 8, 40, 117, 300]))
            V = int(rng.randint(1, tot + 1))
            B = int(rng.randint(1, 4))
            fs, fl, owned = random_tables(rng, B, V, tot, p_unk=float(rng.choice([0.04, 0.6])))
            ll = random_row(rng, tot)
            if rows % 97 == 0:
                ll[:] = -np.inf                                         # nothing allowed
            b, j, t, min_t = int(rng.randint(B)), int(rng.randint(8)), int(rng.randint(6)), int(rng.randint(5))
            seed = int(rng.randint(0, 2 ** 62)) * 4 + 3
            allow = allowed_mask(ll, V, fs, fl[b], owned[b], t, min_t)
            want, amb = np_select(ll, allow, Tf, top_k, pf, seed, b, j, t)
            got = host_lib.select_row(_p(ll), tot, V, b, j, t, min_t, _p(fs), _p(fl), _p(owned), Tf, top_k, pf, seed)
            rows += 1
            near += amb
            empty += want < 0
            assert got == want or amb, (T, top_k, top_p, tot, V, got, want)
            if got >= 0:
                assert allow[got]
    assert rows >= 10000 and near <= rows // 200, (rows, near)
    assert 0 < empty < rows // 20, empty


def test_counter_hash_restated_in_python(host_lib):
    from gtos_amd.search import sample_bits
    for seed, g, j, t in ((0, 0, 0, 0), (1, 2, 3, 4), (2 ** 64 - 1, 63, 7, 49), (0x1234567890ABCDEF, 1000, 31, 511)):
        out = np.zeros(300, dtype=np.uint64)
        host_lib.row_bits(seed, g, j, t, out.size, _p(out))
        assert np.array_equal(out, sample_bits(seed, g, j, t, np.arange(300))), (seed, g, j, t)
        assert np.array_equal(out[[5, 299, 0]], sample_bits(seed, g, j, t, [5, 299, 0]))


def test_work_checks_the_sampling_arguments():
    """No model needed: the checks run before anything is touched."""
    from gtos_amd.generator import Generator
    for kw in (dict(temperature=0.7), dict(top_k=5), dict(top_p=0.9), dict(seed=3)):
        for search in ("host", "device"):
            with pytest.raises(ValueError):
                Generator.work(None, {}, 4, 10, search=search, **kw)
    bad = [dict(temperature=0), dict(temperature=-1.0), dict(temperature=float("inf")), dict(temperature=float("nan")),
           dict(temperature=1e300), dict(top_k=-1), dict(top_k=33), dict(top_k=2.5), dict(top_p=0.0), dict(top_p=1.5),
           dict(top_p=float("nan")), dict(top_p=1e-50), dict(seed=1.5)]
    for kw in bad:
        with pytest.raises(ValueError):
            Generator.work(None, {}, 4, 10, search="sample", **kw)
    with pytest.raises(ValueError):
        Generator.work(None, {}, 0, 10, search="sample")


def test_sample_entry_point_refuses_bad_arguments():
    """-10 for settings outside the rule, nothing launched, no device needed."""
    from gtos_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def call(N=8, k=4, t=0, V=10, tot=12, max_t=5, T=1.0, top_k=0, top_p=1.0, ld=12, C=3):
        return lib.gtos_sample_step(N, k, t, V, tot, 0, max_t, T, top_k, top_p, 7, p, ld, *[p] * 11, C, 0, p, p, p, None)
    assert call(top_k=33) == -10
    assert call(top_k=-1) == -10
    assert call(T=0.0) == -10
    assert call(T=float("inf")) == -10
    assert call(T=float("nan")) == -10
    assert call(top_p=0.0) == -10
    assert call(top_p=1.01) == -10
    assert call(N=9) == -10
    assert call(t=5) == -10
    assert call(ld=11) == -10
    assert call(tot=9) == -10


# ------------------------------------------------------------------------------------------------ GPU: the kernel
def _run_step(t, k, V, tot, min_t, max_t, T, top_k, top_p, seed, ll, fs, fl, owned, score, state, tokens, active, inputs):
    """One ops.sample_step on numpy tables; returns the tables after it and the next inputs."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    tok_shared, tok_local, char_shared, char_local, dead_tok, dead_char = inputs
    N, C = state.shape[0], dead_char.shape[0]
    g = [D(x) for x in (score, state, tokens, active)]
    tok_out = torch.full((N,), -5, dtype=torch.int64, device=dev)
    char_out = torch.full((N, C), -5, dtype=torch.int64, device=dev)
    ops.sample_step(t, k, V, tot, min_t, max_t, T, top_k, top_p, seed, D(ll), D(fs), D(fl) if tot > V else None,
                    D(owned) if tot > V else None, *g, D(tok_shared), D(tok_local) if tot > V else None, D(char_shared),
                    D(char_local) if tot > V else None, dead_tok, D(dead_char), tok_out, char_out)
    return [x.cpu().numpy() for x in g] + [tok_out.cpu().numpy(), char_out.cpu().numpy()]


@pytest.mark.gpu
@pytest.mark.parametrize("tot", [32, 997, 20000, 65536])
def test_sample_step_matches_numpy_rule(tot):
    rng = np.random.RandomState(tot)
    B, k, max_t, C = 3, 6, 9, 5
    N = B * k
    V = tot - max(1, tot // 8)
    checked = near = 0
    for T, top_k, top_p in GRID:
        Tf, pf = f32(T), f32(top_p)
        fs, fl, owned = random_tables(rng, B, V, tot)
        ll = np.stack([random_row(rng, tot) for _ in range(N)])
        ll[0] = -np.inf                                                 # nothing allowed: the slot stops
        t, min_t = int(rng.randint(max_t)), int(rng.randint(4))
        seed = int(rng.randint(0, 2 ** 62)) * 3 + 1
        score = rng.randn(N)
        state = np.zeros((N, 3), dtype=np.int32)
        state[:, 0], state[:, 1] = t, -1
        dead = rng.rand(N) < 0.2
        state[dead, 2] = 1
        tokens = rng.randint(-1, tot, size=(max_t, N)).astype(np.int32)
        tokens[t] = -1
        active = np.zeros(3, dtype=np.int32)
        active[t % 3], active[(t + 2) % 3] = 1, 1
        inputs = (rng.randint(0, 1000, V), rng.randint(0, 1000, (B, tot - V)), rng.randint(0, 100, (V, C)),
                  rng.randint(0, 100, (B, tot - V, C)), 77, rng.randint(0, 100, C))
        got_score, got_state, got_tok, got_active, tok_out, char_out = _run_step(
            t, k, V, tot, min_t, max_t, Tf, top_k, pf, seed, ll, fs, fl, owned, score, state, tokens, active, inputs)
        tok_shared, tok_local, char_shared, char_local, dead_tok, dead_char = inputs
        want_active = False
        for s in range(N):
            b, j = divmod(s, k)
            if dead[s]:
                assert got_score[s] == score[s] and (got_state[s] == state[s]).all() and got_tok[t, s] == -1
                assert tok_out[s] == dead_tok and (char_out[s] == dead_char).all()
                continue
            allow = allowed_mask(ll[s], V, fs, fl[b], owned[b], t, min_t)
            w, amb = np_select(ll[s], allow, Tf, top_k, pf, seed, b, j, t)
            near += amb
            if amb:
                want_active |= bool(got_state[s, 2] == 0 and t + 1 < max_t)
                continue
            checked += 1
            tag = (T, top_k, top_p, s)
            assert got_tok[t, s] == w, tag
            cls = -1 if w < 0 else (fs[w] if w < V else fl[b, w - V])
            end = cls == END_
            assert got_state[s].tolist() == [t + 1, t if end else -1, int(w < 0 or end)], tag
            assert got_score[s] == (score[s] if w < 0 else score[s] + np.float64(ll[s, w])), tag
            on = w >= 0 and not end
            want_active |= on and t + 1 < max_t
            if on and t + 1 < max_t:
                assert tok_out[s] == (tok_shared[w] if w < V else tok_local[b, w - V]), tag
                assert (char_out[s] == (char_shared[w] if w < V else char_local[b, w - V])).all(), tag
            else:
                assert tok_out[s] == dead_tok and (char_out[s] == dead_char).all(), tag
        others = [r for r in range(max_t) if r != t]
        assert (got_tok[others] == tokens[others]).all()
        assert got_active[(t + 2) % 3] == 0 and got_active[t % 3] == 1
        assert bool(got_active[(t + 1) % 3]) == want_active
    assert checked > 300 and near <= checked // 50, (checked, near)
    # a step whose flag is clear changes nothing and hands every slot the padding input
    active = np.zeros(3, dtype=np.int32)
    score = rng.randn(N)
    state = np.zeros((N, 3), dtype=np.int32)
    tokens = np.full((max_t, N), -1, dtype=np.int32)
    out = _run_step(0, k, V, tot, 0, max_t, 1.0, 0, 1.0, 5, ll, fs, fl, owned, score, state, tokens, active, inputs)
    assert (out[0] == score).all() and (out[1] == state).all() and (out[2] == -1).all()
    assert (out[4] == inputs[4]).all() and (out[5] == inputs[5]).all()


@pytest.mark.gpu
@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 1.0), (0.7, 0, 0.9), (1.5, 20, 1.0), (2.5, 12, 0.8)])
def test_sample_step_draws_the_tempered_distribution(T, top_k, top_p):
    """One fixed 40-column row in 4096 slots over 50 steps (no <END>): 204,800 draws against softmax(ll / T) on the kept set."""
    from torch.special import gammaincc
    rng = np.random.RandomState(40)
    B, k, max_t, tot, C = 64, 64, 50, 40, 2
    N = B * k
    V = tot
    Tf, pf = f32(T), f32(top_p)
    row = (rng.randn(tot) * 1.2).astype(np.float32)
    row[7] = row[8]                                                     # a tie
    row = (row - np.log(np.exp(row.astype(np.float64)).sum())).astype(np.float32)
    fs = np.zeros(V, dtype=np.uint8)
    fs[1] = UNK_
    allow = allowed_mask(row, V, fs, np.zeros(0, np.uint8), np.zeros(0, np.uint8), 0, 0)
    kept, v, _ = np_kept(row, allow, Tf, top_k, pf)
    ll = np.broadcast_to(row, (N, tot)).copy()
    score = np.zeros(N)
    state = np.zeros((N, 3), dtype=np.int32)
    state[:, 1] = -1
    tokens = np.full((max_t, N), -1, dtype=np.int32)
    active = np.array([1, 0, 0], dtype=np.int32)
    inputs = (np.zeros(V, np.int64), np.zeros((B, 0), np.int64), np.zeros((V, C), np.int64), np.zeros((B, 0, C), np.int64), 0,
              np.zeros(C, np.int64))
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    g_ll, g_fs = D(ll), D(fs)
    g = [D(x) for x in (score, state, tokens, active)]
    tok_out = torch.empty(N, dtype=torch.int64, device=dev)
    char_out = torch.empty((N, C), dtype=torch.int64, device=dev)
    for t in range(max_t):
        ops.sample_step(t, k, V, tot, 0, max_t, Tf, top_k, pf, 123456789, g_ll, g_fs, None, None, *g, D(inputs[0]), None,
                        D(inputs[2]), None, 0, D(inputs[5]), tok_out, char_out)
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
    if df:
        pval = float(gammaincc(torch.tensor(df / 2.0, dtype=torch.float64), torch.tensor(chi2 / 2.0, dtype=torch.float64)))
        assert pval > 1e-6, (chi2, df, pval)
    score_h = g[0].cpu().numpy()
    assert np.allclose(score_h, np.asarray([row[tokens_col].astype(np.float64).sum()
                                            for tokens_col in g[2].cpu().numpy().T]), rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------------------------ GPU: end to end
def _capture_memory(model, batch, monkeypatch):
    """Generator.work's per-graph memory (encoder run once), by stopping work before its search."""
    import gtos_amd.generator as G
    box = {}
    monkeypatch.setattr(G, "sample_device", lambda m, memory, beams, *a, **kw: box.update(memory=memory) or beams)
    model.work(batch, 1, 1, search="sample", seed=0)
    monkeypatch.undo()
    return box["memory"]


def _fresh(B, k, max_t, min_t):
    from gtos_amd.search import Beam
    return [Beam(k, min_t, max_t) for _ in range(B)]


def _host_decode(model, memory, k, max_t, min_t, choose):
    """A host loop over Generator.decode_slots: every step pulls the ll rows to the host and asks choose(s, t, ll_row, allowed) for
    slot s's token id (None: the slot stops).  -> per slot the token ids and the fp64 sum of their ll."""
    from gtos_amd.search import slot_memory
    B = len(memory['local_idx2token'])
    N = B * k
    dev = memory['probe'].device
    mem = slot_memory(memory, B, k)
    local = memory['local_idx2token']
    V = model.vocabs['predictable_token'].size
    tot = max(int(memory['tot_ext']), V)
    tab = model.search_tables(local, tot)
    owned = model.sample_tables(local, tot)
    fs = tab['flag_shared'].cpu().numpy()
    fl = tab['flag_local'].cpu().numpy() if tot > V else np.zeros((B, 0), np.uint8)
    ow = owned.cpu().numpy() if tot > V else np.zeros((B, 0), np.uint8)
    caches = [c[0] for c in model.slot_caches(max_t, N, copies=1)]
    tok = torch.full((1, N), tab['start_tok'], dtype=torch.int64, device=dev)
    chars = tab['start_char'].expand(1, N, tab['C']).contiguous()
    seqs, scores, live = [[] for _ in range(N)], [0.0] * N, [True] * N
    for t in range(max_t):
        if not any(live):
            break
        ll = model.decode_slots((tok, chars), caches, mem, t).cpu().numpy()
        tok = torch.full((1, N), tab['dead_tok'], dtype=torch.int64, device=dev)
        chars = tab['dead_char'].expand(1, N, tab['C']).contiguous()
        for s in range(N):
            if not live[s]:
                continue
            b = s // k
            w = choose(s, t, ll[s], allowed_mask(ll[s], V, fs, fl[b], ow[b], t, min_t))
            if w is None:
                live[s] = False
                continue
            seqs[s].append(w)
            scores[s] += float(ll[s, w])
            cls = fs[w] if w < V else fl[b, w - V]
            if cls == END_:
                live[s] = False
            elif t + 1 < max_t:
                tok[0, s] = tab['tok_shared'][w] if w < V else tab['tok_local'][b, w - V]
                chars[0, s] = tab['char_shared'][w] if w < V else tab['char_local'][b, w - V]
    return seqs, scores


def _ids_of(model, memory, b, seq):
    """Output ids of a hypothesis' tokens (after <STR>) in graph b."""
    pv = model.vocabs['predictable_token']
    inv = {w: i for i, w in memory['local_idx2token'][b].items()}
    return [inv[w] if w in inv else pv.token2idx(w) for w in seq[1:]]


def _samples(beam):
    """(sequence, score) of every sample of a Beam from sample_device, completed ones first."""
    return [(h.seq, h.score) for h in beam.completed_hypotheses] + [(h.seq, h.score) for h in beam.hypotheses]


def _check_invariants(model, memory, beams, k, max_t, min_t):
    from gtos_amd.vocab import END, UNK, STR
    pv = model.vocabs['predictable_token']
    for b, beam in enumerate(beams):
        local = memory['local_idx2token'][b]
        own = set(local.values())
        assert len(beam.completed_hypotheses) + len(beam.hypotheses) == k, b
        assert 1 <= beam.steps <= max_t
        for h in beam.completed_hypotheses:
            assert h.seq[0] == STR and h.seq[-1] == END and END not in h.seq[1:-1], (b, h.seq)
            assert len(h.seq) - 2 >= min_t, (b, h.seq)
        for h in beam.hypotheses:
            assert h.seq[0] == STR and END not in h.seq and len(h.seq) - 1 == max_t, (b, h.seq)
        for h in beam.completed_hypotheses + beam.hypotheses:
            assert UNK not in h.seq, (b, h.seq)
            for w in h.seq[1:]:
                assert w in own or pv.token2idx(w) != pv.unk_idx, (b, w)      # a copy of this graph, or a vocabulary word
            assert np.isfinite(h.score) and h.score <= 0.0


def _teacher_forced(model, memory, beams, k, max_t, min_t):
    """Each sample's score recomputed through decode_slots fed its own tokens."""
    want = {}
    for b, beam in enumerate(beams):
        for j, (seq, _) in enumerate(_samples(beam)):
            want[b * k + j] = _ids_of(model, memory, b, seq)
    seqs, scores = _host_decode(model, memory, k, max_t, min_t,
                                lambda s, t, row, allow: want[s][t] if t < len(want[s]) else None)
    for b, beam in enumerate(beams):
        for j, (seq, score) in enumerate(_samples(beam)):
            s = b * k + j
            assert seqs[s] == want[s]
            assert abs(scores[s] - score) <= 1e-4 * max(1.0, abs(score)), (b, j, scores[s], score)


@pytest.mark.gpu
def test_sampling_end_to_end_fp32(monkeypatch):
    from test_device_beam_search import _synth_model
    from gtos_amd import search
    model, batch = _synth_model("C1", torch.float32)
    memory = _capture_memory(model, batch, monkeypatch)
    B = len(memory['local_idx2token'])
    k, max_t, min_t = 4, 12, 3
    # top_k = 1 is greedy: a host loop taking the arg-max of the allowed columns (lower column on ties)
    seqs, scores = _host_decode(model, memory, k, max_t, min_t, lambda s, t, row, allow: int(np.argmax(np.where(allow, row, -np.inf))))
    greedy = model.work(batch, k, max_t, min_t, search="sample", top_k=1, seed=11)
    for b, beam in enumerate(greedy):
        got = {tuple(_ids_of(model, memory, b, seq)): score for seq, score in _samples(beam)}
        for j in range(k):
            s = b * k + j
            assert tuple(seqs[s]) in got, (b, j)
            assert got[tuple(seqs[s])] == scores[s], (b, j)
    # one seed, one result; another seed, another; sync_every changes nothing
    run = lambda seed, sync=8, **kw: search.sample_device(model, memory, _fresh(B, k, max_t, min_t), kw.get("T", 1.0),
                                                            kw.get("top_k", 0), kw.get("top_p", 1.0), seed, sync_every=sync)
    key = lambda beams: [(b.steps, _samples(b)) for b in beams]
    for T, top_k, top_p in ((1.0, 0, 1.0), (0.6, 5, 0.9), (2.0, 0, 0.5)):
        a = run(5, T=T, top_k=top_k, top_p=top_p)
        assert key(a) == key(run(5, T=T, top_k=top_k, top_p=top_p))
        for sync in (1, 64):
            assert key(a) == key(run(5, sync, T=T, top_k=top_k, top_p=top_p)), sync
        _check_invariants(model, memory, a, k, max_t, min_t)
        _teacher_forced(model, memory, a, k, max_t, min_t)
    assert key(run(5)) != key(run(6))
    # through work(): same seed, same beams; get_k_best reads them
    w1 = model.work(batch, k, max_t, min_t, search="sample", temperature=0.8, seed=99)
    w2 = model.work(batch, k, max_t, min_t, search="sample", temperature=0.8, seed=99)
    assert key(w1) == key(w2)
    for beam in w1:
        assert len(beam.get_k_best(2, 0.6)) >= 1


@pytest.mark.gpu
def test_sampling_end_to_end_bf16_c2(monkeypatch):
    """C2-shaped eval batch in bf16, 8 samples, 50 steps: the vocabulary invariants, teacher-forced scores, and no host read inside
    the loop but the flag every sync_every steps (stats counts it and the two final tables)."""
    from test_device_beam_search import _synth_model
    from gtos_amd import search, ops
    model, batch = _synth_model("C2", torch.bfloat16)
    memory = _capture_memory(model, batch, monkeypatch)
    B = len(memory['local_idx2token'])
    k, max_t, min_t, sync = 8, 50, 2, 8
    reads = [0]
    inside = [False]

    def spy(name):
        orig = getattr(torch.Tensor, name)

        def f(self, *a, **kw):
            if inside[0] and self.is_cuda:
                reads[0] += 1
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
    monkeypatch.setattr(ops, "sample_step", inside_of(ops.sample_step))
    stats = {}
    beams = search.sample_device(model, memory, _fresh(B, k, max_t, min_t), 0.9, 0, 0.95, 2026, sync_every=sync, stats=stats)
    monkeypatch.undo()
    assert reads[0] == 0
    assert stats["host_reads"] <= (max_t - 1) // sync + 2 and stats["steps"] <= max_t
    _check_invariants(model, memory, beams, k, max_t, min_t)
    _teacher_forced(model, memory, beams, k, max_t, min_t)
    assert sum(len(b.completed_hypotheses) for b in beams) + sum(len(b.hypotheses) for b in beams) == B * k
