"""Device-resident beam search (gtos_amd.search.beam_search_device, csrc/beam.hip, csrc/beam_kernels.h).

CPU: the selection header compiled with g++ is driven through random multi-step searches next to search.py's own loop
(beam_search over Beam.advance, fed the same candidate lists); parents, sequences, fp64 scores, completion order and step counters
must agree exactly.  GPU: the three kernels against torch / Beam.advance, and Generator.work(search="device") against the reference's
beams and against the host search."""
import ctypes

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver


DRIVER = r"""
#include "beam_kernels.h"
using namespace gtos_beam;
// what one gtos_beam_advance launch does, serially: the same flag rotation, every beam's advance by advance_serial
extern "C" void advance_all(int B, int k, int t, int V, int tot, int min_t, int max_t, const float* topv, const int* topi,
                            const uint8_t* fs, const uint8_t* fl, double* slot_score, int* state, int* bp_parent, int* bp_token,
                            int* comp_step, int* comp_parent, double* comp_score, int* active) {
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
"""

PAD, UNK, STR, END = "<PAD>", "<UNK>", "<STR>", "<END>"


@pytest.fixture(scope="module")
def host_advance(tmp_path_factory):
    fn = compile_host_driver(tmp_path_factory, "beam_host", DRIVER).advance_all
    fn.argtypes = [ctypes.c_int] * 7 + [ctypes.c_void_p] * 12
    fn.restype = None
    return fn


def _np_ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Tables(object):
    """The per-search device tables as numpy arrays (int32 state / back-pointers / completions, fp64 scores)."""

    def __init__(self, B, k, max_t):
        N = B * k
        self.B, self.k, self.N, self.max_t = B, k, N, max_t
        self.active = np.array([1, 0, 0], dtype=np.int32)
        self.state = np.zeros((B, 4), dtype=np.int32)
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
                          self.comp_score.ravel().tolist(), lambda b, i: strings[b][i])


def host_step(fn):
    def step(tab, t, V, tot, min_t, topv, topi, fs, fl):
        fn(tab.B, tab.k, t, V, tot, min_t, tab.max_t, _np_ptr(topv), _np_ptr(topi), _np_ptr(fs), _np_ptr(fl),
           *[_np_ptr(a) for a in tab.arrays()])
    return step


def gpu_step(tab, t, V, tot, min_t, topv, topi, fs, fl):
    """The same step on the device kernel: tables up, one gtos_beam_advance, tables down."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    g = [torch.from_numpy(a).to(dev) for a in tab.arrays()]
    ops.beam_advance(t, tab.k, V, tot, min_t, tab.max_t, torch.from_numpy(topv).to(dev), torch.from_numpy(topi).to(dev),
                     torch.from_numpy(fs).to(dev), torch.from_numpy(fl).to(dev) if fl.size else None, *g)
    for a, x in zip(tab.arrays(), g):
        a[...] = x.cpu().numpy()


def random_search(rng, step_fn, B, k, min_t, max_t, V, n_local):
    """One multi-step search: search.py's beam_search (host rules) and step_fn (the fixed-slot tables) fed the same candidate lists.
    Every token class occurs: <UNK> / <END> as vocabulary ids and as copy strings, ties (values on a coarse grid) and -inf.
    Returns the number of beam advances compared."""
    from gtos_amd.search import Beam, beam_search
    tot = V + n_local
    words = [PAD, UNK, END] + ["w%d" % i for i in range(V - 3)]
    strings = []
    for b in range(B):
        loc = [rng.choice([UNK, END, "w1", "c%d" % j, "c%d" % j]) for j in range(n_local)]
        strings.append(words + loc)
    cls = lambda w: 1 if w == UNK else 2 if w == END else 0
    fs = np.array([cls(w) for w in words], dtype=np.uint8)
    fl = np.array([[cls(w) for w in s[V:]] for s in strings], dtype=np.uint8).reshape(B, n_local)
    tab = Tables(B, k, max_t)
    parents_log = []

    class RecBeam(Beam):
        def advance(self, last_steps):
            parents = super().advance(last_steps)
            parents_log[-1][self.index] = parents
            return parents

    beams = [RecBeam(k, min_t, max_t) for _ in range(B)]
    for b, beam in enumerate(beams):
        beam.index = b
    n_adv = [0]
    t_box = [0]

    class FakeModel(object):
        def decode_step_batched(self, tokens, state, memory, beam_of_hyp, offset, topk):
            t = t_box[0]
            # the fixed-slot tables agree with the host beams before this step
            compare(tab.beams(strings, min_t), beams, "before step %d" % t)
            topv = np.full((B * k, k), np.nan, dtype=np.float32)
            topi = np.zeros((B * k, k), dtype=np.int32)
            for s in range(B * k):
                ids = rng.choice(tot, size=k, replace=False)
                vals = rng.choice([-0.5, -1.0, -1.5, -2.0, -3.0, -np.inf], size=k, p=[.25, .25, .2, .15, .1, .05]).astype(np.float32)
                if rng.rand() < 0.5:
                    vals = (vals + rng.randn(k).astype(np.float32) * 0.01).astype(np.float32)
                order = np.lexsort((ids, -vals.astype(np.float64)))       # descending value, lower id first
                topv[s], topi[s] = vals[order], ids[order]
            owners = beam_of_hyp.tolist()
            results, pos = [], {}
            for bi in owners:
                j = pos.get(bi, 0)
                pos[bi] = j + 1
                s = bi * k + j
                results.append([(strings[bi][int(i)], float(v)) for v, i in zip(topv[s], topi[s])])
            if t:
                check_parents(t - 1)
            parents_log.append({})
            step_fn(tab, t, V, tot, min_t, topv, topi, fs, fl)
            t_box[0] += 1
            return {}, results

    def check_parents(t):              # Beam.advance's parents of step t against the back-pointer row t
        for bi, par in parents_log[t].items():
            n_adv[0] += 1
            got = [int(p) - bi * k for p in tab.bp_parent[t, bi * k:bi * k + len(par)]]
            assert got == list(par), ("parents", t, bi)
            assert int(tab.state[bi, 2]) == len(par), ("live", t, bi)

    beam_search(FakeModel(), beams, {'probe': torch.zeros(1)})
    if t_box[0]:
        check_parents(t_box[0] - 1)
    # the device loop keeps launching steps up to max_t: they must change nothing
    snap = [a.copy() for a in tab.arrays()[:-1]]
    for t in range(t_box[0], max_t):
        step_fn(tab, t, V, tot, min_t, np.zeros((B * k, k), np.float32), np.zeros((B * k, k), np.int32), fs, fl)
    for a, b_ in zip(tab.arrays()[:-1], snap):
        assert np.array_equal(a, b_, equal_nan=True), "a step after the end changed the tables"
    compare(tab.beams(strings, min_t), beams, "end")
    return n_adv[0]


def compare(got, want, what):
    for b, (g, w) in enumerate(zip(got, want)):
        tag = "%s, beam %d" % (what, b)
        assert g.steps == w.steps, tag
        assert [(h.seq, h.score) for h in g.hypotheses] == [(h.seq, h.score) for h in w.hypotheses], tag + " alive"
        assert [(h.seq, h.score) for h in g.completed_hypotheses] == [(h.seq, h.score) for h in w.completed_hypotheses], tag + " completed"
        assert g.completed() == w.completed(), tag


def test_selection_header_matches_beam_advance(host_advance):
    rng = np.random.RandomState(20261015)
    step = host_step(host_advance)
    n = 0
    for it in range(900):
        k = int(rng.choice([1, 2, 3, 4, 5, 8])) if it % 50 else 32
        B = int(rng.randint(1, 5))
        max_t = int(rng.randint(1, 9))
        min_t = int(rng.randint(0, 4))
        n += random_search(rng, step, B, k, min_t, max_t, V=int(rng.randint(max(4, k), 40)), n_local=int(rng.randint(0, 6)))
    assert n >= 10000, n


def test_beam_entry_points_refuse_unsupported_shapes():
    """k > 32, tot < k, a step outside the tables, misaligned cache rows: -10 (shape), nothing launched, no device needed."""
    from gtos_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(16)
    assert lib.gtos_beam_topk(4, 100, 33, p, 100, p, p, None) == -10
    assert lib.gtos_beam_topk(4, 8, 9, p, 8, p, p, None) == -10
    assert lib.gtos_beam_topk(4, 100, 8, p, 99, p, p, None) == -10
    assert lib.gtos_beam_advance(2, 33, 0, 10, 10, 0, 5, *[p] * 13) == -10
    assert lib.gtos_beam_advance(2, 4, 5, 10, 10, 0, 5, *[p] * 13) == -10
    assert lib.gtos_beam_advance(2, 4, 0, 10, 9, 0, 5, *[p] * 13) == -10
    args = lambda row_bytes, N, k, t: (1, p, p, row_bytes, N, k, t, 5, p, p, p, p, 10, 10, p, p, p, p, 22, 0, p, p, p, None)
    assert lib.gtos_beam_reorder(*args(24, 8, 4, 0)) == -10
    assert lib.gtos_beam_reorder(*args(32, 9, 4, 0)) == -10
    assert lib.gtos_beam_reorder(*args(32, 8, 4, 5)) == -10
    assert lib.gtos_beam_reorder(*args(32, 8, 33, 0)) == -10


def test_work_refuses_an_unknown_search():
    from gtos_amd.generator import Generator
    with pytest.raises(ValueError):
        Generator.work(None, {}, 4, 10, search="gpu")


# ------------------------------------------------------------------------------------------------ GPU: kernels
@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 8, 32])
@pytest.mark.parametrize("tot", [32, 997, 20000, 65536])
def test_beam_topk_equals_torch_topk(k, tot):
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(k * 100003 + tot)
    rows, ld = 37, tot + 5                                   # ragged leading dimension
    buf = torch.full((rows, ld), float("nan"))
    distinct = torch.stack([torch.randperm(tot, generator=g).float() / tot - 0.5 for _ in range(rows)])
    buf[:, :tot] = distinct
    x = buf.to(dev)[:, :tot]
    v, i = ops.beam_topk(x, k)
    wv, wi = torch.topk(distinct, k, 1)
    assert torch.equal(v.cpu(), wv) and torch.equal(i.cpu().long(), wi)
    # planted ties (a handful of distinct values, -inf among them): the lower column first
    tied = torch.randint(0, 4, (rows, tot), generator=g).float() - 3.0
    tied[tied == -3.0] = float("-inf")
    tied[0] = float("-inf")                                  # an all -inf row
    buf[:, :tot] = tied
    x = buf.to(dev)[:, :tot]
    v, i = ops.beam_topk(x, k)
    order = torch.sort(-tied.double(), dim=1, stable=True)[1][:, :k]
    assert torch.equal(i.cpu().long(), order)
    assert torch.equal(v.cpu(), torch.gather(tied, 1, order))


@pytest.mark.gpu
def test_beam_advance_kernel_matches_beam_advance():
    rng = np.random.RandomState(7)
    n = 0
    for it in range(60):
        k = int(rng.choice([1, 3, 8])) if it % 20 else 32
        B = int(rng.randint(1, 6))
        n += random_search(rng, gpu_step, B, k, int(rng.randint(0, 3)), int(rng.randint(1, 10)),
                           V=int(rng.randint(max(4, k), 50)), n_local=int(rng.randint(0, 5)))
    assert n > 300


@pytest.mark.gpu
@pytest.mark.parametrize("dtype,width", [(torch.bfloat16, 1024), (torch.float32, 72)])
def test_beam_reorder_gathers_exactly(dtype, width):
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(width)
    B, k, T, V, tot, C = 5, 4, 9, 30, 37, 22
    N = B * k
    src = [torch.randn(T, N, width, generator=g).to(dtype).to(dev) for _ in range(3)]
    dst = [torch.full_like(s, 7.0) for s in src]
    bp_parent = torch.randint(-1, N, (T, N), generator=g, dtype=torch.int32)
    bp_token = torch.randint(0, tot, (T, N), generator=g, dtype=torch.int32)
    state = torch.zeros(B, 4, dtype=torch.int32)
    state[2, 3] = 1                                          # a done beam: its slots are dead
    tok_shared = torch.randint(0, 1000, (V,), generator=g)
    char_shared = torch.randint(0, 100, (V, C), generator=g)
    tok_local = torch.randint(0, 1000, (B, tot - V), generator=g)
    char_local = torch.randint(0, 100, (B, tot - V, C), generator=g)
    dead_char = torch.randint(0, 100, (C,), generator=g)
    for t, act in ((0, 1), (4, 1), (T - 1, 1), (3, 0)):
        active = torch.zeros(3, dtype=torch.int32)
        active[t % 3] = act
        tok_out = torch.full((N,), -5, dtype=torch.int64, device=dev)
        char_out = torch.full((N, C), -5, dtype=torch.int64, device=dev)
        before = [d.clone() for d in dst]
        D = lambda x: x.to(dev)
        ops.beam_reorder(src, dst, t, k, D(bp_parent), D(bp_token), D(state), D(active), V, tot, D(tok_shared), D(tok_local),
                         D(char_shared), D(char_local), 3, D(dead_char), tok_out, char_out)
        par = bp_parent[t].long()
        live = (par >= 0) & (state[torch.arange(N) // k, 3] == 0) & bool(act)
        for s_, d_, b_ in zip(src, dst, before):
            want = b_.cpu().clone()
            if act:
                rows = s_.cpu()[: t + 1, par.clamp(min=0)]
                rows[:, ~live] = 0
                want[: t + 1] = rows
            assert torch.equal(d_.cpu(), want), (t, act)
        ids = bp_token[t].long()
        wt = torch.full((N,), 3, dtype=torch.int64)
        wc = dead_char.expand(N, C).clone()
        for s in range(N):
            if live[s]:
                i, b = int(ids[s]), s // k
                wt[s] = tok_shared[i] if i < V else tok_local[b, i - V]
                wc[s] = char_shared[i] if i < V else char_local[b, i - V]
        assert torch.equal(tok_out.cpu(), wt) and torch.equal(char_out.cpu(), wc), (t, act)


# ------------------------------------------------------------------------------------------------ GPU: end to end
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["beam_smatch", "beam_dep_dev"])
def test_device_search_matches_reference(case, tmp_path):
    """The checks of test_beam_and_vocab.py::test_hip_beam_search_matches_reference on work(..., search="device")."""
    from test_beam_and_vocab import load_case, make_vocabs, batch_of, state_dict_of, check_hyps
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
    batch = batch_of(meta, arrs, dev)
    for run in meta["runs"]:
        beams = model.work(batch, run["beam"], run["max_step"], run["min_step"], search="device")
        for b, (beam, want) in enumerate(zip(beams, run["expect"])):
            tag = "run %s sentence %d" % ((run["beam"], run["max_step"], run["min_step"]), b)
            assert beam.steps == want["steps"], tag
            check_hyps([(h.seq, h.score) for h in beam.completed_hypotheses], want["finished"], tag + " finished")
            check_hyps([(h.seq, h.score) for h in beam.hypotheses], want["alive"], tag + " alive")
            best = [(h.seq, h.score) for h in beam.get_k_best(run["beam"], cfg["alpha"])]
            check_hyps(best, want["k_best"], tag + " k-best")


def _synth_model(config, dtype):
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


@pytest.mark.gpu
def test_device_search_equals_host_search_fp32():
    """C1-sized fp32 batch: every row of the decoder's launches is computed the same whatever the row count (fp32 GEMMs on fixed
    128x128 tiles, row-wise attention / LayerNorm / copy mixture), so the two searches pick the same hypotheses."""
    model, batch = _synth_model("C1", torch.float32)
    for beam_size, max_t, min_t in ((4, 12, 1), (6, 9, 3)):
        host = model.work(batch, beam_size, max_t, min_t)
        dev = model.work(batch, beam_size, max_t, min_t, search="device")
        for b, (h, d) in enumerate(zip(host, dev)):
            assert h.steps == d.steps, b
            hb, db = h.get_k_best(beam_size, 0.6), d.get_k_best(beam_size, 0.6)
            assert [x.seq for x in hb] == [x.seq for x in db], b
            for x, y in zip(hb, db):
                assert (x.score == y.score) or abs(x.score - y.score) <= 1e-5 * abs(x.score), (b, x.score, y.score)


@pytest.mark.gpu
def test_device_search_equals_host_search_bf16_where_selection_is_clear(monkeypatch):
    """C2-sized bf16 batch: the host path's GEMMs see the live-hypothesis count as M, the device path's B*k, and the bf16 kernels
    may round differently.  Every sentence whose host selections are all clear by more than 1e-2 (the sorted pool's gap at the cut,
    the final k-best ranking) must come out identical.  With random weights the next-token distributions are near-uniform and those
    gaps are ~1e-4 (measured: none of the 64 sentences clears 1e-2), so the 80 % bar is put on all sentences: at least 80 % of the
    batch must have identical k-best sequences and step counts (measured: 64 of 64)."""
    import gtos_amd.generator as G
    from gtos_amd.search import Beam
    model, batch = _synth_model("C2", torch.bfloat16)
    beam_size, max_t, alpha = 8, 20, 0.6
    margins = {}

    class RecBeam(Beam):
        def advance(self, last_steps):
            pool = []
            for parent, steps in enumerate(last_steps):
                base = self.hypotheses[parent].score
                pool += [float('-inf') if tok == "<UNK>" else base + ll for tok, ll in steps]
            cut = self.beam_size - len(self.completed_hypotheses)
            s = sorted((x for x in pool if x != float('-inf')), reverse=True)
            gap = s[cut - 1] - s[cut] if 0 < cut < len(s) else float('inf')      # the cut decides which hypotheses go on
            margins[id(self)] = min(margins.get(id(self), float('inf')), gap)
            return super().advance(last_steps)

    monkeypatch.setattr(G, "Beam", RecBeam)
    host = model.work(batch, beam_size, max_t)
    monkeypatch.undo()
    dev = model.work(batch, beam_size, max_t, search="device")
    same = 0
    for b, (h, d) in enumerate(zip(host, dev)):
        m = margins.get(id(h), float('inf'))
        hb, db = h.get_k_best(beam_size, alpha), d.get_k_best(beam_size, alpha)
        ns = [x.score / ((1 + len(x.seq)) ** alpha) for x in hb]
        m = min([m] + [a - b_ for a, b_ in zip(ns, ns[1:])])
        equal = h.steps == d.steps and [x.seq for x in hb] == [x.seq for x in db]
        assert equal or m <= 1e-2, "sentence %d differs although every selection was clear by %.3g" % (b, m)
        same += equal
    assert same >= 0.8 * len(host), (same, len(host))
