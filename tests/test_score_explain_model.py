"""Token-level attribution at the model level, on the GPU: Generator.explain on the golden models against Generator.score (bitwise
token_ll, rank 0 at the argmax), against the batch's copy ids (source, copy_share), against the pinned oracle's ll row (entropy), and
on the k-best strings of the device beam search.  (The kernel, the host glue and the dry-run plans are in tests/test_explain.py.)"""
import pytest
import torch

from conftest import load_golden, sub
from test_score_eval_model import FP32, _beam_model, dev, oracle_ll_row, to_dev

pytestmark = pytest.mark.gpu

PAD = 0


def small_generator(g):
    """test_hip_parity.build_generator with STRING vocabularies of the golden sizes (targets are given as strings)"""
    from gtos_amd import synth
    from gtos_amd.generator import Generator
    from tests_support import SMALL_GEN_ARGS, SMALL_VOCAB
    d, ff, H, gl = [int(v) for v in g["cfg"]]
    m = Generator(synth.synth_vocabs(SMALL_VOCAB), *SMALL_GEN_ARGS, d, ff, H, 0.0, 1, gl, 2, None, dev(), factored_relation=True).to(dev())
    m.load_state_dict(sub(g, "sd/"))
    return m


def with_copy_tables(data, V):
    cp = data['cp_seq']
    data = dict(data)
    data['local_idx2token'] = [{int(i): "copy%d" % int(i) for i in cp[:, b].tolist() if i >= V} for b in range(cp.shape[1])]
    return data


def own_strings(data, vocab, b, of=None):
    """the target sentence of column b (without <END>) as strings; copy ids through the table of graph ``of``"""
    table = data['local_idx2token'][b if of is None else of]
    ids = [int(i) for i in data['token_out'][:, b].tolist() if i != PAD][:-1]
    return [table.get(i) or data['local_idx2token'][b].get(i) or vocab.idx2token(i) for i in ids]


def oracle_entropy(om, data):
    """[T,B] float64: the entropy of the oracle's row, p = exp(ll) - 1e-12 clamped at 0"""
    p = (torch.exp(oracle_ll_row(om, data).double()) - 1e-12).clamp(min=0)
    return -(p * torch.log(torch.where(p > 0, p, torch.ones_like(p)))).sum(-1)


def check_invariants(ex, sc, target, cp_seq, V, bitwise=True):
    """what must hold between explain, score and the batch's copy ids on every position; all on the CPU"""
    c = lambda t: t.cpu()                                              # noqa: E731
    target, owner = c(target), c(ex.graph_of)
    live = target.ne(PAD)
    if bitwise:
        assert torch.equal(c(ex.token_ll).view(torch.int32), c(sc.token_ll).view(torch.int32)), "token_ll is not bitwise score's"
    for k in ex._fields[:9]:
        assert bool(torch.isfinite(c(getattr(ex, k)).double()).all()), k
    assert c(ex.tokens).tolist() == live.sum(0).tolist() and owner.tolist() == c(sc.graph_of).tolist()
    rank, source, share, sw, fw = c(ex.rank), c(ex.source).long(), c(ex.copy_share), c(ex.source_weight), c(ex.focus_weight)
    hit = c(sc.pred).long().eq(target) & live
    assert bool((rank[hit] == 0).all()), "a target that is the argmax has something above it"
    ids = c(cp_seq).index_select(1, owner)                             # [S, N] the copy ids each sequence was explained against
    among = (ids.unsqueeze(0) == target.unsqueeze(1)).any(1) & live    # [T, N]
    reachable = live & ((target < V) | among)
    assert torch.equal(rank >= 0, reachable) and bool((rank[~reachable] == -1).all())
    assert torch.equal(source >= 0, among), "source >= 0 exactly where the target is among the graph's copy ids"
    assert torch.equal(ids.gather(0, source.clamp(min=0))[among], target[among])
    assert bool((share[source < 0] == 0).all()) and bool((sw[source < 0] == 0).all())
    copied = (target >= V) & (sw > 0)
    assert bool((share[copied] == 1).all())
    assert bool((fw >= sw).all()) and bool(((share >= 0) & (share <= 1)).all())
    foc = c(ex.focus).long()
    assert bool(((foc >= 0) & (foc < ids.shape[0])).all())
    return live, int(among.sum()), int(copied.sum())


@pytest.mark.parametrize("name", ["gen_small", "gen_padded"])
@pytest.mark.parametrize("which", ["batch/", "ebatch/"])
def test_explain_vs_score_copy_ids_and_oracle_fp32(name, which):
    from test_oracle_golden import build_small_generator
    from gtos_amd.data import batchify_targets
    g = load_golden(name)
    m = small_generator(g)
    om = build_small_generator(g)
    om.eval()
    pv = m.vocabs['predictable_token']
    V = pv.size
    data = with_copy_tables(sub(g, which), V)
    on_dev = to_dev(data)
    B = data['token_out'].shape[1]
    # ---- the batch's own sentences, in both modes
    want_H = oracle_entropy(om, data)
    for mode in (True, False):
        m.train(mode)
        ex, sc = m.explain(on_dev), m.score(on_dev)
        assert m.training == mode
        live, n_among, n_copied = check_invariants(ex, sc, data['token_out'], data['cp_seq'], V)
        torch.testing.assert_close(ex.entropy.cpu().double()[live], want_H[live], **FP32)
    print("MEASURED %s %s own sentences: %d positions, %d hold a copy id, %d copied ids >= V, copy_share > 0.5 on %d, rank 0 on %d" % (
        name, which, int(live.sum()), n_among, n_copied, int((ex.copy_share.cpu()[live] > 0.5).sum()), int((ex.rank.cpu()[live] == 0).sum())))
    assert n_among > 0
    rows = ex.rows(on_dev)
    assert [len(r) for r in rows] == ex.tokens.cpu().tolist() and all(isinstance(d["token"], str) for r in rows for d in r)
    assert all(d["source_concept"] is None or isinstance(d["source_concept"], str) for r in rows for d in r)
    # ---- an n-best list of two per graph: the graph's own sentence, and its neighbour's read through this graph's copy table
    first = [own_strings(data, pv, b) for b in range(B)]
    second = [own_strings(data, pv, (b + 1) % B, of=b)[::-1] for b in range(B)]
    targets = [[first[b], second[b]] for b in range(B)]
    ex, sc = m.explain(on_dev, targets), m.score(on_dev, targets)
    assert ex.graph_of.cpu().tolist() == [b for b in range(B) for _ in range(2)]
    live, n_among, _ = check_invariants(ex, sc, ex.target, data['cp_seq'], V)
    assert n_among > 0
    tables = [{w: i for i, w in t.items()} for t in data['local_idx2token']]
    got_H = ex.entropy.cpu().double()
    for j, seqs in enumerate((first, second)):
        built = batchify_targets(seqs, m.vocabs, tables)
        assert torch.equal(built['token_out'], ex.target.cpu()[:built['token_out'].shape[0], j::2])
        want = oracle_entropy(om, dict(data, **built))
        keep = built['token_out'].ne(PAD)
        torch.testing.assert_close(got_H[:want.shape[0], j::2][keep], want[keep], **FP32)


@pytest.mark.parametrize("name", ["gen_small", "gen_padded"])
def test_explain_bf16_is_finite_and_keeps_the_integer_invariants(name):
    g = load_golden(name)
    m = small_generator(g)
    m.set_compute_dtype(torch.bfloat16)
    V = m.vocabs['predictable_token'].size
    data = with_copy_tables(sub(g, "batch/"), V)
    on_dev = to_dev(data)
    ex, sc = m.explain(on_dev), m.score(on_dev)
    check_invariants(ex, sc, data['token_out'], data['cp_seq'], V, bitwise=False)
    B = data['token_out'].shape[1]
    targets = [[own_strings(data, m.vocabs['predictable_token'], b), []][:1 + b % 2] for b in range(B)]
    ex, sc = m.explain(on_dev, targets), m.score(on_dev, targets)
    check_invariants(ex, sc, ex.target, data['cp_seq'], V, bitwise=False)


@pytest.mark.parametrize("case", ["beam_smatch", "beam_dep_dev"])
def test_explain_sums_to_the_device_beam_search_scores(case, tmp_path):
    """The k-best strings of work(search="device"), passed to explain as targets: the sum of token_ll per sequence is the score the
    search gave the hypothesis, |diff| <= 1e-3 (tokens + 1) (the bar of test_score_agrees_with_the_device_beam_search)."""
    from gtos_amd.vocab import END
    model, batch, meta, _ = _beam_model(case, tmp_path)
    alpha = meta["cfg"]["alpha"]
    run = meta["runs"][0]
    beams = model.work(batch, run["beam"], run["max_step"], run["min_step"], search="device")
    hyps = [beam.get_k_best(run["beam"], alpha) for beam in beams]
    targets = [[list(h.seq[1:-1]) if h.seq[-1] == END else list(h.seq[1:]) for h in hs] for hs in hyps]
    ex = model.explain(batch, targets)
    ll, tokens, owner = ex.token_ll.double().sum(0).cpu().tolist(), ex.tokens.cpu().tolist(), ex.graph_of.cpu().tolist()
    flat = [(b, h) for b, hs in enumerate(hyps) for h in hs]
    assert len(flat) == len(ll) and owner == [b for b, _ in flat]
    compared = 0
    for (b, h), got, n in zip(flat, ll, tokens):
        if h.seq[-1] != END:                      # unfinished: explained (with an <END> the search never took), not compared
            continue
        assert n == len(h.seq) - 1
        assert abs(got - h.score) <= 1e-3 * (n + 1), (case, run["beam"], b, h.seq, got, h.score)
        compared += 1
    assert compared > 0
    rows = ex.rows(batch)
    assert [len(r) for r in rows] == tokens
    assert [d["token"] for d in rows[0][:-1]] == targets[owner[0]][0]
