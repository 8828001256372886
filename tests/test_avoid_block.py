"""Negative constraints (Generator.work(..., avoid=), gtos_amd.search, csrc/avoid.hip, csrc/avoid_kernels.h).

CPU: the rule header compiled with g++ against a brute-force statement of the rule, check_avoid, the entry point's refusals, the launch
plans of both device decoders under the dry run, and the host beam search on a fake model.  GPU: gtos_avoid_block against a numpy
statement (exact), its stores inside guard bands, work() with the host and the device search on the two golden models against a
restatement of the search around the oracle's next-token log-likelihoods, the compositions with every other option on the small
golden generator, and sampling restated draw by draw."""
import collections
import ctypes
import types

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver, Guarded, SMALL_VOCAB, SMALL_GEN_ARGS

NEG_INF = float("-inf")
M64 = (1 << 64) - 1
PAD, UNK, STR, END = '<PAD>', '<UNK>', '<STR>', '<END>'

DRIVER = r"""
#include "avoid_kernels.h"
using namespace gtos_avoid;
extern "C" uint64_t av_next(const int* pat, int n_pos, uint64_t d, uint64_t init, int w) { return next_state(d, init, mask_serial(pat, n_pos, w)); }
extern "C" uint64_t av_ban_word(uint64_t d, uint64_t init, uint64_t last) { return ban_word(d, init, last); }
extern "C" int av_ban_pos(uint64_t ban, int i, int pat_i) { return ban_at(ban, i, pat_i); }
extern "C" int av_banned(const int* pat, int n_pos, uint64_t d, uint64_t init, uint64_t last, int* out) {
    return banned_serial(pat, n_pos, d, init, last, out);
}
extern "C" int av_max_pos() { return MAX_POS; }
"""


def brute_avoided(y, entries, alphabet):
    """The rule, stated without any state: w is banned iff y + [w] ends in some entry."""
    out = set()
    for w in alphabet:
        z = list(y) + [w]
        if any(len(z) >= len(p) and z[len(z) - len(p):] == list(p) for p in entries):
            out.add(w)
    return out


def holds_entry(y, entries):
    y = list(y)
    return any(y[i:i + len(p)] == list(p) for p in entries for i in range(len(y) - len(p) + 1))


def unsigned(x):
    return int(x) & M64


def tables_of(entries):
    """(pat [64] int32, init, last, n_pos) of one graph, init / last as unsigned Python ints"""
    from gtos_amd.search import avoid_tables
    pat, init, last, n_pos = avoid_tables([entries])
    return np.array(pat[0], dtype=np.int32), unsigned(init[0]), unsigned(last[0]), n_pos[0]


# ------------------------------------------------------------------------------------------------ CPU: the header
@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = compile_host_driver(tmp_path_factory, "avoid_host", DRIVER)
    u64, i32, vp = ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p
    lib.av_next.argtypes, lib.av_next.restype = [vp, i32, u64, u64, i32], u64
    lib.av_ban_word.argtypes, lib.av_ban_word.restype = [u64, u64, u64], u64
    lib.av_ban_pos.argtypes = [u64, i32, i32]
    lib.av_banned.argtypes = [vp, i32, u64, u64, u64, vp]
    return lib


def random_entries(rng, alphabet, kind):
    """An entry list of at most 64 positions over ids [0, alphabet); ``kind`` picks the hard cases."""
    a, b, c = (int(x) for x in rng.randint(0, alphabet, size=3))
    if kind == "single":
        return [[int(x) for x in rng.randint(0, alphabet, size=rng.randint(1, 17))]]
    if kind == "full":                                                  # exactly 64 positions
        out, left = [], 64
        while left:
            n = min(left, int(rng.randint(1, 17)))
            out.append([int(x) for x in rng.randint(0, alphabet, size=n)])
            left -= n
        return out
    if kind == "overlap":
        return [[a, a, b], [a, b, a, b, c][:int(rng.randint(2, 6))]]
    if kind == "prefix":
        return [[a, b], [a, b, c], [a]][:int(rng.randint(2, 4))]
    if kind == "suffix":
        return [[b, c], [a, b, c], [c]][:int(rng.randint(2, 4))]
    out = []                                                            # "random": short entries mostly, a long one sometimes
    for _ in range(int(rng.randint(1, 7))):
        n = int(rng.randint(1, 17)) if rng.rand() < 0.2 else int(rng.randint(1, 4))
        if sum(len(p) for p in out) + n > 64:
            break
        out.append([int(x) for x in rng.randint(0, alphabet, size=n)])
    return out


def test_rule_header_matches_brute_force(host_lib):
    from gtos_amd import ops
    from gtos_amd.search import avoided_tokens
    assert host_lib.av_max_pos() == ops.AVOID_TOKENS_MAX == 64
    rng = np.random.RandomState(20261019)
    out = np.zeros(64, dtype=np.int32)
    rows = steps = nonempty = 0
    kinds = ["random", "single", "full", "overlap", "prefix", "suffix"]
    lengths = set()
    W, T = 4, 12                                                        # hypotheses per table, steps
    for rep in range(420):
        for alphabet in (2, 3, 50):
            kind = kinds[rep % len(kinds)]
            entries = random_entries(rng, alphabet, kind)
            lengths.update(len(p) for p in entries)
            pat, init, last, n_pos = tables_of(entries)
            assert n_pos == sum(len(p) for p in entries) <= 64 and (kind != "full" or n_pos == 64) and (kind != "single" or len(entries) == 1)
            hyps = [([], 0)] * W                                        # (history, state): every hypothesis starts from D = 0

            def check(y, d):
                m = host_lib.av_banned(pat.ctypes.data, n_pos, d, init, last, out.ctypes.data)
                got = out[:m].tolist()
                want = brute_avoided(y, entries, range(alphabet))
                assert 0 <= m <= n_pos and set(got) == want, (entries, y, got, want)
                ban = host_lib.av_ban_word(d, init, last)
                if steps % 16 == 0:                                     # position by position, as the kernel's lanes take it
                    per_pos = [host_lib.av_ban_pos(ban, i, int(pat[i]) if 0 <= i < 64 else 5) for i in range(-1, 66)]
                    assert [w for w in per_pos if w >= 0] == got, (entries, y)
                else:
                    assert [int(pat[i]) for i in range(n_pos) if (ban >> i) & 1] == got, (entries, y)
                assert sorted(avoided_tokens(y, entries)) == sorted(got), (entries, y)          # the host search's list form
                return bool(want)
            nonempty += check([], 0)                                    # step 0: only the one-id entries ban
            steps += 1
            for t in range(T):
                nxt = []
                for j in range(W):
                    y, d = hyps[int(rng.randint(W))]                    # a parent: the state is inherited, not recomputed
                    w = int(rng.randint(alphabet))                      # any token, banned or not
                    y2, d2 = y + [w], host_lib.av_next(pat.ctypes.data, n_pos, d, init, w)
                    # bit i of the state: the history ends in its entry up to position i
                    pos = 0
                    for p in entries:
                        for i in range(len(p)):
                            ends = len(y2) >= i + 1 and y2[len(y2) - i - 1:] == p[:i + 1]
                            assert bool((d2 >> (pos + i)) & 1) == ends, (entries, y2, pos + i)
                        pos += len(p)
                    nonempty += check(y2, d2)
                    steps += 1
                    nxt.append((y2, d2))
                hyps = nxt
            rows += W
    assert rows >= 5000 and lengths >= set(range(1, 17)), (rows, sorted(lengths))
    print("MEASURED %d rows, %d steps, %d with a non-empty ban set (%.0f %%)" % (rows, steps, nonempty, 100.0 * nonempty / steps))
    assert 3 * nonempty >= steps, (nonempty, steps)
    # what the rule promises: a history built only from tokens that are not banned never holds an entry
    for trial in range(300):
        alphabet = int(rng.choice([3, 4, 5]))
        entries = random_entries(rng, alphabet, kinds[trial % len(kinds)])
        pat, init, last, n_pos = tables_of(entries)
        y, d = [], 0
        for _step in range(14):
            m = host_lib.av_banned(pat.ctypes.data, n_pos, d, init, last, out.ctypes.data)
            free = [w for w in range(alphabet) if w not in set(out[:m].tolist())]
            if not free:
                break
            w = int(rng.choice(free))
            y, d = y + [w], host_lib.av_next(pat.ctypes.data, n_pos, d, init, w)
            assert not holds_entry(y, entries), (entries, y)
        for w in brute_avoided(y, entries, range(alphabet)):
            assert holds_entry(y + [w], entries)


def test_avoid_tables_by_hand():
    from gtos_amd.search import avoid_tables, avoided_tokens
    pat, init, last, n_pos = avoid_tables([[[5], [7, 8, 9]], [], [[1] * 16] * 4])
    assert pat[0][:4] == [5, 7, 8, 9] and set(pat[0][4:]) == {-1} and (init[0], last[0], n_pos[0]) == (0b0011, 0b1001, 4)
    assert set(pat[1]) == {-1} and (init[1], last[1], n_pos[1]) == (0, 0, 0)
    assert n_pos[2] == 64 and unsigned(last[2]) == sum(1 << i for i in (15, 31, 47, 63)) and last[2] < 0      # bit 63: a signed word
    for bad in ([[[1] * 16] * 4 + [[2]]], [[[]]]):
        with pytest.raises(ValueError):
            avoid_tables(bad)
    assert avoided_tokens([], [["a"], ["a", "b"]]) == ["a"]
    assert avoided_tokens(["x", "a"], [["a"], ["a", "b"], ["x", "a", "c"], ["y", "a", "d"]]) == ["a", "b", "c"]


# ------------------------------------------------------------------------------------------------ CPU: argument checks
def test_check_avoid():
    from gtos_amd import ops, synth
    from gtos_amd.generator import Generator, check_avoid
    pv = synth.synth_vocabs()['predictable_token']
    plain = [pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END)]
    word, word2 = plain[0], plain[1]
    local = [{pv.size: "copy0", pv.size + 1: "copy1"}, {pv.size: "other"}]
    ok = lambda a, cons=None, phr=None: check_avoid(a, cons, phr, local, pv)              # noqa: E731
    assert ok(None) is None and ok(None, [["copy0"], []], [[["copy0"]], []]) is None
    assert ops.AVOID_TOKENS_MAX == 64
    assert ok([["copy0", [word, "copy1"], (word2,)], []]) == [[["copy0"], [word, "copy1"], [word2]], []]
    assert ok(([], ("other", ["other", "other"]))) == [[], [["other"], ["other", "other"]]]
    # dropped: an entry with a string the graph cannot produce (another graph's copy token, no vocabulary word), and exact duplicates
    assert ok([["other", ["copy0", "no-such-word"], "copy0", ["copy0"], [word, word], (word, word)], ["copy0"]]) == [[["copy0"], [word, word]], []]
    assert ok([[plain[:16]] * 5 + [plain[:16], plain[16:32], plain[32:48], plain[48:64]], []])[0] == [plain[:16], plain[16:32], plain[32:48], plain[48:64]]
    bad = [[["copy0"]], [["copy0"], [], []], "ab", 3,                                       # outer shape and count
           [["copy0"], "other"], [{"copy0": 1}, []], [["copy0"], None],                                  # a graph entry that is no list
           [[[]], []], [[()], []], [[3], []], [[["copy0", 3]], []], [[None], []], [[{"copy0"}], []],     # empty phrase, non-strings
           [[PAD], []], [[["copy0", STR]], []], [[[END]], []], [[[word, UNK]], []], [[UNK], []],
           [[["no-such-word", END]], []],                                                                # a special is refused before dropping
           [[plain[:16], plain[16:32], plain[32:48], plain[48:64], [plain[64]]], []],                    # 65 tokens after dropping
           [plain[:65], []]]
    for a in bad:
        with pytest.raises(ValueError):
            ok(a)
    # contradictions
    for a, cons, phr in (([["copy0"], []], [["copy0"], []], None), ([[[word]], []], [[word2, word], []], None),
                         ([["copy1"], []], None, [[["copy0", "copy1"]], []]), ([[], [["other", word]]], None, [[], [[word2, "other", word]]]),
                         ([[[word, word2]], []], None, [[[word2], [word, word2]], []])):
        with pytest.raises(ValueError):
            ok(a, cons, phr)
    assert ok([[["copy0", "copy1"]], []], [["copy0", "copy1"], []]) == [[["copy0", "copy1"]], []]           # a phrase is no single constraint
    assert ok([[["copy1", "copy0"]], ["other"]], None, [[["copy0", "copy1"]], []]) == [[["copy1", "copy0"]], [["other"]]]
    # through work: the checks run before anything of the model is touched
    me = types.SimpleNamespace(vocabs={'predictable_token': pv})
    data = {'local_idx2token': local}
    for a in bad:
        for kw in (dict(search="host"), dict(search="device"), dict(search="sample", seed=1)):
            with pytest.raises(ValueError):
                Generator.work(me, data, 4, 10, avoid=a, **kw)
    with pytest.raises(ValueError):
        Generator.work(me, data, 4, 10, search="device", avoid=[["copy0"], []], constraints=[["copy0"], []])
    with pytest.raises(ValueError):
        Generator.work(me, data, 4, 10, search="host", avoid=[[["copy0", "copy1"]], []], phrases=[[[word, "copy0", "copy1"]], []])


def test_avoid_entry_point_refuses_bad_arguments():
    """-10 outside the shapes, -23 for null pointers; nothing launched, no device needed."""
    from gtos_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 31
    p, q = ctypes.c_void_p(16), ctypes.c_void_p(32)

    def call(N=8, k=4, t=2, tot=12, ld=12, ll=p, parent=p, token=p, pat=p, init=p, last=p, n_pos=p, prev=p, cur=q, active=p):
        return lib.gtos_avoid_block(N, k, t, tot, ll, ld, parent, token, pat, init, last, n_pos, prev, cur, active, None)
    assert call(t=-1) == -10
    assert call(tot=0) == -10
    assert call(ld=11) == -10
    assert call(N=9) == -10
    assert call(k=0) == -10
    assert call(cur=p) == -10                                           # the two state buffers alternate
    for name in ("ll", "token", "pat", "init", "last", "n_pos", "prev", "cur", "active"):
        assert call(**{name: None}) == -23, name
    for name in ("ll", "pat", "init", "last", "n_pos", "prev", "cur", "active"):
        assert call(t=0, token=None, parent=None, **{name: None}) == -23, name
    assert call(N=0, k=0, t=-1) == 0


def test_ops_avoid_block_passes_the_signature_check():
    from dryrun import DryRun
    from gtos_amd import ops, _lib
    with DryRun() as rec:
        B, k, max_t, tot = 2, 3, 9, 20
        N = B * k
        ll = torch.zeros(N, tot + 3)[:, :tot]
        state = [torch.zeros(N, dtype=torch.int64) for _ in range(2)]
        tok = torch.zeros(max_t, N, dtype=torch.int32)
        active = torch.zeros(3, dtype=torch.int32)
        tabs = [torch.zeros(B, 64, dtype=torch.int32), torch.zeros(B, dtype=torch.int64), torch.zeros(B, dtype=torch.int64),
                torch.zeros(B, dtype=torch.int32)]
        ops.avoid_block(0, k, ll, None, None, *tabs, state[1], state[0], active)
        ops.avoid_block(4, k, ll, None, tok[3], *tabs, state[1], state[0], active)
        ops.avoid_block(5, k, ll, tok[4], tok[4], *tabs, state[0], state[1], active)
        with pytest.raises(AssertionError):
            ops.avoid_block(5, k, ll, None, tok[4], *tabs, state[0], state[0], active)
        with pytest.raises(AssertionError):
            ops.avoid_block(5, k, ll, None, tok[4], torch.zeros(B, 63, dtype=torch.int32), *tabs[1:], state[0], state[1], active)
        with pytest.raises(AssertionError):
            ops.avoid_block(5, k, ll, None, tok[4], *tabs, state[0], state[1].int(), active)
        with pytest.raises(AssertionError):
            ops.avoid_block(5, k, ll, None, None, *tabs, state[0], state[1], active)
        with pytest.raises(_lib.GtosHipError):
            ops.avoid_block(5, k, ll.double(), None, tok[4], *tabs, state[0], state[1], active)
    assert rec.names() == ["gtos_avoid_block"] * 3
    assert rec.calls[0][1][:4] == (N, k, 0, tot) and rec.calls[0][1][5] == tot + 3 and rec.calls[0][1][6] is None and rec.calls[0][1][7] is None
    assert rec.calls[1][1][:4] == (N, k, 4, tot) and rec.calls[1][1][6] is None and rec.calls[1][1][7] is not None
    assert rec.calls[2][1][6] is not None


# ------------------------------------------------------------------------------------------------ CPU: launch plans
def test_launch_plans_differ_by_one_avoid_block_per_step():
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
        B = batch['concept'].shape[1]
        word = next(pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END))
        own = [sorted(local.values()) + [word, word] for local in batch['local_idx2token']]
        avoid = [[w[0], [word, w[1]], [w[1], word, w[0]]] if b % 2 else [] for b, w in enumerate(own)]
        assert any(avoid) and not all(avoid)

        def plan(**kw):
            n0 = len(rec.calls)
            beams = model.work(batch, 4, steps, **kw)
            assert len(beams) == B
            return beams, rec.calls[n0:]
        for kw, select in ((dict(search="device"), "gtos_beam_topk"), (dict(search="sample", seed=3), "gtos_sample_step")):
            base = [c[0] for c in plan(**kw)[1]]
            assert base.count(select) == steps and "gtos_avoid_block" not in base
            beams, calls = plan(avoid=None, **kw)
            assert [c[0] for c in calls] == base and not any(hasattr(b, "avoid") for b in beams)
            beams, calls = plan(avoid=[[] for _ in range(B)], **kw)
            assert [c[0] for c in calls] == base and all(b.avoid == [] for b in beams)
            beams, calls = plan(avoid=avoid, **kw)
            names = [c[0] for c in calls]
            assert [x for x in names if x != "gtos_avoid_block"] == base
            at = [i for i, x in enumerate(names) if x == "gtos_avoid_block"]
            assert len(at) == steps and all(names[i + 1] == select for i in at)
            N = 4 * B
            assert [calls[i][1][:3] for i in at] == [(N, 4, t) for t in range(steps)]
            assert all(calls[i][1][7] is not None for i in at[1:]) and calls[at[0]][1][6] is None and calls[at[0]][1][7] is None
            assert all((calls[i][1][6] is None) == (select == "gtos_sample_step") for i in at[1:])          # the sampler: no parent
            assert [b.avoid for b in beams] == [[[e] if isinstance(e, str) else list(e) for e in a] for a in avoid]
            _, calls = plan(avoid=avoid, no_repeat_ngram=3, **kw)
            names = [c[0] for c in calls]
            assert [x for x in names if x not in ("gtos_avoid_block", "gtos_ngram_block")] == base
            assert names.count("gtos_avoid_block") == steps and names.count("gtos_ngram_block") == steps - 1
            for i, x in enumerate(names):
                if x in ("gtos_avoid_block", "gtos_ngram_block"):
                    assert names[i + 1] in (select, "gtos_avoid_block", "gtos_ngram_block")
        # every other device route takes the launch too, in front of its selection
        word2 = [pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END)][1]
        cons = [[word2] if b % 2 else [] for b in range(B)]
        for kw in (dict(groups=2), dict(constraints=cons), dict(coverage_penalty=0.2), dict(phrases=[[c] if c else [] for c in cons])):
            base = [c[0] for c in plan(search="device", **kw)[1]]
            names = [c[0] for c in plan(search="device", avoid=avoid, **kw)[1]]
            assert [x for x in names if x != "gtos_avoid_block"] == base and names.count("gtos_avoid_block") == steps, kw
            for i, x in enumerate(names):
                if x == "gtos_avoid_block":
                    assert "gtos_beam_topk" in names[i + 1:i + 3], kw
        # the host search through the same glue (numbers mean nothing under the dry run): no device bookkeeping kernel
        n0 = len(rec.calls)
        host = model.work(batch, 4, steps, avoid=avoid)
        assert len(host) == B and not [c[0] for c in rec.calls[n0:] if c[0].startswith(("gtos_beam", "gtos_avoid", "gtos_ngram"))]


# ------------------------------------------------------------------------------------------------ CPU: the host beam search
class FakeModel(object):
    """decode_step_batched over a made-up distribution: the ll row of a hypothesis is a fixed function of (graph, step, last token)."""

    def __init__(self, pv, tot):
        self.vocabs = {'predictable_token': pv}
        self.tot = tot
        self.banned_seen = 0

    def decode_step_batched(self, tokens, state, memory, beam_of_hyp, offset, topk, banned=None):
        pv, results = self.vocabs['predictable_token'], []
        for h, (w, b) in enumerate(zip(tokens, beam_of_hyp.tolist())):
            local = memory['local_idx2token'][b]
            seed = (sum(ord(c) * (i + 1) for i, c in enumerate(w)) * 131 + offset * 17 + b) % (2 ** 31)
            ll = np.log(np.random.RandomState(seed).dirichlet(np.ones(self.tot) * 0.3) + 1e-12)
            for i in range(pv.size, self.tot):
                if i not in local:
                    ll[i] = NEG_INF                                     # another graph's copy id
            ll[pv.token2idx(PAD)] = ll[pv.token2idx(UNK)] = NEG_INF
            for i in (banned[h] if banned is not None else ()):
                ll[i] = NEG_INF
                self.banned_seen += 1
            order = np.lexsort((np.arange(self.tot), -ll))[:topk]
            results.append([(local[int(i)] if int(i) in local else pv.idx2token(int(i)), float(ll[i])) for i in order])
        return {}, results


def most_seen_and_first_bigram(seq):
    """The avoid entries every end-to-end test takes from a plain best output: its first bigram and its most frequent token."""
    y = [w for w in seq[1:] if w not in (PAD, UNK, STR, END)]
    entries = [y[:2]] if len(y) >= 2 else []
    if y:
        entries.append([collections.Counter(y).most_common(1)[0][0]])
    return entries


def test_host_beam_search_avoids_on_a_fake_model():
    from gtos_amd import synth
    from gtos_amd.search import Beam, beam_search
    pv = synth.SynthVocab(12, [END])
    local = [{12: "c0", 13: "c1"}, {12: "d0", 14: "d2"}, {13: "e1"}]
    memory = {'probe': torch.zeros(1), 'local_idx2token': local}
    k, min_t, max_t = 4, 2, 9
    key = lambda beams: [(b.steps, [(h.seq, h.score) for h in b.hypotheses], [(h.seq, h.score) for h in b.completed_hypotheses]) for b in beams]

    def run(**kw):
        model = FakeModel(pv, 15)
        beams = beam_search(model, [Beam(k, min_t, max_t) for _ in local], memory, **kw)
        return beams, model
    plain, model = run()
    assert not model.banned_seen
    assert key(run(avoid=None)[0]) == key(plain) == key(run(avoid=[[], [], []])[0])
    avoid = [most_seen_and_first_bigram(b.get_k_best(1, 0.6)[0].seq) for b in plain]
    assert all(len(a) == 2 for a in avoid)
    for kw in (dict(), dict(no_repeat_ngram=2)):
        beams, model = run(avoid=avoid, **kw)
        assert model.banned_seen
        for b, beam in enumerate(beams):
            hyps = beam.hypotheses + beam.completed_hypotheses
            assert hyps and all(np.isfinite(h.score) for h in hyps)
            for h in hyps:
                assert not holds_entry(h.seq, avoid[b]), (b, h.seq, avoid[b])
                if kw:
                    y = [w for w in h.seq[1:] if w != END]
                    assert len(set(zip(y, y[1:]))) == max(len(y) - 1, 0), h.seq
        assert key(beams) != key(plain)


# ------------------------------------------------------------------------------------------------ GPU: the kernel
POISON = -7


def _expect(ll, prev, cur, parent, token, t, k, tabs, act):
    """The numpy statement of one gtos_avoid_block launch: (ll, state_cur) after it.  prev / cur: uint64 [N]; tabs: per graph
    (pat, init, last, n_pos)."""
    ll, cur = ll.copy(), cur.copy()
    if not act:
        return ll, cur
    for s in range(ll.shape[0]):
        pat, init, last, n_pos = tabs[s // k]
        if t == 0:
            d = 0
        else:
            p = s if parent is None else int(parent[s])
            if p < 0 or token[s] < 0:
                continue
            mask = sum(1 << i for i in range(n_pos) if pat[i] == token[s])
            d = ((int(prev[p]) << 1 | init) & mask) & M64
        cur[s] = d
        ban = ((d << 1) | init) & last
        for i in range(n_pos):
            if (ban >> i) & 1:
                ll[s, pat[i]] = -np.inf
    return ll, cur


def _gpu_tables(rng, tot, dev):
    """Three graphs with tables of 0, 1 and 64 positions over the ids {0, 7, tot - 1} -> (per-graph tables, device tensors)"""
    from gtos_amd.search import avoid_tables
    alphabet = [0, 7, tot - 1]
    full, left = [], 64
    while left:
        n = min(left, int(rng.choice([1, 1, 2, 2, 3, 5])))
        full.append([alphabet[int(x)] for x in rng.randint(0, 3, size=n)])
        left -= n
    entries = [[], [[alphabet[int(rng.randint(3))]]], full]
    pat, init, last, n_pos = avoid_tables(entries)
    assert n_pos == [0, 1, 64]
    tabs = [(pat[b], unsigned(init[b]), unsigned(last[b]), n_pos[b]) for b in range(3)]
    g = (torch.tensor(pat, dtype=torch.int32).to(dev), torch.tensor(init, dtype=torch.int64).to(dev),
         torch.tensor(last, dtype=torch.int64).to(dev), torch.tensor(n_pos, dtype=torch.int32).to(dev))
    return tabs, g


def _slots(rng, k, N, variant, alphabet):
    token = alphabet[rng.randint(0, 3, size=N)]
    parent = (np.arange(N) // k) * k + rng.randint(0, k, size=N)          # any slot of the same graph
    if k >= 3:
        parent[1] = parent[0]                                              # two children of one parent
        parent[2::4] = -1                                                  # dead slots, interleaved
        token[4::5] = -1
    else:
        parent[1] = -1
        if variant == "beam":
            token[0] = -1
    return parent.astype(np.int32), token.astype(np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("k", [1, 3, 32])
def test_avoid_block_matches_numpy_rule(k):
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(4000 + k)
    B, max_t = 3, 20
    N = B * k
    D = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    launches = bans = 0
    for t in (0, 1, 2, 17):
        for tot in (40, 1000):
            alphabet = np.array([0, 7, tot - 1], dtype=np.int32)         # few ids: matches are frequent; the last column is one
            tabs, g_tabs = _gpu_tables(rng, tot, dev)
            for ld in (tot, tot + 3):
                for variant in ("beam", "sample", "inactive"):
                    prev = rng.randint(0, 2 ** 32, size=N).astype(np.uint64) << np.uint64(32) | rng.randint(0, 2 ** 32, size=N).astype(np.uint64)
                    prev[N - 1] = M64                                       # every position matched, bit 63 included
                    cur = np.full(N, POISON, dtype=np.int64).view(np.uint64)
                    parent, token = _slots(rng, k, N, variant, alphabet)
                    buf = rng.randn(N * ld).astype(np.float32)
                    buf.reshape(N, ld)[:, tot:] = np.nan                   # the stride gap is no column
                    ll = buf.reshape(N, ld)[:, :tot]
                    active = np.zeros(3, dtype=np.int32)
                    active[t % 3] = variant != "inactive"
                    if variant == "sample":                                # parent = NULL, the token row cut from a [max_t, N] table
                        table = rng.randint(0, 3, size=(max_t, N)).astype(np.int32)
                        table[max(t - 1, 0)] = token
                        g_par, g_tok, parent = None, D(table)[max(t - 1, 0)], None
                    else:
                        g_par, g_tok = D(parent), D(token)
                    if t == 0:
                        g_par = g_tok = None                               # step 0 has neither
                    g_buf, g_prev, g_cur, g_act = D(buf), D(prev.view(np.int64)), D(cur.view(np.int64)), D(active)
                    ops.avoid_block(t, k, g_buf.view(N, ld)[:, :tot], g_par, g_tok, *g_tabs, g_prev, g_cur, g_act)
                    want_ll, want_cur = _expect(ll, prev, cur, parent, token, t, k, tabs, variant != "inactive")
                    want_buf = buf.copy()
                    want_buf.reshape(N, ld)[:, :tot] = want_ll
                    what = (t, tot, ld, variant)
                    assert np.array_equal(g_buf.cpu().numpy().view(np.int32), want_buf.view(np.int32)), what      # bit for bit
                    assert np.array_equal(g_cur.cpu().numpy().view(np.uint64), want_cur), what
                    assert np.array_equal(g_prev.cpu().numpy().view(np.uint64), prev) and np.array_equal(g_act.cpu().numpy(), active), what
                    assert not np.isneginf(want_ll[:k]).any(), what          # the graph with the empty table: nothing banned
                    if variant == "inactive":
                        assert np.array_equal(want_buf.view(np.int32), buf.view(np.int32)) and np.array_equal(want_cur, cur)
                    launches += 1
                    bans += int(np.isneginf(want_ll).sum())
    assert launches == 4 * 2 * 2 * 3 and bans > 0, (launches, bans)


@pytest.mark.gpu
@pytest.mark.parametrize("k,t", [(3, 0), (3, 1), (32, 17), (1, 2)])
def test_avoid_block_stores_inside_its_outputs(k, t):
    """ll and both state buffers carved from poisoned allocations: nothing outside ll's columns and the live slots' words changes."""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rng = np.random.RandomState(99 + t)
    B, tot = 3, 40
    N = B * k
    alphabet = np.array([0, 7, tot - 1], dtype=np.int32)
    tabs, g_tabs = _gpu_tables(rng, tot, dev)
    ll0 = torch.from_numpy(rng.randn(N, tot).astype(np.float32))
    g_ll = Guarded(N, tot, torch.float32, dev, ld=tot + 3, init=ll0.to(dev))
    margin = 1024
    state = []
    for fill in (rng.randint(0, 2 ** 62, size=N, dtype=np.int64), np.full(N, POISON, dtype=np.int64)):
        whole = torch.full((2 * margin + N,), POISON - 1, dtype=torch.int64, device=dev)
        view = whole[margin:margin + N]
        view.copy_(torch.from_numpy(fill))
        state.append((whole, view, fill))
    parent, token = _slots(rng, k, N, "beam", alphabet)
    parent[1::3] = -1
    active = np.zeros(3, dtype=np.int32)
    active[t % 3] = 1
    D = lambda a: torch.from_numpy(a).to(dev)
    ops.avoid_block(t, k, g_ll.view, D(parent) if t else None, D(token) if t else None, *g_tabs, state[0][1], state[1][1], D(active))
    g_ll.check("gtos_avoid_block ll")
    want_ll, want_cur = _expect(ll0.numpy(), state[0][2].view(np.uint64), state[1][2].view(np.uint64), parent, token, t, k, tabs, True)
    assert np.array_equal(g_ll.view.contiguous().cpu().numpy().view(np.int32), np.ascontiguousarray(want_ll).view(np.int32))
    for whole, view, fill in state:
        w = whole.cpu().numpy()
        assert (w[:margin] == POISON - 1).all() and (w[margin + N:] == POISON - 1).all()
    assert np.array_equal(state[0][1].cpu().numpy(), state[0][2])
    cur = state[1][1].cpu().numpy()
    assert np.array_equal(cur.view(np.uint64), want_cur)
    dead = (parent < 0) | (token < 0) if t else np.zeros(N, dtype=bool)
    assert (cur[dead] == POISON).all() and (~dead).any() and (t == 0 or dead.any())


# ------------------------------------------------------------------------------------------------ GPU: end to end
def restate_avoiding(O, model, graph, gmask, probe, cp_seq, local, vocabs, k, max_t, min_t, avoid, alpha):
    """The reference's search (oracle.beam_search_sentence: torch.topk, the pool rule) with the avoid rule, stated on the strings, in
    front of the top-k -> (finished, alive, k-best, steps, the smallest selection gap); the construction of
    test_ngram_block.restate_sentence."""
    from test_ngram_block import _gap
    pv = vocabs['predictable_token']
    inv = {w: i for i, w in local.items()}
    words = sorted({p[-1] for p in avoid})
    alive, fin, steps, gap = [([STR], 0.0)], [], 0, float("inf")
    while len(fin) < k and steps < max_t and alive:
        ll = O.next_token_ll(model, graph, gmask, probe, cp_seq, [s for s, _ in alive], vocabs).clone()
        for h, (seq, _) in enumerate(alive):
            for w in brute_avoided(seq[1:], avoid, words):
                ll[h, inv[w] if w in inv else pv.token2idx(w)] = NEG_INF
        top_s, top_i = torch.topk(ll, min(k + 1, ll.shape[1]), 1)
        pool = []
        for h, (seq, score) in enumerate(alive):
            row = top_s[h].tolist()
            if len(row) > k:
                gap = min(gap, _gap(row[k - 1], row[k]))
            for s, i in zip(row[:k], top_i[h].tolist()[:k]):
                word = local[i] if i in local else pv.idx2token(i)
                pool.append((seq + [word], NEG_INF if word == UNK else score + s))
        pool = sorted(pool, key=lambda c: -c[1])
        cut = k - len(fin)
        if 0 < cut < len(pool):
            gap = min(gap, _gap(pool[cut - 1][1], pool[cut][1]))
        alive = []
        for seq, score in pool[:cut]:
            if seq[-1] == END:
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


GOLDEN_SENTENCES = 30      # beam_smatch: 3 runs x 6 sentences, beam_dep_dev: 2 x 6
_left_out = set()


def _oracle_of(case, tmp_path):
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
    return O, ref, vocabs, batch_of(meta, arrs)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["beam_smatch", "beam_dep_dev"])
def test_avoiding_search_matches_the_restatement(case, tmp_path):
    """work(search="device") and work(search="host") avoiding the first bigram and the most frequent token of the plain search's best
    output, at the fixture's own runs, against each other and against the restatement.  A sentence is left out of the exact comparison
    only when one of the restatement's own selection gaps is below test_ngram_block.NEAR (the two searches round differently there);
    test_blocked_search_matches_the_restatement admits one combination in ten for that reason (9 of its 90), and so does this test:
    3 of the 30 (case, run, sentence) combinations of the two cases together."""
    from test_beam_and_vocab import check_hyps
    from test_ngram_block import _golden_model, _pairs, NEAR
    meta, model, batch = _golden_model(case, tmp_path)
    O, ref, vocabs, cpu_batch = _oracle_of(case, tmp_path)
    alpha = meta["cfg"]["alpha"]
    with torch.no_grad():
        graph, gmask, probe = ref.encode_step(cpu_batch, train=False)
    compared = total = 0
    for r, run in enumerate(meta["runs"]):
        k, max_t, min_t = run["beam"], run["max_step"], run["min_step"]
        plain = model.work(batch, k, max_t, min_t, search="device")
        B = len(plain)
        empty = model.work(batch, k, max_t, min_t, search="device", avoid=[[] for _ in range(B)])
        for a, b in zip(plain, empty):
            assert (a.steps, _pairs(a.hypotheses), _pairs(a.completed_hypotheses)) == (b.steps, _pairs(b.hypotheses), _pairs(b.completed_hypotheses))
        best = [beam.get_k_best(1, alpha)[0].seq for beam in plain]
        avoid = [most_seen_and_first_bigram(seq) for seq in best]
        assert any(len(a) == 2 for a in avoid)
        for b, entries in enumerate(avoid):
            assert entries and all(holds_entry(best[b], [p]) for p in entries), (b, entries, best[b])      # not vacuous
        got = {search: model.work(batch, k, max_t, min_t, search=search, avoid=avoid) for search in ("device", "host")}
        with torch.no_grad():
            want = [restate_avoiding(O, ref, graph[:, b:b + 1], gmask[:, b:b + 1], probe[:, b:b + 1], cpu_batch['cp_seq'][:, b:b + 1],
                                     cpu_batch['local_idx2token'][b], vocabs, k, max_t, min_t, avoid[b], alpha) for b in range(B)]
        for b in range(B):
            tag = "%s run %s sentence %d" % (case, (k, max_t, min_t), b)
            fin, alive, kbest, steps, gap = want[b]
            total += 1
            for search, beams in got.items():
                beam = beams[b]
                assert beam.avoid == avoid[b], tag
                for seq, _ in _pairs(beam.completed_hypotheses) + _pairs(beam.hypotheses):
                    assert not holds_entry(seq, avoid[b]), (tag, search, seq, avoid[b])
            d, h = got["device"][b], got["host"][b]
            lists = {s: (_pairs(x.completed_hypotheses), _pairs(x.hypotheses)) for s, x in (("device", d), ("host", h))}      # before get_k_best sorts
            dev_best = _pairs(d.get_k_best(k, alpha))
            assert [list(s) for s, _ in dev_best[:1]] != [list(best[b])], tag
            print("MEASURED %s: smallest selection gap of the restatement %.3e" % (tag, gap))
            if gap < NEAR:
                _left_out.add((case, r, b))
                continue
            compared += 1
            assert d.steps == h.steps == steps, tag
            host_best = _pairs(h.get_k_best(k, alpha))
            check_hyps(dev_best, host_best, tag + " device against host, k-best")
            if fin:
                check_hyps(lists["device"][0], lists["host"][0], tag + " device against host, finished")
                check_hyps(lists["device"][1], lists["host"][1], tag + " device against host, alive")
            for search, kb in (("device", dev_best), ("host", host_best)):
                if fin:
                    check_hyps(lists[search][0], fin, tag + " %s finished" % search)
                    check_hyps(lists[search][1], alive, tag + " %s alive" % search)
                else:
                    check_hyps(kb, sorted(alive, key=lambda c: -(c[1] / ((1 + len(c[0])) ** alpha))), tag + " %s alive" % search)
                check_hyps(kb, kbest, tag + " %s k-best" % search)
    print("MEASURED %s: %d of %d sentences compared exactly; left out so far %s" % (case, compared, total, sorted(_left_out)))
    assert 10 * len(_left_out) <= GOLDEN_SENTENCES, sorted(_left_out)


_small = {}


def gen_small():
    """The small golden generator (tests/golden/gen_small: its weights, its eval batch) with string vocabularies of its sizes, so that
    work() runs on it, and the avoid list of every graph from the plain device search (k = 4): (model, batch, avoid, plain beams, their lists
    as the search left them)."""
    if not _small:
        from conftest import load_golden, sub
        from gtos_amd import synth
        from gtos_amd.generator import Generator
        dev = torch.device("cuda:0")
        g = load_golden("gen_small")
        d, ff, H, gl = [int(v) for v in g["cfg"]]
        vocabs = synth.synth_vocabs(SMALL_VOCAB)
        model = Generator(vocabs, *SMALL_GEN_ARGS, d, ff, H, 0.0, 1, gl, 2, None, dev).to(dev)
        model.load_state_dict(sub(g, "sd/"))
        model.eval()
        batch = {k: v.to(dev) for k, v in sub(g, "ebatch/").items()}
        pv, cp = vocabs['predictable_token'], batch['cp_seq'].cpu()
        batch['local_idx2token'] = [{int(i): "copy%d" % int(i) for i in cp[:, b].tolist() if i >= pv.size} for b in range(cp.shape[1])]
        plain = model.work(batch, SMALL_K, SMALL_T, 1, search="device")
        plain_key = _key(plain)                                         # (get_k_best sorts the lists it ranks)
        avoid = [most_seen_and_first_bigram(beam.get_k_best(1, 0.6)[0].seq) for beam in plain]
        assert all(avoid) and any(len(a) == 2 for a in avoid), avoid
        _small.update(model=model, batch=batch, avoid=avoid, plain=plain, plain_key=plain_key)
    return _small["model"], _small["batch"], _small["avoid"], _small["plain"], _small["plain_key"]


SMALL_K, SMALL_T = 4, 8


def _key(beams):
    return [(b.steps, [(h.seq, h.score) for h in b.hypotheses], [(h.seq, h.score) for h in b.completed_hypotheses]) for b in beams]


def _avoids(beams, avoid):
    n = 0
    for b, beam in enumerate(beams):
        hyps = beam.hypotheses + beam.completed_hypotheses
        assert hyps, b
        for h in hyps:
            assert not holds_entry(h.seq, avoid[b]), (b, h.seq, avoid[b])
            n += 1
    return n


def _free_words(model, batch, avoid, n):
    """Per graph n producible strings that no avoid entry of the graph holds: its copy tokens first, then vocabulary words"""
    pv = model.vocabs['predictable_token']
    words = [pv.idx2token(i) for i in range(pv.size) if pv.idx2token(i) not in (PAD, UNK, STR, END)]
    out = []
    for local, entries in zip(batch['local_idx2token'], avoid):
        used = {w for p in entries for w in p}
        out.append([w for w in [x for _, x in sorted(local.items())] + words if w not in used][:n])
        assert len(out[-1]) == n
    return out


@pytest.mark.gpu
def test_avoid_composes_with_every_device_route():
    from gtos_amd.search import constraints_met, phrase_state
    model, batch, avoid, plain, plain_key = gen_small()
    k, max_t = SMALL_K, SMALL_T
    B = len(avoid)
    none = [[] for _ in range(B)]
    work = lambda **kw: model.work(batch, k, max_t, 1, search="device", **kw)          # noqa: E731
    assert _key(work(avoid=none)) == plain_key == _key(work(avoid=None))
    alone = work(avoid=avoid)
    _avoids(alone, avoid)
    assert all(holds_entry(p.get_k_best(1, 0.6)[0].seq, [e]) for p, a in zip(plain, avoid) for e in a)          # not vacuous
    # repeat-n-gram blocking
    beams = work(avoid=avoid, no_repeat_ngram=2)
    _avoids(beams, avoid)
    for beam in beams:
        for h in beam.hypotheses + beam.completed_hypotheses:
            y = [w for w in h.seq[1:] if w != END]
            assert len(set(zip(y, y[1:]))) == max(len(y) - 1, 0), h.seq
    assert _key(work(avoid=none, no_repeat_ngram=2)) == _key(work(no_repeat_ngram=2))
    # constraints
    free = _free_words(model, batch, avoid, 2)
    cons = [f[:1] for f in free]
    beams = work(avoid=avoid, constraints=cons)
    _avoids(beams, avoid)
    for b, beam in enumerate(beams):
        for h in beam.completed_hypotheses:
            assert constraints_met(h.seq, cons[b]) == len(cons[b]), (b, h.seq)
    assert _key(work(avoid=none, constraints=cons)) == _key(work(constraints=cons))
    # groups, the coverage penalty, phrases
    beams = work(avoid=avoid, groups=2, diversity=0.5)
    assert _avoids(beams, avoid) and all(len(b.groups) == 2 for b in beams)
    assert _key(work(avoid=none, groups=2, diversity=0.5)) == _key(work(groups=2, diversity=0.5))
    beams = work(avoid=avoid, coverage_penalty=0.2)
    assert _avoids(beams, avoid) and all(hasattr(h, "cp") for b in beams for h in b.hypotheses + b.completed_hypotheses)
    assert _key(work(avoid=none, coverage_penalty=0.2)) == _key(work(coverage_penalty=0.2))
    phrases = [[f] for f in free]
    beams = work(avoid=avoid, phrases=phrases)
    _avoids(beams, avoid)
    for b, beam in enumerate(beams):
        for h in beam.completed_hypotheses:
            assert phrase_state(h.seq, phrases[b])[0] == 1, (b, h.seq)
    assert _key(work(avoid=none, phrases=phrases)) == _key(work(phrases=phrases))
    for beams in (alone,):
        assert [b.avoid for b in beams] == avoid


@pytest.mark.gpu
def test_avoiding_device_search_is_independent_of_sync_every(monkeypatch):
    from gtos_amd import search
    from test_sample_decode import _capture_memory
    model, batch, avoid, _, _ = gen_small()
    memory = _capture_memory(model, batch, monkeypatch)
    out = []
    for sync in (1, 8):
        beams = [search.Beam(SMALL_K, 1, SMALL_T) for _ in avoid]
        with torch.no_grad():
            search.beam_search_device(model, memory, beams, sync_every=sync, avoid=avoid)
        out.append(_key(beams))
    assert out[0] == out[1]
    _avoids(beams, avoid)


@pytest.mark.gpu
@pytest.mark.parametrize("T,top_k,top_p", [(1.0, 0, 1.0), (0.7, 5, 0.9)])
def test_avoiding_samples_are_the_plain_sampler_s_on_the_banned_rows(T, top_k, top_p, monkeypatch):
    """search="sample", k = 8, one seed: no sample holds an avoided entry, and every sample is, draw by draw, what the rule of
    csrc/sample_kernels.h (restated with sample_bits: test_sample_decode.np_select) picks on the decoder's ll row with the banned
    columns at -inf.  A slot one of whose draws is a near tie of the restatement is left out of the comparison from there on."""
    from gtos_amd import search
    from test_sample_decode import _capture_memory, _host_decode, _ids_of, _samples, np_select, f32
    model, batch, avoid, _, _ = gen_small()
    k, max_t, min_t, seed = 8, SMALL_T, 2, 20261019
    memory = _capture_memory(model, batch, monkeypatch)
    B = len(avoid)
    beams = model.work(batch, k, max_t, min_t, search="sample", seed=seed, temperature=T, top_k=top_k, top_p=top_p, avoid=avoid)
    assert _avoids(beams, avoid) == B * k and [b.avoid for b in beams] == avoid
    again = model.work(batch, k, max_t, min_t, search="sample", seed=seed, temperature=T, top_k=top_k, top_p=top_p, avoid=avoid)
    assert _key(beams) == _key(again)
    plain = model.work(batch, k, max_t, min_t, search="sample", seed=seed, temperature=T, top_k=top_k, top_p=top_p)
    assert _key(plain) == _key(model.work(batch, k, max_t, min_t, search="sample", seed=seed, temperature=T, top_k=top_k, top_p=top_p,
                                          avoid=[[] for _ in range(B)]))
    print("MEASURED T=%g top_k=%d top_p=%g: %d of %d plain samples hold an avoided entry" % (
        T, top_k, top_p, sum(holds_entry(h.seq, avoid[b]) for b, beam in enumerate(plain) for h in beam.hypotheses + beam.completed_hypotheses), B * k))
    ids = search.avoid_ids(model, memory['local_idx2token'], avoid)
    hist, near, hits = collections.defaultdict(list), set(), [0]

    def choose(s, t, row, allow):
        b, j = divmod(s, k)
        row = row.copy()
        for p in ids[b]:
            if len(p) - 1 <= len(hist[s]) and hist[s][len(hist[s]) - len(p) + 1:] == p[:-1]:
                hits[0] += bool(allow[p[-1]] and np.isfinite(row[p[-1]]))
                row[p[-1]] = -np.inf
        w, tie = np_select(row, allow & np.isfinite(row), f32(T), top_k, f32(top_p), seed, b, j, t)
        if tie:
            near.add(s)
        if w < 0:
            return None
        hist[s].append(w)
        return w
    seqs, scores = _host_decode(model, memory, k, max_t, min_t, choose)
    assert hits[0] > 0                                                   # the rule took allowed columns away
    compared = 0
    for b, beam in enumerate(beams):
        if any(b * k + j in near for j in range(k)):
            continue
        got = sorted((_ids_of(model, memory, b, seq), score) for seq, score in _samples(beam))
        want = sorted((seqs[b * k + j], scores[b * k + j]) for j in range(k))
        assert [g[0] for g in got] == [w[0] for w in want], b
        for (_, a), (_, c) in zip(got, want):
            assert abs(a - c) <= 1e-4 * max(1.0, abs(c)), (b, a, c)
        compared += 1
    print("MEASURED T=%g top_k=%d top_p=%g: %d of %d graphs compared draw by draw, %d slots with a near tie" % (T, top_k, top_p, compared, B, len(near)))
    assert compared >= 1
