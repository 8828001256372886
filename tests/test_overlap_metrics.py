"""BLEU / chrF++ validation (gtos_amd.metrics, Trainer.validate) and the count under it, gtos_ngram_overlap.

The count is integer arithmetic, so everything about it is tested for EQUALITY: the rule header (csrc/overlap_kernels.h, built with g++)
and the kernel (ops.ngram_overlap) against a collections.Counter statement written here.  The scores are tested against what the
reference's own programs printed for tests/golden/metrics_dev48.json (make_golden_metrics.py), to half a unit of the last printed
digit plus 1e-9: 5e-5 for the chrF++ figures (0..100), 5e-3 for BLEU, 0.05 for its precisions, 5e-4 for the brevity penalty; the
lengths must be equal.
"""
import collections
import ctypes
import json
import math
import os
import random
import string

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver, GuardedFlat, SMALL_VOCAB, SMALL_GEN_ARGS

HERE = os.path.dirname(os.path.abspath(__file__))
TOL_CHRF, TOL_BLEU, TOL_PREC, TOL_BP = 5e-5 + 1e-9, 5e-3 + 1e-9, 0.05 + 1e-9, 5e-4 + 1e-9
MAX_SYMBOLS = 4096


# ------------------------------------------------------------------------------------------------ the statement of the rule
def counter_stats(h, r, n_max):
    """[n_max][3] = (clipped matches, hypothesis n-grams, reference n-grams) of two sequences of hashable symbols"""
    out = []
    for n in range(1, n_max + 1):
        ch = collections.Counter(tuple(h[i:i + n]) for i in range(len(h) - n + 1))
        cr = collections.Counter(tuple(r[i:i + n]) for i in range(len(r) - n + 1))
        out.append([sum(min(c, cr[g]) for g, c in ch.items()), max(len(h) - n + 1, 0), max(len(r) - n + 1, 0)])
    return out


def split_punct(words):
    out = []
    for w in words:
        if len(w) > 1 and w[-1] in string.punctuation:
            out += [w[:-1], w[-1]]
        elif len(w) > 1 and w[0] in string.punctuation:
            out += [w[0], w[1:]]
        else:
            out.append(w)
    return out


def symbols_of(words, kind):
    return {"word": list(words), "chrf_word": split_punct(words), "char": list("".join(words).replace(" ", ""))}[kind]


def f_beta(stats, beta=2.0):
    """per order F of [orders][3] statistics, with the 1e-16 substitutions of the definition"""
    out = []
    for m, hn, rn in stats:
        p = m / hn if hn > 0 else 1e-16
        r = m / rn if rn > 0 else 1e-16
        d = beta * beta * p + r
        out.append((1 + beta * beta) * p * r / d if d > 0 else 1e-16)
    return out


def own_chrf(char, word):
    return 100.0 * (sum(f_beta(char)) + sum(f_beta(word))) / (len(char) + len(word))


def own_scores(hyps, refs):
    """The whole definition on the host from the Counter statistics: what Trainer.validate must return for these strings."""
    st = {kind: [counter_stats(symbols_of(h, kind), symbols_of(r, kind), n) for h, r in zip(hyps, refs)]
          for kind, n in (("word", 4), ("chrf_word", 2), ("char", 6))}
    tot = {kind: np.asarray(v, dtype=np.int64).reshape(len(hyps), -1, 3).sum(0) for kind, v in st.items()}
    sent = [own_chrf(c, w) for c, w in zip(st["char"], st["chrf_word"])]
    hyp_len, ref_len = sum(len(h) for h in hyps), sum(len(r) for r in refs)
    prec = [m / t if t else 0.0 for m, t, _ in tot["word"].tolist()]
    bp = math.exp(1 - ref_len / hyp_len) if hyp_len < ref_len else 1.0
    bleu = bp * math.exp(sum(math.log(p) for p in prec) / 4) if all(p > 0 for p in prec) else 0.0
    return {"bleu": 100 * bleu, "bleu_precisions": [100 * p for p in prec], "brevity_penalty": bp,
            "chrf": own_chrf(tot["char"].tolist(), tot["chrf_word"].tolist()), "chrf_avg": sum(sent) / len(sent), "hyp_tokens": hyp_len,
            "ref_tokens": ref_len, "sentences": len(hyps), "sentence": sent}


@pytest.fixture(scope="module")
def golden():
    g = json.load(open(os.path.join(HERE, "golden", "metrics_dev48.json"), encoding="utf-8"))
    assert len(g["hyps"]) == len(g["refs"]) == 48 and min(g["chrf"]["sentence"]) > 0
    g["stats"] = {kind: torch.tensor([counter_stats(symbols_of(h, kind), symbols_of(r, kind), n) for h, r in zip(g["hyps"], g["refs"])],
                                     dtype=torch.int32) for kind, n in (("word", 4), ("chrf_word", 2), ("char", 6))}
    return g


def check_against_recorded(g, b, c, sent):
    print("MEASURED bleu %.6f precisions %s bp %.6f lengths %d %d | chrF++ F %.6f avgF %.6f | max sentence deviation %.2e" % (
        float(b["bleu"]), [round(float(p), 4) for p in b["precisions"]], float(b["brevity_penalty"]), int(b["hyp_len"]),
        int(b["ref_len"]), float(c["F"]), float(c["avgF"]), max(abs(float(x) - y) for x, y in zip(sent, g["chrf"]["sentence"]))))
    assert abs(float(b["bleu"]) - g["bleu"]["bleu"]) <= TOL_BLEU
    for got, want in zip(b["precisions"].tolist(), g["bleu"]["precisions"]):
        assert abs(got - want) <= TOL_PREC
    assert abs(float(b["brevity_penalty"]) - g["bleu"]["bp"]) <= TOL_BP
    assert int(b["hyp_len"]) == g["bleu"]["hyp_len"] and int(b["ref_len"]) == g["bleu"]["ref_len"]
    assert abs(float(c["F"]) - g["chrf"]["F"]) <= TOL_CHRF and abs(float(c["avgF"]) - g["chrf"]["avgF"]) <= TOL_CHRF
    for got, want in zip(sent.tolist(), g["chrf"]["sentence"]):
        assert abs(got - want) <= TOL_CHRF


# ------------------------------------------------------------------------------------------------ CPU: the rule header
DRIVER = r"""
#include "overlap_kernels.h"
extern "C" void serial(const int* h, int Lh, const int* r, int Lr, int n_max, int* out) {
    gtos_overlap::overlap_serial(h, Lh, r, Lr, n_max, out);
}
extern "C" int check(const int* off, int R, const int* pairs, int P, int n_max) { return gtos_overlap::check_launch(off, R, pairs, P, n_max); }
extern "C" int max_symbols() { return gtos_overlap::MAX_SYMBOLS; }
extern "C" int max_order() { return gtos_overlap::MAX_ORDER; }
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    return compile_host_driver(tmp_path_factory, "overlap", DRIVER)


def serial_stats(lib, h, r, n_max):
    out = np.full(n_max * 3 + 2, -7, dtype=np.int32)
    ha, ra = np.asarray(h, dtype=np.int32), np.asarray(r, dtype=np.int32)
    lib.serial(ha.ctypes.data_as(ctypes.c_void_p), len(h), ra.ctypes.data_as(ctypes.c_void_p), len(r), n_max,
               out.ctypes.data_as(ctypes.c_void_p))
    assert out[-1] == -7 and out[-2] == -7
    return out[:-2].reshape(n_max, 3).tolist()


def test_rule_header_matches_the_counter_statement(host_lib):
    assert host_lib.max_symbols() == MAX_SYMBOLS and host_lib.max_order() == 8
    rng = random.Random(3)
    cases = 0
    for n_max in (1, 4, 6, 8):
        for alphabet in (2, 5, 1000):
            lengths = [0, 1, n_max - 1, n_max, n_max + 1, 17, 64, 300]
            pairs = [(a, b) for a in lengths for b in (0, 1, n_max, n_max + 1)] + [(rng.randrange(301), rng.randrange(301)) for _ in range(12)]
            pairs += [(300, 300), (0, 0)]
            for lh, lr in pairs:
                h = [rng.randrange(alphabet) for _ in range(lh)]
                r = [rng.randrange(alphabet) for _ in range(lr)]
                if rng.random() < 0.3 and lr:                       # a reference that shares long stretches with the hypothesis
                    r = (h[lh // 3:] + r)[:lr]
                assert serial_stats(host_lib, h, r, n_max) == counter_stats(h, r, n_max), (n_max, alphabet, lh, lr)
                cases += 1
            h = [rng.randrange(alphabet) for _ in range(40)]
            assert serial_stats(host_lib, h, h, n_max) == counter_stats(h, h, n_max)
    assert cases > 500


def test_launch_check_of_the_rule_header(host_lib):
    def check(off, pairs, n_max):
        o, p = np.asarray(off, dtype=np.int32), np.asarray(pairs, dtype=np.int32).reshape(-1, 2)
        return host_lib.check(o.ctypes.data_as(ctypes.c_void_p), len(off) - 1, p.ctypes.data_as(ctypes.c_void_p), len(p), n_max)
    assert check([0, 3, 3, 3 + MAX_SYMBOLS], [(0, 1), (2, 2), (1, 0)], 8) == 0
    assert check([0, 3, 3, 4 + MAX_SYMBOLS], [(0, 1)], 4) == -10            # a row of MAX_SYMBOLS + 1
    assert check([0, 3, 2], [(0, 1)], 4) == -10                              # offsets that go down
    assert check([0, 3, 5], [(0, 2)], 4) == -10 and check([0, 3, 5], [(-1, 0)], 4) == -10
    assert check([0, 3, 5], [(0, 1)], 0) == -10 and check([0, 3, 5], [(0, 1)], 9) == -10
    assert check([0], [], 1) == 0


def test_entry_point_refuses_bad_arguments():
    """-10 outside the shapes, nothing launched (fake device pointers are never dereferenced); P == 0 is success."""
    from gtos_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 35
    p = ctypes.c_void_p(16)
    off = np.asarray([0, 2, 5, 5 + MAX_SYMBOLS], dtype=np.int32)
    long_off = np.asarray([0, 2, 5, 6 + MAX_SYMBOLS], dtype=np.int32)
    pairs = np.asarray([[0, 1], [2, 2]], dtype=np.int32)
    bad_pairs = np.asarray([[0, 1], [2, 3]], dtype=np.int32)

    def call(sym=p, off_d=p, R=3, pairs_d=p, P=2, n_max=4, off_h=off, pairs_h=pairs, out=p):
        host = lambda a: None if a is None else a.ctypes.data_as(ctypes.c_void_p)        # noqa: E731
        return lib.gtos_ngram_overlap(sym, off_d, R, pairs_d, P, n_max, host(off_h), host(pairs_h), out, None)
    assert call(n_max=0) == -10 and call(n_max=9) == -10
    assert call(off_h=long_off) == -10
    assert call(pairs_h=bad_pairs) == -10
    assert call(P=-1) == -10 and call(R=-1) == -10
    for name in ("sym", "off_d", "pairs_d", "out", "off_h", "pairs_h"):
        assert call(**{name: None}) == -10, name
    assert call(P=0) == 0 and call(P=0, pairs_d=None, pairs_h=None, out=None) == 0


# ------------------------------------------------------------------------------------------------ CPU: metrics on host tensors
def test_encode():
    from gtos_amd import metrics
    sep = metrics.separate_punctuation
    assert sep(["word."]) == ["word", "."] and sep([".word"]) == [".", "word"] and sep(["."]) == ["."]
    assert sep(["a."]) == ["a", "."] and sep(["..."]) == ["..", "."] and sep(["(a)"]) == ["(a", ")"] and sep(["don't"]) == ["don't"]
    for words in (["Hello,", "world", "(again)", "..."], []):
        assert sep(words) == split_punct(words)
    sents = [["the", "cat", "sat."], ["the", "dog"], [], ["sat.", "the"]]
    sym, off = metrics.encode(sents, "word")
    assert sym.dtype == torch.int32 and off.dtype == torch.int32 and off.tolist() == [0, 3, 5, 5, 7]
    s = sym.tolist()
    assert s[0] == s[3] == s[6] and s[2] == s[5] and len(set(s)) == 4                     # one id table for the whole call
    sym, off = metrics.encode(sents, "chrf_word")
    assert off.tolist() == [0, 4, 6, 6, 9]
    s = sym.tolist()
    assert s[2] == s[6] and s[3] == s[7] and s[0] == s[8]
    sym, off = metrics.encode([["ab", "c d"], ["é"]], "char")
    assert sym.tolist() == [ord("a"), ord("b"), ord("c"), ord("d"), ord("é")] and off.tolist() == [0, 4, 5]
    # an <UNK> is a symbol of its own at every occurrence
    for kind in ("word", "chrf_word", "char"):
        sym, off = metrics.encode([["<UNK>", "a"], ["<UNK>", "<UNK>"]], kind)
        s = sym.tolist()
        assert off.tolist() == [0, 2, 4] and len({s[0], s[2], s[3]}) == 3 and s[1] not in (s[0], s[2], s[3])
    with pytest.raises(ValueError):
        metrics.encode([["a"]], "bpe")
    with pytest.raises(ValueError):
        metrics.encode(["a sentence as one string"], "word")


def test_scores_on_host_tensors_match_the_recorded_results(golden):
    from gtos_amd import metrics
    st = golden["stats"]
    b = metrics.bleu(st["word"], golden["bleu"]["hyp_len"], golden["bleu"]["ref_len"])
    c = metrics.chrf(st["char"], st["chrf_word"])
    sent = metrics.sentence_chrf(st["char"], st["chrf_word"])
    assert sent.dtype == torch.float64 and sent.shape == (48,) and b["bleu"].dtype == torch.float64
    check_against_recorded(golden, b, c, sent)
    b2 = metrics.bleu(st["word"].sum(0))                                # summed statistics, lengths from the unigram totals
    assert float(b2["bleu"]) == float(b["bleu"]) and int(b2["hyp_len"]) == 1072 and int(b2["ref_len"]) == 1157
    own = own_scores(golden["hyps"], golden["refs"])
    assert abs(own["bleu"] - float(b["bleu"])) < 1e-9 and abs(own["chrf"] - float(c["F"])) < 1e-9
    assert abs(own["chrf_avg"] - float(c["avgF"])) < 1e-9
    # ... and the totals route of Trainer.validate gives the same dict
    tot = metrics.accumulate(torch.zeros(metrics.N_TOTALS, dtype=torch.float64), st["word"], st["chrf_word"], st["char"])
    v = metrics.validation_metrics(tot.tolist())
    for key in ("bleu", "brevity_penalty", "chrf", "chrf_avg"):
        assert abs(v[key] - own[key]) < 1e-9, key
    assert (v["hyp_tokens"], v["ref_tokens"], v["sentences"]) == (1072, 1157, 48)


def test_degenerate_pairs_follow_the_definition():
    from gtos_amd import metrics

    def stats(h, r):
        return {kind: torch.tensor([counter_stats(symbols_of(h, kind), symbols_of(r, kind), n)], dtype=torch.int32)
                for kind, n in (("word", 4), ("chrf_word", 2), ("char", 6))}
    # no overlap at all: every precision and recall is 0, every F 0 (the denominator is 0 -> 1e-16), BLEU 0
    st = stats(["aa", "bb", "cc", "dd", "ee"], ["xx", "yy", "zz", "ww", "vv"])
    assert float(metrics.sentence_chrf(st["char"], st["chrf_word"])[0]) == pytest.approx(100 * 1e-16, rel=1e-12)
    assert float(metrics.bleu(st["word"])["bleu"]) == 0.0
    # an empty hypothesis: precision 1e-16 (no hypothesis n-grams), recall 0 -> F 0 exactly; BLEU 0, BP exp(1 - ref / max(hyp, 1))
    st = stats([], ["xx", "yy", "zz", "ww", "vv"])
    assert float(metrics.sentence_chrf(st["char"], st["chrf_word"])[0]) == 0.0
    b = metrics.bleu(st["word"])
    assert float(b["bleu"]) == 0.0 and int(b["hyp_len"]) == 0 and int(b["ref_len"]) == 5 and math.isfinite(float(b["brevity_penalty"]))
    # an empty reference: recall 1e-16, precision 0 -> F 0 exactly
    st = stats(["xxx", "yyy"], [])
    assert float(metrics.sentence_chrf(st["char"], st["chrf_word"])[0]) == 0.0
    assert float(metrics.bleu(st["word"])["bleu"]) == 0.0
    # both empty: precision = recall = 1e-16 -> F = 1e-16 per order
    st = stats([], [])
    assert float(metrics.sentence_chrf(st["char"], st["chrf_word"])[0]) == pytest.approx(100 * 1e-16, rel=1e-12)
    # a short perfect match: the orders the pair is too short for hold 1e-16, BLEU is 0 (no 4-gram)
    st = stats(["ab"], ["ab"])
    assert float(metrics.sentence_chrf(st["char"], st["chrf_word"])[0]) == pytest.approx(100 * (2 + 1 + 5e-16) / 8, rel=1e-12)
    assert float(metrics.bleu(st["word"])["bleu"]) == 0.0
    # a perfect match of five words: everything 100
    st = stats(["a1", "b2", "c3", "d4", "e5"], ["a1", "b2", "c3", "d4", "e5"])
    assert float(metrics.bleu(st["word"])["bleu"]) == pytest.approx(100.0, rel=1e-12)
    assert float(metrics.chrf(st["char"], st["chrf_word"])["F"]) == pytest.approx(100.0, rel=1e-12)
    assert math.isnan(metrics.validation_metrics([0.0] * metrics.N_TOTALS)["bleu"])


def test_ops_ngram_overlap_refuses_cpu_symbols():
    from gtos_amd import ops, _lib
    with pytest.raises(_lib.GtosHipError):
        ops.ngram_overlap(torch.zeros(3, dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32), torch.zeros((1, 2), dtype=torch.int32), 4)


# ------------------------------------------------------------------------------------------------ GPU: the kernel
def csr(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r))
    return torch.tensor([s for r in rows for s in r], dtype=torch.int32), torch.tensor(off, dtype=torch.int32)


def kernel_rows():
    rng = random.Random(11)
    rnd = lambda n, a: [rng.randrange(a) for _ in range(n)]         # noqa: E731
    rows = [[], rnd(1, 3), rnd(3, 3), rnd(4, 3), rnd(5, 3), rnd(7, 2), rnd(8, 2), rnd(9, 2),           # 0-7: around the orders 4 and 8
            rnd(255, 6), rnd(256, 6), rnd(257, 6), rnd(700, 6),                                           # 8-11: the thread stride wraps
            rnd(300, 2), rnd(300, 2),                                                                     # 12-13: heavy clipping
            rnd(MAX_SYMBOLS, 40), rnd(1, 40),                                                             # 14-15
            rnd(120, 1000)]                                                                               # 16: hardly a repeat
    rows.append(rows[11][200:650] + rnd(50, 6))                                                           # 17: long stretches of row 11
    pairs = [(0, 0), (0, 4), (4, 0), (1, 1), (1, 2), (2, 3), (3, 4), (4, 3), (5, 6), (6, 7), (7, 5), (7, 7),
             (8, 9), (9, 10), (10, 8), (11, 17), (17, 11), (11, 10), (12, 13), (13, 12), (12, 12), (14, 15), (15, 14),
             (16, 11), (11, 11), (3, 4), (0, 0), (12, 13), (2, 3)]                                        # repeats, not sorted
    return rows, pairs


@pytest.mark.gpu
@pytest.mark.parametrize("n_max", [1, 4, 6, 8])
def test_kernel_equals_the_counter_statement_inside_guard_bands(n_max):
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rows, pairs = kernel_rows()
    sym, off = csr(rows)
    pt = torch.tensor(pairs, dtype=torch.int32)
    want = torch.tensor([counter_stats(rows[a], rows[b], n_max) for a, b in pairs], dtype=torch.int32)
    got = ops.ngram_overlap(sym.to(dev), off, pt, n_max)
    assert got.dtype == torch.int32 and got.shape == (len(pairs), n_max, 3)
    assert torch.equal(got.cpu(), want)
    # sentinel rows in front of and behind the output stay untouched
    gi = GuardedFlat(len(pairs) * n_max * 3, torch.float32, dev)
    out = gi.view.view(torch.int32)
    ops.ngram_overlap_into(sym.to(dev), off, pt, n_max, out)
    gi.check("gtos_ngram_overlap n_max %d" % n_max)
    assert torch.equal(out.cpu().view(len(pairs), n_max, 3), want)
    # P = 1 and P = 0
    one = ops.ngram_overlap(sym.to(dev), off, pt[18:19], n_max)
    assert torch.equal(one.cpu(), want[18:19])
    none = ops.ngram_overlap(sym.to(dev), off, pt[:0], n_max)
    assert none.shape == (0, n_max, 3)
    empty = ops.ngram_overlap(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(3, dtype=torch.int32),
                              torch.tensor([[0, 1], [1, 1]], dtype=torch.int32), n_max)
    assert torch.equal(empty.cpu(), torch.zeros((2, n_max, 3), dtype=torch.int32))


@pytest.mark.gpu
def test_bad_launches_raise_and_leave_the_output_unwritten():
    from gtos_amd import ops, _lib
    dev = torch.device("cuda:0")
    rows = [[1, 2, 3], [1] * (MAX_SYMBOLS + 1), [2, 3]]
    sym, off = csr(rows)
    ok_sym, ok_off = csr([[1, 2, 3], [2, 3], [3]])
    pairs = torch.tensor([[0, 2], [2, 0]], dtype=torch.int32)
    g = GuardedFlat(0, torch.float32, dev, lead=64, trail=64)
    # (the outputs handed in below lie INSIDE the band: any store shows)
    cases = [(sym, off, pairs, 4), (ok_sym, ok_off, pairs, 0), (ok_sym, ok_off, pairs, 9),
             (ok_sym, ok_off, torch.tensor([[0, 3], [1, 1]], dtype=torch.int32), 4)]
    for s, o, p, n in cases:
        with pytest.raises(_lib.GtosHipError):
            ops.ngram_overlap(s.to(dev), o, p, n)
        with pytest.raises(_lib.GtosHipError):
            ops.ngram_overlap_into(s.to(dev), o, p, n, g.buf[32:32 + 2 * n * 3].view(torch.int32))
    with pytest.raises(_lib.GtosHipError):
        ops.ngram_overlap(ok_sym.to(dev), ok_off.to(dev), pairs, 4)                 # off and pairs are host tensors
    g.check("a refused gtos_ngram_overlap")


@pytest.mark.gpu
def test_fixture_end_to_end_on_the_device(golden):
    from gtos_amd import metrics
    dev = torch.device("cuda:0")
    st = {kind: metrics.overlap(golden["hyps"], golden["refs"], None, kind, device=dev) for kind in ("word", "chrf_word", "char")}
    for kind, v in st.items():
        assert v.is_cuda and torch.equal(v.cpu(), golden["stats"][kind]), kind
    b = metrics.bleu(st["word"], golden["bleu"]["hyp_len"], golden["bleu"]["ref_len"])
    c = metrics.chrf(st["char"], st["chrf_word"])
    sent = metrics.sentence_chrf(st["char"], st["chrf_word"])
    assert sent.is_cuda and sent.dtype == torch.float64 and b["bleu"].is_cuda and c["F"].is_cuda
    check_against_recorded(golden, b, c, sent.cpu())
    # any pair list: every hypothesis against reference 5, and a reversed list
    pairs = [(i, 5) for i in range(47, -1, -1)]
    got = metrics.overlap(golden["hyps"], golden["refs"], pairs, "char", device=dev)
    want = torch.tensor([counter_stats(symbols_of(golden["hyps"][i], "char"), symbols_of(golden["refs"][5], "char"), 6) for i, _ in pairs],
                        dtype=torch.int32)
    assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------------------------------------ GPU: the n-best selection and Trainer.validate
SMALL_K, SMALL_T = 4, 8
_small = {}


def gen_small():
    """A fresh small golden generator (tests/golden/gen_small) with string vocabularies, its eval batch and the batch with the graphs
    in another order: (model, [batch, batch2], d)."""
    from conftest import load_golden, sub
    from gtos_amd import synth
    from gtos_amd.generator import Generator
    dev = torch.device("cuda:0")
    g = _small.setdefault("g", load_golden("gen_small"))
    d, ff, H, gl = [int(v) for v in g["cfg"]]
    vocabs = synth.synth_vocabs(SMALL_VOCAB)
    model = Generator(vocabs, *SMALL_GEN_ARGS, d, ff, H, 0.0, 1, gl, 2, None, dev).to(dev)
    model.load_state_dict(sub(g, "sd/"))
    model.eval()
    batch = {k: v.to(dev) for k, v in sub(g, "ebatch/").items()}
    pv, cp = vocabs['predictable_token'], batch['cp_seq'].cpu()
    batch['local_idx2token'] = [{int(i): "copy%d" % int(i) for i in cp[:, b].tolist() if i >= pv.size} for b in range(cp.shape[1])]
    perm = torch.tensor([2, 0, 1], device=dev)
    axis = {"concept": 1, "concept_char": 1, "concept_depth": 1, "relation": 2, "token_in": 1, "token_char_in": 1, "token_out": 1, "cp_seq": 1}
    batch2 = {k: (v.index_select(axis[k], perm).contiguous() if k in axis else v) for k, v in batch.items() if k != 'local_idx2token'}
    batch2['local_idx2token'] = [batch['local_idx2token'][i] for i in perm.tolist()]
    train = {k: v.to(dev) for k, v in sub(g, "batch/").items()}
    return model, [batch, batch2], d, train


def strip(h):
    seq = h.seq[1:]
    return seq[:-1] if seq and seq[-1] == "<END>" else seq


def true_references(model, batch):
    pv = model.vocabs['predictable_token']
    out = []
    for b, local in enumerate(batch['local_idx2token']):
        words = [local[y] if y in local else pv.idx2token(y) for y in batch['token_out'][:, b].tolist()]
        out.append([w for w in words if w not in ("<END>", "<PAD>")])
    return out


@pytest.mark.gpu
def test_best_of_nbest_is_the_argmax_of_the_sentence_scores():
    from gtos_amd import metrics
    model, (batch, _), _, _ = gen_small()
    refs = true_references(model, batch)
    beams = model.work(batch, SMALL_K, SMALL_T, 1, search="device")
    got = metrics.best_of_nbest(beams, refs, alpha=0.6)
    beams = model.work(batch, SMALL_K, SMALL_T, 1, search="device")
    assert len(got) == len(beams) == 3
    seen = 0
    for (tokens, index, score), beam, ref in zip(got, beams, refs):
        lists = [strip(h) for h in beam.get_k_best(SMALL_K, 0.6)]
        scores = [own_chrf(counter_stats(symbols_of(h, "char"), symbols_of(ref, "char"), 6),
                           counter_stats(symbols_of(h, "chrf_word"), symbols_of(ref, "chrf_word"), 2)) for h in lists]
        best = max(range(len(lists)), key=lambda j: (scores[j], -j))
        assert index == best and tokens == lists[best] and abs(score - scores[best]) < 1e-9
        seen += len(lists)
    assert seen > 3
    short = metrics.best_of_nbest(beams, refs, k=1)
    assert [i for _, i, _ in short] == [0, 0, 0]


def _bits(t):
    return t.detach().clone().view(torch.int32)


@pytest.mark.gpu
def test_validate_matches_the_host_computation_and_leaves_the_trainer_alone(monkeypatch):
    from gtos_amd import ops
    from gtos_amd.train import Trainer
    model, batches, d, train_batch = gen_small()
    trainer = Trainer(model, d, warmup_steps=10)
    model.train()
    trainer.step(train_batch)                                           # a trainer in mid-training: moments and counters are not zero
    torch.cuda.synchronize()
    flat = trainer.flat
    before = [_bits(flat.param), _bits(flat.m), _bits(flat.v), _bits(flat.grad), trainer._state.clone(), trainer.steps_issued]
    seed_before = ops._seed_state[0]

    # host reads, counted on device tensors: validate adds exactly one to those of its searches
    reads, inside = [0], []
    for name in ("tolist", "item", "cpu", "numpy", "__int__", "__float__", "__bool__", "__index__"):
        orig = getattr(torch.Tensor, name)

        def counted(self, *a, _orig=orig, **k):
            if self.is_cuda and not inside:
                reads[0] += 1
                inside.append(1)                                        # (a read that is built on another one counts once)
                try:
                    return _orig(self, *a, **k)
                finally:
                    inside.pop()
            return _orig(self, *a, **k)
        monkeypatch.setattr(torch.Tensor, name, counted)

    for options in (dict(search="device"), dict(search="host", no_repeat_ngram=2)):
        model.eval()
        reads[0] = 0
        outs = [[strip(b.get_k_best(1, 0.6)[0]) for b in model.work(batch, SMALL_K, SMALL_T, 1, **options)] for batch in batches]
        search_reads = reads[0]
        model.train()
        refs = [true_references(model, batch) for batch in batches]
        own = own_scores(outs[0] + outs[1], refs[0] + refs[1])
        reads[0] = 0
        got = trainer.validate(batches, None, beam_size=SMALL_K, alpha=0.6, max_time_step=SMALL_T, min_time_step=1, return_outputs=True,
                               **options)
        assert reads[0] == search_reads + 1, (reads[0], search_reads)
        assert got["outputs"] == outs[0] + outs[1]
        print("MEASURED validate %s: %s" % (options, {k: v for k, v in got.items() if k != "outputs"}))
        for key in ("bleu", "brevity_penalty", "chrf", "chrf_avg"):
            assert abs(got[key] - own[key]) < 1e-9, (key, got[key], own[key])
        assert all(abs(a - b) < 1e-9 for a, b in zip(got["bleu_precisions"], own["bleu_precisions"]))
        assert (got["hyp_tokens"], got["ref_tokens"], got["sentences"]) == (own["hyp_tokens"], own["ref_tokens"], 6)
        assert model.training
        # the true strings as references: the same result (nothing is <UNK> in this batch)
        assert not any(w == "<UNK>" for r in refs for s in r for w in s)
        given = trainer.validate(batches, refs, beam_size=SMALL_K, alpha=0.6, max_time_step=SMALL_T, **options)
        assert given == {k: v for k, v in got.items() if k != "outputs"}
        if "no_repeat_ngram" in options:
            for sent in got["outputs"]:
                grams = [tuple(sent[i:i + 2]) for i in range(len(sent) - 1)]
                assert len(grams) == len(set(grams)), sent              # the option reached the search
    monkeypatch.undo()
    torch.cuda.synchronize()
    after = [_bits(flat.param), _bits(flat.m), _bits(flat.v), _bits(flat.grad), trainer._state.clone(), trainer.steps_issued]
    for a, b, what in zip(before, after, ("parameters", "Adam m", "Adam v", "gradient bucket", "counters")):
        assert torch.equal(a, b), what + " changed under validate"
    assert before[5] == after[5]
    assert ops._seed_state[0] == seed_before                            # (a beam search draws no seed)
    model.eval()
    with pytest.raises(ValueError):
        trainer.validate(batches, [[["a"]], [["a"]]], beam_size=SMALL_K, max_time_step=SMALL_T)
