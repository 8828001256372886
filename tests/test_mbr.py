"""Minimum-Bayes-risk selection (gtos_amd.metrics.pairwise / expected_utility / mbr_select, Trainer.validate(select="mbr")) and the
count under it, gtos_ngram_overlap_groups: all ordered pairs inside groups of candidates.

The count is integer arithmetic, so everything about it is tested for EQUALITY: the rule header (csrc/mbr_kernels.h, built with g++)
and the kernel (ops.ngram_overlap_groups) against a collections.Counter statement written here, and against the pair-list kernel.
The fp64 weighting is tested against a plain Python statement of chrF++ and of the expectation, to 1e-9 (both sides are a few dozen
fp64 operations on numbers of at most 100: their rounding differs by some 1e-13).
"""
import collections
import ctypes
import math
import random
import string

import numpy as np
import pytest
import torch

from tests_support import compile_host_driver, GuardedFlat, SMALL_VOCAB, SMALL_GEN_ARGS

MAX_GROUP, GROUP_MAX_SYMBOLS, MAX_ORDER, MAX_OUT = 64, 1024, 8, 2 ** 31 - 1
TOL = 1e-9


# ------------------------------------------------------------------------------------------------ the statements
def counter_stats(h, r, n_max):
    """[n_max][3] = (clipped matches, hypothesis n-grams, reference n-grams) of two sequences of hashable symbols"""
    out = []
    for n in range(1, n_max + 1):
        ch = collections.Counter(tuple(h[i:i + n]) for i in range(len(h) - n + 1))
        cr = collections.Counter(tuple(r[i:i + n]) for i in range(len(r) - n + 1))
        out.append([sum(min(c, cr[g]) for g, c in ch.items()), max(len(h) - n + 1, 0), max(len(r) - n + 1, 0)])
    return out


def group_cells(rows, sizes, n_max):
    """The whole output of a grouped launch: per group every (hypothesis i, reference j), i-major -> [cells][n_max][3]"""
    out, start = [], 0
    for n in sizes:
        out += [counter_stats(rows[start + i], rows[start + j], n_max) for i in range(n) for j in range(n)]
        start += n
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
    out = []
    for m, hn, rn in stats:
        p = m / hn if hn > 0 else 1e-16
        r = m / rn if rn > 0 else 1e-16
        d = beta * beta * p + r
        out.append((1 + beta * beta) * p * r / d if d > 0 else 1e-16)
    return out


def own_chrf(char, word):
    return 100.0 * (sum(f_beta(char)) + sum(f_beta(word))) / (len(char) + len(word))


def sentence_chrf(h, r):
    """chrF++ of two token-string lists"""
    return own_chrf(counter_stats(symbols_of(h, "char"), symbols_of(r, "char"), 6),
                    counter_stats(symbols_of(h, "chrf_word"), symbols_of(r, "chrf_word"), 2))


def own_expectation(U, w=None):
    """U [n][n] -> (values, index of the first maximum or -1): value_i = sum_j w_j U[i][j] / sum_j w_j; weights that sum to 0: uniform"""
    n = len(U)
    w = [1.0] * n if w is None or sum(w) == 0 else list(w)
    values = [sum(w[j] * U[i][j] for j in range(n)) / sum(w) for i in range(n)]
    return values, (max(range(n), key=lambda i: (values[i], -i)) if n else -1)


def own_mbr(cands, w=None):
    return own_expectation([[sentence_chrf(a, b) for b in cands] for a in cands], w)


def own_scores(hyps, refs):
    """BLEU and chrF++ of a corpus from the Counter statistics: what Trainer.validate must return for these strings."""
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
            "ref_tokens": ref_len, "sentences": len(hyps)}


def csr(rows):
    off = [0]
    for r in rows:
        off.append(off[-1] + len(r))
    return torch.tensor([s for r in rows for s in r], dtype=torch.int32), torch.tensor(off, dtype=torch.int32)


def offsets(sizes):
    out = [0]
    for n in sizes:
        out.append(out[-1] + n)
    return out


# ------------------------------------------------------------------------------------------------ CPU: the rule header
DRIVER = r"""
#include "mbr_kernels.h"
using namespace gtos_mbr;
extern "C" void serial(const int* sym, const int* off, int row0, int n, int n_max, int* cells) { group_serial(sym, off, row0, n, n_max, cells); }
extern "C" void split(const int* h, int Lh, const int* r, int Lr, int n_max, int i, int* counts) {
    int e[MAX_ORDER], in[MAX_ORDER], c[MAX_ORDER];
    earlier_counts(h, Lh, n_max, i, e);
    inref_counts(h, Lh, r, Lr, n_max, i, in);
    position_matches(Lh, n_max, i, e, in, c);
    for (int n = 0; n < MAX_ORDER; ++n) counts[n] = c[n];
}
extern "C" void whole(const int* h, int Lh, const int* r, int Lr, int n_max, int i, int* counts) {
    int c[MAX_ORDER];
    gtos_overlap::position_counts(h, Lh, r, Lr, n_max, i, c);
    for (int n = 0; n < MAX_ORDER; ++n) counts[n] = c[n];
}
// owners[i * n + j] += 1 for every cell a candidate stores
extern "C" void schedule(int n, int* owners, int* scans) {
    for (int i = 0; i < n; ++i) {
        owners[i * n + i] += 1;
        scans[i] = scan_count(i, n);
        for (int k = 0; k < scan_count(i, n); ++k) {
            const int j = scan_ref(i, n, k);
            owners[i * n + j] += 1;
            owners[j * n + i] += 1;
        }
    }
}
extern "C" int check(const int* off, int R, const int* grp, int G, int n_max) { return check_groups(off, R, grp, G, n_max); }
extern "C" void cells_of(const int* grp, int G, long long* cell_off) {
    static_assert(sizeof(long long) == sizeof(int64_t), "");
    cell_offsets(grp, G, reinterpret_cast<int64_t*>(cell_off));
}
extern "C" int max_group() { return MAX_GROUP; }
extern "C" int max_symbols() { return GROUP_MAX_SYMBOLS; }
extern "C" long long max_out() { return MAX_OUT; }
"""


@pytest.fixture(scope="module")
def host_lib(tmp_path_factory):
    lib = compile_host_driver(tmp_path_factory, "mbr", DRIVER)
    lib.max_out.restype = ctypes.c_longlong
    return lib


def vp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def serial_cells(lib, rows, n_max):
    sym, off = (t.numpy() for t in csr(rows))
    sym = np.concatenate([sym, np.zeros(1, dtype=np.int32)])
    n = len(rows)
    out = np.full(n * n * n_max * 3 + 2, -7, dtype=np.int32)
    lib.serial(vp(sym), vp(off), 0, n, n_max, vp(out))
    assert out[-1] == -7 and out[-2] == -7
    return out[:-2].reshape(n * n, n_max, 3).tolist()


def random_group(rng, n, alphabet, n_max):
    """n rows with an empty row, two identical rows and rows that share long stretches among them (where n allows)"""
    lengths = [0, 1, n_max - 1, n_max, n_max + 1, 17, 40, 64]
    rows = [[rng.randrange(alphabet) for _ in range(rng.choice(lengths) if rng.random() < 0.5 else rng.randrange(50))] for _ in range(n)]
    if n >= 2:
        rows[rng.randrange(n)] = []
    if n >= 3:
        a, b = rng.sample(range(n), 2)
        rows[a] = [rng.randrange(alphabet) for _ in range(30)]
        rows[b] = list(rows[a])
    if n >= 5:
        a, b = rng.sample(range(n), 2)
        rows[a] = [rng.randrange(alphabet) for _ in range(45)]
        rows[b] = rows[a][12:] + [rng.randrange(alphabet) for _ in range(9)]
    return rows


def test_group_serial_matches_the_counter_statement(host_lib):
    assert (host_lib.max_group(), host_lib.max_symbols(), host_lib.max_out()) == (MAX_GROUP, GROUP_MAX_SYMBOLS, MAX_OUT)
    rng = random.Random(5)
    for n_max in (1, 4, 6, 8):
        for alphabet in (2, 1000):
            for n in (1, 2, 3, 4, 5, 8, MAX_GROUP):
                rows = random_group(rng, n, alphabet, n_max)
                assert serial_cells(host_lib, rows, n_max) == group_cells(rows, [n], n_max), (n_max, alphabet, n)


def test_split_helpers_restate_position_counts(host_lib):
    rng = random.Random(6)
    cases = 0
    for n_max in (1, 4, 6, 8):
        for alphabet in (2, 5, 1000):
            for _ in range(12):
                h = [rng.randrange(alphabet) for _ in range(rng.randrange(1, 60))]
                r = [rng.randrange(alphabet) for _ in range(rng.randrange(0, 60))]
                if rng.random() < 0.3:
                    r = (h[len(h) // 3:] + r)[:len(r)]
                ha, ra = np.asarray(h + [0], dtype=np.int32), np.asarray(r + [0], dtype=np.int32)
                for i in range(len(h)):
                    a, b = np.full(MAX_ORDER, -7, dtype=np.int32), np.full(MAX_ORDER, -9, dtype=np.int32)
                    host_lib.split(vp(ha), len(h), vp(ra), len(r), n_max, i, vp(a))
                    host_lib.whole(vp(ha), len(h), vp(ra), len(r), n_max, i, vp(b))
                    assert a.tolist() == b.tolist(), (n_max, alphabet, h, r, i)
                    cases += 1
    assert cases > 2000


def test_schedule_gives_every_ordered_cell_one_owner(host_lib):
    for n in list(range(1, 10)) + [MAX_GROUP]:
        owners, scans = np.zeros(n * n, dtype=np.int32), np.zeros(n, dtype=np.int32)
        host_lib.schedule(n, vp(owners), vp(scans))
        assert owners.tolist() == [1] * (n * n), n
        assert int(scans.sum()) == n * (n - 1) // 2 and int(scans.max()) - int(scans.min()) <= 1      # half of the pairs, spread evenly


def test_check_groups(host_lib):
    def check(off, grp, n_max):
        o, g = np.asarray(off, dtype=np.int32), np.asarray(grp, dtype=np.int32)
        return host_lib.check(vp(o), len(o) - 1, vp(g), len(g) - 1, n_max)
    ok_off = [0, 3, 3, 3 + GROUP_MAX_SYMBOLS, 10 + GROUP_MAX_SYMBOLS]
    assert check(ok_off, [0, 1, 1, 4], 8) == 0 and check(ok_off, [0, 4], 1) == 0           # a row of the limit, an empty group
    assert check(ok_off, [1, 4], 4) == -10 and check(ok_off, [0, 3], 4) == -10 and check(ok_off, [0, 5], 4) == -10
    assert check(ok_off, [0, 3, 2, 4], 4) == -10                                             # grp goes down
    assert check(ok_off, [0, 4], 0) == -10 and check(ok_off, [0, 4], 9) == -10
    assert check([0, 3, 3, 4 + GROUP_MAX_SYMBOLS], [0, 3], 4) == -10                         # a row of the limit + 1
    assert check([0, 3, 2, 5], [0, 3], 4) == -10 and check([-1, 3, 4, 5], [0, 3], 4) == -10  # off goes down / starts below 0
    assert check([0] * (MAX_GROUP + 1), [0, MAX_GROUP], 8) == 0                              # a group of the limit
    assert check([0] * (MAX_GROUP + 2), [0, MAX_GROUP + 1], 8) == -10
    assert check([0], [0], 4) == 0                                                            # G = 0
    # the output's index type: cells * n_max * 3 <= 2^31 - 1.  At n_max = 1 the limit is 715827882 cells = 174762 * 64^2 + 52^2 + 5^2
    # + 1^2, met exactly by these groups of empty rows; one more group of one row is refused, and so is n_max = 2
    sizes = [MAX_GROUP] * 174762 + [52, 5, 1]
    assert sum(n * n for n in sizes) == MAX_OUT // 3
    grp = np.concatenate([[0], np.cumsum(np.asarray(sizes, dtype=np.int64))]).astype(np.int32)
    off = np.zeros(int(grp[-1]) + 2, dtype=np.int32)
    assert host_lib.check(vp(off), int(grp[-1]), vp(grp), len(sizes), 1) == 0
    assert host_lib.check(vp(off), int(grp[-1]), vp(grp), len(sizes), 2) == -10
    more = np.concatenate([grp, [grp[-1] + 1]]).astype(np.int32)
    assert host_lib.check(vp(off), int(more[-1]), vp(more), len(sizes) + 1, 1) == -10
    # cell_offsets: the running sum of the squares, in int64
    cell_off = np.zeros(len(sizes) + 1, dtype=np.int64)
    host_lib.cells_of(vp(grp), len(sizes), vp(cell_off))
    assert cell_off.tolist()[:3] == [0, 4096, 8192] and int(cell_off[-1]) == MAX_OUT // 3


def test_entry_point_refuses_bad_arguments():
    """-10 outside the shapes and for null pointers, nothing launched (fake device pointers are never dereferenced); G == 0 is success."""
    from gtos_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION >= 36
    p = ctypes.c_void_p(16)
    off = np.asarray([0, 2, 5, 5 + GROUP_MAX_SYMBOLS], dtype=np.int32)
    long_off = np.asarray([0, 2, 5, 6 + GROUP_MAX_SYMBOLS], dtype=np.int32)
    grp = np.asarray([0, 1, 3], dtype=np.int32)

    def call(sym=p, off_d=p, R=3, grp_d=p, G=2, n_max=4, off_h=off, grp_h=grp, out=p):
        host = lambda a: None if a is None else vp(a)        # noqa: E731
        return lib.gtos_ngram_overlap_groups(sym, off_d, R, grp_d, G, n_max, host(off_h), host(grp_h), out, None)
    assert call(n_max=0) == -10 and call(n_max=9) == -10
    assert call(off_h=long_off) == -10
    assert call(grp_h=np.asarray([0, 1, 2], dtype=np.int32)) == -10 and call(grp_h=np.asarray([1, 1, 3], dtype=np.int32)) == -10
    assert call(grp_h=np.asarray([0, 4, 3], dtype=np.int32)) == -10
    big = np.zeros(MAX_GROUP + 3, dtype=np.int32)
    assert call(R=MAX_GROUP + 1, G=1, off_h=big, grp_h=np.asarray([0, MAX_GROUP + 1], dtype=np.int32)) == -10
    assert call(G=-1) == -10 and call(R=-1) == -10
    for name in ("sym", "off_d", "grp_d", "out", "off_h", "grp_h"):
        assert call(**{name: None}) == -10, name
    zero = np.asarray([0], dtype=np.int32)
    assert call(R=0, G=0, off_h=zero, grp_h=zero) == 0 and call(R=0, G=0, off_h=zero, grp_h=zero, sym=None, off_d=None, grp_d=None, out=None) == 0
    assert call(R=0, G=2, off_h=zero, grp_h=np.asarray([0, 0, 0], dtype=np.int32), out=None) == 0        # only empty groups


# ------------------------------------------------------------------------------------------------ CPU: the expectation on host tensors
def stats_of(groups, kind, n):
    return torch.tensor([counter_stats(symbols_of(a, kind), symbols_of(b, kind), n) for g in groups for a in g for b in g],
                        dtype=torch.int32).reshape(-1, n, 3)


def sentences(rng, n, words=("ab", "cd.", "efg", "h", "ij,", "klm", "no", "(p", "q", "rs")):
    return [[rng.choice(words) for _ in range(rng.randrange(0, 9))] for _ in range(n)]


def test_expected_utility_on_host_tensors():
    from gtos_amd import metrics
    rng = random.Random(8)
    same = ["ab", "cd.", "efg"]
    groups = [sentences(rng, 5), sentences(rng, 1), [], sentences(rng, 7), [list(same) for _ in range(4)], sentences(rng, 2)]
    sizes = [len(g) for g in groups]
    char, word = stats_of(groups, "char", 6), stats_of(groups, "chrf_word", 2)
    weightings = {
        "uniform": None,
        "random": [rng.random() for _ in range(sum(sizes))],
        "a zero": [0.0 if k % 3 == 0 else rng.random() for k in range(sum(sizes))],
        "all zero in group 0 and 3": [0.0] * 5 + [rng.random() for _ in range(sum(sizes) - 5 - 7 - 4 - 2)] + [0.0] * 7
                                     + [rng.random() for _ in range(6)],
        "all zero": [0.0] * sum(sizes),
    }
    for name, w in weightings.items():
        value, index = metrics.expected_utility(char, word, sizes, w)
        assert value.dtype == torch.float64 and value.shape == (sum(sizes),) and index.dtype == torch.int64 and index.shape == (len(sizes),)
        start = 0
        for g, cands in enumerate(groups):
            want, best = own_mbr(cands, None if w is None else w[start:start + len(cands)])
            got = value[start:start + len(cands)].tolist()
            assert all(abs(a - b) <= TOL for a, b in zip(got, want)), (name, g)
            assert int(index[g]) == best, (name, g, got, want)
            if cands and (w is None or sum(w[start:start + len(cands)]) == 0):
                uniform, _ = own_mbr(cands)
                assert all(abs(a - b) <= TOL for a, b in zip(got, uniform))
            start += len(cands)
        assert int(index[2]) == -1 and int(index[1]) == 0
        # identical candidates: the first, and every value the self-score
        self_score = sentence_chrf(same, same)
        first = sum(sizes[:4])
        assert int(index[4]) == 0 and all(abs(v - self_score) <= TOL for v in value[first:first + 4].tolist())
        assert len(set(value[first:first + 4].tolist())) == 1
    # a tensor of weights is taken as well as a list; no groups at all
    value, index = metrics.expected_utility(char, word, sizes, torch.tensor(weightings["random"], dtype=torch.float64))
    assert torch.equal(value, metrics.expected_utility(char, word, sizes, weightings["random"])[0])
    value, index = metrics.expected_utility(char[:0], word[:0], [0, 0])
    assert value.numel() == 0 and index.tolist() == [-1, -1]
    with pytest.raises(ValueError):
        metrics.expected_utility(char, word, sizes[:-1])
    with pytest.raises(ValueError):
        metrics.expected_utility(char, word, sizes, [1.0])


def test_ops_refuse_cpu_symbols_and_name_the_offending_value():
    from gtos_amd import ops, _lib
    assert (ops.OVERLAP_MAX_GROUP, ops.OVERLAP_GROUP_MAX_SYMBOLS) == (MAX_GROUP, GROUP_MAX_SYMBOLS)
    with pytest.raises(_lib.GtosHipError):
        ops.ngram_overlap_groups(torch.zeros(3, dtype=torch.int32), torch.tensor([0, 3], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.int32), 4)
    assert ops.group_cell_offsets(torch.tensor([0, 2, 2, 5], dtype=torch.int32)).tolist() == [0, 4, 4, 13]


# ------------------------------------------------------------------------------------------------ GPU: the kernel
def kernel_case(n_max):
    """(rows, sizes): one launch with groups of 1, 2, 3, 4, 0, 7 and 8 rows"""
    rng = random.Random(13)
    rnd = lambda n, a: [rng.randrange(a) for _ in range(n)]         # noqa: E731
    twin = rnd(90, 4)
    long_row = rnd(700, 6)
    groups = [
        [rnd(GROUP_MAX_SYMBOLS, 40)],                                                   # 1: one row of exactly the limit
        [rnd(300, 2), rnd(300, 2)],                                                     # 2: heavy clipping
        [rnd(255, 6), rnd(256, 6), rnd(257, 6)],                                        # 3: the thread stride wraps
        [[], rnd(1, 3), rnd(n_max + 1, 3), rnd(n_max, 2)],                              # 4: around the order
        [],                                                                             # 0: an empty group in the middle
        [rnd(max(n_max - 1, 0), 3), twin, rnd(120, 1000), list(twin), rnd(17, 2), [], long_row],          # 7: twins, an empty row
        [rnd(64, 5), long_row[200:650] + rnd(50, 6), rnd(GROUP_MAX_SYMBOLS - 1, 3), rnd(513, 6), rnd(n_max, 3), rnd(1, 2), long_row,
         rnd(33, 1000)],                                                                # 8: long shared stretches, two buffers' worth
    ]
    return [r for g in groups for r in g], [len(g) for g in groups]


def pair_list(sizes):
    return [(s + i, s + j) for s, n in zip(offsets(sizes), sizes) for i in range(n) for j in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("n_max", [1, 4, 6, 8])
def test_kernel_equals_the_counter_statement_inside_guard_bands(n_max):
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rows, sizes = kernel_case(n_max)
    assert sizes == [1, 2, 3, 4, 0, 7, 8]
    sym, off = csr(rows)
    grp = torch.tensor(offsets(sizes), dtype=torch.int32)
    cells = sum(n * n for n in sizes)
    want = torch.tensor(group_cells(rows, sizes, n_max), dtype=torch.int32)
    got = ops.ngram_overlap_groups(sym.to(dev), off, grp, n_max)
    assert got.dtype == torch.int32 and got.shape == (cells, n_max, 3)
    assert torch.equal(got.cpu(), want)
    # ... the pair-list kernel on the explicit ordered pairs stores the same integers
    listed = ops.ngram_overlap(sym.to(dev), off, torch.tensor(pair_list(sizes), dtype=torch.int32), n_max)
    assert torch.equal(got, listed)
    # sentinel elements in front of and behind the output stay untouched; a second launch into the same buffer gives identical bits
    gi = GuardedFlat(cells * n_max * 3, torch.float32, dev)
    out = gi.view.view(torch.int32)
    ops.ngram_overlap_groups_into(sym.to(dev), off, grp, n_max, out)
    gi.check("gtos_ngram_overlap_groups n_max %d" % n_max)
    first = out.clone()
    assert torch.equal(first.cpu().view(cells, n_max, 3), want)
    ops.ngram_overlap_groups_into(sym.to(dev), off, grp, n_max, out)
    gi.check("gtos_ngram_overlap_groups n_max %d, second launch" % n_max)
    assert torch.equal(out, first)
    # G = 0, one group of one, only empty rows
    none = ops.ngram_overlap_groups(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32),
                                    torch.zeros(1, dtype=torch.int32), n_max)
    assert none.shape == (0, n_max, 3)
    s1, o1 = csr([rows[3]])
    one = ops.ngram_overlap_groups(s1.to(dev), o1, torch.tensor([0, 1], dtype=torch.int32), n_max)
    assert torch.equal(one.cpu(), torch.tensor([counter_stats(rows[3], rows[3], n_max)], dtype=torch.int32))
    empty = ops.ngram_overlap_groups(torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(4, dtype=torch.int32),
                                     torch.tensor([0, 2, 3], dtype=torch.int32), n_max)
    assert torch.equal(empty.cpu(), torch.zeros((5, n_max, 3), dtype=torch.int32))


@pytest.mark.gpu
def test_a_full_group_of_the_largest_size():
    """MAX_GROUP candidates: the longest half circle (32 references through the two buffers) and, n being even, the shared n/2 pair"""
    from gtos_amd import ops
    dev = torch.device("cuda:0")
    rng = random.Random(17)
    rows = [[rng.randrange(4) for _ in range(rng.randrange(0, 40))] for _ in range(MAX_GROUP)] + [[1, 2, 3]]
    sizes = [MAX_GROUP, 1]
    sym, off = csr(rows)
    got = ops.ngram_overlap_groups(sym.to(dev), off, torch.tensor(offsets(sizes), dtype=torch.int32), 6)
    assert torch.equal(got.cpu(), torch.tensor(group_cells(rows, sizes, 6), dtype=torch.int32))


@pytest.mark.gpu
def test_bad_launches_raise_and_leave_the_output_unwritten():
    from gtos_amd import ops, _lib
    dev = torch.device("cuda:0")
    sym, off = csr([[1, 2, 3], [1] * (GROUP_MAX_SYMBOLS + 1), [2, 3]])
    ok_sym, ok_off = csr([[1, 2, 3], [2, 3], [3]])
    grp = torch.tensor([0, 2, 3], dtype=torch.int32)
    many_sym, many_off = csr([[1]] * (MAX_GROUP + 1))
    g = GuardedFlat(0, torch.float32, dev, lead=64 + 3 * (MAX_GROUP + 1) ** 2, trail=64)
    # (the outputs handed in below lie INSIDE the band: any store shows)
    cases = [(sym, off, grp, 4), (ok_sym, ok_off, grp, 0), (ok_sym, ok_off, grp, 9),
             (ok_sym, ok_off, torch.tensor([0, 2, 2], dtype=torch.int32), 4), (ok_sym, ok_off, torch.tensor([1, 2, 3], dtype=torch.int32), 4),
             (ok_sym, ok_off, torch.tensor([0, 3, 2, 3], dtype=torch.int32), 4),
             (many_sym, many_off, torch.tensor([0, MAX_GROUP + 1], dtype=torch.int32), 1)]
    for s, o, gr, n in cases:
        with pytest.raises(_lib.GtosHipError):
            ops.ngram_overlap_groups(s.to(dev), o, gr, n)
        sizes = (gr[1:] - gr[:-1]).tolist()
        with pytest.raises(_lib.GtosHipError):
            ops.ngram_overlap_groups_into(s.to(dev), o, gr, n, g.buf[32:32 + sum(k * k for k in sizes) * n * 3].view(torch.int32))
    with pytest.raises(_lib.GtosHipError):
        ops.ngram_overlap_groups(ok_sym.to(dev), ok_off, grp.to(dev), 4)                # grp is a host tensor
    with pytest.raises(_lib.GtosHipError):
        ops.ngram_overlap_groups_into(ok_sym.to(dev), ok_off, grp.to(dev), 4, g.buf[32:32 + 5 * 4 * 3].view(torch.int32))
    with pytest.raises(_lib.GtosHipError):
        ops.ngram_overlap_groups(ok_sym.to(dev), ok_off.to(dev), grp, 4)
    g.check("a refused gtos_ngram_overlap_groups")


@pytest.mark.gpu
def test_pairwise_routes_and_layout():
    from gtos_amd import metrics
    dev = torch.device("cuda:0")
    rng = random.Random(19)
    groups = [sentences(rng, 3), [], sentences(rng, 2), sentences(rng, 1)]
    for kind, n in (("char", 6), ("chrf_word", 2), ("word", 4)):
        got, cell_off = metrics.pairwise(groups, kind, device=dev)
        assert got.is_cuda and cell_off.tolist() == [0, 9, 9, 13, 14] and cell_off.dtype == torch.int64
        assert torch.equal(got.cpu(), stats_of(groups, kind, n))
    # a row of GROUP_MAX_SYMBOLS + 1 symbols: the pair-list route, the same layout
    long_sentence = ["x" * 5] * ((GROUP_MAX_SYMBOLS + 1) // 5) + ["y" * ((GROUP_MAX_SYMBOLS + 1) % 5)]
    assert len("".join(long_sentence)) == GROUP_MAX_SYMBOLS + 1
    groups[2].append(long_sentence)
    got, cell_off = metrics.pairwise(groups, "char", n_max=3, device=dev)
    assert cell_off.tolist() == [0, 9, 9, 18, 19] and torch.equal(got.cpu(), stats_of(groups, "char", 3))
    # ... and a group of MAX_GROUP + 1 candidates
    wide = [sentences(rng, MAX_GROUP + 1), sentences(rng, 2)]
    got, cell_off = metrics.pairwise(wide, "chrf_word", device=dev)
    assert cell_off.tolist() == [0, (MAX_GROUP + 1) ** 2, (MAX_GROUP + 1) ** 2 + 4] and torch.equal(got.cpu(), stats_of(wide, "chrf_word", 2))
    got, cell_off = metrics.pairwise([], "char", device=dev)
    assert got.shape == (0, 6, 3) and cell_off.tolist() == [0]


# ------------------------------------------------------------------------------------------------ GPU: mbr_select and Trainer.validate
SMALL_K, SMALL_T, ALPHA = 4, 8, 0.6
SAMPLE_SEED, STOCHASTIC_SEED = 5, 7
_small = {}


def gen_small():
    """A fresh small golden generator (tests/golden/gen_small) with string vocabularies, its eval batch and the batch with the graphs
    in another order: (model, [batch, batch2], d, train batch)."""
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


def host_candidates(beam, weights, scale=1.0):
    """The candidates of one beam and their weights, stated apart from gtos_amd.metrics"""
    from gtos_amd import search
    if weights == "stochastic":
        pairs = search.stochastic_weights(beam)[0]
        return [strip(h) for h, _ in pairs], [w for _, w in pairs]
    best = beam.get_k_best(SMALL_K, ALPHA)
    if weights == "uniform":
        return [strip(h) for h in best], None
    top = max(scale * h.score for h in best)
    e = [math.exp(scale * h.score - top) for h in best]
    return [strip(h) for h in best], [x / sum(e) for x in e]


SEARCHES = [(dict(search="sample", seed=SAMPLE_SEED), "uniform"), (dict(search="device"), "score"),
            (dict(search="stochastic", seed=STOCHASTIC_SEED), "stochastic")]


@pytest.mark.gpu
def test_mbr_select_equals_the_host_statement():
    from gtos_amd import metrics
    model, (batch, _), _, _ = gen_small()
    clear = 0
    for options, weights in SEARCHES:
        beams = model.work(batch, SMALL_K, SMALL_T, 1, **options)
        got = metrics.mbr_select(beams, SMALL_K, ALPHA, weights)
        assert len(got) == len(beams) == 3
        for (tokens, index, utility), beam in zip(got, beams):
            cands, w = host_candidates(beam, weights)
            if not cands:
                assert tokens is None and index == -1 and math.isnan(utility)
                continue
            values, best = own_mbr(cands, w)
            ranked = sorted(values, reverse=True)
            gap = ranked[0] - ranked[1] if len(ranked) > 1 else float("inf")
            print("MEASURED %s graph: %d candidates, host values %s, device index %d utility %.12f" % (
                options["search"], len(cands), [round(v, 6) for v in values], index, utility))
            assert tokens == cands[index] and abs(utility - values[index]) <= TOL
            if gap > TOL:
                assert index == best
                clear += 1
            else:
                assert values[index] >= ranked[0] - TOL
    assert clear >= 6, "only %d of the 9 graphs have a clear host winner: the comparison of the indices has emptied out" % clear
    # one candidate: index 0; no hypotheses: (None, -1, nan)
    beams = model.work(batch, SMALL_K, SMALL_T, 1, search="device")
    short = metrics.mbr_select(beams, 1, ALPHA, "score")
    assert [i for _, i, _ in short] == [0, 0, 0]
    for (tokens, _, utility), beam in zip(short, beams):
        assert tokens == strip(beam.get_k_best(1, ALPHA)[0]) and abs(utility - sentence_chrf(tokens, tokens)) <= TOL
    beams[1].hypotheses, beams[1].completed_hypotheses = [], []
    holed = metrics.mbr_select(beams, SMALL_K, ALPHA, "uniform")
    assert holed[1][0] is None and holed[1][1] == -1 and math.isnan(holed[1][2]) and holed[0][0] is not None and holed[2][1] >= 0
    with pytest.raises(ValueError):
        metrics.mbr_select(beams, SMALL_K, ALPHA, "softmax")


def _bits(t):
    return t.detach().clone().view(torch.int32)


@pytest.mark.gpu
def test_validate_mbr_matches_the_host_computation_and_leaves_the_trainer_alone(monkeypatch):
    from gtos_amd.train import Trainer
    model, batches, d, train_batch = gen_small()
    trainer = Trainer(model, d, warmup_steps=10)
    model.train()
    trainer.step(train_batch)                                           # a trainer in mid-training: moments and counters are not zero
    torch.cuda.synchronize()
    flat = trainer.flat
    before = [_bits(flat.param), _bits(flat.m), _bits(flat.v), _bits(flat.grad), trainer._state.clone(), trainer.steps_issued]

    # host reads, counted on device tensors as tests/test_overlap_metrics.py counts them
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

    common = dict(beam_size=SMALL_K, alpha=ALPHA, max_time_step=SMALL_T, min_time_step=1)
    for options, weights in SEARCHES:
        model.eval()
        picks = []
        for batch in batches:
            for beam in model.work(batch, SMALL_K, SMALL_T, 1, **options):
                cands, w = host_candidates(beam, weights)
                picks.append(cands[own_mbr(cands, w)[1]] if cands else strip(beam.get_k_best(1, ALPHA)[0]))
        model.train()
        refs = [true_references(model, batch) for batch in batches]
        own = own_scores(picks, refs[0] + refs[1])
        reads[0] = 0
        plain = trainer.validate(batches, None, return_outputs=True, **common, **options)
        best_reads, reads[0] = reads[0], 0
        got = trainer.validate(batches, None, return_outputs=True, select="mbr", mbr_weights=weights, **common, **options)
        mbr_reads, reads[0] = reads[0], 0
        trainer.validate(batches, None, select="mbr", mbr_weights=weights, **common, **options)
        assert mbr_reads <= best_reads + 1 and reads[0] <= best_reads, (best_reads, mbr_reads, reads[0])
        print("MEASURED validate %s mbr: %s; host reads %d (best) %d (mbr)" % (
            options["search"], {k: v for k, v in got.items() if k != "outputs"}, best_reads, mbr_reads))
        assert got["outputs"] == picks
        for key in ("bleu", "brevity_penalty", "chrf", "chrf_avg"):
            assert abs(got[key] - own[key]) < 1e-9, (key, got[key], own[key])
        assert all(abs(a - b) < 1e-9 for a, b in zip(got["bleu_precisions"], own["bleu_precisions"]))
        assert (got["hyp_tokens"], got["ref_tokens"], got["sentences"]) == (own["hyp_tokens"], own["ref_tokens"], 6)
        assert model.training
        # select="best" is the call without the keyword
        assert trainer.validate(batches, None, return_outputs=True, select="best", **common, **options) == plain
    monkeypatch.undo()
    torch.cuda.synchronize()
    after = [_bits(flat.param), _bits(flat.m), _bits(flat.v), _bits(flat.grad), trainer._state.clone(), trainer.steps_issued]
    for a, b, what in zip(before, after, ("parameters", "Adam m", "Adam v", "gradient bucket", "counters")):
        assert torch.equal(a, b), what + " changed under validate"
    assert before[5] == after[5]
    model.eval()
    with pytest.raises(ValueError):
        trainer.validate(batches, None, select="oracle", **common)
