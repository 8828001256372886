"""BLEU and chrF++ of decoded text, on one exact device count.

The reference picks its checkpoints by decoding a held-out set and scoring it with multi-bleu.perl and chrF++.py
(generator/work.py ``validate``).  Both scores are functions of one statistic, the clipped n-gram matches between a hypothesis and a
reference for the orders 1..n, over three kinds of symbols:

  "word"       word ids, order 4                                   -> BLEU
  "chrf_word"  word ids after chrF++'s punctuation separation, 2   -> the word half of chrF++
  "char"       code points of the sentence without its spaces, 6   -> the character half of chrF++

``encode`` turns token-string lists into symbol rows on the host (strings live there), ``overlap`` counts on the GPU
(ops.ngram_overlap -> gtos_ngram_overlap, the rule in csrc/overlap_kernels.h: one workgroup per pair, any pair list -- row i with
row i, an n-best list against its reference, all pairs of a sample set) and ``bleu`` / ``chrf`` / ``sentence_chrf`` are a few fp64
torch operations on those counts that never read the host: they take host or device tensors and return tensors where the counts
live.  Scores are on the 0..100 scale the two programs print.  ``best_of_nbest`` picks, per graph, the hypothesis of an n-best list
that scores best against the reference; ``Trainer.validate`` (gtos_amd.train) is the checkpoint-selection step itself.

Without a reference, ``mbr_select`` picks by minimum Bayes risk: the candidate of a sample set or n-best list with the highest
expected sentence chrF++ against the set itself, each member weighted by how probable it is.  ``pairwise`` counts all ordered pairs
inside every graph's candidate group in one launch (ops.ngram_overlap_groups -> gtos_ngram_overlap_groups, csrc/mbr_kernels.h: one
workgroup per candidate, half of the group scanned, no pair list) and ``expected_utility`` is the fp64 weighting and the per-group
argmax, again without a host read.

One reference per hypothesis; the tokens are scored as given (no lowercasing, no tokeniser of its own).
"""
import math
import string

import torch

from . import ops
from .vocab import END, STR, UNK

KINDS = {"word": 4, "chrf_word": 2, "char": 6}       # kind -> the order its score uses
_PUNCT = frozenset(string.punctuation)

# Trainer.validate's totals, one fp64 device buffer (the counts are integers, exact in fp64 below 2^53): the summed statistics of
# the three kinds as [orders, 3] blocks, then hypothesis tokens, reference tokens, sentences, and the sum of the sentence chrF++
_W4, _W2, _C6 = slice(0, 12), slice(12, 18), slice(18, 36)
_HYP, _REF, _SENTS, _SUMF = 36, 37, 38, 39
N_TOTALS = 40


def separate_punctuation(words):
    """chrF++'s word tokens: a word longer than one character whose last character is in string.punctuation is split before that
    character; otherwise, if its first character is, it is split after it.  One split per word at most."""
    out = []
    for w in words:
        if len(w) > 1 and w[-1] in _PUNCT:
            out += [w[:-1], w[-1]]
        elif len(w) > 1 and w[0] in _PUNCT:
            out += [w[0], w[1:]]
        else:
            out.append(w)
    return out


def encode(sentences, kind, unknown=UNK):
    """Host side: token-string lists -> (sym int32 [total], off int32 [len(sentences) + 1]) host tensors, the CSR rows
    ops.ngram_overlap takes.  ``kind`` as in KINDS.  The sentences of one call share the id table (pass hypotheses and references
    together); ids are only compared for equality, within the call.  A token equal to ``unknown`` (the vocabulary's <UNK>: a word
    whose text was lost) is a symbol of its own at every occurrence, one word and one character that match nothing; None: no such
    token."""
    if kind not in KINDS:
        raise ValueError("kind must be one of %s, got %r" % (sorted(KINDS), kind))
    table, sym, off = {}, [], [0]
    fresh = -1                                   # ids of unknown words: negative, never equal to a table id or a code point
    seen = {}                                    # token string -> its symbols (the candidates of a sample set repeat their words)
    for words in sentences:
        if isinstance(words, str) or not all(isinstance(w, str) for w in words):
            raise ValueError("a sentence is a list of token strings, got %r" % (words,))
        for w in words:
            if unknown is not None and w == unknown:
                sym.append(fresh)
                fresh -= 1
                continue
            s = seen.get(w)
            if s is None:
                if kind == "char":
                    s = [ord(c) for c in w if c != " "]
                else:
                    s = [table.setdefault(x, len(table)) for x in (separate_punctuation([w]) if kind == "chrf_word" else [w])]
                seen[w] = s
            sym.extend(s)
        off.append(len(sym))
    return torch.tensor(sym, dtype=torch.int32), torch.tensor(off, dtype=torch.int32)


def _pair_tensor(pairs, n_hyps, n_refs):
    if pairs is None:
        if n_hyps != n_refs:
            raise ValueError("pairs=None pairs row i with row i: %d hypotheses, %d references" % (n_hyps, n_refs))
        idx = torch.arange(n_hyps, dtype=torch.int32)
        return torch.stack([idx, idx + n_hyps], 1)
    p = torch.as_tensor(pairs, dtype=torch.int64).reshape(-1, 2)
    if p.numel() and (int(p[:, 0].min()) < 0 or int(p[:, 0].max()) >= n_hyps or int(p[:, 1].min()) < 0 or int(p[:, 1].max()) >= n_refs):
        raise ValueError("pairs: (hypothesis, reference) indices into %d hypotheses and %d references" % (n_hyps, n_refs))
    return torch.stack([p[:, 0], p[:, 1] + n_hyps], 1).to(torch.int32)


def overlap(hyps, refs, pairs=None, kind="word", n_max=None, device="cuda"):
    """The device statistics int32 [P, n_max, 3] (matches, hypothesis n-grams, reference n-grams per order) of ``pairs``, a host
    list / tensor of (index into hyps, index into refs); None: row i with row i.  ``n_max`` None: the order ``kind``'s score uses.
    One launch; the host reads nothing."""
    n_max = KINDS[kind] if n_max is None else n_max
    hyps, refs = list(hyps), list(refs)
    sym, off = encode(hyps + refs, kind)
    return ops.ngram_overlap(sym.to(device), off, _pair_tensor(pairs, len(hyps), len(refs)), n_max)


def _summed(stats):
    s = torch.as_tensor(stats)
    return (s if s.dim() == 2 else s.sum(0)).to(torch.float64)


def bleu(stats_word4, hyp_len=None, ref_len=None):
    """Corpus BLEU as multi-bleu.perl computes it for one reference, from the "word" statistics at order 4 ([P,4,3], or their sum
    [4,3]): precisions from the summed clipped counts, their geometric mean, the brevity penalty exp(1 - ref_len / hyp_len) when
    the hypothesis side is shorter, 0 when any of the four counts is 0.  ``hyp_len`` / ``ref_len``: the token totals (numbers or
    tensors); None: the order-1 n-gram totals, which they equal.  Returns a dict of fp64 tensors where the statistics live: ``bleu``
    (0..100), ``precisions`` [4] (0..100), ``brevity_penalty``, ``hyp_len``, ``ref_len``."""
    s = _summed(stats_word4)
    if s.shape != (4, 3):
        raise ValueError("bleu takes the order-4 statistics [P,4,3] or [4,3], got %s" % (tuple(s.shape),))
    as_t = lambda v, d: d if v is None else torch.as_tensor(v, dtype=torch.float64, device=s.device)       # noqa: E731
    hyp_len, ref_len = as_t(hyp_len, s[0, 1]), as_t(ref_len, s[0, 2])
    match, total = s[:, 0], s[:, 1]
    prec = torch.where(total > 0, match / total.clamp(min=1.0), torch.zeros_like(match))
    bp = torch.where(hyp_len < ref_len, torch.exp(1.0 - ref_len / hyp_len.clamp(min=1.0)), torch.ones_like(hyp_len))
    geo = torch.exp(torch.log(prec.clamp(min=1e-300)).sum() / 4.0)
    score = torch.where((match > 0).all(), bp * geo, torch.zeros_like(geo))
    return {"bleu": 100.0 * score, "precisions": 100.0 * prec, "brevity_penalty": bp, "hyp_len": hyp_len, "ref_len": ref_len}


def _order_f(stats, beta):
    """F_beta per order from float64 statistics [..., orders, 3], with chrF++'s 1e-16 where a side has no n-grams."""
    match, hyp, ref = stats[..., 0], stats[..., 1], stats[..., 2]
    tiny = torch.full_like(match, 1e-16)
    prec = torch.where(hyp > 0, match / hyp.clamp(min=1.0), tiny)
    rec = torch.where(ref > 0, match / ref.clamp(min=1.0), tiny)
    factor = beta * beta
    denom = factor * prec + rec
    return torch.where(denom > 0, (1.0 + factor) * prec * rec / torch.where(denom > 0, denom, torch.ones_like(denom)), tiny)


def _chrf_of(char, word, beta):
    orders = char.shape[-2] + word.shape[-2]
    return 100.0 * (_order_f(char, beta).sum(-1) + _order_f(word, beta).sum(-1)) / orders


def sentence_chrf(stats_char6, stats_word2, beta=2.0):
    """chrF++ per pair, fp64 [P] (0..100) where the statistics live: per order precision and recall (1e-16 where that side has no
    n-grams) and F_beta, the mean over the 6 character and 2 word orders."""
    char, word = torch.as_tensor(stats_char6).to(torch.float64), torch.as_tensor(stats_word2).to(torch.float64)
    if char.dim() != 3 or word.dim() != 3 or char.shape[0] != word.shape[0] or char.shape[2] != 3 or word.shape[2] != 3:
        raise ValueError("sentence_chrf takes statistics [P, orders, 3] of the same pairs, got %s and %s"
                         % (tuple(char.shape), tuple(word.shape)))
    return _chrf_of(char, word, beta)


def chrf(stats_char6, stats_word2, beta=2.0):
    """chrF++ as the reference's program computes it for one reference, from the "char" statistics at order 6 and the "chrf_word"
    statistics at order 2 of the same pairs: ``F``, the corpus score from the summed counts, and ``avgF``, the mean of the sentence
    scores; a dict of fp64 tensors (0..100) where the statistics live.  (For a pair that scores 0 the program adds the previous
    sentence's counts to its corpus totals; here every pair contributes its own.)"""
    sent = sentence_chrf(stats_char6, stats_word2, beta)
    char, word = torch.as_tensor(stats_char6).sum(0).to(torch.float64), torch.as_tensor(stats_word2).sum(0).to(torch.float64)
    avg = sent.sum() / max(sent.numel(), 1)
    return {"F": _chrf_of(char, word, beta), "avgF": avg}


def hypothesis_tokens(hyp):
    """The token strings of a search Hypothesis without <STR> and <END>."""
    seq = hyp.seq[1:] if hyp.seq and hyp.seq[0] == STR else hyp.seq
    return list(seq[:-1] if seq and seq[-1] == END else seq)


def best_of_nbest(beams, references, k=None, alpha=0.6, beta=2.0, device="cuda"):
    """Per graph, the hypothesis of its n-best list -- ``beam.get_k_best(k, alpha)``, in that order; ``k`` None: the beam's width --
    with the highest sentence chrF++ against the graph's reference (a token-string list); among equals the first.  One launch per
    statistic kind for the whole batch (B * k pairs) and one host read.  Returns one (tokens, index, score) per graph; (None, -1,
    nan) for a beam without hypotheses.  The gap between index 0's score and the best one's is search error, the rest the model's."""
    if len(beams) != len(references):
        raise ValueError("one reference per beam: %d beams, %d references" % (len(beams), len(references)))
    hyps, pairs, lists = [], [], []
    for b, beam in enumerate(beams):
        best = beam.get_k_best(beam.beam_size if k is None else k, alpha)
        lists.append([hypothesis_tokens(h) for h in best])
        pairs += [(len(hyps) + j, b) for j in range(len(best))]
        hyps += lists[-1]
    if not hyps:
        return [(None, -1, float("nan")) for _ in beams]
    refs = [list(r) for r in references]
    sent = sentence_chrf(overlap(hyps, refs, pairs, "char", device=device), overlap(hyps, refs, pairs, "chrf_word", device=device), beta)
    width = max(len(l) for l in lists)
    graph = torch.tensor([b for _, b in pairs], dtype=torch.int64)
    rank = torch.tensor([j for l in lists for j in range(len(l))], dtype=torch.int64)
    grid = torch.full((len(beams), width), -1.0, dtype=torch.float64, device=sent.device)
    grid[graph.to(sent.device), rank.to(sent.device)] = sent
    score, index = grid.max(1)
    picked = torch.stack([index.to(torch.float64), score]).tolist()                 # the one host read
    out = []
    for b, (i, s) in enumerate(zip(*picked)):
        out.append((lists[b][int(i)], int(i), s) if lists[b] else (None, -1, float("nan")))
    return out


def pairwise(groups, kind, n_max=None, device="cuda"):
    """All ordered (hypothesis, reference) pairs inside every group: ``groups`` is a list of G lists of token-string lists (the
    candidates of G graphs; a group may be empty).  Returns ``(stats, cell_off)``: the device statistics int32 [cells, n_max, 3],
    cells = sum n_g^2, and the host tensor cell_off int64 [G+1], the running sum of n_g^2 -- the cell of (candidate i as
    hypothesis, candidate j as reference) of group g is ``cell_off[g] + i * n_g + j`` and holds what ``overlap`` gives for that
    pair.  One ``encode`` call for everything (ids are comparable across the batch) and ONE gtos_ngram_overlap_groups launch; the
    host reads nothing.  A batch in which some group holds more than ops.OVERLAP_MAX_GROUP candidates or some row more than
    ops.OVERLAP_GROUP_MAX_SYMBOLS symbols goes through ops.ngram_overlap on the explicit ordered pair list instead (rows up to
    ops.OVERLAP_MAX_SYMBOLS symbols stay legal there), into the same layout.  The limits alone decide the route: inside them the
    grouped kernel measured faster at every shape, 1.2x at 8 candidates per group to 3.1x at 64 (tools/bench_mbr.py)."""
    n_max = KINDS[kind] if n_max is None else n_max
    groups = [[list(c) for c in g] for g in groups]
    sizes = [len(g) for g in groups]
    sym, off = encode([c for g in groups for c in g], kind)
    grp = torch.tensor([0] + sizes, dtype=torch.int64).cumsum(0).to(torch.int32)
    cell_off = ops.group_cell_offsets(grp)
    longest = int((off[1:] - off[:-1]).max()) if off.numel() > 1 else 0
    if max(sizes, default=0) <= ops.OVERLAP_MAX_GROUP and longest <= ops.OVERLAP_GROUP_MAX_SYMBOLS \
            and int(cell_off[-1]) * n_max * 3 <= ops.OVERLAP_GROUP_MAX_OUT:
        return ops.ngram_overlap_groups(sym.to(device), off, grp, n_max), cell_off
    pairs = torch.cat([torch.stack([a.repeat_interleave(n), a.repeat(n)], 1)
                       for a, n in ((torch.arange(s, s + n, dtype=torch.int32), n) for s, n in zip(grp.tolist(), sizes))]
                      or [torch.zeros((0, 2), dtype=torch.int32)])
    return ops.ngram_overlap(sym.to(device), off, pairs, n_max), cell_off


def expected_utility(stats_char6, stats_word2, sizes, weights=None, beta=2.0):
    """Minimum-Bayes-risk values from ``pairwise``'s statistics of the same groups ("char" at order 6, "chrf_word" at order 2;
    ``sizes`` = the host list of the G group sizes n_g, R = their sum).  With U[i, j] the sentence chrF++ of candidate i as
    hypothesis against candidate j as reference, the value of candidate i is sum_j w_j U[i, j] / sum_j w_j over its own group, j = i
    included.  ``weights``: None (uniform: the Monte-Carlo estimate for independent samples) or one non-negative fp64 value per
    candidate, in row order (a list, a host or a device tensor); a candidate of weight 0 is still a candidate but no evidence, and a
    group whose weights sum to 0 is treated as uniform.  A few fp64 torch operations where the statistics live, in a fixed order
    (identical candidates get identical values); nothing reads the host.  Returns ``(value fp64 [R], index int64 [G])``: the first
    maximum of every group, counted inside the group, -1 for an empty group."""
    sizes = [int(n) for n in sizes]
    U = sentence_chrf(stats_char6, stats_word2, beta)
    dev = U.device
    G, R, m = len(sizes), sum(sizes), max(sizes, default=0)
    if U.numel() != sum(n * n for n in sizes):
        raise ValueError("expected_utility: %d cells for groups of sizes %s" % (U.numel(), sizes))
    if weights is not None:
        weights = torch.as_tensor(weights, dtype=torch.float64).reshape(-1)
        if weights.numel() != R:
            raise ValueError("expected_utility: one weight per candidate: %d candidates, %d weights" % (R, weights.numel()))
    if R == 0:
        return torch.zeros(0, dtype=torch.float64, device=dev), torch.full((G,), -1, dtype=torch.int64, device=dev)
    # index tensors built on the host from the sizes alone
    group_of = torch.repeat_interleave(torch.arange(G, dtype=torch.int64), torch.tensor(sizes, dtype=torch.int64))
    start = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0)
    within = torch.arange(R, dtype=torch.int64) - start[group_of]
    n_of = torch.tensor(sizes, dtype=torch.int64)[group_of]
    cell_g = torch.repeat_interleave(group_of, n_of)                                   # [cells]: row-major inside a group
    cell_i = torch.repeat_interleave(within, n_of)
    cell_start = (torch.cumsum(n_of, 0) - n_of)
    cell_j = torch.arange(U.numel(), dtype=torch.int64) - torch.repeat_interleave(cell_start, n_of)
    group_of, within, cell_g, cell_i, cell_j = (t.to(dev) for t in (group_of, within, cell_g, cell_i, cell_j))
    grid = torch.zeros((G, m, m), dtype=torch.float64, device=dev)
    grid[cell_g, cell_i, cell_j] = U
    valid = torch.zeros((G, m), dtype=torch.bool, device=dev)
    valid[group_of, within] = True
    w = valid.to(torch.float64)
    if weights is not None:
        given = torch.zeros((G, m), dtype=torch.float64, device=dev)
        given[group_of, within] = weights.to(dev)
        w = torch.where(given.sum(1, keepdim=True) > 0, given, w)
    total = w.sum(1, keepdim=True)
    value = (grid * w[:, None, :]).sum(2) / torch.where(total > 0, total, torch.ones_like(total))
    masked = torch.where(valid, value, torch.full_like(value, -1.0))                   # (chrF++ is never negative)
    top = masked.max(1, keepdim=True).values
    column = torch.arange(m, dtype=torch.int64, device=dev).expand(G, m)
    index = torch.where(valid & (masked == top), column, torch.full_like(column, m)).min(1).values
    index = torch.where(index < m, index, torch.full_like(index, -1))
    return value[group_of, within], index


def mbr_candidates(beams, k=None, alpha=0.6, weights="uniform", scale=1.0):
    """The candidates ``mbr_select`` weighs, per beam, and their weights: (groups, per-group weight lists or None for uniform)."""
    if weights not in ("uniform", "score", "stochastic"):
        raise ValueError("weights must be 'uniform', 'score' or 'stochastic', got %r" % (weights,))
    groups, w = [], []
    for beam in beams:
        if weights == "stochastic":
            from .search import stochastic_weights
            pairs = stochastic_weights(beam)[0]
            groups.append([hypothesis_tokens(h) for h, _ in pairs])
            w.append([float(x) for _, x in pairs])
            continue
        best = beam.get_k_best(beam.beam_size if k is None else k, alpha)
        groups.append([hypothesis_tokens(h) for h in best])
        w.append([])
        if weights == "score" and best:
            top = max(scale * h.score for h in best)
            e = [math.exp(scale * h.score - top) for h in best]
            w[-1] = [x / sum(e) for x in e]
    return groups, (None if weights == "uniform" else w)


def mbr_select(beams, k=None, alpha=0.6, weights="uniform", scale=1.0, beta=2.0, device="cuda"):
    """Per graph, the minimum-Bayes-risk choice among its candidates: the one with the highest expected sentence chrF++ against the
    candidates themselves (``expected_utility``); among equals the first.  The sibling of ``best_of_nbest`` for when there is no
    reference.  Candidates: ``beam.get_k_best(k, alpha)`` in that order (``k`` None: the beam's width) without <STR> / <END>;
    with ``weights="stochastic"`` the hypotheses ``search.stochastic_weights(beam)`` returns, in its order.  ``weights``:
      "uniform"     every candidate counts once -- the Monte-Carlo estimate for independent samples (search="sample"): a sentence
                    drawn twice is in the list twice and counts twice;
      "score"       w proportional to exp(scale * h.score), normalised per graph with the maximum subtracted, in fp64: for n-best lists;
      "stochastic"  the importance weights of a stochastic beam search (search="stochastic").
    Two ``pairwise`` launches for the whole batch (character order 6, chrF++ words order 2) and ONE host read.  Returns one
    (tokens, index, expected utility) per graph; (None, -1, nan) for a beam without candidates."""
    groups, per_group = mbr_candidates(beams, k, alpha, weights, scale)
    w = None if per_group is None else [x for ws in per_group for x in ws]
    sizes = [len(g) for g in groups]
    if not sum(sizes):
        return [(None, -1, float("nan")) for _ in beams]
    char, _ = pairwise(groups, "char", device=device)
    word, _ = pairwise(groups, "chrf_word", device=device)
    value, index = expected_utility(char, word, sizes, w, beta)
    first = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0).to(value.device)
    chosen = value[(first + index.clamp(min=0)).clamp(max=value.numel() - 1)]
    picked = torch.stack([index.to(torch.float64), chosen]).tolist()                # the one host read
    return [(groups[b][int(i)], int(i), u) if sizes[b] else (None, -1, float("nan")) for b, (i, u) in enumerate(zip(*picked))]


def accumulate(totals, stats_word4, stats_chrf_word2, stats_char6, beta=2.0):
    """Add one batch's device statistics (the same P pairs in all three) to ``totals`` (fp64 [N_TOTALS] on the device), in place."""
    totals[_W4] += stats_word4.sum(0).reshape(-1)
    totals[_W2] += stats_chrf_word2.sum(0).reshape(-1)
    totals[_C6] += stats_char6.sum(0).reshape(-1)
    totals[_HYP] += stats_word4[:, 0, 1].sum()
    totals[_REF] += stats_word4[:, 0, 2].sum()
    totals[_SENTS] += stats_word4.shape[0]
    totals[_SUMF] += sentence_chrf(stats_char6, stats_chrf_word2, beta).sum()
    return totals


def validation_metrics(totals, beta=2.0):
    """The dict of Trainer.validate from its totals (a list of N_TOTALS numbers, or a tensor): ``bleu``, ``bleu_precisions``,
    ``brevity_penalty``, ``chrf`` (corpus chrF++), ``chrf_avg`` (mean sentence chrF++), ``hyp_tokens``, ``ref_tokens``,
    ``sentences``.  NaN scores where nothing was scored."""
    t = torch.as_tensor(totals, dtype=torch.float64).cpu()
    n = int(t[_SENTS])
    if not n:
        nan = float("nan")
        return {"bleu": nan, "bleu_precisions": [nan] * 4, "brevity_penalty": nan, "chrf": nan, "chrf_avg": nan, "hyp_tokens": 0,
                "ref_tokens": 0, "sentences": 0}
    b = bleu(t[_W4].reshape(4, 3), t[_HYP], t[_REF])
    return {"bleu": float(b["bleu"]), "bleu_precisions": b["precisions"].tolist(), "brevity_penalty": float(b["brevity_penalty"]),
            "chrf": float(_chrf_of(t[_C6].reshape(6, 3), t[_W2].reshape(2, 3), beta)), "chrf_avg": float(t[_SUMF]) / n,
            "hyp_tokens": int(t[_HYP]), "ref_tokens": int(t[_REF]), "sentences": n}
