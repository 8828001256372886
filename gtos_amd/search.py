"""Batched beam search over the incremental decoder.

Selection rules of /root/reference/generator/search.py (Hypothesis / Beam.update / Beam.completed / get_k_best /
search_by_batch): per sentence, the top-k continuations of every live hypothesis are pooled, <UNK> continuations score
-inf, the pool is sorted by accumulated log-likelihood (stable, descending) and cut to ``beam_size - #finished``;
a continuation ending in <END> finishes its hypothesis (kept only if it has at least ``min_time_step`` tokens); a beam
stops when it holds ``beam_size`` finished hypotheses or after ``max_time_step`` steps; the final ranking divides the
score by ``(1 + len(seq)) ** alpha``.

What differs is the machinery: hypotheses carry no tensors.  The decoder state of ALL live hypotheses of ALL sentences
is one set of K/V-cache tensors ``[t, N, 2d]`` (gtos_amd.generator.Generator.decode_step_batched); a step returns, per beam,
the parent index of every surviving hypothesis, and the caches are re-gathered with ONE index_select per tensor
instead of being split into per-hypothesis slices and concatenated again.

``beam_search_device`` runs the same rules with the bookkeeping on the GPU as well (csrc/beam.hip): B sentences x k fixed
hypothesis slots, the graph memory gathered per slot once, preallocated caches reordered by a kernel, and the host reading one
flag every ``sync_every`` steps and the back-pointer / completion tables once at the end.

``groups`` / ``diversity`` turn either beam search into diverse (group) beam search (GroupBeam; on the device csrc/diverse.hip, the
rule in csrc/diverse_kernels.h): the k hypotheses of a sentence are cut into groups that search one after the other, each steered away
from the tokens the groups before it took at the same step.

``constraints`` turn either beam search into lexically constrained beam search with dynamic beam allocation (ConstrainedBeam; on the
device csrc/constrain.hip, the rule in csrc/constrain_kernels.h): tokens every finished hypothesis of a graph must hold.

``phrases`` do the same for constraints of several tokens (PhraseBeam; on the device csrc/phrase.hip, the rule in
csrc/phrase_kernels.h): every finished hypothesis holds every phrase as consecutive tokens, a phrase listed twice twice.

``coverage`` turns either beam search into coverage-penalised beam search (CoverageBeam; on the device csrc/coverage.hip, the rule in
csrc/coverage_kernels.h): every hypothesis accumulates the alignment weights of its steps over the graph nodes, and the selection
prefers hypotheses that have looked at all of them.

``avoid`` gives every search negative constraints (avoided_tokens; on the device csrc/avoid.hip, the rule in csrc/avoid_kernels.h):
words and phrases the output of a graph must not hold, banned in ll before the selection like a repeated n-gram.

``sample_device`` decodes by sampling instead (csrc/sample.hip): the same fixed slots, one independent sample per slot with
temperature / top-k / top-p, and Beam objects filled the same way.

``stochastic_beam_search_device`` samples WITHOUT replacement (csrc/sbs.hip, the rule in csrc/sbs_kernels.h): the slots, tables and
reorder of the beam search, the selection by perturbed values, k distinct sequences per graph with the quantities an estimator needs
(``stochastic_weights``).
"""
import math
import types

import torch

from . import ops
from .vocab import END, UNK, STR


class Hypothesis(object):
    __slots__ = ("seq", "score")

    def __init__(self, seq, score):
        self.seq = seq          # token strings, starting with <STR>
        self.score = score      # accumulated log-likelihood

    def is_completed(self):
        return self.seq[-1] == END

    def __len__(self):
        return len(self.seq)


class Beam(object):
    """The search frontier of one sentence."""

    def __init__(self, beam_size, min_time_step, max_time_step):
        self.beam_size, self.min_time_step, self.max_time_step = beam_size, min_time_step, max_time_step
        self.hypotheses = [Hypothesis([STR], 0.)]
        self.completed_hypotheses = []
        self.steps = 0

    def advance(self, last_steps):
        """last_steps[h] = [(token, log-likelihood), ...] for live hypothesis h.  Returns the parent index (into the
        old ``hypotheses``) of every hypothesis that stays alive, in their new order."""
        pool = []
        for parent, steps in enumerate(last_steps):
            base = self.hypotheses[parent].score
            for token, ll in steps:
                pool.append((parent, token, float('-inf') if token == UNK else base + ll))
        pool.sort(key=lambda c: c[2], reverse=True)                     # stable: ties keep (parent, rank) order
        return [c[0] for c in self.place(pool)]

    def place(self, ranked, make=lambda parent, seq, score: Hypothesis(seq, score)):
        """The placement every selection rule ends with (place_cut in csrc/beam_kernels.h).  ranked: the whole pool in its final order,
        entries (parent, token, score, ...).  Cuts it to ``beam_size - #finished``; in that order a continuation ending in <END> finishes
        its hypothesis (kept only if it has at least ``min_time_step`` tokens) and any other one is the next live hypothesis, built by
        make(parent, seq, score); counts the step.  Returns the entries that stay alive, in their new order."""
        alive, kept = [], []
        for c in ranked[:self.beam_size - len(self.completed_hypotheses)]:
            parent, token, score = c[:3]
            hyp = make(parent, self.hypotheses[parent].seq + [token], score)
            if hyp.is_completed():
                if len(hyp) - 2 >= self.min_time_step:
                    self.completed_hypotheses.append(hyp)
            else:
                alive.append(hyp)
                kept.append(c)
        self.hypotheses = alive
        self.steps += 1
        return kept

    def completed(self):
        return len(self.completed_hypotheses) >= self.beam_size or self.steps >= self.max_time_step

    def get_k_best(self, k, alpha):
        if not self.completed_hypotheses:
            self.completed_hypotheses = self.hypotheses
        self.completed_hypotheses.sort(key=lambda h: h.score / ((1 + len(h.seq)) ** alpha), reverse=True)
        return self.completed_hypotheses[:k]


class GroupBeam(Beam):
    """Diverse (group) beam search of one sentence (Vijayakumar et al., "Diverse Beam Search", Hamming penalty): the rule of
    csrc/diverse_kernels.h in Python.  ``groups`` Beam objects of width g = beam_size / groups, each a search of its own (steps,
    completions, done when it holds g completions or after max_time_step steps).  A step takes the groups in order with a list of the
    tokens chosen so far in this step: a group sorts its pool by ``score - diversity * chosen.count(token)`` (stable, descending),
    cuts and places it as Beam.advance does, and the tokens of its surviving hypotheses join the list.  A hypothesis's score stays
    the model's log-likelihood; the penalty only steers the selection.  ``hypotheses`` / ``completed_hypotheses`` are the groups'
    lists in group order, ``steps`` the most of any group."""

    def __init__(self, beam_size, min_time_step, max_time_step, groups, diversity):
        assert groups >= 1 and beam_size % groups == 0 and 0 <= diversity < float('inf')
        super().__init__(beam_size, min_time_step, max_time_step)
        self.diversity = float(diversity)
        self.groups = [Beam(beam_size // groups, min_time_step, max_time_step) for _ in range(groups)]
        self.last_parents = [None] * groups
        gather_groups(self, self.groups)

    def live_hypotheses(self):
        """The hypotheses the next step decodes: those of the groups that are not completed, in group order."""
        return [h for grp in self.groups if not grp.completed() for h in grp.hypotheses]

    def completed(self):
        return all(grp.completed() for grp in self.groups)

    def advance(self, last_steps):
        """last_steps[h] = [(token, log-likelihood), ...] (the top beam_size, in rank order) for h in live_hypotheses().  Returns the
        index into that list of the parent of every hypothesis of the next live_hypotheses(), in its order; ``last_parents[j]``
        keeps group j's parents as indices into its own old hypotheses (None for a group that was completed before the step)."""
        chosen, keep, pos = [], [], 0
        self.last_parents = [None] * len(self.groups)
        for j, grp in enumerate(self.groups):
            if grp.completed():
                continue
            n = len(grp.hypotheses)
            pool = []
            for parent, steps in enumerate(last_steps[pos:pos + n]):
                base = grp.hypotheses[parent].score
                for token, ll in steps:
                    score = float('-inf') if token == UNK else base + ll
                    pool.append((parent, token, score, score - self.diversity * chosen.count(token)))
            pool.sort(key=lambda c: c[3], reverse=True)                 # stable: ties keep (parent, rank) order
            kept = grp.place(pool)
            chosen.extend(token for _, token, _, _ in kept)             # no one reads the list before the next group does
            self.last_parents[j] = parents = [c[0] for c in kept]
            if not grp.completed():
                keep.extend(pos + p for p in parents)
            pos += n
        gather_groups(self, self.groups)
        return keep


def gather_groups(beam, groups):
    """``beam`` (width k) as the result of a grouped search over ``groups`` (Beam objects of width k / G): the attribute ``groups``,
    the groups' hypothesis lists concatenated in group order, the most steps of any group."""
    beam.groups = groups
    beam.hypotheses = [h for grp in groups for h in grp.hypotheses]
    beam.completed_hypotheses = [h for grp in groups for h in grp.completed_hypotheses]
    beam.steps = max(grp.steps for grp in groups)
    return beam


class ConstrainedBeam(Beam):
    """Lexically constrained beam search of one sentence with dynamic beam allocation (Post & Vilar 2018, single-token constraints):
    the rule of csrc/constrain_kernels.h in Python.  ``constraints``: distinct token strings every finished hypothesis must hold;
    ``met[h]``: the bit mask of those live hypothesis h has produced.  A step pools, per live hypothesis in order, its top-k candidates
    -- an <END> only when the hypothesis holds every constraint -- and then, per constraint in order, a forced candidate when the
    hypothesis lacks it, it is not among the top-k tokens and its log-likelihood is above -inf.  A candidate's bank is the number of
    constraints it would hold.  Within a bank candidates rank by score (stable, descending); the pool is ordered by that rank, then by
    bank, fullest first (the best of every bank, then the second best of every bank, ...), and cut and placed as Beam.advance does.
    Without constraints this is Beam."""

    def __init__(self, beam_size, min_time_step, max_time_step, constraints):
        super().__init__(beam_size, min_time_step, max_time_step)
        self.constraints = list(constraints)
        assert len(set(self.constraints)) == len(self.constraints), "constraints are a set of single tokens"
        self.met = [0]

    def advance(self, last_steps, forced):
        """last_steps as in Beam.advance; forced[h] = [(token, log-likelihood), ...], one entry per constraint in constraint order
        (the log-likelihood as the selection sees it, after repeat-n-gram blocking) for live hypothesis h; which of them enter the pool
        is decided here.  Returns the parents like Beam.advance."""
        full = (1 << len(self.constraints)) - 1
        bit = {w: 1 << i for i, w in enumerate(self.constraints)}
        pool = []                                                       # (parent, token, score, mask), in pool position order
        for parent, (steps, want) in enumerate(zip(last_steps, forced)):
            base, met = self.hypotheses[parent].score, self.met[parent]
            for token, ll in steps:
                if token == END and met != full:
                    continue
                pool.append((parent, token, float('-inf') if token == UNK else base + ll, met | bit.get(token, 0)))
            top = [token for token, _ in steps]
            for i, (token, ll) in enumerate(want):
                if (met >> i) & 1 or token in top or not ll > float('-inf'):
                    continue
                pool.append((parent, token, float('-inf') if token == UNK else base + ll, met | (1 << i)))
        banks = {}
        for c in pool:
            banks.setdefault(bin(c[3]).count("1"), []).append(c)
        ranked = []
        for bank, cands in banks.items():
            cands.sort(key=lambda c: c[2], reverse=True)                # stable: ties keep pool order
            ranked.extend((q, -bank, c) for q, c in enumerate(cands))
        ranked.sort(key=lambda x: x[:2])                                # (q, bank) is unique
        kept = self.place([c for _, _, c in ranked])
        self.met = [mask for _, _, _, mask in kept]
        return [c[0] for c in kept]


def phrase_step(phrases, met, open_, pos, token):
    """The transition of csrc/phrase_kernels.h on one token: (met, open, pos) -> (met, open, pos).  A token that continues the open
    phrase advances it and finishes it at its last token; any other token drops the progress and starts the lowest-index phrase whose
    bit is clear and whose first token it is, if any.  No failure links."""
    if open_ >= 0 and phrases[open_][pos] == token:
        return (met | 1 << open_, -1, 0) if pos + 1 == len(phrases[open_]) else (met, open_, pos + 1)
    for i, p in enumerate(phrases):
        if not (met >> i) & 1 and p[0] == token:
            return (met | 1 << i, -1, 0) if len(p) == 1 else (met, i, 1)
    return met, -1, 0


def phrase_state(seq, phrases):
    """(met, open, pos) of ``seq`` (a list of token strings, e.g. Hypothesis.seq) under ``phrases`` (a list of non-empty token-string
    lists): phrase_step over its tokens from (0, -1, 0).  met == (1 << len(phrases)) - 1: the sequence holds every phrase."""
    state = (0, -1, 0)
    for token in seq:
        state = phrase_step(phrases, *state, token)
    return state


class PhraseBeam(Beam):
    """Beam search of one sentence under phrase constraints: the rule of csrc/phrase_kernels.h in Python, ConstrainedBeam with
    constraints of several tokens.  ``phrases``: non-empty lists of token strings every finished hypothesis must hold as consecutive
    tokens, a phrase listed twice twice.  Live hypothesis h carries ``met[h]``, the bit mask of the phrases it has finished, and
    ``progress[h]`` = (open, pos): the phrase in progress and its tokens matched so far, (-1, 0) when none is (phrase_step).  A step
    pools, per live hypothesis in order, its top-k candidates -- an <END> only when every phrase is finished -- and then its forced
    candidates: the next token of the open phrase or, with none open, the first token of every unfinished phrase in order (once per
    token), each only when it is not among the top-k tokens and its log-likelihood is above -inf.  A candidate's bank is the number of
    constraint tokens its next state holds: the lengths of the finished phrases plus pos.  Order, cut and placement as in
    ConstrainedBeam.  With single-token phrases this is ConstrainedBeam, without phrases Beam."""

    def __init__(self, beam_size, min_time_step, max_time_step, phrases):
        super().__init__(beam_size, min_time_step, max_time_step)
        self.phrases = [list(p) for p in phrases]
        assert all(self.phrases), "a phrase holds at least one token"
        self.met, self.progress = [0], [(-1, 0)]

    def bank(self, met, open_, pos):
        return sum(len(p) for i, p in enumerate(self.phrases) if (met >> i) & 1) + pos

    def advance(self, last_steps, forced):
        """last_steps as in Beam.advance; forced[h]: for live hypothesis h a dict from every token of the phrases to its log-likelihood
        (as the selection sees it, after repeat-n-gram blocking); which of them enter the pool is decided here.  Returns the parents
        like Beam.advance."""
        full = (1 << len(self.phrases)) - 1
        pool = []                                                       # (parent, token, score, next state), in pool position order
        for parent, (steps, want) in enumerate(zip(last_steps, forced)):
            base, met, (open_, pos) = self.hypotheses[parent].score, self.met[parent], self.progress[parent]
            for token, ll in steps:
                if token == END and met != full:
                    continue
                pool.append((parent, token, float('-inf') if token == UNK else base + ll, phrase_step(self.phrases, met, open_, pos, token)))
            top = [token for token, _ in steps]
            if open_ >= 0:
                offers = [self.phrases[open_][pos]]
            else:
                offers = []
                for i, p in enumerate(self.phrases):
                    if not (met >> i) & 1 and p[0] not in offers:
                        offers.append(p[0])
            for token in offers:
                if token in top or not want[token] > float('-inf'):
                    continue
                pool.append((parent, token, float('-inf') if token == UNK else base + want[token],
                             phrase_step(self.phrases, met, open_, pos, token)))
        banks = {}
        for c in pool:
            banks.setdefault(self.bank(*c[3]), []).append(c)
        ranked = []
        for bank, cands in banks.items():
            cands.sort(key=lambda c: c[2], reverse=True)                # stable: ties keep pool order
            ranked.extend((q, -bank, c) for q, c in enumerate(cands))
        ranked.sort(key=lambda x: x[:2])                                # (q, bank) is unique
        kept = self.place([c for _, _, c in ranked])
        self.met = [c[3][0] for c in kept]
        self.progress = [c[3][1:] for c in kept]
        return [c[0] for c in kept]


class CoveredHypothesis(Hypothesis):
    __slots__ = ("cp", "coverage")

    def __init__(self, seq, score, cp, coverage):
        super().__init__(seq, score)
        self.cp = cp                    # coverage penalty of the step that produced the last token: sum_i log(min(coverage_i, 1) + 1e-12)
        self.coverage = coverage        # per graph node the alignment weight accumulated up to that step (0 at padded nodes)


class CoverageBeam(Beam):
    """Coverage-penalised beam search of one sentence (the GNMT coverage penalty, Wu et al. 2016, eq. 14): the rule of
    csrc/coverage_kernels.h in Python.  Beam with the pool sorted by ``score + beta * cp[parent]`` (stable, descending), cp[parent] the
    penalty of the parent's coverage with this step's alignment weights added; a hypothesis's score stays the model's log-likelihood,
    and it records the cp and the coverage it was selected with.  get_k_best ranks by GNMT's s(Y, X)."""

    def __init__(self, beam_size, min_time_step, max_time_step, beta):
        assert 0 <= beta < float('inf')
        super().__init__(beam_size, min_time_step, max_time_step)
        self.beta = float(beta)
        self.hypotheses = [CoveredHypothesis([STR], 0., 0., [])]

    def advance(self, last_steps, cp, coverage):
        """last_steps as in Beam.advance; cp[h] / coverage[h]: the penalty and the coverage (a list of floats) of live hypothesis h at
        this step.  Returns the parents like Beam.advance."""
        pool = []
        for parent, steps in enumerate(last_steps):
            base = self.hypotheses[parent].score
            for token, ll in steps:
                score = float('-inf') if token == UNK else base + ll
                pool.append((parent, token, score, score + self.beta * cp[parent]))
        pool.sort(key=lambda c: c[3], reverse=True)                     # stable: ties keep (parent, rank) order
        return [c[0] for c in self.place(pool, lambda parent, seq, score: CoveredHypothesis(seq, score, cp[parent], coverage[parent]))]

    def get_k_best(self, k, alpha):
        if not self.completed_hypotheses:
            self.completed_hypotheses = self.hypotheses
        self.completed_hypotheses.sort(key=lambda h: h.score / ((1 + len(h.seq)) ** alpha) + self.beta * h.cp, reverse=True)
        return self.completed_hypotheses[:k]


def constraints_met(seq, constraints):
    """How many distinct strings of ``constraints`` occur in ``seq`` (a list of token strings, e.g. Hypothesis.seq)."""
    have = set(seq)
    return sum(1 for w in set(constraints) if w in have)


def constraint_ids(model, local_idx2token, constraints):
    """Per graph the output ids of its constraint strings, by the convention of the n-gram code: the graph's copy id first, else the
    predictable-token vocabulary's id."""
    pv = model.vocabs['predictable_token']
    out = []
    for local, words in zip(local_idx2token, constraints):
        copy_id = {w: i for i, w in local.items()}
        out.append([copy_id[w] if w in copy_id else pv.token2idx(w) for w in words])
    return out


def banned_tokens(y, n):
    """The rule of csrc/ngram_kernels.h on a Python list: the tokens that would complete a repeated n-gram of y (n >= 1; n = 1: all of
    y), in position order, repeats included."""
    t = len(y)
    suffix = y[t - n + 1:] if n > 1 else []
    return [y[i + n - 1] for i in range(t - n + 1) if y[i:i + n - 1] == suffix]


def avoided_tokens(seq, entries):
    """The rule of csrc/avoid_kernels.h on Python lists: the last token of every entry of ``entries`` (non-empty token lists) whose
    other tokens ``seq`` ends in -- the tokens that would complete an avoid entry -- in entry order, repeats included."""
    seq = list(seq)
    t = len(seq)
    return [p[-1] for p in (list(p) for p in entries) if len(p) - 1 <= t and seq[t - len(p) + 1:] == p[:-1]]


def avoid_tables(ids):
    """The per-graph tables of gtos_avoid_block from the per-graph lists of avoid entries (non-empty lists of output ids): (pat, one
    row of ops.AVOID_TOKENS_MAX ids per graph, the entries concatenated, then -1; init; last; n_pos), init / last the bit masks of the
    entries' first / last positions as signed 64-bit integers.  ValueError for an empty entry or more positions than a row holds."""
    W = ops.AVOID_TOKENS_MAX
    signed = lambda x: x - (1 << 64) if x >> 63 else x
    pat, init, last, n_pos = [], [], [], []
    for b, entries in enumerate(ids):
        row, first, end = [], 0, 0
        for p in entries:
            if not len(p) or len(row) + len(p) > W:
                raise ValueError("avoid: graph %d holds an empty entry or more than %d ids" % (b, W))
            first |= 1 << len(row)
            row.extend(int(i) for i in p)
            end |= 1 << len(row) - 1
        pat.append(row + [-1] * (W - len(row)))
        init.append(signed(first))
        last.append(signed(end))
        n_pos.append(len(row))
    return pat, init, last, n_pos


def avoid_ids(model, local_idx2token, avoid):
    """Per graph the avoid entries (lists of token strings) as lists of output ids by constraint_ids' convention; None when ``avoid``
    is None or every graph's list is empty: nothing to avoid."""
    if avoid is None or not any(avoid):
        return None
    assert len(avoid) == len(local_idx2token), "avoid: one list per graph"
    return [constraint_ids(model, [local] * len(entries), entries) for local, entries in zip(local_idx2token, avoid)]


def beam_search(model, beams, memory, no_repeat_ngram=0, groups=1, diversity=0.0, constraints=None, coverage=None, phrases=None,
                avoid=None):
    """Runs all beams to completion.  ``model.decode_step_batched(tokens, state, memory, beam_of_hyp, offset, topk)`` ->
    (state, results); ``state`` is opaque here except that every tensor in it has the hypothesis axis at dim 1.  With
    ``no_repeat_ngram`` = n > 0 the call also gets, per hypothesis, the output ids that would repeat an n-gram of its tokens
    (banned_tokens on the strings after <STR>; string and id map one to one within a graph), which then score -inf.
    ``groups`` / ``diversity`` other than (1, 0.0): diverse beam search -- every (fresh) beam is searched as a GroupBeam of its
    settings and then holds that search's result (gather_groups).
    ``constraints`` (one list of token strings per graph, not with groups): lexically constrained search -- every (fresh) beam is
    searched as a ConstrainedBeam and then holds that search's lists, steps and ``met``; the decode call also gets ``want``, per
    hypothesis the output ids of its graph's constraints, and returns their log-likelihoods after banning.
    ``coverage`` = beta (not with groups or constraints): coverage-penalised search -- every (fresh) beam is searched as a
    CoverageBeam and then holds that search's lists and steps; the decode call also returns the alignment weights, the live hypotheses'
    coverage is one device tensor gathered with the caches, ops.coverage_step (the kernel of the device search, a hypothesis its own
    parent) adds and reduces it, and the host reads penalty and coverage in one copy per step.
    ``phrases`` (one list of token-string lists per graph, not with groups, constraints or coverage): phrase-constrained search --
    every (fresh) beam is searched as a PhraseBeam and then holds that search's lists, steps, ``met`` and ``progress``; ``want`` is per
    hypothesis the output ids of the distinct tokens of its graph's phrases.
    ``avoid`` (one list of entries per graph, an entry a non-empty list of token strings; with every other option): negative
    constraints -- per hypothesis the output ids that would complete an entry of its graph (avoided_tokens on the strings after
    <STR>) join the banned ids.  None, or every list empty: nothing of it."""
    device = memory['probe'].device
    if avoid is not None and not any(avoid):
        avoid = None
    assert avoid is None or len(avoid) == len(beams), "avoid: one list per graph"
    use_banned = bool(no_repeat_ngram) or avoid is not None
    state = None
    result = beams
    cov = None
    if coverage is not None:
        assert groups == 1 and diversity == 0.0 and constraints is None, "coverage: no groups, no constraints"
        beams = [CoverageBeam(b.beam_size, b.min_time_step, b.max_time_step, coverage) for b in beams]
        live = lambda beam: beam.hypotheses
        ones = torch.ones(3, dtype=torch.int32, device=device)
    elif phrases is not None:
        assert groups == 1 and diversity == 0.0 and constraints is None and len(phrases) == len(beams), "phrases: one list per graph, no groups, no constraints"
        beams = [PhraseBeam(b.beam_size, b.min_time_step, b.max_time_step, p) for b, p in zip(beams, phrases)]
        phrase_tokens = [sorted(set(w for p in ps for w in p)) for ps in phrases]
        cons_id = constraint_ids(model, memory['local_idx2token'], phrase_tokens)
        live = lambda beam: beam.hypotheses
    elif constraints is not None:
        assert groups == 1 and diversity == 0.0 and len(constraints) == len(beams), "constraints: one list per graph, no groups"
        beams = [ConstrainedBeam(b.beam_size, b.min_time_step, b.max_time_step, c) for b, c in zip(beams, constraints)]
        cons_id = constraint_ids(model, memory['local_idx2token'], constraints)
        live = lambda beam: beam.hypotheses
    elif groups != 1 or diversity != 0.0:
        beams = [GroupBeam(b.beam_size, b.min_time_step, b.max_time_step, groups, diversity) for b in beams]
        live = GroupBeam.live_hypotheses
    else:
        live = lambda beam: beam.hypotheses
    if use_banned:
        pv = model.vocabs['predictable_token']
        copy_id = [{w: i for i, w in local.items()} for local in memory['local_idx2token']]
    while True:
        owners, tokens, banned = [], [], []
        forced = None
        for bi, beam in enumerate(beams):
            if not beam.completed():
                for hyp in live(beam):
                    owners.append(bi)
                    tokens.append(hyp.seq[-1])
                    offset = len(hyp.seq) - 1
                    if use_banned:
                        words = banned_tokens(hyp.seq[1:], no_repeat_ngram) if no_repeat_ngram else []
                        if avoid is not None:
                            words = words + avoided_tokens(hyp.seq[1:], avoid[bi])
                        banned.append([copy_id[bi][w] if w in copy_id[bi] else pv.token2idx(w) for w in words])
        if not owners:
            break
        beam_of_hyp = torch.tensor(owners, dtype=torch.int64, device=device)
        if constraints is not None or phrases is not None:
            state, results, lls = model.decode_step_batched(tokens, state, memory, beam_of_hyp, offset, beams[0].beam_size,
                                                            banned if use_banned else None, want=[cons_id[bi] for bi in owners])
            if phrases is not None:
                forced = [dict(zip(phrase_tokens[bi], row)) for bi, row in zip(owners, lls)]
            else:
                forced = [list(zip(constraints[bi], row)) for bi, row in zip(owners, lls)]
        elif coverage is not None:
            state, results, align = model.decode_step_batched(tokens, state, memory, beam_of_hyp, offset, beams[0].beam_size,
                                                              banned if use_banned else None, want_align=True)
            pad = memory['graph_padding_mask'].index_select(1, beam_of_hyp).contiguous()
            prev, cov = torch.zeros_like(align) if cov is None else cov, torch.empty_like(align)
            cp = torch.empty(len(owners), dtype=torch.float64, device=device)
            ops.coverage_step(offset, 1, align, pad, None, prev, cov, cp, ones)
            rows = torch.cat([cp.unsqueeze(1), cov.masked_fill(pad.t(), 0.).double()], 1).tolist()       # the step's one extra read
        elif use_banned:
            state, results = model.decode_step_batched(tokens, state, memory, beam_of_hyp, offset, beams[0].beam_size, banned)
        else:
            state, results = model.decode_step_batched(tokens, state, memory, beam_of_hyp, offset, beams[0].beam_size)
        # hand every beam its slice of the results; collect the flat parent index of each survivor
        keep, pos = [], 0
        for bi, beam in enumerate(beams):
            if beam.completed():
                continue
            n = len(live(beam))
            if coverage is not None:
                parents = beam.advance(results[pos:pos + n], [r[0] for r in rows[pos:pos + n]], [r[1:] for r in rows[pos:pos + n]])
            elif forced is None:
                parents = beam.advance(results[pos:pos + n])
            else:
                parents = beam.advance(results[pos:pos + n], forced[pos:pos + n])
            if not beam.completed():
                keep.extend(pos + p for p in parents)
            pos += n
        if not keep:
            break
        idx = torch.tensor(keep, dtype=torch.int64, device=device)
        state = {k: [c.index_select(1, idx) for c in v] for k, v in state.items()}
        if coverage is not None:
            cov = cov.index_select(0, idx)
    if result is not beams:
        for beam, run in zip(result, beams):
            if coverage is not None:
                beam.hypotheses, beam.completed_hypotheses, beam.steps = run.hypotheses, run.completed_hypotheses, run.steps
            elif phrases is not None:
                beam.hypotheses, beam.completed_hypotheses, beam.steps = run.hypotheses, run.completed_hypotheses, run.steps
                beam.met, beam.progress = run.met, run.progress
            elif constraints is not None:
                beam.hypotheses, beam.completed_hypotheses, beam.steps, beam.met =run.hypotheses, run.completed_hypotheses, run.steps, run.met
            else:
                gather_groups(beam, run.groups)
    return result


def _arena(dtype, cuts, dev):
    """One zeroed allocation cut into named views, so that the host reads all of them with one copy.  ``cuts``: (name, shape, init),
    init a number, or a tuple that every row of the last axis starts as.  -> ({name: view}, read), read() -> {name: flat list}."""
    sizes = [math.prod(shape) for _, shape, _ in cuts]
    flat = torch.zeros(sum(sizes), dtype=dtype, device=dev)
    views = {}
    for (name, shape, init), part in zip(cuts, torch.split(flat, sizes)):
        views[name] = part.view(shape)
        if isinstance(init, tuple):
            for j, x in enumerate(init):
                if x:
                    views[name][..., j] = x
        elif init:
            views[name].fill_(init)
    return views, lambda: {cut[0]: part.tolist() for cut, part in zip(cuts, torch.split(flat.cpu(), sizes))}


def _slot_decode(who, model, memory, beams, sync_every, stats, copies, live0, layout, step, fill, no_repeat_ngram=0, taken=None,
                 want_align=False, extra_reads=0, avoid=None):
    """The fixed-slot decode loop (the contract of csrc/slot_kernels.h) behind ``who``, a public function: B graphs x k slots, N = B*k,
    slot s belongs to graph s // k, the graph memory gathered per slot once, every slot decoded every step (a dead slot on the
    padding input), the input of step t + 1 written by step t's kernels into the other of two buffers.  The loop reads the device's
    continue flag ``active`` every ``sync_every`` steps (steps past the end are no-ops) and the tables once at the end, one copy per
    arena; ``stats`` (a dict, optional) receives the decoder steps launched and the host reads made.  A decoder supplies
      copies: buffers per self-attention cache (Generator.slot_caches), 2 when step() reorders one into the other;
      live0: slots per graph that start on <STR>, the rest on the padding input (None: all k); a pair (g, n): the first n slots of
        every g consecutive ones;
      layout(d) -> (int32 cuts, fp64 cuts) of its tables, as _arena takes them (also the place to hang tables of its own on d);
        d holds B, k, N, min_t, max_t, V, tot, local, tab (Generator.search_tables) and then arr, the views by name with ``active``;
      step(d, t, ll, cur, nxt, tok_out, char_out): step t's launches after the decoder's, ll [N, tot] fp32; cur / nxt: the caches
        read and those step t + 1 reads (the same with one copy); tok_out [N] / char_out [N,C]: step t + 1's input, for EVERY slot;
      fill(beams, k, token_string=, **tables) -> the Beam objects from its tables as flat lists; token_string(b, id) -> the string;
      taken(d, t) -> (parent [N] int32 or None, token [N] int32): what every slot took at step t (a negative entry: a dead slot), for
        ``no_repeat_ngram`` = n > 0, the rule of csrc/ngram_kernels.h: two int32 [N, max_t] history buffers alternate by step parity and
        ops.ngram_block bans, in ll, the columns that would repeat an n-gram, at every step t >= 1 before step().  n = 0: nothing of it.
      want_align: the decoder also returns the slots' alignment weights [N, n] fp32, which step() finds as d.align;
      extra_reads: host reads fill() makes beyond the two arenas, counted in stats['host_reads'];
      avoid: per graph a list of avoid entries (non-empty lists of output ids, avoid_ids), the rule of csrc/avoid_kernels.h: the
        per-graph tables (avoid_tables) are built once, two int64 [N] matcher-state buffers alternate by step parity and
        ops.avoid_block bans, in ll, the columns that would complete an entry, at every step t >= 0 before step() (with taken(d, t - 1)
        for t >= 1).  None, or every list empty: nothing of it."""
    B = len(beams)
    if not B:
        return beams
    k, min_t, max_t = beams[0].beam_size, beams[0].min_time_step, beams[0].max_time_step
    for beam in beams:
        assert (beam.beam_size, beam.min_time_step, beam.max_time_step) == (k, min_t, max_t), "beams of one search share their settings"
        assert beam.steps == 0 and len(beam.hypotheses) == 1 and not beam.completed_hypotheses, who + " takes fresh beams"
    n_steps, reads = 0, 0
    if max_t <= 0:                                          # every beam is complete before the first step
        if stats is not None:
            stats.update(steps=0, host_reads=0)
        return beams
    dev = memory['probe'].device
    N = B * k
    mem = slot_memory(memory, B, k)
    local = memory['local_idx2token']
    V = model.vocabs['predictable_token'].size
    tot = max(int(memory['tot_ext']), V)
    tab = model.search_tables(local, tot)
    C = tab['C']
    d = types.SimpleNamespace(B=B, k=k, N=N, min_t=min_t, max_t=max_t, V=V, tot=tot, local=local, tab=tab)
    int_cuts, dbl_cuts = layout(d)
    ints, read_ints = _arena(torch.int32, [('active', (3,), (1, 0, 0))] + int_cuts, dev)
    dbls, read_dbls = _arena(torch.float64, dbl_cuts, dev)
    d.arr = dict(ints, **dbls)
    caches = model.slot_caches(max_t, N, copies=copies)
    caches = [[c[i] for c in caches] for i in range(copies)]
    tok = [torch.full((1, N), tab['dead_tok'], dtype=torch.int64, device=dev) for _ in range(2)]
    chars = [tab['dead_char'].expand(1, N, C).contiguous() for _ in range(2)]
    width, live0 = live0 if isinstance(live0, tuple) else (k, live0)
    tok[0].view(B, k // width, width)[:, :, :live0] = tab['start_tok']
    chars[0].view(B, k // width, width, C)[:, :, :live0] = tab['start_char']
    hist = [torch.zeros((N, max_t), dtype=torch.int32, device=dev) for _ in range(2)] if no_repeat_ngram else None
    avo = None
    if avoid is not None and any(avoid):
        if len(avoid) != B or any(not 0 <= i < tot for entries in avoid for p in entries for i in p):
            raise ValueError("avoid: one list of entries per graph, each id an output id of the batch")
        pat, init, last, n_pos = avoid_tables(avoid)
        avo = types.SimpleNamespace(pat=torch.tensor(pat, dtype=torch.int32).to(dev), init=torch.tensor(init, dtype=torch.int64).to(dev),
                                    last=torch.tensor(last, dtype=torch.int64).to(dev), n_pos=torch.tensor(n_pos, dtype=torch.int32).to(dev),
                                    state=[torch.zeros(N, dtype=torch.int64, device=dev) for _ in range(2)])
    for t in range(max_t):
        cur, nxt = t % 2, (t + 1) % 2
        if want_align:
            ll, d.align = model.decode_slots((tok[cur], chars[cur]), caches[cur % copies], mem, t, want_align=True)
        else:
            ll = model.decode_slots((tok[cur], chars[cur]), caches[cur % copies], mem, t)
        if no_repeat_ngram and t:
            parent, token = taken(d, t - 1)
            ops.ngram_block(t, k, no_repeat_ngram, ll, parent, token, hist[nxt], hist[cur], ints['active'])
        if avo is not None:
            parent, token = taken(d, t - 1) if t else (None, None)
            ops.avoid_block(t, k, ll, parent, token, avo.pat, avo.init, avo.last, avo.n_pos, avo.state[nxt], avo.state[cur], ints['active'])
        step(d, t, ll, caches[cur % copies], caches[nxt % copies], tok[nxt][0], chars[nxt][0])
        n_steps += 1
        if (t + 1) % sync_every == 0 and t + 1 < max_t:
            reads += 1
            if not int(ints['active'][(t + 1) % 3].item()):
                break
    host = dict(read_ints(), **read_dbls())
    del host['active']
    reads += 2 + extra_reads
    if stats is not None:
        stats.update(steps=n_steps, host_reads=reads)
    pv = model.vocabs['predictable_token']
    return fill(beams, k, token_string=lambda b, i: local[b][i] if i in local[b] else pv.idx2token(i), **host)


def _plain_cuts(d, rows, ints=(), dbls=()):
    """The int32 and fp64 cuts (a layout() result) of the tables every beam route keeps, in the format fill_beams reads: ``rows`` state
    rows of (steps, #completed, #live, done) with slot 0 live, the back-pointer rows and the completion tables; then the route's own."""
    return ([('state', (rows, 4), (0, 0, 1, 0)), ('bp_parent', (d.max_t, d.N), -1), ('bp_token', (d.max_t, d.N), -1),
             ('comp_step', (d.B, d.k), 0), ('comp_parent', (d.B, d.k), 0)] + list(ints),
            [('slot_score', (d.N,), 0), ('comp_score', (d.B, d.k), 0)] + list(dbls))


def _plain_tables(d):
    """The tables of _plain_cuts as every ops.*_advance takes them after topv / topi, up to ``active``"""
    a, tab = d.arr, d.tab
    return (tab['flag_shared'], tab['flag_local'], a['slot_score'], a['state'], a['bp_parent'], a['bp_token'], a['comp_step'],
            a['comp_parent'], a['comp_score'])


def _plain_reorder(d, t, cur, nxt, tok_out, char_out, width=None):
    """The reorder that ends a step of every beam route: gtos_beam_reorder, or gtos_diverse_reorder for groups of ``width`` slots"""
    a, tab = d.arr, d.tab
    rest = (a['bp_parent'], a['bp_token'], a['state'], a['active'], d.V, d.tot, tab['tok_shared'], tab['tok_local'], tab['char_shared'],
            tab['char_local'], tab['dead_tok'], tab['dead_char'], tok_out, char_out)
    if width is None:
        ops.beam_reorder(cur, nxt, t, d.k, *rest)
    else:
        ops.diverse_reorder(cur, nxt, t, d.k, width, *rest)


def _taken(d, t):
    """_slot_decode's ``taken`` of every beam route: row t of the back-pointer tables"""
    return d.arr['bp_parent'][t], d.arr['bp_token'][t]


def _beam_route(model, memory, beams, sync_every, stats, no_repeat_ngram, layout, step, fill, live0=1, fresh=None, **more):
    """_slot_decode for a beam route (two cache copies, _taken); a beam no step ran for (max_time_step <= 0) is then left as the
    route's fill leaves a beam: fresh(beam)."""
    _slot_decode("beam_search_device", model, memory, beams, sync_every, stats, 2, live0, layout, step, fill, no_repeat_ngram, _taken, **more)
    for beam in beams:
        if fresh is not None and beam.steps == 0:
            fresh(beam)
    return beams


def beam_search_device(model, memory, beams, sync_every=8, stats=None, no_repeat_ngram=0, groups=1, diversity=0.0, grouped=None,
                       constraints=None, constrained=None, coverage=None, covered=None, phrases=None, phrased=None, avoid=None):
    """beam_search with selection, bookkeeping and state reorder on the device.  ``model``: a Generator (search_tables, slot_caches,
    decode_slots); ``memory``: per graph, as Generator.work builds it; ``beams``: fresh Beam objects of one (beam size, min, max
    steps), one per graph.  Slot s of the N = B*k slots belongs to graph s // k; at step 0 only slot 0 of each beam is live; dead slots
    keep computing on the padding input and zero cache rows, their candidates are ignored.  The continue flag is "some not-done
    beam has a live slot"; ``sync_every``, ``stats`` and ``no_repeat_ngram`` as in _slot_decode.  The Beam objects are filled as beam_search leaves them
    (hypotheses, completed_hypotheses in append order, steps).
    ``groups`` / ``diversity`` other than (1, 0.0): diverse beam search (the rule of csrc/diverse_kernels.h, GroupBeam on the host) --
    the k slots of a graph are ``groups`` groups of k // groups, slot 0 of every group live at step 0, per-group state, and the
    advance and the reorder of a step are gtos_diverse_advance / gtos_diverse_reorder; a beam then holds what gather_groups leaves.
    ``grouped`` = True takes that route whatever the two settings are (groups = 1 must give the plain search's beams).
    ``constraints`` (one list of token strings per graph, not with groups): lexically constrained search (the rule of
    csrc/constrain_kernels.h, ConstrainedBeam on the host) -- the plain tables plus the slots' masks ``met`` and the constraint ids, a
    step's advance being gtos_constrain_advance between the plain top-k and the plain reorder; a beam then also carries ``met``, the
    masks of its live hypotheses.  ``constrained`` = True takes that route even without constraints (it must give the plain search's
    beams).
    ``coverage`` = beta (not with groups or constraints): coverage-penalised search (the rule of csrc/coverage_kernels.h, CoverageBeam
    on the host) -- per step gtos_coverage_step before the plain top-k and gtos_coverage_advance as the advance, the plain reorder; a
    beam's hypotheses are then CoveredHypothesis objects.  ``covered`` = True takes that route even without a penalty (beta = 0: it
    must give the plain search's beams, with the coverage reported).
    ``phrases`` (one list of token-string lists per graph, not with groups, constraints or coverage): phrase-constrained search (the
    rule of csrc/phrase_kernels.h, PhraseBeam on the host) -- the plain tables plus the slots' packed states and the phrase ids, a step's
    advance being gtos_phrase_advance between the plain top-k and the plain reorder; a beam then also carries ``met`` and ``progress``
    of its live hypotheses.  ``phrased`` = True takes that route even without phrases (it must give the plain search's beams).
    ``avoid`` (one list of entries per graph, an entry a non-empty list of token strings; with every route): negative constraints (the
    rule of csrc/avoid_kernels.h, avoided_tokens on the host) -- one gtos_avoid_block per step in front of the route's selection, as
    _slot_decode describes; None, or every list empty: the route's calls as they are without."""
    avoid = avoid_ids(model, memory['local_idx2token'], avoid)
    if phrased is None:
        phrased = phrases is not None
    if grouped is None:
        grouped = groups != 1 or diversity != 0.0
    if constrained is None:
        constrained = constraints is not None
    if covered is None:
        covered = coverage is not None
    if phrased:
        assert not grouped and not constrained and not covered, "phrases do not combine with groups, constraints or coverage"
        return _phrase_search_device(model, memory, beams, sync_every, stats, no_repeat_ngram, phrases, avoid)
    if covered:
        assert not grouped and not constrained, "coverage does not combine with groups or constraints"
        return _covered_search_device(model, memory, beams, sync_every, stats, no_repeat_ngram, 0.0 if coverage is None else float(coverage), avoid)
    if constrained:
        assert not grouped, "constraints do not combine with groups"
        return _constrained_search_device(model, memory, beams, sync_every, stats, no_repeat_ngram, constraints, avoid)
    if grouped:
        return _group_search_device(model, memory, beams, sync_every, stats, no_repeat_ngram, groups, float(diversity), avoid)

    def step(d, t, ll, cur, nxt, tok_out, char_out):
        topv, topi = ops.beam_topk(ll, d.k)
        ops.beam_advance(t, d.k, d.V, d.tot, d.min_t, d.max_t, topv, topi, *_plain_tables(d), d.arr['active'])
        _plain_reorder(d, t, cur, nxt, tok_out, char_out)
    return _beam_route(model, memory, beams, sync_every, stats, no_repeat_ngram, lambda d: _plain_cuts(d, d.B), step, fill_beams, avoid=avoid)


def _group_search_device(model, memory, beams, sync_every, stats, no_repeat_ngram, G, diversity, avoid=None):
    """The grouped route of beam_search_device: the same launch sequence per step (one top-k over the whole k, one advance, one
    reorder, the n-gram kernel when asked -- parents are global slot indices, so it works as it is) and the same host reads."""
    if beams:
        assert G >= 1 and beams[0].beam_size % G == 0 and 0 <= diversity < float('inf'), "groups divide the beam size; diversity is finite and >= 0"
        g = beams[0].beam_size // G

    def step(d, t, ll, cur, nxt, tok_out, char_out):
        topv, topi = ops.beam_topk(ll, d.k)
        ops.diverse_advance(t, d.k, G, diversity, d.V, d.tot, d.min_t, d.max_t, topv, topi, *_plain_tables(d), d.arr['active'])
        _plain_reorder(d, t, cur, nxt, tok_out, char_out, width=g)
    fill = lambda beams_, k, **tables: fill_beams(beams_, k, groups=G, **tables)
    fresh = lambda beam: gather_groups(beam, [Beam(g, beam.min_time_step, beam.max_time_step) for _ in range(G)])
    return _beam_route(model, memory, beams, sync_every, stats, no_repeat_ngram, lambda d: _plain_cuts(d, d.B * G), step, fill,
                       live0=(g, 1) if beams else 1, fresh=fresh, avoid=avoid)


def _constrained_search_device(model, memory, beams, sync_every, stats, no_repeat_ngram, constraints, avoid=None):
    """The constrained route of beam_search_device: the plain launch sequence per step with gtos_constrain_advance as the advance (it
    reads ll after the n-gram kernel, so a banned constraint is not forced) and the same host reads."""
    if constraints is None:
        constraints = [[] for _ in beams]
    assert len(constraints) == len(beams), "constraints: one list per graph"

    def layout(d):
        ids = constraint_ids(model, d.local, constraints)
        width = max([len(x) for x in ids] + [0])
        if width > ops.CONSTRAIN_MAX or any(not 0 <= i < d.tot for x in ids for i in x):
            raise ValueError("constraints: at most %d per graph, each an output id of the batch" % ops.CONSTRAIN_MAX)
        d.cons = torch.tensor([x + [-1] * (width - len(x)) for x in ids], dtype=torch.int32).view(d.B, width).to(memory['probe'].device)
        return _plain_cuts(d, d.B, ints=[('met', (2, d.N), 0)])

    def step(d, t, ll, cur, nxt, tok_out, char_out):
        topv, topi = ops.beam_topk(ll, d.k)
        ops.constrain_advance(t, d.k, d.V, d.tot, d.min_t, d.max_t, topv, topi, ll, d.cons, *_plain_tables(d), d.arr['met'], d.arr['active'])
        _plain_reorder(d, t, cur, nxt, tok_out, char_out)

    def fill(beams_, k, met, state, **tables):
        fill_beams(beams_, k, state=state, **tables)
        N = len(beams_) * k
        for b, beam in enumerate(beams_):                    # the row the beam's last advance wrote: step t writes row (t + 1) % 2
            steps, nlive = state[4 * b], state[4 * b + 2]
            beam.met = [met[(steps % 2) * N + b * k + j] for j in range(nlive)] if steps else [0]
        return beams_
    return _beam_route(model, memory, beams, sync_every, stats, no_repeat_ngram, layout, step, fill,
                       fresh=lambda beam: setattr(beam, 'met', [0]), avoid=avoid)


def _phrase_search_device(model, memory, beams, sync_every, stats, no_repeat_ngram, phrases, avoid=None):
    """The phrase route of beam_search_device: the plain launch sequence per step with gtos_phrase_advance as the advance (it reads ll
    after the n-gram kernel, so a banned token is not forced) and the same host reads."""
    if phrases is None:
        phrases = [[] for _ in beams]
    assert len(phrases) == len(beams), "phrases: one list per graph"

    def layout(d):
        ids = [constraint_ids(model, [local] * len(ps), ps) for local, ps in zip(d.local, phrases)]
        Cw = max([len(x) for x in ids] + [0])
        Lw = max([len(p) for x in ids for p in x] + [1])
        if (Cw > ops.PHRASE_MAX or Lw > ops.PHRASE_LEN_MAX or any(not p for x in ids for p in x)
                or any(sum(len(p) for p in x) > ops.PHRASE_TOKENS_MAX for x in ids) or any(not 0 <= i < d.tot for x in ids for p in x for i in p)):
            raise ValueError("phrases: at most %d per graph, each of 1 to %d output ids of the batch, at most %d ids per graph"
                             % (ops.PHRASE_MAX, ops.PHRASE_LEN_MAX, ops.PHRASE_TOKENS_MAX))
        rows = [[p + [-1] * (Lw - len(p)) for p in x] + [[-1] * Lw] * (Cw - len(x)) for x in ids]
        d.phr = torch.tensor(rows, dtype=torch.int32).view(d.B, Cw, Lw).to(memory['probe'].device)
        return _plain_cuts(d, d.B, ints=[('pst', (2, d.N), 0)])

    def step(d, t, ll, cur, nxt, tok_out, char_out):
        topv, topi = ops.beam_topk(ll, d.k)
        ops.phrase_advance(t, d.k, d.V, d.tot, d.min_t, d.max_t, topv, topi, ll, d.phr, *_plain_tables(d), d.arr['pst'], d.arr['active'])
        _plain_reorder(d, t, cur, nxt, tok_out, char_out)

    def fresh(beam):
        beam.met, beam.progress = [0], [(-1, 0)]

    def fill(beams_, k, pst, state, **tables):
        fill_beams(beams_, k, state=state, **tables)
        N = len(beams_) * k
        for b, beam in enumerate(beams_):                    # the row the beam's last advance wrote: step t writes row (t + 1) % 2
            steps, nlive = state[4 * b], state[4 * b + 2]
            words = [pst[(steps % 2) * N + b * k + j] for j in range(nlive)] if steps else [0]
            beam.met = [w & 0xFFFF for w in words]
            beam.progress = [((w >> 16 & 31) - 1, w >> 21 & 31) for w in words]
        return beams_
    return _beam_route(model, memory, beams, sync_every, stats, no_repeat_ngram, layout, step, fill, fresh=fresh, avoid=avoid)


def _covered_search_device(model, memory, beams, sync_every, stats, no_repeat_ngram, beta, avoid=None):
    """The coverage route of beam_search_device.  Per step: the decoder (which also hands out its alignment weights),
    gtos_ngram_block if asked, gtos_coverage_step (coverage and penalty of every slot, two [N, n] buffers alternating by step parity as
    the n-gram histories do), gtos_beam_topk, gtos_coverage_advance, gtos_beam_reorder.  The fp64 arena also holds slot_cp / comp_cp;
    the fp32 tables slot_cov [N, n] / comp_cov [B, k, n] cost one more host read at the end."""
    assert 0 <= beta < float('inf'), "coverage: a finite weight >= 0"

    tables = types.SimpleNamespace()                         # the fp32 tables and the step's scratch, which no arena holds

    def layout(d):
        c, mask = tables, memory['graph_padding_mask']
        n, dev = mask.shape[0], mask.device
        c.pad = mask.repeat_interleave(d.k, dim=1).contiguous()              # [n, N]: slot s reads graph s // k
        c.cov = [torch.zeros((d.N, n), dtype=torch.float32, device=dev) for _ in range(2)]
        c.cp = torch.zeros(d.N, dtype=torch.float64, device=dev)
        c.slot_cov = torch.zeros((d.N, n), dtype=torch.float32, device=dev)
        c.comp_cov = torch.zeros((d.B, d.k, n), dtype=torch.float32, device=dev)
        return _plain_cuts(d, d.B, dbls=[('slot_cp', (d.N,), 0), ('comp_cp', (d.B, d.k), 0)])

    def step(d, t, ll, cur, nxt, tok_out, char_out):
        a, c = d.arr, tables
        ops.coverage_step(t, d.k, d.align, c.pad, a['bp_parent'][t - 1] if t else None, c.cov[(t + 1) % 2], c.cov[t % 2], c.cp, a['active'])
        topv, topi = ops.beam_topk(ll, d.k)
        ops.coverage_advance(t, d.k, beta, d.V, d.tot, d.min_t, d.max_t, topv, topi, *_plain_tables(d), c.cp, c.cov[t % 2], a['slot_cp'],
                             a['comp_cp'], c.comp_cov, c.slot_cov, a['active'])
        _plain_reorder(d, t, cur, nxt, tok_out, char_out)

    def fill(beams_, k, slot_cp, comp_cp, state, **plain):
        c, N = tables, len(beams_) * k
        keep = (~c.pad.t()).to(torch.float32)                # [N, n]: 0 at the padded nodes of the slot's graph
        rows = torch.cat([c.slot_cov * keep, c.comp_cov.view(N, -1) * keep]).tolist()           # a completion row b*k + j is of graph b too
        fill_beams(beams_, k, state=state, **plain)
        for b, beam in enumerate(beams_):
            if not state[4 * b]:
                continue
            beam.completed_hypotheses = [CoveredHypothesis(h.seq, h.score, comp_cp[b * k + j], rows[N + b * k + j])
                                         for j, h in enumerate(beam.completed_hypotheses)]
            beam.hypotheses = [CoveredHypothesis(h.seq, h.score, slot_cp[b * k + j], rows[b * k + j]) for j, h in enumerate(beam.hypotheses)]
        return beams_
    return _beam_route(model, memory, beams, sync_every, stats, no_repeat_ngram, layout, step, fill, want_align=True, extra_reads=1,
                       fresh=lambda beam: setattr(beam, 'hypotheses', [CoveredHypothesis([STR], 0., 0., [])]), avoid=avoid)


def slot_memory(memory, B, k):
    """The graph memory of Generator.work (B graphs) gathered once per fixed slot: slot s reads graph s // k."""
    graph_of = torch.arange(B * k, device=memory['probe'].device) // k
    sel = lambda v: v.index_select(1, graph_of)
    return {'graph_padding_mask': sel(memory['graph_padding_mask']), 'cp_seq': sel(memory['cp_seq']), 'probe': sel(memory['probe']),
            'tot_ext': memory['tot_ext'], 'snt_ext_kv': [sel(v) for v in memory['snt_ext_kv']],
            'inf_ext_kv': [sel(v) for v in memory['inf_ext_kv']], 'align_kv': sel(memory['align_kv'])}


def fill_beams(beams, k, state, bp_parent, bp_token, comp_step, comp_parent, slot_score, comp_score, token_string, groups=None):
    """The Beam objects of a fixed-slot search from its tables (flat lists): state [B*4] (steps, #completed, #live, done),
    bp_parent / bp_token [T*N] (row t: parent slot and token id of every slot after step t), comp_step / comp_parent / comp_score
    [B*k] (completions in append order), slot_score [N]; token_string(b, id) -> the string of an output id of graph b.
    ``groups`` = G (a grouped search, state [B*G*4]): beam b is gather_groups over G Beam objects of width k // G, group j filled from
    state row b*G + j, slots and completion rows b*k + j*(k // G) onwards."""
    N = len(beams) * k

    def fill(beam, b, q, width):
        """``beam`` (width ``width``) of graph b from state row q, slots and completion rows q*width onwards"""
        steps, ncomp, nlive = state[4 * q:4 * q + 3]
        if steps == 0:
            return

        def seq_of(slot, tl):
            ids = []
            while tl >= 0:
                ids.append(bp_token[tl * N + slot])
                slot = bp_parent[tl * N + slot]
                tl -= 1
            return [STR] + [token_string(b, i) for i in reversed(ids)]
        at = q * width
        beam.completed_hypotheses = [Hypothesis(seq_of(comp_parent[at + j], comp_step[at + j] - 1) + [END], comp_score[at + j])
                                     for j in range(ncomp)]
        beam.hypotheses = [Hypothesis(seq_of(at + j, steps - 1), slot_score[at + j]) for j in range(nlive)]
        beam.steps = steps
    for b, beam in enumerate(beams):
        if groups is None:
            fill(beam, b, b, k)
        else:
            subs = [Beam(k // groups, beam.min_time_step, beam.max_time_step) for _ in range(groups)]
            for j, sub in enumerate(subs):
                fill(sub, b, b * groups + j, k // groups)
            gather_groups(beam, subs)
    return beams


def sample_bits(seed, graph, sample, t, cols):
    """The 64-bit counter hash of csrc/sample_kernels.h for the columns ``cols`` of one (seed, graph, sample, step) row, as numpy
    uint64: draw i of a splitmix64 stream seeded with s is ``synth.SplitMix64(s).u64(i + 1)[i]``; the row's key is three chained
    draws (graph, sample, step) from the seed, and column c is draw c of the stream seeded with that key."""
    import numpy as np
    from .synth import SplitMix64
    key = int(seed) & 0xFFFFFFFFFFFFFFFF
    for w in (graph, sample, t):
        key = int(SplitMix64(key).u64(int(w) + 1)[int(w)])
    cols = np.asarray(cols, dtype=np.int64)
    return SplitMix64(key).u64(int(cols.max()) + 1 if cols.size else 0)[cols]


def sample_device(model, memory, beams, temperature, top_k, top_p, seed, sync_every=8, stats=None, no_repeat_ngram=0, avoid=None,
                  min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """Sampling decode on the device (csrc/sample.hip), the counterpart of beam_search_device with the same ``memory``: every graph
    gets ``beam_size`` independent samples in fixed slots (slot s is sample s % k of graph s // k), each drawing its next token by the
    rule of csrc/sample_kernels.h (temperature, top_k, top_p; <UNK>, other graphs' copy ids and <END> before min_time_step are never
    drawn) from a counter hash of (seed, graph, sample, step, column).  A sample never changes parent, so each layer keeps ONE
    [max_time_step, N, 2d] cache and nothing is reordered; ``sync_every``, ``stats`` and ``no_repeat_ngram`` as in _slot_decode, ``avoid`` as in
    beam_search_device.  Returns the beams filled
    like a beam search's: completed_hypotheses (ended by <END>) by completion step, then sample index; hypotheses (unfinished) in
    sample order; score = the fp64 sum of the model's ll of the drawn tokens.
    ``min_p`` (0 = off), ``typical_p`` (1 = off), ``epsilon_cutoff`` / ``eta_cutoff`` (0 = off): the cuts of csrc/truncate_kernels.h,
    which depend on each row's maximum, entropy and normaliser.  With one of them on (as the fp32 value the kernel takes), every step
    launches gtos_truncate_block after the bans and directly before gtos_sample_step: it removes columns from the row in that order
    (min-p, typical, epsilon / eta, each on the renormalised survivors), and ``top_k`` / ``top_p`` then act on what is left -- other
    toolkits apply top_k / top_p first.  With all four at their defaults nothing more is launched."""
    import ctypes
    cuts = tuple(ctypes.c_float(v).value for v in (min_p, typical_p, epsilon_cutoff, eta_cutoff))
    truncate = cuts != (0.0, 1.0, 0.0, 0.0)

    def layout(d):
        d.owned = model.sample_tables(d.local, d.tot)
        return [('state', (d.N, 3), (0, -1, 0)), ('tokens', (d.max_t, d.N), -1)], [('score', (d.N,), 0)]      # -1: no completion yet

    def step(d, t, ll, cur, nxt, tok_out, char_out):
        a, tab = d.arr, d.tab
        if truncate:
            ops.truncate_block(t, d.k, d.V, d.tot, d.min_t, temperature, *cuts, ll, tab['flag_shared'], tab['flag_local'], d.owned,
                               a['state'], a['active'])
        ops.sample_step(t, d.k, d.V, d.tot, d.min_t, d.max_t, temperature, top_k, top_p, seed, ll, tab['flag_shared'], tab['flag_local'],
                        d.owned, a['score'], a['state'], a['tokens'], a['active'], tab['tok_shared'], tab['tok_local'],
                        tab['char_shared'], tab['char_local'], tab['dead_tok'], tab['dead_char'], tok_out, char_out)
    return _slot_decode("sample_device", model, memory, beams, sync_every, stats, 1, None, layout, step, fill_samples, no_repeat_ngram,
                        lambda d, t: (None, d.arr['tokens'][t]), avoid=avoid_ids(model, memory['local_idx2token'], avoid))


class StochasticHypothesis(Hypothesis):
    __slots__ = ("logq", "gumbel")

    def __init__(self, seq, score, logq, gumbel):
        super().__init__(seq, score)
        self.logq = logq                # log-probability under the distribution drawn from: tempered, locally normalised over the allowed tokens
        self.gumbel = gumbel            # the perturbed value G the hypothesis was ranked by


def stochastic_roots(seed, B):
    """root_gumbel of csrc/sbs_kernels.h for graphs 0 .. B-1 as numpy fp64: the perturbed value of every graph's empty prefix, a
    Gumbel(0) draw from column 0 of the hash row of (seed, graph, slot index ops.SBS_MAX_K -- which no slot has --, step 0)."""
    import numpy as np
    from .synth import SplitMix64
    graphs = SplitMix64(int(seed) & 0xFFFFFFFFFFFFFFFF).u64(B) if B else np.zeros(0, np.uint64)
    bits = np.array([SplitMix64(int(SplitMix64(int(SplitMix64(int(g)).u64(ops.SBS_MAX_K + 1)[-1])).u64(1)[0])).u64(1)[0] for g in graphs],
                    dtype=np.uint64)
    u = ((bits >> np.uint64(11)).astype(np.float64) + 0.5) * 2.0 ** -53
    return -np.log(-np.log(np.where(u < 1.0, u, 1.0 - 2.0 ** -53)))


def stochastic_beam_search_device(model, memory, beams, temperature, seed, sync_every=8, stats=None, no_repeat_ngram=0, avoid=None):
    """Stochastic beam search on the device (csrc/sbs.hip, the rule in csrc/sbs_kernels.h; Kool, van Hoof and Welling 2019): every
    graph gets ``beam_size`` DISTINCT sequences drawn without replacement from the distribution ``sample_device`` draws one sequence
    from at this temperature (top_k = 0, top_p = 1; <UNK>, other graphs' copy ids and <END> before min_time_step are never drawn), at
    the cost of a beam search of that width.  The slots, the back-pointer, completion and state tables and the reorder are those of
    beam_search_device; the selection is gtos_sbs_step (per live row the k best candidates by perturbed key, from the counter hash of
    (seed, graph, slot, step, column); the empty prefix's value is stochastic_roots(seed, B)) and gtos_sbs_advance (the graph's completions and candidates ranked by perturbed value:
    finished hypotheses keep competing until the search ends).  ``sync_every``, ``stats`` and ``no_repeat_ngram`` as in _slot_decode,
    ``avoid`` as in beam_search_device: a banned column is not allowed, and the distribution is normalised over what is left.
    Returns the beams filled with StochasticHypothesis objects (score = the fp64 sum of the model's ll, logq, gumbel):
    completed_hypotheses (ended by <END>) and hypotheses (cut at max_time_step), each in descending gumbel; together min(k, number of
    allowed sequences) of them.  stochastic_weights turns a beam into importance weights."""
    tables = types.SimpleNamespace()                         # the candidate tables, which the host never reads

    def layout(d):
        c, dev = tables, memory['probe'].device
        c.owned = model.sample_tables(d.local, d.tot)
        c.root = torch.from_numpy(stochastic_roots(seed, d.B)).to(dev)
        c.tok = torch.full((d.N, d.k), -1, dtype=torch.int32, device=dev)
        c.ll = torch.zeros((d.N, d.k), dtype=torch.float32, device=dev)
        c.logq, c.gumbel = (torch.zeros((d.N, d.k), dtype=torch.float64, device=dev) for _ in range(2))
        return _plain_cuts(d, d.B, dbls=[('slot_logq', (d.N,), 0), ('slot_gumbel', (d.N,), 0), ('comp_logq', (d.B, d.k), 0),
                                         ('comp_gumbel', (d.B, d.k), 0)])

    def step(d, t, ll, cur, nxt, tok_out, char_out):
        a, c, tab = d.arr, tables, d.tab
        if t == 0:
            a['slot_gumbel'].view(d.B, d.k)[:, 0] = c.root
        ops.sbs_step(t, d.k, d.V, d.tot, d.min_t, d.max_t, temperature, seed, ll, tab['flag_shared'], tab['flag_local'], c.owned,
                     a['slot_logq'], a['slot_gumbel'], a['state'], a['active'], c.tok, c.ll, c.logq, c.gumbel)
        ops.sbs_advance(t, d.k, d.V, d.tot, d.min_t, d.max_t, c.tok, c.ll, c.logq, c.gumbel, tab['flag_shared'], tab['flag_local'],
                        a['slot_score'], a['slot_logq'], a['slot_gumbel'], a['state'], a['bp_parent'], a['bp_token'], a['comp_step'],
                        a['comp_parent'], a['comp_score'], a['comp_logq'], a['comp_gumbel'], a['active'])
        _plain_reorder(d, t, cur, nxt, tok_out, char_out)
    _slot_decode("stochastic_beam_search_device", model, memory, beams, sync_every, stats, 2, 1, layout, step, fill_stochastic,
                 no_repeat_ngram, _taken, avoid=avoid_ids(model, memory['local_idx2token'], avoid))
    for b, beam in enumerate(beams):
        if beam.steps == 0:
            beam.hypotheses = [StochasticHypothesis([STR], 0., 0., float(stochastic_roots(seed, b + 1)[b]))]
    return beams


def fill_stochastic(beams, k, state, slot_logq, slot_gumbel, comp_logq, comp_gumbel, **plain):
    """The Beam objects of a stochastic beam search from its tables (flat lists): fill_beams, every hypothesis a StochasticHypothesis
    with the logq / gumbel of its completion row (comp_* [B*k]) or slot (slot_* [N]).  Both lists are in descending gumbel."""
    fill_beams(beams, k, state=state, **plain)
    for b, beam in enumerate(beams):
        if not state[4 * b]:
            continue
        beam.completed_hypotheses = [StochasticHypothesis(h.seq, h.score, comp_logq[b * k + j], comp_gumbel[b * k + j])
                                     for j, h in enumerate(beam.completed_hypotheses)]
        beam.hypotheses = [StochasticHypothesis(h.seq, h.score, slot_logq[b * k + j], slot_gumbel[b * k + j])
                           for j, h in enumerate(beam.hypotheses)]
    return beams


def stochastic_weights(beam):
    """The importance weights that make a stochastic beam search's sample an estimator (Kool et al. 2019, section 4.2): with kappa the
    smallest ``gumbel`` of the beam's hypotheses (finished and unfinished), every hypothesis h with gumbel > kappa gets
    w = q(h) / P(G_h > kappa) = exp(logq) / (1 - exp(-exp(logq - kappa))), and sum_h w_h f(h) is an unbiased estimate of E_q[f].
    -> ([(hypothesis, w), ...] in descending gumbel, kappa); a beam with one hypothesis has no threshold below it: ([], its gumbel)."""
    hyps = sorted(list(beam.completed_hypotheses) + list(beam.hypotheses), key=lambda h: h.gumbel, reverse=True)
    if not hyps:
        return [], float('inf')
    kappa = hyps[-1].gumbel
    def weight(logq):
        above = logq - kappa                                 # past exp's range the probability of inclusion is 1, or exp(above), in fp64
        if above < -700.0:
            return math.exp(kappa)
        return math.exp(logq) / -math.expm1(-math.exp(above)) if above < 700.0 else math.exp(logq)
    return [(h, weight(h.logq)) for h in hyps if h.gumbel > kappa], kappa


def fill_samples(beams, k, state, tokens, score, token_string):
    """The Beam objects of a sampling decode from its tables (flat lists): state [N*3] (steps, completion step or -1, dead), tokens
    [T*N] (row t: the token id every slot drew at step t, or -1), score [N]; token_string(b, id) -> the string of an output id of
    graph b.  A graph's steps are the most any of its slots took part in."""
    N = len(beams) * k
    for b, beam in enumerate(beams):
        slots = range(b * k, b * k + k)
        steps = max(state[3 * s] for s in slots)
        if steps == 0:
            continue

        def seq_of(s, n):
            return [STR] + [token_string(b, tokens[u * N + s]) for u in range(n)]
        done = sorted((state[3 * s + 1], s) for s in slots if state[3 * s + 1] >= 0)
        beam.completed_hypotheses = [Hypothesis(seq_of(s, e) + [END], score[s]) for e, s in done]
        # unfinished: every step drew a token, except the step a slot stopped in for want of an allowed column
        beam.hypotheses = [Hypothesis(seq_of(s, state[3 * s] - state[3 * s + 2]), score[s]) for s in slots if state[3 * s + 1] < 0]
        beam.steps = steps
    return beams
