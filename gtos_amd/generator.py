"""Generator: the model assembly of /root/reference/generator/generator.py (encode_step / forward) wired to the
HIP-backed modules.  Same constructor arguments and state_dict keys, so reference checkpoints load.

Train-mode ``encode_step`` hands the graph encoder the relation in FACTORED form (bank + type ids): it is the
exact same function as the reference's ``relation.index_select(0, idx).view(n,n,B,d)`` (generator.py:79) but the
[n,n,B,d] tensor is never built.  Eval mode aggregates alternative shortest paths with the gather-mean kernel
(generator.py:83-88).  Inference (work, generator.py:96-110) runs the beam search of gtos_amd.search over projected K/V caches
(decode_step_batched): the reference re-projects the whole prefix in every layer at every step.  ``decode_step`` keeps the
reference's signature (generator.py:119) for callers that bring their own search loop.
"""
import collections
import contextlib
import ctypes
import math
import numbers

import torch
from torch import nn
import torch.nn.functional as F

from . import ops
from .encoder import TokenEncoder, RelationEncoder
from .decoder import DecodeLayer
from .transformer import Transformer, SinusoidalPositionalEmbedding, SelfAttentionMask
from .graph_transformer import GraphTransformer, set_compute_dtype
from .search import Beam, CoverageBeam, beam_search, beam_search_device, sample_device, stochastic_beam_search_device
from .vocab import PAD, UNK, STR, END, lists_to_tensor, strings_to_char_tensor


def check_sampling(samples, temperature, top_k, top_p, seed):
    """The argument checks of Generator.work(search="sample"): ValueError on anything gtos_sample_step would refuse."""
    if isinstance(samples, bool) or not isinstance(samples, numbers.Integral) or samples < 1:
        raise ValueError("beam_size (samples per graph) must be an integer >= 1, got %r" % (samples,))
    if (isinstance(temperature, bool) or not isinstance(temperature, numbers.Real)
            or not (0 < ctypes.c_float(temperature).value < math.inf)):           # the kernel takes it as fp32
        raise ValueError("temperature must be a number > 0, finite in fp32, got %r" % (temperature,))
    if isinstance(top_k, bool) or not isinstance(top_k, numbers.Integral) or not 0 <= top_k <= 32:
        raise ValueError("top_k must be an integer in [0, 32] (0 = off), got %r" % (top_k,))
    if isinstance(top_p, bool) or not isinstance(top_p, numbers.Real) or not (0 < ctypes.c_float(top_p).value and top_p <= 1):
        raise ValueError("top_p must lie in (0, 1] and be > 0 in fp32, got %r" % (top_p,))
    if seed is not None and (isinstance(seed, bool) or not isinstance(seed, numbers.Integral)):
        raise ValueError("seed must be an integer or None, got %r" % (seed,))


def check_stochastic(beam_size, top_k, top_p):
    """The argument checks of Generator.work(search="stochastic") beyond check_sampling's: the width gtos_sbs_step takes, and no
    truncation -- the rule draws from the whole allowed set."""
    if beam_size > ops.SBS_MAX_K:
        raise ValueError("search='stochastic' takes beam_size up to %d, got %r" % (ops.SBS_MAX_K, beam_size))
    if top_k != 0 or top_p != 1:
        raise ValueError("top_k and top_p do not apply to search='stochastic' (got top_k = %r, top_p = %r)" % (top_k, top_p))


def check_truncation(search, min_p, typical_p, epsilon_cutoff, eta_cutoff):
    """The argument checks of Generator.work(min_p=, typical_p=, epsilon_cutoff=, eta_cutoff=): ValueError unless every value lies in
    its range as the fp32 value gtos_truncate_block takes (min_p in [0, 1], typical_p in (0, 1], the cutoffs in [0, 1)), a value
    other than "off" stays one in fp32, and anything but the defaults comes with search="sample".  -> the cuts that are on, as the
    keywords of search.sample_device (empty: the call as it always was)."""
    given = dict(min_p=min_p, typical_p=typical_p, epsilon_cutoff=epsilon_cutoff, eta_cutoff=eta_cutoff)
    off = dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0)
    ranges = dict(min_p=("[0, 1] (0 = off)", lambda f: 0 <= f <= 1), typical_p=("(0, 1] (1 = off)", lambda f: 0 < f <= 1),
                  epsilon_cutoff=("[0, 1) (0 = off)", lambda f: 0 <= f < 1), eta_cutoff=("[0, 1) (0 = off)", lambda f: 0 <= f < 1))
    on = {}
    for name, v in given.items():
        if isinstance(v, bool) or not isinstance(v, numbers.Real):
            raise ValueError("%s must be a number in %s, got %r" % (name, ranges[name][0], v))
        f = ctypes.c_float(v).value                                               # the kernel takes it as fp32
        if not ranges[name][1](f) or (v == off[name]) != (f == off[name]):
            raise ValueError("%s must lie in %s as an fp32 value, got %r" % (name, ranges[name][0], v))
        if v != off[name]:
            on[name] = float(v)
    if on and search != "sample":
        raise ValueError("%s apply to search='sample' only, not to search=%r" % (", ".join(sorted(on)), search))
    return on


def check_no_repeat_ngram(n, search, max_time_step):
    """The argument check of Generator.work(no_repeat_ngram=): ValueError unless n is an integer >= 0 and, for the device searches,
    n and the step count fit the history row gtos_ngram_block stages (ops.NGRAM_MAX_T)."""
    if isinstance(n, bool) or not isinstance(n, numbers.Integral) or n < 0:
        raise ValueError("no_repeat_ngram must be an integer >= 0 (0 = off), got %r" % (n,))
    if n and search != "host" and max(n, max_time_step) > ops.NGRAM_MAX_T:
        raise ValueError("no_repeat_ngram with search=%r takes n and max_time_step up to %d, got n = %d, max_time_step = %d"
                         % (search, ops.NGRAM_MAX_T, n, max_time_step))
    return int(n)


def check_groups(groups, diversity, beam_size, search):
    """The argument checks of Generator.work(groups=, diversity=): ValueError unless groups is an integer >= 1 that divides beam_size
    and diversity a finite real >= 0; both belong to the beam searches, and a penalty without groups would do nothing."""
    if isinstance(groups, bool) or not isinstance(groups, numbers.Integral) or groups < 1:
        raise ValueError("groups must be an integer >= 1, got %r" % (groups,))
    if isinstance(diversity, bool) or not isinstance(diversity, numbers.Real) or not 0 <= diversity < math.inf:
        raise ValueError("diversity must be a finite number >= 0, got %r" % (diversity,))
    if search in ("sample", "stochastic"):
        if groups != 1 or diversity != 0:
            raise ValueError("groups and diversity apply to the beam searches, not to search=%r" % (search,))
        return 1, 0.0
    if isinstance(beam_size, bool) or not isinstance(beam_size, numbers.Integral) or beam_size < 1 or beam_size % groups:
        raise ValueError("groups must divide beam_size, got groups = %r, beam_size = %r" % (groups, beam_size))
    if diversity > 0 and groups == 1:
        raise ValueError("diversity = %r with groups = 1 would do nothing: ask for groups > 1" % (diversity,))
    return int(groups), float(diversity)


def check_constraints(constraints, search, groups, local_idx2token, vocab):
    """The argument checks of Generator.work(constraints=): None passes as None.  Otherwise ValueError unless the search is a beam
    search without groups and ``constraints`` holds, per graph of ``local_idx2token`` (the batch's copy tables), a list of at most
    ops.CONSTRAIN_MAX distinct token strings, none of them <PAD>, <STR>, <END> or <UNK>, each producible for its graph: one of the
    graph's copy tokens, or a word of ``vocab`` (the predictable-token vocabulary) with an id of its own.  -> a list of lists."""
    if constraints is None:
        return None
    if search in ("sample", "stochastic"):
        raise ValueError("constraints apply to the beam searches, not to search=%r" % (search,))
    if groups != 1:
        raise ValueError("constraints do not combine with groups (got groups = %r)" % (groups,))
    if isinstance(constraints, str) or not isinstance(constraints, (list, tuple)) or len(constraints) != len(local_idx2token):
        raise ValueError("constraints holds one list of token strings per graph: %d graphs, got %r"
                         % (len(local_idx2token), constraints if not isinstance(constraints, (list, tuple)) else len(constraints)))
    out = []
    for b, (words, local) in enumerate(zip(constraints, local_idx2token)):
        if isinstance(words, str) or not isinstance(words, (list, tuple)):
            raise ValueError("constraints[%d] is a list of token strings, got %r" % (b, words))
        if len(words) > ops.CONSTRAIN_MAX:
            raise ValueError("constraints[%d]: at most %d constraints per graph, got %d" % (b, ops.CONSTRAIN_MAX, len(words)))
        copies = set(local.values())
        for w in words:
            if not isinstance(w, str):
                raise ValueError("constraints[%d]: a constraint is a token string, got %r" % (b, w))
            if w in (PAD, STR, END, UNK):
                raise ValueError("constraints[%d]: %s cannot be a constraint" % (b, w))
            if w not in copies and vocab.token2idx(w) == vocab.unk_idx:
                raise ValueError("constraints[%d]: %r is neither a copy token of the graph nor in the vocabulary" % (b, w))
        if len(set(words)) != len(words):
            raise ValueError("constraints[%d]: constraints are a set of single tokens, got a duplicate in %r" % (b, list(words)))
        out.append(list(words))
    return out


def check_phrases(phrases, search, groups, constraints, coverage_penalty, local_idx2token, vocab):
    """The argument checks of Generator.work(phrases=): None passes as None.  Otherwise ValueError unless the search is a beam search
    without groups, constraints or coverage penalty and ``phrases`` holds, per graph of ``local_idx2token`` (the batch's copy tables),
    a list of at most ops.PHRASE_MAX phrases of at most ops.PHRASE_TOKENS_MAX tokens together, a phrase being a non-empty list or tuple
    of at most ops.PHRASE_LEN_MAX token strings (never a bare string), none of them <PAD>, <STR>, <END> or <UNK>, each producible for
    its graph as in check_constraints.  A phrase may be listed twice.  -> a list of lists of lists."""
    if phrases is None:
        return None
    if search in ("sample", "stochastic"):
        raise ValueError("phrases apply to the beam searches, not to search=%r" % (search,))
    if groups != 1:
        raise ValueError("phrases do not combine with groups (got groups = %r)" % (groups,))
    if constraints is not None:
        raise ValueError("phrases do not combine with constraints: state a single token as a phrase of one")
    if coverage_penalty is not None:
        raise ValueError("phrases do not combine with coverage_penalty")
    if isinstance(phrases, str) or not isinstance(phrases, (list, tuple)) or len(phrases) != len(local_idx2token):
        raise ValueError("phrases holds one list of phrases per graph: %d graphs, got %r"
                         % (len(local_idx2token), phrases if not isinstance(phrases, (list, tuple)) else len(phrases)))
    out = []
    for b, (entry, local) in enumerate(zip(phrases, local_idx2token)):
        if isinstance(entry, str) or not isinstance(entry, (list, tuple)):
            raise ValueError("phrases[%d] is a list of phrases, got %r" % (b, entry))
        if len(entry) > ops.PHRASE_MAX:
            raise ValueError("phrases[%d]: at most %d phrases per graph, got %d" % (b, ops.PHRASE_MAX, len(entry)))
        copies = set(local.values())
        for phrase in entry:
            if isinstance(phrase, str):
                raise ValueError("phrases[%d]: a phrase is a list of token strings, got the bare string %r (write [%r])" % (b, phrase, phrase))
            if not isinstance(phrase, (list, tuple)) or not phrase:
                raise ValueError("phrases[%d]: a phrase is a non-empty list of token strings, got %r" % (b, phrase))
            if len(phrase) > ops.PHRASE_LEN_MAX:
                raise ValueError("phrases[%d]: at most %d tokens per phrase, got %d" % (b, ops.PHRASE_LEN_MAX, len(phrase)))
            for w in phrase:
                if not isinstance(w, str):
                    raise ValueError("phrases[%d]: a phrase holds token strings, got %r" % (b, w))
                if w in (PAD, STR, END, UNK):
                    raise ValueError("phrases[%d]: %s cannot be part of a phrase" % (b, w))
                if w not in copies and vocab.token2idx(w) == vocab.unk_idx:
                    raise ValueError("phrases[%d]: %r is neither a copy token of the graph nor in the vocabulary" % (b, w))
        if sum(len(phrase) for phrase in entry) > ops.PHRASE_TOKENS_MAX:
            raise ValueError("phrases[%d]: at most %d tokens per graph, got %d"
                             % (b, ops.PHRASE_TOKENS_MAX, sum(len(phrase) for phrase in entry)))
        out.append([list(phrase) for phrase in entry])
    return out


def check_coverage(beta, search, groups, constraints):
    """The argument checks of Generator.work(coverage_penalty=): None passes as None.  Otherwise ValueError unless beta is a finite
    real >= 0 (0.0: the plain search with the coverage reported) and the search is a beam search without groups or constraints."""
    if beta is None:
        return None
    if isinstance(beta, bool) or not isinstance(beta, numbers.Real) or not 0 <= beta < math.inf:
        raise ValueError("coverage_penalty must be a finite number >= 0 or None, got %r" % (beta,))
    if search in ("sample", "stochastic"):
        raise ValueError("coverage_penalty applies to the beam searches, not to search=%r" % (search,))
    if groups != 1:
        raise ValueError("coverage_penalty does not combine with groups (got groups = %r)" % (groups,))
    if constraints is not None:
        raise ValueError("coverage_penalty does not combine with constraints")
    return float(beta)


def check_avoid(avoid, constraints, phrases, local_idx2token, vocab):
    """The argument checks of Generator.work(avoid=), for every search: None passes as None.  Otherwise ValueError unless ``avoid``
    holds, per graph of ``local_idx2token`` (the batch's copy tables), a list of entries, an entry being a token string (one word) or
    a non-empty list or tuple of token strings (a phrase), none of them <PAD>, <STR>, <END> or <UNK>.  An entry with a string the
    graph cannot produce (neither one of its copy tokens nor a word of ``vocab``, the predictable-token vocabulary, with an id of its
    own) can never occur and is dropped, as is an exact duplicate; what is left holds at most ops.AVOID_TOKENS_MAX tokens per graph.
    Contradictions with the graph's ``constraints`` / ``phrases`` (as their checks return them, or None) are refused: a one-word
    entry that is a constraint, and an entry that occurs as consecutive tokens of a phrase.  -> a list of lists of lists: per graph
    the entries that apply, each a list of strings."""
    if avoid is None:
        return None
    if isinstance(avoid, str) or not isinstance(avoid, (list, tuple)) or len(avoid) != len(local_idx2token):
        raise ValueError("avoid holds one list of entries per graph: %d graphs, got %r"
                         % (len(local_idx2token), avoid if not isinstance(avoid, (list, tuple)) else len(avoid)))
    out = []
    for b, (entries, local) in enumerate(zip(avoid, local_idx2token)):
        if isinstance(entries, str) or not isinstance(entries, (list, tuple)):
            raise ValueError("avoid[%d] is a list of words and phrases, got %r" % (b, entries))
        copies = set(local.values())
        kept = []
        for entry in entries:
            words = [entry] if isinstance(entry, str) else entry
            if not isinstance(words, (list, tuple)) or not words:
                raise ValueError("avoid[%d]: an entry is a token string or a non-empty list of token strings, got %r" % (b, entry))
            for w in words:
                if not isinstance(w, str):
                    raise ValueError("avoid[%d]: an entry holds token strings, got %r" % (b, w))
                if w in (PAD, STR, END, UNK):
                    raise ValueError("avoid[%d]: %s cannot be avoided" % (b, w))
            words = list(words)
            if words in kept or any(w not in copies and vocab.token2idx(w) == vocab.unk_idx for w in words):
                continue                                                # a duplicate, or an entry that can never occur
            if len(words) == 1 and constraints is not None and words[0] in constraints[b]:
                raise ValueError("avoid[%d]: %r is one of the graph's constraints" % (b, words[0]))
            for phrase in phrases[b] if phrases is not None else ():
                if any(list(phrase[i:i + len(words)]) == words for i in range(len(phrase) - len(words) + 1)):
                    raise ValueError("avoid[%d]: %r occurs in the graph's phrase %r" % (b, words, list(phrase)))
            kept.append(words)
        if sum(len(words) for words in kept) > ops.AVOID_TOKENS_MAX:
            raise ValueError("avoid[%d]: at most %d tokens per graph, got %d"
                             % (b, ops.AVOID_TOKENS_MAX, sum(len(words) for words in kept)))
        out.append(kept)
    return out


Coverage = collections.namedtuple("Coverage", "coverage cp tokens graph_of")
Coverage.__doc__ = """What Generator.coverage returns, all DEVICE tensors over N sequences: coverage [N,n] fp32 (per graph node the
alignment weight summed over the sequence's target positions, <END> included), cp [N] fp64 (the coverage penalty of that row: the sum
over the nodes that are not padding of log(min(coverage, 1) + 1e-12)), tokens [N] int32 (target positions), graph_of [N] int64."""


class Scores(collections.namedtuple("Scores", "sentence_ll tokens correct token_ll pred graph_of")):
    """What Generator.score returns, all DEVICE tensors over N scored sequences of at most T target positions (tokens + <END>):
    sentence_ll [N] fp64 = log p(sequence | graph), tokens [N] int32 (target positions), correct [N] int32 (positions whose argmax
    is the target), token_ll [T,N] fp32 (0 at padding), pred [T,N] int32 (the argmax column of every position, over the vocabulary and
    the graph's copy ids), graph_of [N] int64 (the graph each sequence was scored against)."""
    vocab = None         # the predictable-token vocabulary (Generator.score sets it on the instance)

    def strings(self, data, vocab=None):
        """Host side, on demand: ``pred`` as token strings, one list per sequence cut to its ``tokens`` positions -- a copy id through
        the graph's ``data['local_idx2token']``, anything else through the predictable-token vocabulary."""
        local, vocab = data['local_idx2token'], vocab if vocab is not None else self.vocab
        pred, owner, n_tok = self.pred.t().tolist(), self.graph_of.tolist(), self.tokens.tolist()
        return [[local[g][i] if i in local[g] else vocab.idx2token(i) for i in row[:n]] for row, g, n in zip(pred, owner, n_tok)]


class Explained(collections.namedtuple("Explained", "token_ll entropy copy_gate copy_share source source_weight focus focus_weight rank "
                                                    "tokens graph_of")):
    """What Generator.explain returns, all DEVICE tensors over N sequences of at most T target positions (tokens + <END>).  Per
    position [T,N]: token_ll fp32 (log p of the target, bitwise Generator.score's; 0 at padding), entropy fp32 (of the generate/copy
    mixture over the vocabulary and the graph's copy ids, nats), copy_gate fp32, copy_share fp32 (the part of the target's probability
    that was copied from the graph), source int32 / source_weight fp32 (the graph node the target was copied from: the heaviest
    alignment among the nodes whose copy id is the target; -1 / 0 when no node holds it), focus int32 / focus_weight fp32 (the node
    the alignment is heaviest on, whatever its id) and rank int32 (how many outputs the model put strictly above the target; 0: it
    was the argmax; -1: the model cannot produce it).  At padding: copy_share 0, source -1, source_weight 0, rank -1.  ``source`` and
    ``focus`` index the graph-state axis: row s of ``data['cp_seq'][:, graph_of]``, the axis of ``Coverage.coverage``.
    tokens [N] int32 (target positions), graph_of [N] int64 (the graph each sequence was explained against)."""
    vocab = None             # the predictable-token vocabulary,
    concept_vocab = None     # the concept vocabulary and
    target = None            # the target ids [T,N] int64 that were explained (Generator.explain sets the three on the instance)

    def rows(self, data, vocab=None, concept_vocab=None):
        """Host side, on demand (the one host read): per sequence a list of per-token dicts, padded positions skipped -- ``token``
        (a copy id through the graph's ``data['local_idx2token']``, anything else through the predictable-token vocabulary), ``ll``,
        ``entropy``, ``copy_gate``, ``copy_share``, ``rank``, ``source`` and ``focus`` (graph-state positions, -1: none) and, where
        ``data`` carries the concept ids, ``source_concept`` / ``focus_concept``: the strings of those two nodes (None at -1)."""
        local, vocab = data['local_idx2token'], vocab if vocab is not None else self.vocab
        concept_vocab = concept_vocab if concept_vocab is not None else self.concept_vocab
        concept = data.get('concept') if concept_vocab is not None else None
        if concept is not None:
            concept = concept.t().tolist()                 # per graph <CLS> and then its nodes: position s is entry s + 1
        target = data['token_out'] if self.target is None else self.target
        cols = [v.t().tolist() for v in (target, self.token_ll, self.entropy, self.copy_gate, self.copy_share, self.rank, self.source,
                                         self.focus)]
        owner, n_tok = self.graph_of.tolist(), self.tokens.tolist()

        def node(g, s):
            return None if s < 0 else concept_vocab.idx2token(concept[g][s + 1])
        out = []
        for j, (g, n) in enumerate(zip(owner, n_tok)):
            seq = []
            for y, ll, ent, gate, share, rank, src, foc in zip(*(c[j][:n] for c in cols)):
                d = {"token": local[g][y] if y in local[g] else vocab.idx2token(y), "ll": ll, "entropy": ent, "copy_gate": gate,
                     "copy_share": share, "rank": rank, "source": src, "focus": foc}
                if concept is not None:
                    d["source_concept"], d["focus_concept"] = node(g, src), node(g, foc)
                seq.append(d)
            out.append(seq)
        return out


class Generator(nn.Module):
    def __init__(self, vocabs, word_char_dim, word_dim, concept_char_dim, concept_dim, cnn_filters, char2word_dim,
                 char2concept_dim, rel_dim, rnn_hidden_size, rnn_num_layers, embed_dim, ff_embed_dim, num_heads,
                 dropout, snt_layers, graph_layers, inference_layers, pretrained_file, device, depth_size=32,
                 factored_relation=True, label_smoothing=0.0):
        super().__init__()
        label_smoothing = ops.check_label_smoothing(label_smoothing)
        self.vocabs = vocabs
        self.concept_encoder = TokenEncoder(vocabs['concept'], vocabs['concept_char'], concept_char_dim, concept_dim,
                                            embed_dim, cnn_filters, char2concept_dim, dropout, pretrained_file)
        self.relation_encoder = RelationEncoder(vocabs['relation'], rel_dim, embed_dim, rnn_hidden_size,
                                                rnn_num_layers, dropout)
        self.token_encoder = TokenEncoder(vocabs['token'], vocabs['token_char'], word_char_dim, word_dim, embed_dim,
                                          cnn_filters, char2word_dim, dropout, pretrained_file)
        self.graph_encoder = GraphTransformer(graph_layers, embed_dim, ff_embed_dim, num_heads, dropout)
        self.snt_encoder = Transformer(snt_layers, embed_dim, ff_embed_dim, num_heads, dropout, with_external=True)
        self.embed_dim = embed_dim
        self.embed_scale = math.sqrt(embed_dim)
        self.token_position = SinusoidalPositionalEmbedding(embed_dim, device)
        self.concept_depth = nn.Embedding(depth_size, embed_dim)     # 32 (generator) / 256 (translator/generator.py:39)
        self.token_embed_layer_norm = nn.LayerNorm(embed_dim)
        self.concept_embed_layer_norm = nn.LayerNorm(embed_dim)
        self.self_attn_mask = SelfAttentionMask(device)
        self.decoder = DecodeLayer(vocabs, inference_layers, embed_dim, ff_embed_dim, num_heads, concept_dim, rel_dim, dropout,
                                   label_smoothing)
        self.dropout = dropout
        self.probe_generator = nn.Linear(embed_dim, embed_dim)
        self.device = device
        self.factored_relation = factored_relation
        self.compute_dtype = torch.float32
        self.grad_sync = None           # train.Trainer (data parallel): places the gradient-segment boundary markers
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.normal_(self.probe_generator.weight, std=0.02)
        nn.init.constant_(self.probe_generator.bias, 0.)
        nn.init.constant_(self.concept_depth.weight, 0.)

    def set_compute_dtype(self, dtype):
        return set_compute_dtype(self, dtype)

    def _concepts(self, inp):
        c = self.embed_scale * self.concept_encoder(inp['concept'], inp['concept_char']) \
            + self.concept_depth(inp['concept_depth']).to(self.compute_dtype)
        ln = self.concept_embed_layer_norm
        c = ops.layer_norm_residual(c, None, ln.weight, ln.bias, 0.0, ln.eps)
        return c, torch.eq(inp['concept'], self.vocabs['concept'].padding_idx)

    def encode_step(self, inp, train=True):
        ops.refresh_side_policy(inp['concept'].device)      # auxiliary stream yes / no for this step (memory: ops.SIDE_STREAMS)
        if 'relation_graphs' in inp:           # a loader batch whose relation section was left to this device (index_prep="device_all")
            from .data import complete_on_device
            complete_on_device(inp, inp['concept'].device)
        concept_repr, concept_mask = self._concepts(inp)
        with ops._Timed("relation_encoder_fwd"):
            bank = self.relation_encoder(inp['relation_bank'], inp['relation_length'], trie=inp.get('relation_trie'))   # [R, d]
        if train and self.grad_sync is not None:
            # everything downstream of these two belongs to gradient segments <= 2 (graph encoder, probe, decoders)
            concept_repr, bank = self.grad_sync.boundary(2, concept_repr, bank)
        if train:
            if self.factored_relation:
                relation = ops.FactoredRelation(bank, inp['relation'], index=inp.get('relation_index'))
            else:
                relation = bank.index_select(0, inp['relation'].reshape(-1)).view(*inp['relation'].size(), -1)
        elif inp['relation'].dim() == 4 and self.factored_relation:
            # generator flavour, eval: [n,n,B,K] alternative paths averaged (generator.py:83-88) -- as a derived bank of the
            # distinct K-tuples + per-pair ids, so the [n,n,B,d] tensor and its projection are never built
            relation = ops.factored_eval_relation(bank.detach(), inp['relation'])
        elif inp['relation'].dim() == 3 and self.factored_relation:
            # translator flavour: one path per pair, the plain lookup (translator/generator.py:73), no autograd graph
            relation = ops.FactoredRelation(bank.detach(), inp['relation'], index=inp.get('relation_index'))
        else:
            relation = ops.relation_gather_mean(bank.detach(), inp['relation'], zero_row0=inp['relation'].dim() == 4)
        with ops._Timed("graph_encoder_fwd"):
            concept_repr = self.graph_encoder(concept_repr, relation, self_padding_mask=concept_mask)
        ops.note_memory(inp['concept'].device)               # a high-water point of the step (ops.refresh_side_policy)
        # (bf16 mode: the encoder returns its fp32 residual stream carrying the bf16 twin; everything downstream is a GEMM operand)
        concept_repr = ops.split_stream(concept_repr, self.compute_dtype)[1]
        probe = torch.tanh(ops.linear(concept_repr[:1], self.probe_generator.weight, self.probe_generator.bias))
        return concept_repr[1:], concept_mask[1:], probe

    def encoder_attn(self, inp):
        with torch.no_grad():
            if 'relation_graphs' in inp:
                from .data import complete_on_device
                complete_on_device(inp, inp['concept'].device)
            concept_repr, concept_mask = self._concepts(inp)
            bank = self.relation_encoder(inp['relation_bank'], inp['relation_length'], trie=inp.get('relation_trie'))
            relation = (ops.factored_eval_relation(bank, inp['relation']) if self.factored_relation
                        else ops.relation_gather_mean(bank, inp['relation'], zero_row0=True))
            return self.graph_encoder.get_attn_weights(concept_repr, relation, self_padding_mask=concept_mask)

    def forward(self, data):
        concept_repr, concept_mask, probe = self.encode_step(data)
        pos = self.token_position(data['token_in']).to(self.compute_dtype)
        token_repr = self.embed_scale * self.token_encoder(data['token_in'], data['token_char_in']) + pos
        ln = self.token_embed_layer_norm
        token_repr = ops.layer_norm_residual(token_repr, None, ln.weight, ln.bias, 0.0, ln.eps)
        token_repr = F.dropout(token_repr, p=self.dropout, training=self.training)
        token_mask = torch.eq(data['token_in'], self.vocabs['token'].padding_idx)
        attn_mask = self.self_attn_mask(data['token_in'].size(0))
        concept_repr = concept_repr.contiguous()
        gs = self.grad_sync
        if gs is not None:          # downstream: sentence encoder (segment 1) and decoder (segment 0)
            token_repr, concept_repr, probe = gs.boundary(1, token_repr, concept_repr, probe)
        token_repr = self.snt_encoder(token_repr, self_padding_mask=token_mask, self_attn_mask=attn_mask,
                                      external_memories=concept_repr, external_padding_mask=concept_mask)
        token_repr = ops.split_stream(token_repr, self.compute_dtype)[1]
        probe = probe.expand_as(token_repr)
        if gs is not None:          # downstream: the decoder only
            probe, concept_repr, token_repr = gs.boundary(0, probe, concept_repr, token_repr)
        out = self.decoder(probe, concept_repr, token_repr, concept_mask, token_mask, attn_mask,
                           data['cp_seq'], target=data['token_out'])
        ops.note_memory(token_repr.device)                   # end of the forward pass: everything saved for backward is alive
        return out

    # ------------------------------------------------------------------------------------------------ inference
    def work(self, data, beam_size, max_time_step, min_time_step=1, search="host", *, temperature=1.0, top_k=0, top_p=1.0,
             seed=None, no_repeat_ngram=0, groups=1, diversity=0.0, constraints=None, coverage_penalty=None, phrases=None,
             avoid=None, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
        """Beam search for every graph of the batch (generator.py:96-110).  Returns the finished Beam objects
        (``beam.get_k_best(k, alpha)``).  search="host": gtos_amd.search.beam_search (selection on the host, one read per
        step); "device": gtos_amd.search.beam_search_device (fixed hypothesis slots, selection and cache reorder on the GPU);
        "sample": gtos_amd.search.sample_device, ``beam_size`` independent samples per graph drawn with ``temperature``, ``top_k``
        (0 = off, at most 32) and ``top_p`` from ``seed`` (None: ops.next_seed()); these four keywords belong to the sampling searches.
        "stochastic": gtos_amd.search.stochastic_beam_search_device, stochastic beam search -- ``beam_size`` (at most 32) DISTINCT
        sequences per graph drawn WITHOUT replacement from the distribution "sample" draws from at ``temperature`` with ``seed``
        (``top_k`` / ``top_p`` stay at their defaults: truncation is not part of it), at the cost of a beam search of that width (the
        rule of csrc/sbs_kernels.h; on the device by gtos_sbs_step / gtos_sbs_advance).  The first hypothesis is distributed as one
        sample; with ``beam_size`` = 1 it is "sample"'s for the same seed.  The hypotheses are StochasticHypothesis objects in
        descending ``gumbel``, each with ``score`` (the log-likelihood), ``logq`` (the log-probability under the distribution drawn
        from) and ``gumbel``; gtos_amd.search.stochastic_weights gives the importance weights of an unbiased estimator.  Groups,
        constraints, phrases and the coverage penalty do not apply to it.
        ``no_repeat_ngram`` = n > 0 (any search): no hypothesis or sample repeats an n-gram of tokens -- the continuations that would
        are scored -inf before the selection (the rule of csrc/ngram_kernels.h; on the device by gtos_ngram_block).
        ``groups`` = G > 1 ("host" and "device"): diverse beam search -- the beam_size hypotheses of a graph are G groups of
        beam_size / G that search one after the other, a group's selection lowering every candidate by ``diversity`` for each
        hypothesis of the groups before it that took the same token at this step (gtos_amd.search.GroupBeam, the rule of
        csrc/diverse_kernels.h; on the device by gtos_diverse_advance / gtos_diverse_reorder).  Scores stay log-likelihoods.  A
        returned beam then carries ``groups``, G Beam objects of width beam_size / G, and its own lists are theirs in group order.
        ``constraints`` ("host" and "device", groups = 1): one list of token strings per graph (a list may be empty) that its output
        must hold -- lexically constrained beam search with dynamic beam allocation (gtos_amd.search.ConstrainedBeam, the rule of
        csrc/constrain_kernels.h; on the device by gtos_constrain_advance).  A string is one of the graph's copy tokens
        (``data['local_idx2token']``) or a vocabulary word; a hypothesis ends only when it holds them all; scores stay
        log-likelihoods (check_constraints).  A returned beam then carries ``met``, the constraint bit masks of its live hypotheses.
        ``coverage_penalty`` = beta >= 0 ("host" and "device", groups = 1, no constraints): the GNMT coverage penalty -- every
        hypothesis accumulates the alignment weights of its steps over the graph nodes, and the selection ranks a candidate by its
        log-likelihood plus beta * sum over the nodes of log(min(coverage, 1)) of its parent (gtos_amd.search.CoverageBeam, the rule of
        csrc/coverage_kernels.h; on the device by gtos_coverage_step / gtos_coverage_advance).  Scores stay log-likelihoods.  The
        returned beams are CoverageBeam objects -- ``get_k_best`` adds beta * cp to the length-normalised score -- of
        CoveredHypothesis, each with ``cp`` and ``coverage`` (one float per node); 0.0 searches as without and reports them.
        ``phrases`` ("host" and "device", groups = 1, no constraints, no coverage penalty): one list of phrases per graph (a list may
        be empty), a phrase being a non-empty list of token strings that the output must hold as consecutive tokens -- ``constraints``
        with constraints of several tokens (gtos_amd.search.PhraseBeam, the rule of csrc/phrase_kernels.h; on the device by
        gtos_phrase_advance).  A phrase listed twice must occur twice; the strings resolve as for ``constraints`` (check_phrases).  A
        returned beam then carries ``met``, the bit masks of the phrases its live hypotheses have finished, and ``progress``, per live
        hypothesis (open, pos): the phrase in progress and its tokens matched so far, (-1, 0) when none is.
        ``avoid`` (any search, with every other option): negative constraints -- one list of entries per graph (a list may be empty),
        an entry being a token string or a non-empty list of token strings that the output must NOT hold as consecutive tokens: a
        continuation that would complete an entry is scored -inf before the selection, like a repeated n-gram (the rule of
        csrc/avoid_kernels.h, a shift-and matcher word per hypothesis; on the device by gtos_avoid_block, on the host by
        gtos_amd.search.avoided_tokens).  The strings resolve as for ``constraints``; an entry the graph cannot produce and a
        duplicate are dropped, at most ops.AVOID_TOKENS_MAX tokens per graph remain, and an entry that one of the graph's
        ``constraints`` or ``phrases`` demands is refused (check_avoid).  A returned beam then carries ``avoid``, the entries that
        were applied, as lists of strings.
        ``min_p``, ``typical_p``, ``epsilon_cutoff``, ``eta_cutoff`` ("sample" only; any other search, "stochastic" included, refuses
        a value other than the default): cuts of the sampled distribution that follow each step's own shape, where ``top_k`` /
        ``top_p`` are fixed (the rule of csrc/truncate_kernels.h; on the device by gtos_truncate_block, one launch per step in front
        of gtos_sample_step, none with the defaults).  On the tempered distribution over the allowed tokens, in this order, each on the
        renormalised survivors of the one before: ``min_p`` in (0, 1] (0 = off) keeps the tokens with at least ``min_p`` times the
        probability of the likeliest one; ``typical_p`` in (0, 1) (1 = off), locally typical sampling, keeps the tokens whose
        information content lies nearest the entropy, up to a ``typical_p`` share of the mass; ``epsilon_cutoff`` e and
        ``eta_cutoff`` h in [0, 1) (0 = off) keep the tokens of probability >= max(e, min(h, sqrt(h) exp(-entropy))) and always the
        likeliest.  ``top_k`` / ``top_p`` then act on what is left -- other toolkits apply ``top_k`` / ``top_p`` first.  The bans of
        ``no_repeat_ngram`` and ``avoid`` come before all of them.  Scores stay log-likelihoods (check_truncation)."""
        if search not in ("host", "device", "sample", "stochastic"):
            raise ValueError("search must be 'host', 'device', 'sample' or 'stochastic', got %r" % (search,))
        no_repeat_ngram = check_no_repeat_ngram(no_repeat_ngram, search, max_time_step)
        groups, diversity = check_groups(groups, diversity, beam_size, search)
        coverage_penalty = check_coverage(coverage_penalty, search, groups, constraints)
        if constraints is not None:
            constraints = check_constraints(constraints, search, groups, data['local_idx2token'], self.vocabs['predictable_token'])
        if phrases is not None:
            phrases = check_phrases(phrases, search, groups, constraints, coverage_penalty, data['local_idx2token'],
                                    self.vocabs['predictable_token'])
        if avoid is not None:
            avoid = check_avoid(avoid, constraints, phrases, data['local_idx2token'], self.vocabs['predictable_token'])
        if search in ("sample", "stochastic"):
            check_sampling(beam_size, temperature, top_k, top_p, seed)
            if search == "stochastic":
                check_stochastic(beam_size, top_k, top_p)
            if seed is None:
                seed = ops.next_seed()
        elif (temperature, top_k, top_p, seed) != (1.0, 0, 1.0, None):
            raise ValueError("temperature, top_k, top_p and seed apply to search='sample' and search='stochastic' only")
        cuts = check_truncation(search, min_p, typical_p, epsilon_cutoff, eta_cutoff)
        with torch.no_grad():
            concept_repr, concept_mask, probe = self.encode_step(data, train=False)
            concept_repr = concept_repr.contiguous()
            dec = self.decoder
            memory = {
                'probe': probe,
                'graph_padding_mask': concept_mask,
                'cp_seq': data['cp_seq'],
                'tot_ext': 1 + int(data['cp_seq'].max().item()),
                'local_idx2token': data['local_idx2token'],
                # K/V projections of the graph states for every cross-attention that reads them: computed once
                'snt_ext_kv': [l.external_attn.project_kv(concept_repr) for l in self.snt_encoder.layers],
                'inf_ext_kv': [l.external_attn.project_kv(concept_repr) for l in dec.inference_core.layers],
                'align_kv': dec.token_generator.alignment_layer.project_kv(concept_repr),
            }
            beams = [Beam(beam_size, min_time_step, max_time_step) for _ in range(concept_repr.size(1))]
            block = dict(no_repeat_ngram=no_repeat_ngram) if no_repeat_ngram else {}       # n = 0: the calls as they always were
            if groups != 1:                                                                # groups = 1: likewise
                block.update(groups=groups, diversity=diversity)
            if constraints is not None:                                                    # None: likewise
                block.update(constraints=constraints)
            if coverage_penalty is not None:                                               # None: likewise
                block.update(coverage=coverage_penalty)
                beams = [CoverageBeam(beam_size, min_time_step, max_time_step, coverage_penalty) for _ in beams]
            if phrases is not None:                                                        # None: likewise
                block.update(phrases=phrases)
            if avoid is not None and any(avoid):                                           # nothing to avoid: likewise
                block.update(avoid=avoid)
            if search == "device":
                beam_search_device(self, memory, beams, **block)
            elif search == "sample":
                sample_device(self, memory, beams, temperature, top_k, top_p, seed, **block, **cuts)      # no cut: the call as it always was
            elif search == "stochastic":
                stochastic_beam_search_device(self, memory, beams, temperature, seed, **block)
            else:
                beam_search(self, beams, memory, **block)
            if avoid is not None:
                for beam, entries in zip(beams, avoid):
                    beam.avoid = entries
        return beams

    # ------------------------------------------------------------------------------------------------ teacher-forced scoring
    def _score_sequences(self, data, targets):
        """(sequences, graph of each sequence, copy table of each sequence) of ``score(data, targets)``; ValueError on anything
        that is not one token-string list, or a list of them, per graph."""
        B = data['concept'].size(1)
        if isinstance(targets, str) or len(targets) != B:
            raise ValueError("targets holds one entry per graph: %d graphs, got %r entries"
                             % (B, len(targets) if not isinstance(targets, str) else targets))
        tables = data.get('local_token2idx')
        if tables is None:
            inverse = data.get('local_idx2token')
            if inverse is None:
                raise ValueError("scoring given targets needs the batch's copy table: 'local_token2idx' or 'local_idx2token'")
            tables = [{w: i for i, w in t.items()} for t in inverse]
        seqs, owner = [], []
        for b, entry in enumerate(targets):
            if isinstance(entry, str) or not isinstance(entry, (list, tuple)):
                raise ValueError("targets[%d] is a token-string list or a list of them, got %r" % (b, entry))
            nbest = [entry] if entry and isinstance(entry[0], str) else entry      # (an empty entry: nothing to score for this graph)
            for x in nbest:
                if isinstance(x, str) or not isinstance(x, (list, tuple)) or not all(isinstance(w, str) for w in x):
                    raise ValueError("targets[%d]: a target is a list of token strings, got %r" % (b, x))
                seqs.append(list(x))
                owner.append(b)
        return seqs, owner, [tables[b] for b in owner]

    def score_rows(self, data, targets=None):
        """The device part of ``score``: (nll [T,N] fp32, pred [T,N] int32, p_pred [T,N] fp32, target [T,N] int64, graph_of [N]
        int64).  Eval mode and no autograd whatever the module's state, which is left as found; no dropout seed is drawn."""
        given = None if targets is None else self._score_sequences(data, targets)
        with self._as_scorer():
            return self._score_rows(data, given)

    @contextlib.contextmanager
    def _as_scorer(self):
        """Eval mode under no_grad for a teacher-forced post-pass (score, coverage, explain); the module's mode and the relation
        encoder's ``trie_in_eval`` are put back as found."""
        modes = [(m, m.training) for m in self.modules()]
        enc = self.relation_encoder
        trie_was = getattr(enc, "trie_in_eval", True)
        try:
            self.eval()
            # the whole bank in one packed pass, as in training: the trie evaluation eval mode otherwise takes is a chain of small
            # launches per trie level, three times slower at C2 where one pass over all rows is wanted
            enc.trie_in_eval = False
            with torch.no_grad():
                yield
        finally:
            enc.trie_in_eval = trie_was
            for m, was in modes:
                m.training = was

    def _score_rows(self, data, given):
        dev = data['concept'].device
        if given is not None and not given[0]:          # every n-best list empty: nothing to launch
            z = lambda dt: torch.zeros((0, 0), dtype=dt, device=dev)        # noqa: E731
            return z(torch.float32), z(torch.int32), z(torch.float32), z(torch.int64), torch.zeros(0, dtype=torch.int64, device=dev)
        probe, concept_repr, token_repr, concept_mask, token_mask, attn_mask, cp_seq, target, graph_of = self._teacher_forced(data, given)
        nll, pred, p_pred = self.decoder.evaluate(probe, concept_repr, token_repr, concept_mask, token_mask, attn_mask, cp_seq, target)
        return nll, pred, p_pred, target, graph_of

    def _teacher_forced(self, data, given):
        """The full-sequence pass up to the decoder, for the batch's own sentences or ``given`` (_score_sequences): the decoder's
        operands (probe, graph states, sentence states, their masks, the copy ids) per sequence, then target [T,N] and graph_of [N]."""
        dev = data['concept'].device
        concept_repr, concept_mask, probe = self.encode_step(data, train=False)
        concept_repr, cp_seq = concept_repr.contiguous(), data['cp_seq']
        if given is None:
            token_in, token_char_in, target = data['token_in'], data['token_char_in'], data['token_out']
            graph_of = torch.arange(concept_repr.size(1), device=dev)
        else:
            from .data import batchify_targets
            seqs, owner, tables = given
            built = batchify_targets(seqs, self.vocabs, tables)
            token_in, token_char_in, target = (built[k].to(dev) for k in ('token_in', 'token_char_in', 'token_out'))
            # the graph is encoded once; its memory is gathered per sequence, as search.slot_memory gathers it per slot
            graph_of = torch.tensor(owner, dtype=torch.int64).to(dev)
            sel = lambda v: v.index_select(1, graph_of)                      # noqa: E731
            concept_repr, concept_mask, cp_seq, probe = sel(concept_repr), sel(concept_mask), sel(cp_seq), sel(probe)
        pos = self.token_position(token_in).to(self.compute_dtype)
        token_repr = self.embed_scale * self.token_encoder(token_in, token_char_in) + pos
        ln = self.token_embed_layer_norm
        token_repr = ops.layer_norm_residual(token_repr, None, ln.weight, ln.bias, 0.0, ln.eps)
        token_mask = torch.eq(token_in, self.vocabs['token'].padding_idx)
        attn_mask = self.self_attn_mask(token_in.size(0))
        token_repr = self.snt_encoder(token_repr, self_padding_mask=token_mask, self_attn_mask=attn_mask,
                                      external_memories=concept_repr, external_padding_mask=concept_mask)
        token_repr = ops.split_stream(token_repr, self.compute_dtype)[1]
        return probe.expand_as(token_repr), concept_repr, token_repr, concept_mask, token_mask, attn_mask, cp_seq.contiguous(), target, graph_of

    def score(self, data, targets=None):
        """Teacher-forced log-likelihoods: of the batch's own sentences (``data['token_out']`` given ``data['token_in']``), or of
        ``targets`` -- per graph one token-string list or a list of them (an n-best list; lengths may differ, a list may be empty),
        without <STR> / <END>.  The graph is encoded once; the strings become ids through the vocabularies and the graph's copy table
        as the loader builds them (data.batchify_targets).  A score is the plain log-likelihood: label smoothing does not enter, the
        module runs as in eval mode under no_grad (its mode is left as found), no seed is drawn and the host reads nothing.  Returns
        ``Scores`` (device tensors)."""
        nll, pred, _, target, graph_of = self.score_rows(data, targets)
        live = target.ne(self.vocabs['predictable_token'].padding_idx)
        out = Scores(sentence_ll=-nll.double().sum(0), tokens=live.sum(0).to(torch.int32),
                     correct=(pred.eq(target) & live).sum(0).to(torch.int32), token_ll=-nll, pred=pred, graph_of=graph_of)
        out.vocab = self.vocabs['predictable_token']
        return out

    def coverage(self, data, targets=None):
        """Teacher-forced coverage of the graph nodes, next to ``score`` and with its target handling: per sequence the alignment
        weights of the full-sequence pass (the attention the copy mechanism reads) summed over its target positions, and the coverage
        penalty of that row, by the kernel the searches use (gtos_coverage_step on a zero coverage).  A node whose coverage stays
        near 0 was never verbalised.  Eval mode under no_grad, the module's mode left as found.  Returns ``Coverage``."""
        given = None if targets is None else self._score_sequences(data, targets)
        with self._as_scorer():
            return self._coverage(data, given)

    def explain(self, data, targets=None):
        """Token-level attribution, next to ``score`` and with its target handling: for every target position, whether the token was
        copied from the graph or generated from the vocabulary, from which node, how sure the model was and how many outputs it
        preferred (``Explained``).  A post-pass over finished strings -- the batch's own sentences, or the output of any search -- by
        ONE kernel (gtos_copy_explain_fwd) on the operands of the teacher-forced pass; the [T,N,V+copies] row is never built.  Eval
        mode under no_grad, the module's mode left as found; no seed is drawn and the host reads nothing (``Explained.rows`` does)."""
        given = None if targets is None else self._score_sequences(data, targets)
        with self._as_scorer():
            out = self._explain(data, given)
        out.vocab, out.concept_vocab = self.vocabs['predictable_token'], self.vocabs['concept']
        return out

    def _explain(self, data, given):
        dev = data['concept'].device
        if given is not None and not given[0]:          # every n-best list empty: nothing to launch
            z = lambda dt: torch.zeros((0, 0), dtype=dt, device=dev)        # noqa: E731
            out = Explained(*[z(d) for _, d in ops.EXPLAIN_OUTPUTS], tokens=torch.zeros(0, dtype=torch.int32, device=dev),
                            graph_of=torch.zeros(0, dtype=torch.int64, device=dev))
            out.target = z(torch.int64)
            return out
        probe, concept_repr, token_repr, concept_mask, token_mask, attn_mask, cp_seq, target, graph_of = self._teacher_forced(data, given)
        nll, *rest = self.decoder.explain(probe, concept_repr, token_repr, concept_mask, token_mask, attn_mask, cp_seq, target)
        live = target.ne(self.vocabs['predictable_token'].padding_idx)
        out = Explained(-nll, *rest, tokens=live.sum(0).to(torch.int32), graph_of=graph_of)
        out.target = target
        return out

    def _coverage(self, data, given):
        dev = data['concept'].device
        if given is not None and not given[0]:          # every n-best list empty: nothing to launch
            n = max(data['concept'].size(0) - 1, 0)
            return Coverage(torch.zeros((0, n), dtype=torch.float32, device=dev), torch.zeros(0, dtype=torch.float64, device=dev),
                            torch.zeros(0, dtype=torch.int32, device=dev), torch.zeros(0, dtype=torch.int64, device=dev))
        probe, concept_repr, token_repr, concept_mask, token_mask, attn_mask, cp_seq, target, graph_of = self._teacher_forced(data, given)
        _, align = self.decoder(probe, concept_repr, token_repr, concept_mask, token_mask, attn_mask, cp_seq, work=True, want_align=True)
        live = target.ne(self.vocabs['predictable_token'].padding_idx)
        total = (align * live.unsqueeze(2).to(align.dtype)).sum(0).contiguous()                 # [N, n]
        N = total.size(0)
        cov, cp = torch.empty_like(total), torch.empty(N, dtype=torch.float64, device=dev)
        ops.coverage_step(0, 1, total, concept_mask.contiguous(), None, torch.zeros_like(total), cov, cp,
                          torch.ones(3, dtype=torch.int32, device=dev))
        return Coverage(coverage=cov, cp=cp, tokens=live.sum(0).to(torch.int32), graph_of=graph_of)

    # ---- fixed-slot decoding for gtos_amd.search.beam_search_device
    def search_tables(self, local_idx2token, tot):
        """Per batch, for every output id of the ll row [0, tot): its string class (0 plain, 1 <UNK>, 2 <END>), and the token id and
        character row prepare_incremental_input builds for its string.  Ids < V (the predictable-token vocabulary) share one table,
        kept across batches; ids in [V, tot) get one table per graph from local_idx2token (copy ids start at V, the reference's
        data.py).  Returns a dict of device tensors plus the start (<STR>) and dead-slot (<PAD>) inputs."""
        pv, tv, cv = self.vocabs['predictable_token'], self.vocabs['token'], self.vocabs['token_char']
        V = pv.size

        def cls(w):
            return 1 if w == UNK else 2 if w == END else 0

        def chars(ws):
            return strings_to_char_tensor([ws], cv)[:, 0] if ws else None
        shared = self.__dict__.get('_search_shared')
        if shared is None or shared[0] != (V, str(self.device)):
            words = [pv.idx2token(i) for i in range(V)]
            shared = ((V, str(self.device)), torch.tensor([cls(w) for w in words], dtype=torch.uint8).to(self.device),
                      torch.tensor(tv.token2idx(words), dtype=torch.int64).to(self.device), chars(words).to(self.device))
            self.__dict__['_search_shared'] = shared
        B, L = len(local_idx2token), tot - V
        C = shared[3].shape[1]
        flag_l = torch.zeros((B, max(L, 0)), dtype=torch.uint8)
        tok_l = torch.full((B, max(L, 0)), tv.unk_idx, dtype=torch.int64)
        char_l = torch.zeros((B, max(L, 0), C), dtype=torch.int64)
        for b, local in enumerate(local_idx2token):
            items = sorted((i, w) for i, w in local.items() if V <= i < tot)
            for i, w in local.items():
                if i < V and w != pv.idx2token(i):
                    raise ValueError("copy id %d of graph %d lies inside the vocabulary (%r vs %r)" % (i, b, w, pv.idx2token(i)))
            if items:
                ids = [i - V for i, _ in items]
                words = [w for _, w in items]
                flag_l[b, ids] = torch.tensor([cls(w) for w in words], dtype=torch.uint8)
                tok_l[b, ids] = torch.tensor(tv.token2idx(words), dtype=torch.int64)
                char_l[b, ids] = chars(words)
        start = (tv.token2idx(STR), strings_to_char_tensor([[STR]], cv)[0, 0])
        dead = (tv.padding_idx, strings_to_char_tensor([[PAD]], cv)[0, 0])
        dev = self.device
        return {'V': V, 'C': C, 'flag_shared': shared[1], 'tok_shared': shared[2], 'char_shared': shared[3],
                'flag_local': flag_l.to(dev) if L > 0 else None, 'tok_local': tok_l.to(dev) if L > 0 else None,
                'char_local': char_l.to(dev) if L > 0 else None,
                'start_tok': start[0], 'start_char': start[1].to(dev), 'dead_tok': dead[0], 'dead_char': dead[1].to(dev)}

    def sample_tables(self, local_idx2token, tot):
        """For gtos_amd.search.sample_device, next to search_tables: owned uint8 [B, tot-V], 1 where copy id V + i belongs to graph
        b (is in its local_idx2token); None when tot == V."""
        V = self.vocabs['predictable_token'].size
        if tot <= V:
            return None
        owned = torch.zeros((len(local_idx2token), tot - V), dtype=torch.uint8)
        for b, local in enumerate(local_idx2token):
            ids = [i - V for i in local if V <= i < tot]
            if ids:
                owned[b, ids] = 1
        return owned.to(self.device)

    def slot_caches(self, max_time_step, N, copies=2):
        """Preallocated self-attention caches of the fixed-slot search: per sentence-encoder and inference layer ``copies`` zeroed
        [max_time_step, N, 2d] buffers in the layer's compute dtype (a pair for the beam search's reorder, one for sampling)."""
        layers = list(self.snt_encoder.layers) + list(self.decoder.inference_core.layers)
        return [[torch.zeros((max_time_step, N, 2 * self.embed_dim), dtype=l.self_attn.compute_dtype, device=self.device)
                 for _ in range(copies)] for l in layers]

    def decode_slots(self, inp, caches, mem, t, want_align=False):
        """Step t of the fixed-slot search: inp = (step_token [1,N], step_token_char [1,N,C]); caches: one [T_max,N,2d] buffer per
        sentence-encoder layer, then per inference layer (rows [0,t) hold the prefix, row t is written); mem: everything per slot.
        -> ll [N, V+ext] fp32; with ``want_align`` (ll, align [N, n] fp32: the slots' alignment weights over the graph nodes)."""
        n_snt = len(self.snt_encoder.layers)
        x = self._step_embed(inp, t)
        for li, layer in enumerate(self.snt_encoder.layers):
            x = layer.step_into(x, x, caches[li], t, mem['snt_ext_kv'][li], mem['graph_padding_mask'])
        if want_align:
            ll, align = self.decoder.step_into(mem['probe'], x, caches[n_snt:], t, mem, want_align=True)
            return ll[0], align[0]
        return self.decoder.step_into(mem['probe'], x, caches[n_snt:], t, mem)[0]

    def prepare_incremental_input(self, step_seq):
        """step_seq: one single-token list per live hypothesis (generator.py:112-117).  Token id and character row of a
        string are cached: beam search feeds the same few thousand strings over and over."""
        if any(len(x) != 1 for x in step_seq):
            token = lists_to_tensor(step_seq, self.vocabs['token'])
            token_char = strings_to_char_tensor(step_seq, self.vocabs['token_char'])
            return token.to(self.device), token_char.to(self.device)
        cache = self.__dict__.setdefault('_step_input_cache', {})
        ids, rows = [], []
        for (w,) in step_seq:
            hit = cache.get(w)
            if hit is None:
                hit = (self.vocabs['token'].token2idx(w), strings_to_char_tensor([[w]], self.vocabs['token_char'])[0, 0].tolist())
                cache[w] = hit
            ids.append(hit[0])
            rows.append(hit[1])
        token = torch.tensor([ids], dtype=torch.int64)
        token_char = torch.tensor([rows], dtype=torch.int64)
        return token.to(self.device), token_char.to(self.device)

    def decode_step_batched(self, tokens, state, memory, beam_of_hyp, offset, topk, banned=None, want=None, want_align=False):
        """One step for N live hypotheses of ALL beams (what gtos_amd.search.beam_search drives).  tokens: their last token
        strings; state: None or {'snt': [cache per sentence-encoder layer], 'inf': [cache per inference layer]}, every cache
        [t,N,2d]; memory: per GRAPH (``work``); beam_of_hyp [N]: graph index of each hypothesis; banned: None or per hypothesis the output
        ids whose ll is -inf before the top-k (search.banned_tokens).  Returns (state grown by one row, per hypothesis the top-k
        [(token string, log-likelihood)]); with ``want`` (per hypothesis a list of output ids) a third value: per hypothesis the
        log-likelihoods of those ids after the banning; with ``want_align`` a last value: the alignment weights [N, n] fp32."""
        inp = self.prepare_incremental_input([[t] for t in tokens])
        sel = lambda v: v.index_select(1, beam_of_hyp)
        owners = beam_of_hyp.tolist()
        mem = {'graph_padding_mask': sel(memory['graph_padding_mask']), 'cp_seq': sel(memory['cp_seq']), 'probe': sel(memory['probe']),
               'tot_ext': memory['tot_ext'], 'inf_ext_kv': [sel(v) for v in memory['inf_ext_kv']],
               'snt_ext_kv': [sel(v) for v in memory['snt_ext_kv']], 'align_kv': sel(memory['align_kv']),
               'local_idx2token': [memory['local_idx2token'][bi] for bi in owners]}
        snt, inf, results, *lls = self._decode_core(inp, None if state is None else state['snt'], None if state is None else state['inf'],
                                                    mem, offset, topk, banned, want, want_align)
        return ({'snt': snt, 'inf': inf}, results, *lls)

    def _step_embed(self, inp, offset):
        step_token, step_token_char = inp
        pos = self.token_position(step_token, offset).to(self.compute_dtype)
        x = self.embed_scale * self.token_encoder(step_token, step_token_char) + pos
        ln = self.token_embed_layer_norm
        return ops.layer_norm_residual(x, None, ln.weight, ln.bias, 0.0, ln.eps)

    def _decode_core(self, inp, snt_state, inf_state, mem, offset, topk, banned=None, want=None, want_align=False):
        """inp = (step_token [1,N], step_token_char [1,N,C]); snt_state / inf_state: per layer [t,N,2d] or None; mem: everything
        already per hypothesis; banned: None or per hypothesis the output ids that score -inf; want: None or per hypothesis output ids
        whose ll (after the banning) is returned too; want_align: the alignment weights [N, n] fp32 are returned last.
        -> (new sentence-encoder caches, new inference caches, top-k results[, wanted lls][, align])."""
        x = self._step_embed(inp, offset)
        snt_caches = []
        for li, layer in enumerate(self.snt_encoder.layers):
            x, c = layer.step(x, x, None if snt_state is None else snt_state[li], mem['snt_ext_kv'][li], mem['graph_padding_mask'])
            snt_caches.append(c)
        if want_align:
            ll, inf_caches, align = self.decoder.step(mem['probe'], x, inf_state, mem, want_align=True)
            tail = (align.squeeze(0),)
        else:
            ll, inf_caches = self.decoder.step(mem['probe'], x, inf_state, mem)
            tail = ()
        ll = ll.squeeze(0).float()
        if banned is not None and any(banned):
            rows = [h for h, ids in enumerate(banned) for _ in ids]
            cols = [i for ids in banned for i in ids]
            ll = ll.index_put((torch.tensor(rows, device=ll.device), torch.tensor(cols, device=ll.device)),
                              torch.tensor(float('-inf'), device=ll.device))
        topk_scores, topk_token = torch.topk(ll, topk, 1)
        vocab = self.vocabs['predictable_token']
        results = []
        for s, t, local in zip(topk_scores.tolist(), topk_token.tolist(), mem['local_idx2token']):
            results.append([(local[i] if i in local else vocab.idx2token(i), sc) for sc, i in zip(s, t)])
        if want is not None:
            rows = [h for h, ids in enumerate(want) for _ in ids]
            cols = [i for ids in want for i in ids]
            flat = ll[torch.tensor(rows, dtype=torch.int64, device=ll.device), torch.tensor(cols, dtype=torch.int64, device=ll.device)].tolist() if rows else []
            at = iter(flat)
            return (snt_caches, inf_caches, results, [[next(at) for _ in ids] for ids in want]) + tail
        return (snt_caches, inf_caches, results) + tail

    # ---- the reference's decoding interface (generator/generator.py:96-167, generator/search.py:113-166)
    def reference_memory(self, data):
        """``mem_dict`` as the reference's ``work`` builds it (generator.py:100-104: graph_state, graph_padding_mask, probe,
        local_idx2token, cp_seq -- one column / entry per graph), extended by the K/V projections of the graph states for every
        cross-attention that reads them.  The reference's ``search_by_batch`` treats the dictionary generically (tensors are
        ``index_select``-ed along dim 1 per live hypothesis, lists are indexed), so the extra entries travel with the rest and
        ``decode_step`` never re-projects the graph."""
        with torch.no_grad():
            concept_repr, concept_mask, probe = self.encode_step(data, train=False)
            concept_repr = concept_repr.contiguous()
            mem = {'graph_state': concept_repr, 'graph_padding_mask': concept_mask, 'probe': probe,
                   'local_idx2token': data['local_idx2token'], 'cp_seq': data['cp_seq']}
            for li, l in enumerate(self.snt_encoder.layers):
                mem['snt_ext_kv_%d' % li] = l.external_attn.project_kv(concept_repr)
            for li, l in enumerate(self.decoder.inference_core.layers):
                mem['inf_ext_kv_%d' % li] = l.external_attn.project_kv(concept_repr)
            mem['align_kv'] = self.decoder.token_generator.alignment_layer.project_kv(concept_repr)
        return mem

    def decode_step(self, inp, state_dict, mem_dict, offset, topk):
        """The reference's signature and data flow (generator/generator.py:119-167): inp = (step_token [1,N], step_token_char
        [1,N,C]) from ``prepare_incremental_input``; ``mem_dict``: the reference's keys, every entry already gathered per live
        hypothesis by the caller; ``state_dict``: {} at the first step, afterwards what the previous call returned, split / joined
        along dim 1 by the caller.  Returns (new_state_dict, per hypothesis the top-k [(token string, log-likelihood)]).

        The state carried between steps is the PROJECTED K/V rows of every self-attention ('snt_kv_i', 'inf_kv_i', [t,N,2d]) in
        place of the reference's unprojected 'token_repr_i' / 'token_state' histories -- the same information, so the reference
        re-projecting the whole prefix in every layer at every step is not needed; any caller that treats the dictionary
        opaquely (the reference's Beam / search_by_batch do) works unchanged.  ``mem_dict`` entries made by ``reference_memory``
        are used as they are; with only the reference's own five keys the graph projections are computed here."""
        with torch.no_grad():
            dec = self.decoder
            n_snt, n_inf = len(self.snt_encoder.layers), len(dec.inference_core.layers)
            graph = mem_dict.get('graph_state')

            def kv(key, attn):
                v = mem_dict.get(key)
                return v if v is not None else attn.project_kv(graph)
            cp_seq = mem_dict['cp_seq']
            mem = {'graph_padding_mask': mem_dict['graph_padding_mask'], 'cp_seq': cp_seq, 'probe': mem_dict['probe'],
                   'local_idx2token': mem_dict['local_idx2token'],
                   'tot_ext': 1 + int(cp_seq.max().item()),          # like decoder.py:48 on the live hypotheses' copy ids
                   'snt_ext_kv': [kv('snt_ext_kv_%d' % i, l.external_attn) for i, l in enumerate(self.snt_encoder.layers)],
                   'inf_ext_kv': [kv('inf_ext_kv_%d' % i, l.external_attn) for i, l in enumerate(dec.inference_core.layers)],
                   'align_kv': kv('align_kv', dec.token_generator.alignment_layer)}
            first = not state_dict
            snt_state = None if first else [state_dict['snt_kv_%d' % i] for i in range(n_snt)]
            inf_state = None if first else [state_dict['inf_kv_%d' % i] for i in range(n_inf)]
            snt, inf, results = self._decode_core(inp, snt_state, inf_state, mem, offset, topk)
            new_state = {'snt_kv_%d' % i: c for i, c in enumerate(snt)}
            new_state.update({'inf_kv_%d' % i: c for i, c in enumerate(inf)})
        return new_state, results
