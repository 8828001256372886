"""Batch assembly for the translator flavour: dependency trees -> the batch dict the model consumes.

Counterpart of /root/reference/translator/data.py:126-201 (``batchify``) with the graph work of
translator/dependencyGraph.py:30-74 (BFS node order, all-pairs shortest label paths) done by the C++ host library
(gtos_amd.relbatch, include/gtos_host.h) and the token / character tensors by gtos_amd.vocab.  Bit-exact with the
reference on its own data (tests/test_host_relbatch.py, tests/test_beam_and_vocab.py); the only freedom is the numbering
of the per-graph copy ids, which the reference takes from a ``set`` iteration (extract.py:56-62) and this module assigns
in first-occurrence order.
"""
import os

import torch

from . import relbatch
from .pathtrie import build_path_trie
from .relindex import attach_relation_index
from .vocab import CLS, rCLS, SEL, TL, STR, END, lists_to_tensor, strings_to_char_tensor, copy_vocab


def relation_special_ids(rel_vocab):
    return (rel_vocab.padding_idx, rel_vocab.token2idx(CLS), rel_vocab.token2idx(rCLS), rel_vocab.token2idx(SEL),
            rel_vocab.token2idx(TL))


def resolve_index_prep(index_prep):
    """``index_prep="auto"`` (the loaders' default since round 4): the relation section of every batch -- all-pairs label paths, type
    numbering, bank, relation index, path tries -- is left to the consumer's GPU (``"device_all"``: the loader ships the flattened graphs,
    ~30 KB, and the token / character tensors; gtos_amd.relbatch_hip / relindex_hip / pathtrie_hip build the rest in ~6 ms of device
    time per C2 batch, array for array equal to the host builders) when this process can see a GPU and libgtos_hip.so loads; on a
    host without one the C++ host builders run as before (``True``).  ``GTOS_INDEX_PREP=host|device|device_all`` overrides "auto";
    an explicit argument always wins.  Resolved ONCE, in the process that constructs the loader (worker processes inherit the value)."""
    if index_prep != "auto":
        return index_prep
    env = os.environ.get("GTOS_INDEX_PREP", "")
    if env:
        known = {"host": True, "device": "device", "device_all": "device_all", "off": False}
        if env not in known:
            raise ValueError("GTOS_INDEX_PREP=%r: expected one of %s" % (env, ", ".join(sorted(known))))
        return known[env]
    try:
        if torch.cuda.is_available():
            from . import _lib
            _lib.load()
            return "device_all"
    except Exception:
        pass
    return True


def complete_on_device(batch, device=None, tries="hip"):
    """A batch that reached its consumer with ``relation_graphs`` instead of relation / bank / length (``index_prep="device_all"`` without
    a ``Prefetcher`` in between, e.g. ``for batch in loader: model({k: v.to(dev) ...})``): build them, the relation index and the path
    tries on the batch's device, on the current stream.  A complete batch is returned unchanged."""
    if 'relation_graphs' not in batch:
        return batch
    train = batch['relation_graphs'].path_mode != relbatch.PATH_ALL
    attach_device_relations(batch, device)
    from .relbatch_hip import HipBackend
    if not batch['relation'].is_cuda and HipBackend.backend_needs_device():
        return batch                       # completed by the host builder (the consumer is not a GPU): reference-shaped, nothing device-side to add
    if train:
        attach_device_relation_index(batch)
    return attach_device_tries(batch, tries)


def _index_prep(batch, on):
    """Host-side index preparation of the bf16 training path (gtos_amd.pathtrie, gtos_amd.relindex): the path tries of the
    trie-evaluated RelationEncoder and the relation index of the factored attention operand.  ``on=False`` (fp32 / CPU use,
    ``GTOS_GRU_TRIE=0``) skips it; a bank the trie builder rejects (a path longer than 64 labels -- the translator flavour
    puts no cap on path length --, an empty path) leaves the batch without ``relation_trie`` and RelationEncoder takes its per-row path.
    ``on="device"``: only the relation index is built here; the tries are left to the consumer's device (``Prefetcher(device_tries=
    True)`` builds them with torch ops on its copy stream, gtos_amd.pathtrie_device) -- the tries are the larger half of the
    host time of a batch (0.19 of 0.35 s per C2 batch on the development container)."""
    if not on or 'relation_graphs' in batch:      # ("device_all": nothing to index yet -- the relation tensors do not exist on the host)
        return batch
    if on not in ("device", "device_all"):
        try:
            batch['relation_trie'] = build_path_trie(batch['relation_bank'], batch['relation_length'])
        except ValueError:
            pass              # no 'relation_trie' key: RelationEncoder.forward falls back to one row per (path, position)
    else:
        batch['relation_rows'] = HostInt(batch['relation_length'].sum())   # host integer the staged device builder would have to read back
    return attach_relation_index(batch)


def attach_device_tries(batch, how=True):
    """``batch['relation_trie']`` built on the device the bank lives on, for a batch that came without one; a bank outside the
    device builders' case (paths longer than 8 labels, label ids >= 255) is left alone.  ``how``: True / "torch" = the torch-op
    builder (gtos_amd.pathtrie_device, ~12 ms of small ATen kernels and 6 host reads per C2 batch); "hip" = the staged HIP builder
    (gtos_amd.pathtrie_hip: rocPRIM sorts / scans + the stage kernels of csrc/trie_kernels.h, 2 host reads).  ``batch[
    'relation_rows']`` (sum of the path lengths, known to the loader on the host) saves the staged builder a device read."""
    if 'relation_trie' not in batch and 'relation_bank' in batch:
        try:
            if how == "hip":
                from .pathtrie_hip import HipBackend, build_path_trie_staged
                batch['relation_trie'] = build_path_trie_staged(batch['relation_bank'], batch['relation_length'], HipBackend.shared(),
                                                                n_rows=batch.get('relation_rows'))
            else:
                from .pathtrie_device import build_path_trie_device
                batch['relation_trie'] = build_path_trie_device(batch['relation_bank'], batch['relation_length'])
        except ValueError:
            pass
    return batch


class HostInt(int):
    """A host integer that rides in a batch dict (``relation_rows``): ``.to()`` returns it unchanged, so ``{k: v.to(device) ...}`` works."""

    def to(self, *a, **k):
        return self


class RelationGraphs(object):
    """The graphs of a batch flattened for the GPU relation-batch builder (gtos_amd.relbatch_hip.graphs_csr: ordered adjacency + BFS
    order, a few thousand integers) with the arguments of the build: what a loader ships instead of relation / bank / length when the
    all-pairs work is left to the consumer's device (``index_prep="device_all"``).  Host data; ``.to()`` returns self so that
    ``{k: v.to(device) for k, v in batch.items()}`` passes it through."""

    def __init__(self, csr, special_ids, path_mode, seed, max_len=8, graphs=None):
        self.csr, self.special_ids, self.path_mode, self.seed, self.max_len = csr, tuple(int(v) for v in special_ids), path_mode, int(seed), max_len
        # the graphs themselves ((n_nodes, root, edges[E,3]) each, a few KB): what the C++ host builder takes when the consumer turns out NOT
        # to be a GPU (a CPU / fp32 parity model fed from a loader that resolved index_prep="auto" on a GPU box)
        self.graphs = graphs

    def to(self, *a, **k):
        return self


def attach_device_relations(batch, device=None):
    """``relation`` / ``relation_bank`` / ``relation_length`` of a batch that came with ``relation_graphs`` instead, built on ``device``
    (default: the device of the batch's concept tensor) by the staged HIP builder (gtos_amd.relbatch_hip) on the current stream."""
    rg = batch.get('relation_graphs')
    if rg is None or 'relation' in batch:
        return batch
    dev = batch['concept'].device if device is None else torch.device(device)
    from .relbatch_hip import HipBackend, build_relation_batch_all_staged, build_relation_batch_staged
    if dev.type != "cuda" and HipBackend.backend_needs_device():
        # the HIP stage kernels take device pointers: a consumer on the host gets the C++ host builder's tensors (the same arrays, element
        # for element: tests/test_zzz_hip_relbatch.py) -- complete, reference-shaped.  (The tests' emulation backends run the stage code
        # on host memory and do not set ``needs_device``.)
        if rg.graphs is None:
            raise ValueError("a batch that ships 'relation_graphs' can only be completed on a GPU (or needs RelationGraphs.graphs for the host builder)")
        full = relbatch.build_relation_batch(rg.graphs, rg.special_ids, path_mode=rg.path_mode, seed=rg.seed, max_len=rg.max_len)
        for k in ('relation', 'relation_bank', 'relation_length'):
            batch[k] = full[k].to(dev)
        batch['relation_rows'] = HostInt(int(full['relation_length'].sum()))
        del batch['relation_graphs']
        return batch
    if rg.path_mode == relbatch.PATH_ALL:        # an eval batch: every shortest path, relation [n,n,B,K]
        rel = build_relation_batch_all_staged(None, rg.special_ids, HipBackend.shared(), max_len=rg.max_len, device=dev, csr=rg.csr)
    else:
        rel = build_relation_batch_staged(None, rg.special_ids, HipBackend.shared(), path_mode=rg.path_mode, seed=rg.seed, max_len=rg.max_len,
                                          device=dev, csr=rg.csr)
    batch['relation'], batch['relation_bank'], batch['relation_length'] = rel['relation'], rel['relation_bank'], rel['relation_length']
    batch['relation_rows'] = HostInt(rel['relation_rows'])                 # sum of the path lengths: saves the trie builder a device read
    del batch['relation_graphs']
    return batch


def attach_device_relation_index(batch):
    """``batch['relation_index']`` of a train-mode batch whose ``relation`` lives on the device, by the staged HIP builder
    (gtos_amd.relindex_hip) on the current stream; outside that builder's case the batch is left alone (ops.FactoredRelation then
    derives an index with torch ops)."""
    if 'relation_index' not in batch and batch['relation'].dim() == 3:        # (eval batches are [n,n,B,K]: not factored)
        from .relindex_hip import HipBackend, build_relation_index_staged
        try:
            batch['relation_index'] = build_relation_index_staged(batch['relation'], batch['relation_bank'].shape[1], HipBackend.shared())
        except ValueError:
            pass
    return batch


def batchify_dependency(trees, vocabs, n_threads=0, unk_rate=0., rng=None, replay_reference_draws=False, index_prep=True):
    """``unk_rate`` / ``rng``: the training-time <UNK> noise on ``concept`` and ``token_in`` only (translator/data.py:129,185),
    see vocab.lists_to_tensor.  Between those two tensors the reference's batchify calls ``random.choice`` once per node
    pair on a one-element path list (data.py:149); ``replay_reference_draws`` consumes ``rng`` the same way so that the
    ``token_in`` noise is bit-identical to the reference's under the same generator state (a Python loop over n^2 pairs:
    for tests, off by default).  trees: list of (dep labels, heads (1-based, 0 = root), source tokens, target tokens) as translator/extract.py's
    IO.read1 yields them.  Returns the dict of translator/data.py:185-201 (int64 tensors, time-major) including
    ``local_idx2token`` / ``local_token2idx``; ``concept_depth`` is the node's position in the source sentence
    (dependencyGraph.py:72-73), concepts are in BFS order from the root."""
    rv = vocabs['relation']
    graphs = []
    for dep, head, tok, tgt in trees:
        ids = rv.token2idx(list(dep))
        rev = rv.token2idx([r + '_r_' for r in dep])
        graphs.append(relbatch.dependency_edges(list(head), ids, rev))
    if index_prep == "device_all":
        # the all-pairs work, the bank, the tries and the relation index are left to the consumer's device: ship the graphs
        from .relbatch_hip import graphs_csr
        csr = graphs_csr(graphs)
        orders = [csr['order'][int(csr['node_off'][b]):int(csr['node_off'][b + 1])].tolist() for b in range(len(trees))]
        rel = {'relation_graphs': RelationGraphs(csr, relation_special_ids(rv), relbatch.PATH_FIRST, 0, graphs=graphs)}
    else:
        full = relbatch.build_relation_batch(graphs, relation_special_ids(rv), path_mode=relbatch.PATH_FIRST, n_threads=n_threads)
        orders = [full['order'][b, :len(t[2])].tolist() for b, t in enumerate(trees)]
        rel = {k: full[k] for k in ('relation', 'relation_bank', 'relation_length')}
    concepts, depths, cps, t2is, i2ts = [], [], [], [], []
    for b, (dep, head, tok, tgt) in enumerate(trees):
        order = orders[b]
        conc = [tok[n] for n in order]
        concepts.append(conc)
        depths.append(order)                              # "we just use the sequential order" (dependencyGraph.py:72)
        cp_seq, t2i, i2t = copy_vocab(conc, vocabs['predictable_token'])
        cps.append(cp_seq); t2is.append(t2i); i2ts.append(i2t)
    aug = [[STR] + list(tgt) + [END] for _, _, _, tgt in trees]
    with_cls = [[CLS] + c for c in concepts]
    concept = lists_to_tensor(with_cls, vocabs['concept'], unk_rate=unk_rate, rng=rng)
    if replay_reference_draws and unk_rate > 0.:
        import random
        gen, one = (rng if rng is not None else random), [0]
        for c in concepts:
            for _ in range(len(c) * len(c)):
                gen.choice(one)
    return _index_prep({
        'concept': concept,
        'concept_char': strings_to_char_tensor(with_cls, vocabs['concept_char']),
        'concept_depth': lists_to_tensor([[0] + d for d in depths]),
        **rel,
        'local_idx2token': i2ts, 'local_token2idx': t2is,
        'token_in': lists_to_tensor(aug, vocabs['token'], unk_rate=unk_rate, rng=rng)[:-1],
        'token_char_in': strings_to_char_tensor(aug, vocabs['token_char'])[:-1],
        'token_out': lists_to_tensor(aug, vocabs['predictable_token'], t2is)[1:],
        'cp_seq': lists_to_tensor(cps, vocabs['predictable_token'], t2is),
    }, index_prep)


def read_dependency_file(path):
    """The reference's 4-lines-per-example text format (translator/extract.py:11-45): dependency labels, heads, source
    tokens, target tokens, separated by single spaces."""
    out = []
    with open(path, encoding='utf8') as f:
        lines = [l.rstrip('\n') for l in f]
    for k in range(0, len(lines) - 3, 4):
        dep, head = lines[k].split(' '), [int(x) for x in lines[k + 1].split(' ')]
        tok, tgt = lines[k + 2].split(' '), lines[k + 3].split(' ')
        assert len(dep) == len(head) == len(tok)
        out.append((dep, head, tok, tgt))
    return out


class DependencyLoader(object):
    """Batching policy of translator/data.py:207-264 (``DataLoader``): examples are shuffled and (stably) sorted by size
    ``n_source_tokens**2 + n_target_tokens`` when training, packed greedily until a batch holds ``batch_size`` size units
    (or 257 examples), a trailing batch is kept if it is at least half full (always in evaluation), and the batch order is
    shuffled.  Both shuffles draw from ``rng`` (default: the ``random`` module, like the reference) BEFORE the first batch is
    assembled, so under the same seed the batches and their order are the reference's.  Yields batchify_dependency dicts."""

    def __init__(self, vocabs, filename, batch_size, for_train, rng=None, n_threads=0, index_prep="auto"):
        import random
        self.data = read_dependency_file(filename) if isinstance(filename, str) else list(filename)
        self.vocabs, self.batch_size, self.train = vocabs, batch_size, for_train
        self.rng = rng if rng is not None else random
        self.n_threads = n_threads
        self.unk_rate = 0.
        self.index_prep = resolve_index_prep(index_prep)   # relation section on the consumer's GPU when there is one (see resolve_index_prep)

    def set_unk_rate(self, x):
        """translator/data.py:218-219; train.py:128 calls it with --unk_rate (0.33 in train.sh)."""
        self.unk_rate = x

    @staticmethod
    def size_of(tree):
        dep, head, tok, tgt = tree
        return len(tok) ** 2 + len(tgt)

    def batch_indices(self):
        idx = list(range(len(self.data)))
        if self.train:
            self.rng.shuffle(idx)
            idx.sort(key=lambda i: self.size_of(self.data[i]))
        batches, units, cur = [], 0, []
        for i in idx:
            units += self.size_of(self.data[i])
            cur.append(i)
            if units >= self.batch_size or len(cur) > 256:
                batches.append(cur)
                units, cur = 0, []
        if cur and (not self.train or units > self.batch_size / 2):     # (an empty trailing batch is dropped, see AMRLoader)
            batches.append(cur)
        if self.train:
            self.rng.shuffle(batches)
        return batches

    def __iter__(self):
        for b in self.batch_indices():
            yield batchify_dependency([self.data[i] for i in b], self.vocabs, n_threads=self.n_threads,
                                      unk_rate=self.unk_rate, rng=self.rng, index_prep=self.index_prep)

    def jobs(self):
        """The same batches as small picklable job records for ``Prefetcher(..., runner=loader.run_job, processes=True)``:
        (example indices, seed of a private <UNK>-noise generator), drawn from ``rng`` in batch order."""
        for b in self.batch_indices():
            yield (b, self.rng.getrandbits(63))

    def run_job(self, job):
        import random
        b, unk_seed = job
        return batchify_dependency([self.data[i] for i in b], self.vocabs, n_threads=self.n_threads, unk_rate=self.unk_rate,
                                   rng=random.Random(unk_seed), index_prep=self.index_prep)

    def thunks(self):
        """The same batches as callables (``Prefetcher`` runs a callable on its worker thread, so several workers assemble
        batches in parallel; plain iteration assembles under the prefetcher's source lock, one at a time).  The <UNK> noise
        of a batch then draws from a private ``random.Random`` seeded from ``rng`` when the thunk is CREATED, so the batches do
        not depend on which worker runs first (they differ from plain iteration's draws, which share ``rng``)."""
        import random
        for b in self.batch_indices():
            trees, sub = [self.data[i] for i in b], random.Random(self.rng.getrandbits(63))
            yield lambda trees=trees, sub=sub: batchify_dependency(trees, self.vocabs, n_threads=self.n_threads, unk_rate=self.unk_rate,
                                                                   rng=sub, index_prep=self.index_prep)


# ------------------------------------------------------------------------------------------------ generator flavour
def _edges_from_paths(item, rel_vocab):
    """The preprocessed AMR items store, per ordered pair of BFS positions, the list of shortest label paths
    (generator/AMRGraph.py:100-115) but not the graph.  Its edges are exactly the pairs joined by a path of length 1, and
    because positions are BFS discovery order, inserting them sorted by (source, target) position reproduces that order."""
    n = len(item['concept'])
    rel = item['relation']
    edges = []
    for i in range(n):
        row = rel[str(i)] if str(i) in rel else rel[i]
        for j in range(n):
            for path in (row[str(j)] if str(j) in row else row[j]):
                if len(path['edge']) == 1:
                    edges.append((i, j, rel_vocab.token2idx(path['edge'][0])))
                    break
    import numpy as np
    return n, 0, np.array(edges, dtype=np.int32).reshape(-1, 3)


def _item_graph(item, rel_vocab, cache=None):
    """(n, root, edges) of an item.  The recovery is a Python loop over all n^2 pairs (0.5 s for a 64 x 100-node batch) and
    does not depend on the batch, so a loader passes a ``cache`` dict (keyed by the item object's id; the loader keeps the
    items alive) and recovers every graph once; the items themselves are never written to (they stay JSON-serialisable for
    ``record()`` consumers)."""
    if cache is None:
        return _edges_from_paths(item, rel_vocab)
    g = cache.get(id(item))
    if g is None or g[0] is not rel_vocab or g[1] is not item:
        g = cache[id(item)] = (rel_vocab, item, _edges_from_paths(item, rel_vocab))
    return g[2]


def batchify_amr(items, vocabs, train=True, seed=0, n_threads=0, unk_rate=0., rng=None, index_prep=True, graph_cache=None):
    """``unk_rate`` / ``rng``: <UNK> noise on ``concept`` and ``token_in`` (generator/data.py:127,244).
    Generator flavour (generator/data.py:126-267).  items: dicts with 'concept' (BFS order), 'depth', 'relation'
    (path lists, only used to recover the edges), 'token', and optionally 'abstract'.  train=True draws ONE shortest path
    per pair, uniformly among the alternatives like the reference's random.choice (from a splitmix64 stream seeded with
    ``seed``); train=False keeps them all: relation is [n,n,B,K], type 0 = <PAD> (data.py:178-232).  The alternatives of a
    pair are the reference's set; their order over K and the numbering of the types follow this module's enumeration
    (the model averages over K, so neither is observable)."""
    rv = vocabs['relation']
    graphs = [_item_graph(x, rv, graph_cache) for x in items]
    if index_prep == "device_all":
        # the all-pairs work, the bank, the tries and the relation index are all left to the consumer's device: ship the graphs
        from .relbatch_hip import graphs_csr
        csr = graphs_csr(graphs)
        for b, x in enumerate(items):
            lo, hi = int(csr['node_off'][b]), int(csr['node_off'][b + 1])
            assert csr['order'][lo:hi].tolist() == list(range(len(x['concept']))), "items must list their concepts in BFS order"
        rel = {'relation_graphs': RelationGraphs(csr, relation_special_ids(rv), relbatch.PATH_UNIFORM if train else relbatch.PATH_ALL, seed, graphs=graphs)}
    else:
        rel = relbatch.build_relation_batch(graphs, relation_special_ids(rv),
                                            path_mode=relbatch.PATH_UNIFORM if train else relbatch.PATH_ALL, seed=seed,
                                            n_threads=n_threads)
        for b, x in enumerate(items):
            n = len(x['concept'])
            assert rel['order'][b, :n].tolist() == list(range(n)), "items must list their concepts in BFS order"
        rel = {k: rel[k] for k in ('relation', 'relation_bank', 'relation_length')}
    cps, t2is, i2ts = [], [], []
    for x in items:
        cp_seq, t2i, i2t = copy_vocab(x['concept'], vocabs['predictable_token'])
        cps.append(cp_seq); t2is.append(t2i); i2ts.append(i2t)
    aug = [[STR] + list(x['token']) + [END] for x in items]
    with_cls = [[CLS] + list(x['concept']) for x in items]
    return _index_prep({
        'concept': lists_to_tensor(with_cls, vocabs['concept'], unk_rate=unk_rate, rng=rng),
        'concept_char': strings_to_char_tensor(with_cls, vocabs['concept_char']),
        'concept_depth': lists_to_tensor([[0] + list(x['depth']) for x in items]),
        **rel,
        'local_idx2token': i2ts, 'local_token2idx': t2is,
        'token_in': lists_to_tensor(aug, vocabs['token'], unk_rate=unk_rate, rng=rng)[:-1],
        'token_char_in': strings_to_char_tensor(aug, vocabs['token_char'])[:-1],
        'token_out': lists_to_tensor(aug, vocabs['predictable_token'], t2is)[1:],
        'cp_seq': lists_to_tensor(cps, vocabs['predictable_token'], t2is),
        'abstract': [x.get('abstract') for x in items],
    }, index_prep)   # train batches also carry 'relation_index' (eval batches are [n,n,B,K]: not factored)


def batchify_targets(sequences, vocabs, local_token2idx):
    """Decoder inputs and targets of given token-string lists, exactly as the two batchify functions build them for a batch's own
    sentences (<STR> + tokens for the input, tokens + <END> for the target): ``sequences[i]`` is scored against the graph whose copy
    table is ``local_token2idx[i]`` (token -> copy id; it takes precedence over the predictable vocabulary, and a string in neither
    is <UNK>).  Returns int64 'token_in' [T,N], 'token_char_in' [T,N,chars], 'token_out' [T,N] (what Generator.score feeds)."""
    if len(sequences) != len(local_token2idx):
        raise ValueError("%d sequences for %d copy tables" % (len(sequences), len(local_token2idx)))
    if not sequences:
        raise ValueError("nothing to score: no target sequence")
    for x in sequences:
        if isinstance(x, str) or not all(isinstance(w, str) for w in x):
            raise ValueError("a target is a list of token strings, got %r" % (x,))
    aug = [[STR] + list(x) + [END] for x in sequences]
    return {
        'token_in': lists_to_tensor(aug, vocabs['token'])[:-1],
        'token_char_in': strings_to_char_tensor(aug, vocabs['token_char'])[:-1],
        'token_out': lists_to_tensor(aug, vocabs['predictable_token'], list(local_token2idx))[1:],
    }


class AMRLoader(object):
    """Batching policy of generator/data.py:269-316 (``DataLoader``): the preprocessed JSON items are shuffled and (stably)
    sorted by size ``n_tokens + n_concepts**2`` when training, packed greedily until a batch holds ``batch_size`` size units
    (or 257 items), a trailing batch is kept if it is more than half full (always in evaluation), and the batch order is
    shuffled.  Both shuffles draw from ``rng`` (default: the ``random`` module, like the reference) BEFORE the first batch is
    assembled, so under the same seed the batches and their order are the reference's.  Yields batchify_amr dicts (with
    ``record()``: (batch, items) pairs, data.py:287-288,313-316); the path sampling of a training batch is seeded from
    ``rng`` per batch.  The graph of every item is recovered from its path lists once, at load time."""

    def __init__(self, vocabs, filename, batch_size, for_train, rng=None, n_threads=0, index_prep="auto", graphs=None):
        """``graphs``: (n, root, edges) per item when the caller already holds them (gtos_amd.synth.make_amr_items): the items
        then need no 'relation' path lists."""
        import json
        import random
        if isinstance(filename, str):
            with open(filename, encoding='utf8') as fi:
                self.data = json.load(fi)
        else:
            self.data = list(filename)
        self.vocabs, self.batch_size, self.train = vocabs, batch_size, for_train
        self.rng = rng if rng is not None else random
        self.n_threads = n_threads
        self.unk_rate = 0.
        self.record_flag = False
        self.index_prep = resolve_index_prep(index_prep)
        self._graphs = {}
        if graphs is not None:
            assert len(graphs) == len(self.data)
            for d, g in zip(self.data, graphs):
                self._graphs[id(d)] = (vocabs['relation'], d, g)
        elif vocabs is not None:
            for d in self.data:
                _item_graph(d, vocabs['relation'], self._graphs)

    def set_unk_rate(self, x):
        """generator/data.py:284-285; train.py calls it with --unk_rate."""
        self.unk_rate = x

    def record(self):
        self.record_flag = True

    @staticmethod
    def size_of(item):
        return len(item['token']) + len(item['concept']) ** 2

    def batch_indices(self):
        idx = list(range(len(self.data)))
        if self.train:
            self.rng.shuffle(idx)
            idx.sort(key=lambda i: self.size_of(self.data[i]))
        batches, units, cur = [], 0, []
        for i in idx:
            units += self.size_of(self.data[i])
            cur.append(i)
            if units >= self.batch_size or len(cur) > 256:
                batches.append(cur)
                units, cur = 0, []
        # the reference appends the trailing batch in evaluation even when the last item closed a batch exactly and nothing is
        # left (generator/data.py:306-307: batchify then fails on the empty list at the end of a dev pass); an empty batch is
        # dropped here -- the non-empty compositions are the reference's
        if cur and (not self.train or units > self.batch_size / 2):
            batches.append(cur)
        if self.train:
            self.rng.shuffle(batches)
        return batches

    def _assemble(self, items, seed, rng):
        batch = batchify_amr(items, self.vocabs, train=self.train, seed=seed, n_threads=self.n_threads, unk_rate=self.unk_rate,
                             rng=rng, index_prep=self.index_prep, graph_cache=self._graphs)
        return (batch, items) if self.record_flag else batch

    def __iter__(self):
        for b in self.batch_indices():
            yield self._assemble([self.data[i] for i in b], self.rng.getrandbits(63), self.rng)

    def jobs(self):
        """Small picklable job records for ``Prefetcher(..., runner=loader.run_job, processes=True)``: (item indices,
        path-sampling seed, seed of a private <UNK>-noise generator), drawn from ``rng`` in batch order -- the same draws as
        ``thunks()``, so both give the same batches."""
        for b in self.batch_indices():
            yield (b, self.rng.getrandbits(63), self.rng.getrandbits(63))

    def run_job(self, job):
        import random
        b, seed, unk_seed = job
        return self._assemble([self.data[i] for i in b], seed, random.Random(unk_seed))

    def thunks(self):
        """The same batches as callables for ``Prefetcher(workers > 1)`` (see DependencyLoader.thunks): path-sampling seed and
        a private <UNK>-noise generator are drawn from ``rng`` when the thunk is created, in batch order."""
        import random
        for b in self.batch_indices():
            items, seed, sub = [self.data[i] for i in b], self.rng.getrandbits(63), random.Random(self.rng.getrandbits(63))
            yield lambda items=items, seed=seed, sub=sub: self._assemble(items, seed, sub)


# ------------------------------------------------------------------------------------------------ host / device overlap
def _device_tensors(obj, seen=None):
    """Every tensor reachable from a batch value: tensors, the index objects (PathTrie / TrieSide / RelationIndex keep theirs
    as attributes), lists / tuples / dicts of those."""
    seen = set() if seen is None else seen
    if id(obj) in seen:
        return
    seen.add(id(obj))
    if isinstance(obj, torch.Tensor):
        yield obj
    elif isinstance(obj, dict):
        for v in obj.values():
            yield from _device_tensors(v, seen)
    elif isinstance(obj, (list, tuple)):
        if obj and not isinstance(obj[0], (str, int, float)):      # token / id lists: nothing to find
            for v in obj:
                yield from _device_tensors(v, seen)
    elif hasattr(obj, "__dict__") and not isinstance(obj, type):
        for v in vars(obj).values():
            yield from _device_tensors(v, seen)


_PACK_ALIGN = 256


def _pack_batch(batch, shared=False):
    """A batch (nested dicts / lists / index objects holding CPU tensors) as (pickle bytes, ONE flat uint8 tensor): every tensor
    is copied to a 256-byte aligned offset of the flat buffer and replaced by an (offset, shape, dtype) record in the pickle.
    A worker process hands the pair to its parent through ONE shared-memory segment instead of one per tensor (a C2 batch has
    45), and the parent uploads it with ONE host-to-device copy."""
    import io
    import pickle
    tensors, off = [], [0]

    class P(pickle.Pickler):
        def persistent_id(self, obj):
            if isinstance(obj, torch.Tensor):
                t = obj.detach().contiguous()
                o = off[0]
                tensors.append((o, t))
                off[0] = (o + t.numel() * t.element_size() + _PACK_ALIGN - 1) // _PACK_ALIGN * _PACK_ALIGN
                return ("gtos_tensor", o, tuple(t.shape), str(t.dtype).replace("torch.", ""))
            return None
    buf = io.BytesIO()
    P(buf, protocol=pickle.HIGHEST_PROTOCOL).dump(batch)
    nbytes = max(off[0], _PACK_ALIGN)
    if shared:                      # straight into a shared-memory segment: no second copy by share_memory_()
        flat = torch.empty(0, dtype=torch.uint8).set_(torch.UntypedStorage._new_shared(nbytes))
    else:
        flat = torch.empty(nbytes, dtype=torch.uint8)
    for o, t in tensors:
        n = t.numel() * t.element_size()
        if n:
            flat[o:o + n] = t.view(-1).view(torch.uint8) if t.dim() else t.reshape(1).view(torch.uint8)
    return buf.getvalue(), flat


def _unpack_batch(meta, flat):
    """Inverse of _pack_batch; the tensors are VIEWS of ``flat`` (which may already live on the device)."""
    import io
    import pickle

    class U(pickle.Unpickler):
        def persistent_load(self, pid):
            tag, o, shape, dtype = pid
            assert tag == "gtos_tensor"
            dt_ = getattr(torch, dtype)
            n = 1
            for d_ in shape:
                n *= d_
            nbytes = n * torch.empty((), dtype=dt_).element_size()
            return flat[o:o + nbytes].view(dt_).view(shape)
    return U(io.BytesIO(meta)).load()


def _process_worker(runner, jobq, resq):
    """Main loop of a forked loader process: CPU work only (the parent's GPU context is never touched here)."""
    torch.set_num_threads(1)
    while True:
        item = jobq.get()
        if item is None:
            break
        k, job = item
        try:
            meta, flat = _pack_batch(runner(job), shared=True)
            resq.put((k, meta, flat, None))
        except BaseException as e:                    # reported to the consumer through the receiver thread
            import traceback
            resq.put((k, None, None, "%r\n%s" % (e, traceback.format_exc())))


class Prefetcher(object):
    """Keeps ``depth`` batches assembled ahead of the consumer on background threads or worker processes.

    Batch assembly is host work -- graph paths + relation bank, path tries, relation index (csrc_host) -- and all of it runs
    inside libgtos_host.so, which ctypes calls with the GIL released, so it overlaps the GPU step driven by the main thread.
    The reference assembles every batch synchronously in the training loop (generator/data.py:290-316).

    * ``batches`` yields batch dicts or CALLABLES returning one.  The source iterable is advanced under a lock, so a loader
      that assembles inside ``__next__`` (``iter(AMRLoader)``) is serialised no matter how many ``workers`` there are;
      ``workers > 1`` only pays off for sources that yield callables (``AMRLoader.thunks()``, ``DependencyLoader.thunks()``,
      or ``(lambda i=i: make(i)) for i in ...``), which run on the worker that took them.
    * With ``device`` the finished batch is copied to the GPU on a dedicated copy stream (pinned staging).  When the consumer
      takes a batch, its current stream is made to wait for that copy AND every device tensor of the batch (including those
      inside PathTrie / RelationIndex) is ``record_stream``-ed on the consumer's stream: the blocks live in the copy stream's
      pool, and without the record the caching allocator could hand them to a later upload while the consumer's kernels
      (backward, optimizer) still read them.
    * ``processes=True`` with ``runner``: the source yields small picklable JOB records and ``runner(job)`` assembles the batch in
      one of ``workers`` forked worker PROCESSES (``loader.jobs()`` / ``loader.run_job``).  Threads share the interpreter lock
      with the training loop, whose ~1,200 kernel launches per step are Python work: every Python-level loop of the assembly
      (token / character tensors, copy vocabularies) stalls the launch thread, and more worker threads make the step SLOWER
      (measured at C2: 69.6 / 75.4 / 98.0 ms per step with 2 / 4 / 8 threads against 64.2 ms on a pre-built batch).  Worker
      processes have their own interpreter; finished batches come back through shared memory (torch.multiprocessing) and a
      single receiver thread uploads them.  The workers are forked at construction and must not touch the GPU.
    * Order of the batches is the iterable's order.  ``close()`` (also on garbage collection / context exit) stops the
      workers; batches already assembled are dropped."""

    def __init__(self, batches, depth=2, workers=1, device=None, processes=False, runner=None, device_tries=False, prep_in_worker=False):
        import threading
        self._it = iter(batches)
        self._device_tries = device_tries
        self.stats = {"batches": 0, "queue_wait_s": 0.0, "device_prep_s": 0.0}     # where __next__ spent the consumer's time
        # device-side preparation (relation tensors / index / tries of a batch that ships without them) on the upload thread instead of
        # the consumer's: its host reads then stall the loader thread, not the training loop (the HIP builders are a few dozen
        # allocations and ctypes calls per batch; the torch-op trie builder's ~200 small calls belonged on the consumer, see __next__)
        self._prep_in_worker = bool(prep_in_worker)
        self._prep_lock = threading.Lock()
        self._out = {}
        self._cv = threading.Condition()          # hand-over lock: depth reservation, finished batches, the consumer's wait
        self._src_lock = threading.Lock()         # source advance (taken before _cv by the workers: keeps slots and items in order)
        self._next_in, self._next_out, self._done, self._err, self._stop = 0, 0, False, None, False
        self._depth = max(1, depth)
        self._device = torch.device(device) if device is not None else None
        self._copy_stream = torch.cuda.Stream(self._device) if self._device is not None and self._device.type == "cuda" else None
        self.workers = max(1, workers)
        self._procs = []
        if processes:
            if runner is None:
                raise ValueError("processes=True needs runner(job) -> batch (e.g. loader.run_job with loader.jobs() as the source)")
            import torch.multiprocessing as mp
            ctx = mp.get_context("fork")          # the runner and everything it references are inherited, not pickled
            self._jobq, self._resq = ctx.Queue(), ctx.Queue()
            self._procs = [ctx.Process(target=_process_worker, args=(runner, self._jobq, self._resq), daemon=True)
                           for _ in range(self.workers)]
            for p_ in self._procs:
                p_.start()
            self._threads = [threading.Thread(target=self._feed, daemon=True), threading.Thread(target=self._receive, daemon=True)]
        else:
            self._threads = [threading.Thread(target=self._work, daemon=True) for _ in range(self.workers)]
        for t in self._threads:
            t.start()

    def _take(self):
        """Reserve a slot within ``depth`` of the consumer, then take the next source item.  The slot is reserved under the
        hand-over lock ``_cv`` (held for a few instructions only); the source advances under ``_src_lock``, which every worker takes
        FIRST, so reservations and source items stay in the same order while the consumer's ``__next__`` -- which needs ``_cv`` alone
        -- never waits for a source that assembles a whole batch inside its ``__next__`` (``iter(AMRLoader)``)."""
        with self._src_lock:
            with self._cv:
                self._cv.wait_for(lambda: self._stop or self._done or self._err is not None or
                                  self._next_in - self._next_out < self._depth)
                if self._stop or self._done or self._err is not None:
                    return None, None
                k = self._next_in
                self._next_in += 1
            try:
                item = next(self._it)
            except StopIteration:
                with self._cv:
                    self._next_in -= 1                   # nobody else reserved meanwhile: _src_lock is still held
                    self._done = True
                    self._cv.notify_all()
                return None, None
            except BaseException as e:                   # a failing source: hand the error to the consumer like a failing worker
                with self._cv:
                    self._next_in -= 1
                    if self._err is None:
                        self._err = e
                    self._cv.notify_all()
                return None, None
            return k, item

    def _needs_prep(self, b0):
        return (isinstance(b0, dict) and (self._device_tries or 'relation_graphs' in b0) and
                ('relation_graphs' in b0 or ('relation_trie' not in b0 and 'relation_bank' in b0)))

    def _device_prep(self, b0):
        """The relation tensors of a batch that ships its graphs (index_prep="device_all": gtos_amd.relbatch_hip), their relation index
        (gtos_amd.relindex_hip) and the tries of a batch that came without them, built on the copy stream by the calling thread.
        Returns (what was made, an event behind it or None without a device)."""
        def prep():
            made = []
            if 'relation_graphs' in b0:
                attach_device_relations(b0, self._device)
                made += [b0['relation'], b0['relation_bank'], b0['relation_length']]
                if 'relation_index' not in b0:
                    attach_device_relation_index(b0)
                    made.append(b0.get('relation_index'))
            if 'relation_trie' not in b0:
                attach_device_tries(b0, self._device_tries or "hip")
                made.append(b0.get('relation_trie'))
            return made
        with self._prep_lock:
            if self._copy_stream is not None:
                with torch.cuda.stream(self._copy_stream):
                    made = prep()
                    ev = torch.cuda.Event()
                    ev.record(self._copy_stream)
                return made, ev
            return prep(), None

    def _upload(self, batch):
        with torch.cuda.stream(self._copy_stream):
            def up(v):                               # (no pin_memory(): a fresh pinned allocation per tensor and batch costs more
                if isinstance(v, torch.Tensor):      #  than the staged copy it saves, and only this worker waits for the copy)
                    return v.to(self._device, non_blocking=True)
                return v.to(self._device) if hasattr(v, "to") else v
            if isinstance(batch, tuple):           # (batch, items) of a recording loader
                out = (dict((n, up(v)) for n, v in batch[0].items()),) + tuple(batch[1:])
            else:
                out = {n: up(v) for n, v in batch.items()}
            ev = torch.cuda.Event()
            ev.record(self._copy_stream)
        return out, ev

    def _work(self):
        try:
            while True:
                k, item = self._take()
                if k is None:
                    break
                batch = item() if callable(item) else item        # a callable defers the assembly to this thread
                ev = None
                if self._copy_stream is not None:
                    batch, ev = self._upload(batch)
                extra = None
                b0 = batch[0] if isinstance(batch, tuple) else batch
                if self._prep_in_worker and self._needs_prep(b0):
                    extra, ev2 = self._device_prep(b0)
                    ev = ev2 if ev2 is not None else ev
                with self._cv:
                    if self._stop:
                        break
                    self._out[k] = (batch, ev, None, extra)
                    self._cv.notify_all()
        except BaseException as e:            # surfaced in the consumer
            with self._cv:
                self._err = e
                self._cv.notify_all()
        finally:
            with self._cv:
                self._cv.notify_all()

    # ---- process mode: a feeder thread hands out jobs within ``depth`` of the consumer, a receiver thread collects results
    def _feed(self):
        try:
            while True:
                k, job = self._take()
                if k is None:
                    break
                self._jobq.put((k, job))
        except BaseException as e:
            with self._cv:
                self._err = e
                self._cv.notify_all()

    def _receive(self):
        import queue
        try:
            while True:
                with self._cv:
                    if self._stop or self._err is not None:
                        break
                    if self._done and len(self._out) + self._next_out >= self._next_in:
                        break
                try:
                    k, meta, flat, err = self._resq.get(timeout=0.2)
                except queue.Empty:
                    if any(not p_.is_alive() for p_ in self._procs) and not self._stop:
                        raise RuntimeError("a loader worker process died")
                    continue
                if err is not None:
                    raise RuntimeError("loader worker failed: %s" % err)
                # this thread shares the interpreter lock with the training loop: one shared-memory segment to map, ONE
                # host-to-device copy of the whole batch, then the tensors are rebuilt as views of the device buffer
                ev = None
                if self._copy_stream is not None:
                    with torch.cuda.stream(self._copy_stream):
                        flat = flat.to(self._device, non_blocking=True)
                        ev = torch.cuda.Event()
                        ev.record(self._copy_stream)
                batch = _unpack_batch(meta, flat)
                extra = None
                b0 = batch[0] if isinstance(batch, tuple) else batch
                if self._prep_in_worker and self._needs_prep(b0):
                    extra, ev2 = self._device_prep(b0)
                    ev = ev2 if ev2 is not None else ev
                with self._cv:
                    if self._stop:
                        break
                    self._out[k] = (batch, ev, flat, extra)  # every tensor of the batch is a view of `flat` (or listed in `extra`)
                    self._cv.notify_all()
        except BaseException as e:
            with self._cv:
                self._err = e
                self._cv.notify_all()
        finally:
            with self._cv:
                self._cv.notify_all()

    def close(self):
        """Stop the workers and release everything in flight.  Safe to call more than once; joins the helper threads so that no
        thread of this object can still be inside a device call when the interpreter (and the HIP runtime) shuts down."""
        import threading
        with self._cv:
            already = self._stop
            self._stop = True
            self._out.clear()
            self._cv.notify_all()
        procs, self._procs = self._procs, []
        for p_ in procs:
            try:
                self._jobq.put_nowait(None)
            except Exception:
                pass
        for p_ in procs:
            p_.join(timeout=0.5)
            if p_.is_alive():
                p_.terminate()
                p_.join(timeout=1.0)
        if not already:
            me = threading.current_thread()
            for t in self._threads:
                if t is not me and t.is_alive():
                    t.join(timeout=2.0)
        if procs:
            # no draining: a worker terminated in the middle of a put leaves a PARTIAL message in the pipe, and a get on it blocks
            # forever inside recv (round 3: bench.py --fresh-batches --workers 2 hung in close()).  Results nobody will take die
            # with the queue; their shared-memory segments go with the workers' file descriptors.
            for q_ in (self._resq, self._jobq):
                try:
                    q_.close()
                    q_.cancel_join_thread()
                except Exception:
                    pass

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __iter__(self):
        return self

    def __next__(self):
        import time
        t_in = time.perf_counter()
        with self._cv:
            self._cv.wait_for(lambda: self._next_out in self._out or self._err is not None or self._stop or
                              (self._done and self._next_out >= self._next_in))
            if self._err is not None:
                raise self._err
            if self._next_out not in self._out:       # source exhausted (or closed) and everything taken from it handed out
                raise StopIteration
            batch, ev, flat, extra = self._out.pop(self._next_out)
            self._next_out += 1
            self._cv.notify_all()
        t_got = time.perf_counter()
        self.stats["batches"] += 1
        self.stats["queue_wait_s"] += t_got - t_in            # the consumer waited for a finished batch (loader too slow / too shallow)
        b0 = batch[0] if isinstance(batch, tuple) else batch
        if self._needs_prep(b0):
            # Index preparation left to the device, done HERE, by the consumer's thread, on the copy stream (behind the batch's upload,
            # beside the previous step's kernels) unless prep_in_worker moved it to the upload thread.  Built on the upload thread the
            # torch-op tries cost 0.2 s per batch: ~200 small torch calls, each waiting for the interpreter lock the training loop
            # holds (round 3, C2, 2 worker processes: 230 ms per step).
            extra, ev2 = self._device_prep(b0)
            ev = ev2 if ev2 is not None else ev
        self.stats["device_prep_s"] += time.perf_counter() - t_got      # host side of the device-side preparation (launches + host reads)
        if ev is not None:
            cur = torch.cuda.current_stream(self._device)
            cur.wait_event(ev)
            if flat is not None:
                flat.record_stream(cur)              # one storage behind every tensor of the batch
                for t in _device_tensors(extra):     # (device-built tries are not views of it)
                    if t.is_cuda:
                        t.record_stream(cur)
            else:
                for t in _device_tensors(batch):
                    if t.is_cuda:
                        t.record_stream(cur)
        return batch
