"""One training step of the gtos Generator on MI355X, data-parallel over RCCL.

Counterpart of the hot loop of /root/reference/generator/train.py:136-154: forward -> loss -> (abnormal-loss rule)
-> backward -> gradient averaging -> clip -> lr schedule -> Adam -> zero_grad.  Differences by design:
  * gradients live in one flat bucket cut into a few contiguous SEGMENTS in reverse execution order (decoder ->
    sentence encoder -> graph encoder -> input encoders); each segment is all-reduced (RCCL over xGMI, async) from inside
    backward as soon as the autograd graph has passed the segment's boundary, so only the last segment's collective is
    exposed -- instead of 182 blocking per-parameter all-reduces after backward (train.py:74-79);
  * the abnormal-loss skip (train.py:142-145) and the lr schedule are evaluated ON THE DEVICE (gtos_step_control): the host
    never reads the loss between forward and backward, so the launch queue stays full (the reference's ``loss.item()`` in
    front of ``backward`` drains it every step).  A discarded batch still runs its backward; the Adam kernel reads the skip
    flag and leaves parameters and moments untouched.  Data parallel, the decision is COLLECTIVE (MAX all-reduce of the
    flag on the device), because the reference's rank-local ``continue`` would desynchronise the collective sequence;
  * dropout streams are decorrelated across ranks by seeding the hash stream with base + rank after the (identical)
    weight initialisation, like train.py:113-116.
"""
import math
import os
import time

import torch
import torch.distributed as dist

from . import ops
from ._lib import call, ptr, stream
from .flat import FlatParams

# segment 0 finishes first in backward.  The LAST segment is reduced after backward() returned (it holds everything whose
# gradient is only known to be complete then: the input encoders, the relation GRU's side-stream weight gradients).
GENERATOR_SEGMENTS = ("decoder.", "snt_encoder.", ("graph_encoder.", "probe_generator."))
# steps the host may queue ahead of the device (0: unbounded, as up to round 4); see Trainer.step
MAX_STEPS_AHEAD = int(os.environ.get("GTOS_MAX_STEPS_AHEAD", "2"))


def generator_segment_of(name):
    for i, pref in enumerate(GENERATOR_SEGMENTS):
        if name.startswith(pref):
            return i
    return len(GENERATOR_SEGMENTS)


def discard_partial_step(flat):
    """A step that raised between its forward and the optimizer: drop the small weight gradients its backward noted (ops.discard_dw) and
    zero the bucket, so that nothing of the failed step reaches the next one."""
    ops.discard_dw(flat.grad.device)
    ops.join_side(flat.grad.device)
    flat.grad.zero_()


class SegmentBoundaryFn(torch.autograd.Function):
    """Identity on ``tensors``; its backward runs once the gradients of ALL of them are complete, i.e. when every
    autograd node downstream of the boundary has run -- the moment the parameters of segments <= ``seg`` hold their final
    gradients.  ``sync.segment_ready(seg)`` then launches their all-reduce."""

    @staticmethod
    def forward(ctx, sync, seg, *tensors):
        ctx.sync, ctx.seg = sync, seg
        return tuple(t.view_as(t) for t in tensors)

    @staticmethod
    def backward(ctx, *grads):
        ctx.sync.segment_ready(ctx.seg)
        return (None, None) + grads


class Trainer:
    def __init__(self, model, embed_dim, warmup_steps=2000, compute_dtype=torch.float32, world_size=1, rank=0,
                 segment_of="auto", base_seed=19940117, overlap=True, force_collectives=False):
        """``force_collectives``: issue the gradient collectives even with world_size == 1 (an initialised process group of one
        rank): the RCCL code path -- async all-reduce of bucket views from inside backward -- on a single GPU."""
        self.model = model
        self.embed_dim, self.warmup_steps = embed_dim, warmup_steps
        self.world_size, self.rank = world_size, rank
        if segment_of == "auto":
            names = [n for n, _ in model.named_parameters()]
            segment_of = generator_segment_of if any(n.startswith("graph_encoder.") for n in names) else None
        self.flat = FlatParams(model, mirror_dtype=compute_dtype, segment_of=segment_of)
        dev = self.flat.param.device
        self._state = torch.zeros(3, dtype=torch.float64, device=dev)       # {loss_acm, batches_acm, discarded}, device-resident
        self._flag = torch.zeros(1, dtype=torch.float32, device=dev)
        self._ctl = torch.zeros(2, dtype=torch.float32, device=dev)         # {lr of this step, skip}
        self.steps_issued = 0           # host-side count of step() calls: an upper bound of batches_acm (no device read needed)
        self._counters, self._counters_at = None, -1
        self.collective = world_size > 1 or force_collectives
        self.overlap = overlap and self.collective and len(self.flat.segments) > 1
        self._launched = 0              # segments [0, _launched) have their all-reduce in flight
        self._works = []
        self.comm_exposed_s = 0.0       # host time spent waiting for collectives after backward (gloo blocks here)
        self._comm_events = []          # (start, end) HIP events around the waits on the compute stream: the GPU-side exposed time
        self._done_events = [] if (dev.type == "cuda" and MAX_STEPS_AHEAD > 0) else None    # end-of-step events of the steps in flight
        if self.overlap and hasattr(model, "grad_sync"):
            model.grad_sync = self      # Generator.forward places the SegmentBoundaryFn markers
        if world_size > 1:
            # Replicas must start identical.  The reference relies on every rank seeding torch alike before it builds the model
            # (generator/train.py:98-100); here rank 0's flat parameter buffer is broadcast once (one collective over the whole
            # model, like DistributedDataParallel does at construction), so a rank that was built differently -- another seed, a
            # checkpoint loaded on rank 0 only -- cannot drift silently.
            dist.broadcast(self.flat.param, src=0)
            self.flat.sync_mirror()
            ops.set_seed(base_seed + rank)

    # ---- boundary markers (called from the model's forward)
    def boundary(self, seg, *tensors):
        """Mark the inputs of segment ``seg`` (everything that consumes ``tensors`` belongs to segments <= seg)."""
        if not (self.overlap and torch.is_grad_enabled() and any(t.requires_grad for t in tensors)):
            return tensors
        return SegmentBoundaryFn.apply(self, seg, *tensors)

    def segment_ready(self, seg):
        """Segments 0..seg hold final gradients: put their all-reduce in flight (once, in segment order on every rank)."""
        if self._launched <= seg and self.collective:
            ops.flush_dw(self.flat.grad.device)        # the small layers' batched weight gradients (ops.DW_BATCH) belong to the segment
        while self._launched <= seg and self._launched < len(self.flat.segments):
            lo, hi = self.flat.segments[self._launched]
            self._launched += 1
            if hi > lo and self.collective:
                # async: enqueued on the process group's own stream after the work already on the current stream -- and, when a
                # deferred side-stream product still writes into the bucket (ops.GradAccumGroup.finish_dw), behind that stream too,
                # without stalling this one (ops.behind_side)
                with ops.behind_side(self.flat.grad.device):
                    self._works.append(dist.all_reduce(self.flat.grad[lo:hi], op=dist.ReduceOp.SUM, async_op=True))

    def all_reduce_grads(self):
        """After backward(): launch what backward did not (at least the last segment) and wait for everything."""
        ops.join_side()                    # deferred side-stream gradient GEMMs (gru.py) land before the bucket is read
        self.segment_ready(len(self.flat.segments) - 1)
        timed = bool(self._works) and self.flat.grad.is_cuda
        if timed:
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            ev[0].record()
        t0 = time.perf_counter()
        for w in self._works:
            w.wait()                       # nccl: the current stream waits for the collective; gloo: blocks the host
        self.comm_exposed_s += time.perf_counter() - t0
        if timed:
            ev[1].record()
            self._comm_events.append(ev)
            if len(self._comm_events) > 512:       # nobody is reading them: keep the list bounded
                del self._comm_events[:256]
        self._works, self._launched = [], 0

    def comm_exposed_ms(self, reset=True):
        """Milliseconds the compute stream spent stalled on gradient collectives since the last call (HIP events around the
        waits; needs the stream to be idle, i.e. call it after a synchronize)."""
        ms = sum(s.elapsed_time(e) for s, e in self._comm_events)
        if reset:
            self._comm_events = []
        return ms

    # ---- counters of the reference loop, kept on the device.  READING THEM SYNCHRONISES (one device -> host copy): use
    # ``steps_issued`` (host-side, no read) for per-step cadence checks like the reference's ``batches_acm % print_every`` and read
    # the counters only when something is printed / evaluated.  One read serves all three: ``counters()`` copies the state once
    # per issued step and the properties share that copy, so reference-style logging that touches batches_acm, loss_acm and
    # discarded in one iteration costs one synchronisation, not three.  (A discarded batch still ran its backward and its
    # gradient all-reduce -- only the Adam kernel is skipped)
    def counters(self):
        """(loss_acm, batches_acm, discarded) as of the last issued step: ONE host read, cached until the next ``step()``."""
        if self._counters_at != self.steps_issued or self._counters is None:
            la, ba, di = self._state.tolist()
            self._counters, self._counters_at = (float(la), int(ba), int(di)), self.steps_issued
        return self._counters

    @property
    def batches_acm(self):
        return self.counters()[1]

    @property
    def loss_acm(self):
        return self.counters()[0]

    @property
    def discarded(self):
        return self.counters()[2]

    def set_counters(self, batches_acm, loss_acm, discarded=0):
        """Resume from a checkpoint (train.py keeps batches_acm / loss_acm across restarts)."""
        self._state.copy_(torch.tensor([float(loss_acm), float(batches_acm), float(discarded)], dtype=torch.float64))
        self.steps_issued = int(batches_acm) + int(discarded)
        self._counters = None

    def _control(self, phase, loss):
        """gtos_step_control: phase 0 writes this rank's abnormal-loss flag, phase 1 applies the (all-reduced) flag to the
        counters and writes {lr, skip} for the Adam kernel."""
        call("gtos_step_control", phase, ptr(loss), ptr(self._state), ptr(self._flag), int(self.warmup_steps), int(self.embed_dim),
             ptr(self._ctl), stream())

    def step(self, batch, sync=True):
        """One training step.  ``sync=True`` returns the loss value (float), or None when the batch was discarded -- one host
        read AFTER every launch of the step has been queued.  ``sync=False`` returns a PendingLoss (``.value()`` reads it
        later): the host runs ahead into the next step, which is what the launch-bound small configurations need."""
        if self._done_events is not None:
            # Bounded run-ahead.  Nothing in a step reads the device any more, so the host could queue many steps ahead of it -- and the
            # caching allocator can only recycle a block that was freed on one stream while another still used it once the DEVICE has
            # passed that point: an unbounded run-ahead keeps several steps' worth of such blocks in limbo and mallocs new ones (C2:
            # 237 GB reserved for 44 GB allocated).  Waiting here for the end of step k - MAX_STEPS_AHEAD costs nothing while the device
            # is the bottleneck and never triggers when the host is (the event has long completed).
            while len(self._done_events) >= MAX_STEPS_AHEAD:
                self._done_events.pop(0).synchronize()
        try:
            loss = self.model(batch)
            loss = loss if loss.dtype == torch.float32 else loss.float()
            self._control(0, loss.detach())
            if self.collective and self.steps_issued > self.warmup_steps:       # batches_acm <= steps_issued: never needed earlier
                dist.all_reduce(self._flag, op=dist.ReduceOp.MAX)
            self._control(1, loss.detach())
            self.steps_issued += 1
            loss.backward()
            self.all_reduce_grads()
        except BaseException:
            discard_partial_step(self.flat)
            self._works, self._launched = [], 0     # (data parallel, a rank that raised has left the collective sequence anyway)
            raise
        self.flat.step(None, gscale=1.0 / self.world_size, max_norm=1.0, ctl=self._ctl)
        self.flat.zero_grad()
        res = PendingLoss(torch.cat([loss.detach().reshape(1), self._flag]))
        if self._done_events is not None:
            ev = torch.cuda.Event()
            ev.record()
            self._done_events.append(ev)
        return res.value() if sync else res

    def evaluate(self, batches, totals=None):
        """Held-out evaluation, teacher-forced: ``Generator.score_rows`` (one gtos_copy_eval_fwd) and one gtos_eval_accumulate per
        batch into one device buffer of five fp64 totals, ONE host read at the end; data parallel, each rank passes its own shard of
        batches and the totals are summed by one all-reduce before that read.  Returns ``eval_metrics``: nll_per_token, perplexity,
        accuracy, tokens, sentences and loss (the reference-normalised mean, comparable with the training loss).  ``totals`` (fp64
        [5] on the device) continues a running evaluation.  The training state is left alone: parameters, bf16 mirror, gradient
        bucket, Adam moments, counters, the seed counter and the model's train / eval mode."""
        if totals is None:
            totals = torch.zeros(5, dtype=torch.float64, device=self.flat.param.device)
        pad = self.model.vocabs['predictable_token'].padding_idx
        for batch in batches:
            nll, pred, _, target, _ = self.model.score_rows(batch)
            if nll.numel():
                ops.eval_accumulate(nll, pred, target, pad, totals)
        if self.world_size > 1:
            dist.all_reduce(totals, op=dist.ReduceOp.SUM)       # the one collective of an evaluation
        return eval_metrics(totals.tolist())                    # ... and its one host read

    def validate(self, batches, references=None, beam_size=8, alpha=0.6, max_time_step=100, min_time_step=1, search="device",
                 return_outputs=False, select="best", mbr_weights="uniform", mbr_scale=1.0, **work_options):
        """Held-out validation by decoding, the reference's checkpoint-selection step (generator/work.py ``validate``): per batch
        ``model.work(batch, beam_size, max_time_step, min_time_step, search, **work_options)``, the best hypothesis of every graph by
        ``get_k_best(1, alpha)`` without <STR> / <END>, and three gtos_ngram_overlap launches (gtos_amd.metrics: word order 4 for
        BLEU, punctuation-separated word order 2 and character order 6 for chrF++) accumulated into one device buffer of fp64
        totals (metrics.N_TOTALS: the summed counts, which are integers and exact, the two lengths, the sentence count and the sum
        of the sentence chrF++).  Data parallel, each rank passes its own shard of batches and the totals are summed by one
        all-reduce; then ONE host read, beyond those the searches make.  Returns ``metrics.validation_metrics``: bleu,
        bleu_precisions, brevity_penalty, chrf (corpus chrF++), chrf_avg (mean sentence chrF++), hyp_tokens, ref_tokens, sentences --
        and with ``return_outputs`` also ``outputs``, the hypotheses as token-string lists in batch order.
        ``references``: per batch, one token-string list per graph.  None: they are rebuilt from ``batch['token_out']`` through the
        predictable-token vocabulary and the graph's ``local_idx2token`` (the ids ride to the host on an asynchronous copy queued
        in front of the search, whose own reads complete it); a word that was neither in the vocabulary nor copyable is <UNK> there,
        and an <UNK> matches nothing -- each one is a word and a character of its own -- so such a validation scores a little below
        one on the true strings.  What is scored are the preprocessed token strings as given: no lowercasing, no de-anonymising
        post-processing.
        The training state is left alone, as for ``evaluate``: parameters, bf16 mirror, gradient bucket, Adam moments, counters and
        the model's train / eval mode.  A ``search`` that draws a seed ("sample", "stochastic") without ``seed=`` moves the seed
        counter exactly as ``work`` moves it, once per batch; pass ``seed`` for a repeatable validation.
        ``select``: "best" (above), or "mbr": what is scored per graph is the minimum-Bayes-risk choice among the beam's candidates,
        ``metrics.mbr_select(beams, beam_size, alpha, mbr_weights, mbr_scale)`` -- the candidate with the highest expected sentence
        chrF++ against the candidates themselves, weighted "uniform" (independent samples, search="sample"), by "score" (exp(mbr_scale
        * log-likelihood), n-best lists) or "stochastic" (the importance weights of search="stochastic") -- and ``outputs`` are those
        choices.  It adds two gtos_ngram_overlap_groups launches per batch, scores every candidate against the reference and lets the
        device pick the rows of the choices: at most ONE host read more than "best", for all batches, and only with
        ``return_outputs``.  A graph whose beam offers mbr_select no candidate keeps its ``get_k_best(1, alpha)`` choice.  Any other ``select`` raises ValueError."""
        from . import metrics
        if select not in ("best", "mbr"):
            raise ValueError("select must be 'best' or 'mbr', got %r" % (select,))
        from .vocab import END, PAD
        dev = self.flat.param.device
        totals = torch.zeros(metrics.N_TOTALS, dtype=torch.float64, device=dev)
        vocab = self.model.vocabs['predictable_token']
        outputs, chosen = [], []
        modes = [(m, m.training) for m in self.model.modules()]
        try:
            self.model.eval()
            for i, batch in enumerate(batches):
                ids = done = None
                if references is None:
                    ids, done = _ids_to_host(batch['token_out'])
                beams = self.model.work(batch, beam_size, max_time_step, min_time_step, search, **work_options)
                if select == "mbr":                         # (before get_k_best below, which may merge a beam's two lists)
                    groups, weights = metrics.mbr_candidates(beams, beam_size, alpha, mbr_weights, mbr_scale)
                hyps = [metrics.hypothesis_tokens(best[0]) if best else [] for best in (beam.get_k_best(1, alpha) for beam in beams)]
                if select == "mbr":
                    for b, h in enumerate(hyps):
                        if not groups[b]:                   # no candidate to weigh: the graph keeps its model-score choice
                            groups[b] = [h]
                            if weights is not None:
                                weights[b] = [1.0]
                if references is None:
                    if done is not None:
                        done.synchronize()          # long complete: work() has read the device since
                    refs = []
                    for b, local in enumerate(batch['local_idx2token']):
                        words = [local[y] if y in local else vocab.idx2token(y) for y in ids[:, b].tolist()]
                        refs.append([w for w in words if w not in (END, PAD)])
                else:
                    refs = [list(r) for r in references[i]]
                if len(refs) != len(hyps):
                    raise ValueError("references[%d] holds one token-string list per graph: %d graphs, got %d" % (i, len(hyps), len(refs)))
                if hyps and select == "mbr":
                    # every candidate is scored against its graph's reference and the device picks the rows of the choices: the
                    # host learns the choices only when it has to return them, in one read for all batches
                    sizes = [len(g) for g in groups]
                    _, index = metrics.expected_utility(metrics.pairwise(groups, "char", device=dev)[0],
                                                        metrics.pairwise(groups, "chrf_word", device=dev)[0], sizes,
                                                        None if weights is None else [x for ws in weights for x in ws])
                    rows = torch.tensor([0] + sizes[:-1], dtype=torch.int64).cumsum(0).to(dev) + index
                    flat = [c for g in groups for c in g]
                    pairs = [(r, b) for r, b in enumerate(b for b, n in enumerate(sizes) for _ in range(n))]
                    metrics.accumulate(totals, *(metrics.overlap(flat, refs, pairs, kind, device=dev)[rows]
                                                 for kind in ("word", "chrf_word", "char")))
                    chosen.append(index)
                    outputs += groups
                elif hyps:
                    metrics.accumulate(totals, *(metrics.overlap(hyps, refs, None, kind, device=dev) for kind in ("word", "chrf_word", "char")))
                    outputs += hyps
        finally:
            for m, was in modes:
                m.training = was
        if self.world_size > 1:
            dist.all_reduce(totals, op=dist.ReduceOp.SUM)       # the one collective of a validation
        out = metrics.validation_metrics(totals.tolist())       # ... and its one host read
        if return_outputs:
            if chosen:                                          # select="mbr": outputs holds the candidate groups
                outputs = [g[j] for g, j in zip(outputs, torch.cat(chosen).tolist())]     # ... its one host read more
            out["outputs"] = outputs
        return out


def eval_metrics(totals):
    """The dict of Trainer.evaluate from the five totals of gtos_eval_accumulate (sum nll, tokens, correct, sentences, sum over
    sentences of nll / tokens): corpus NLL per token, its perplexity, token accuracy, and ``loss`` = the reference-normalised mean
    (mean over sentences of the per-sentence mean NLL, decoder.py:91-94: what ``forward`` reports).  NaN where nothing was scored."""
    s, n, ok, sents, norm = (float(v) for v in totals)
    per_token = s / n if n else float("nan")
    return {"nll_per_token": per_token, "perplexity": math.exp(min(per_token, 700.0)) if n else float("nan"),
            "accuracy": ok / n if n else float("nan"), "tokens": int(n), "sentences": int(sents),
            "loss": norm / sents if sents else float("nan")}


def _ids_to_host(t):
    """(host copy of the id tensor ``t``, the event that completes it or None): a device tensor is copied asynchronously into pinned
    memory on the current stream -- the host does not wait here."""
    if not t.is_cuda:
        return t, None
    host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
    host.copy_(t, non_blocking=True)
    done = torch.cuda.Event()
    done.record()
    return host, done


class GraphedStep:
    """A training step captured once as a hipGraph and replayed: for the configurations whose step is a thousand small launches (C1:
    9.7 ms of Python-paced launches around ~3 ms of kernels), when consecutive batches have the SAME shapes -- the captured launch
    plan, every tensor size and every trie level count belongs to the batch it was captured on.

        gs = GraphedStep(trainer, batch)        # warm-up steps + capture (a few real steps on ``batch``)
        pending = gs()                          # one replay = one training step on ``batch``; PendingLoss like Trainer.step(sync=False)

    New token / concept contents may be copied INTO the captured batch's tensors between replays; a batch with another relation
    structure (other trie level sizes, another number of distinct paths) is another launch plan and needs its own capture.

    Dropout: kernel arguments are frozen by the capture, so the library's kernels fold a device-side epoch into their seeds
    (ops.set_seed_epoch) which the captured step increments first thing; torch's own generator is graph-safe by itself.
    Limits: one process (world_size 1: the gradient collectives' host-side bookkeeping is not captured); a batch that carries its path
    trie (``batch['relation_trie']``: the RelationEncoder then takes the sort order and the step sizes from it -- since round 5 also with
    the reference's dropout semantics, whose packed sequence used to be sized by a host read; a bare bank still costs that read and cannot
    be captured) and its relation tensors already built (device builders run before, not inside, the capture).
    Robustness (ROCm 7.2, torch 2.10): C1 captures and replays correctly (equal to the eager steps at dropout 0).
    At C2, where the auxiliary stream is forked in three places, ``hipStreamEndCapture`` crashed inside the runtime, and with every
    use of that stream switched off a replay hung; with one use it worked and bought nothing (the step is not launch-bound).  Use it
    for launch-bound configurations."""

    def __init__(self, trainer, batch, warmup=3):
        if trainer.collective:
            raise ValueError("GraphedStep: single-process training only")
        dev = trainer.flat.grad.device
        self.trainer, self.batch, self._dev = trainer, batch, dev
        self.epoch = torch.zeros((), dtype=torch.int64, device=dev)
        ops.set_seed_epoch(self.epoch)
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):           # torch's capture protocol: a few eager steps on a side stream first (workspaces,
            for _ in range(warmup):             # cuBLAS-style lazy state, the allocator's pools): REAL training steps on ``batch``
                self.epoch.add_(1)
                self._body()
                trainer.steps_issued += 1
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self.epoch.add_(1)
            self._out = self._body()
        torch.cuda.synchronize(dev)
        self.replays = 0

    def _body(self):
        t = self.trainer
        # fork the auxiliary stream into the capture before anything else and join it at the end: the step makes the main stream wait
        # for it in places where, on small inputs, it was never given work -- outside a capture a no-op, inside one a dependency on a
        # stream that is not being captured
        main, side = torch.cuda.current_stream(self._dev), ops.side_stream(self._dev)
        side.wait_stream(main)
        try:
            loss = t.model(self.batch)
            loss = loss if loss.dtype == torch.float32 else loss.float()
            t._control(0, loss.detach())
            t._control(1, loss.detach())
            loss.backward()
            ops.join_side()
        except BaseException:
            discard_partial_step(t.flat)
            raise
        t.flat.step(None, gscale=1.0, max_norm=1.0, ctl=t._ctl)
        t.flat.zero_grad()
        main.wait_stream(side)
        return torch.cat([loss.detach().reshape(1), t._flag])

    def __call__(self):
        self.graph.replay()
        self.replays += 1
        self.trainer.steps_issued += 1
        return PendingLoss(self._out.clone())

    def close(self):
        ops.set_seed_epoch(None)


class PendingLoss:
    """Loss and skip flag of a step, still on the device."""

    def __init__(self, pair):
        self._pair, self._val = pair, False

    def value(self):
        """float, or None when the batch was discarded by the abnormal-loss rule."""
        if self._val is False:
            v, f = self._pair.tolist()
            self._val = None if f > 0 else v
            self._pair = None
        return self._val
