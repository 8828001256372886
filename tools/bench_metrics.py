"""Cost of BLEU / chrF++ validation (gtos_amd.metrics, Trainer.validate) and of the count under it, gtos_ngram_overlap.  Prints one
JSON line:

  validate     per decode batch of `bench.py --decode` (C2 eval batch, 64 synthetic 100-node graphs, beam 8, random weights): the
               seconds of the decode part (model.work, search="device") next to the metric part of Trainer.validate (best hypothesis
               per graph, the references from the batch's token_out, three overlap launches, the accumulation), each ended by a
               device synchronise, interleaved over --repeats
  kernel       gtos_ngram_overlap alone through the C ABI, HIP events around --launches launches after a warm-up, for the three
               statistic kinds (word order 4, punctuation-separated word order 2, character order 6) at 64 pairs (a validation batch),
               512 pairs (the n-best lists of 64 graphs x 8 against their references) and 64 x 8^2 pairs (all pairs of those lists);
               the text is seeded: 64 references of 12..40 words, hypotheses perturbed from them
  counter      the same counts by a plain collections.Counter statement on the host, one pass, for scale; `equal` says that the two
               agree on every pair

    python tools/bench_metrics.py [--config C2] [--beam 8] [--max-steps 50] [--repeats 3] [--launches 50] [--dtype bf16]
"""
import argparse
import collections
import json
import os
import random
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def counter_stats(h, r, n_max):
    out = []
    for n in range(1, n_max + 1):
        ch = collections.Counter(tuple(h[i:i + n]) for i in range(len(h) - n + 1))
        cr = collections.Counter(tuple(r[i:i + n]) for i in range(len(r) - n + 1))
        out.append([sum(min(c, cr[g]) for g, c in ch.items()), max(len(h) - n + 1, 0), max(len(r) - n + 1, 0)])
    return out


def seeded_text(graphs, k, seed=7):
    """``graphs`` references of 12..40 words over a 3000-word vocabulary of 2..9 letter words (some end in punctuation), and k
    hypotheses per reference: words dropped (0.12), replaced (0.08), doubled (0.05)."""
    rng = random.Random(seed)
    letters = "etaoinshrdlucmfwypvbgk"
    vocab = ["".join(rng.choice(letters) for _ in range(rng.randint(2, 9))) + rng.choice(["", "", "", "", ",", "."]) for _ in range(3000)]
    refs = [[vocab[min(int(rng.expovariate(1 / 300.0)), 2999)] for _ in range(rng.randint(12, 40))] for _ in range(graphs)]
    hyps = []
    for r in refs:
        for _ in range(k):
            h = []
            for w in r:
                u = rng.random()
                if u < 0.12:
                    continue
                h += [rng.choice(r)] if u < 0.20 else [w, w] if u < 0.25 else [w]
            hyps.append(h or [r[0]])
    return hyps, refs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--alpha", type=float, default=0.6)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_metrics.py measures on the GPU: no GPU visible")
    from gtos_amd import metrics, synth
    from gtos_amd._lib import call, ptr, stream
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.vocab import END, PAD
    dev = torch.device("cuda:0")
    out = {"metric": "BLEU / chrF++ validation: decode part, metric part and gtos_ngram_overlap alone"}

    # ---- the kernel alone, and the Counter statement
    graphs, k = 64, 8
    hyps, refs = seeded_text(graphs, k)
    first = [hyps[g * k] for g in range(graphs)]
    sets = {"64_validation": (first, [(g, g) for g in range(graphs)]),
            "512_nbest": (hyps, [(g * k + j, g) for g in range(graphs) for j in range(k)]),
            "4096_all_pairs": (hyps, None)}
    kernel, counter, equal = {}, {}, True
    for name, (hs, pairs) in sets.items():
        for kind, n_max in metrics.KINDS.items():
            if pairs is None:                   # all pairs of each n-best list: hypotheses on both sides
                sym, off = metrics.encode(hs, kind)
                rows = [(g * k + i, g * k + j) for g in range(graphs) for i in range(k) for j in range(k)]
            else:
                sym, off = metrics.encode(hs + refs, kind)
                rows = [(i, len(hs) + j) for i, j in pairs]
            pt = torch.tensor(rows, dtype=torch.int32)
            sym_d, off_d, pt_d = sym.to(dev), off.to(dev), pt.to(dev)
            res = torch.empty((len(rows), n_max, 3), dtype=torch.int32, device=dev)

            def launch():
                call("gtos_ngram_overlap", ptr(sym_d), ptr(off_d), off.numel() - 1, ptr(pt_d), len(rows), n_max, ptr(off), ptr(pt),
                     ptr(res), stream())
            for _ in range(3):
                launch()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.launches):
                launch()
            e1.record()
            torch.cuda.synchronize()
            kernel["%s/%s" % (name, kind)] = e0.elapsed_time(e1) / a.launches
            seqs, o = sym.tolist(), off.tolist()
            t0 = time.perf_counter()
            want = [counter_stats(seqs[o[i]:o[i + 1]], seqs[o[j]:o[j + 1]], n_max) for i, j in rows]
            counter["%s/%s" % (name, kind)] = 1e3 * (time.perf_counter() - t0)
            equal = equal and res.cpu().tolist() == want
    out.update(kernel_ms_per_launch=kernel, counter_ms=counter, equal=equal, launches=a.launches,
               symbols_per_row={kind: metrics.encode(hyps, kind)[0].numel() / len(hyps) for kind in metrics.KINDS})

    # ---- Trainer.validate's two parts on the decode benchmark's batch
    cfg = synth.CONFIGS[a.config]
    vocabs = synth.synth_vocabs()
    torch.manual_seed(19940117)
    model = Generator(vocabs, device=dev, depth_size=256 if cfg["kind"] == "dep" else 32, **generator_args(cfg)).to(dev)
    model.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    model.eval()
    batch, stats = synth.make_config_batch(a.config, train=False)
    pv, cp = vocabs['predictable_token'], batch['cp_seq']
    batch_dev = {key: v.to(dev) for key, v in attach_path_trie(batch).items()}
    batch_dev['local_idx2token'] = [{int(i): "copy%d" % int(i) for i in cp[:, b].tolist() if i >= pv.size} for b in range(cp.shape[1])]
    model.work(batch_dev, a.beam, 3, search="device")                         # warm-up
    decode_s, metric_s, result = [], [], None
    for rep in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.beam, a.max_steps, search="device")
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        best = [metrics.hypothesis_tokens(beam.get_k_best(1, a.alpha)[0]) for beam in beams]
        ids = batch_dev['token_out'].cpu()
        truth = []
        for b, local in enumerate(batch_dev['local_idx2token']):
            words = [local[y] if y in local else pv.idx2token(y) for y in ids[:, b].tolist()]
            truth.append([w for w in words if w not in (END, PAD)])
        totals = torch.zeros(metrics.N_TOTALS, dtype=torch.float64, device=dev)
        metrics.accumulate(totals, *(metrics.overlap(best, truth, None, kind, device=dev) for kind in ("word", "chrf_word", "char")))
        result = metrics.validation_metrics(totals.tolist())
        t2 = time.perf_counter()
        if rep:                                                               # (the first pass warms the metric part up)
            decode_s.append(t1 - t0)
            metric_s.append(t2 - t1)
    out.update(validate={"workload": "%s eval batch: %d graphs, beam %d, max %d decoder steps, %s, random weights" % (
        a.config, stats["B"], a.beam, a.max_steps, a.dtype), "decode_seconds": decode_s, "metric_seconds": metric_s,
        "metric_over_decode": [m / d for m, d in zip(metric_s, decode_s)], "scores": result})
    print(json.dumps(out))
    if not equal:
        raise SystemExit("gtos_ngram_overlap and the Counter statement disagree")


if __name__ == "__main__":
    main()
