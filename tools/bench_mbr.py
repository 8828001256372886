"""Cost of minimum-Bayes-risk selection (gtos_amd.metrics.mbr_select) and of the count under it, gtos_ngram_overlap_groups.  Prints
one JSON line:

  kernel     (a) gtos_ngram_overlap_groups alone against gtos_ngram_overlap on the explicit ordered pair list of the same groups, both
             through the C ABI: HIP events around --launches launches after a warm-up of both, the two kernels alternating over
             --repeats rounds (every round's milliseconds per launch is listed, the ratio is taken on the medians).  Shapes: 64
             groups x {8, 32, 64} candidates, character rows at order 6 and punctuation-separated word rows at order 2; the text is
             seeded: a reference of 20..30 words per group, candidates perturbed from it.  `equal` says that the two kernels
             stored the same integers; if they did not, the tool exits non-zero.
  select     (b) on the decode benchmark's batch (C2 eval batch, random weights): the seconds of work(search="sample",
             beam_size=32) next to those of mbr_select on its beams, each ended by a device synchronise, interleaved over --repeats
  chrf       (c) mean sentence chrF++ against the batch's references of the model-score choice (get_k_best(1)), the MBR choice and
             best_of_nbest's choice (the best the list holds, which bounds the other two).  The weights are random and the graphs
             synthetic: this checks the mechanics, it is NOT a statement about quality.  mbr_select's time is mostly host work on
             strings (two encode calls over every candidate); the two launches are part (a)'s figures.

    python tools/bench_mbr.py [--config C2] [--beam 32] [--max-steps 50] [--repeats 3] [--launches 200] [--dtype bf16] [--seed 3]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def seeded_groups(graphs, k, seed=7):
    """``graphs`` groups of k candidates: per group a reference of 20..30 words over a 3000-word vocabulary of 2..9 letter words (some
    end in punctuation), every candidate a perturbation of it: words dropped (0.12), replaced (0.08), doubled (0.05)."""
    rng = random.Random(seed)
    letters = "etaoinshrdlucmfwypvbgk"
    vocab = ["".join(rng.choice(letters) for _ in range(rng.randint(2, 9))) + rng.choice(["", "", "", "", ",", "."]) for _ in range(3000)]
    groups = []
    for _ in range(graphs):
        r = [vocab[min(int(rng.expovariate(1 / 300.0)), 2999)] for _ in range(rng.randint(20, 30))]
        cands = []
        for _ in range(k):
            h = []
            for w in r:
                u = rng.random()
                if u < 0.12:
                    continue
                h += [rng.choice(r)] if u < 0.20 else [w, w] if u < 0.25 else [w]
            cands.append(h or [r[0]])
        groups.append(cands)
    return groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--beam", type=int, default=32)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--alpha", type=float, default=0.6)
    ap.add_argument("--seed", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="part (a) alone")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mbr.py measures on the GPU: no GPU visible")
    from gtos_amd import metrics, synth
    from gtos_amd._lib import call, ptr, stream
    dev = torch.device("cuda:0")
    out = {"metric": "minimum-Bayes-risk selection: gtos_ngram_overlap_groups against gtos_ngram_overlap on the same cells, "
                     "mbr_select next to the sampling decode, chrF++ of the choices"}

    # ---- (a) the two kernels on the same cells
    graphs, kernel, equal = 64, {}, True
    for k in (8, 32, 64):
        groups = seeded_groups(graphs, k)
        rows = [c for g in groups for c in g]
        grp = torch.arange(0, graphs * k + 1, k, dtype=torch.int32)
        cells = graphs * k * k
        idx = torch.arange(k, dtype=torch.int32)
        pt = torch.cat([torch.stack([(g * k + idx).repeat_interleave(k), (g * k + idx).repeat(k)], 1) for g in range(graphs)]).contiguous()
        for kind in ("char", "chrf_word"):
            n_max = metrics.KINDS[kind]
            sym, off = metrics.encode(rows, kind)
            sym_d, off_d, grp_d, pt_d = sym.to(dev), off.to(dev), grp.to(dev), pt.to(dev)
            res_g = torch.zeros((cells, n_max, 3), dtype=torch.int32, device=dev)
            res_p = torch.ones((cells, n_max, 3), dtype=torch.int32, device=dev)

            def grouped():
                call("gtos_ngram_overlap_groups", ptr(sym_d), ptr(off_d), off.numel() - 1, ptr(grp_d), graphs, n_max, ptr(off), ptr(grp),
                     ptr(res_g), stream())

            def listed():
                call("gtos_ngram_overlap", ptr(sym_d), ptr(off_d), off.numel() - 1, ptr(pt_d), cells, n_max, ptr(off), ptr(pt),
                     ptr(res_p), stream())
            for fn in (grouped, listed, grouped, listed):
                fn()
            torch.cuda.synchronize()
            ms = {"groups": [], "pair_list": []}
            for _ in range(a.repeats):
                for name, fn in (("groups", grouped), ("pair_list", listed)):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.launches):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    ms[name].append(e0.elapsed_time(e1) / a.launches)
            same = bool(torch.equal(res_g, res_p))
            equal = equal and same
            med = {name: statistics.median(v) for name, v in ms.items()}
            kernel["64x%d/%s" % (k, kind)] = {"cells": cells, "symbols_per_row": sym.numel() / len(rows), "n_max": n_max,
                                              "groups_ms": ms["groups"], "pair_list_ms": ms["pair_list"],
                                              "pair_list_over_groups": med["pair_list"] / med["groups"], "equal": same}
    out.update(kernel=kernel, equal=equal, launches=a.launches)
    if a.kernel_only or not equal:
        print(json.dumps(out))
        if not equal:
            raise SystemExit("gtos_ngram_overlap_groups and gtos_ngram_overlap disagree")
        return

    # ---- (b), (c) on the decode benchmark's batch
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.vocab import END, PAD
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
    ids = batch_dev['token_out'].cpu()
    truth = []
    for b, local in enumerate(batch_dev['local_idx2token']):
        words = [local[y] if y in local else pv.idx2token(y) for y in ids[:, b].tolist()]
        truth.append([w for w in words if w not in (END, PAD)])
    model.work(batch_dev, a.beam, 3, search="sample", seed=a.seed)                        # warm-up
    decode_s, select_s = [], []
    for rep in range(a.repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.beam, a.max_steps, search="sample", seed=a.seed)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        picks = metrics.mbr_select(beams, a.beam, a.alpha, "uniform", device=dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        if rep:                                                                           # (the first pass warms the selection up)
            decode_s.append(t1 - t0)
            select_s.append(t2 - t1)
    first = [metrics.hypothesis_tokens(best[0]) if best else [] for best in (beam.get_k_best(1, a.alpha) for beam in beams)]
    mbr = [tokens if tokens is not None else h for (tokens, _, _), h in zip(picks, first)]
    upper = metrics.best_of_nbest(beams, truth, a.beam, a.alpha, device=dev)
    sizes = [len(beam.get_k_best(a.beam, a.alpha)) for beam in beams]

    def mean_chrf(hyps):
        s = metrics.sentence_chrf(metrics.overlap(hyps, truth, None, "char", device=dev), metrics.overlap(hyps, truth, None, "chrf_word", device=dev))
        return float(s.mean())
    out.update(select={"workload": "%s eval batch: %d graphs, search=sample, %d samples per graph, max %d decoder steps, %s, random weights" % (
        a.config, stats["B"], a.beam, a.max_steps, a.dtype), "candidates_per_graph": [min(sizes), max(sizes)],
        "decode_seconds": decode_s, "mbr_select_seconds": select_s,
        "select_over_decode": [s / d for s, d in zip(select_s, decode_s)]},
        chrf={"note": "synthetic graphs and random weights: a check of the mechanics, not a quality claim",
              "model_score_choice": mean_chrf(first), "mbr_choice": mean_chrf(mbr),
              "best_of_nbest_choice": mean_chrf([t if t is not None else [] for t, _, _ in upper]),
              "mean_expected_utility_of_the_mbr_choice": statistics.fmean(u for _, i, u in picks if i >= 0) if any(i >= 0 for _, i, _ in picks) else None,
              "mbr_differs_from_model_score_in": sum(1 for x, y in zip(mbr, first) if x != y)})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
