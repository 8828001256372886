"""Cost and effect of negative constraints (work(..., avoid=)) in the device decoders, on the C1 synthetic eval batch (8 synthetic
20-node AMR graphs, beam / samples 8, 16 steps, fp32, random weights): work(search="device") and work(search="sample", one seed) without
and with an avoid list, interleaved in one process after a warm-up.  The list is built from the plain device search's own best
outputs: each sentence's first bigram and its most frequent token.  Prints one JSON line: per search and leg the ms per decoder step
of every repeat (the comparable figure: avoiding changes how long hypotheses run), the share of sentences whose best output changed,
the mean log-likelihood given up (best plain score minus best avoiding score), and the share of returned hypotheses that hold an
avoided entry -- 0 with the list.

    python tools/bench_avoid.py [--config C1] [--beam 8] [--max-steps 16] [--repeats 3] [--dtype fp32] [--seed 5] [--alpha 0.6]
"""
import argparse
import collections
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def avoid_list(seq):
    """The first bigram and the most frequent token of a best output (token strings, <STR> first)"""
    from gtos_amd.vocab import PAD, UNK, STR, END
    y = [w for w in seq[1:] if w not in (PAD, UNK, STR, END)]
    entries = [y[:2]] if len(y) >= 2 else []
    if y:
        entries.append([collections.Counter(y).most_common(1)[0][0]])
    return entries


def holds(seq, entries):
    return any(seq[i:i + len(p)] == p for p in entries for i in range(len(seq) - len(p) + 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C1")
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=16)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="fp32")
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--alpha", type=float, default=0.6)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_avoid.py measures the GPU decoders: no GPU visible")
    from gtos_amd import synth, search
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    import gtos_amd.generator as G
    dev = torch.device("cuda:0")
    cfg = synth.CONFIGS[a.config]
    vocabs = synth.synth_vocabs()
    torch.manual_seed(19940117)
    model = Generator(vocabs, device=dev, depth_size=256 if cfg["kind"] == "dep" else 32, **generator_args(cfg)).to(dev)
    model.set_compute_dtype(torch.bfloat16 if a.dtype == "bf16" else torch.float32)
    model.eval()
    batch, stats = synth.make_config_batch(a.config, train=False)
    B = stats["B"]
    pv, cp = vocabs['predictable_token'], batch['cp_seq']
    batch_dev = {k: v.to(dev) for k, v in attach_path_trie(batch).items()}
    batch_dev['local_idx2token'] = [{int(i): "copy%d" % int(i) for i in cp[:, b].tolist() if i >= pv.size} for b in range(cp.shape[1])]

    dev_stats = {}
    plain_beam, plain_sample = search.beam_search_device, search.sample_device
    G.beam_search_device = lambda model_, memory, beams, **kw: plain_beam(model_, memory, beams, stats=dev_stats, **kw)
    G.sample_device = lambda model_, memory, beams, *args, **kw: plain_sample(model_, memory, beams, *args, stats=dev_stats, **kw)

    def run(how, avoid, steps, measure=None):
        """One work() call; ``measure``: the avoid list the returned hypotheses are held against (the plain legs too)"""
        kw = dict(search="sample", seed=a.seed) if how == "sample" else dict(search="device")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.encode_step(batch_dev, train=False)
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.beam, steps, avoid=avoid, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        launched = dev_stats["steps"]
        entries = measure or [[] for _ in beams]
        hyps = [(h, e) for b, e in zip(beams, entries) for h in b.completed_hypotheses + b.hypotheses]
        best = [b.get_k_best(1, a.alpha)[0] for b in beams]
        return {"ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, launched), "steps": launched,
                "held_share": sum(holds(h.seq, e) for h, e in hyps) / max(1, len(hyps)), "best": [(h.seq, h.score) for h in best]}

    avoid = [avoid_list(seq) for seq, _ in run("device", None, a.max_steps)["best"]]
    for how in ("device", "sample"):                      # warm-up: every shape, the search tables, the allocator
        for av in (None, avoid):
            run(how, av, 3)
            run(how, av, a.max_steps)
    legs = {(how, leg): [] for how in ("device", "sample") for leg in ("plain", "avoid")}
    for _ in range(a.repeats):
        for how in ("device", "sample"):
            legs[how, "plain"].append(run(how, None, a.max_steps, avoid))
            legs[how, "avoid"].append(run(how, avoid, a.max_steps, avoid))
    out = {"metric": "device beam search and sampling without and with an avoid list (%s eval batch %d graphs, beam %d, %d steps, %s)" % (
        a.config, B, a.beam, a.max_steps, a.dtype), "repeats": a.repeats,
        "avoid_tokens_per_graph": sum(len(p) for e in avoid for p in e) / max(1, B)}
    for how in ("device", "sample"):
        for leg in ("plain", "avoid"):
            runs = legs[how, leg]
            out["%s/%s" % (how, leg)] = {key: [r[key] for r in runs] for key in ("ms_per_decoder_step", "steps", "held_share")}
        p, v = legs[how, "plain"][-1]["best"], legs[how, "avoid"][-1]["best"]
        out["%s/best_changed_share" % how] = sum(x[0] != y[0] for x, y in zip(p, v)) / max(1, B)
        out["%s/mean_ll_given_up" % how] = sum(x[1] - y[1] for x, y in zip(p, v)) / max(1, B)
        worst = max(out["%s/plain" % how]["ms_per_decoder_step"])
        out["%s/ms_per_step_avoid_over_worst_plain" % how] = [x / worst for x in out["%s/avoid" % how]["ms_per_decoder_step"]]
    print(json.dumps(out))
    if any(share for how in ("device", "sample") for share in out["%s/avoid" % how]["held_share"]):
        raise SystemExit("a hypothesis of an avoiding decoder holds an avoided entry")


if __name__ == "__main__":
    main()
