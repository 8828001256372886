"""Cost and effect of diverse (group) beam search on the device, on the `bench.py --decode` workload (C2 eval batch: 64 synthetic
100-node AMR graphs, beam 8, 50 steps, bf16, random weights): work(search="device") three ways, interleaved in one process after a
warm-up -- plain; groups = 1 forced through gtos_diverse_advance / gtos_diverse_reorder (the same search by the new kernels: their
cost alone); groups = G with diversity = lambda.  Prints one JSON line: per leg sentences/s, ms per decoder step and the steps launched
for every repeat, and the mean number of distinct first-three-token prefixes among a graph's returned hypotheses -- the number the
feature exists to raise.

    python tools/bench_diverse_beam.py [--config C2] [--beam 8] [--max-steps 50] [--groups 4] [--diversity 0.5] [--repeats 3] [--dtype bf16]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def distinct_prefixes(beams, n=3):
    """Mean over the graphs of the number of distinct first-n-token prefixes among the hypotheses (finished and alive) of a beam."""
    counts = [len({tuple(h.seq[1:1 + n]) for h in b.completed_hypotheses + b.hypotheses}) for b in beams]
    return sum(counts) / max(1, len(counts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--groups", type=int, default=4)
    ap.add_argument("--diversity", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_diverse_beam.py measures the GPU search: no GPU visible")
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

    dev_stats, route = {}, {}
    plain = search.beam_search_device
    G.beam_search_device = lambda model_, memory, beams, **kw: plain(model_, memory, beams, stats=dev_stats, **dict(kw, **route))
    legs = {"plain": (dict(), dict()), "groups=1 by the new kernels": (dict(), dict(grouped=True)),
            "groups=%d diversity=%g" % (a.groups, a.diversity): (dict(groups=a.groups, diversity=a.diversity), dict())}

    def run(leg, steps):
        kw, forced = legs[leg]
        route.clear()
        route.update(forced)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.encode_step(batch_dev, train=False)
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.beam, steps, search="device", **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        launched = dev_stats["steps"]
        return {"sentences_per_s": B / dt, "ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, launched), "steps": launched,
                "distinct_prefixes": distinct_prefixes(beams)}, beams

    for leg in legs:                                      # warm-up: every shape, the search tables, the allocator
        run(leg, 3)
        run(leg, a.max_steps)
    runs = {leg: [] for leg in legs}
    key = lambda beams: [(b.steps, [(h.seq, h.score) for h in b.hypotheses], [(h.seq, h.score) for h in b.completed_hypotheses]) for b in beams]
    differing = lambda x, y: sum(p != q for p, q in zip(x, y))
    names = list(legs)
    last, plain_drift, forced_drift = {}, 0, 0
    for _ in range(a.repeats):
        for leg in legs:
            r, beams = run(leg, a.max_steps)
            runs[leg].append(r)
            if leg == names[0] and leg in last:               # the control: does the plain search repeat itself (bf16 kernels that accumulate with atomics need not)?
                plain_drift = max(plain_drift, differing(key(beams), last[leg]))
            last[leg] = key(beams)
        forced_drift = max(forced_drift, differing(last[names[0]], last[names[1]]))
    out = {"metric": "device beam search: plain, one group by the diverse kernels, and %d groups with diversity %g (%s eval batch %d "
                     "graphs, beam %d, %d steps, %s); distinct_prefixes: mean distinct first-3-token prefixes per graph" % (
                         a.groups, a.diversity, a.config, B, a.beam, a.max_steps, a.dtype), "repeats": a.repeats}
    for leg, rs in runs.items():
        out[leg] = {k_: [r[k_] for r in rs] for k_ in ("sentences_per_s", "ms_per_decoder_step", "steps", "distinct_prefixes")}
    worst = max(out["plain"]["ms_per_decoder_step"])
    for leg in names[1:]:
        out[leg]["ms_per_step_over_worst_plain"] = [x / worst for x in out[leg]["ms_per_decoder_step"]]
    # graphs (of B) whose beams differ: between two plain runs (the control), and between the plain run and one group by the new kernels
    out["graphs_differing_plain_vs_plain"] = plain_drift
    out["graphs_differing_plain_vs_one_group"] = forced_drift
    print(json.dumps(out))
    if forced_drift and not plain_drift:
        raise SystemExit("one group through the diverse kernels differs from the plain device search, which repeats itself exactly")


if __name__ == "__main__":
    main()
