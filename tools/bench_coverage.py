"""Cost and effect of the coverage penalty on the device beam search, on the `bench.py --decode` workload (C2 eval batch: 64 synthetic
100-node AMR graphs, beam 8, 50 steps, bf16, random weights): work(search="device") with coverage_penalty None (the plain search), 0.0
(the same search through gtos_coverage_step / gtos_coverage_advance: the cost of the two extra launches per step alone) and BETA,
interleaved in one process after a warm-up.  Prints one JSON line: per leg sentences/s, ms per decoder step and the steps launched for
every repeat; for the covered legs, over the graphs' best hypotheses (get_k_best(1, alpha)), the mean coverage penalty cp, the share of
the nodes that are not padding with a coverage below 0.5 (concepts the string never looked at) and the mean log-likelihood given up
against the plain search's best hypothesis.

    python tools/bench_coverage.py [--config C2] [--beam 8] [--max-steps 50] [--beta 0.2] [--repeats 3] [--dtype bf16]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ALPHA = 0.6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--beta", type=float, default=0.2)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_coverage.py measures the GPU search: no GPU visible")
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
    real = (~batch['concept'][1:].eq(vocabs['concept'].padding_idx)).t().tolist()            # per graph: which nodes are not padding

    dev_stats = {}
    plain = search.beam_search_device
    G.beam_search_device = lambda model_, memory, beams, **kw: plain(model_, memory, beams, stats=dev_stats, **kw)
    legs = {"plain": None, "beta 0 by the new kernels": 0.0, "beta %g" % a.beta: a.beta}

    def run(leg, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.encode_step(batch_dev, train=False)
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.beam, steps, search="device", coverage_penalty=legs[leg])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        launched = dev_stats["steps"]
        return {"sentences_per_s": B / dt, "ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, launched), "steps": launched,
                "host_reads": dev_stats["host_reads"]}, beams

    for leg in legs:                                      # warm-up: every shape, the search tables, the allocator
        run(leg, 3)
        run(leg, a.max_steps)
    best = lambda beam: beam.get_k_best(1, ALPHA)[0]                      # noqa: E731
    key = lambda beams_: [(b.steps, [(h.seq, h.score) for h in b.hypotheses], [(h.seq, h.score) for h in b.completed_hypotheses]) for b in beams_]   # noqa: E731
    differing = lambda x, y: sum(p != q for p, q in zip(x, y))           # noqa: E731
    names = list(legs)
    runs = {leg: [] for leg in legs}
    last, plain_drift, zero_drift = {}, 0, 0
    for _ in range(a.repeats):
        for leg in legs:
            r, beams = run(leg, a.max_steps)
            if leg == names[0] and leg in last:               # the control: does the plain search repeat itself?
                plain_drift = max(plain_drift, differing(key(beams), last[leg][0]))
            last[leg] = (key(beams), [best(b) for b in beams])
            if legs[leg] is not None:
                tops, base = last[leg][1], last[names[0]][1]
                r["mean_cp"] = sum(h.cp for h in tops) / B
                r["share_nodes_covered_below_half"] = (sum(c < 0.5 for h, keep in zip(tops, real) for c, m in zip(h.coverage, keep) if m)
                                                       / sum(sum(keep) for keep in real))
                r["mean_ll_given_up"] = sum(p.score - h.score for p, h in zip(base, tops)) / B
            runs[leg].append(r)
        zero_drift = max(zero_drift, differing(last[names[0]][0], last[names[1]][0]))
    out = {"metric": "device beam search: plain, through the coverage kernels with beta = 0, and with beta = %g (%s eval batch %d graphs, "
                     "beam %d, %d steps, %s); over the graphs' best hypotheses: mean_cp, share_nodes_covered_below_half (of the nodes "
                     "that are not padding), mean_ll_given_up = plain best score - covered best score" % (
                         a.beta, a.config, B, a.beam, a.max_steps, a.dtype), "repeats": a.repeats}
    for leg, rs in runs.items():
        out[leg] = {k_: [r[k_] for r in rs] for k_ in rs[0]}
    ms = out["plain"]["ms_per_decoder_step"]
    out["plain_ms_per_step_spread"] = (max(ms) - min(ms)) / min(ms)
    median = lambda xs: sorted(xs)[len(xs) // 2]                          # noqa: E731
    for leg in names[1:]:
        out[leg]["median_ms_per_step_over_plain"] = median(out[leg]["ms_per_decoder_step"]) / median(ms)
    # graphs (of B) whose beams differ: between two plain runs (the control), and between the plain run and the covered route with beta = 0
    out["graphs_differing_plain_vs_plain"] = plain_drift
    out["graphs_differing_plain_vs_beta_0"] = zero_drift
    print(json.dumps(out))
    if zero_drift and not plain_drift:
        raise SystemExit("the coverage route with beta = 0 differs from the plain device search, which repeats itself exactly")


if __name__ == "__main__":
    main()
