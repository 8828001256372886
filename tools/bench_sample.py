"""Sampling vs device beam search on the `bench.py --decode` workload (C2 eval batch: 64 synthetic 100-node AMR graphs, 8 samples or
beams, 50 steps, bf16, random weights), both in one process, alternating after a warm-up.  Prints one JSON line: per path the median
sentences/s, ms per decoder step and host reads per search, plus the spread over the repeats.

search="sample" (gtos_amd.search.sample_device) keeps one cache per layer and reorders nothing; search="device"
(beam_search_device) gathers the caches by parent slot every step.  Host reads: tot_ext in Generator.work, the continue flag every
`sync_every` steps and the final tables (the search's stats).

    python tools/bench_sample.py [--config C2] [--samples 8] [--max-steps 50] [--repeats 5] [--dtype bf16]
                                 [--temperature 1.0] [--top-k 0] [--top-p 1.0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sync-every", type=int, default=8)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--temperature", type=float, default=1.0)
    ap.add_argument("--top-k", type=int, default=0)
    ap.add_argument("--top-p", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sample.py measures the GPU decode paths: no GPU visible")
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

    path_stats = {}
    beam_plain, sample_plain = search.beam_search_device, search.sample_device

    def beam_counted(model_, memory, beams, sync_every=a.sync_every):
        return beam_plain(model_, memory, beams, sync_every=sync_every, stats=path_stats)

    def sample_counted(model_, memory, beams, temperature, top_k, top_p, seed, sync_every=a.sync_every):
        return sample_plain(model_, memory, beams, temperature, top_k, top_p, seed, sync_every=sync_every, stats=path_stats)
    G.beam_search_device, G.sample_device = beam_counted, sample_counted
    kw = {"sample": dict(temperature=a.temperature, top_k=a.top_k, top_p=a.top_p, seed=20261016), "device": {}}

    def run(path, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.encode_step(batch_dev, train=False)
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.samples, steps, search=path, **kw[path])
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = max(b.steps for b in beams)
        return {"seconds": dt, "sentences_per_s": B / dt, "decoder_steps": n, "steps_launched": path_stats["steps"],
                "ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, n), "host_reads": 1 + path_stats["host_reads"]}

    for path in ("device", "sample"):                     # warm-up: every shape, the search tables, the allocator
        run(path, 3)
        run(path, a.max_steps)
    legs = {"device": [], "sample": []}
    for _ in range(a.repeats):
        for path in ("device", "sample"):
            legs[path].append(run(path, a.max_steps))
    out = {"metric": "sampling vs device beam search (%s eval batch %d graphs, %d samples / beams, %d steps, %s)" % (
        a.config, B, a.samples, a.max_steps, a.dtype), "repeats": a.repeats, "sync_every": a.sync_every,
        "sampling": {"temperature": a.temperature, "top_k": a.top_k, "top_p": a.top_p}}
    for path, runs in legs.items():
        med = lambda key: statistics.median(r[key] for r in runs)
        out[path] = {"sentences_per_s": med("sentences_per_s"), "ms_per_decoder_step": med("ms_per_decoder_step"),
                     "seconds": med("seconds"), "decoder_steps": runs[-1]["decoder_steps"], "steps_launched": runs[-1]["steps_launched"],
                     "host_reads_per_search": runs[-1]["host_reads"],
                     "sentences_per_s_range": [min(r["sentences_per_s"] for r in runs), max(r["sentences_per_s"] for r in runs)]}
    out["sample_over_device"] = out["sample"]["sentences_per_s"] / out["device"]["sentences_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
