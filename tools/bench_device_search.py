"""Host vs device beam search on the `bench.py --decode` workload (C2 eval batch: 64 synthetic 100-node AMR graphs, beam 8, 50 steps,
bf16, random weights), both in one process, alternating after a warm-up.  Prints one JSON line: per search path the median
sentences/s, ms per decoder step and host reads per search, plus the spread over the repeats.

Host reads: the host path makes one .tolist() per decoder step (the top-k results) plus the read of tot_ext in Generator.work; the
device path reads tot_ext, the continue flag every `sync_every` steps, and its two final tables (beam_search_device's stats).

    python tools/bench_device_search.py [--config C2] [--beam 8] [--max-steps 50] [--repeats 5] [--dtype bf16]
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
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sync-every", type=int, default=8)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_device_search.py measures the GPU search paths: no GPU visible")
    from gtos_amd import synth, search
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
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
    plain = search.beam_search_device

    def counted(model_, memory, beams, sync_every=a.sync_every):
        return plain(model_, memory, beams, sync_every=sync_every, stats=dev_stats)
    import gtos_amd.generator as G
    G.beam_search_device = counted

    def run(path, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.encode_step(batch_dev, train=False)
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.beam, steps, search=path)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = max(b.steps for b in beams)
        launched = dev_stats["steps"] if path == "device" else n
        reads = 1 + (dev_stats["host_reads"] if path == "device" else n)
        return {"seconds": dt, "sentences_per_s": B / dt, "decoder_steps": n, "steps_launched": launched,
                "ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, n), "host_reads": reads}

    for path in ("host", "device"):                       # warm-up: every shape, the search tables, the allocator
        run(path, 3)
        run(path, a.max_steps)
    legs = {"host": [], "device": []}
    for _ in range(a.repeats):
        for path in ("host", "device"):
            legs[path].append(run(path, a.max_steps))
    out = {"metric": "beam search, host vs device selection (%s eval batch %d graphs, beam %d, %d steps, %s)" % (
        a.config, B, a.beam, a.max_steps, a.dtype), "repeats": a.repeats, "sync_every": a.sync_every}
    for path, runs in legs.items():
        med = lambda key: statistics.median(r[key] for r in runs)
        out[path] = {"sentences_per_s": med("sentences_per_s"), "ms_per_decoder_step": med("ms_per_decoder_step"),
                     "seconds": med("seconds"), "decoder_steps": runs[-1]["decoder_steps"], "steps_launched": runs[-1]["steps_launched"],
                     "host_reads_per_search": runs[-1]["host_reads"],
                     "sentences_per_s_range": [min(r["sentences_per_s"] for r in runs), max(r["sentences_per_s"] for r in runs)]}
    out["device_over_host"] = out["device"]["sentences_per_s"] / out["host"]["sentences_per_s"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
