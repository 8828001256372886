"""Cost of repeat-n-gram blocking in the device beam search, on the `bench.py --decode` workload (C2 eval batch: 64 synthetic
100-node AMR graphs, beam 8, 50 steps, bf16, random weights): work(search="device") with no_repeat_ngram = 0 and = n, interleaved in
one process after a warm-up.  Prints one JSON line: per leg sentences/s and ms per decoder step (the comparable figure: blocking
changes how long hypotheses run) for every repeat, and the share of returned hypotheses that hold a repeated n-gram -- 0 with blocking.

    python tools/bench_ngram_block.py [--config C2] [--beam 8] [--max-steps 50] [--ngram 3] [--repeats 3] [--dtype bf16]
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def repeat_share(beams, n):
    """Share of the hypotheses (finished and alive) of ``beams`` whose tokens hold some n-gram twice."""
    from gtos_amd.vocab import END
    hyps = [h for b in beams for h in b.completed_hypotheses + b.hypotheses]
    bad = 0
    for h in hyps:
        y = [w for w in h.seq[1:] if w != END]
        grams = [tuple(y[i:i + n]) for i in range(len(y) - n + 1)]
        bad += len(grams) != len(set(grams))
    return bad / max(1, len(hyps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--beam", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--ngram", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ngram_block.py measures the GPU search: no GPU visible")
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
    plain = search.beam_search_device
    G.beam_search_device = lambda model_, memory, beams, **kw: plain(model_, memory, beams, stats=dev_stats, **kw)

    def run(n, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.encode_step(batch_dev, train=False)
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.beam, steps, search="device", no_repeat_ngram=n)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        launched = dev_stats["steps"]
        return {"sentences_per_s": B / dt, "ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, launched), "steps": launched,
                "repeat_share": repeat_share(beams, a.ngram)}

    for n in (0, a.ngram):                                # warm-up: every shape, the search tables, the allocator
        run(n, 3)
        run(n, a.max_steps)
    legs = {0: [], a.ngram: []}
    for _ in range(a.repeats):
        for n in (0, a.ngram):
            legs[n].append(run(n, a.max_steps))
    out = {"metric": "device beam search with and without repeat-%d-gram blocking (%s eval batch %d graphs, beam %d, %d steps, %s)" % (
        a.ngram, a.config, B, a.beam, a.max_steps, a.dtype), "repeats": a.repeats}
    for n, runs in legs.items():
        out["n=%d" % n] = {key: [r[key] for r in runs] for key in ("sentences_per_s", "ms_per_decoder_step", "steps", "repeat_share")}
    worst0 = max(out["n=0"]["ms_per_decoder_step"])
    out["ms_per_step_blocked_over_worst_plain"] = [x / worst0 for x in out["n=%d" % a.ngram]["ms_per_decoder_step"]]
    print(json.dumps(out))
    if any(out["n=%d" % a.ngram]["repeat_share"]):
        raise SystemExit("a hypothesis of the blocked search repeats an n-gram")


if __name__ == "__main__":
    main()
