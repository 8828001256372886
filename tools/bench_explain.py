"""Cost of token-level attribution.  Prints one JSON line:
  * model: Generator.explain next to Generator.score (bf16) on the own sentences of one synthetic batch of the configuration, wall
    time per call after warm-up, median of --reps;
  * kernel: gtos_copy_explain_fwd alone (ops.copy_explain) next to gtos_copy_eval_fwd (ops.copy_eval) on the same rows, T*B = 3,200,
    S = 100, V = 10,000 and 30,000, bf16 logits: HIP events around every launch, every shape warmed up, the two alternated, median over
    --launches launches each.  ``ratio`` = explain / eval; explain makes three passes over the logits where eval makes two;
  * summary of the model leg's result: the share of tokens with copy_share > 0.5, the mean entropy (nats) and the share with rank 0.
There is no bar on the times.

    python tools/bench_explain.py [--config C2] [--reps 5] [--launches 30] [--out profiles/explain.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def kernel_pair_ms(V, launches, T=50, B=64, S=100):
    from gtos_amd import ops
    dev = torch.device("cuda")
    g = torch.Generator(device="cuda").manual_seed(5)
    lg = (torch.randn(T, B, V, device=dev, generator=g) * 4).to(torch.bfloat16)
    dv = torch.randn(T, B, 2, device=dev, generator=g).to(torch.bfloat16)
    al = torch.softmax(torch.randn(T, B, S, device=dev, generator=g), -1)
    cp = torch.randint(1, V + 40, (S, B), device=dev, generator=g)
    tg = torch.randint(1, V, (T, B), device=dev, generator=g)
    ev_out = ops.copy_eval(lg, dv, al, cp, tg, 0)
    ex_out = ops.copy_explain(lg, dv, al, cp, tg, 0)

    def explain():
        return ops.copy_explain(lg, dv, al, cp, tg, 0, out=ex_out)

    def evaluate():
        return ops.copy_eval(lg, dv, al, cp, tg, 0, out=ev_out)
    for _ in range(5):
        explain()
        evaluate()
    torch.cuda.synchronize()
    times = {"explain": [], "eval": []}
    for _ in range(launches):
        for name, fn in (("explain", explain), ("eval", evaluate)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e))
    ex_ms, ev_ms = statistics.median(times["explain"]), statistics.median(times["eval"])
    return {"rows": T * B, "V": V, "S": S, "copy_explain_ms": ex_ms, "copy_eval_ms": ev_ms, "ratio": ex_ms / ev_ms,
            "copy_explain_min_ms": min(times["explain"]), "copy_eval_min_ms": min(times["eval"]), "logits_passes": [3, 2],
            "copy_explain_logits_GBps": T * B * V * lg.element_size() / (ex_ms * 1e-3) / 1e9, "launches_each": launches}


def model_leg(config, reps):
    from gtos_amd import synth
    from gtos_amd.config import build_generator
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.relindex import attach_relation_index
    dev = torch.device("cuda:0")
    model = build_generator(Generator, config, dev).to(dev)
    model.set_compute_dtype(torch.bfloat16)
    model.eval()
    batch, stats = synth.make_config_batch(config)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in attach_relation_index(attach_path_trie(batch)).items()}
    for _ in range(2):
        ex = model.explain(batch)
        model.score(batch)
    times = {"explain": [], "score": []}
    for _ in range(reps):
        for name, fn in (("explain", model.explain), ("score", model.score)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(batch)
            torch.cuda.synchronize()
            times[name].append(time.perf_counter() - t0)
    e, s = statistics.median(times["explain"]), statistics.median(times["score"])
    live = batch['token_out'].ne(0)
    n = int(live.sum())
    summary = {"tokens": n, "copied_share": float((ex.copy_share[live] > 0.5).sum()) / n,
               "mean_entropy": float(ex.entropy[live].double().mean()), "rank0_share": float((ex.rank[live] == 0).sum()) / n}
    return {"config": config, "B": stats["B"], "reps": reps, "explain_ms": e * 1e3, "score_ms": s * 1e3, "ratio": e / s}, summary


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=30, help="timed launches of each kernel per shape (>= 20)")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_explain.py measures GPU kernels: no GPU visible")
    if a.launches < 20:
        raise SystemExit("--launches must be at least 20")
    kernel = [kernel_pair_ms(V, a.launches) for V in (10000, 30000)]
    model, summary = model_leg(a.config, a.reps)
    line = json.dumps({"model": model, "kernel": kernel, "summary": summary, "dtype": "bf16", "device": torch.cuda.get_device_name(0)})
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
