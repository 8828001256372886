"""Cost of teacher-forced scoring and held-out evaluation.  Prints one JSON line:
  * evaluate: Trainer.evaluate (bf16) over a few copies of one synthetic batch of each configuration, in graphs/s and tokens/s, next
    to the forward time of the training step (model(batch) in train mode, autograd graph built) on the same batch;
  * kernel: gtos_copy_eval_fwd alone (ops.copy_eval) next to the alternative built from the ops that existed before it
    (ops.copy_log_likelihood + torch.max + gather of the target) at T*B = 3,200 rows, S = 100, V = 10,000 and 30,000, bf16 logits:
    HIP events around every launch, every shape warmed up, the two alternated, median over --launches launches each.  The new kernel
    reads the same logits and writes 12 bytes per row where the alternative writes and re-reads a 4*C-byte row, so ``not_slower``
    must be true; the script exits with status 1 when it is not.

    python tools/bench_eval.py [--configs C2,C3] [--batches 4] [--reps 5] [--launches 30] [--out profiles/score_eval.json]
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
    tot = max(V, 1 + int(cp.max()))

    def new():
        return ops.copy_eval(lg, dv, al, cp, tg, 0)

    def old():
        ll = ops.copy_log_likelihood(lg, dv, al, cp, tot)
        top, pred = ll.max(-1)
        nll = -ll.gather(-1, tg.unsqueeze(-1)).squeeze(-1)
        return nll, pred, top
    for _ in range(5):
        new()
        old()
    torch.cuda.synchronize()
    times = {"new": [], "old": []}
    for _ in range(launches):
        for name, fn in (("new", new), ("old", old)):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            fn()
            e.record()
            e.synchronize()
            times[name].append(s.elapsed_time(e))
    new_ms, old_ms = statistics.median(times["new"]), statistics.median(times["old"])
    es = lg.element_size()
    return {"rows": T * B, "V": V, "S": S, "copy_eval_ms": new_ms, "ll_max_gather_ms": old_ms, "speedup": old_ms / new_ms,
            "copy_eval_min_ms": min(times["new"]), "ll_max_gather_min_ms": min(times["old"]),
            "copy_eval_logits_GBps": T * B * V * es / (new_ms * 1e-3) / 1e9, "launches_each": launches}


def evaluate_leg(config, n_batches, reps):
    from gtos_amd import synth
    from gtos_amd.config import build_generator
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.relindex import attach_relation_index
    from gtos_amd.train import Trainer
    dev = torch.device("cuda:0")
    model = build_generator(Generator, config, dev).to(dev)
    model.set_compute_dtype(torch.bfloat16)
    model.train()
    trainer = Trainer(model, synth.CONFIGS[config]["d"], warmup_steps=2000, compute_dtype=torch.bfloat16)
    batch, stats = synth.make_config_batch(config)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in attach_relation_index(attach_path_trie(batch)).items()}
    batches = [batch] * n_batches
    tokens = int(batch['token_out'].ne(0).sum()) * n_batches
    for _ in range(2):
        res = trainer.evaluate(batches)
        model(batch)
    ev, fw = [], []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = trainer.evaluate(batches)               # (ends with its one host read)
        torch.cuda.synchronize()
        ev.append((time.perf_counter() - t0) / n_batches)
        t0 = time.perf_counter()
        for _ in range(n_batches):
            loss = model(batch)                       # the training step's forward, autograd graph and all
            del loss
        torch.cuda.synchronize()
        fw.append((time.perf_counter() - t0) / n_batches)
    e, f = statistics.median(ev), statistics.median(fw)
    return {"config": config, "B": stats["B"], "batches": n_batches, "reps": reps, "evaluate_ms_per_batch": e * 1e3,
            "train_forward_ms_per_batch": f * 1e3, "graphs_per_s": stats["B"] / e, "tokens_per_s": tokens / n_batches / e,
            "result": res}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="C2,C3")
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=30, help="timed launches of each alternative per shape (>= 20)")
    ap.add_argument("--out", default=None, help="also write the line to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_eval.py measures GPU kernels: no GPU visible")
    if a.launches < 20:
        raise SystemExit("--launches must be at least 20")
    kernel = [kernel_pair_ms(V, a.launches) for V in (10000, 30000)]
    out = {"evaluate": [evaluate_leg(c, a.batches, a.reps) for c in a.configs.split(",") if c], "kernel": kernel,
           "not_slower": all(k["copy_eval_ms"] <= k["ll_max_gather_ms"] for k in kernel), "dtype": "bf16",
           "device": torch.cuda.get_device_name(0)}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not out["not_slower"]:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
