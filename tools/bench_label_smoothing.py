"""Cost of label smoothing (TokenGenerator.label_smoothing) on the training step.  Prints one JSON line:
  * step: the median step time and graphs/s of C2 bf16 Trainer steps with eps = 0 and eps = 0.1, one model and trainer in one
    process, the two settings in alternating blocks (set_label_smoothing between blocks) after a warm-up of both;
  * loss_op: the copy-loss forward + backward alone at the C2 decoder shape (T=50, B=64, V=10000, S=100, bf16 logits), from HIP
    events: gtos_copy_nll_fwd/bwd (eps = 0) against gtos_copy_nll_ls_prep/fwd/bwd (eps = 0.1).

    python tools/bench_label_smoothing.py [--config C2] [--eps 0.1] [--steps 10] [--blocks 6] [--warmup 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def loss_op_ms(eps, iters=50, T=50, B=64, V=10000, S=100):
    from gtos_amd import ops
    g = torch.Generator(device="cuda").manual_seed(5)
    dev = torch.device("cuda")
    lg = torch.randn(T, B, V, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    dv = torch.randn(T, B, 2, device=dev, generator=g).to(torch.bfloat16).requires_grad_(True)
    al = torch.softmax(torch.randn(T, B, S, device=dev, generator=g), -1).requires_grad_(True)
    cp = torch.randint(1, V + 40, (S, B), device=dev, generator=g)
    tg = torch.randint(1, V, (T, B), device=dev, generator=g)
    up = torch.ones(T, B, device=dev)

    def once():
        out = ops.copy_nll(lg, dv, al, cp, tg, 0, label_smoothing=eps)
        torch.autograd.grad(out, (lg, dv, al), grad_outputs=up)
    for _ in range(5):
        once()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    s.record()
    for _ in range(iters):
        once()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--eps", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=10, help="steps per block")
    ap.add_argument("--blocks", type=int, default=6, help="blocks per setting")
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_label_smoothing.py measures GPU training steps: no GPU visible")
    from gtos_amd import synth
    from gtos_amd.config import build_generator
    from gtos_amd.decoder import set_label_smoothing
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.relindex import attach_relation_index
    from gtos_amd.train import Trainer
    dev = torch.device("cuda:0")
    model = build_generator(Generator, a.config, dev).to(dev)
    model.set_compute_dtype(torch.bfloat16)
    model.train()
    trainer = Trainer(model, synth.CONFIGS[a.config]["d"], warmup_steps=2000, compute_dtype=torch.bfloat16)
    batch, stats = synth.make_config_batch(a.config)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in attach_relation_index(attach_path_trie(batch)).items()}
    B = stats["B"]
    settings = (0.0, a.eps)
    for eps in settings:
        set_label_smoothing(model, eps)
        for _ in range(a.warmup):
            trainer.step(batch)
    times = {eps: [] for eps in settings}
    losses = {eps: None for eps in settings}
    for _ in range(a.blocks):
        for eps in settings:
            set_label_smoothing(model, eps)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                losses[eps] = trainer.step(batch)
            torch.cuda.synchronize()
            times[eps].append((time.perf_counter() - t0) / a.steps)
    med = {eps: statistics.median(v) for eps, v in times.items()}
    op = {"plain_ms": loss_op_ms(0.0), "smoothed_ms": loss_op_ms(a.eps)}
    out = {
        "config": a.config, "dtype": "bf16", "B": B, "eps": a.eps, "steps_per_block": a.steps, "blocks": a.blocks,
        "step_ms": {"eps0": med[0.0] * 1e3, "eps": med[a.eps] * 1e3},
        "graphs_per_s": {"eps0": B / med[0.0], "eps": B / med[a.eps]},
        "ratio_eps_over_eps0": med[a.eps] / med[0.0],
        "block_step_ms": {"eps0": [t * 1e3 for t in times[0.0]], "eps": [t * 1e3 for t in times[a.eps]]},
        "last_loss": {"eps0": losses[0.0], "eps": losses[a.eps]},
        "loss_op_c2_fwd_bwd_ms": op,
        "device": torch.cuda.get_device_name(0),
    }
    print(json.dumps(out))


if __name__ == "__main__":
    main()
