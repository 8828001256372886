"""Cost and effect of the distribution-shaped cuts of the sampling decode (work(search="sample", min_p=, typical_p=, ...)) on the
`bench.py --decode` workload (C2 eval batch: 64 synthetic 100-node AMR graphs, 8 samples, 50 steps, bf16, random weights):
search="sample" without a cut, with typical_p = 0.9 and with min_p = 0.05, interleaved in one process after a warm-up.  Prints one JSON
line: per leg the ms per decoder step of every repeat and their median; per cut the mean share of a live row's allowed columns that
gtos_truncate_block keeps (one extra, untimed run that counts them around every launch); and the time of one gtos_truncate_block launch
per cut next to one gtos_sample_step launch on the same ll rows, those of decoder step 0 with every slot live (HIP events around a run
of launches, the copy that restores the rows taken off).  The weights are random, so the model's distribution is close to flat: a
trained model's rows are peaked and keep a smaller share.

    python tools/bench_truncate.py [--config C2] [--samples 8] [--max-steps 50] [--repeats 5] [--dtype bf16] [--temperature 1.0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LEGS = (("plain", {}), ("typical_p=0.9", dict(typical_p=0.9)), ("min_p=0.05", dict(min_p=0.05)))


def allowed_columns(ll, t, k, V, tot, min_t, flag_shared, flag_local, owned):
    """Rule 1 of csrc/sample_kernels.h for every row of ll [N, tot], as a bool tensor"""
    N = ll.shape[0]
    B = N // k
    cls = flag_shared[:V].view(1, V).expand(B, V)
    own = torch.ones((B, V), dtype=torch.bool, device=ll.device)
    if tot > V:
        cls = torch.cat([cls, flag_local.view(B, tot - V)], 1)
        own = torch.cat([own, owned.view(B, tot - V).bool()], 1)
    ok = own & ((cls == 0) | ((cls == 2) & (t >= min_t)))
    return torch.isfinite(ll) & ok.repeat_interleave(k, 0)


def kernel_times(model, memory, k, temperature, launches=50):
    """us per launch of gtos_truncate_block (per cut) and gtos_sample_step on the ll rows of decoder step 0 with every slot live"""
    from gtos_amd import ops, search
    dev = memory['probe'].device
    B = len(memory['local_idx2token'])
    N = B * k
    V = model.vocabs['predictable_token'].size
    tot = max(int(memory['tot_ext']), V)
    tab = model.search_tables(memory['local_idx2token'], tot)
    owned = model.sample_tables(memory['local_idx2token'], tot)
    caches = [c[0] for c in model.slot_caches(2, N, copies=1)]
    tok = torch.full((1, N), tab['start_tok'], dtype=torch.int64, device=dev)
    chars = tab['start_char'].expand(1, N, tab['C']).contiguous()
    ll0 = model.decode_slots((tok, chars), caches, search.slot_memory(memory, B, k), 0)
    ll = ll0.clone()
    state = torch.zeros((N, 3), dtype=torch.int32, device=dev)
    tokens = torch.full((2, N), -1, dtype=torch.int32, device=dev)
    score = torch.zeros(N, dtype=torch.float64, device=dev)
    active = torch.ones(3, dtype=torch.int32, device=dev)
    tok_out, char_out = torch.empty(N, dtype=torch.int64, device=dev), torch.empty((N, tab['C']), dtype=torch.int64, device=dev)

    def resets():                                           # what the launches below put in front of theirs, alone
        ll.copy_(ll0)
        state.zero_()
        active.fill_(1)

    def truncate(**cut):
        full = dict(dict(min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0), **cut)

        def fn():
            resets()
            ops.truncate_block(0, k, V, tot, 0, temperature, full['min_p'], full['typical_p'], full['epsilon_cutoff'], full['eta_cutoff'],
                               ll, tab['flag_shared'], tab['flag_local'], owned, state, active)
        return fn

    def sample_step():
        resets()
        ops.sample_step(0, k, V, tot, 0, 2, temperature, 0, 1.0, 7, ll, tab['flag_shared'], tab['flag_local'], owned, score, state,
                        tokens, active, tab['tok_shared'], tab['tok_local'], tab['char_shared'], tab['char_local'], tab['dead_tok'],
                        tab['dead_char'], tok_out, char_out)
    fns = [("resets", resets), ("gtos_sample_step", sample_step)]
    fns += [("gtos_truncate_block/" + name, truncate(**cut)) for name, cut in LEGS if cut]
    out = {}
    for name, fn in fns:
        for _ in range(5):
            fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            fn()
        end.record()
        torch.cuda.synchronize()
        out[name] = 1e3 * start.elapsed_time(end) / launches
    for name in list(out):
        if name != "resets":
            out[name] = max(0.0, out[name] - out["resets"])
    del out["resets"]
    out["rows"], out["columns"] = N, tot
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sync-every", type=int, default=8)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--temperature", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_truncate.py measures the GPU sampling decode: no GPU visible")
    from gtos_amd import ops, synth, search
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

    path_stats, box = {}, {}
    sample_plain = search.sample_device

    def sample_counted(model_, memory, beams, *args, **kw):
        box["memory"] = memory
        return sample_plain(model_, memory, beams, *args, sync_every=a.sync_every, stats=path_stats, **kw)
    G.sample_device = sample_counted

    def run(cut, steps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.encode_step(batch_dev, train=False)
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.samples, steps, search="sample", temperature=a.temperature, seed=20261020, **cut)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = max(b.steps for b in beams)
        return {"ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, n), "decoder_steps": n, "steps_launched": path_stats["steps"]}

    for _, cut in LEGS:                                     # warm-up: every shape, the search tables, the allocator
        run(cut, 3)
        run(cut, a.max_steps)
    legs = {name: [] for name, _ in LEGS}
    for _ in range(a.repeats):
        for name, cut in LEGS:
            legs[name].append(run(cut, a.max_steps))
    out = {"metric": "sampling decode without and with a distribution-shaped cut (%s eval batch %d graphs, %d samples, %d steps, %s)" % (
        a.config, B, a.samples, a.max_steps, a.dtype), "repeats": a.repeats, "sync_every": a.sync_every, "temperature": a.temperature}
    for name, runs in legs.items():
        ms = [r["ms_per_decoder_step"] for r in runs]
        out[name] = {"ms_per_decoder_step": ms, "ms_per_decoder_step_median": statistics.median(ms),
                     "decoder_steps": runs[-1]["decoder_steps"], "steps_launched": runs[-1]["steps_launched"]}
    worst = max(out["plain"]["ms_per_decoder_step"])
    for name, cut in LEGS:
        if cut:
            out[name]["ms_per_step_over_worst_plain"] = [x / worst for x in out[name]["ms_per_decoder_step"]]
    # the share of a live row's allowed columns that survives, counted around every launch of one more run per cut
    plain_truncate = ops.truncate_block
    counts = []

    def truncate_counted(t, k, V, tot, min_t, temperature, min_p, typical_p, eps, eta, ll, flag_shared, flag_local, owned, state, active):
        live = (state[:, 2] == 0) & (active[t % 3] != 0)
        before = allowed_columns(ll, t, k, V, tot, min_t, flag_shared, flag_local, owned).sum(1)
        plain_truncate(t, k, V, tot, min_t, temperature, min_p, typical_p, eps, eta, ll, flag_shared, flag_local, owned, state, active)
        after = allowed_columns(ll, t, k, V, tot, min_t, flag_shared, flag_local, owned).sum(1)
        rows = live & (before > 0)
        counts.append((after[rows].double() / before[rows].double()).sum().item())
        counts.append(float(rows.sum().item()))
    ops.truncate_block = truncate_counted
    try:
        for name, cut in LEGS:
            if cut:
                del counts[:]
                run(cut, a.max_steps)
                out[name]["mean_share_of_allowed_columns_kept"] = sum(counts[0::2]) / max(1.0, sum(counts[1::2]))
                out[name]["rows_counted"] = int(sum(counts[1::2]))
    finally:
        ops.truncate_block = plain_truncate
    with torch.no_grad():
        out["kernel_us"] = kernel_times(model, box["memory"], a.samples, a.temperature)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
