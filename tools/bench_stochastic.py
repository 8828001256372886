"""Stochastic beam search vs sampling vs device beam search on the `bench.py --decode` workload (C2 eval batch: 64 synthetic 100-node
AMR graphs, 8 slots, 50 steps, bf16, random weights), all in one process, alternating after a warm-up.  Prints one JSON line: per path
the median sentences/s, ms per decoder step and host reads per search with the spread over the repeats; the distinct sequences per
graph of search="stochastic" and search="sample" at temperatures 1.0 and 0.7; and the time of one gtos_sbs_step / gtos_sbs_advance
launch next to one gtos_sample_step launch on the same ll rows (HIP events around a run of launches).

search="stochastic" (gtos_amd.search.stochastic_beam_search_device) and search="device" (beam_search_device) both gather the caches
by parent slot every step: that is the like-for-like pair.  search="sample" keeps one cache per layer and reorders nothing.  The
weights are random, so the model's distribution is close to flat and independent samples rarely coincide; the distinct-sequence count
of a trained model at these temperatures is what the without-replacement draw is for.

    python tools/bench_stochastic.py [--config C2] [--slots 8] [--max-steps 50] [--repeats 5] [--dtype bf16] [--temperature 1.0]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def distinct_per_graph(beams):
    """mean over the graphs of the number of different sequences among a graph's hypotheses"""
    return statistics.mean(len(set(tuple(h.seq) for h in list(b.completed_hypotheses) + list(b.hypotheses))) for b in beams)


def kernel_times(model, memory, k, temperature, launches=50):
    """us per launch of gtos_sbs_step, gtos_sbs_advance and gtos_sample_step on the ll rows of decoder step 0 with every slot live"""
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
    ll = model.decode_slots((tok, chars), caches, search.slot_memory(memory, B, k), 0)
    ints = lambda *shape, fill=0: torch.full(shape, fill, dtype=torch.int32, device=dev)            # noqa: E731
    dbls = lambda *shape: torch.zeros(shape, dtype=torch.float64, device=dev)                        # noqa: E731
    state0 = torch.tensor([0, 0, k, 0], dtype=torch.int32, device=dev).repeat(B, 1)                  # every slot live
    state = state0.clone()
    active = torch.ones(3, dtype=torch.int32, device=dev)
    cand = [ints(N, k, fill=-1), torch.zeros((N, k), dtype=torch.float32, device=dev), dbls(N, k), dbls(N, k)]
    slot = [dbls(N), dbls(N), dbls(N)]
    bp, comp_i, comp_d = [ints(2, N, fill=-1) for _ in range(2)], [ints(B, k) for _ in range(2)], [dbls(B, k) for _ in range(3)]
    s_state, s_tokens, s_score = ints(N, 3), ints(2, N, fill=-1), dbls(N)
    tok_out, char_out = torch.empty(N, dtype=torch.int64, device=dev), torch.empty((N, tab['C']), dtype=torch.int64, device=dev)

    def sbs_step():
        ops.sbs_step(0, k, V, tot, 0, 2, temperature, 7, ll, tab['flag_shared'], tab['flag_local'], owned, slot[1], slot[2], state, active, *cand)

    def sbs_advance():
        state.copy_(state0)
        active.fill_(1)
        ops.sbs_advance(0, k, V, tot, 0, 2, *cand, tab['flag_shared'], tab['flag_local'], *slot, state, *bp, *comp_i, *comp_d, active)

    def sample_step():
        s_state.zero_()
        active.fill_(1)
        ops.sample_step(0, k, V, tot, 0, 2, temperature, 0, 1.0, 7, ll, tab['flag_shared'], tab['flag_local'], owned, s_score, s_state,
                        s_tokens, active, tab['tok_shared'], tab['tok_local'], tab['char_shared'], tab['char_local'], tab['dead_tok'],
                        tab['dead_char'], tok_out, char_out)

    def resets():                                           # what sbs_advance / sample_step put in front of their launch, alone
        s_state.zero_()
        active.fill_(1)
    out = {}
    for name, fn in (("resets", resets), ("gtos_sbs_step", sbs_step), ("gtos_sample_step", sample_step), ("gtos_sbs_advance", sbs_advance)):
        for _ in range(5):
            fn()
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(launches):
            fn()
        end.record()
        torch.cuda.synchronize()
        out[name] = 1e3 * start.elapsed_time(end) / launches
    for name in ("gtos_sample_step", "gtos_sbs_advance"):   # their state resets are not theirs
        out[name] = max(0.0, out[name] - out["resets"])
    del out["resets"]
    out["rows"], out["columns"] = N, tot
    out["sbs_step_over_sample_step"] = out["gtos_sbs_step"] / out["gtos_sample_step"] if out["gtos_sample_step"] else None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="C2")
    ap.add_argument("--slots", type=int, default=8)
    ap.add_argument("--max-steps", type=int, default=50)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--sync-every", type=int, default=8)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    ap.add_argument("--temperature", type=float, default=1.0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_stochastic.py measures the GPU decode paths: no GPU visible")
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

    path_stats, box = {}, {}
    beam_plain, sample_plain, stochastic_plain = search.beam_search_device, search.sample_device, search.stochastic_beam_search_device

    def beam_counted(model_, memory, beams, sync_every=a.sync_every):
        return beam_plain(model_, memory, beams, sync_every=sync_every, stats=path_stats)

    def sample_counted(model_, memory, beams, temperature, top_k, top_p, seed, sync_every=a.sync_every):
        return sample_plain(model_, memory, beams, temperature, top_k, top_p, seed, sync_every=sync_every, stats=path_stats)

    def stochastic_counted(model_, memory, beams, temperature, seed, sync_every=a.sync_every):
        box["memory"] = memory
        return stochastic_plain(model_, memory, beams, temperature, seed, sync_every=sync_every, stats=path_stats)
    G.beam_search_device, G.sample_device, G.stochastic_beam_search_device = beam_counted, sample_counted, stochastic_counted
    draw = dict(temperature=a.temperature, seed=20261020)
    kw = {"stochastic": draw, "sample": draw, "device": {}}
    paths = ("stochastic", "sample", "device")

    def run(path, steps, **over):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.no_grad():
            model.encode_step(batch_dev, train=False)
        torch.cuda.synchronize()
        t_enc = time.perf_counter() - t0
        t0 = time.perf_counter()
        beams = model.work(batch_dev, a.slots, steps, search=path, **dict(kw[path], **over))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        n = max(b.steps for b in beams)
        return {"seconds": dt, "sentences_per_s": B / dt, "decoder_steps": n, "steps_launched": path_stats["steps"],
                "ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, n), "host_reads": 1 + path_stats["host_reads"],
                "distinct": distinct_per_graph(beams)}

    for path in paths:                                      # warm-up: every shape, the search tables, the allocator
        run(path, 3)
        run(path, a.max_steps)
    legs = {path: [] for path in paths}
    for _ in range(a.repeats):
        for path in paths:
            legs[path].append(run(path, a.max_steps))
    out = {"metric": "stochastic beam search vs sampling vs device beam search (%s eval batch %d graphs, %d slots, %d steps, %s)" % (
        a.config, B, a.slots, a.max_steps, a.dtype), "repeats": a.repeats, "sync_every": a.sync_every, "temperature": a.temperature}
    for path, runs in legs.items():
        med = lambda key: statistics.median(r[key] for r in runs)           # noqa: E731
        out[path] = {"sentences_per_s": med("sentences_per_s"), "ms_per_decoder_step": med("ms_per_decoder_step"),
                     "seconds": med("seconds"), "decoder_steps": runs[-1]["decoder_steps"], "steps_launched": runs[-1]["steps_launched"],
                     "host_reads_per_search": runs[-1]["host_reads"],
                     "sentences_per_s_range": [min(r["sentences_per_s"] for r in runs), max(r["sentences_per_s"] for r in runs)]}
    out["stochastic_over_device_ms_per_step"] = out["stochastic"]["ms_per_decoder_step"] / out["device"]["ms_per_decoder_step"]
    out["distinct_sequences_per_graph"] = {
        "T=%g" % T: {path: run(path, a.max_steps, temperature=T)["distinct"] for path in ("stochastic", "sample")} for T in (1.0, 0.7)}
    with torch.no_grad():
        out["kernel_us"] = kernel_times(model, box["memory"], a.slots, a.temperature)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
