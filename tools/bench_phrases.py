"""Cost and effect of phrase-constrained beam search on the device, on the `bench.py --decode` workload (C2 eval batch: 64 synthetic
100-node AMR graphs, beam 8, 50 steps, bf16, random weights): work(search="device") four ways, interleaved in one process after a
warm-up -- plain; the phrase route without phrases (the same search through gtos_phrase_advance: the kernel's cost alone); N
single-token phrases per graph; N two-token phrases per graph (the tokens: copy tokens of the graph that the plain search's best
hypothesis lacks, topped up with vocabulary words).  Prints one JSON line: per leg sentences/s, ms per decoder step and the steps
launched for every repeat; for the two legs with phrases the share of graphs all of whose finished hypotheses hold every phrase (and
the graphs that finished any), the share of graphs whose best hypothesis (get_k_best(1, alpha)) holds every phrase with the mean
log-likelihood given up for it (plain best score - phrase best score), and -- since the rule keeps the best hypothesis of every bank,
the unconstrained one included -- the share of graphs that hold SOME hypothesis, live or finished, with every phrase and the
log-likelihood its best one gives up.  Every leg is also reported against the slowest plain repeat of the same run, next to the plain
leg's own spread.

    python tools/bench_phrases.py [--config C2] [--beam 8] [--max-steps 50] [--phrases 4] [--repeats 3] [--dtype bf16]
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
    ap.add_argument("--phrases", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--dtype", choices=["bf16", "fp32"], default="bf16")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_phrases.py measures the GPU search: no GPU visible")
    from gtos_amd import synth, search
    from gtos_amd.config import generator_args
    from gtos_amd.generator import Generator
    from gtos_amd.pathtrie import attach_path_trie
    from gtos_amd.vocab import PAD, UNK, STR, END
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
    ones, twos = "%d single-token phrases per graph" % a.phrases, "%d two-token phrases per graph" % a.phrases
    legs = {"plain": (dict(), dict()), "no phrases by the new kernel": (dict(), dict(phrased=True)), ones: (dict(), dict()),
            twos: (dict(), dict())}

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
        return {"sentences_per_s": B / dt, "ms_per_decoder_step": 1e3 * (dt - t_enc) / max(1, launched), "steps": launched}, beams

    best = lambda beam: beam.get_k_best(1, ALPHA)[0]                      # noqa: E731
    # the phrases come from a plain run: what its best hypothesis of every graph lacks
    _, beams = run("plain", a.max_steps)
    words = [pv.idx2token(i) for i in range(pv.size - 1, -1, -1) if pv.idx2token(i) not in (PAD, UNK, STR, END)]
    phrases = {ones: [], twos: []}
    for b, beam in enumerate(beams):
        have = set(best(beam).seq)
        lacking = [w for _, w in sorted(batch_dev['local_idx2token'][b].items()) if w not in have] + [w for w in words if w not in have]
        phrases[ones].append([[w] for w in lacking[:a.phrases]])
        phrases[twos].append([lacking[2 * i:2 * i + 2] for i in range(a.phrases)])
    for leg, ps in phrases.items():
        legs[leg] = (dict(phrases=ps), dict())

    for leg in legs:                                      # warm-up: every shape, the search tables, the allocator
        run(leg, 3)
        run(leg, a.max_steps)
    runs = {leg: [] for leg in legs}
    key = lambda beams_: [(b.steps, [(h.seq, h.score) for h in b.hypotheses], [(h.seq, h.score) for h in b.completed_hypotheses]) for b in beams_]   # noqa: E731
    differing = lambda x, y: sum(p != q for p, q in zip(x, y))           # noqa: E731
    holds = lambda h, ps: search.phrase_state(h.seq, ps)[0] == (1 << len(ps)) - 1      # noqa: E731
    names = list(legs)
    last, plain_drift, forced_drift = {}, 0, 0
    for _ in range(a.repeats):
        for leg in legs:
            r, beams = run(leg, a.max_steps)
            if leg == names[0] and leg in last:               # the control: does the plain search repeat itself?
                plain_drift = max(plain_drift, differing(key(beams), last[leg][0]))
            finished = [list(b.completed_hypotheses) for b in beams]     # (get_k_best fills an empty list with the live hypotheses)
            held = [b.hypotheses + b.completed_hypotheses for b in beams]
            last[leg] = (key(beams), [best(b) for b in beams])
            if leg in phrases:
                ps, tops, base = phrases[leg], last[leg][1], last[names[0]][1]
                r["graphs_with_finished"] = sum(bool(f) for f in finished)
                r["share_finished_hold_all"] = sum(all(holds(h, p) for h in f) for f, p in zip(finished, ps)) / B
                r["share_best_holds_all"] = sum(holds(h, p) for h, p in zip(tops, ps)) / B
                r["mean_ll_given_up"] = sum(p.score - h.score for p, h in zip(base, tops)) / B
                full = [[h for h in hs if holds(h, p)] for hs, p in zip(held, ps)]
                r["share_some_holds_all"] = sum(bool(f) for f in full) / B
                gaps = [p.score - max(h.score for h in f) for p, f in zip(base, full) if f]
                r["mean_ll_given_up_by_best_full"] = sum(gaps) / len(gaps) if gaps else None
            runs[leg].append(r)
        forced_drift = max(forced_drift, differing(last[names[0]][0], last[names[1]][0]))
    out = {"metric": "device beam search: plain, the phrase route without phrases, and with %d single-token / %d two-token phrases per "
                     "graph (%s eval batch %d graphs, beam %d, %d steps, %s); share_finished_hold_all: graphs all of whose finished "
                     "hypotheses hold every phrase (graphs_with_finished: those that finished any); share_best_holds_all: graphs whose "
                     "best hypothesis holds every phrase; mean_ll_given_up: plain best score - phrase best score, mean over the graphs; "
                     "share_some_holds_all / mean_ll_given_up_by_best_full: the same for the best-scoring hypothesis, live or finished, "
                     "that holds every phrase" % (a.phrases, a.phrases, a.config, B, a.beam, a.max_steps, a.dtype), "repeats": a.repeats,
           "tokens_per_graph": {leg: [min(sum(len(p) for p in ps) for ps in pss), max(sum(len(p) for p in ps) for ps in pss)]
                                for leg, pss in phrases.items()}}
    for leg, rs in runs.items():
        out[leg] = {k_: [r[k_] for r in rs] for k_ in rs[0]}
    ms = out["plain"]["ms_per_decoder_step"]
    out["plain_ms_per_step_spread"] = (max(ms) - min(ms)) / min(ms)
    for leg in names[1:]:
        out[leg]["ms_per_step_over_worst_plain"] = [x / max(ms) for x in out[leg]["ms_per_decoder_step"]]
    # graphs (of B) whose beams differ: between two plain runs (the control), and between the plain run and the new route without phrases
    out["graphs_differing_plain_vs_plain"] = plain_drift
    out["graphs_differing_plain_vs_no_phrases"] = forced_drift
    print(json.dumps(out))
    if forced_drift and not plain_drift:
        raise SystemExit("the phrase route without phrases differs from the plain device search, which repeats itself exactly")


if __name__ == "__main__":
    main()
