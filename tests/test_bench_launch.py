"""`python bench.py --gpus N` must launch its own ranks (one per GPU) when it is not already under torch.distributed.run
-- the reference spawns its ranks itself (generator/train.py:173-190).  Checked on CPU with the --dry-launch leg (gloo)."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=e, capture_output=True, text=True, timeout=300)


def test_bench_self_launches_two_ranks():
    r = _run(["--gpus", "2", "--dry-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "dry-launch rank 0 of 2 ok" in r.stdout and "dry-launch rank 1 of 2 ok" in r.stdout


def test_bench_self_launches_eight_ranks_with_per_rank_thread_caps():
    """`python bench.py --gpus 8 --dry-launch`: the driver's 8-GPU command shape on this box (gloo rendezvous of eight ranks), and every
    rank reports its share of the usable host cores (bench.rank_cores: torch's intra-op pool and the loader threads are capped to it)."""
    import re
    r = _run(["--gpus", "8", "--dry-launch"])
    assert r.returncode == 0, r.stderr[-2000:]
    seen = re.findall(r"dry-launch rank (\d) of 8 ok \(host threads per rank (\d+) of (\d+) usable cores\)", r.stdout)
    assert sorted(int(x[0]) for x in seen) == list(range(8)), r.stdout
    assert all(int(x[1]) == max(1, int(x[2]) // 8) for x in seen)


def test_bench_rejects_mismatched_world_size():
    r = _run(["--gpus", "2", "--dry-launch"], env={"WORLD_SIZE": "1", "RANK": "0", "LOCAL_RANK": "0"})
    assert r.returncode != 0 and "WORLD_SIZE=1" in (r.stderr + r.stdout)


def test_cpu_baseline_leg_runs_on_a_tiny_config(monkeypatch):
    """bench.py's cpu_baseline leg end to end on the CPU (the oracle on a 2-graph C1 sample): the record carries every field
    the bench line promises -- a formatting slip here would only show up on the GPU box otherwise."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rec = bench.cpu_baseline("C1", 2, 1, budget_s=5.0, warmup=1)
    assert rec["kind"] == "port" and rec["unit"] == "graphs/s" and rec["value"] > 0 and rec["cores"] >= 1
    assert rec["encoder_only"]["value"] > 0 and "1 warm-up + 1 timed steps" in rec["sample"] and isinstance(rec["cpu"], str)


def test_bench_defaults_are_the_library_defaults(monkeypatch):
    """`python bench.py` with no flags measures what a user of the library gets: the reference's dropout semantics in the RelationEncoder
    (masks per (path, position), `encoder.MASK_SHARING`), one GPU, the BASELINE configuration the metric is quoted on, no opt-in legs."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_mod2", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    monkeypatch.setattr(sys, "argv", ["bench.py"])
    a = bench.parse()
    from gtos_amd import encoder
    assert a.relation_masks == "path" == encoder.MASK_SHARING
    assert a.gpus == 1 and a.config == "C2" and not a.graph_leg and not a.fresh_batches


def test_plain_run_leaves_the_secondary_legs_to_full(monkeypatch):
    """`python bench.py` runs what its headline needs; --full adds the legs after the timed region, and the options that only add to
    those legs imply it."""
    bench = _bench_module("bench_mod5")
    for argv, full in (([], False), (["--no-cpu-baseline", "--no-masks-leg"], False), (["--full"], True), (["--cpu-protocol"], True),
                       (["--config", "C1", "--graph-leg"], True)):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        assert bench.parse().full is full, argv


def _bench_module(name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_bench_rejects_zero_steps_and_dump_outside_the_training_step(monkeypatch, capsys):
    import pytest
    bench = _bench_module("bench_mod3")
    for argv in (["--steps", "0"], ["--dump-outputs", "d", "--decode"], ["--dump-outputs", "d", "--fresh-batches"]):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        with pytest.raises(SystemExit):
            bench.parse()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "7", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.steps == 7 and a.dump_outputs == "d"


def test_dump_outputs_writes_the_step_results_in_parameter_order(tmp_path, monkeypatch):
    """bench.dump_outputs on a CPU FlatParams: loss, parameters and Adam moments as float arrays in named_parameters order (the flat
    buffer's alignment padding left out), cut to the same seeded positions in every call once they exceed DUMP_SAMPLE, <= 64 MB."""
    import types
    import numpy as np
    import torch
    from gtos_amd.flat import FlatParams
    bench = _bench_module("bench_mod4")
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(13, 7), torch.nn.Linear(7, 5))
    flat = FlatParams(model)                          # CPU: views only, no kernels
    flat.m.normal_()
    flat.v.uniform_()
    trainer = types.SimpleNamespace(flat=flat, model=model)
    want = torch.cat([p.detach().reshape(-1) for p in model.parameters()]).numpy()
    bench.dump_outputs(str(tmp_path / "full"), trainer, 2.5)
    got = {k: np.load(str(tmp_path / "full" / (k + ".npy"))) for k in ("loss", "params", "adam_m", "adam_v")}
    assert got["loss"].dtype == np.float64 and got["loss"].tolist() == [2.5]
    assert got["params"].dtype == np.float32 and np.array_equal(got["params"], want)
    where = {n: o for n, _, o in flat.entries}
    m_want = np.concatenate([flat.m[where[n]:where[n] + p.numel()].numpy() for n, p in model.named_parameters()])
    assert np.array_equal(got["adam_m"], m_want) and got["adam_v"].shape == want.shape
    bench.dump_outputs(str(tmp_path / "skipped"), trainer, None)
    assert np.isnan(np.load(str(tmp_path / "skipped" / "loss.npy"))).all()
    assert 3 * 4 * bench.DUMP_SAMPLE + 8 < 64 * 10 ** 6                        # three fp32 arrays and the loss at the cap
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 40)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), trainer, 2.5)
    s1, s2 = (np.load(str(tmp_path / d / "params.npy")) for d in ("s1", "s2"))
    assert s1.shape == (40,) and np.array_equal(s1, s2) and np.isin(s1, want).all()
