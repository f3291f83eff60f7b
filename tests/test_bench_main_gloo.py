"""bench.py's main() end to end on CPU, world size 2 over gloo -- the path the driver runs on an 8-GPU node and the builder
never could: self-launch (`--gpus 2` without a launcher environment re-executes under torch.distributed.run) -> RANK /
WORLD_SIZE from the environment -> init_process_group -> barrier -> timed steps -> barrier -> MAX over ranks -> ONE JSON line
from rank 0, for the inference workload and for `--workload train`.  tests/bench_main_harness.py replaces device management
and the compute with stubs (rank r sleeps 5 (r + 1) ms per step); the control flow is bench.py's."""
import json
import os
import socket
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HARNESS = os.path.join(HERE, "bench_main_harness.py")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _env():
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    env["OMP_NUM_THREADS"] = "1"
    return env


def _json_lines(out):
    return [json.loads(ln) for ln in out.splitlines() if ln.startswith("{")]


@pytest.mark.parametrize("workload", ["rpn", "train", "train-rcnn"])
def test_main_under_torch_distributed_run(workload):
    """launched exactly as the driver launches it: python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py"""
    steps = 4
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), HARNESS, "--gpus", "2", "--steps", str(steps), "--warmup", "1", "--workload", workload,
           "--no-roofline", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1, "exactly one JSON line, from rank 0: %r" % r.stdout
    line = lines[0]
    assert line["n_gpus"] == 2 and line["steps"] == steps and line["scaling"] == "weak"
    # the slow rank (rank 1: 10 ms per step) sets the time; value = frames of BOTH ranks over it
    assert line["ms_per_step"] >= 9.5
    batch = {"rpn": 32, "train": 16, "train-rcnn": 4}[workload]
    assert abs(line["value"] - batch * 2 * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    if workload == "rpn":
        assert line["config"]["parallelism"] == "frames sharded, dp2" and line["value_h2d_inclusive"] > 0 and line["value_latency_mode"] > 0


def test_main_self_launches_when_asked_for_more_than_one_gpu():
    """`python bench.py --gpus 2` with no launcher environment: re-executes itself as one rank per device"""
    r = subprocess.run([sys.executable, HARNESS, "--gpus", "2", "--steps", "3", "--warmup", "1", "--no-roofline", "--no-cpu-baseline",
                        "--no-variants"], capture_output=True, text=True, timeout=300, env=_env())
    assert r.returncode == 0, r.stderr[-2000:]
    assert "re-executing" in r.stderr
    lines = _json_lines(r.stdout)
    assert len(lines) == 1 and lines[0]["n_gpus"] == 2 and lines[0]["steps"] == 3


def test_main_refuses_a_world_size_that_disagrees_with_gpus():
    env = dict(_env(), WORLD_SIZE="2", RANK="0", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()))
    r = subprocess.run([sys.executable, HARNESS, "--gpus", "4"], capture_output=True, text=True, timeout=120, env=env)
    assert r.returncode != 0 and "WORLD_SIZE=2 but --gpus 4" in r.stderr


def test_inference_pipeline_bookkeeping_under_torch_distributed_run():
    """bench.py's REAL InferenceBench + pointrcnn_amd.pipeline.InferencePipeline (device "cpu": the slot / ticket /
    bounded-queue logic, eager steps) under `python -m torch.distributed.run`, world 2, gloo: 3 slots, more steps than slots (slots are
    reused, results collected in order), H2D-style submits and the one-batch-in-flight loop included (the variants' loops); rank 1's
    model is the slow one and sets the time"""
    steps = 7
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), HARNESS, "--gpus", "2", "--steps", str(steps), "--warmup", "2", "--batch", "4", "--npoints", "256",
           "--streams", "3", "--proposals", "off", "--graph", "off", "--no-roofline", "--no-cpu-baseline", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(_env(), PRCNN_HARNESS_REAL_PIPELINE="1", PRCNN_BENCH_NO_SPLIT="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    lines = _json_lines(r.stdout)
    assert len(lines) == 1
    line = lines[0]
    assert line["n_gpus"] == 2 and line["steps"] == steps and line["config"]["streams"] == 3 and line["config"]["launch"] == "eager"
    assert line["ms_per_step"] >= 5.5                                  # rank 1: 6 ms per step
    assert abs(line["value"] - 4 * 2 * 1e3 / line["ms_per_step"]) <= 0.01 * line["value"]
    assert line["value_h2d_inclusive"] > 0 and line["value_latency_mode"] > 0


def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    """without --full the line holds the timed loop only (no variant loops); --dump-outputs writes what the last timed step returned
    (the REAL InferenceBench + InferencePipeline on device "cpu" around the harness's toy model), identically from run to run"""
    import numpy as np
    steps, lines = 5, []
    for d in ("a", "b"):
        cmd = [sys.executable, HARNESS, "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--batch", "2", "--npoints", "64",
               "--streams", "2", "--proposals", "off", "--graph", "off", "--dump-outputs", str(tmp_path / d)]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=300, env=dict(_env(), PRCNN_HARNESS_REAL_PIPELINE="1"))
        assert r.returncode == 0, r.stderr[-3000:]
        lines += _json_lines(r.stdout)
    assert len(lines) == 2
    for line in lines:
        assert line["steps"] == steps and line["ms_per_step"] > 0 and line["unit"] == "frames/s" and line["higher_is_better"] is True
        assert not any(k in line for k in ("value_h2d_inclusive", "value_latency_mode", "roofline", "cpu_baseline", "arithmetics"))
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["backbone_features.npy", "backbone_xyz.npy", "rpn_cls.npy", "rpn_reg.npy"]
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype == np.float32 and a.size > 0 and np.array_equal(a, b)
    # the toy model's rpn_cls is 0.5 x the sum of each point's coordinates: the dump holds the batch of the LAST step's slot
    import bench
    from pointrcnn_amd import rpn
    slot = (1 + steps - 1) % 2          # tickets run on from the warm-up: timed step k runs on slot (warmup + k) % streams
    clouds = rpn.synthetic_clouds(2, 64, seed0=bench.shard_seed0(0, 1, slot, 2))
    assert np.allclose(np.load(tmp_path / "a" / "rpn_cls.npy"), clouds.sum(2, keepdim=True).numpy() * 0.5)


def test_dump_outputs_samples_what_exceeds_the_budget(tmp_path):
    """bench.dump_outputs: small outputs whole, larger ones a seeded sample within the byte budget; integers as float64"""
    import numpy as np
    import torch
    import bench
    outs = {"big": torch.arange(100000, dtype=torch.float32).reshape(100, 1000), "small": torch.ones(3, 2, dtype=torch.float16),
            "keep": torch.tensor([3, -1, 7], dtype=torch.int32), "pair": (torch.zeros(2), torch.ones(1, dtype=torch.float64))}
    rep = bench.dump_outputs(str(tmp_path / "a"), outs, budget=40000)
    bench.dump_outputs(str(tmp_path / "b"), outs, budget=40000)
    assert sorted(os.listdir(tmp_path / "a")) == ["big.npy", "keep.npy", "pair_0.npy", "pair_1.npy", "small.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) - 128 for f in os.listdir(tmp_path / "a")) <= 40000
    small, keep = np.load(tmp_path / "a" / "small.npy"), np.load(tmp_path / "a" / "keep.npy")
    assert small.dtype == np.float32 and small.shape == (3, 2) and keep.dtype == np.float64 and keep.tolist() == [3, -1, 7]
    big = np.load(tmp_path / "a" / "big.npy")
    assert big.ndim == 1 and 0 < big.size < 100000 and rep["big"] == ((100, 1000), big.size)
    assert np.all(np.diff(big) > 0) and np.array_equal(big, np.load(tmp_path / "b" / "big.npy"))     # sorted distinct elements, same sample
