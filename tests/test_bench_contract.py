"""bench.py's output contract: one JSON line with the driver's fields, `roofline` and `cpu_baseline`."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DRIVER_FIELDS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better",
                 "scaling", "vs_baseline", "dtype", "data", "config", "roofline"}
ROOFLINE_FIELDS = {"bound", "achieved", "peak", "unit", "frac", "traffic"}
CPU_FIELDS = {"value", "unit", "cores", "kind", "sample"}


def test_cpu_baseline_leg_reports_the_oracle_on_host_cores():
    # the CPU leg runs before the GPU is touched and needs no device: the oracle in worker processes
    import bench
    import pydrobert_speech_amd as ps
    from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg

    cfg, n, _, _ = bench.WORKLOADS[bench.DEFAULT_WORKLOAD]
    comp = alias_factory_subclass_from_arg(ps.compute.FrameComputer, cfg)
    os.environ["OMP_NUM_THREADS"] = "1"
    res = bench.cpu_baseline(comp, 16000, budget_s=0.002)  # two one-second utterances per worker
    assert CPU_FIELDS <= set(res)
    assert res["kind"] == "port" and res["unit"] == "frames/s" and res["value"] > 0 and 1 <= res["cores"] <= 32
    json.dumps(res)


def test_workloads_name_the_baseline_configurations():
    import bench

    with open(os.path.join(ROOT, "BASELINE.json")) as fh:
        baseline = json.load(fh)
    assert bench.DEFAULT_WORKLOAD in bench.WORKLOADS
    cfg, n, batch, post = bench.WORKLOADS[bench.DEFAULT_WORKLOAD]
    # configs[1]: 1024 utterances of 10 s at 16 kHz, 40 mel filters, 25 / 10 ms frames
    assert (n, batch, post) == (160000, 1024, None)
    assert cfg["bank"]["num_filts"] == 40 and cfg["frame_length_ms"] == 25 and cfg["frame_shift_ms"] == 10
    assert "40-mel" in baseline["metric"] and "frames/s" in baseline["metric"]


def test_plain_run_leaves_the_extra_legs_to_full():
    import bench

    args = bench.build_parser().parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert args.steps == 7 and args.warmup == 2 and args.full is False and args.dump_outputs is None
    args = bench.build_parser().parse_args(["--full", "--dump-outputs", "out"])
    assert args.full is True and args.dump_outputs == "out"


def test_dump_outputs_samples_whole_utterances_within_the_budget(tmp_path):
    import numpy as np
    import torch

    import bench

    rng = np.random.default_rng(5)
    row_offsets = np.concatenate([[0], np.cumsum(rng.integers(0, 60, size=50))])
    feats = torch.from_numpy(rng.standard_normal((int(row_offsets[-1]), 6)).astype(np.float32))
    norm = torch.from_numpy(rng.standard_normal((int(row_offsets[-1]), 6)))
    # everything fits: the whole arrays
    picks = bench.dump_outputs(str(tmp_path / "all"), {"features": feats, "cmvn": norm}, row_offsets)
    assert list(picks) == list(range(50))
    got = np.load(tmp_path / "all" / "features.npy")
    assert got.dtype == np.float32 and np.array_equal(got, feats.numpy())
    assert np.load(tmp_path / "all" / "cmvn.npy").dtype == np.float64
    # over the budget: whole utterances in batch order, the same ones every time, within the budget
    budget = 400 * 6 * (4 + 8)
    picks = bench.dump_outputs(str(tmp_path / "a"), {"features": feats, "cmvn": norm}, row_offsets, budget=budget)
    again = bench.dump_outputs(str(tmp_path / "b"), {"features": feats, "cmvn": norm}, row_offsets, budget=budget)
    assert 0 < len(picks) < 50 and list(picks) == sorted(picks) and list(picks) == list(again)
    for name, full in (("features", feats), ("cmvn", norm)):
        got = np.load(tmp_path / "a" / f"{name}.npy")
        want = np.concatenate([full.numpy()[row_offsets[b] : row_offsets[b + 1]] for b in picks])
        assert np.array_equal(got, want) and np.array_equal(got, np.load(tmp_path / "b" / f"{name}.npy"))
    assert sum(np.load(tmp_path / "a" / f"{n}.npy").nbytes for n in ("features", "cmvn")) <= budget


@pytest.mark.gpu
def test_bench_prints_one_json_line_with_the_contract_fields():
    res = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--batch", "16", "--full",
         "--no-cpu-baseline", "--preroll-ms", "5"],
        capture_output=True, text=True, timeout=600,
    )
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert DRIVER_FIELDS <= set(line), sorted(DRIVER_FIELDS - set(line))
    assert ROOFLINE_FIELDS <= set(line["roofline"])
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1 and line["unit"] == "frames/s"
    assert line["scaling"] == "weak" and line["higher_is_better"] is True and line["vs_baseline"] is None
    assert line["dtype"] == "f32" and line["data"] == "synthetic" and "workload" in line["config"]
    assert line["roofline"]["bound"] == "hbm" and line["roofline"]["peak"] == 8000.0
    assert 0 < line["roofline"]["frac"] < 1 and line["value"] > 0 and line["outputs_finite"] is True
    # self-proving line: rows of the timed buffer against the oracle, the secondary ceilings, the cold step time
    spot = line["parity_spot_check"]
    assert spot["pass"] is True and spot["rows"] > 0 and spot["max_err_over_tolerance"] <= 1.0
    sec = line["roofline"]["secondary"]
    assert sec["fp32_valu"]["peak_tflops"] == 157.3 and 0 < sec["fp32_valu"]["frac"] < 1
    assert 10e3 < sec["fp32_valu"]["algorithmic_flop_per_frame"] < 20e3  # ~14 kflop per frame
    assert "lds" in sec
    assert line["cold_ms_per_step"] > 0


@pytest.mark.gpu
def test_bench_two_ranks_rehearsal_on_one_gpu():
    # the N > 1 path (launcher environment, barrier, max-over-ranks timing, rank 0 prints) with two
    # ranks sharing GPU 0 over gloo: RCCL needs one GPU per rank, which the driver's scaling run has
    import socket

    with socket.socket() as sock:
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    res = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr",
         "127.0.0.1", "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--backend", "gloo",
         "--steps", "3", "--warmup", "1", "--batch", "16", "--preroll-ms", "5"],
        capture_output=True, text=True, timeout=900, env=env,
    )
    assert res.returncode == 0, res.stderr[-3000:]
    lines = [l for l in res.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["value"] > 0
    # whole-job value: both ranks' frames over the slowest rank's time
    assert line["config"]["frames_per_gpu_per_step"] * 2 * line["steps"] / (line["ms_per_step"] * 1e-3 * line["steps"]) == pytest.approx(line["value"], rel=1e-6)


@pytest.mark.gpu
def test_plain_bench_times_the_steps_and_dumps_the_last_one(tmp_path):
    import types

    import numpy as np
    import torch

    import bench
    import pydrobert_speech_amd as ps
    from pydrobert_speech_amd.alias import alias_factory_subclass_from_arg

    res = subprocess.run(
        [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--batch", "16",
         "--preroll-ms", "5", "--dump-outputs", str(tmp_path)],
        capture_output=True, text=True, timeout=600,
    )
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, res.stdout[-2000:]
    line = json.loads(lines[0])
    assert DRIVER_FIELDS <= set(line) and line["steps"] == 4 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["dtype"] == "f32" and line["higher_is_better"] is True and line["unit"] == "frames/s"
    # the legs beyond the headline are --full's
    assert "cpu_baseline" not in line and line["parity_spot_check"] is None and line["roofline"]["power"] is None
    assert sorted(os.listdir(tmp_path)) == ["features.npy"]
    feats = np.load(tmp_path / "features.npy")
    frames, C = line["config"]["frames_per_gpu_per_step"], line["config"]["num_coeffs"]
    assert feats.dtype == np.float32 and feats.shape == (frames, C)
    # the dump is what the timed path computed from the benchmark's seeded input: rows against the oracle
    cfg, n, _, _ = bench.WORKLOADS[bench.DEFAULT_WORKLOAD]
    comp = alias_factory_subclass_from_arg(ps.compute.FrameComputer, cfg)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(1234)
    signal = torch.randn(16 * n, generator=g, device=dev, dtype=torch.float32).mul_(3000.0)
    lengths = np.full(16, n, dtype=np.int64)
    offsets = np.arange(16, dtype=np.int64) * n
    rows = np.arange(17, dtype=np.int64) * (frames // 16)
    spot = bench.parity_spot_check(comp, signal, offsets, lengths, types.SimpleNamespace(row_offsets=rows),
                                   torch.from_numpy(feats))
    assert spot["pass"] is True and spot["rows"] == 3 * (frames // 16), spot
