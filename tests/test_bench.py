"""bench.py's contract: `--steps` is the number of timed steps, a plain run times the headline only (everything else
behind --full), and --dump-outputs writes what the timed pass computed, the same from run to run."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import cases

BENCH = os.path.join(cases.ROOT, "bench.py")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_for_test", BENCH)
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def test_timed_steps_are_cut_into_windows_that_add_up_to_steps():
    bench = _bench_module()
    for steps in (1, 2, 5, 7, 20, 199, 200):
        for windows in (1, 2, 7, 50):
            sizes = bench.split_steps(steps, windows)
            assert sum(sizes) == steps and len(sizes) == min(windows, steps)
            assert max(sizes) - min(sizes) <= 1 and min(sizes) >= 1


def test_only_the_options_that_measure_more_ask_for_the_full_run(monkeypatch):
    bench = _bench_module()
    for argv, full in ((["--gpus", "1", "--steps", "5", "--warmup", "2"], False),
                       (["--steps", "5", "--no-configs", "--no-cpu-baseline"], False),
                       (["--steps", "5", "--dump-outputs", "d"], False),
                       (["--full"], True), (["--detail"], True), (["--extra"], True)):
        monkeypatch.setattr(sys, "argv", ["bench.py"] + argv)
        assert bench.parse_args().full is full, argv
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "0"])
    with pytest.raises(SystemExit):
        bench.parse_args()


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["SHL_BENCH_FULL"] = os.path.join(out_dir, "bench_full.json")
    res = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "9", "--warmup", "2", "--dump-outputs",
                          os.path.join(out_dir, "outputs")], capture_output=True, text=True, timeout=600, env=env, cwd=cases.ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    line = json.loads(res.stdout.strip().splitlines()[-1])
    with open(env["SHL_BENCH_FULL"]) as f:
        full = json.load(f)
    return line, full


@pytest.mark.gpu
def test_plain_run_times_exactly_steps_and_dumps_the_same_outputs_twice(tmp_path):
    dumps = []
    for k in range(2):
        d = str(tmp_path / ("run%d" % k))
        os.makedirs(d)
        line, full = _plain_run(d)
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in line, key
        assert line["steps"] == 9 and full["window_steps"] == [9] and len(full["windows_ms"]) == 1
        assert line["ms_per_step"] > 0 and line["value"] == pytest.approx(1e3 / line["ms_per_step"], rel=1e-3)
        for key in ("roofline", "cpu_baseline", "configs", "mfma_rate", "session_ms_per_image"):
            assert key not in line, key
        files = sorted(os.listdir(os.path.join(d, "outputs")))
        # MobileNetV1: the last pointwise layer's output (read by the average pooling, outside the 28 conv layers) and the
        # classifier's
        assert files == ["layer26.npy", "layer27.npy"], files
        arrays = [np.load(os.path.join(d, "outputs", f)) for f in files]
        assert [a.shape for a in arrays] == [(1, 7, 7, 1024), (1, 1, 1, 1000)]
        assert all(a.dtype == np.float32 and np.all(a == np.round(a)) and a.min() >= -128 and a.max() <= 127 for a in arrays)
        assert arrays[1].std() > 0
        dumps.append(arrays)
    for a, b in zip(*dumps):
        assert np.array_equal(a, b)


@pytest.mark.gpu
def test_dump_of_a_large_output_is_a_fixed_sample_within_the_limit(tmp_path):
    """the ResNet-50 3x3 set at batch 128: sixteen independent layers, 25 MB of int8 output each -- the dump holds a seeded
    sample of every one of them, within the limit"""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_PORT")}
    env["SHL_BENCH_FULL"] = str(tmp_path / "bench_full.json")
    out = tmp_path / "outputs"
    res = subprocess.run([sys.executable, BENCH, "--workload", "resnet50_3x3", "--steps", "2", "--warmup", "1", "--dump-outputs",
                          str(out)], capture_output=True, text=True, timeout=600, env=env, cwd=cases.ROOT)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-3000:]
    files = sorted(os.listdir(out))
    assert files == ["layer%02d.npy" % i for i in range(16)], files
    assert sum(os.path.getsize(out / f) for f in files) <= 64 * 1000 * 1000
    for f in files:
        a = np.load(out / f)
        assert a.dtype == np.float32 and a.ndim == 1 and a.std() > 0
