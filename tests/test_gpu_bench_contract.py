"""bench.py's one-line JSON contract on a short config-2 run (MI355X): the
keys the driver reads, and under --full the roofline and cpu_baseline objects
and the parity probe within tolerance, for serial and pipelined steps
(--lanes 1 / 2); a plain run's lean line and its --dump-outputs files."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("lanes", [1, 2])
def test_bench_json_line(lanes):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--steps", "4", "--warmup", "2",
           "--seconds", "10", "--cpu-seconds", "1", "--lanes", str(lanes), "--preroll-s", "0.2",
           "--kernel-launches", "5"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
              "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline", "parity"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 4 and d["warmup"] == 2
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["higher_is_better"] is True
    assert d["config"]["workload"].startswith("config2") and d["config"]["lanes"] == lanes
    samples = d["config"]["channels"] * d["config"]["samples_per_channel"]
    assert abs(d["value"] - samples / (d["ms_per_step"] / 1e3) / 1e6) / d["value"] < 0.01
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5
    # config 2's 4 001 linear-phase taps: the L = 32 768 register-resident kernel
    assert r["kernel"] == "fir_fft32r_kernel" and r["launches_timed"] == 5
    # achieved = algorithmic read bytes of one launch / its exclusive duration
    assert abs(r["achieved"] - 4 * samples / (r["kernel_ms"] / 1e3) / 1e9) / r["achieved"] < 1e-3
    assert d["preroll"]["steps"] > 0
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["kind"] == "port" and cb["cores"] >= 1 and cb["sample"]
    assert d["parity"]["rms_vs_longdouble"] <= d["parity"]["tol"] == 1e-9
    assert d["parity"]["max_ulp"] <= 1.0
    ing = d["ingest"]  # PCIe ingest probe: reported beside `value`, never in it
    assert ing["format"] == "s24le" and ing["decode_exact"] is True
    assert ing["bytes"] == 3 * ing["frames"] * ing["channels"] and 0 < ing["h2d_GBps"] < 200


def test_bench_plain_line_and_dumped_outputs(tmp_path):
    """A plain run (no --full): the headline keys, the whole-step roofline, none
    of the probes, and --dump-outputs' files = the last timed step's outputs:
    float32, the shard's shape, the filter's output at sampled positions (long-
    double oracle, 1 f32 ulp as the parity probe allows) and peaks = max |y|."""
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    import oracle  # conftest.py puts oracle/ and the package on sys.path
    import synth
    out_dir = tmp_path / "out"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--seconds", "2", "--preroll-s", "0.2", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["full"] is False and d["steps"] == 3 and d["warmup"] == 1 and d["n_gpus"] == 1
    assert d["metric"] and d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    samples = d["config"]["channels"] * d["config"]["samples_per_channel"]
    assert samples == 2 * 96000
    assert abs(d["value"] - samples / (d["ms_per_step"] / 1e3) / 1e6) / d["value"] < 0.01
    for k in ("cpu_baseline", "parity", "ingest"):
        assert k not in d, k
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["peak"] == 8000.0 and "kernel_ms" not in r
    assert abs(r["achieved"] - 4 * samples / (d["ms_per_step"] / 1e3) / 1e9) / r["achieved"] < 0.01
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-5
    assert sorted(os.listdir(out_dir)) == ["peaks.npy", "y_file0_0_96000.npy"]
    assert set(d["outputs"]["files"]) == {"peaks", "y_file0_0_96000"}
    y = np.load(out_dir / "y_file0_0_96000.npy")
    pk = np.load(out_dir / "peaks.npy")
    assert y.dtype == np.float32 and y.shape == (2, 96000) and pk.dtype == np.float32 and pk.shape == (1,)
    assert d["outputs"]["bytes"] == sum(os.path.getsize(out_dir / f) for f in os.listdir(out_dir)) <= 64_000_000
    assert pk[0] == np.abs(y).max()  # below 1: the step's normalize left the outputs alone
    oracle.load()
    x = synth.file_buffer(2, 96000, 48000.0, file=0, bits=24)
    taps = bench.design_taps(4001, 48000.0)
    idx = np.unique(np.r_[np.arange(64), np.arange(96000 - 64, 96000),
                          np.random.default_rng(11).integers(0, 96000, 512)])
    for c in range(2):
        ref, _ = oracle.filter_points(x[c], taps, idx, oracle.MODE_LD)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(y[c][idx].astype(np.float64) - ref) <= ulp)


def test_bench_gpus2_spawns_two_ranks():
    """`bench.py --gpus 2` started bare (no WORLD_SIZE) runs two ranks itself
    (torch.distributed.run, one process per rank); on the one-GPU box they
    share the device (LCFIR_BENCH_SHARE_DEVICE=1, gloo).  Config 5 with 2
    files: one file per rank and the peak exchange of --normalize."""
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    env["LCFIR_BENCH_SHARE_DEVICE"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--full", "--gpus", "2", "--config", "5", "--files", "2",
           "--seconds", "20", "--steps", "3", "--warmup", "1", "--preroll-s", "0.2", "--kernel-launches", "3",
           "--no-ingest"]
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=110, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["n_gpus"] == 2 and d["config"]["files"] == 2
    assert d["config"]["peak_exchange"] is True and d["config"]["normalize"] is True
    assert d["parity"]["rms_vs_longdouble"] <= 1e-9
    assert "cpu_baseline" not in d  # rank 0 at N = 1 only
