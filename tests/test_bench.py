"""bench.py's JSON line contract (the driver parses it): BASELINE.json's
metric, the roofline and cpu_baseline objects, and values that recompute from
the line's own fields.  GPU: one short C1 run."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_line_contract(gpu_available):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c1", "--batch", "256",
                        "--steps", "3", "--warmup", "1", "--full", "--cpu-baseline-seconds", "1"],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    base = json.load(open(os.path.join(ROOT, "BASELINE.json")))
    assert d["metric"] == base["metric"] and d["unit"] == "info-bits/s"
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and "synthetic" in d["data"]
    cfg = d["config"]
    assert cfg["workload"].startswith("C1") and cfg["batch_per_gpu"] == 256 and cfg["global_batch"] == 256
    # value = frames * info bits / wall; ms_per_step is the same wall over the steps
    frames = cfg["global_batch"] * d["steps"]
    assert d["value"] == pytest.approx(frames * cfg["info_bits_per_frame"] / (d["ms_per_step"] * d["steps"] / 1e3),
                                       rel=1e-9)
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") or rf["bound"].startswith("fp64")
    assert rf["unit"] and rf["peak"] > 0 and rf["achieved"] > 0
    assert rf["frac"] == pytest.approx(rf["achieved"] / rf["peak"], rel=1e-12)
    assert "traffic" in rf
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["unit"] == "info-bits/s" and cb["cores"] >= 1 and cb["kind"] in ("port", "reference")
    assert cb["sample"]
    assert 0.0 <= d["fer"] <= 1.0 and d["mean_iterations"] >= 1.0
    assert d["decode_kernel_ms"] > 0 and d["trial_generation_s"] > 0


@pytest.mark.gpu
def test_bench_plain_run_dumps_its_outputs(gpu_available, tmp_path):
    """Without --full the run times its steps and prints the line (no serial
    roofline launches, no CPU baseline); --dump-outputs writes the last timed
    step's outputs as float32 .npy files that agree with the line's counters."""
    import numpy as np

    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "c1", "--batch", "256",
                        "--steps", "3", "--warmup", "1", "--dump-outputs", str(out)],
                       env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["cpu_baseline"] is None and d["decode_kernel_ms"] is None and d["trial_generation_s"] is None
    assert d["roofline"]["achieved"] > 0
    n = d["config"]["n"]
    got = {p.name: np.load(p) for p in out.iterdir()}
    assert sorted(got) == ["bits.npy", "bits_frames.npy", "iterations.npy", "key_match.npy", "synd_ok.npy"]
    assert all(a.dtype == np.float32 for a in got.values())
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert got["bits.npy"].shape == (256, n) and np.array_equal(got["bits_frames.npy"], np.arange(256))
    assert set(np.unique(got["bits.npy"])) <= {0.0, 1.0}
    for k in ("iterations.npy", "synd_ok.npy", "key_match.npy"):
        assert got[k].shape == (256,)
    assert d["mean_iterations"] == pytest.approx(got["iterations.npy"].mean(), rel=1e-6)
    assert d["fer"] == pytest.approx(1.0 - got["synd_ok.npy"].mean(), abs=1e-9)
    assert d["key_mismatch_rate"] == pytest.approx(1.0 - got["key_match.npy"].mean(), abs=1e-9)
