"""bench.py's plain run and --dump-outputs: a plain run prints the headline line alone (the other
legs are behind --full), --steps sets the timed steps, and the dump is float32 / float64 .npy
files within the size bound, the same rows from run to run."""
import importlib.util
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
FULL_ONLY = ("roofline", "matcher_roofline", "latency", "cpu_baseline", "local_ba", "global_ba", "ransac",
             "nfeatures_2000", "sequence_pipeline", "value_host_io")


def _bench_module():
    spec = importlib.util.spec_from_file_location("bench_under_test", ROOT / "bench.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_keeps_everything_under_the_bound(tmp_path):
    bench = _bench_module()
    rng = np.random.default_rng(0)
    arrays = {"a": rng.random((1000, 7)).astype(np.float32), "b": rng.random(63), "c": rng.random((63, 16))}
    bench.dump_outputs(tmp_path / "d", arrays)
    for k, v in arrays.items():
        got = np.load(tmp_path / "d" / f"{k}.npy")
        assert got.dtype == v.dtype and np.array_equal(got, v)


def test_dump_samples_the_same_rows_over_the_bound(tmp_path, monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 64 << 10)
    rng = np.random.default_rng(1)
    arrays = {"big": rng.random((20000, 8)), "small": rng.random((63, 16)).astype(np.float32)}
    for d in ("d1", "d2"):
        bench.dump_outputs(tmp_path / d, arrays)
    size = sum(f.stat().st_size for f in (tmp_path / "d1").iterdir())
    assert size <= 64 << 10
    for k, v in arrays.items():
        a, b = np.load(tmp_path / "d1" / f"{k}.npy"), np.load(tmp_path / "d2" / f"{k}.npy")
        assert np.array_equal(a, b) and a.dtype == v.dtype and 1 <= len(a) < len(v)
        # every kept row is a row of the output, in order
        rows = [int(np.flatnonzero((v == r).all(axis=1))[0]) for r in a[:50]]
        assert rows == sorted(rows)


def test_dump_refuses_integer_arrays(tmp_path):
    with pytest.raises(AssertionError):
        _bench_module().dump_outputs(tmp_path / "d", {"n": np.arange(4)})


@pytest.mark.gpu
def test_plain_run_line_and_dump(gpu, tmp_path):
    """A small plain run (4 stereo frames per step, 3 timed steps): the line has the headline keys
    and none of the --full legs, and the dump holds the last step's results."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--batch", "4", "--dump-outputs", str(out)], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["unit"] == "frames/s" and line["higher_is_better"] is True
    assert line["dtype"] == "u8" and line["ms_per_step"] > 0 and line["value"] > 0
    # value and ms_per_step describe the same timed region (3 tracked pairs per step); ms_per_step
    # is rounded to 1e-3 ms
    assert abs(3e3 / line["value"] - line["ms_per_step"]) <= 1e-3
    assert not [k for k in FULL_ONLY if k in line]
    files = sorted(out.glob("*.npy"))
    assert files and sum(f.stat().st_size for f in files) <= 64 << 20
    z = {f.stem: np.load(f) for f in files}
    assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in z.values())
    nL = z["n_keypoints_left"].astype(int)
    assert nL.shape == (4,) and (nL > 0).all()
    cap = len(z["keypoints_left"]) // 4
    kps = z["keypoints_left"].reshape(4, cap, 7)
    for b in range(4):   # written rows are keypoints inside the image, the rest is zero
        assert (kps[b, :nL[b], 2] > 0).all() and not kps[b, nL[b]:].any()
        assert (kps[b, :nL[b], 0] < 1241).all() and (kps[b, :nL[b], 1] < 376).all()
    for name in ("pose_motion_model", "pose_local_map"):   # rigid poses: orthonormal rotation, last row 0 0 0 1
        T = z[name].reshape(3, 4, 4)
        R = T[:, :3, :3].astype(np.float64)
        assert np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max() < 1e-4
        assert np.array_equal(T[:, 3], np.tile(np.float32([0, 0, 0, 1]), (3, 1)))
    assert z["n_inliers_local_map"].shape == (3,) and (z["n_inliers_local_map"] > 0).all()
