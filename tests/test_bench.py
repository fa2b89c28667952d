"""bench.py's inputs and outputs: the rendered frames do not depend on how many processes rendered them, and a plain run at a small size prints
the headline alone and writes the same --dump-outputs arrays every time it is run with the same arguments."""
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--gpus", "1", "--sequences", "8", "--unique", "2", "--cycle-frames", "2", "--map-length", "100", "--steps", "3", "--warmup", "2"]


def test_worker_processes_render_the_same_inputs(tmp_path, monkeypatch):
    sys.path.insert(0, ROOT)
    import bench
    import tc2li_loader
    tc2li_loader.load()
    from tc2li_slam_amd import synthetic
    runs = []
    for workers in (1, 3):
        cache = tmp_path / str(workers)
        cache.mkdir()
        monkeypatch.setattr(tempfile, "tempdir", str(cache))   # (a cache of its own: render, do not load)
        runs.append(bench.Workload._render_frames(synthetic, 2, 2, synthetic.WIDTH, synthetic.HEIGHT, workers=workers))
        assert len(os.listdir(cache)) == 1
    for a, b in zip(*runs):
        assert np.array_equal(a.images, b.images) and a.images.shape == (2, 2, synthetic.HEIGHT, synthetic.WIDTH)
        assert len(a.scans) == len(b.scans) == 2 and all(np.array_equal(x, y) for x, y in zip(a.scans, b.scans))


def _plain_run(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + list(extra), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_dumps_the_same_outputs_twice(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    for line in (_plain_run("--dump-outputs", str(a)), _plain_run("--dump-outputs", str(b))):
        assert line["steps"] == 3 and line["warmup"] == 2 and line["ms_per_step"] > 0 and line["value"] > 0 and line["unit"] == "frames/s"
        assert line["roofline"] is None and line["cpu_baseline"] is None and "detail" not in line   # the other legs run with --full
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    assert {"orb_keypoints.npy", "orb_descriptors.npy", "stereo_matches.npy", "track_motion_poses.npy", "track_local_poses.npy", "lidar_counts.npy",
            "map_incremental.npy", "map_sizes.npy", "ba_windows.npy", "ba_poses.npy", "ba_points.npy", "ba_chi2.npy"} <= set(names)
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), n
        assert np.array_equal(x, y, equal_nan=True), n
        total += x.nbytes
    assert total <= 64 << 20
    assert len(np.load(a / "orb_keypoints.npy")) > 1000 and len(np.load(a / "ba_windows.npy")) == 8   # 2 windows per step x 4 mapping workers
