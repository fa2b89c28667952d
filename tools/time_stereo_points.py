"""Timings of tc2li_stereo_points_batch and tc2li_new_keyframe_batch for a batch of generated frames (tests/stereo_points_cases.py: 2000
keypoints, about two thirds with depth, every decision a yes) beside the host entries on the same frames.  Call times are host clocks
around whole calls (validation, packing, upload, one kernel, download, copy-out); the Python binding's packing of the frame structures is
outside the clock.  Median, minimum and maximum of --reps after one warm-up.  Every leg runs in a child process of its own under a time
limit, so that a hang ends that step and nothing more is started on the GPU after it.

    python tools/time_stereo_points.py [--frames 512] [--keypoints 2000] [--reps 9] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_BASE = 16


def frames_of(n_frames, n_keypoints):
    import stereo_points_cases as K
    base = []
    for i in range(N_BASE):
        rng = np.random.default_rng(800 + i)
        d = np.where(rng.random(n_keypoints) < 0.3, rng.uniform(0.5, K.TH_DEPTH, n_keypoints), rng.uniform(K.TH_DEPTH, 300.0, n_keypoints))
        d[rng.random(n_keypoints) < 0.33] = -1.0
        base.append(K.frame(d, rng.choice([0, 1, 2], n_keypoints, p=[0.5, 0.4, 0.1]), rng.random(n_keypoints) < 0.1, seed=800 + i))
    return base, [base[i % N_BASE] for i in range(n_frames)], [K.decision(frame_id=120) for _ in range(n_frames)]


def child(entry, n_frames, n_keypoints, reps, host):
    import stereo_points_cases as K
    import stereo_points_ref as ref
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    base, frames, decisions = frames_of(n_frames, n_keypoints)
    arr, outs, keep = capi.pack_stereo_points_frames(frames)
    u4 = K.UNPROJECT4
    if entry == "points":
        f = getattr(capi.lib(), "tc2li_%sstereo_points_batch" % ("host_" if host else ""))
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p] + ([] if host else [C.c_void_p])
        call = lambda: f(C.addressof(arr), n_frames, u4.ctypes.data, *([] if host else [None]))
    else:
        dec, ver = (capi.KeyframeDecision * n_frames)(), (capi.KeyframeVerdict * n_frames)()
        for i, d in enumerate(decisions):
            for k in capi._DECISION_SCALARS:
                setattr(dec[i], k, float(d[k]) if k.startswith("time_") else int(d[k]))
        f = getattr(capi.lib(), "tc2li_%snew_keyframe_batch" % ("host_" if host else ""))
        f.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_void_p] + ([] if host else [C.c_void_p])
        call = lambda: f(C.addressof(arr), C.addressof(dec), C.addressof(ver), n_frames, u4.ctypes.data, *([] if host else [None]))
    assert call() == n_frames, capi.lib().tc2li_last_error()      # warm-up: buffers, pools
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        rc = call()
        times.append((time.perf_counter() - t) * 1e3)
        assert rc == n_frames
    want = [ref.stereo_points(fr, u4) for fr in base]
    for i in range(n_frames):
        w = want[i % N_BASE]
        assert outs[i]["counts"].tolist() == [w["n_created"], w["n_visited"], w["n_with_depth"]], i
        assert np.array_equal(outs[i]["created_keypoint"][:w["n_created"]], w["created_keypoint"]), i
        assert np.array_equal(outs[i]["x3D"][:w["n_created"]].view(np.uint32), w["x3D"].view(np.uint32)), i
        assert entry == "points" or ver[i].need == 1
    print(json.dumps(dict(entry=entry, frames=n_frames, keypoints=n_keypoints, host=host, ms=float(np.median(times)), min_ms=min(times), max_ms=max(times),
                          all_ms=times, created_per_frame=sum(w["n_created"] for w in want) / N_BASE, host_threads=capi.host_threads()["tracking_pool"])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=512)
    ap.add_argument("--keypoints", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--timeout", type=int, default=120)
    ap.add_argument("--json")
    ap.add_argument("--child", help="points or decision: one leg in this process")
    ap.add_argument("--host", action="store_true", help="with --child: the host entry")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.frames, a.keypoints, a.reps, a.host)
        return
    rows = []
    for entry in ("points", "decision"):
        for host in (False, True):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", entry, "--frames", str(a.frames),
                   "--keypoints", str(a.keypoints), "--reps", str(a.reps)]
            r = subprocess.run(cmd + (["--host"] if host else []), capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("the %s leg of %s ended with status %d; nothing more is started\n%s" % ("host" if host else "device", entry, r.returncode, r.stderr[-2000:]))
            rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
            o = rows[-1]
            print("%-8s %-6s %d frames x %d keypoints: %.2f ms (min %.2f, max %.2f over %d calls); %.0f points created per frame; tracking pool of %d threads"
                  % (entry, "host" if host else "device", a.frames, a.keypoints, o["ms"], o["min_ms"], o["max_ms"], a.reps, o["created_per_frame"], o["host_threads"]), flush=True)
    if a.json:
        json.dump(dict(reps=a.reps, rows=rows), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
