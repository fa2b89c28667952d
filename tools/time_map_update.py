"""Timings of the map update of IMU initialisation: tc2li_apply_scaled_rotation_batch and tc2li_gba_map_correction_batch for a batch of maps
of the size IMU initialisation meets (30 keyframes, 6 000 points with 5 observations each), beside their host twins on the same input,
host memory to host memory.  Call times are host clocks around whole calls (validation, concatenation, upload, two kernels, download,
copy-out); the Python binding's packing of the problem structures is outside the clock.  Median of --reps after --warmup calls.  Every leg
runs in a child process of its own under a time limit, so that a hang ends that step and nothing more is started on the GPU after it.  The
kernel leg repeats the device calls with tc2li_profile_enable(1) and prints tc2li_profile_report's per-kernel times; the copy leg times one
upload and one download of the call's byte counts between pinned memory and the device.

    python tools/time_map_update.py [--problems 64] [--reps 20] [--warmup 3] [--json out.json]
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

N_BASE = 8
N_KF, N_POINTS, N_OBS = 30, 6000, 5


def problems_of(entry, n):
    import map_update_cases as K
    if entry == "rotation":
        base = [K.rot_problem(100 + i, N_KF, [N_OBS] * N_POINTS, s=[0.1, 1.0, 7.3][i % 3], scaled_vel=i & 1, has_tcb=1) for i in range(N_BASE)]
    else:
        base = [K.random_gba_problem(100 + i, N_KF, N_POINTS) for i in range(N_BASE)]
    return base, [base[i % N_BASE] for i in range(n)]


def call_bytes(entry, n):
    """(upload, download) bytes of one device call, as csrc/map_update_host.cpp lays them out (without the 256-byte rounding)"""
    tiles = 8 * ((N_POINTS + 255) // 256)
    if entry == "rotation":
        return n * (64 + 8 + tiles + 40 * N_KF + 21 * N_POINTS + 4 * (N_POINTS + 1) + 4 * N_OBS * N_POINTS), n * (80 * N_KF + 32 * N_POINTS)
    return n * (16 + tiles + 165 * N_KF + 30 * N_POINTS), n * (94 * N_KF + 13 * N_POINTS)


def child(entry, leg, n, reps, warmup):
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    import map_update_cases as K
    import map_update_ref as ref
    if leg == "copy":
        import torch
        up, down = call_bytes(entry, n)
        out = {}
        for name, nbytes, to_device in (("upload_ms", up, True), ("download_ms", down, False)):
            h, d = torch.empty(nbytes, dtype=torch.uint8).pin_memory(), torch.empty(nbytes, dtype=torch.uint8, device="cuda")
            times = []
            for _ in range(warmup + reps):
                torch.cuda.synchronize()
                t = time.perf_counter()
                (d.copy_(h, non_blocking=True) if to_device else h.copy_(d, non_blocking=True))
                torch.cuda.synchronize()
                times.append((time.perf_counter() - t) * 1e3)
            out[name] = float(np.median(times[warmup:]))
        print(json.dumps(dict(entry=entry, leg=leg, upload_bytes=up, download_bytes=down, **out)))
        return
    base, problems = problems_of(entry, n)
    pack, name, prefix = ((capi.pack_scaled_rotation_problems, "tc2li_%sapply_scaled_rotation_batch", "k_rot") if entry == "rotation" else
                          (capi.pack_gba_correction_problems, "tc2li_%sgba_map_correction_batch", "k_gba"))
    arr, outs, keep = pack(problems, K.FILL)
    if leg == "host":
        f = getattr(capi.lib(), name % "host_")
        f.argtypes = [C.c_void_p, C.c_int]
        call = lambda: f(C.addressof(arr), n)
    else:
        f = getattr(capi.lib(), name % "")
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        call = lambda: f(C.addressof(arr), n, None)
    for _ in range(warmup):                                  # buffers, pools, clocks
        assert call() == n, capi.lib().tc2li_last_error()
    if leg == "kernels":
        capi.profile_enable(True)
        capi.profile_report()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        rc = call()
        times.append((time.perf_counter() - t) * 1e3)
        assert rc == n
    res = dict(entry=entry, leg=leg, problems=n, ms=float(np.median(times)), min_ms=float(min(times)), max_ms=float(max(times)))
    if leg == "kernels":
        res["kernels_ms_per_call"] = {k: v[1] / v[0] for k, v in capi.profile_report().items() if k.startswith(prefix)}
        capi.profile_enable(False)
    want = (ref.apply_scaled_rotation(base[0], K.FILL) if entry == "rotation" else ref.gba_map_correction(base[0]))   # a Python loop: one of the eight
    for i in range(0, n, N_BASE):
        K.assert_equal(outs[i], want, "problem %d" % i)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--json")
    ap.add_argument("--child", nargs=2, metavar=("ENTRY", "LEG"), help="one leg in this process: rotation or correction; device, host, kernels or copy")
    a = ap.parse_args()
    if a.child:
        child(a.child[0], a.child[1], a.problems, a.reps, a.warmup)
        return
    rows = {}
    for entry in ("rotation", "correction"):
        for leg in ("device", "kernels", "copy", "host"):
            cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", entry, leg, "--problems", str(a.problems),
                   "--reps", str(a.reps), "--warmup", str(a.warmup)]
            r = subprocess.run(cmd, capture_output=True, text=True)
            if r.returncode != 0:
                sys.exit("the %s leg of %s ended with status %d; nothing more is started\n%s" % (leg, entry, r.returncode, r.stderr[-2000:]))
            rows[entry + "_" + leg] = json.loads(r.stdout.strip().splitlines()[-1])
            print(json.dumps(rows[entry + "_" + leg]), flush=True)
        d, h, c, k = (rows[entry + "_" + leg] for leg in ("device", "host", "copy", "kernels"))
        print("%s, %d maps of %d keyframes and %d points with %d observations each: device call %.2f ms (%.2f-%.2f), host entry %.2f ms (%.2f-%.2f); "
              "upload %.1f MB %.2f ms, download %.1f MB %.2f ms; kernels per call %s"
              % (entry, a.problems, N_KF, N_POINTS, N_OBS, d["ms"], d["min_ms"], d["max_ms"], h["ms"], h["min_ms"], h["max_ms"], c["upload_bytes"] / 1e6,
                 c["upload_ms"], c["download_bytes"] / 1e6, c["download_ms"], ", ".join("%s %.3f ms" % kv for kv in sorted(k["kernels_ms_per_call"].items()))),
              flush=True)
    if a.json:
        json.dump(dict(reps=a.reps, warmup=a.warmup, **rows), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
