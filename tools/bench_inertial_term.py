#!/usr/bin/env python3
"""Times tc2li_inertial_term_batch (device) and tc2li_host_inertial_term_batch (host twin, tracking pool) on a batch of identical 25-link
windows -- the reference's bLarge inertial window, synthetic.inertial_window(2, n_opt=25, n_points=60) -- with linearize 1 and 0.  A tool
beside bench.py (which it does not touch); it needs a GPU and fails without one.

Only the C entry points are timed: the ctypes tables are packed before the clock starts, and each entry returns with its results in host
memory (the device entry ends in its own synchronise).  Both entries include the per-link preparation of the information matrices on the
host, which the contract puts into every call.  The four variants alternate inside every repetition, after warm-up calls of each.  Before
the clock the device results are compared with the host twin's.

Prints one JSON line: per variant the median, minimum and maximum call time in milliseconds, the pool size, the batch's sizes."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--windows", type=int, default=96)
    ap.add_argument("--n-opt", type=int, default=25)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import tc2li_loader
    pkg = tc2li_loader.load()
    if pkg.device_count() < 1:
        raise SystemExit("bench_inertial_term needs a GPU")
    from tc2li_slam_amd import synthetic
    capi, L = pkg.capi, pkg.lib()
    w = synthetic.inertial_window(2, n_opt=a.n_opt, n_points=60)
    pre = []
    for s, t1, t2 in w["samples"]:
        p = capi.Preintegrated(w["bias6"], *synthetic.IMU_NOISE)
        p.preintegrate(s, t1, t2)
        pre.append(p)
    problems = [dict(kf33=w["kf33"], fixed=w["fixed"], has_imu=w["has_imu"], link4=w["link4"], pre=pre)] * a.windows
    fd, fh = L.tc2li_inertial_term_batch, L.tc2li_host_inertial_term_batch
    fd.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    fh.argtypes = [C.c_void_p, C.c_int, C.c_int]
    packed = {lin: capi.pack_inertial_term_problems(problems, bool(lin)) for lin in (1, 0)}

    def call(device, lin):
        arr = packed[lin][0]
        rc = fd(C.addressof(arr), a.windows, lin, None) if device else fh(C.addressof(arr), a.windows, lin)
        if rc < 0:
            raise RuntimeError(L.tc2li_last_error().decode())

    # the same term on both sides before anything is timed
    got = capi.inertial_term_batch(problems[:2]), capi.inertial_term_batch(problems[:2], host=True)
    scale = np.abs(got[1][0][1]).max()
    assert abs(got[0][0][0] - got[1][0][0]) <= 1e-9 * abs(got[1][0][0]) and np.abs(got[0][0][1] - got[1][0][1]).max() <= 1e-9 * scale

    variants = [("device_linearize", True, 1), ("host_linearize", False, 1), ("device_cost", True, 0), ("host_cost", False, 0)]
    for _, device, lin in variants:
        for _ in range(a.warmup):
            call(device, lin)
    times = {name: [] for name, _, _ in variants}
    for _ in range(a.reps):
        for name, device, lin in variants:
            t0 = time.perf_counter()
            call(device, lin)
            times[name].append(time.perf_counter() - t0)
    out = dict(tool="bench_inertial_term", windows=a.windows, links_per_window=len(w["link4"]), keyframes_per_window=len(w["kf33"]), reps=a.reps,
               warmup=a.warmup, tracking_pool_threads=capi.host_threads()["tracking_pool"])
    for name, t in times.items():
        t = sorted(t)
        out[name] = dict(median_ms=1e3 * t[len(t) // 2], min_ms=1e3 * t[0], max_ms=1e3 * t[-1])
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
