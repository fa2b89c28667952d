"""Timings of the inertial local-BA window: tc2li_inertial_window_batch for a batch of windows of the camera-LiDAR-inertial loop's shape
(synthetic.inertial_window(100 + k, n_opt=25, n_points=1500), the windows bench.py's inertial loop optimises), their flat graphs built from
the windows' own edges (tests/inertial_window_cases.py from_inertial_window), beside the host entry tc2li_host_inertial_window_batch on the
same input.  Call times are host clocks around whole calls (validation, concatenation, upload, two kernels, download, copy-out); the Python
binding's packing of the problem structures is outside the clock.  Median of --reps after --warmup calls.  Every leg runs in a child process
of its own under a time limit, so that a hang ends that step and nothing more is started on the GPU after it.  The kernel leg repeats the
device calls with tc2li_profile_enable(1) and prints tc2li_profile_report's per-kernel times; the copy leg times one upload and one download
of the call's byte counts between pinned memory and the device.

    python tools/time_inertial_window.py [--problems 64] [--reps 20] [--warmup 3] [--json out.json]
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


def windows_of(pkg, n):
    """N_BASE windows, each with slots of its own in one store table -> (views of all slots, the base problems, the n problems, sigma)"""
    import inertial_window_cases as K
    from tc2li_slam_amd import synthetic
    views, base, sigma = [], [], None
    for i in range(N_BASE):
        v, pr, sigma = K.from_inertial_window(synthetic.inertial_window(100 + i, n_opt=25, n_points=1500))
        pr["kf_slot"] = pr["kf_slot"] + len(views)
        pr["with_lidar"] = 1
        views += v
        base.append(pr)
    return views, base, [base[i % N_BASE] for i in range(n)], sigma


def call_bytes(problems, outs):
    """(upload, download) bytes of one device call, as csrc/inertial_window_host.cpp lays them out (without the 256-byte rounding)"""
    up = down = 0
    for p, o in zip(problems, outs):
        nk, ns, npt, no = len(p["kf_slot"]), len(p["slot_point"]), len(p["point_flags"]), len(p["obs_kf"])
        up += 80 + (8 + 264 + 4 + 4 + 1) * nk + 4 * (nk + 1) + 4 * ns + 25 * npt + 4 * (npt + 1) + 8 * no
        down += 40 + 24 + 25 * 36 + (264 + 4 + 2) * min(nk, 225) + 28 * npt + 40 * no
    return up, down


def child(leg, n, reps, warmup):
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    import inertial_window_cases as K
    import inertial_window_ref as ref
    views, base, problems, sigma = windows_of(pkg, n)
    arr, outs, keep = capi.pack_inertial_window_problems(problems)
    if leg == "copy":
        import torch
        up, down = call_bytes(problems, outs)
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
        print(json.dumps(dict(leg=leg, upload_bytes=up, download_bytes=down, **out)))
        return
    sg = np.ascontiguousarray(sigma, np.float32)
    store = None
    if leg == "host":
        varr, vkeep = capi._pack_ba_window_views(views)
        f = capi.lib().tc2li_host_inertial_window_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        call = lambda: f(C.addressof(varr), len(views), C.addressof(arr), n, sg.ctypes.data, len(sg))
    else:
        store = pkg.KeyframeStore(len(views), max(len(v["keys"]) for v in views))
        store.put_batch(list(range(len(views))), views, K.BOUNDS, n_levels=K.N_LEVELS)
        f = capi.lib().tc2li_inertial_window_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        call = lambda: f(store._handle(), C.addressof(arr), n, sg.ctypes.data, len(sg), None)
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
    res = dict(leg=leg, problems=n, ms=float(np.median(times)), min_ms=float(min(times)), max_ms=float(max(times)))
    if leg == "kernels":
        res["kernels_ms_per_call"] = {k: v[1] / v[0] for k, v in capi.profile_report().items() if k.startswith(("k_iw", "k_window"))}
        capi.profile_enable(False)
    want = [ref.gather(p, views, sigma) for p in base[:2]]   # the restatement is a Python loop: two windows of the eight
    for i in range(n):
        if i % N_BASE < 2:
            w, o = want[i % N_BASE], outs[i]
            c = o["counts"]
            assert c[0] == w["status"] and np.array_equal(o["kf_row"][:c[3]], w["kf_row"]) and np.array_equal(o["point_row"][:c[4]], w["point_row"]) and \
                o["edges"][:c[5]].tobytes() == w["edges"].tobytes() and c[6] == len(w["link4"]) and c[7] == w["n_lidar"], i
    sizes = np.array([o["counts"] for o in outs[:N_BASE]])
    res.update(free_keyframes=[int(v) for v in sizes[:, 2]], vertices=[int(v) for v in sizes[:, 3]], points=[int(v) for v in sizes[:, 4]],
               edges=[int(v) for v in sizes[:, 5]], mean_vertices=float(sizes[:, 3].mean()), mean_points=float(sizes[:, 4].mean()),
               mean_edges=float(sizes[:, 5].mean()))
    if store is not None:
        store.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--json")
    ap.add_argument("--child", help="one leg in this process: device, host, kernels or copy")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.problems, a.reps, a.warmup)
        return
    rows = {}
    for leg in ("device", "kernels", "copy", "host"):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--problems", str(a.problems),
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("the %s leg ended with status %d; nothing more is started\n%s" % (leg, r.returncode, r.stderr[-2000:]))
        rows[leg] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rows[leg]), flush=True)
    d, h, c = rows["device"], rows["host"], rows["copy"]
    print("%d windows (%.0f vertices, %.0f points, %.0f edges each on average): device call %.2f ms (%.2f-%.2f), host entry %.2f ms (%.2f-%.2f); "
          "upload %.1f MB %.2f ms, download %.1f MB %.2f ms; kernels per call %s"
          % (a.problems, d["mean_vertices"], d["mean_points"], d["mean_edges"], d["ms"], d["min_ms"], d["max_ms"], h["ms"], h["min_ms"], h["max_ms"],
             c["upload_bytes"] / 1e6, c["upload_ms"], c["download_bytes"] / 1e6, c["download_ms"],
             ", ".join("%s %.3f ms" % kv for kv in sorted(rows["kernels"]["kernels_ms_per_call"].items()))))
    if a.json:
        json.dump(dict(reps=a.reps, warmup=a.warmup, **rows), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
