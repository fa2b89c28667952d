"""Timings of local mapping's covisibility update: tc2li_update_connections_batch for a batch of generated problems of the workload's own
shape (tests/connections_cases.py workload(): about 1 000 slots, 10-20 observations per point, 40-120 counted keyframes) beside the host
entry tc2li_host_update_connections_batch on the same problems.  Call times are host clocks around whole calls (validation, concatenation,
upload, two kernels, download, copy-out); the Python binding's packing of the problem structures is outside the clock.  Median of --reps
after --warmup calls.  Every leg runs in a child process of its own under a time limit, so that a hang ends that step and nothing more is
started on the GPU after it.  The kernel leg repeats the device calls with tc2li_profile_enable(1) and prints tc2li_profile_report's
per-kernel times; the copy leg times one upload and one download of the call's byte counts between pinned memory and the device.

    python tools/time_connections.py [--problems 512] [--reps 20] [--warmup 3] [--json out.json]
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

N_BASE = 32


def problems_of(n):
    import connections_cases as K
    base = [K.workload(900 + i) for i in range(N_BASE)]
    return base, [base[i % N_BASE] for i in range(n)]


def call_bytes(problems):
    """(upload, download) bytes of one device call, as csrc/connections_host.cpp lays them out (without the 256-byte rounding)"""
    up = down = 0
    for p in problems:
        nk, nc, ns, npt, no = len(p["kf_flags"]), len(p["conn_kf"]), len(p["slot_point"]), len(p["point_bad"]), len(p["obs_kf"])
        cc, oc, hc = nk, nk, nc + nk
        up += 80 + 4 * oc + nk + 4 * (nk + 1) + 8 * nc + 4 * ns + npt + 4 * (npt + 1) + 4 * no
        down += 32 + 8 * cc + 13 * oc + 4 * (oc + 1) + 8 * hc
    return up, down


def child(leg, n, reps, warmup):
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    base, problems = problems_of(n)
    if leg == "copy":
        import torch
        up, down = call_bytes(problems)
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
    arr, outs, keep = capi.pack_connections_problems(problems)
    if leg == "host":
        f = capi.lib().tc2li_host_update_connections_batch
        f.argtypes = [C.c_void_p, C.c_int]
        call = lambda: f(C.addressof(arr), n)
    else:
        f = capi.lib().tc2li_update_connections_batch
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
    res = dict(leg=leg, problems=n, ms=float(np.median(times)), min_ms=float(min(times)), max_ms=float(max(times)))
    if leg == "kernels":
        res["kernels_ms_per_call"] = {k: v[1] / v[0] for k, v in capi.profile_report().items() if k.startswith("k_conn")}
        capi.profile_enable(False)
    import connections_ref as ref
    want = [ref.update_connections(p) for p in base]
    for i in range(n):
        w, c = want[i % N_BASE], outs[i]["counts"]
        assert c[0] == w["status"] and np.array_equal(outs[i]["ordered_kf"][:c[2]], w["ordered_kf"]) and \
            np.array_equal(outs[i]["changed_kf"][:c[4]], w["changed_kf"]), i
    res.update(counted=float(np.mean([len(w["counter_kf"]) for w in want])), ordered=float(np.mean([len(w["ordered_kf"]) for w in want])),
               changed_entries=float(np.mean([len(w["changed_kf"]) for w in want])),
               votes=float(np.mean([int(w["counter_weight"].sum()) for w in want])))
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", type=int, default=512)
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
    print("%d problems (%.0f counted, %.0f ordered keyframes, %.0f votes, %.0f entries in the changed lists each): device call %.2f ms "
          "(%.2f-%.2f), host entry %.2f ms (%.2f-%.2f); upload %.1f MB %.2f ms, download %.1f MB %.2f ms; kernels per call %s"
          % (a.problems, d["counted"], d["ordered"], d["votes"], d["changed_entries"], d["ms"], d["min_ms"], d["max_ms"], h["ms"], h["min_ms"], h["max_ms"],
             c["upload_bytes"] / 1e6, c["upload_ms"], c["download_bytes"] / 1e6, c["download_ms"],
             ", ".join("%s %.3f ms" % kv for kv in sorted(rows["kernels"]["kernels_ms_per_call"].items()))))
    if a.json:
        json.dump(dict(reps=a.reps, warmup=a.warmup, **rows), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
