"""Timings of the PnP stage of relocalisation: tc2li_mlpnp_ransac_batch for batches of problems of 100 matches whose solvers run all 35
iterations of their first call (70 % gross outliers: no iteration reaches min_inliers, so none returns early), beside the host entry
tc2li_host_mlpnp_ransac_batch on the same problems.  Call times are host clocks around whole calls (packing, draws, upload, three kernels,
download); the Python binding's own packing of the problem structures is outside the clock.  Kernel times come from a rocprofv3
--kernel-trace --stats run of this script, summed per kernel and grid by --summarize.

    python tools/time_mlpnp.py [--sizes 512,2048] [--matches 100] [--reps 5] [--json out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_mlpnp.py --reps 3 --no-host
    python tools/time_mlpnp.py --summarize DIR/.../*_kernel_trace.csv profiles/mlpnp_kernel_stats.csv
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def build_call(pkg, capi, problems, level_sigma2, cam5, host):
    """The ctypes call of capi.mlpnp_ransac_batch with everything packed beforehand -> a function that resets the states and calls."""
    P = len(problems)
    cap = max(len(p["keys"]) for p in problems)
    arr, states, keep = (capi.MlpnpProblem * P)(), (capi.MlpnpState * P)(), []
    best = np.zeros((P, cap), np.uint8)
    for i, p in enumerate(problems):
        keys, match = np.ascontiguousarray(p["keys"], capi.KEYPOINT_DTYPE), np.ascontiguousarray(p["match"], np.int32)
        xw, draws = np.ascontiguousarray(p["Xw"], np.float32), np.ascontiguousarray(p["draws"], np.uint32)
        keep.append((keys, match, xw, draws))
        arr[i].keys, arr[i].match, arr[i].Xw, arr[i].draws = keys.ctypes.data, match.ctypes.data, xw.ctypes.data, draws.ctypes.data
        arr[i].state, arr[i].best_inlier = C.addressof(states[i]), best[i].ctypes.data
        arr[i].n_keypoints, arr[i].n_points, arr[i].n_draws, arr[i].n_iterations = len(keys), len(xw), len(draws), 5
    params = capi.mlpnp_params()
    sig, cam = np.ascontiguousarray(level_sigma2, np.float32), np.ascontiguousarray(cam5, np.float64)
    out = [np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros(P, np.int32), np.zeros((P, 7), np.float32), np.zeros((P, 12)), np.zeros((P, cap), np.uint8)]
    f = capi.lib().tc2li_host_mlpnp_ransac_batch if host else capi.lib().tc2li_mlpnp_ransac_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_int] + ([] if host else [C.c_void_p])
    args = [C.addressof(arr), P, C.addressof(params), sig.ctypes.data, len(sig), cam.ctypes.data] + [o.ctypes.data for o in out] + [cap] + ([] if host else [None])

    def call():
        C.memset(states, 0, C.sizeof(states))
        best[:] = 0
        rc = f(*args)
        assert rc == P, (rc, capi.lib().tc2li_last_error())
        return states, out, (keep, params, sig, cam, arr)
    return call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,2048")
    ap.add_argument("--matches", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json")
    ap.add_argument("--summarize", nargs=2, metavar=("TRACE_CSV", "OUT_CSV"))
    a = ap.parse_args()
    if a.summarize:
        from time_reloc import summarize
        summarize(*a.summarize)
        return
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    import mlpnp_cases as K
    result = dict(matches=a.matches, reps=a.reps, rows=[])
    base = [K.make_problem(900 + i, a.matches, 0.7, 0.3, n_draws=6 * 35) for i in range(64)]
    for n in [int(s) for s in a.sizes.split(",")]:
        problems = [base[i % len(base)] for i in range(n)]
        row = dict(problems=n)
        for host in ([False] if a.no_host else [False, True]):
            call = build_call(pkg, capi, problems, K.LEVEL_SIGMA2, K.CAM5, host)
            states, out, _ = call()      # warm-up: buffers, pools
            assert all(states[i].iterations == 35 for i in range(n)), "every solver must run its 35 iterations"
            times = []
            for _ in range(a.reps):
                t = time.perf_counter()
                call()
                times.append((time.perf_counter() - t) * 1e3)
            row["host_ms" if host else "device_ms"] = float(np.median(times))
            row["host_all" if host else "device_all"] = times
        row["solves"] = 35 * n
        result["rows"].append(row)
        print("%5d problems x %d matches x 35 iterations: device call %.2f ms%s" % (
            n, a.matches, row["device_ms"], "" if a.no_host else ", host entry %.1f ms" % row["host_ms"]))
    if a.json:
        json.dump(result, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
