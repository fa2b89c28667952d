"""Timings of local mapping's KeyFrameCulling: tc2li_keyframe_culling_batch for batches of generated problems (tests/culling_cases.py: K = 40
keyframes, P = 3000 points, runs of 5-9 keyframes, where culls cascade; and a sparse variant, runs of 2-3, where no keyframe is redundant)
beside the host entry tc2li_host_keyframe_culling_batch on the same problems.  Call times are host clocks around whole calls (validation,
concatenation, upload, two kernels, download); the Python binding's packing of the problem structures is outside the clock.  Median of
--reps after one warm-up.  Every size runs the device leg in a child process of its own under a time limit, so that a hang ends that step
and nothing more is started on the GPU after it.  Kernel times come from a rocprofv3 --kernel-trace --stats run of the child, summed per
kernel and grid by --summarize.

    python tools/time_culling.py [--sizes 64,512,1024] [--reps 5] [--json out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_culling.py --child dense,512 --reps 3 --no-host
    python tools/time_culling.py --summarize DIR/.../*_kernel_trace.csv profiles/culling_kernel_stats.csv
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

N_BASE = 16


def problems_of(kind, n):
    import culling_cases as K
    base = [K.make_problem(800 + i, 40, 3000, (5, 9), inertial=bool(i % 2), sparse=kind == "sparse") for i in range(N_BASE)]
    return base, [base[i % N_BASE] for i in range(n)]


def algorithmic_bytes(pr, want):
    """k_cull_count's byte count for one problem (csrc/culling_kernels.hip): per slot of a listed keyframe 4 + 4 + 1 B, per slot that passes
    the gates of :966-977 the point's 1 + 4 B and its observation row x (4 + 1 B).  Counted over every listed keyframe that is not skipped
    (the kernel also counts those after the break)."""
    so, oo = pr["slot_offsets"], pr["obs_offsets"]
    total = 0
    for kf in pr["local"]:
        if pr["kf_flags"][kf] & 3:
            continue
        s = slice(so[kf], so[kf + 1])
        p = pr["slot_point"][s]
        total += 9 * len(p)
        ok = p >= 0
        ok[ok] &= pr["point_bad"][p[ok]] == 0
        total += int(ok.sum())
        d = pr["slot_depth"][s]
        ok &= ~((d > pr["kf_th_depth"][kf]) | (d < 0))
        total += 4 * int(ok.sum())
        q = p[ok]
        q = q[pr["point_nobs"][q] > 3]
        total += 5 * int((oo[q + 1] - oo[q]).sum())
    return total


def child(kind, n, reps, host):
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    base, problems = problems_of(kind, n)
    arr, outs, keep = capi.pack_culling_problems(problems)
    if host:
        f = capi.lib().tc2li_host_keyframe_culling_batch
        f.argtypes = [C.c_void_p, C.c_int]
        call = lambda: f(C.addressof(arr), n)
    else:
        f = capi.lib().tc2li_keyframe_culling_batch
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        call = lambda: f(C.addressof(arr), n, None)
    assert call() == n, capi.lib().tc2li_last_error()      # warm-up: buffers, pools
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        rc = call()
        times.append((time.perf_counter() - t) * 1e3)
        assert rc == n
    import culling_ref as ref
    want = [ref.keyframe_culling(p) for p in base]
    for i in range(n):
        assert np.array_equal(outs[i]["verdict"], want[i % N_BASE]["verdict"]), i
    decided = sum(int((w["verdict"] >= 0).sum()) for w in want)
    print(json.dumps(dict(kind=kind, problems=n, host=host, ms=float(np.median(times)), all_ms=times,
                          culls_per_problem=sum(w["culled"] for w in want) / N_BASE, dirty_share=sum(int(w["dirty"].sum()) for w in want) / max(decided, 1),
                          count_bytes_per_problem=sum(algorithmic_bytes(p, w) for p, w in zip(base, want)) / N_BASE)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,512,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--json")
    ap.add_argument("--child", help="kind,problems: one leg in this process")
    ap.add_argument("--host", action="store_true", help="with --child: the host entry")
    ap.add_argument("--summarize", nargs=2, metavar=("TRACE_CSV", "OUT_CSV"))
    a = ap.parse_args()
    if a.summarize:
        from time_reloc import summarize
        summarize(*a.summarize)
        return
    if a.child:
        kind, n = a.child.split(",")
        child(kind, int(n), a.reps, a.host)
        return
    rows = []
    for kind in ("dense", "sparse"):
        for n in [int(s) for s in a.sizes.split(",")]:
            row = dict(kind=kind, problems=n)
            for host in ([False] if a.no_host else [False, True]):
                cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", "%s,%d" % (kind, n), "--reps", str(a.reps)]
                r = subprocess.run(cmd + (["--host"] if host else []), capture_output=True, text=True)
                if r.returncode != 0:
                    sys.exit("the %s leg of %s x %d ended with status %d; nothing more is started\n%s" % ("host" if host else "device", kind, n, r.returncode, r.stderr[-2000:]))
                out = json.loads(r.stdout.strip().splitlines()[-1])
                row["host_ms" if host else "device_ms"] = out["ms"]
                row.update({k: out[k] for k in ("culls_per_problem", "dirty_share", "count_bytes_per_problem")})
            rows.append(row)
            print("%-6s %5d problems: device call %.2f ms%s; %.1f culls per problem, %.0f %% of the decided keyframes dirty, k_cull_count %.0f KB per problem"
                  % (kind, n, row["device_ms"], "" if a.no_host else ", host entry %.2f ms" % row["host_ms"], row["culls_per_problem"], 100 * row["dirty_share"],
                     row["count_bytes_per_problem"] / 1e3), flush=True)
    if a.json:
        json.dump(dict(reps=a.reps, rows=rows), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
