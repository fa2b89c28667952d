"""Timings of the local BA from the flat graph, three ways, for a batch of windows of the size synthetic.ba_window_varied draws (seeds 0-15,
taken --problems / 16 times each; their flat graphs from tests/ba_window_cases.py from_window):
    host    tc2li_host_ba_window_batch + tc2li_local_bundle_adjustment_batch_group + tc2li_ba_window_outliers per window
    device  the same with tc2li_ba_window_batch as the gather
    solve   tc2li_ba_window_solve_batch: one call, the windows stay on the device in between (edges, chi2 and depth flags not asked for)
Per leg: wall time of the whole sequence and CPU seconds of the process (all threads), median and range of --reps after --warmup calls; the
Python binding's packing of the problem structures is outside the clock.  Every leg runs in a child process of its own under a time limit, so
that a hang ends that step and nothing more is started on the GPU after it.  The kernels leg repeats the solve calls with
tc2li_profile_enable(1) and prints the k_bas_*, k_baw_* and k_window_* times of tc2li_profile_report.  The solve leg also checks its poses, points and
outlier pairs against the device leg's arithmetic (the same calls through the Python wrappers) for the first four windows, byte for byte.

    python tools/time_ba_window_solve.py [--problems 64] [--reps 20] [--warmup 3] [--json out.json]
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

N_BASE, GROUP = 16, 0


def windows_of(n):
    """N_BASE windows, each with slots of its own in one store table -> (views, the n problem dicts with their clouds, sigma, cam)"""
    import ba_window_cases as K
    from tc2li_slam_amd import synthetic
    views, base, sigma, cam = [], [], None, None
    for i in range(N_BASE):
        w = synthetic.ba_window_varied(seed=i)
        v, pr, sigma = K.from_window(w)
        pr["kf_slot"] = pr["kf_slot"] + len(views)
        pr.update(iterations=int(w["iterations"]))
        if len(w["win_pose"]):
            rows = [int(k) for k in w["win_pose"]]
            pr.update(clouds=[w["clouds"][rows.index(k)] if k in rows else None for k in range(len(w["poses"]))], Tcl7=synthetic.TCL7, weight=float(w["weight"]))
        views += v
        base.append(pr)
        cam = np.asarray(w["cam"], np.float64)
    return views, [base[i % N_BASE] for i in range(n)], sigma, cam


def moved_bytes(problems, counts, leg):
    """(up, down) bytes of one sequence: the flat graph / the window lists and the BA's input blocks and results (without paddings)"""
    up = down = 0
    for p, c in zip(problems, counts):
        nk, ns, nc, npt, no = len(p["kf_slot"]), len(p["slot_point"]), len(p["cov_kf"]), len(p["point_flags"]), len(p["obs_kf"])
        K_, P, E = int(c[3]), int(c[4]), int(c[5])
        graph = 80 + 73 * nk + 4 * (nk + 1) + 4 * ns + 4 * nc + 25 * npt + 4 * (npt + 1) + 8 * no
        lists = 32 + 24 + 61 * K_ + 28 * P
        block = 56 * K_ + 24 * P + 40 * E + 4 * K_ + 4 * (P + 1) + 4 * E + 8 * P + 16 * E + 8 * P   # poses, points, edges, the index structure (about)
        results = 56 * K_ + 24 * P
        if leg == "host":
            up, down = up + block, down + results + 9 * E
        elif leg == "device":
            up, down = up + graph + block, down + lists + 40 * E + results + 9 * E
        else:
            up, down = up + graph, down + lists + 4 * K_ + 32 + results
    return up, down


def child(leg, n, reps, warmup):
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    import ba_window_cases as K
    views, problems, sigma, cam = windows_of(n)
    sg = np.ascontiguousarray(sigma, np.float32)
    store = None
    if leg != "host":
        store = pkg.KeyframeStore(len(views), max(len(v["keys"]) for v in views))
        store.put_batch(list(range(len(views))), views, K.BOUNDS, n_levels=K.N_LEVELS)
    if leg in ("host", "device"):
        arr, outs, keep = capi.pack_ba_window_problems(problems)
        if leg == "host":
            varr, vkeep = capi._pack_ba_window_views(views)
            g = capi.lib().tc2li_host_ba_window_batch
            g.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
            gather = lambda: g(C.addressof(varr), len(views), C.addressof(arr), n, sg.ctypes.data, len(sg))
        else:
            g = capi.lib().tc2li_ba_window_batch
            g.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
            gather = lambda: g(store._handle(), C.addressof(arr), n, sg.ctypes.data, len(sg), None)
        assert gather() == n, capi.lib().tc2li_last_error()
        counts = [o["counts"].copy() for o in outs]
        # the BA's problems point at the gather's output arrays: what the shim hands over
        ba = (capi.BaProblem * n)()
        stats, lstats = (capi.BaStats * n)(), (capi.LidarBaStats * n)()
        results = np.zeros(n, np.int32)
        extra = []
        for i, (p, o, c) in enumerate(zip(problems, outs, counts)):
            E = int(c[5])
            chi2, dpos, bad = np.zeros(max(E, 1)), np.zeros(max(E, 1), np.uint8), np.zeros(max(int(c[4]), 1), np.uint8)
            ep, et = np.zeros(max(E, 1), np.int32), np.zeros(max(E, 1), np.int32)
            lw = None
            if p.get("clouds") is not None and c[6]:
                idx = o["lidar_pose_index"][:c[6]]
                lw = capi._pack_lidar_window(idx, [p["clouds"][o["pose_row"][k]] for k in idx], p["Tcl7"], p["weight"])
            extra.append((chi2, dpos, bad, ep, et, lw))
            ba[i] = capi.BaProblem(o["poses7_out"].ctypes.data, o["fixed"].ctypes.data, o["points3_out"].ctypes.data, o["edges"].ctypes.data, int(c[3]), int(c[4]), E,
                                   int(p["iterations"]), 0.0, None, chi2.ctypes.data, dpos.ctypes.data, C.addressof(stats) + i * C.sizeof(capi.BaStats),
                                   C.addressof(lw[0]) if lw else None, C.addressof(lstats) + i * C.sizeof(capi.LidarBaStats))
        b = capi.lib().tc2li_local_bundle_adjustment_batch_group
        b.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        r = capi.lib().tc2li_ba_window_outliers
        r.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]

        def call():
            assert gather() == n
            assert b(C.addressof(ba), n, cam.ctypes.data, GROUP, results.ctypes.data) == n, capi.lib().tc2li_last_error()
            for i in range(n):
                chi2, dpos, bad, ep, et, _ = extra[i]
                E = int(counts[i][5])
                assert r(outs[i]["edges"].ctypes.data, chi2.ctypes.data, dpos.ctypes.data, E, bad.ctypes.data, int(counts[i][4]), ep.ctypes.data, et.ctypes.data, E) >= 0
    else:
        arr, outs, keep = capi.pack_ba_window_solve_problems([dict(p, want_edges=False, want_chi2=False) for p in problems])
        results = np.zeros(n, np.int32)
        f = capi.lib().tc2li_ba_window_solve_batch
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]

        def call():
            assert f(store._handle(), C.addressof(arr), n, sg.ctypes.data, len(sg), cam.ctypes.data, GROUP, results.ctypes.data) == n, capi.lib().tc2li_last_error()
    for _ in range(warmup):                                  # buffers, pools, clocks
        call()
    if leg == "kernels":
        capi.profile_enable(True)
        capi.profile_report()
    wall, cpu = [], []
    for _ in range(reps):
        c0, t0 = time.process_time(), time.perf_counter()
        call()
        wall.append((time.perf_counter() - t0) * 1e3)
        cpu.append((time.process_time() - c0) * 1e3)
    res = dict(leg=leg, problems=n, ms=float(np.median(wall)), min_ms=float(min(wall)), max_ms=float(max(wall)), cpu_ms=float(np.median(cpu)),
               cpu_min_ms=float(min(cpu)), cpu_max_ms=float(max(cpu)), iterations=[int(v) for v in results[:N_BASE]])
    if leg == "kernels":
        res["kernels_ms_per_call"] = {k: v[1] / reps for k, v in capi.profile_report().items() if k.startswith(("k_bas", "k_baw", "k_window"))}
        capi.profile_enable(False)
    counts = [o["counts"].copy() for o in outs]
    up, down = moved_bytes(problems, counts, "solve" if leg == "kernels" else leg)
    res.update(upload_bytes=int(up), download_bytes=int(down))
    if leg == "solve":                                       # the same arithmetic as the three calls: four windows, byte for byte
        first = problems[:4]
        g = capi.ba_window_batch(first, sigma, store=store)
        wins = []
        for p, w in zip(first, g):
            d = dict(poses=w["poses7"], fixed=w["fixed"], points=w["points3"], edges=w["edges"], iterations=p["iterations"])
            if p.get("clouds") is not None and w["n_lidar"]:
                d.update(win_pose=w["lidar_pose_index"], clouds=[p["clouds"][w["pose_row"][k]] for k in w["lidar_pose_index"]], Tcl7=p["Tcl7"], weight=p["weight"])
            wins.append(d)
        batch = capi.BaBatch(wins, cam)
        batch.run_group(GROUP)
        got = capi.ba_window_solve_batch(first, sigma, store, cam, group=GROUP)
        for i in range(4):
            poses, pts, chi2, dpos, _, _ = batch.result(i)
            assert got[i]["result"] == batch.results[i] and got[i]["poses7"].tobytes() == poses.tobytes() and got[i]["points3"].tobytes() == pts.tobytes(), i
            assert np.array_equal(got[i]["erase"], capi.ba_window_outliers(g[i]["edges"], chi2, dpos, np.zeros(len(pts), np.uint8))), i
        res["checked"] = 4
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
    ap.add_argument("--child", help="one leg in this process: host, device, solve or kernels")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.problems, a.reps, a.warmup)
        return
    rows = {}
    for leg in ("host", "device", "solve", "kernels"):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--problems", str(a.problems),
               "--reps", str(a.reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("the %s leg ended with status %d; nothing more is started\n%s" % (leg, r.returncode, r.stderr[-2000:]))
        rows[leg] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rows[leg]), flush=True)
    for leg in ("host", "device", "solve"):
        d = rows[leg]
        print("%-6s %d windows: %.2f ms (%.2f-%.2f), CPU %.1f ms (%.1f-%.1f); up %.1f MB, down %.1f MB"
              % (leg, a.problems, d["ms"], d["min_ms"], d["max_ms"], d["cpu_ms"], d["cpu_min_ms"], d["cpu_max_ms"], d["upload_bytes"] / 1e6, d["download_bytes"] / 1e6))
    print("kernels per solve call: " + ", ".join("%s %.3f ms" % kv for kv in sorted(rows["kernels"]["kernels_ms_per_call"].items())))
    if a.json:
        json.dump(dict(reps=a.reps, warmup=a.warmup, **rows), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
