"""Timings of the local-BA gather from the resident map graph beside the gather from host arrays, for 512 sequences of the bundle
adjustment's own window shape (synthetic.ba_window: 10 free and 30 fixed keyframes, 2 000 points; 32 different windows, each sequence one
of them).  Two pairs of legs and a fifth:

    gather   tc2li_ba_window_batch on host arrays          against   tc2li_map_graph_apply_batch + tc2li_ba_window_graph_batch
    solve    tc2li_ba_window_solve_batch, edges == NULL     against   tc2li_map_graph_apply_batch + tc2li_ba_window_solve_graph_batch
    resident_commit   tc2li_map_graph_apply_batch of the delta WITHOUT its SET_POSE / SET_POSITION edits, then
                      tc2li_ba_window_solve_graph_commit_batch, which writes the BA's result into the resident tables itself.  Its graph
                      changes from cycle to cycle (the solved poses and points stay, the outlier pairs go), so from the second cycle on
                      its BA starts from a converged map: the mean iterations and trials of the last cycle are printed for every solve leg.

The delta of every apply is one keyframe's worth per sequence: one new keyframe row, 400 slots set and 400 observations added on it, 40
poses and 2 000 positions overwritten.  The host-array legs gather the graph as it was set (the resident one grows by a row per call; 400
observations in about 16 000).  Call times are host clocks around the library calls; the Python binding's packing of the problem structures
and of the logs is outside the clock.  Median, min and max of --reps after --warmup calls.  Every leg runs in a child process of its own
under a time limit, so that a hang ends that step and nothing more is started on the GPU after it.  Bytes: what each leg put on the bus,
host to device -- the tables and records of the host-array gather as csrc/window_gather_host.hpp lays them out (without the 256-byte
rounding), and tc2li_map_graph_info's counts for the resident legs.

    python tools/time_map_graph.py [--sequences 512] [--reps 10] [--warmup 2] [--solve-reps 3] [--json out.json]
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
N_SLOTS, N_OBS, N_POSES, N_POSITIONS = 400, 400, 40, 2000


def world(pkg):
    """32 windows behind one store -> (views, problems, sigma, cam)"""
    import ba_window_cases as K
    from tc2li_slam_amd import synthetic
    views, problems, sigma, cam = [], [], None, None
    for i in range(N_BASE):
        w = synthetic.ba_window(500 + i, n_opt=10, n_fix=30, n_points=2000, pose_noise=(0.1, 0.01))
        v, pr, sigma = K.from_window(w)
        problems.append(dict(pr, kf_slot=pr["kf_slot"] + len(views), iterations=5, want_edges=False, want_chi2=False))
        views += v
        cam = np.asarray(w["cam"], np.float64)
    return views, problems, sigma, cam


def delta_of(pr, n_keys, call, rng, with_results=True):
    """one keyframe's worth of edits for the graph of `pr` after `call` earlier ones -> (edits, values).  with_results: the BA's result
    sent back as SET_POSE / SET_POSITION edits, which a committing solve makes unnecessary."""
    import map_graph_cases as M
    L = M.Log(pr)
    for _ in range(call):                                                               # the rows the earlier calls appended
        L.kf_slot.append(0); L.n_slots.append(N_SLOTS)
    n_kf, n_pt, cur = len(pr["kf_slot"]), len(pr["point_flags"]), int(pr["current"])
    slot = int(pr["kf_slot"][cur])
    k = L.add_keyframe(slot, N_SLOTS, 10 ** 6 + call, 0, pr["poses7"][cur])
    pts = rng.choice(n_pt, min(N_OBS, n_pt), replace=False)
    for i, p in enumerate(pts):
        L.set_slot(k, i, int(p))
        L.add_observation(int(p), k, i % n_keys[slot])
    for r in rng.choice(n_kf, min(N_POSES, n_kf), replace=False) if with_results else ():
        L.set_pose(int(r), pr["poses7"][r])
    for p in rng.choice(n_pt, min(N_POSITIONS, n_pt), replace=False) if with_results else ():
        L.set_position(int(p), pr["positions"][p])
    return L.done()


def host_array_bytes(pkg, problems, n_levels):
    rec = pkg.map_graph_limits()["gather_record_bytes"]
    up = 4 * n_levels
    for p in problems:
        nk, npt, ns, no = len(p["kf_slot"]), len(p["point_flags"]), len(p["slot_point"]), len(p["obs_kf"])
        up += rec + nk * (8 + 4 + 1 + 56) + 4 * (nk + 1) + 4 * ns + npt * (1 + 24) + 4 * (npt + 1) + 8 * no + 4 * len(p["cov_kf"])
    return up


def child(leg, n, reps, warmup):
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    import ba_window_cases as K
    views, base, sigma, cam = world(pkg)
    sg = np.ascontiguousarray(sigma, np.float32)
    commit = leg == "resident_commit"
    solve, resident = leg.endswith("solve") or commit, leg.startswith("resident")
    calls = warmup + reps
    # room for what the resident graph grows to: every call's new keyframe sees 400 points and so becomes a fixed camera with 400 edges
    base = [dict(p, pose_capacity=len(p["kf_slot"]) + calls, edge_capacity=len(p["obs_kf"]) + N_OBS * calls, erase_capacity=len(p["obs_kf"]) + N_OBS * calls)
            for p in base]
    problems = [base[i % N_BASE] for i in range(n)]
    n_keys = [len(v["keys"]) for v in views]
    with pkg.KeyframeStore(len(views), max(n_keys)) as store:
        store.put_batch(list(range(len(views))), views, K.BOUNDS, n_levels=K.N_LEVELS)
        if solve:
            arr, outs, keep = capi.pack_ba_window_solve_problems(problems)
            results = np.zeros(n, np.int32)
        else:
            arr, outs, keep = capi.pack_ba_window_problems(problems)
        graph, deltas = None, []
        seq = np.arange(n, dtype=np.int32)
        if resident:
            for i in range(n):
                capi._without_tables(arr[i].window if solve else arr[i])
            nk, ns, npt, no = (max(len(p[k]) for p in base) for k in ("kf_slot", "slot_point", "point_flags", "obs_kf"))
            graph = pkg.ResidentMapGraph(store, n, [nk + calls, ns + N_SLOTS * calls, npt, no + N_OBS * calls])
            graph.set_batch(seq, problems)
            rng = np.random.default_rng(1)
            for c in range(calls):                                                      # the logs of every call, packed outside the clock
                per_base = [delta_of(p, n_keys, c, rng, with_results=not commit) for p in base]
                darr, dkeep = (capi.MapGraphDelta * n)(), per_base
                for i in range(n):
                    e, v = per_base[i % N_BASE]
                    darr[i].edits, darr[i].values, darr[i].sequence, darr[i].n_edits, darr[i].n_values = e.ctypes.data, v.ctypes.data, i, len(e), len(v)
                deltas.append((darr, dkeep))
        L = capi.lib()
        L.tc2li_map_graph_apply_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.tc2li_ba_window_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.tc2li_ba_window_graph_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.tc2li_ba_window_solve_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.tc2li_ba_window_solve_graph_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        L.tc2li_ba_window_solve_graph_commit_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                                               C.c_uint32, C.c_void_p]
        a, s, h = C.addressof(arr), store._handle(), graph._handle() if resident else None
        bytes_of_apply = [0]

        def call(c):
            t_apply = 0.0
            if resident:
                t = time.perf_counter()
                rc = L.tc2li_map_graph_apply_batch(h, C.addressof(deltas[c][0]), n, None)
                t_apply = (time.perf_counter() - t) * 1e3
                assert rc == n, (rc, L.tc2li_last_error())
                if commit and c == calls - 1:                                           # (the commit overwrites the counter; outside the clocks)
                    bytes_of_apply[0] = int(sum(graph.info(i)["apply_bytes"] for i in range(n)))
            t = time.perf_counter()
            if commit:
                rc = L.tc2li_ba_window_solve_graph_commit_batch(s, h, seq.ctypes.data, a, n, sg.ctypes.data, len(sg), cam.ctypes.data, 0, 0, results.ctypes.data)
            elif solve and resident:
                rc = L.tc2li_ba_window_solve_graph_batch(s, h, seq.ctypes.data, a, n, sg.ctypes.data, len(sg), cam.ctypes.data, 0, results.ctypes.data)
            elif solve:
                rc = L.tc2li_ba_window_solve_batch(s, a, n, sg.ctypes.data, len(sg), cam.ctypes.data, 0, results.ctypes.data)
            elif resident:
                rc = L.tc2li_ba_window_graph_batch(s, h, seq.ctypes.data, a, n, sg.ctypes.data, len(sg), None)
            else:
                rc = L.tc2li_ba_window_batch(s, a, n, sg.ctypes.data, len(sg), None)
            t_gather = (time.perf_counter() - t) * 1e3
            assert rc == n, (rc, L.tc2li_last_error())
            return t_apply, t_gather
        times = [call(c) for c in range(calls)][warmup:]
        total = [x + y for x, y in times]
        stat = lambda v: dict(ms=float(np.median(v)), min_ms=float(min(v)), max_ms=float(max(v)))
        res = dict(leg=leg, sequences=n, reps=reps, pair=stat(total), apply=stat([x for x, _ in times]), gather=stat([y for _, y in times]),
                   n_keyframes=float(np.mean([len(p["kf_slot"]) for p in base])), n_points=float(np.mean([len(p["point_flags"]) for p in base])),
                   n_observations=float(np.mean([len(p["obs_kf"]) for p in base])), windows_ok=int(sum(int(o["counts"][0]) == 0 for o in outs)))
        if solve:
            res.update(windows_solved=int((results > 0).sum()), iterations=float(np.mean([o["stats"].iterations for o in outs])),
                       trials=float(np.mean([o["stats"].trials for o in outs])), erase_pairs=float(np.mean([int(o["n_erase"][0]) for o in outs])))
        if resident:
            info = [graph.info(i) for i in range(n)]
            if commit:
                res.update(commit_bytes=int(sum(i["apply_bytes"] for i in info)), applies=int(info[0]["applies"]))
            res.update(apply_bytes=bytes_of_apply[0] if commit else int(sum(i["apply_bytes"] for i in info)), gather_bytes=int(info[0]["gather_bytes"]),
                       edits_per_sequence=float(np.mean([len(e) for e, _ in deltas[-1][1]])))
            graph.close()
        else:
            res.update(apply_bytes=0, gather_bytes=host_array_bytes(pkg, problems, len(sg)))
        del keep
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sequences", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--solve-reps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--legs", default="host_gather,resident_gather,host_solve,resident_solve")
    ap.add_argument("--json")
    ap.add_argument("--child", help="one leg in this process: host_gather, resident_gather, host_solve, resident_solve or resident_commit")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.sequences, a.reps, a.warmup)
        return
    rows = {}
    for leg in a.legs.split(","):
        reps = a.solve_reps if leg.endswith("solve") or leg == "resident_commit" else a.reps
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--sequences", str(a.sequences),
               "--reps", str(reps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("the %s leg ended with status %d; nothing more is started\n%s" % (leg, r.returncode, r.stderr[-3000:]))
        rows[leg] = json.loads(r.stdout.strip().splitlines()[-1])
        print(json.dumps(rows[leg]), flush=True)
    for kind in ("gather", "solve"):
        if "host_" + kind in rows and "resident_" + kind in rows:
            b, r = rows["host_" + kind], rows["resident_" + kind]
            print("%s, %d sequences: host arrays %.2f ms (%.2f-%.2f), %.1f MB up; resident apply %.2f + %s %.2f = %.2f ms (%.2f-%.2f), %.2f + %.3f MB up"
                  % (kind, b["sequences"], b["pair"]["ms"], b["pair"]["min_ms"], b["pair"]["max_ms"], b["gather_bytes"] / 1e6, r["apply"]["ms"], kind,
                     r["gather"]["ms"], r["pair"]["ms"], r["pair"]["min_ms"], r["pair"]["max_ms"], r["apply_bytes"] / 1e6, r["gather_bytes"] / 1e6))
    if "resident_commit" in rows:
        r = rows["resident_commit"]
        print("committed cycle, %d sequences: apply %.2f + solve and commit %.2f = %.2f ms (%.2f-%.2f), %.2f + %.3f + %.3f MB up (apply, gather, commit); %.1f iterations, %.1f trials, %.1f erase pairs per window"
              % (r["sequences"], r["apply"]["ms"], r["gather"]["ms"], r["pair"]["ms"], r["pair"]["min_ms"], r["pair"]["max_ms"], r["apply_bytes"] / 1e6, r["gather_bytes"] / 1e6,
                 r["commit_bytes"] / 1e6, r["iterations"], r["trials"], r["erase_pairs"]))
    if a.json:
        json.dump(rows, open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
