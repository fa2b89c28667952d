"""Timings of LocalMapping::SearchInNeighbors for many sequences: one tc2li_search_in_neighbors_batch call beside the host twin
tc2li_host_search_in_neighbors_batch on the same problems.  The problems are random graphs at the reference's sizes: 45 keyframes of about
2 000 keypoints, 2 600 locations each seen by two or three tracks (map points) with disjoint observers, a current keyframe with 8
first-ring neighbours of 6 neighbours each (30 to 60 targets); --base different graphs are repeated up to --problems, all on one keyframe
store.  Call times are host clocks around whole calls (validation, packing, upload, kernel, download, scatter); the Python binding's
packing of the problem structures is outside the clock.  Median of --reps after --warmup calls.  The shares of upload, kernel and download come from
tc2li_profile_report in a separate call with profiling on (the entry brackets its two copies with events as the launches are); what
remains of that call is the host's validation, packing and scatter.  Every leg runs in a child process of its own under a time limit, so that a hang ends that
step and nothing more is started on the GPU after it.

    python tools/time_search_in_neighbors.py [--problems 64,512] [--base 4] [--reps 10] [--warmup 3] [--legs device,kernel,host] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(HERE, "tests"))
sys.path.insert(0, HERE)

KEYFRAMES, LOCATIONS = 45, 2600
LEGS = ("device", "kernel", "host")


def big_case(env, seed, n_kf=KEYFRAMES, n_loc=LOCATIONS):
    """-> (problem on local rows, views): the random graph of tests/search_in_neighbors_cases.py at the reference's sizes, vectorised"""
    import mapping_cases as mc
    import search_in_neighbors_cases as sc
    g = sc.Graph(env, "rotated", n_kf, seed=seed)   # the poses
    rng = np.random.default_rng(seed)
    uv0 = np.stack([rng.uniform(130, 660, n_loc), rng.uniform(45, 250, n_loc)], 1)
    z = rng.uniform(7.0, 11.0, n_loc)
    level = rng.integers(1, 5, n_loc)
    R0, t0 = g.poses[0]
    xc = np.stack([(uv0[:, 0] - env.cx) * z / env.fx, (uv0[:, 1] - env.cy) * z / env.fy, z], 1)
    X = ((xc - t0) @ R0).astype(np.float32)
    X64 = X.astype(np.float64)
    PO = X64 - mc.centre(g.poses[0])
    dist = np.linalg.norm(PO, axis=1)
    max_raw = (dist * 1.2 ** (level - 0.5)).astype(np.float32)
    base = rng.integers(0, 256, (n_loc, 32), dtype=np.uint8)
    views, loc_of, kp_of = [], [], np.full((n_kf, n_loc), -1, np.int64)
    for kf in range(n_kf):
        R, t = g.poses[kf]
        pc = X64 @ R.T + t
        u, v = env.fx * pc[:, 0] / pc[:, 2] + env.cx, env.fy * pc[:, 1] / pc[:, 2] + env.cy
        seen = np.nonzero((rng.random(n_loc) < 0.75) & (u > 8) & (u < 792) & (v > 8) & (v < 292))[0]
        n = len(seen)
        d = np.linalg.norm(X64[seen] - mc.centre(g.poses[kf]), axis=1)
        octave = np.clip(np.ceil(np.log(max_raw[seen] / d) / env.logsf), 0, 7).astype(np.int32)
        keys = np.zeros(n, mc.KP)
        keys["x"], keys["y"], keys["size"], keys["response"], keys["octave"] = u[seen], v[seen], 31.0, 1.0, octave
        stereo = rng.random(n) < 0.7
        bits = np.unpackbits(base[seen], axis=1)
        flips, where = rng.integers(0, 13, n), rng.integers(0, 256, (n, 12))
        for j in range(12):
            rows = np.nonzero(flips > j)[0]
            bits[rows, where[rows, j]] ^= 1
        views.append(dict(keys=keys, descriptors=np.packbits(bits, axis=1), u_right=np.where(stereo, u[seen] - env.bf / pc[seen, 2], -1.0).astype(np.float32),
                          depth=np.where(stereo, pc[seen, 2], -1.0).astype(np.float32), has_point=np.zeros(n, np.uint8), fv_node=np.zeros(1, np.int32),
                          fv_offset=np.array([0, n], np.int32), fv_index=np.arange(n, dtype=np.int32), pose7=g.poses7[kf]))
        kp_of[kf, seen] = np.arange(n)
    owner = rng.integers(0, 4, (n_kf, n_loc))
    kf_i, loc_i = np.nonzero((kp_of >= 0) & (owner < 3))
    track = loc_i * 3 + owner[kf_i, loc_i]
    ids, point = np.unique(track, return_inverse=True)
    order = np.lexsort((kf_i, point))
    kf_i, loc_i, point = kf_i[order], loc_i[order], point[order]
    idx = kp_of[kf_i, loc_i]
    n_points = len(ids)
    obs_offsets = np.concatenate([[0], np.cumsum(np.bincount(point, minlength=n_points))]).astype(np.int32)
    n_kp = np.array([len(v["keys"]) for v in views])
    so = np.concatenate([[0], np.cumsum(n_kp)]).astype(np.int32)
    slot_point = np.full(int(so[-1]), -1, np.int32)
    slot_point[so[kf_i] + idx] = point
    first = obs_offsets[:-1]
    loc_p = ids // 3
    pts = np.zeros(n_points, mc.MP)
    pts["pos"], pts["normal"] = X[loc_p], (PO[loc_p] / dist[loc_p, None]).astype(np.float32)
    pts["min_distance"], pts["max_distance"], pts["max_distance_raw"] = (0.5 * dist[loc_p]).astype(np.float32), (2 * dist[loc_p]).astype(np.float32), max_raw[loc_p]
    weight = np.array([2 if views[k]["u_right"][i] >= 0 else 1 for k, i in zip(kf_i, idx)], np.int32)
    pts["descriptor"] = np.array([views[kf_i[o]]["descriptors"][idx[o]] for o in first], np.uint8)
    others = np.arange(1, n_kf)
    covis = [[] for _ in range(n_kf)]
    covis[0] = [int(k) for k in rng.permutation(others)[:8]]
    for k in covis[0]:
        covis[k] = [int(j) for j in rng.permutation(n_kf)[:6]]
    pr = dict(kf_slot=np.arange(n_kf, dtype=np.int32), kf_flags=np.zeros(n_kf, np.uint8), prev_kf=np.full(n_kf, -1, np.int32), poses7=np.array(g.poses7, np.float32),
              covis_offsets=np.concatenate([[0], np.cumsum([len(c) for c in covis])]).astype(np.int32), covis=np.array([k for c in covis for k in c], np.int32),
              slot_offsets=so, slot_point=slot_point, points=pts, point_flags=np.zeros(n_points, np.uint8),
              point_nobs=np.add.reduceat(weight, first).astype(np.int32), point_found=np.ones(n_points, np.int32), point_visible=np.full(n_points, 2, np.int32),
              point_ref_kf=kf_i[first].astype(np.int32), point_ref_level_scale=env.sf[[views[kf_i[o]]["keys"]["octave"][idx[o]] for o in first]].astype(np.float32),
              obs_offsets=obs_offsets, obs_kf=kf_i.astype(np.int32), obs_index=idx.astype(np.int32), current=0, inertial=False, abort=False,
              last_level_scale=float(env.sf[-1]))
    return pr, views


def timed(call, reps, warmup):
    for _ in range(warmup):                                  # buffers, pools, clocks
        call()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        call()
        times.append((time.perf_counter() - t) * 1e3)
    return dict(ms=float(np.median(times)), min_ms=float(min(times)), max_ms=float(max(times)))


def child(leg, n, n_base, reps, warmup):
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    from tc2li_slam_amd import synthetic
    import search_in_neighbors_cases as sc
    env = sc.env_of(synthetic)
    bases = [big_case(env, 900 + i) for i in range(n_base)]
    views, problems = [], []
    for pr, v in bases:
        pr["kf_slot"] = (pr["kf_slot"] + len(views)).astype(np.int32)
        views += v
    problems = [bases[i % n_base][0] for i in range(n)]
    res = dict(leg=leg, problems=n, keyframes=KEYFRAMES, keypoints=int(np.mean([len(v["keys"]) for v in views])), points=int(np.mean([len(p["points"]) for p, _ in bases])))
    # capacities once, from a host run of the base problems
    sized = capi.search_in_neighbors_batch([p for p, _ in bases], env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=sc.mc.BOUNDS0)
    res["targets"] = [int(r["counts"]["targets"]) for r in sized]
    res["ops"] = [int(r["counts"]["ops"]) for r in sized]
    caps = [dict(targets=210, candidates=len(bases[i % n_base][0]["points"]), ops=sized[i % n_base]["counts"]["ops"] + 8,
                 observations=sized[i % n_base]["counts"]["observations"] + 8) for i in range(n)]
    arr, outs, keep = capi.pack_neighbors_problems(problems, caps)
    if leg == "host":
        call = lambda: capi.run_search_in_neighbors_batch(arr, n, env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=sc.mc.BOUNDS0)
        assert call() == n
        res.update(timed(call, reps, warmup), host_threads=capi.host_threads())
    else:
        store = capi.KeyframeStore(len(views), 3072)
        store.put_batch(np.arange(len(views)), views, sc.mc.BOUNDS0)
        call = lambda: capi.run_search_in_neighbors_batch(arr, n, env.cam4, env.bf, env.sf, env.isg, env.logsf, store=store)
        assert call() == n, capi.lib().tc2li_last_error()
        res["on_host"] = int(sum(int(o["counts"][0]) for o in outs))
        if leg == "device":
            res.update(timed(call, reps, warmup))
        else:
            for _ in range(warmup):
                call()
            capi.profile_enable(True)
            capi.profile_report()
            t = time.perf_counter()
            call()
            res["ms"] = (time.perf_counter() - t) * 1e3
            res["kernels"] = {k: v for k, v in capi.profile_report().items()}
            capi.profile_enable(False)
            part = lambda head: float(sum(v[1] for k, v in res["kernels"].items() if k.startswith(head)))
            res["upload_ms"], res["kernel_ms"], res["download_ms"] = part("upload"), part("k_"), part("download")
            res["host_ms"] = res["ms"] - res["upload_ms"] - res["kernel_ms"] - res["download_ms"]   # validation, packing, scatter
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="64,512")
    ap.add_argument("--base", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS))
    ap.add_argument("--limit", type=int, default=240, help="seconds per leg")
    ap.add_argument("--json")
    ap.add_argument("--child", nargs=2)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.base, a.reps, a.warmup)
    results = []
    for n in [int(v) for v in a.problems.split(",")]:
        for leg in a.legs.split(","):
            try:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", leg, str(n), "--base", str(a.base), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                                   capture_output=True, text=True, timeout=None if a.limit <= 0 else a.limit)
            except subprocess.TimeoutExpired:
                print("leg %s with %d problems passed its time limit of %d s; stopping" % (leg, n, a.limit))
                return 1
            if r.returncode != 0:   # a fault, an abort or a hang: nothing more is started on the GPU
                print(r.stdout[-2000:] + r.stderr[-2000:])
                print("leg %s with %d problems ended with status %d; stopping" % (leg, n, r.returncode))
                return 1
            for line in r.stdout.splitlines():
                if line.startswith("RESULT "):
                    results.append(json.loads(line[7:]))
                    print(line[7:], flush=True)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        json.dump(results, open(a.json, "w"), indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
