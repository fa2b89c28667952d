"""Timings of LocalMapping::ProcessNewKeyFrame for many sequences: one tc2li_process_new_keyframe_batch call beside the host twin
tc2li_host_process_new_keyframe_batch on the same problems, host memory to host memory.  A problem is a keyframe of 1 200 keypoints with
about 1 000 occupied slots, 600 of them holding a point the keyframe does not observe yet (to associate) and 400 one it observes (recent),
every point with 3 to 20 observers among 29 other keyframes of 1 200 keypoints; --base different graphs are repeated up to --problems, all
on one keyframe store.  Call times are host clocks around whole calls (validation, packing, upload, kernels, download, scatter); the Python
binding's packing of the problem structures is outside the clock.  The two legs alternate call by call in one process, after --warmup
calls of each; median and range of --reps.  The shares of upload, kernels and download come from tc2li_profile_report in one more call with
profiling on (the entry brackets its two copies with events as the launches are).  The bytes of the two copies are the tables' sizes
(without the padding of each table to 256 bytes).  Every problem count runs in a child process of its own under a time limit, so that a
hang ends that step and nothing more is started on the GPU after it.

    python tools/time_process_new_keyframe.py [--problems 64,512] [--base 4] [--reps 10] [--warmup 3] [--json out.json]
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

KEYFRAMES, KEYPOINTS, OCCUPIED, TO_ASSOCIATE = 30, 1200, 1000, 600
BOUNDS = (0.0, 800.0, 0.0, 300.0)


def big_case(seed):
    """-> (problem on local rows, views)"""
    import mapping_cases as mc
    rng = np.random.default_rng(seed)
    views = []
    for kf in range(KEYFRAMES):
        keys = np.zeros(KEYPOINTS, mc.KP)
        k = np.arange(KEYPOINTS)
        keys["x"], keys["y"], keys["size"], keys["response"] = 10.0 + 12.0 * (k % 64), 10.0 + 14.0 * (k // 64), 31.0, 1.0
        stereo = rng.random(KEYPOINTS) < 0.7
        views.append(dict(keys=keys, descriptors=rng.integers(0, 256, (KEYPOINTS, 32), dtype=np.uint8), u_right=np.where(stereo, 5.0, -1.0).astype(np.float32),
                          depth=np.where(stereo, 4.0, -1.0).astype(np.float32), has_point=np.zeros(KEYPOINTS, np.uint8), fv_node=np.zeros(1, np.int32),
                          fv_offset=np.array([0, KEYPOINTS], np.int32), fv_index=np.arange(KEYPOINTS, dtype=np.int32), pose7=np.float32([0, 0, 0, 1, 0, 0, 0])))
    cur = KEYFRAMES // 2
    others = np.array([k for k in range(KEYFRAMES) if k != cur])
    slots = np.sort(rng.choice(KEYPOINTS, OCCUPIED, replace=False))
    slot_point = np.full(KEYPOINTS, -1, np.int32)
    slot_point[slots] = rng.permutation(OCCUPIED)
    obs_kf, obs_index, lens = [], [], []
    for p in range(OCCUPIED):
        seen_by = np.sort(rng.choice(others, int(rng.integers(3, 21)), replace=False))
        idx = rng.integers(0, KEYPOINTS, len(seen_by))
        if p >= TO_ASSOCIATE:                                   # observed on entry from its slot
            at = int(np.searchsorted(seen_by, cur))
            seen_by, idx = np.insert(seen_by, at, cur), np.insert(idx, at, int(np.flatnonzero(slot_point == p)[0]))
        obs_kf.append(seen_by); obs_index.append(idx); lens.append(len(seen_by))
    conn = [{int(j): int(rng.integers(1, 60)) for j in rng.choice(KEYFRAMES, 12, replace=False) if j != k} for k in range(KEYFRAMES)]
    first = [o[0] for o in obs_kf]
    pr = dict(kf_slot=np.arange(KEYFRAMES, dtype=np.int32), kf_flags=np.zeros(KEYFRAMES, np.uint8), centres=rng.uniform(-1, 1, (KEYFRAMES, 3)).astype(np.float32),
              conn_offsets=np.concatenate([[0], np.cumsum([len(c) for c in conn])]).astype(np.int32), conn_kf=np.array([k for c in conn for k in sorted(c)], np.int32),
              conn_weight=np.array([c[k] for c in conn for k in sorted(c)], np.int32), slot_point=slot_point, point_bad=np.zeros(OCCUPIED, np.uint8),
              positions=(rng.uniform(-4, 4, (OCCUPIED, 3)) + [0, 0, 12]).astype(np.float32), point_nobs=np.array(lens, np.int32),
              point_ref_kf=np.array(first, np.int32), point_ref_level_scale=np.full(OCCUPIED, 1.44, np.float32),
              obs_offsets=np.concatenate([[0], np.cumsum(lens)]).astype(np.int32), obs_kf=np.concatenate(obs_kf).astype(np.int32),
              obs_index=np.concatenate(obs_index).astype(np.int32), current=cur, last_level_scale=float(np.float32(1.2 ** 7)), first_connection=1, is_init_kf=0)
    return pr, views


def stats(times):
    return dict(ms=float(np.median(times)), min_ms=float(min(times)), max_ms=float(max(times)))


def child(n, n_base, reps, warmup):
    import tc2li_loader
    pkg = tc2li_loader.load()
    capi = pkg.capi
    bases = [big_case(700 + i) for i in range(n_base)]
    views = []
    for pr, v in bases:
        pr["kf_slot"] = (pr["kf_slot"] + len(views)).astype(np.int32)
        views += v
    problems = [bases[i % n_base][0] for i in range(n)]
    lite = [dict(descriptors=v["descriptors"], u_right=v["u_right"]) for v in views]
    arr, outs, keep = capi.pack_process_keyframe_problems(problems)
    res = dict(problems=n, keyframes=KEYFRAMES, keypoints=KEYPOINTS, occupied=OCCUPIED, host_threads=capi.host_threads())
    store = capi.KeyframeStore(len(views), KEYPOINTS)
    store.put_batch(np.arange(len(views)), views, BOUNDS)
    device = lambda: capi.run_process_new_keyframe_batch(arr, n, store=store)
    host = lambda: capi.run_process_new_keyframe_batch(arr, n, views=lite)
    assert device() == n, capi.lib().tc2li_last_error()
    res["on_host"] = int(sum(int(o["counts"][0]) for o in outs))
    res["associated"] = int(outs[0]["counts"][1]); res["recent"] = int(outs[0]["counts"][2]); res["observations_out"] = int(outs[0]["counts"][3])
    kept = [{k: np.array(v) for k, v in o.items()} for o in outs[:n_base]]
    assert host() == n
    for a, b in zip(kept, outs):                                # the two legs compute the same (the status aside)
        assert all(np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)) for k in a if k != "counts"), "device and host twin differ"
    for _ in range(warmup):                                     # buffers, pools, clocks
        device(); host()
    t_dev, t_host = [], []
    for _ in range(reps):                                       # the legs alternate
        t = time.perf_counter(); device(); t_dev.append((time.perf_counter() - t) * 1e3)
        t = time.perf_counter(); host(); t_host.append((time.perf_counter() - t) * 1e3)
    res["device"], res["host"] = stats(t_dev), stats(t_host)
    capi.profile_enable(True)
    capi.profile_report()
    t = time.perf_counter()
    device()
    res["profiled_ms"] = (time.perf_counter() - t) * 1e3
    res["kernels"] = {k: v for k, v in capi.profile_report().items()}
    capi.profile_enable(False)
    part = lambda head: float(sum(v[1] for k, v in res["kernels"].items() if k.startswith(head)))
    res["upload_ms"], res["kernel_ms"], res["download_ms"] = part("upload"), part("k_"), part("download")
    res["host_share_ms"] = res["profiled_ms"] - res["upload_ms"] - res["kernel_ms"] - res["download_ms"]   # validation, packing, scatter
    up = down = 0
    for pr, o in zip(problems, outs):
        nk, npts, ns, no, nc = len(pr["kf_flags"]), len(pr["point_bad"]), len(pr["slot_point"]), len(pr["obs_kf"]), len(pr["conn_kf"])
        occ = int((pr["slot_point"] >= 0).sum())
        up += 64 + 72 + 4 * len(o["ordered_kf"]) + 24 * nk + nk + 4 * (nk + 1) + 8 * nc + 4 * ns + npts * (1 + 12 + 4 + 4 + 4) + 4 * (npts + 1) + 8 * no
        down += 16 + 12 * occ + npts * (4 + 4 + 4 + 1 + 12 + 4 + 4) + 4 * (npts + 1) + 8 * (no + occ) + 32 + 8 * len(o["counter_kf"]) + 17 * len(o["ordered_kf"]) + \
            4 * (len(o["ordered_kf"]) + 1) + 8 * len(o["changed_kf"])
    res["upload_bytes"], res["download_bytes"] = int(up), int(down)
    del keep
    store.close()
    print("RESULT " + json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--problems", default="64,512")
    ap.add_argument("--base", type=int, default=4)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--limit", type=int, default=240, help="seconds per problem count")
    ap.add_argument("--json")
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.base, a.reps, a.warmup)
    results = []
    for n in [int(v) for v in a.problems.split(",")]:
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(n), "--base", str(a.base), "--reps", str(a.reps), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=None if a.limit <= 0 else a.limit)
        except subprocess.TimeoutExpired:
            print("%d problems passed the time limit of %d s; stopping" % (n, a.limit))
            return 1
        if r.returncode != 0:   # a fault, an abort or a hang: nothing more is started on the GPU
            print(r.stdout[-2000:] + r.stderr[-2000:])
            print("%d problems ended with status %d; stopping" % (n, r.returncode))
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
