#!/usr/bin/env python3
"""CreateNewMapPoints and the Fuse search of SearchInNeighbors for many sequences: the single-keyframe entries in a loop against the
keyframe store + the batch entries.  A tool beside bench.py (which it does not touch); it needs a GPU and fails without one.

Keyframes come from the product's own extractor and stereo matcher on `synthetic` scenes at the benched image size; every sequence
owns its slots in the store (the host arrays of a scene are shared between the sequences that tile it, the device copies are not).
Only the C entry points are timed: the ctypes tables of both paths are packed before the clock starts.  Every timed region ends in
the entry's own synchronise.  Both paths are run on the same inputs first and their results compared byte for byte.

Prints one JSON line: medians, min / max over the repetitions, host<->device bytes per step on each path (computed from the shapes,
as the host code moves them) and the launches per step (kernels + copies + fills, counted the same way)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def camera_position(k):
    return np.array([0.25 * k + 0.05 * np.sin(1.3 * k), 0.0, 0.45 * k])


def make_keyframes(pkg, synthetic, seed, n_kf, W, H, nfeatures):
    scene = synthetic.Scene(seed)
    rng = np.random.default_rng(100 + seed)
    el = pkg.OrbExtractor(nfeatures=nfeatures, max_width=W, max_height=H, max_images=1)
    er = pkg.OrbExtractor(nfeatures=nfeatures, max_width=W, max_height=H, max_images=1)
    bf = float(np.float32(synthetic.BF)); b = float(np.float32(synthetic.BF) / np.float32(synthetic.FX))
    kfs = []
    for k in range(n_kf):
        c = camera_position(k)
        left, _ = scene.render(c[0], W, H, noise_seed=2 * k + 1, cam_z=c[2])
        right, _ = scene.render(c[0] + synthetic.BASELINE, W, H, noise_seed=2 * k + 2, cam_z=c[2])
        _, keys, desc = el.extract(left)
        _, kr, dr = er.extract(right)
        keys, desc = keys.copy(), desc.copy()
        u_right, depth, _ = pkg.compute_stereo_matches(el, er, keys, desc, kr, dr, bf, b)
        n = len(keys)
        node = np.zeros(n, np.int32)
        for bit, byte in enumerate((0, 5, 9, 14, 21, 27, 3, 30)):  # 256 stand-in vocabulary nodes from descriptor bits
            node |= (desc[:, byte] & 1).astype(np.int32) << bit
        ids = np.unique(node)
        order = np.argsort(node, kind="stable")
        off = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=256)[ids])]).astype(np.int32)
        kfs.append(dict(keys=keys, descriptors=desc, u_right=u_right.astype(np.float32), depth=depth.astype(np.float32),
                        has_point=(rng.random(n) < 0.45).astype(np.uint8), fv_node=ids.astype(np.int32), fv_offset=off, fv_index=order.astype(np.int32),
                        pose7=np.concatenate([[0, 0, 0, 1], -c]).astype(np.float32), centre=c))
    return kfs


def map_points_of(pkg, kf, cam4, sf):
    sel = np.nonzero(kf["depth"] > 0)[0]
    z = kf["depth"][sel]
    Xc = np.stack([(kf["keys"]["x"][sel] - cam4[2]) * z / cam4[0], (kf["keys"]["y"][sel] - cam4[3]) * z / cam4[1], z], 1).astype(np.float32)
    Xw = (Xc + kf["centre"].astype(np.float32)).astype(np.float32)
    pts = np.zeros(len(sel), pkg.MAP_POINT_DTYPE)
    pts["pos"] = Xw
    v = Xw - kf["centre"].astype(np.float32)
    dist = np.linalg.norm(v, axis=1).astype(np.float32)
    pts["normal"] = v / dist[:, None]
    raw = (dist * sf[kf["keys"]["octave"][sel]]).astype(np.float32)
    pts["max_distance_raw"] = raw
    pts["max_distance"] = np.float32(1.2) * raw
    pts["min_distance"] = np.float32(0.8) * (raw / sf[-1])
    pts["descriptor"] = kf["descriptors"][sel]
    return pts


def kf_bytes(kf, with_has_point=True):
    n, nn, ne = len(kf["keys"]), len(kf["fv_node"]), len(kf["fv_index"])
    return (24 + 32 + 4 + 4 + (1 if with_has_point else 0)) * n + 4 * nn + 4 * (nn + 1) + 4 * ne


def spread(samples):
    s = sorted(samples)
    return dict(median_ms=1e3 * s[len(s) // 2], min_ms=1e3 * s[0], max_ms=1e3 * s[-1], reps=len(s))


def timed(fn, warmup, reps):
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return spread(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--problems", type=int, default=512, help="sequences: one CreateNewMapPoints problem and one Fuse step each")
    ap.add_argument("--neighbours", type=int, default=10)
    ap.add_argument("--fuse-targets", type=int, default=20)
    ap.add_argument("--unique", type=int, default=2, help="distinct scenes rendered, tiled over the sequences")
    ap.add_argument("--width", type=int, default=None)
    ap.add_argument("--height", type=int, default=None)
    ap.add_argument("--nfeatures", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--put-chunk", type=int, default=512, help="keyframes per put_batch call")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    a = ap.parse_args()

    import tc2li_loader
    pkg = tc2li_loader.load()
    if pkg.device_count() < 1:
        raise SystemExit("bench_mapping_batch needs a GPU")
    from tc2li_slam_amd import synthetic
    capi, L = pkg.capi, pkg.lib()
    W, H = a.width or synthetic.WIDTH, a.height or synthetic.HEIGHT
    P, NN, NT = a.problems, a.neighbours, a.fuse_targets
    per_seq = 1 + max(NN, NT)
    bf32 = np.float32(synthetic.BF)
    cam4, mbf, mb = np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY]), float(bf32), float(bf32 / np.float32(synthetic.FX))
    cam5 = np.float32([cam4[0], cam4[1], cam4[2], cam4[3], mbf]).astype(np.float64)
    sf = np.cumprod(np.concatenate([[np.float32(1)], np.full(7, np.float32(1.2))])).astype(np.float32)
    sg = (sf * sf).astype(np.float32)
    isg, logsf = (np.float32(1) / sg).astype(np.float32), float(np.log(np.float32(1.2)))
    # newest first: keyframe 0 of a scene is the current one, 1.. its neighbours / fuse targets
    scenes = [make_keyframes(pkg, synthetic, 5 + u, per_seq, W, H, a.nfeatures)[::-1] for u in range(a.unique)]
    max_kp = max(len(k["keys"]) for sc in scenes for k in sc)
    slot_of = lambda s, k: s * per_seq + k  # noqa: E731
    void = C.c_void_p

    # ---- the store: the one-off upload --------------------------------------------------------------------------------------------------
    t0 = time.perf_counter()
    store = pkg.KeyframeStore(P * per_seq, max_kp)
    t_create = time.perf_counter() - t0
    all_slots = [(s, k) for s in range(P) for k in range(per_seq)]
    t_put, put_bytes = 0.0, 0
    for at in range(0, len(all_slots), a.put_chunk):
        chunk = all_slots[at:at + a.put_chunk]
        t0 = time.perf_counter()
        store.put_batch([slot_of(s, k) for s, k in chunk], [scenes[s % a.unique][k] for s, k in chunk], (0.0, float(W), 0.0, float(H)))
        t_put += time.perf_counter() - t0
        put_bytes += sum(kf_bytes(scenes[s % a.unique][k], False) + 12 * len(scenes[s % a.unique][k]["keys"]) for s, k in chunk)

    # ---- CreateNewMapPoints -------------------------------------------------------------------------------------------------------------
    single_views = [capi.pack_keyframe_views(scenes[u][:1 + NN]) for u in range(a.unique)]  # (ctypes array, keep-alive) per scene
    caps = [len(scenes[s % a.unique][0]["keys"]) for s in range(P)]
    single_pts = (capi.NewMapPoint * max(caps))()
    f1 = L.tc2li_create_new_map_points
    f1.argtypes = [void, void, C.c_int, void, C.c_float, void, void, C.c_int, C.c_float, C.c_int, C.c_int, C.c_float, C.c_int, void, C.c_int, void]

    def single_one(s):
        arr = single_views[s % a.unique][0]
        return f1(C.addressof(arr), C.addressof(arr) + C.sizeof(capi.KeyframeView), NN, cam5.ctypes.data, mb, sf.ctypes.data, sg.ctypes.data, len(sf), 1.2, 0, 0,
                  0.0, 0, C.addressof(single_pts), caps[s], None)

    def single_loop():
        for s in range(P):
            if single_one(s) < 0:
                raise RuntimeError(L.tc2li_last_error().decode())

    problems = []
    for s in range(P):
        sc = scenes[s % a.unique]
        problems.append(dict(current=slot_of(s, 0), neighbours=[slot_of(s, 1 + j) for j in range(NN)], poses7=np.stack([k["pose7"] for k in sc[:1 + NN]]),
                             has_point=[k["has_point"] for k in sc[:1 + NN]]))
    parr, pkeep, _ = capi.pack_new_points_problems(store, problems)
    off = np.concatenate([[0], np.cumsum(caps)]).astype(np.int32)
    bpts = np.zeros(int(off[-1]), capi.NEW_MAP_POINT_DTYPE)
    bcnt = np.zeros(P, np.int32)
    f2 = L.tc2li_create_new_map_points_batch
    f2.argtypes = [void, void, C.c_int, void, C.c_float, void, void, C.c_int, C.c_float, void, void, void, void]

    def batch_call():
        rc = f2(store._handle(), C.addressof(parr), P, cam5.ctypes.data, mb, sf.ctypes.data, sg.ctypes.data, len(sf), 1.2, bpts.ctypes.data, off.ctypes.data,
                bcnt.ctypes.data, None)
        if rc < 0:
            raise RuntimeError(L.tc2li_last_error().decode())
        return rc

    # the same results on both paths (scene by scene: the sequences that tile a scene are identical)
    batch_call()
    for u in range(min(a.unique, P)):
        n = single_one(u)
        one = np.frombuffer(single_pts, capi.NEW_MAP_POINT_DTYPE, count=n)
        assert n == bcnt[u] and one.tobytes() == bpts[off[u]:off[u] + n].tobytes(), "batch and single call differ for sequence %d" % u
    points_per_problem = float(np.mean(bcnt))
    new_points = dict(single_loop=timed(single_loop, a.warmup, a.reps), batch=timed(batch_call, a.warmup, a.reps))
    n_of = lambda s, k: len(scenes[s % a.unique][k]["keys"])  # noqa: E731
    slots = sum(NN * n_of(s, 0) for s in range(P))
    new_points["h2d_bytes_single"] = sum(kf_bytes(scenes[s % a.unique][k]) for s in range(P) for k in range(1 + NN)) + P * (NN * 200 + 64)
    new_points["h2d_bytes_batch"] = sum(n_of(s, k) for s in range(P) for k in range(1 + NN)) + P * (NN * (200 + 8) + 304 + 16) + 64
    new_points["d2h_bytes_single"] = slots * (4 + 1 + 12)
    new_points["d2h_bytes_batch"] = 4 * P + 32 * int(off[-1])
    new_points["launches_single"] = P * (2 + 2 + 3 + 3 + (1 + NN) * 8)   # kernels, fills, table / level copies, downloads, keyframe uploads
    new_points["launches_batch"] = 3 + 2 + 1 + 1
    new_points["points_per_problem"] = points_per_problem

    # ---- Fuse, stage 1: the current keyframe's points into every target -----------------------------------------------------------------
    lists = [map_points_of(pkg, scenes[u][0], cam4, sf) for u in range(a.unique)]
    rng = np.random.default_rng(3)
    first_point, at = [], 0
    for s in range(P):
        first_point.append(at)
        at += len(lists[s % a.unique])
    points = np.concatenate([lists[s % a.unique] for s in range(P)])
    items, nv = [], 0
    for s in range(P):
        m = len(lists[s % a.unique])
        for t in range(NT):
            items.append(dict(keyframe=slot_of(s, 1 + t), first_point=first_point[s], first_valid=nv, n_points=m, pose7=scenes[s % a.unique][1 + t]["pose7"], th=3.0))
            nv += m
    valid = (rng.random(nv) < 0.85).astype(np.uint8)
    iarr = (capi.FuseItem * len(items))()
    for i, it in enumerate(items):
        iarr[i].keyframe, iarr[i].first_point, iarr[i].first_valid, iarr[i].n_points, iarr[i].th = it["keyframe"], it["first_point"], it["first_valid"], it["n_points"], it["th"]
        iarr[i].pose7 = (C.c_float * 7)(*[float(v) for v in it["pose7"]])
    bi, bd, nfused = np.zeros(nv, np.int32), np.zeros(nv, np.int32), np.zeros(len(items), np.int32)
    f4 = L.tc2li_fuse_search_batch
    f4.argtypes = [void, void, C.c_int, void, C.c_float, void, void, C.c_int, C.c_float, void, C.c_int, void, C.c_int, void, void, void, void]

    def fuse_batch():
        rc = f4(store._handle(), C.addressof(iarr), len(items), cam4.ctypes.data, mbf, sf.ctypes.data, isg.ctypes.data, len(sf), logsf, points.ctypes.data, len(points),
                valid.ctypes.data, nv, bi.ctypes.data, bd.ctypes.data, nfused.ctypes.data, None)
        if rc < 0:
            raise RuntimeError(L.tc2li_last_error().decode())

    fviews = [[capi.FrameView(k["keys"].ctypes.data, k["descriptors"].ctypes.data, k["u_right"].ctypes.data, None, len(k["keys"]), 0.0, float(W), 0.0, float(H))
               for k in sc] for sc in scenes]
    poses = [[np.ascontiguousarray(k["pose7"], np.float32) for k in sc] for sc in scenes]
    sbi, sbd = np.zeros(max(len(l) for l in lists), np.int32), np.zeros(max(len(l) for l in lists), np.int32)
    f3 = L.tc2li_fuse_search
    f3.argtypes = [void, void, void, C.c_float, void, void, C.c_int, C.c_float, void, void, C.c_int, C.c_float, void, void, void]

    def fuse_one(i):
        it = items[i]
        s, t = divmod(i, NT)
        u = s % a.unique
        return f3(C.addressof(fviews[u][1 + t]), poses[u][1 + t].ctypes.data, cam4.ctypes.data, mbf, sf.ctypes.data, isg.ctypes.data, len(sf), logsf,
                  points.ctypes.data + 68 * it["first_point"], valid.ctypes.data + it["first_valid"], it["n_points"], 3.0, sbi.ctypes.data, sbd.ctypes.data, None)

    def fuse_loop():
        for i in range(len(items)):
            if fuse_one(i) < 0:
                raise RuntimeError(L.tc2li_last_error().decode())

    fuse_batch()
    for i in list(range(min(NT, len(items)))) + [len(items) - 1]:
        n = fuse_one(i)
        r = slice(items[i]["first_valid"], items[i]["first_valid"] + items[i]["n_points"])
        assert n == nfused[i] and np.array_equal(sbi[:items[i]["n_points"]], bi[r]) and np.array_equal(sbd[:items[i]["n_points"]], bd[r]), "fuse item %d differs" % i
    fuse = dict(single_loop=timed(fuse_loop, a.warmup, a.reps), batch=timed(fuse_batch, a.warmup, a.reps))
    fuse["h2d_bytes_single"] = sum((24 + 12 + 4 + 32) * n_of(s, 1 + t) + 69 * len(lists[s % a.unique]) + 128 for s in range(P) for t in range(NT))
    fuse["h2d_bytes_batch"] = 68 * len(points) + nv + 192 * len(items) + 64
    fuse["d2h_bytes_single"] = fuse["d2h_bytes_batch"] = 8 * nv
    fuse["launches_single"] = len(items) * (2 + 1 + 9 + 2)   # grid + search kernels, one fill, uploads, downloads
    fuse["launches_batch"] = 1 + 1 + 1
    fuse["fused_per_item"] = float(np.mean(nfused))

    store.close()
    out = dict(tool="bench_mapping_batch", problems=P, neighbours=NN, fuse_targets=NT, image=[W, H], keypoints_per_keyframe=float(np.mean([len(k["keys"]) for sc in scenes for k in sc])),
               keyframes_stored=P * per_seq, store_create_ms=1e3 * t_create, store_put_ms=1e3 * t_put, store_put_bytes=put_bytes,
               create_new_map_points=new_points, fuse_stage1=fuse)
    m = new_points
    m["speedup_steady"] = m["single_loop"]["median_ms"] / m["batch"]["median_ms"]
    m["speedup_with_put"] = m["single_loop"]["median_ms"] / (m["batch"]["median_ms"] + 1e3 * t_put * (1 + NN) / per_seq)
    fuse["speedup_steady"] = fuse["single_loop"]["median_ms"] / fuse["batch"]["median_ms"]
    fuse["speedup_with_put"] = fuse["single_loop"]["median_ms"] / (fuse["batch"]["median_ms"] + 1e3 * t_put * NT / per_seq)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
