"""Timings of relocalisation's database query on the GPU: tc2li_detect_relocalization_candidates_batch for batches of queries, each against
its own database of 256 / 1 024 / 4 096 keyframes of about 1 000 words (keyframes drawn around a few "places", so that the word gate
passes a realistic share of them), tc2li_vocabulary_score_batch on the same vectors, and tc2li_relocalization_refine_batch for 512
hypotheses beside tc2li_track_reference_keyframe_batch for the same 512 frames.  Call times are host clocks around calls that end
in a device synchronisation (they include the uploads of the frames' BowVectors and the downloads of the results); kernel times come from
a rocprofv3 --kernel-trace --stats run of this script, summed per kernel and grid by --summarize.

    python tools/time_reloc.py [--sizes 256:512,1024:512,4096:128] [--reps 5] [--json out.json]
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/time_reloc.py --reps 3
    python tools/time_reloc.py --summarize DIR/.../*_kernel_trace.csv profiles/reloc_kernel_stats.csv
"""
import argparse
import csv
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_VOC = 10 ** 6  # word ids of a k = 10, L = 6 vocabulary


def summarize(trace_csv, out_csv):
    """Sums a rocprofv3 kernel trace per (kernel, grid): Name, BlocksX, GridY, Calls, TotalDurationNs, AverageNs, MinNs, MaxNs."""
    groups = {}
    for r in csv.DictReader(open(trace_csv)):
        name = r["Kernel_Name"].replace("(anonymous namespace)::", "").split("(")[0]
        if "tc2li::" not in name:
            continue
        name = "tc2li::" + name.split("tc2li::")[-1]
        wx = max(int(r.get("Workgroup_Size_X", r.get("Workgroup_Size", 1))), 1)
        key = (name, int(r["Grid_Size_X"]) // wx, int(r.get("Grid_Size_Y", 1)))
        groups.setdefault(key, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
    with open(out_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Name", "BlocksX", "GridY", "Calls", "TotalDurationNs", "AverageNs", "MinNs", "MaxNs"])
        for (name, bx, gy), d in sorted(groups.items()):
            w.writerow([name, bx, gy, len(d), sum(d), "%.1f" % (sum(d) / len(d)), min(d), max(d)])


def bow_pool(rng, n, places, n_words=1000):
    """n BowVectors of about n_words words around the given places."""
    out = []
    for _ in range(n):
        base = places[int(rng.integers(len(places)))]
        w = np.unique(np.concatenate([base[rng.random(len(base)) < rng.uniform(0.75, 1.0)], rng.integers(0, N_VOC, n_words // 4)])).astype(np.int32)
        v = rng.uniform(0.1, 1.0, len(w))
        out.append((w, v / v.sum()))
    return out


def time_ladder(pkg, B, nf, reps):
    """tc2li_relocalization_refine_batch for nf hypotheses beside tc2li_track_reference_keyframe_batch for the same nf frames (KITTI-size
    stereo frames at 2 000 features, as tools/time_bow.py builds them): the candidate / reference keyframe of frame f is frame f + 8, the
    same image, its points back-projected from the stereo depth; the first 14 points are the PnP inliers, so every hypothesis takes the
    (10, 100) search and the second optimisation."""
    import torch
    from tc2li_slam_amd import synthetic
    Wd, Hd = 1242, 375
    base = [np.stack(synthetic.stereo_pair(s, Wd, Hd)) for s in range(8)]
    dev = torch.from_numpy(np.concatenate([base[f % len(base)] for f in range(nf)])).cuda()
    ext = pkg.OrbExtractor(nfeatures=2000, max_width=Wd, max_height=Hd, max_images=2 * nf)
    kps, desc, counts, _ = ext.extract_batch_dev(dev.data_ptr(), 2 * nf, Wd, Hd, Wd, Wd * Hd)
    torch.cuda.synchronize()
    p, lf, d, w = B.random_tree(10, 6, seed=11)
    voc = pkg.Vocabulary.from_arrays(10, 6, B.L1_NORM, B.TF_IDF, p, lf, d, w)
    bows = voc.transform_orb(ext, counts[0:2 * nf:2], levelsup=4)
    bf = np.float32(synthetic.BF); b = np.float32(bf / np.float32(synthetic.FX))
    u_right, depth, _ = pkg.stereo_match_batch(ext, nf, float(bf), float(b))
    fx, fy, cx, cy = [np.float32(v) for v in (synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY)]
    cam5 = np.float32([fx, fy, cx, cy, bf]).astype(np.float64)
    sf = np.asarray(ext.GetScaleFactors(), np.float32)
    refs, hyps = [], []
    for f in range(nf):
        g = (f + 8) % nf
        n = int(counts[2 * g])
        k = kps[2 * g][:n]
        z = depth[g, :n]
        zz = np.where(z > 0, z, 1).astype(np.float32)
        Xw = np.stack([(k["x"] - cx) * zz / fx, (k["y"] - cy) * zz / fy, zz], 1).astype(np.float32)
        hp = (z > 0).astype(np.uint8)
        refs.append(dict(keys=k, descriptors=desc[2 * g][:n], fv_node=bows[g]["fv_node"], fv_offset=bows[g]["fv_offset"], fv_index=bows[g]["fv_index"],
                         has_point=hp, Xw=Xw, observed=np.ones(n, np.uint8), last_pose7=[0, 0, 0, 1, 0.01, 0, 0]))
        dist = np.sqrt((Xw ** 2).sum(1)).astype(np.float32)
        max_raw = (dist * sf[k["octave"]]).astype(np.float32)
        match = np.where(z > 0, np.arange(n), -1).astype(np.int32)
        inl = np.zeros(n, np.uint8)
        inl[np.flatnonzero(z > 0)[:14]] = 1
        hyps.append(dict(frame_index=f, has_point=hp, Xw=Xw, point_descriptors=desc[2 * g][:n], min_distance=np.float32(0.8) * max_raw / sf[-1],
                         max_distance=np.float32(1.2) * max_raw, max_distance_raw=max_raw, angle=k["angle"].astype(np.float32),
                         pose7=[0, 0, 0, 1, 0.01, 0, 0], match=match, inlier=inl))
    keypoints = kps[:2 * nf]
    legs = dict(relocalization_refine=lambda: pkg.capi.relocalization_refine_batch(ext, hyps, u_right, cam5),
                track_reference_keyframe=lambda: pkg.capi.track_reference_keyframe_batch(ext, voc, keypoints, u_right, refs, cam5))
    res = {}
    for name, fn in legs.items():
        out = fn()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        r = dict(frames=nf, call_ms=float(np.median(ts)))
        if name == "relocalization_refine":
            r.update(success=int(((out["status"] & 64) != 0).sum()), mean_n_good=float(out["n_good"].mean()),
                     mean_additional=float(out["n_additional"][:, 0].mean()), third_optimisations=int(((out["status"] & 32) != 0).sum()))
        else:
            r.update(mean_inliers=float(np.mean(out[3])))
        res["%s_%d" % (name, nf)] = r
        print(json.dumps(r), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="256:512,1024:512,4096:128", help="keyframes per database : queries (databases) per call")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--ladder", type=int, default=512, help="hypotheses of the refinement-ladder leg (0: skip)")
    ap.add_argument("--summarize", nargs=2, metavar=("TRACE_CSV", "OUT_CSV"))
    a = ap.parse_args()
    if a.summarize:
        summarize(*a.summarize)
        return
    import tc2li_loader
    import bow_ref as B
    pkg = tc2li_loader.load()
    if pkg.device_count() < 1:
        raise SystemExit("time_reloc.py needs a GPU")
    p, lf, d, w = B.random_tree(10, 6, seed=11)
    voc = pkg.Vocabulary.from_arrays(10, 6, B.L1_NORM, B.TF_IDF, p, lf, d, w)
    rng = np.random.default_rng(1)
    places = [np.unique(rng.integers(0, N_VOC, 800)).astype(np.int32) for _ in range(8)]
    res = {}
    for spec in a.sizes.split(","):
        n_kf, n_q = [int(x) for x in spec.split(":")]
        pool = bow_pool(rng, n_kf, places)
        dbs = []
        t0 = time.perf_counter()
        for q in range(n_q):   # the same keyframes in every database, in a rotated order: what is timed does not depend on the content
            db = pkg.KeyFrameDatabase(voc)
            for i in range(n_kf):
                k = (i + q) % n_kf
                db.add(k, 0, *pool[k])
            for i in range(0, n_kf, 3):
                db.set_covisibility(i, [(i + j) % n_kf for j in range(1, 11)])
            dbs.append(db)
        build_s = time.perf_counter() - t0
        frames = bow_pool(rng, n_q, places)
        queries = [(db, 0, *f) for db, f in zip(dbs, frames)]
        t0 = time.perf_counter()
        cands, _ = pkg.detect_relocalization_candidates_batch(queries, capacity=n_kf)   # warm-up: the databases' device copies
        first_ms = (time.perf_counter() - t0) * 1e3
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            cands, _ = pkg.detect_relocalization_candidates_batch(queries, capacity=n_kf)
            ts.append((time.perf_counter() - t0) * 1e3)
        words = sum(len(v[0]) for v in pool)
        res["query_%d" % n_kf] = dict(keyframes=n_kf, queries=n_q, mean_words=words / n_kf, call_ms=float(np.median(ts)), first_call_ms=first_ms,
                                      build_s=build_s, mean_candidates=float(np.mean([len(c) for c in cands])),
                                      # what the two list reads move at least: every keyframe row once per query, the frame's vector once
                                      pool_bytes=12 * words * n_q + 12 * sum(len(f[0]) for f in frames))
        print(json.dumps(res["query_%d" % n_kf]), flush=True)
        del dbs, queries
    pool = bow_pool(rng, 4096, places)
    pairs = [(pool[i], pool[(7 * i + 1) % len(pool)]) for i in range(len(pool))]
    voc.score(pairs)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        voc.score(pairs)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["score_4096"] = dict(pairs=len(pairs), call_ms=float(np.median(ts)))
    print(json.dumps(res["score_4096"]), flush=True)
    if a.ladder > 0:
        res.update(time_ladder(pkg, B, a.ladder, a.reps))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
