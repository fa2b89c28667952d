"""Timings of the ORB vocabulary on the GPU: ComputeBoW (tc2li_orb_compute_bow_batch) for 128 / 512 / 1024 frames of KITTI-size stereo
features against a generated k = 10, L = 6 vocabulary, the host-descriptor entry for the same frames, SearchByBoW for 512 pairs, and the
text loader on a generated 1.1 M-node file.  Call times are host clocks around calls that end in a device synchronisation (they include
the downloads of the results); kernel times come from a rocprofv3 --kernel-trace --stats run of this script.

    python tools/time_bow.py [--frames 128,512,1024] [--reps 5] [--json out.json]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", default="128,512,1024")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=None)
    ap.add_argument("--skip-loader", action="store_true")
    a = ap.parse_args()
    import torch
    import tc2li_loader
    import bow_ref as R
    pkg = tc2li_loader.load()
    from tc2li_slam_amd import synthetic
    if pkg.device_count() < 1:
        raise SystemExit("time_bow.py needs a GPU")
    res = {}
    p, lf, d, w = R.random_tree(10, 6, seed=11)
    voc = pkg.Vocabulary.from_arrays(10, 6, R.L1_NORM, R.TF_IDF, p, lf, d, w)
    Wd, Hd = 1242, 375
    base = [np.stack(synthetic.stereo_pair(s, Wd, Hd)) for s in range(8)]
    nmax = max(int(x) for x in a.frames.split(","))
    imgs = np.concatenate([base[f % len(base)] for f in range(nmax)])
    dev = torch.from_numpy(imgs).cuda()
    ext = pkg.OrbExtractor(nfeatures=2000, max_width=Wd, max_height=Hd, max_images=2 * nmax)
    kps, desc, counts, _ = ext.extract_batch_dev(dev.data_ptr(), 2 * nmax, Wd, Hd, Wd, Wd * Hd)
    torch.cuda.synchronize()
    for nf in [int(x) for x in a.frames.split(",")]:
        c = counts[0:2 * nf:2]
        voc.transform_orb(ext, c, levelsup=4, raw=True)  # warm-up (and the vocabulary's device copy)
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            voc.transform_orb(ext, c, levelsup=4, raw=True)
            ts.append((time.perf_counter() - t0) * 1e3)
        descs = [desc[2 * f][:counts[2 * f]] for f in range(nf)]
        voc.transform(descs, levelsup=4)
        th = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            voc.transform(descs, levelsup=4)
            th.append((time.perf_counter() - t0) * 1e3)
        res["compute_bow_%d" % nf] = dict(frames=nf, descriptors=int(c.sum()), orb_entry_ms=float(np.median(ts)), host_entry_ms=float(np.median(th)))
        print(json.dumps(res["compute_bow_%d" % nf]), flush=True)
    # SearchByBoW: frame f against frame f + 8, which is the same image (the batch repeats 8 scenes): every feature matches, the dense case
    nf = min(512, nmax)
    bows = voc.transform_orb(ext, counts[0:2 * nf:2], levelsup=4)
    frames = [dict(keys=kps[2 * f][:counts[2 * f]], descriptors=desc[2 * f][:counts[2 * f]]) for f in range(nf)]

    def view(f, hp=False):
        v = dict(keys=frames[f]["keys"], descriptors=frames[f]["descriptors"], fv_node=bows[f]["fv_node"], fv_offset=bows[f]["fv_offset"],
                 fv_index=bows[f]["fv_index"])
        if hp:
            v["has_point"] = np.ones(len(frames[f]["keys"]), np.uint8)
        return v
    pairs = [dict(keyframe=view(f, True), frame=view((f + 8) % nf), nn_ratio=0.7, check_orientation=True) for f in range(nf)]
    pkg.search_by_bow_batch(pairs, capacity=ext.capacity)
    ts = []
    for _ in range(a.reps):
        t0 = time.perf_counter()
        _, nm = pkg.search_by_bow_batch(pairs, capacity=ext.capacity)
        ts.append((time.perf_counter() - t0) * 1e3)
    res["search_by_bow_%d" % nf] = dict(pairs=nf, call_ms=float(np.median(ts)), mean_matches=float(nm.mean()))
    print(json.dumps(res["search_by_bow_%d" % nf]), flush=True)
    # TrackReferenceKeyFrame beside TrackWithMotionModel on the same frames: the reference keyframe / last frame of frame f is frame f + 8
    # (the same image), its points back-projected from the stereo depth
    bf = np.float32(synthetic.BF); b = np.float32(bf / np.float32(synthetic.FX))
    u_right, depth, _ = pkg.stereo_match_batch(ext, nf, float(bf), float(b))
    fx, fy, cx, cy = [np.float32(v) for v in (synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY)]
    cam5 = np.float32([fx, fy, cx, cy, bf]).astype(np.float64)
    refs, lasts = [], []
    for f in range(nf):
        g = (f + 8) % nf
        n = int(counts[2 * g])
        k = kps[2 * g][:n]
        z = depth[g, :n]
        zz = np.where(z > 0, z, 1).astype(np.float32)
        Xw = np.stack([(k["x"] - cx) * zz / fx, (k["y"] - cy) * zz / fy, zz], 1).astype(np.float32)
        hp = (z > 0).astype(np.uint8)
        refs.append(dict(view(g, True), has_point=hp, Xw=Xw, observed=np.ones(n, np.uint8), last_pose7=[0, 0, 0, 1, 0.01, 0, 0]))
        lasts.append(dict(has_point=hp, outlier=np.zeros(n, np.uint8), Xw=Xw, keys=k, descriptors=desc[2 * g][:n], pose7=[0, 0, 0, 1, 0, 0, 0]))
    keypoints = kps[:2 * nf]
    packed = pkg.capi.pack_last_frames(lasts)
    preds = np.tile(np.array([0, 0, 0, 1, 0.01, 0, 0], np.float32), (nf, 1))
    legs = dict(track_reference_keyframe=lambda: pkg.capi.track_reference_keyframe_batch(ext, voc, keypoints, u_right, refs, cam5),
                track_motion_model=lambda: pkg.capi.track_motion_model_batch(ext, nf, keypoints, u_right, packed, preds, cam5, float(b)))
    for name, fn in legs.items():
        out = fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        res["%s_%d" % (name, nf)] = dict(frames=nf, call_ms=float(np.median(ts)), mean_inliers=float(np.mean(out[3])))
        print(json.dumps(res["%s_%d" % (name, nf)]), flush=True)
    if not a.skip_loader:
        ref = R.Voc(10, 6, R.L1_NORM, R.TF_IDF, p, lf, d, w)
        with tempfile.TemporaryDirectory() as td:
            path = os.path.join(td, "voc.txt")
            R.write_text(path, ref)
            t0 = time.perf_counter()
            v2 = pkg.Vocabulary.load_text(path)
            res["load_text"] = dict(nodes=v2.info()["nodes"], bytes=os.path.getsize(path), ms=(time.perf_counter() - t0) * 1e3)
        print(json.dumps(res["load_text"]), flush=True)
    if a.json:
        with open(a.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
