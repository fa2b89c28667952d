"""Device time of the preprocess stage of tc2li_lidar_frontend_batch (last_timings()[0]) for S KITTI-size scans (synthetic HDL-64
sweeps, ~130 000 points each), with Preprocess::feature_enabled off (k_pre_stream) and on (the plane / edge classifier).
python tools/time_preprocess_features.py [S] [reps]"""
import json
import os
import sys

sys.path.insert(0, os.getcwd())
import numpy as np
import tc2li_loader

pkg = tc2li_loader.load()
from tc2li_slam_amd import synthetic
import torch

S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 5
U = 4
scans = [synthetic.lidar_scan(synthetic.Scene(u), u + 1) for u in range(U)]
tile = [s % U for s in range(S)]
boot = scans[0][:2000]
fe = pkg.LidarFrontEnd(max_points_per_scan=int(max(len(x) for x in scans)), max_scans=S)
m = pkg.LidarMap()
pts = np.zeros(len(boot), pkg.capi.POINT_DTYPE)
for f in ("x", "y", "z", "intensity"):
    pts[f] = boot[f]
m.Build(pts)
maps = [m] * S
states = np.stack([pkg.pack_lidar_state(np.eye(3), np.zeros(3))] * S)
raw = np.concatenate([scans[t] for t in tile])
offs = np.concatenate([[0], np.cumsum([len(scans[t]) for t in tile])]).astype(np.int32)
dev = torch.from_numpy(raw.view(np.uint8)).cuda()
stream = torch.cuda.current_stream().cuda_stream
out = {"scans": S, "points": int(len(raw))}
for name, feat in (("off", None), ("on", 64)):
    fe.set_features(feat)
    ms = []
    for r in range(REPS + 1):
        counts, _, _ = fe.frontend_batch(dev.data_ptr(), offs, maps, states, want_points=False, stream=stream)
        if r:  # the first call allocates
            ms.append(float(fe.last_timings()[0]))
    out[name] = {"preprocess_ms_median": float(np.median(ms)), "preprocess_ms_min": float(np.min(ms)),
                 "surface_points": int(counts[0].sum())}
out["ratio_on_off"] = out["on"]["preprocess_ms_median"] / out["off"]["preprocess_ms_median"]
print(json.dumps(out))
