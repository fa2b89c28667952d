"""Timings of the image ingest (tc2li_image_prep_batch) for a step's worth of camera images -- 1 024 images of 1242 x 375 by default -- in
three cases: BGR to gray, rectification of gray images, rectification of BGR images followed by gray.  Beside each: the host twin
(tc2li_host_image_prep_batch) on the same images, and the time the bytes of the case would take at the copy rate tc2li_diag_peaks reports
on the same GPU (bytes moved: source + gray per image, plus the fixed-point maps once -- the whole batch shares them).
Device times are HIP events around one call on device-resident images (the kernel and its launch; no upload); host times are host clocks
around one call.  Median, minimum and maximum of --reps after one warm-up.  Every leg runs in a child process of its own under a time
limit, so that a hang ends that step and nothing more is started on the GPU after it.

    python tools/time_image_prep.py [--images 1024] [--width 1242] [--height 375] [--reps 9] [--json out.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CASES = {"bgr_to_gray": (3, 0), "rectify_gray": (1, 1), "rectify_bgr_to_gray": (3, 1)}   # channels, mode
N_BASE = 8


def images_of(n, h, w, c):
    base = np.random.default_rng(77).integers(0, 256, (N_BASE, h, w, c), dtype=np.uint8)
    return base, base[np.arange(n) % N_BASE]


def maps_of(w, h):
    import image_prep_cases as K
    return K.make_map("warp", w, h, w, h, 5) + K.make_map("warp", w, h, w, h, 6)


def bytes_moved(case, n, h, w):
    c, mode = CASES[case]
    return n * h * w * (c + 1) + (2 * h * ((w + 3) // 4 * 4) * 6 if mode else 0)


def child_device(case, n, h, w, reps):
    import torch
    import image_prep_ref as ref
    import tc2li_loader
    pkg = tc2li_loader.load()
    c, mode = CASES[case]
    base, imgs = images_of(n, h, w, c)
    maps = maps_of(w, h) if mode else None
    prep = pkg.ImagePrep(w, h, c, rgb=False, mode=mode, max_images=n)
    if mode:
        prep.set_maps(0, maps[0], maps[1])
        prep.set_maps(1, maps[2], maps[3])
    dev = torch.from_numpy(imgs if c > 1 else imgs[..., 0]).cuda()
    out = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    pkg.image_prep_batch(prep, dev, out=out, stream=stream)          # warm-up: the code object
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pkg.image_prep_batch(prep, dev, out=out, stream=stream)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    for i in (0, 1, n - 1):                                         # an even and an odd camera, and the last image
        src = base[i % N_BASE] if c > 1 else base[i % N_BASE][..., 0]
        want = ref.image_prep(src, mode, 0, None if maps is None else maps[2 * (i & 1):2 * (i & 1) + 2])
        assert np.array_equal(out[i].cpu().numpy(), want), i
    print(json.dumps(dict(case=case, leg="device", images=n, ms=float(np.median(times)), min_ms=min(times), max_ms=max(times), all_ms=times,
                          bytes=bytes_moved(case, n, h, w))))


def child_host(case, n, h, w, reps):
    import tc2li_loader
    pkg = tc2li_loader.load()
    c, mode = CASES[case]
    _, imgs = images_of(n, h, w, c)
    imgs = np.ascontiguousarray(imgs if c > 1 else imgs[..., 0])
    maps = maps_of(w, h) if mode else None
    p = pkg.capi.image_prep_params(w, h, c, rgb=False, mode=mode)
    pkg.image_prep_batch(p, imgs[:4], maps=maps, host=True)           # warm-up: the pool
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        pkg.image_prep_batch(p, imgs, maps=maps, host=True)
        times.append((time.perf_counter() - t) * 1e3)
    print(json.dumps(dict(case=case, leg="host", images=n, ms=float(np.median(times)), min_ms=min(times), max_ms=max(times), all_ms=times,
                          host_threads=pkg.capi.host_threads()["extractor_pool"])))


def child_peaks():
    import tc2li_loader
    pkg = tc2li_loader.load()
    print(json.dumps(dict(leg="peaks", hbm_copy_gbps=pkg.capi.diag_peaks()[2])))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=1024)
    ap.add_argument("--width", type=int, default=1242)
    ap.add_argument("--height", type=int, default=375)
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=150)
    ap.add_argument("--json")
    ap.add_argument("--child", help="peaks, or device:<case> / host:<case>: one leg in this process")
    a = ap.parse_args()
    if a.child:
        if a.child == "peaks":
            child_peaks()
        else:
            leg, case = a.child.split(":")
            (child_device if leg == "device" else child_host)(case, a.images, a.height, a.width, a.reps if leg == "device" else a.host_reps)
        return
    rows = []

    def run(leg):
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--child", leg, "--images", str(a.images), "--width",
               str(a.width), "--height", str(a.height), "--reps", str(a.reps), "--host-reps", str(a.host_reps)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            sys.exit("the leg %s ended with status %d; nothing more is started\n%s" % (leg, r.returncode, r.stderr[-2000:]))
        rows.append(json.loads(r.stdout.strip().splitlines()[-1]))
        return rows[-1]

    gbps = run("peaks")["hbm_copy_gbps"]
    print("copy rate of tc2li_diag_peaks: %.0f GB/s" % gbps, flush=True)
    for case in CASES:
        d, h = run("device:" + case), run("host:" + case)
        floor_ms = d["bytes"] / (gbps * 1e9) * 1e3
        print("%-20s %d images %dx%d: device %.3f ms (min %.3f, max %.3f over %d calls) = %.2f x the %.3f ms of %.2f GB at the copy rate; "
              "host twin %.0f ms (min %.0f, max %.0f; pool of %d threads) = %.0f x the device"
              % (case, a.images, a.width, a.height, d["ms"], d["min_ms"], d["max_ms"], a.reps, d["ms"] / floor_ms, floor_ms, d["bytes"] / 1e9,
                 h["ms"], h["min_ms"], h["max_ms"], h["host_threads"], h["ms"] / d["ms"]), flush=True)
    if a.json:
        json.dump(dict(images=a.images, width=a.width, height=a.height, rows=rows), open(a.json, "w"), indent=1)


if __name__ == "__main__":
    main()
