"""Timings of the batched inertial optimisation of the IMU initialisation: tc2li_inertial_optimization_batch (first overload, the
reference's priors 1e2 / 1e6 and 200 iterations) and tc2li_inertial_scale_refinement_batch (second overload, 10 iterations) beside
tc2li_host_inertial_optimization_batch / tc2li_host_inertial_scale_refinement_batch on the same input, host memory to host memory, for 64
and 512 maps of 12, 50 and 150 keyframes.  Call times are host clocks around whole calls (validation, the links' informations, concatenation,
upload, kernel, download, copy-out on the device side; the single-problem entries on the pool's threads on the host side); the Python
binding's packing of the problem structures is outside the clock, and the in / out arrays are put back before every call.  The legs
alternate -- device, host, device, host, ... -- after one untimed call of each; the kernel's share is one more device call with
tc2li_profile_enable(1).  The host leg gets --threads CPUs (16: what a rank is granted) as the library's thread budget AND as the size of
the pool the batch entries run on (TC2LI_TRACKING_THREADS; under a budget of 16 that pool has 5 threads by default, the rest of the budget
belongs to the other stages of a running system).  One process: run it under a time limit of its own.

    timeout -k 10 900 python tools/time_imu_init.py [--maps 64 512] [--keyframes 12 50 150] [--reps 2] [--threads 16] [--json out.json]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_BASE = 4  # distinct maps per size; a batch cycles through them


def base_problems(pkg, oracle, synthetic, form, n_kf):
    import imu_init_cases as ic
    out = []
    for k in range(N_BASE):
        w = ic.world(pkg, oracle, synthetic, 40 + k, n_kf)
        if form == "optimization":
            out.append(ic.first_form(w))
        else:
            out.append(dict(Rwb=w["Rwb"], twb=w["twb"], vel=w["vel_true"], pres=list(w["pres"]), Rwg=w["Rwg0"], scale=1.0, bg3=np.tile(w["bg_true"], (n_kf, 1)),
                            ba3=np.tile(w["ba_true"], (n_kf, 1)), refine=True))
    return out


def measure(pkg, form, base, n_maps, reps):
    capi = pkg.capi
    arr, outs, keep = capi.pack_inertial_init_problems([base[i % N_BASE] for i in range(n_maps)])
    state = [{k: o[k].copy() for k in ("vel3", "Rwg9", "scale", "bg", "ba") if o.get(k) is not None} for o in outs]

    def put_back():
        for o, s in zip(outs, state):
            for k, v in s.items():
                o[k][...] = v
    name = "inertial_optimization_batch" if form == "optimization" else "inertial_scale_refinement_batch"
    dev, hst = getattr(capi.lib(), "tc2li_" + name), getattr(capi.lib(), "tc2li_host_" + name)
    dev.argtypes, hst.argtypes = [C.c_void_p, C.c_int, C.c_void_p], [C.c_void_p, C.c_int]
    legs = {"device": lambda: dev(C.addressof(arr), n_maps, None), "host": lambda: hst(C.addressof(arr), n_maps)}
    results = {}

    def run(leg):
        put_back()
        t = time.perf_counter()
        rc = legs[leg]()
        ms = (time.perf_counter() - t) * 1e3
        assert rc == n_maps, capi.lib().tc2li_last_error()
        results[leg] = [(int(o["iterations_run"][0]), o["Rwg9"].copy()) for o in outs[:N_BASE]]
        return ms
    for leg in ("device", "host"):  # buffers, pools, clocks
        run(leg)
    times = {"device": [], "host": []}
    for _ in range(reps):
        for leg in ("device", "host"):
            times[leg].append(run(leg))
    capi.profile_enable(True)
    capi.profile_report()
    run("device")
    kernels = {k: v[1] for k, v in capi.profile_report().items() if k.startswith("k_ii_")}
    capi.profile_enable(False)
    run("host")
    # the two paths solved the same problems (with the reference's priors the tail of the first form is decided by rounding: the two may
    # stop an iteration or two apart, test_imu_init.py; the tests compare states at their bars on problems chosen for it)
    rwg_diff = max(float(np.abs(R_d - R_h).max()) for (_, R_d), (_, R_h) in zip(results["device"], results["host"]))
    assert rwg_diff < 1e-3, (form, n_maps, rwg_diff)
    del keep
    return dict(form=form, maps=n_maps, keyframes=len(base[0]["Rwb"]), device_ms=times["device"], host_ms=times["host"], kernel_ms=kernels, rwg_difference=rwg_diff,
                iterations_device=[r[0] for r in results["device"]], iterations_host=[r[0] for r in results["host"]])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--maps", type=int, nargs="+", default=[64, 512])
    ap.add_argument("--keyframes", type=int, nargs="+", default=[12, 50, 150])
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--json")
    a = ap.parse_args()
    from oracle import pyoracle as oracle
    oracle.build()  # (before the first HIP call: a process that has initialised the GPU starts no children)
    os.environ["TC2LI_TRACKING_THREADS"] = str(a.threads)
    import tc2li_loader
    pkg = tc2li_loader.load()
    pkg.capi.set_host_thread_budget(a.threads)
    from tc2li_slam_amd import synthetic
    rows = []
    threads = pkg.capi.host_threads()
    print("host thread budget %d, the batch entries' pool %d threads" % (threads["budget"], threads["tracking_pool"]), flush=True)
    for form in ("optimization", "refinement"):
        for n_kf in a.keyframes:
            base = base_problems(pkg, oracle, synthetic, form, n_kf)
            for n_maps in a.maps:
                r = measure(pkg, form, base, n_maps, a.reps)
                rows.append(r)
                print(json.dumps(r), flush=True)
                if a.json:
                    json.dump(dict(reps=a.reps, rows=rows), open(a.json, "w"), indent=1)
    print("| form | maps | keyframes | device call ms | of it kernel ms | host batch ms (%d threads) |" % threads["tracking_pool"])
    print("|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %s | %.2f | %s |" % (r["form"], r["maps"], r["keyframes"], " / ".join("%.2f" % t for t in r["device_ms"]), sum(r["kernel_ms"].values()),
                                                 " / ".join("%.2f" % t for t in r["host_ms"])))


if __name__ == "__main__":
    main()
