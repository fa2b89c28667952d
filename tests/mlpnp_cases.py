"""Generated MLPnP RANSAC problems and the comparison of a library result with the restatement (tests/mlpnp_ref.py), shared by
tests/test_mlpnp.py (host entry) and tests/test_mlpnp_gpu.py (device entry).

The comparison, per problem and call:
* the restatement runs in its variants (SVD or eigh for the eigenvector, two null-space bases); ``s`` is the largest difference of [R | t]
  between the first variant and the others over all iterations of the call that reach min_inliers, rotation entries absolute,
  translation relative to max(1, |t|).  The finite-difference Jacobian is NOT among the variants: it would only widen the bound.
* the library's Rt12 must be within max(10 s, 1e-12) of the first variant's: ten times what two correct f64 codes of one formula differ by.
* pose7: every component within one float32 unit in the last place of the restatement's (of the component itself; translation: of
  max(1, |t|)): both are roundings of doubles that are closer than that.
* found, no_more, n_inliers, the state (iterations, best_inliers, best_Tcw, best flags) and every inlier flag: equal.
* a problem is left out of the flag and selection comparison only if the variants disagree among themselves on any of these, or if some
  correspondence has |error2 / maxError - 1| < 1e-4 in an iteration up to the selected one.  The caller fails above 5 % left out.
"""
import numpy as np

import mlpnp_ref as ref

CAM5 = np.array([718.856, 718.856, 607.1928, 185.2157, 386.1448])      # KITTI 00-02 pinhole (fx fy cx cy bf)
CAM4 = CAM5[:4]
N_LEVELS = 8
SCALE = 1.2 ** np.arange(N_LEVELS)
LEVEL_SIGMA2 = (SCALE.astype(np.float32) ** 2).astype(np.float32)
KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])   # tc2li_keypoint
VARIANTS = [dict(evec="svd", basis=0), dict(evec="eigh", basis=0), dict(evec="svd", basis=1), dict(evec="eigh", basis=1)]


def _keys(xy, octave):
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    k["x"], k["y"], k["octave"] = xy[:, 0], xy[:, 1], octave
    k["size"] = 31.0 * SCALE[octave]
    return k


def make_problem(seed, N, outliers, noise_px, planar=False, n_unmatched=None, n_iterations=5, n_draws=6 * 400):
    """One frame with N matched keypoints (and some unmatched ones between them) of a scene seen from a random pose."""
    rng = np.random.default_rng(seed)
    n_unmatched = N // 3 if n_unmatched is None else n_unmatched
    w = rng.normal(size=3); w *= rng.uniform(0.05, 0.6) / np.linalg.norm(w)
    R = ref.rodrigues2rot(w)
    if planar:
        # z exactly 0: rank exactly 2.  A near scene: the planar branch's scale (MLPnPsolver.cpp:524, taken after transposeInPlace) puts
        # the linear translation off by a factor, and Gauss-Newton gives up on a first step above 5 (:724)
        Xw = np.stack([rng.uniform(-1.5, 1.5, N), rng.uniform(-1.5, 1.5, N), np.zeros(N)], 1).astype(np.float32)
        t = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), rng.uniform(2.5, 4)])
        Xc = Xw.astype(np.float64) @ R.T + t
    else:
        t = rng.uniform(-3, 3, 3)
        uv = np.stack([rng.uniform(20, 1220, N), rng.uniform(20, 350, N)], 1)
        z = rng.uniform(4, 40, N)
        Xc = np.stack([(uv[:, 0] - CAM4[2]) / CAM4[0] * z, (uv[:, 1] - CAM4[3]) / CAM4[1] * z, z], 1)
        Xw = ((Xc - t) @ R).astype(np.float32)
        Xc = Xw.astype(np.float64) @ R.T + t
    octave = rng.integers(0, N_LEVELS, N)
    uv = np.stack([CAM4[0] * Xc[:, 0] / Xc[:, 2] + CAM4[2], CAM4[1] * Xc[:, 1] / Xc[:, 2] + CAM4[3]], 1)
    uv += rng.normal(size=(N, 2)) * noise_px * SCALE[octave][:, None]
    bad = rng.random(N) < outliers
    uv[bad] = np.stack([rng.uniform(0, 1241, bad.sum()), rng.uniform(0, 376, bad.sum())], 1)
    # the frame: matched keypoints at random places among unmatched ones, the points in another order than the keypoints
    n_kp = N + n_unmatched
    place = np.sort(rng.permutation(n_kp)[:N])
    xy = np.stack([rng.uniform(0, 1241, n_kp), rng.uniform(0, 376, n_kp)], 1)
    octs = rng.integers(0, N_LEVELS, n_kp)
    xy[place], octs[place] = uv, octave
    order = rng.permutation(N)
    match = np.full(n_kp, -1, np.int32)
    match[place] = order
    Xw_store = np.zeros((N, 3), np.float32)
    Xw_store[order] = Xw
    return dict(keys=_keys(xy.astype(np.float32), octs), match=match, Xw=Xw_store, draws=rng.integers(0, 2 ** 31, n_draws, dtype=np.uint32),
                n_iterations=n_iterations, true_Rt=np.hstack([R, t[:, None]]))


def easy(seed, N):
    return make_problem(seed, N, 0.15, 0.3)


def hard(seed, N):
    return make_problem(seed, N, 0.40, 0.7)


def solvers_for(problem, params=None, level_sigma2=LEVEL_SIGMA2, cam4=CAM4):
    return [ref.Solver(problem["keys"], problem["match"], problem["Xw"], level_sigma2, cam4, params, **v) for v in VARIANTS]


def _rt_diff(a, b):
    d = np.abs(a - b)
    return max(d[:, :3].max(), (d[:, 3] / max(1.0, np.linalg.norm(b[:, 3]))).max())


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def compare_call(solvers, n_iterations, draws, got, p, report):
    """One iterate() call: ``solvers`` are the restatement's variants in the state before the call (advanced here), ``got`` the library's
    batch output, ``p`` the problem's row in it.  Appends to ``report`` (dict of lists: s, dist, left_out) and asserts."""
    outs = [sv.iterate(n_iterations, draws) for sv in solvers]
    for sv in solvers:
        sv.forget_double_best()
    o0, sv0 = outs[0], solvers[0]
    s = 0.0
    for o in outs[1:]:
        for (Rt0, c0, _, _), (Rt1, _, _, _) in zip(o0["log"], o["log"]):
            if c0 >= sv0.min_inliers and np.all(np.isfinite(Rt0)) and np.all(np.isfinite(Rt1)):
                s = max(s, _rt_diff(Rt1, Rt0))
    bound = max(10 * s, 1e-12)
    report["s"].append(s)

    def summary(o, sv):
        return (o["found"], o["no_more"], o["n_inliers"], o["ret"], len(o["log"]), o["inlier"].tobytes(), sv.iterations, sv.best_inliers, sv.best_flags.tobytes())
    agree = all(summary(o, sv) == summary(o0, sv0) for o, sv in zip(outs[1:], solvers[1:]))
    close = any(np.any(np.abs(ratio - 1.0) < 1e-4) for (_, _, _, ratio) in o0["log"])
    left_out = (not agree) or close
    report["left_out"].append(bool(left_out))
    if left_out:
        return dict(bound=bound, left_out=True, out=o0)
    n_kp = sv0.n_keypoints
    assert (int(got["found"][p]), int(got["no_more"][p]), int(got["n_inliers"][p])) == (o0["found"], o0["no_more"], o0["n_inliers"]), \
        (p, got["found"][p], got["no_more"][p], got["n_inliers"][p], o0["found"], o0["no_more"], o0["n_inliers"])
    assert np.array_equal(got["inlier"][p][:n_kp], o0["inlier"]) and not got["inlier"][p][n_kp:].any(), p
    assert (int(got["iterations"][p]), int(got["best_inliers"][p])) == (sv0.iterations, sv0.best_inliers), p
    best = np.zeros(n_kp, np.uint8)
    best[sv0.kp_index[sv0.best_flags]] = 1
    assert np.array_equal(got["best_inlier"][p][:n_kp], best), p
    Rt = got["Rt12"][p].reshape(3, 4)
    dist = _rt_diff(Rt, o0["Rt"])
    report["dist"].append(dist)
    assert dist <= bound, (p, dist, s)
    want7 = ref.pose7_of(o0["Rt"])
    tn = max(1.0, float(np.linalg.norm(o0["Rt"][:, 3])))
    for k in range(7):
        tol = _ulp(want7[k]) if k < 4 else _ulp(tn)
        assert abs(float(got["pose7"][p][k]) - float(want7[k])) <= tol, (p, k, got["pose7"][p], want7)
    assert np.array_equal(got["best_Tcw"][p].reshape(3, 4), sv0.best_Tcw), (p, got["best_Tcw"][p], sv0.best_Tcw)
    return dict(bound=bound, left_out=False, out=o0)


def new_report():
    return dict(s=[], dist=[], left_out=[])


def check_left_out(report):
    n = len(report["left_out"])
    assert sum(report["left_out"]) <= 0.05 * n, "%d of %d problems left out" % (sum(report["left_out"]), n)


def state_of(got, p, problem):
    """the problem dict for the next call on the same solver"""
    n = len(problem["keys"])
    return dict(problem, iterations=int(got["iterations"][p]), best_inliers=int(got["best_inliers"][p]), best_Tcw=got["best_Tcw"][p].copy(),
                best_inlier=got["best_inlier"][p][:n].copy())
