"""Hand-made windows for the directed tests of the local bundle adjustment's Levenberg-Marquardt loop: test_ba_exit_cases.py shows
with the oracle alone that every window reaches the branch it is named for, test_ba_exits_gpu.py then compares the product with the
oracle on the same dicts, in every place the loop lives.

The windows of synthetic.ba_window / ba_window_varied / inertial_window start far from their optimum (the loop runs its 10
iterations), in a world whose origin lies on the trajectory with Rcw the identity to 0.03 rad, and every observed depth is at least
1 m.  The cases here are the base window, synthetic.ba_window(3, n_opt=3, n_fix=3, n_points=120, pose_noise=(0.1, 0.01)) -- 87 points,
300 edges -- changed in one respect each:

  plain                 the base window itself: 10 iterations, one trial each.
  converged             the base window's optimum, rounded through float32 as the map stores it: three accepted steps that each lower chi2
                        by less than 1e-3 of it, so n_bad counts 1, 2, 3 and the loop ends after 3 iterations (n_bad >= 3).
  rho_zero              lambda_init = 1e30.  The increment is ~1e-27 and adds to nothing: the first step only normalises the quaternions that
                        the window holds rounded to float32 (|q| - 1 ~ 1e-8), which lowers chi2 by a few 1e-8 of it; the second step
                        leaves every pose and point as it was, tempChi == currentChi, rho == 0, ok = false: 2 iterations.  Seed
                        RHO_ZERO_SEED is the first one at which the first step's decrease is RHO_ZERO_ROOM times the 1e-8 that
                        test_ba_exit_cases.py asks of an accepted step (4.0e-8; at the base window's seed it is 0.97e-8).
  stall_after_progress  lambda_init = 1e-300, Gauss-Newton: real progress (n_bad stays 0 or is reset), then three stalled steps.
  rotated_a, _b, _c     the base window in a moved world frame, X' = R X + t and Tcw' = Tcw T^-1, both rounded through float32:
                        a  rotation vector 1.7 rad about (1, 2, 3), t = (50, -20, 10);
                        b  0.999 pi about x, every qw below 0.1 in size, t = 0;
                        c  rotation vector (0, 3.0, 0.3), t = (-300, 500, 40).
  behind                one landmark with four observations, the last of them in the window's last keyframe, placed at z = -0.5 m in that
                        keyframe's frame (its x and y there scaled by 0.02): edge_depth_positive ends 0 on that edge and 1 on its three others.
  close                 the same landmark at z = +0.05 m: the run recovers, all flags 1.
  lidar_converged       the base window with a LiDAR edge over its three free keyframes (600-point clouds, weight 1), fed back like `converged`.
  inertial_converged    synthetic.inertial_window(4, n_opt=4, n_points=200) fed back through oracle.local_inertial_ba after five of its
                        iterations: three steps of 3e-5 to 6e-5 remain and n_bad ends the loop.  (Fed back after the full run, the window
                        decides at the rounding level: test_ba_exit_cases.py's docstring.)

Every builder returns a dict with "window" (the dict BaBatch / LviBatch takes), "cam", "edges6" (the oracle's edge layout), "want" (the
oracle's result), "kw" (iterations / lambda_init) and "initial_chi2" (the robust cost the first iteration starts from, from the oracle's
own edge errors).  The dicts are built once per session and must not be written to."""
import numpy as np

BASE = dict(seed=3, n_opt=3, n_fix=3, n_points=120, pose_noise=(0.1, 0.01))
ITERATIONS = 10
INERTIAL = dict(seed=4, n_opt=4, n_points=200, first_iterations=5)
ROTATIONS = {"rotated_a": (1.7 * np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0), (50.0, -20.0, 10.0)),
             "rotated_b": ((0.999 * np.pi, 0.0, 0.0), (0.0, 0.0, 0.0)),
             "rotated_c": ((0.0, 3.0, 0.3), (-300.0, 500.0, 40.0))}
EXIT_CASES = ("converged", "rho_zero", "stall_after_progress", "lidar_converged", "inertial_converged")
VISUAL_CASES = ("plain", "converged", "rho_zero", "stall_after_progress", "rotated_a", "rotated_b", "rotated_c", "behind", "close", "lidar_converged")
ALL_CASES = VISUAL_CASES + ("inertial_converged",)
RHO_ZERO_SEED, RHO_ZERO_ROOM = 12, 3.0
TH_HUBER2 = (5.991, 7.815)   # mono, stereo: the Huber widths squared and the outlier rules of LocalBundleAdjustment

_cache = {}


def f32(a):
    """Through float32 and back: what the map keeps of an estimate."""
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def rot_from_rvec(r):
    r = np.asarray(r, np.float64)
    th = np.linalg.norm(r)
    if th < 1e-12:
        return np.eye(3)
    k = r / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def rot_from_quat(q):
    x, y, z, w = np.asarray(q, np.float64) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def quat_from_rot(R):
    """(qx, qy, qz, qw) by the largest of the four squares, so that a rotation by nearly pi (qw ~ 0) keeps its digits."""
    m = np.array([R[0, 0] - R[1, 1] - R[2, 2], R[1, 1] - R[0, 0] - R[2, 2], R[2, 2] - R[0, 0] - R[1, 1], R[0, 0] + R[1, 1] + R[2, 2]])
    i = int(np.argmax(m))
    s = 2.0 * np.sqrt(1.0 + m[i])
    if i == 3:
        q = [(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4]
    elif i == 0:
        q = [s / 4, (R[0, 1] + R[1, 0]) / s, (R[0, 2] + R[2, 0]) / s, (R[2, 1] - R[1, 2]) / s]
    elif i == 1:
        q = [(R[0, 1] + R[1, 0]) / s, s / 4, (R[1, 2] + R[2, 1]) / s, (R[0, 2] - R[2, 0]) / s]
    else:
        q = [(R[0, 2] + R[2, 0]) / s, (R[1, 2] + R[2, 1]) / s, s / 4, (R[1, 0] - R[0, 1]) / s]
    return np.array(q)


def rel(a, b):
    """Largest difference against the size of the reference, the measure of test_ba_gpu.py's pose bar."""
    return np.abs(np.asarray(a) - np.asarray(b)).max() / max(1.0, np.abs(b).max())


def move_world(w, rvec, t):
    """The window in the world frame X' = R X + t: points and Tcw' = Tcw T^-1, rounded through float32."""
    R, t = rot_from_rvec(rvec), np.asarray(t, np.float64)
    poses = np.empty_like(w["poses"])
    for k, p in enumerate(w["poses"]):
        Rcw = rot_from_quat(p[:4]) @ R.T
        poses[k] = np.concatenate([quat_from_rot(Rcw), p[4:] - Rcw @ t])
    return dict(w, poses=f32(poses), points=f32(w["points"] @ R.T + t))


def move_back(poses7, points3, rvec, t):
    """A result in the moved frame back in the original one -> (Rcw [K, 3, 3], tcw [K, 3], points)."""
    R, t = rot_from_rvec(rvec), np.asarray(t, np.float64)
    Rm = np.stack([rot_from_quat(p[:4]) for p in poses7])
    return Rm @ R, np.einsum("kij,j->ki", Rm, t) + poses7[:, 4:], (points3 - t) @ R


def pose_matrices(poses7):
    return np.stack([rot_from_quat(p[:4]) for p in poses7]), poses7[:, 4:].copy()


def depths(poses7, points3, edges6):
    """z of every edge's point in its keyframe."""
    Rm, tm = pose_matrices(poses7)
    k, p = edges6[:, 1].astype(int), edges6[:, 0].astype(int)
    return np.einsum("ej,ej->e", Rm[k, 2], points3[p]) + tm[k, 2]


def robust_chi2(oracle, poses7, points3, edges6, cam):
    """The Huber cost of the visual edges at a state, from the oracle's own edge errors: what the first iteration calls currentChi."""
    total = 0.0
    for e in edges6:
        err, _, _ = oracle.edge_linearize(poses7[int(e[1])], points3[int(e[0])], e, cam)
        c = e[5] * float(err @ err)
        d2 = TH_HUBER2[len(err) - 2]
        total += c if c <= d2 else 2.0 * np.sqrt(c * d2) - d2
    return total


def outliers(edges6, chi2, depth_positive):
    """The outlier set of LocalBundleAdjustment: chi2 over 5.991 (mono) / 7.815 (stereo), or a depth that is not positive."""
    return (chi2 > np.where(edges6[:, 4] >= 0, TH_HUBER2[1], TH_HUBER2[0])) | (depth_positive == 0)


def base_window(synthetic, seed=None):
    kw = dict(BASE)
    s = kw.pop("seed")
    return synthetic.ba_window(s if seed is None else seed, **kw)


def visual_case(pkg, oracle, w, lidar=None, **kw):
    """A case from a ba_window()-shaped dict: the oracle's run and the dict the product's batch takes."""
    window = dict(poses=w["poses"], fixed=w["fixed"], points=w["points"], edges=pkg.pack_ba_edges(w["edges"]), **kw)
    if lidar is None:
        want = oracle.local_ba(w["poses"], w["fixed"], w["points"], w["edges"], w["cam"], iterations=kw.get("iterations", ITERATIONS),
                               lambda_init=kw.get("lambda_init", 0.0))
    else:
        window.update(lidar)
        want = oracle.local_ba_lidar(w["poses"], w["fixed"], w["points"], w["edges"], w["cam"], lidar["win_pose"], lidar["clouds"], lidar["Tcl7"],
                                     lidar["weight"], iterations=kw.get("iterations", ITERATIONS), lambda_init=kw.get("lambda_init", 0.0))
    initial = robust_chi2(oracle, w["poses"], w["points"], w["edges"], w["cam"])
    if lidar is not None:   # the LiDAR edge's chi2 is information * residual^2, its planes those of the initial poses
        residual = oracle.lidar_window_evaluate(w["poses"], lidar["win_pose"], lidar["clouds"], lidar["Tcl7"])[1]
        initial += lidar["weight"] * residual * residual
    return dict(window=window, cam=w["cam"], edges6=w["edges"], want=want, kw=kw, initial_chi2=initial)


def _fed_back(w, want):
    return dict(w, poses=f32(want[0]), points=f32(want[1]))


def behind_landmark(w):
    """The first landmark with exactly four observations of which the last is in the window's last keyframe -> (point, that edge)."""
    last = len(w["poses"]) - 1
    e = w["edges"]
    for p in range(len(w["points"])):
        idx = np.flatnonzero(e[:, 0] == p)
        if len(idx) == 4 and int(e[idx[-1], 1]) == last:
            return p, int(idx[-1])
    raise AssertionError("no landmark with four observations ends in the last keyframe")


def _displaced(w, z):
    p, edge = behind_landmark(w)
    k = int(w["edges"][edge, 1])
    Rcw, tcw = rot_from_quat(w["poses"][k, :4]), w["poses"][k, 4:]
    Xc = Rcw @ w["points"][p] + tcw
    pts = w["points"].copy()
    pts[p] = f32(Rcw.T @ (np.array([0.02 * Xc[0], 0.02 * Xc[1], z]) - tcw))
    return dict(w, points=pts)


def lidar_window(synthetic, w):
    last = len(w["poses"]) - 1
    win = [last, last - 1, last - 2]
    return dict(win_pose=win, clouds=synthetic.ba_window_clouds(w, win, n_points=600), Tcl7=synthetic.TCL7, weight=1.0)


def inertial_problem(pkg, oracle, synthetic, seed, **kw):
    """synthetic.inertial_window with the product's pre-integrations, for both sides (as test_inertial_ba_gpu.py does)."""
    w = synthetic.inertial_window(seed, **kw)
    pre, pre298 = [], []
    for s, t1, t2 in w["samples"]:
        p = pkg.capi.Preintegrated(w["bias6"], *synthetic.IMU_NOISE)
        p.preintegrate(s, t1, t2)
        pre.append(p)
        pre298.append(oracle.pack_preintegrated(p.fields(), w["bias6"]))
    w["pre"], w["pre298"] = pre, np.stack(pre298)
    return w


def run_inertial_oracle(oracle, w, kf33, points, **kw):
    return oracle.local_inertial_ba(kf33, w["fixed"], w["has_imu"], w["calib24"], points, w["edges"], w["link4"], w["pre298"], w["cam"], **kw)


def inertial_window_dict(pkg, w, kf33, points, **kw):
    return dict(kf33=kf33, fixed=w["fixed"], has_imu=w["has_imu"], points=points, edges=pkg.pack_ba_edges(w["edges"]), link4=w["link4"], pre=w["pre"], **kw)


def _build(name, pkg, oracle, synthetic):
    if name == "inertial_converged":
        w = inertial_problem(pkg, oracle, synthetic, INERTIAL["seed"], n_opt=INERTIAL["n_opt"], n_points=INERTIAL["n_points"])
        first = run_inertial_oracle(oracle, w, w["kf33"], w["points"], iterations=INERTIAL["first_iterations"])
        kf, pts = f32(first[0]), f32(first[1])
        want = run_inertial_oracle(oracle, w, kf, pts)
        return dict(window=inertial_window_dict(pkg, w, kf, pts), cam=w["cam"], calib24=w["calib24"], edges6=w["edges"], want=want, kw={},
                    initial_chi2=want[6][0], first=first, problem=w)
    w = base_window(synthetic)
    if name == "plain":
        return visual_case(pkg, oracle, w)
    if name == "converged":
        return visual_case(pkg, oracle, _fed_back(w, case("plain", pkg, oracle, synthetic)["want"]))
    if name == "rho_zero":
        return dict(visual_case(pkg, oracle, base_window(synthetic, RHO_ZERO_SEED), lambda_init=1e30), seed=RHO_ZERO_SEED)
    if name == "stall_after_progress":
        return visual_case(pkg, oracle, w, lambda_init=1e-300)
    if name in ROTATIONS:
        return dict(visual_case(pkg, oracle, move_world(w, *ROTATIONS[name])), transform=ROTATIONS[name])
    if name in ("behind", "close"):
        p, edge = behind_landmark(w)
        return dict(visual_case(pkg, oracle, _displaced(w, -0.5 if name == "behind" else 0.05)), point=p, edge=edge)
    if name == "lidar_converged":
        lw = lidar_window(synthetic, w)
        first = visual_case(pkg, oracle, w, lidar=lw)
        return dict(visual_case(pkg, oracle, _fed_back(w, first["want"]), lidar=lw), first=first)
    raise KeyError(name)


def case(name, pkg, oracle, synthetic):
    if name not in _cache:
        _cache[name] = _build(name, pkg, oracle, synthetic)
    return _cache[name]


def catalogue(pkg, oracle, synthetic):
    """Every case by name, in the order of ALL_CASES."""
    return {name: case(name, pkg, oracle, synthetic) for name in ALL_CASES}


def trace(c):
    """(iterations, trials per iteration, chi2 at the start of every iteration and after the last one, lambda after every iteration)."""
    want = c["want"]
    return want[4], [int(t) for t in want[5]["trials"]], np.concatenate([[c["initial_chi2"]], want[5]["chi2"]]), want[5]["lam"]


def assert_clean(c):
    """Finite inputs only: no NaN, no Inf."""
    w = c["window"]
    for k in ("poses", "kf33", "points"):
        if k in w:
            assert np.isfinite(np.asarray(w[k], np.float64)).all(), k
    assert np.isfinite(c["edges6"]).all() and np.isfinite(c["kw"].get("lambda_init", 0.0))
    for cl in w.get("clouds", []):
        assert np.isfinite(cl).all()
