"""Hand-made frames for the directed tests of the pose-inertial optimiser (k_pose_inertial / k_pose_inertial_batch,
pose_inertial_kernel.hip): test_pose_inertial_cases.py shows with the oracle alone that every case reaches the branch it is made
for, test_pose_inertial_gates_gpu.py then compares the product with the oracle on the same dicts.

Every builder returns the dict of problem(): synthetic.pose_inertial_problem() plus the product's pre-integration ("pre", the
record the product reads; "pre298", the same numbers packed for the oracle), "last_frame" and "packed_edges".  The kernel reads
the point of edge i at Xw[i], so edges[:, 0] == arange(E) holds in every case and is restored after every subset.

What the cases are (the letters are those of the tests):
  A  a frame that starts converged (exact observations at the float32 true state), with eight edges displaced by sqrt(t) pixels so
     that their chi2 is t: either side of 5.991 (mono), of 1.5 x 5.991 (mono, close point), of 7.815 (stereo), and one mono edge with
     chi2 ~ 0 whose point is behind the camera.  Its twin has fewer than 30 edges and five edges either side of the recovery gates
     18 / 24.
  B  the first n edges of a random frame around the n_graph_edges < 10 break (n + 3 graph edges in the keyframe form, n + 4 in the
     previous-frame form); one stereo edge sits between the gates of round 0 and round 1, so that the rounds that ran show in the inlier count.
  C  29 and 30 inliers after the last round, each with and without bRecInit.
  D  1, 127, 128, 129, 255, 256, 257 edges: the strides of the 128-lane linearisation and of the 256-lane loops; a gross outlier is
     moved to index 256 so that the second trip of the 256-lane loops decides a flag.
  E  an indefinite prior whose first pivot of the previous state's accelerometer bias is negative in every factorisation.
  F  an indefinite prior that the prior edge's Huber weight hides while the previous state is 2 m from the prior's mean: the
     factorisation fails only after accepted increments have brought the state back.
  G  a positive-definite prior 1 m from the previous state: the Huber weight is active, nothing fails.
  H  a pre-integrated rotation whose R^T R is 3.5e-3 from the identity: pi_normalize_rotation_f leaves its Newton steps (below 1e-3) for
     the Jacobi sweeps."""
import numpy as np

RTOL = 1e-4  # BASELINE.json's bar for SE3 poses

DESIGNED_T = (5.5, 6.5, 6.5, 8.6, 9.4, 7.4, 8.3, 0.0)          # chi2 of the designed edges of case A; the last one is behind the camera
DESIGNED_KIND = ("mono", "mono", "close", "close", "close", "stereo", "stereo", "behind")
DESIGNED_GATE = (5.991, 5.991, 1.5 * 5.991, 1.5 * 5.991, 1.5 * 5.991, 7.815, 7.815, None)
DESIGNED_FLAGS = (0, 1, 0, 0, 1, 0, 1, 1)
# the second one: a kernel that recovers below 17 instead of 18 leaves it flagged.  Its target differs between the forms because the few
# edges of this frame let the previous-frame form's pose drift, which takes 0.3 off this edge's chi2: it shall end 2 % from 17 and from 18.
RECOVERY_T = {False: (17.0, 17.5, 19.0, 23.0, 25.0), True: (17.0, 17.8, 19.0, 23.0, 25.0)}
RECOVERY_KIND = ("mono", "mono", "mono", "stereo", "stereo")
RECOVERY_GATE = (18.0, 18.0, 18.0, 24.0, 24.0)
RECOVERY_FLAGS = (0, 0, 1, 0, 1)
SMALL_PUSHED, SMALL_PUSHED_T = 2, 15.0                          # case B: a stereo edge between the stereo gates of round 0 and round 1
SMALL_N = (0, 1, 5, 6, 7, 10)
STRIDE_N = (1, 127, 128, 129, 255, 256, 257)


def problem(pkg, oracle, synthetic, seed, last_frame, **kw):
    w = synthetic.pose_inertial_problem(seed, last_frame=last_frame, **kw)
    p = pkg.capi.Preintegrated(w["bias6"], *synthetic.IMU_NOISE)
    p.preintegrate(w["samples"], w["t1"], w["t2"])
    w["pre"], w["pre298"] = p, oracle.pack_preintegrated(p.fields(), w["bias6"])
    w["last_frame"] = last_frame
    w["packed_edges"] = pkg.pack_ba_edges(w["edges"])
    return w


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def check(got, want, n_flag_slack=0, solver_failed=False):
    cur, oth, outlier, prior, rv, counts, failed = got
    wcur, woth, woutlier, wprior, wrv, wcounts = want[:6]
    assert failed == solver_failed
    assert np.sum(outlier != woutlier) <= n_flag_slack
    if n_flag_slack == 0:
        assert rv == wrv and counts == wcounts
    assert rel(cur[:24], wcur[:24]) < RTOL and np.allclose(cur[24:], wcur[24:], rtol=RTOL, atol=1e-6)
    assert rel(oth[:24], woth[:24]) < RTOL and np.allclose(oth[24:], woth[24:], rtol=RTOL, atol=1e-6)
    H, wH = prior[21:].reshape(15, 15), wprior[21:].reshape(15, 15)
    assert np.allclose(prior[:21], wprior[:21], rtol=RTOL, atol=1e-6)
    assert np.abs(H - wH).max() <= 1e-4 * np.abs(wH).max()


def run_oracle(oracle, w, details=True):
    return oracle.pose_inertial(w["cur33"], w["other33"], w["last_frame"], w["prior246"], w["calib24"], w["pre298"], w["pre298"], w["Xw"], w["edges"],
                                w["close"], w["cam"], rec_init=bool(w.get("rec_init")), details=details)


def item(w):
    """The dict the product's batch entry takes."""
    return dict(w, edges=w["packed_edges"])


def subset(pkg, w, idx, **more):
    """The frame with the edges idx only, in that order, re-indexed."""
    idx = np.asarray(idx, np.int64)
    e = w["edges"][idx].copy()
    Xw = w["Xw"][w["edges"][idx, 0].astype(np.int64)].copy()
    e[:, 0] = np.arange(len(idx))
    out = dict(w, edges=e, Xw=Xw.reshape(-1, 3), close=w["close"][idx].copy(), gross=w["gross"][idx].copy(), packed_edges=pkg.pack_ba_edges(e), **more)
    assert np.array_equal(out["edges"][:, 0], np.arange(len(idx))) and len(out["Xw"]) == len(idx)
    return out


def project(state33, Xw, cam):
    """(u, v, u - bf / z, z) of world points at the camera pose of a kf33 state."""
    Xc = Xw @ state33[:9].reshape(3, 3).T + state33[9:12]
    z = Xc[:, 2]
    u, v = cam[0] * Xc[:, 0] / z + cam[2], cam[1] * Xc[:, 1] / z + cam[3]
    return u, v, u - cam[4] / z, z


def edge_chi2(state33, w):
    """chi2 of every edge of w at a state, in plain numpy (pinhole / rectified stereo, information = edges[:, 5])."""
    u, v, ur, _ = project(state33, w["Xw"], w["cam"])
    e = w["edges"]
    stereo = e[:, 4] >= 0
    return e[:, 5] * ((e[:, 2] - u) ** 2 + (e[:, 3] - v) ** 2 + np.where(stereo, (e[:, 4] - ur) ** 2, 0.0))


def _design(w, i, kind, t):
    """Edge i becomes mono / mono with the close flag / stereo with chi2 t at w["cur33"]: its u is sqrt(t) pixels off."""
    w["edges"][i, 2] += np.sqrt(t)
    if kind != "stereo":
        w["edges"][i, 4] = -1.0
    w["close"][i] = 1 if kind == "close" else 0


def _converged(pkg, oracle, synthetic, last_frame):
    w = problem(pkg, oracle, synthetic, 5, last_frame, n_points=400, outlier_frac=0, mono_frac=0)
    w["cur33"] = w["cur33_true"].astype(np.float32).astype(np.float64)
    u, v, ur, z = project(w["cur33"], w["Xw"], w["cam"])
    assert (z > 1.0).all()
    w["edges"][:, 2], w["edges"][:, 3], w["edges"][:, 4], w["edges"][:, 5] = u, v, ur, 1.0
    w["close"][:] = 0
    w["gross"][:] = False
    return w


def designed_frame(pkg, oracle, synthetic, last_frame):
    """Case A -> (frame, indices of the eight designed edges)."""
    w = _converged(pkg, oracle, synthetic, last_frame)
    E = len(w["edges"])
    idx = np.arange(E - 8, E)
    for i, kind, t in zip(idx, DESIGNED_KIND, DESIGNED_T):
        if kind == "behind":
            Rcw, tcw = w["cur33"][:9].reshape(3, 3), w["cur33"][9:12]
            w["Xw"][i] = Rcw.T @ (np.array([1.0, 0.5, -8.0]) - tcw)
            u, v, _, z = project(w["cur33"], w["Xw"][i:i + 1], w["cam"])
            assert z[0] < -7.0
            w["edges"][i, 2:5] = u[0], v[0], -1.0
            w["close"][i] = 0
        else:
            _design(w, i, kind, t)
    w["packed_edges"] = pkg.pack_ba_edges(w["edges"])
    return w, idx


def recovery_frame(pkg, oracle, synthetic, last_frame, n_plain=20):
    """The twin of case A: n_plain exact edges and five on either side of the recovery gates -> (frame, indices of the five)."""
    w = subset(pkg, _converged(pkg, oracle, synthetic, last_frame), np.arange(n_plain + len(RECOVERY_KIND)))
    idx = np.arange(n_plain, n_plain + len(RECOVERY_KIND))
    for i, kind, t in zip(idx, RECOVERY_KIND, RECOVERY_T[last_frame]):
        _design(w, i, kind, t)
    w["packed_edges"] = pkg.pack_ba_edges(w["edges"])
    return w, idx


def small_frames(pkg, oracle, synthetic, last_frame):
    """Case B -> {n: frame}: the first n edges of seed 0.  The stereo edge SMALL_PUSHED has its u moved so far that its chi2 grows by
    about SMALL_PUSHED_T: an inlier by the 15.6 of round 0, an outlier by the 9.8 of round 1, so the inlier count tells whether
    the rounds after the first one ran (the flag itself is cleared again by the recovery pass)."""
    w = problem(pkg, oracle, synthetic, 0, last_frame)
    w["edges"] = w["edges"].copy()
    assert w["edges"][SMALL_PUSHED, 4] >= 0 and not w["gross"][SMALL_PUSHED]
    w["edges"][SMALL_PUSHED, 2] += np.sqrt(SMALL_PUSHED_T / w["edges"][SMALL_PUSHED, 5])
    return {n: subset(pkg, w, np.arange(n)) for n in SMALL_N}


BOUNDARY_PUSHED = 5  # the edge of case C that is made a recoverable outlier


def inlier_boundary_frames(pkg, oracle, synthetic, n_first=(31, 32), target=14.0):
    """Case C -> {(n, rec_init): frame}, keyframe form: the first n edges of seed 0.  One of them is a gross outlier; another one
    (BOUNDARY_PUSHED, stereo) has its u moved so far that its chi2 grows by about `target`: beyond 7.815 after the last round and below
    the 24 of the recovery pass, which therefore changes a flag exactly when it runs."""
    w = problem(pkg, oracle, synthetic, 0, False)
    w["edges"] = w["edges"].copy()
    assert w["edges"][BOUNDARY_PUSHED, 4] >= 0 and not w["gross"][BOUNDARY_PUSHED]
    w["edges"][BOUNDARY_PUSHED, 2] += np.sqrt(target / w["edges"][BOUNDARY_PUSHED, 5])
    return {(n, r): subset(pkg, w, np.arange(n), rec_init=r) for n in n_first for r in (False, True)}


def stride_frames(pkg, oracle, synthetic, seed, last_frame):
    """Case D -> {n: frame}; edge 256 of the full frame is one of its gross outliers."""
    w = problem(pkg, oracle, synthetic, seed, last_frame, n_points=900)
    E = len(w["edges"])
    assert E >= 257
    order = np.arange(E)
    if not w["gross"][256]:
        g = np.nonzero(w["gross"])[0]
        g = g[g > 256][0] if (g > 256).any() else g[-1]
        order[256], order[g] = g, 256
    w = subset(pkg, w, order)
    return {n: subset(pkg, w, np.arange(n)) for n in STRIDE_N}


IMU_WHITE_NOISE_SCALE = 100.0


def _failure_base(pkg, oracle, synthetic):
    """The frame of cases E, F and G: previous-frame form, seed 3, 200 points, pre-integrated with IMU_WHITE_NOISE_SCALE times the white
    noise of synthetic.IMU_NOISE.  With the plain noise the inertial edge's information is ~1e9 and every pivot of the previous state
    is what is left of two such terms (the smallest: 4e2 of 2e7); a pivot that changes sign through a prior entry of ~1e4 then decides
    at 1e-5 of its terms.  With the information a factor 1e4 smaller the deciding pivots stand at 3e-3 of their terms or more (the
    figures: test_pose_inertial_cases.py)."""
    w = problem(pkg, oracle, synthetic, 3, True, n_points=200)
    ng, na, ngw, naw = synthetic.IMU_NOISE
    p = pkg.capi.Preintegrated(w["bias6"], ng * IMU_WHITE_NOISE_SCALE, na * IMU_WHITE_NOISE_SCALE, ngw, naw)
    p.preintegrate(w["samples"], w["t1"], w["t2"])
    w["pre"], w["pre298"] = p, oracle.pack_preintegrated(p.fields(), w["bias6"])
    return w


def first_factorisation_failure(pkg, oracle, synthetic):
    """Case E."""
    w = _failure_base(pkg, oracle, synthetic)
    w["prior246"] = w["prior246"].copy()
    w["prior246"][21:].reshape(15, 15)[12, 12] = -1e9
    return w


def shift_previous_state(w, metres):
    """The previous state moved along its own body y axis, its camera pose re-derived as synthetic.pose_inertial_problem does."""
    o = w["other33"].copy()
    Rcb, tcb = w["calib24"][:9].reshape(3, 3), w["calib24"][9:12]
    R = o[12:21].reshape(3, 3)
    p = o[21:24] + metres * R[:, 1]
    o[21:24] = p
    o[9:12] = Rcb @ (-R.T @ p) + tcb
    return o


def mid_round_failure(pkg, oracle, synthetic, lam=2.0e4):
    """Case F: the prior's mean stays at the unshifted state."""
    w = _failure_base(pkg, oracle, synthetic)
    w["prior246"] = w["prior246"].copy()
    w["prior246"][21:].reshape(15, 15)[3, 3] = -lam
    w["other33"] = shift_previous_state(w, 2.0)
    return w


def active_prior_weight(pkg, oracle, synthetic, offset=1.0):
    """Case G -> (frame with the prior's mean `offset` metres off in x, the same frame with the plain prior)."""
    plain = _failure_base(pkg, oracle, synthetic)
    w = dict(plain, prior246=plain["prior246"].copy())
    w["prior246"][9] += offset
    return w, plain


def orthogonality_defect(R):
    """The measure pi_normalize_rotation_f chooses its path by: the largest |R^T R - I| entry."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    return np.abs(R.T @ R - np.eye(3)).max()


def skewed_preintegration(pkg, oracle, synthetic, eps=3e-3):
    """Case H -> (frame whose pre-integrated dR is dR (I + eps S), S symmetric with unit Frobenius norm; the unperturbed frame)."""
    plain = problem(pkg, oracle, synthetic, 4, False, n_points=200)
    w = problem(pkg, oracle, synthetic, 4, False, n_points=200)
    S = np.random.default_rng(7).normal(0, 1, (3, 3))
    S = (S + S.T) / 2
    S /= np.linalg.norm(S)
    dR = (np.array(w["pre"].p.dR, np.float64).reshape(3, 3) @ (np.eye(3) + eps * S)).astype(np.float32)
    for k in range(9):
        w["pre"].p.dR[k] = float(dR.ravel()[k])
    w["pre298"] = oracle.pack_preintegrated(w["pre"].fields(), w["bias6"])
    return w, plain


def assert_clean(w):
    """No NaN, no Inf, no zero depth, edges indexed in order."""
    for k in ("cur33", "other33", "Xw", "edges", "pre298", "calib24", "cam"):
        assert np.isfinite(np.asarray(w[k], np.float64)).all(), k
    if w["prior246"] is not None:
        assert np.isfinite(w["prior246"]).all()
    assert np.array_equal(w["edges"][:, 0], np.arange(len(w["edges"]))) and len(w["Xw"]) == len(w["edges"]) == len(w["close"])
    if len(w["edges"]):
        assert (np.abs(project(w["cur33"], w["Xw"], w["cam"])[3]) > 0.5).all()


def catalogue(pkg, oracle, synthetic):
    """Every frame of every case, by name, in the order of the mixed launch: {"B/kf/6": frame, ...}."""
    env = (pkg, oracle, synthetic)
    out = {}
    for lf, form in ((False, "kf"), (True, "pf")):
        out["A/designed/" + form] = designed_frame(*env, lf)[0]
        out["A/recovery/" + form] = recovery_frame(*env, lf)[0]
    for lf, form in ((False, "kf"), (True, "pf")):
        for n, w in small_frames(*env, lf).items():
            out["B/%s/%d" % (form, n)] = w
    for (n, r), w in inlier_boundary_frames(*env).items():
        out["C/%d/rec_init=%d" % (n, r)] = w
    for seed in (0, 1):
        for lf, form in ((False, "kf"), (True, "pf")):
            for n, w in stride_frames(*env, seed, lf).items():
                out["D/%d/%s/%d" % (seed, form, n)] = w
    out["E"] = first_factorisation_failure(*env)
    out["F"] = mid_round_failure(*env)
    out["G"], out["G/plain"] = active_prior_weight(*env)
    out["H"], out["H/plain"] = skewed_preintegration(*env)
    for w in out.values():
        assert_clean(w)
    return out
