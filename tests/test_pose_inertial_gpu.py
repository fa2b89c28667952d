"""GPU parity of Optimizer::PoseInertialOptimizationLastKeyFrame / LastFrame (VERDICT r1 row a10')
with the oracle: same outlier flags and inlier counts, frame state within 1e-4 relative (BASELINE.json's bar for SE3 poses), the new
prior's Hessian within 1e-4 of its scale.  Both sides get the product's pre-integration (row a11), so the test isolates the optimiser."""
import numpy as np
import pytest

from pose_inertial_cases import RTOL, check, problem, rel  # shared with the directed tests (test_pose_inertial_gates_gpu.py)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("last_frame", [False, True])
@pytest.mark.parametrize("seed,n_points", [(0, 500), (1, 900), (2, 150)])
def test_pose_inertial_optimisation(pkg, oracle, synthetic, seed, n_points, last_frame):
    w = problem(pkg, oracle, synthetic, seed, last_frame, n_points=n_points)
    want = oracle.pose_inertial(w["cur33"], w["other33"], last_frame, w["prior246"], w["calib24"], w["pre298"], w["pre298"], w["Xw"], w["edges"], w["close"],
                                w["cam"])
    got = pkg.capi.pose_inertial_optimization_batch([dict(w, edges=w["packed_edges"])], w["calib24"], w["cam"])[0]
    check(got, want)
    assert got[5][2] > 0.8 * len(w["edges"]) and got[2][w["gross"]].mean() > 0.9
    # it optimises: the body position moves towards the truth
    assert np.linalg.norm(got[0][21:24] - w["cur33_true"][21:24]) < 0.6 * np.linalg.norm(w["cur33"][21:24] - w["cur33_true"][21:24])
    assert np.array_equal(got[1], w["other33"]) != last_frame


def test_batch_of_mixed_frames(pkg, oracle, synthetic):
    """Keyframe and previous-frame forms, different sizes, bRecInit and an edge-less frame in one launch: every frame as if alone."""
    ws = [problem(pkg, oracle, synthetic, 10, False, n_points=300), problem(pkg, oracle, synthetic, 11, True, n_points=700),
          problem(pkg, oracle, synthetic, 12, True, n_points=40, outlier_frac=0.3), problem(pkg, oracle, synthetic, 13, False, n_points=30, outlier_frac=0.3)]
    ws[3]["rec_init"] = True
    got = pkg.capi.pose_inertial_optimization_batch([dict(w, edges=w["packed_edges"]) for w in ws], ws[0]["calib24"], ws[0]["cam"])
    for w, g in zip(ws, got):
        want = oracle.pose_inertial(w["cur33"], w["other33"], w["last_frame"], w["prior246"], w["calib24"], w["pre298"], w["pre298"], w["Xw"], w["edges"],
                                    w["close"], w["cam"], rec_init=bool(w.get("rec_init")))
        check(g, want)
    assert got[2][5][2] < 30 or got[3][5][2] < 30  # the recovery pass ran for at least one of the two small frames
    # no edges: the inertial terms alone move the state; nothing crashes, nothing is an outlier
    e0 = dict(ws[0], edges=ws[0]["packed_edges"][:0], Xw=ws[0]["Xw"][:0], close=ws[0]["close"][:0])
    g = pkg.capi.pose_inertial_optimization_batch([e0], ws[0]["calib24"], ws[0]["cam"])[0]
    want = oracle.pose_inertial(ws[0]["cur33"], ws[0]["other33"], False, None, ws[0]["calib24"], ws[0]["pre298"], ws[0]["pre298"], np.zeros((0, 3)), np.zeros((0, 6)),
                                np.zeros(0, np.uint8), ws[0]["cam"])
    assert g[4] == want[4] == 0 and rel(g[0][:24], want[0][:24]) < RTOL


def test_pose_inertial_argument_errors(pkg, oracle, synthetic):
    w = problem(pkg, oracle, synthetic, 0, True, n_points=100)
    bad = dict(w, edges=w["packed_edges"], prior246=None)  # the previous-frame form needs the previous frame's prior
    with pytest.raises(pkg.capi.Tc2liError):
        pkg.capi.pose_inertial_optimization_batch([bad], w["calib24"], w["cam"])
    assert pkg.capi.pose_inertial_optimization_batch([], w["calib24"], w["cam"]) == []


def test_a_batch_beyond_256_frames_takes_the_two_per_cu_kernel_with_the_same_bits(pkg, oracle, synthetic):
    """More than 256 frames run k_pose_inertial_batch (the same body held to two wavefronts per SIMD): every frame's result is the one the
    frame gets in a small batch (k_pose_inertial), bit for bit."""
    ws = [problem(pkg, oracle, synthetic, 20, True, n_points=400), problem(pkg, oracle, synthetic, 21, False, n_points=250),
          problem(pkg, oracle, synthetic, 22, True, n_points=60, outlier_frac=0.3)]
    items = [dict(w, edges=w["packed_edges"]) for w in ws]
    small = pkg.capi.pose_inertial_optimization_batch(items, ws[0]["calib24"], ws[0]["cam"])
    big = pkg.capi.pose_inertial_optimization_batch([items[k % 3] for k in range(258)], ws[0]["calib24"], ws[0]["cam"])
    for k in (0, 1, 2, 128, 255, 256, 257):
        s, b = small[k % 3], big[k]
        assert np.array_equal(b[0], s[0]) and np.array_equal(b[1], s[1]) and np.array_equal(b[2], s[2]) and np.array_equal(b[3], s[3])
        assert b[4] == s[4] and b[5] == s[5] and b[6] == s[6]
