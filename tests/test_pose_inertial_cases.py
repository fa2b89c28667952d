"""The frames of pose_inertial_cases.py are what they claim to be: shown with the oracle alone, before any GPU sees them
(test_pose_inertial_gates_gpu.py compares the product with the oracle on the same frames).

Margins.  The device and the oracle agree on a state within 1e-4 (relative); a decision they must share needs room for that.
  * chi2 of a designed edge against its gate, recomputed in numpy at the oracle's final pose: at least 2 % is asked, more than a
    hundred times 1e-4.  Measured (chi2 / gate - 1, keyframe form | previous-frame form):
      mono 5.991            -8.8 %, +7.8 %   | -10.6 %, +7.0 %
      mono, close 8.9865    -28 %, -4.9 %, +4.1 % | -30 %, -6.6 %, +3.5 %
      stereo 7.815          -6.0 %, +5.6 %   | -8.7 %, +4.0 %
      recovery 18 / 24      -5.6 %, -2.8 %, +5.5 %, -4.2 %, +4.1 % | -5.6 %, -2.9 %, +4.8 %, -5.2 %, +3.3 %
                            (the second one is also 2.9 % | 2.8 % above 17)
    The pushed edge of case B ends between 10.93 and 13.79, inside 9.8 .. 15.6 by 11 % or more, and the pushed edge of case C at 14.09,
    between 7.815 and 24.
  * the pivot that decides a factorisation (the smallest when all are positive, the first that is not otherwise) against the
    largest term it is the sum of.  The largest difference between device and oracle recorded for such sums is 3.0e-8 of their size
    (the inertial Hessian, commit 91c83b0); four orders of magnitude over it is PIVOT_CLEARANCE = 3e-4.  Measured pivot / largest term:
      E  -1.001 in each of the four factorisations (unknown 27, the previous state's accelerometer bias x)
      F  +2.9e-3, -0.70 | +3.4e-3, -0.21 | +2.7e-3, -0.58 | +3.4e-3, -1.65e-2 (four rounds of a success and a failure; unknowns 21 =
         the previous state's velocity x for the successes, 21, 21, 19, 18 for the failures)
      G  +1.87e-2 to +2.05e-2 in all 40 (unknown 21)
    With the plain IMU noise of synthetic.IMU_NOISE the same figures are 3e-7 for the successes of F and 2e-6 for G -- the smallest
    pivot is then the previous state's velocity, 4e2 left of two terms of 2e7 -- which is why cases E to G integrate with a hundred
    times the white noise (pose_inertial_cases._failure_base).  Pivots other than the deciding one are not held to the bar: in every
    previous-frame system some pivot of ~1e3 is what two terms of ~1e9 leave (ratio ~1e-6), far from zero in its own size."""
import numpy as np
import pytest

import pose_inertial_cases as pc

PIVOT_CLEARANCE = 1e4 * 3.0e-8
CHI2_MARGIN = 0.02


@pytest.fixture(scope="module")
def env(pkg, oracle, synthetic):
    return pkg, oracle, synthetic


def run(oracle, w):
    pc.assert_clean(w)
    return pc.run_oracle(oracle, w)


def gate_distance(chi2, gate):
    return chi2 / gate - 1.0


@pytest.mark.parametrize("last_frame", [False, True])
def test_designed_edges_fall_on_their_side_of_the_gates(env, last_frame):
    w, idx = pc.designed_frame(*env, last_frame)
    cur, _, outlier, _, _, counts, d = run(env[1], w)
    assert len(w["edges"]) > 128 and not d["solver_failed"] and d["rounds"] == (10, 10, 10, 10)
    assert tuple(outlier[idx]) == pc.DESIGNED_FLAGS
    assert outlier.sum() == sum(pc.DESIGNED_FLAGS)  # every other edge is an inlier
    chi2 = pc.edge_chi2(cur, w)
    for i, gate, flag, kind in zip(idx, pc.DESIGNED_GATE, pc.DESIGNED_FLAGS, pc.DESIGNED_KIND):
        if kind == "behind":
            # an inlier by its chi2, an outlier by its depth alone
            assert chi2[i] < 0.1 and pc.project(cur, w["Xw"][i:i + 1], w["cam"])[3][0] < -7.0 and flag == 1
            continue
        dist = gate_distance(chi2[i], gate)
        print(kind, gate, "chi2 %.4f" % chi2[i], "distance %+.3f" % dist)
        assert abs(dist) >= CHI2_MARGIN and (dist > 0) == bool(flag)
    # the close rule and the plain rule disagree on the edges between the two gates: 6.5 is out when far and in when close
    assert outlier[idx[1]] == 1 and outlier[idx[2]] == 0
    assert np.abs(chi2[:idx[0]]).max() < 0.5


@pytest.mark.parametrize("last_frame", [False, True])
def test_recovery_twin_falls_on_its_side_of_18_and_24(env, last_frame):
    w, idx = pc.recovery_frame(*env, last_frame)
    cur, _, outlier, _, rv, counts, d = run(env[1], w)
    assert len(w["edges"]) < 30 and counts[2] == len(w["edges"]) - len(idx)  # all five are outliers after round 3, so the recovery pass runs
    assert tuple(outlier[idx]) == pc.RECOVERY_FLAGS and outlier.sum() == 2 and counts[1] == 2 and rv == len(w["edges"]) - 2
    chi2 = pc.edge_chi2(cur, w)
    for i, gate, flag in zip(idx, pc.RECOVERY_GATE, pc.RECOVERY_FLAGS):
        dist = gate_distance(chi2[i], gate)
        print(gate, "chi2 %.4f" % chi2[i], "distance %+.3f" % dist)
        assert abs(dist) >= CHI2_MARGIN and (dist > 0) == bool(flag)
    assert chi2[idx[1]] > 17.0 * (1 + CHI2_MARGIN)  # recovered by 18, not by 17
    # without the recovery pass all five stay outliers
    w2 = dict(w, rec_init=True)
    assert tuple(run(env[1], w2)[2][idx]) == (1, 1, 1, 1, 1)


@pytest.mark.parametrize("last_frame", [False, True])
def test_small_graphs_straddle_the_ten_edge_break(env, last_frame):
    frames = pc.small_frames(*env, last_frame)
    graph_extra = 4 if last_frame else 3  # inertial, two random walks, and the prior in the previous-frame form
    seen = set()
    p = pc.SMALL_PUSHED
    for n, w in frames.items():
        assert len(w["edges"]) == n
        r = run(env[1], w)
        d = r[6]
        breaks = n + graph_extra < 10
        assert d["rounds"] == ((10, -1, -1, -1) if breaks else (10, 10, 10, 10)) and not d["solver_failed"]
        seen.add((n + graph_extra, breaks))
        if n > p:
            # the pushed edge: an inlier where only round 0 ran (15.6), an outlier where round 1 ran too (9.8), 2 % clear of both and of
            # the 24 below which the recovery pass (fewer than 30 inliers) clears its flag again: it shows in the inlier count alone
            print(n, "pushed edge chi2 %.4f, inliers %d" % (d["chi2"][p], r[5][2]))
            assert 9.8 * (1 + CHI2_MARGIN) < d["chi2"][p] < 15.6 * (1 - CHI2_MARGIN)
            assert r[5][2] == (n if breaks else n - 1) and r[2].sum() == 0 and r[5][1] == 0
    assert (9, True) in seen and (10, False) in seen  # both sides of the boundary
    last_breaking = 5 if last_frame else 6
    assert last_breaking in frames and last_breaking + 1 in frames


def test_twenty_nine_and_thirty_inliers(env):
    frames = pc.inlier_boundary_frames(*env)
    res = {k: run(env[1], w) for k, w in frames.items()}
    (n29, n30) = sorted({k[0] for k in frames})
    for n, inliers in ((n29, 29), (n30, 30)):
        assert res[(n, False)][5][2] == res[(n, True)][5][2] == inliers
        for r in (False, True):
            assert not res[(n, r)][6]["solver_failed"] and res[(n, r)][6]["rounds"] == (10, 10, 10, 10)
    p = pc.BOUNDARY_PUSHED
    # the pushed edge is an outlier after round 3 in all four runs, and the recovery pass would clear it: 2 % clear of 7.815 and of 24
    for k, r in res.items():
        if k != (n29, False):
            assert r[2][p] == 1 and 7.815 * (1 + CHI2_MARGIN) < r[6]["chi2"][p] < 24.0 * (1 - CHI2_MARGIN)
    # 29 inliers: the pass runs unless bRecInit -- the pair differs in that flag; 30 inliers: it does not run, the pair is the same
    assert res[(n29, False)][2][p] == 0 and 7.815 * (1 + CHI2_MARGIN) < res[(n29, False)][6]["chi2"][p] < 24.0 * (1 - CHI2_MARGIN)
    assert np.sum(res[(n29, False)][2] != res[(n29, True)][2]) == 1 and res[(n29, False)][4] == res[(n29, True)][4] + 1
    assert np.array_equal(res[(n30, False)][2], res[(n30, True)][2]) and res[(n30, False)][4] == res[(n30, True)][4]


@pytest.mark.parametrize("last_frame", [False, True])
@pytest.mark.parametrize("seed", [0, 1])
def test_stride_frames_keep_an_outlier_beyond_index_255(env, seed, last_frame):
    frames = pc.stride_frames(*env, seed, last_frame)
    assert tuple(frames) == pc.STRIDE_N
    for n, w in frames.items():
        assert len(w["edges"]) == n
    r = run(env[1], frames[257])
    assert r[2][256] == 1 and r[2][128:256].any() and r[2][:128].any() and not r[6]["solver_failed"]
    # the same edges, cut elsewhere: an outlier in the last trip of the 128-lane loop too
    assert run(env[1], frames[129])[2][:129].any()


def pivot_ratios(d):
    r = d["pivot"] / d["pivot_scale"]
    print("pivot / largest term:", " ".join("%+.3g" % x for x in r), "| unknowns", d["pivot_index"])
    return r


def test_failure_at_the_first_factorisation(env):
    w = pc.first_factorisation_failure(*env)
    cur, oth, outlier, prior, rv, counts, d = run(env[1], w)
    assert d["solver_failed"] and d["rounds"] == (1, 1, 1, 1)
    r = pivot_ratios(d)
    assert len(r) == 4 and (r <= -PIVOT_CLEARANCE).all() and (d["pivot_index"] == 27).all()
    # no increment was ever accepted: the zero increment is applied, the states stay, the edges are classified where they started
    assert np.array_equal(cur[21:24], w["cur33"][21:24]) and np.array_equal(oth[21:24], w["other33"][21:24])
    assert np.isfinite(prior).all() and 0 < counts[1] < counts[0]


def test_failure_after_an_accepted_increment(env):
    w = pc.mid_round_failure(*env)
    cur, oth, outlier, prior, rv, counts, d = run(env[1], w)
    assert d["solver_failed"] and d["rounds"][0] >= 2 and max(d["rounds"]) < 10
    r = pivot_ratios(d)
    assert (np.abs(r) >= PIVOT_CLEARANCE).all()
    # a round is: successes, then one failure that ends it
    k = 0
    for its in d["rounds"]:
        assert (r[k:k + its - 1] > 0).all() and r[k + its - 1] < 0
        k += its
    assert k == len(r)
    # the prior's weight: small while the previous state is 2 m from the prior's mean, 1 when the first failure happens
    assert d["prior_chi2"][0] > 100 * 25.0 and d["prior_chi2"][d["rounds"][0] - 1] < 25.0
    # the increment that is applied once more is not zero: both states moved, by far more than the comparison's tolerance
    assert np.linalg.norm(cur[21:24] - w["cur33"][21:24]) > 100 * pc.RTOL and np.linalg.norm(oth[21:24] - w["other33"][21:24]) > 100 * pc.RTOL
    assert np.isfinite(prior).all() and np.isfinite(cur).all() and np.isfinite(oth).all()


def test_active_prior_weight(env):
    w, plain = pc.active_prior_weight(*env)
    got, ref = run(env[1], w), run(env[1], plain)
    d = got[6]
    assert not d["solver_failed"] and d["rounds"] == (10, 10, 10, 10) and not ref[6]["solver_failed"]
    assert d["prior_chi2"][0] > 25.0 and d["prior_chi2"].min() > 25.0 and ref[6]["prior_chi2"].max() < 25.0
    r = pivot_ratios(d)
    assert len(r) == 40 and (r >= PIVOT_CLEARANCE).all()
    diff = np.abs(got[1][21:24] - ref[1][21:24]).max()
    print("previous state against the plain prior's: %.3g m" % diff)
    assert diff > 100 * pc.RTOL
    eig = np.linalg.eigvalsh(w["prior246"][21:].reshape(15, 15))
    assert eig.min() > 0  # positive definite caller data


def test_skewed_preintegration_takes_the_jacobi_path(env):
    w, plain = pc.skewed_preintegration(*env)
    dR = w["pre"].fields()["dR"]
    assert pc.orthogonality_defect(dR) > 2e-3 > 1e-3 > 1e-5 > pc.orthogonality_defect(plain["pre"].fields()["dR"])
    # the bias update multiplies by a rotation: the defect's Frobenius norm stays, so its largest entry stays above a third of it
    assert np.linalg.norm(dR.astype(np.float64).T @ dR.astype(np.float64) - np.eye(3)) / 3 > 1e-3
    assert np.array_equal(w["pre298"][1:10], dR.ravel())
    got, ref = run(env[1], w), run(env[1], plain)
    for a, b in zip(got[:4], ref[:4]):
        assert np.isfinite(a).all()
    assert pc.rel(got[0][:24], ref[0][:24]) < 1e-3 and np.allclose(got[0][24:], ref[0][24:], rtol=1e-3, atol=1e-6)
    assert not got[6]["solver_failed"]


def test_details_leave_the_six_tuple_alone(env):
    w = pc.small_frames(*env, True)[10]
    a, b = pc.run_oracle(env[1], w, details=False), pc.run_oracle(env[1], w, details=True)
    assert len(a) == 6 and len(b) == 7
    for x, y in zip(a, b[:6]):
        assert np.array_equal(np.asarray(x), np.asarray(y))
    d = b[6]
    assert len(d["pivot"]) == len(d["pivot_scale"]) == len(d["prior_chi2"]) == sum(k for k in d["rounds"] if k > 0) and len(d["chi2"]) == 10
