"""CPU tests of the MLPnP RANSAC stage: the restatement (tests/mlpnp_ref.py) against itself, then tc2li_host_mlpnp_ransac_batch against
the restatement on generated problems (tests/mlpnp_cases.py states the comparison rule).  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import mlpnp_cases as K
import mlpnp_ref as ref


# ---- the restatement against itself ------------------------------------------------------------------------------------------------
def test_jacobian_against_central_differences():
    rng = np.random.default_rng(0)
    for trial in range(20):
        x = np.concatenate([rng.normal(size=3) * rng.uniform(0.01, 1.5), rng.uniform(-3, 3, 3)])
        pts = [rng.uniform(-5, 5, 3) + np.array([0, 0, 12.0]) for _ in range(6)]
        nulls = [ref.null_space(np.array([rng.uniform(-0.8, 0.8), rng.uniform(-0.3, 0.3), 1.0]), trial % 2) for _ in range(6)]
        r, J = ref.residuals_and_jacs(x, pts, nulls, "analytic")
        r2, Jfd = ref.residuals_and_jacs(x, pts, nulls, "fd")
        assert np.array_equal(r, r2)
        # central differences with h = 1e-6: truncation h^2 |f'''| / 6 ~ 1e-12, rounding eps / h ~ 2e-10
        assert np.abs(J - Jfd).max() < 5e-9, np.abs(J - Jfd).max()


def test_null_space_bases_are_orthonormal_complements():
    rng = np.random.default_rng(1)
    for basis in (0, 1):
        for _ in range(20):
            f = np.array([rng.uniform(-1, 1), rng.uniform(-0.5, 0.5), 1.0])
            r, s = ref.null_space(f, basis)
            G = np.stack([r, s, f / np.linalg.norm(f)])
            assert np.abs(G @ G.T - np.eye(3)).max() < 1e-15


def test_rank_rule():
    rng = np.random.default_rng(2)
    P = rng.normal(size=(3, 6))
    assert ref.fullpiv_rank(P @ P.T) == 3
    P[2] = 0.0
    assert ref.fullpiv_rank(P @ P.T) == 2
    P[1] = 0.0
    assert ref.fullpiv_rank(P @ P.T) == 1
    # a plane that does not pass through the origin is not "planar": the second moment is uncentred (MLPnPsolver.cpp:361)
    P = rng.normal(size=(3, 6)); P[2] = 4.0
    assert ref.fullpiv_rank(P @ P.T) == 3


def test_noise_free_iterations_recover_the_pose():
    for seed in range(3):
        pr = K.make_problem(100 + seed, 40, 0.0, 0.0)
        for variant in K.VARIANTS:
            sv = ref.Solver(pr["keys"], pr["match"], pr["Xw"], K.LEVEL_SIGMA2, K.CAM4, dict(max_iterations=6), **variant)
            # every iteration of a noise-free problem has all N inliers, so each call returns after one; keep calling
            d = 0
            for it in range(6):
                o = sv.iterate(1, pr["draws"][d:])
                d += o["used"]
                assert o["found"] == 1 and o["n_inliers"] == sv.N and len(o["log"]) == 1
                # keypoints are float32 pixels: 2^-14 px of rounding at u ~ 1000 over fx ~ 700 is 1e-7 rad; poorly spread minimal sets amplify it
                assert np.abs(o["Rt"][:, :3] - pr["true_Rt"][:, :3]).max() < 1e-4 and np.abs(o["Rt"][:, 3] - pr["true_Rt"][:, 3]).max() < 1e-2, (seed, it)


def test_noise_free_planar_scene():
    """The planar branch as written does not recover every pose: its scale is taken from tmp after transposeInPlace (:521-524), so the
    linear translation is off by a factor and Gauss-Newton has to make up for it or give up (:724).  What holds: the branch is taken, and an
    iteration that explains every correspondence is at the true pose as closely as the inlier bound allows."""
    taken = full = 0
    for seed in range(3):
        pr = K.make_problem(200 + seed, 40, 0.0, 0.0, planar=True)
        sv = ref.Solver(pr["keys"], pr["match"], pr["Xw"], K.LEVEL_SIGMA2, K.CAM4)
        rng = np.random.default_rng(seed)
        for it in range(8):
            pick = rng.permutation(sv.N)[:6]
            Rt, planar = ref.compute_pose(sv.f[pick], sv.Xw[pick].astype(np.float64))
            assert planar
            taken += 1
            if sv.check_inliers(Rt)[1] == sv.N:
                full += 1
                # an inlier is within sqrt(5.991) * 1.2^octave <= 8.8 px: 8.8 / 718.9 = 1.2e-2 rad, and that angle at 4 m of depth
                assert np.abs(Rt[:, :3] - pr["true_Rt"][:, :3]).max() < 2e-2 and np.abs(Rt[:, 3] - pr["true_Rt"][:, 3]).max() < 0.1, (seed, it)
    print("planar: %d of %d noise-free iterations explain every correspondence" % (full, taken))


def test_iterations_restatement():
    for N in (20, 21, 57, 100, 300):
        assert ref.ransac_parameters(N) == (N // 2, 35)
    assert ref.ransac_parameters(10) == (10, 1)
    assert ref.ransac_parameters(15) == (10, 14)      # epsilon = 10 / 15: ceil(log(0.01) / log(1 - 0.2963)) = ceil(13.1)
    assert ref.ransac_parameters(8)[0] == 10          # N below min_inliers: iterate() gives up at once


# ---- the host entry against the restatement ---------------------------------------------------------------------------------------------
def test_mlpnp_iterations(pkg):
    for N in (20, 21, 57, 100, 300):
        assert pkg.mlpnp_iterations(N) == (N // 2, 35)
    assert pkg.mlpnp_iterations(10) == (10, 1)
    for N in range(0, 120):
        assert pkg.mlpnp_iterations(N) == ref.ransac_parameters(N), N
    p = pkg.mlpnp_params(probability=0.9, min_inliers=8, max_iterations=20, epsilon=0.3)
    for N in range(6, 80):
        assert pkg.mlpnp_iterations(N, p) == ref.ransac_parameters(N, probability=0.9, min_inliers=8, max_iterations=20, epsilon=0.3), N


def _run(pkg, problems, host=True, params=None, **kw):
    return pkg.mlpnp_ransac_batch(problems, K.LEVEL_SIGMA2, K.CAM5, params=pkg.mlpnp_params(**(params or {})), host=host, **kw)


def _check_family(pkg, problems, report, host=True):
    got = _run(pkg, problems, host)
    for p, pr in enumerate(problems):
        K.compare_call(K.solvers_for(pr), pr["n_iterations"], pr["draws"], got, p, report)
    return got


FAMILY_N = [15, 22, 31, 47, 64, 65, 90, 128, 150, 200, 257, 300]


def test_host_easy_family(pkg):
    report = K.new_report()
    got = _check_family(pkg, [K.easy(1000 + i, N) for i, N in enumerate(FAMILY_N)], report)
    K.check_left_out(report)
    assert got["found"].all() and not got["no_more"].any()          # the early return
    print("easy: s max %.3g, distance max %.3g, left out %d" % (max(report["s"]), max(report["dist"]), sum(report["left_out"])))


def test_host_hard_family(pkg):
    report = K.new_report()
    got = _check_family(pkg, [K.hard(2000 + i, N) for i, N in enumerate(FAMILY_N)], report)
    K.check_left_out(report)
    assert got["no_more"].any()                                     # the exhausted solver, with or without a best so far
    print("hard: s max %.3g, distance max %.3g, left out %d, exhausted %d, best-so-far %d"
          % (max(report["s"]), max(report["dist"] or [0]), sum(report["left_out"]), int(got["no_more"].sum()), int((got["no_more"] & got["found"]).sum())))


def test_host_planar_scene(pkg):
    """World z exactly 0: every minimal set takes the planar branch (9 columns, four candidate poses).  The branch depends on the signs of
    the planar frame's eigenvectors and of result1, which are the decomposition's choice: the library normalises them as the restatement
    does (largest entry positive), so the comparison is with the restatement's default signs."""
    problems = [K.make_problem(3000 + i, N, 0.15, 0.3, planar=True) for i, N in enumerate([15, 40, 100, 260])]
    for pr in problems:
        f = (np.stack([pr["keys"]["x"], pr["keys"]["y"]], 1)[pr["match"] >= 0][:6].astype(np.float64) - K.CAM4[2:]) / K.CAM4[:2]
        X = pr["Xw"][pr["match"][pr["match"] >= 0][:6]].astype(np.float64)
        assert ref.compute_pose(np.hstack([f, np.ones((6, 1))]), X)[1]
    report = K.new_report()
    _check_family(pkg, problems, report)
    K.check_left_out(report)
    assert not any(report["left_out"])


def test_host_fewer_matches_than_min_inliers(pkg):
    pr = K.easy(4000, 9)
    got = _run(pkg, [pr])
    assert (got["found"][0], got["no_more"][0], got["n_inliers"][0], got["iterations"][0]) == (0, 1, 0, 0)
    assert not got["inlier"].any() and np.array_equal(got["pose7"][0], np.array([0, 0, 0, 1, 0, 0, 0], np.float32))
    o = K.solvers_for(pr)[0].iterate(5, pr["draws"])
    assert (o["found"], o["no_more"]) == (0, 1)


def test_host_as_many_matches_as_min_inliers(pkg):
    """N == min_inliers: one iteration at most, and Refine() needs MORE than min_inliers, so the only way to a pose is the best so far."""
    report = K.new_report()
    problems = [K.make_problem(4100 + i, 10, 0.0, 0.1) for i in range(4)]
    got = _check_family(pkg, problems, report)
    assert np.array_equal(got["iterations"], [5, 5, 5, 5]) and got["no_more"].all()    # max(1, n_iterations = 5) passes (:95 is an or)
    K.check_left_out(report)


def test_host_resumed_solver(pkg):
    """A second and a third call on the same state, past max_iterations: each runs n_iterations more (:95)."""
    report = K.new_report()
    # 70 % gross outliers leave fewer than min_inliers = N / 2 that any pose can explain: those two solvers run to 35, 40, 45 iterations
    problems = [K.make_problem(5200 + i, N, 0.7, 0.3) for i, N in enumerate([40, 100])] + [K.hard(5000 + i, N) for i, N in enumerate([30, 60, 120, 240])] \
        + [K.easy(5100, 80)]
    solvers = [K.solvers_for(pr) for pr in problems]
    used = [0] * len(problems)
    for call in range(3):
        batch = [dict(pr, draws=pr["draws"][used[i]:]) for i, pr in enumerate(problems)]
        got = _run(pkg, batch)
        for i, pr in enumerate(problems):
            before = solvers[i][0].iterations
            K.compare_call(solvers[i], pr["n_iterations"], batch[i]["draws"], got, i, report)
            used[i] += 6 * (solvers[i][0].iterations - before)
            problems[i] = K.state_of(got, i, pr)
        assert [int(v) for v in got["iterations"][:2]] == [35 + 5 * call] * 2 and got["no_more"][:2].all() and not got["found"][:2].any()
    K.check_left_out(report)


def test_host_matches_skip_keypoints(pkg):
    """inlier is per frame keypoint: unmatched keypoints stay 0 and the capacity may exceed the frame."""
    pr = K.make_problem(6000, 50, 0.15, 0.3, n_unmatched=70)
    got = _run(pkg, [pr], capacity=160)
    report = K.new_report()
    K.compare_call(K.solvers_for(pr), 5, pr["draws"], got, 0, report)
    assert not report["left_out"][0] and got["found"][0] == 1
    assert not got["inlier"][0][:120][pr["match"] < 0].any() and got["inlier"].shape == (1, 160)


def test_host_invalid_arguments(pkg):
    pr = K.easy(7000, 40)
    with pytest.raises(Exception, match="min_set"):
        _run(pkg, [pr], params=dict(min_set=4))
    with pytest.raises(Exception, match="draws"):
        _run(pkg, [dict(pr, draws=pr["draws"][:6 * 35 - 1])])          # a fresh solver may run max(35, 5) iterations
    _run(pkg, [dict(pr, draws=pr["draws"][:6 * 35])])
    big = pr["draws"].copy(); big[7] = 2 ** 31
    with pytest.raises(Exception, match="rand"):
        _run(pkg, [dict(pr, draws=big)])
    bad = pr["match"].copy(); bad[np.nonzero(bad >= 0)[0][3]] = 40
    with pytest.raises(Exception, match="match"):
        _run(pkg, [dict(pr, match=bad)])
    bad[bad == 40] = -2
    with pytest.raises(Exception, match="match"):
        _run(pkg, [dict(pr, match=bad)])


def test_device_entry_without_a_device_is_an_error(pkg):
    """No quiet fall-back to the host arithmetic: without a GPU the device entry fails; with one it answers."""
    pr = K.easy(7100, 30)
    if pkg.device_count() > 0:
        assert _run(pkg, [pr], host=False)["found"].shape == (1,)
    else:
        with pytest.raises(Exception, match="no HIP device"):
            _run(pkg, [pr], host=False)


def test_new_kernels_use_no_scratch(tmp_path):
    """The resource report of the compiler for csrc/mlpnp_kernels.hip: three kernels, no private memory in any of them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tc2li-slam_amd", "csrc", "mlpnp_kernels.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "mlpnp_kernels.o")],
                         capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    assert len(names) == 3 and all(any(k in n for n in names) for k in ("k_mlpnp_solve", "k_mlpnp_inliers", "k_mlpnp_select")), names
    assert scratch == [0, 0, 0], list(zip(names, scratch))
