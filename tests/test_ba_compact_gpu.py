"""The lock-step batch's compact grids: a launch gives every window the workgroups ITS sizes need (BaPhase::first_block), so windows of
very different sizes share a launch.  A window must give the same bits in such a group as in a call of its own."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4  # the tolerance tests/test_ba_gpu.py uses for optimised SE3 poses


def rel_pose_err(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def window_dict(pkg, synthetic, w, lidar_keyframes=0, cloud_points=1200, weight=1.0, **kw):
    d = dict(poses=w["poses"], fixed=w["fixed"], points=w["points"], edges=pkg.pack_ba_edges(w["edges"]), **kw)
    if lidar_keyframes:
        last = len(w["poses"]) - 1
        win = list(range(last, last - lidar_keyframes, -1))
        d.update(win_pose=win, clouds=synthetic.ba_window_clouds(w, win, n_points=cloud_points), Tcl7=synthetic.TCL7, weight=weight)
    return d


def varied_dict(pkg, synthetic, w, **kw):
    d = dict(poses=w["poses"], fixed=w["fixed"], points=w["points"], edges=pkg.pack_ba_edges(w["edges"]), iterations=w["iterations"])
    if w["win_pose"]:
        d.update(win_pose=w["win_pose"], clouds=w["clouds"], Tcl7=synthetic.TCL7, weight=w["weight"])
    d.update(kw)
    return d


def results_of(batch, i):
    r = batch.result(i)
    return tuple(np.array(a, copy=True) for a in r[:4]) + (int(batch.results[i]), r[4].iterations, r[4].trials, r[4].initial_chi2, r[4].final_chi2,
                                                           r[4].final_lambda, r[5].n_planes, r[5].residual, r[5].chi2, r[5].hessian_evaluations)


def assert_same(got, want, what):
    for k, name in enumerate(("poses", "points", "edge chi2", "depth flags")):
        assert np.array_equal(got[k], want[k]), (what, name)
    assert got[4:] == want[4:], (what, got[4:], want[4:])


def alone(pkg, d, cam):
    """The window in a call of its own."""
    b = pkg.capi.BaBatch([d], cam)
    b.run_group(0)
    return results_of(b, 0)


def test_unequal_windows_in_one_group(pkg, oracle, synthetic):
    """One window of 6 free + 4 fixed keyframes and 400 points beside five of 2 free + 2 fixed keyframes and 40 points: the small ones own one
    workgroup of a launch where the large one owns several.  The large window and one small window carry a LiDAR edge, the others none."""
    big = synthetic.ba_window(3, n_opt=6, n_fix=4, n_points=400, pose_noise=(0.1, 0.01))
    smalls = [synthetic.ba_window(60 + s, n_opt=2, n_fix=2, n_points=40, pose_noise=(0.1, 0.01)) for s in range(5)]
    cam = big["cam"]
    dicts = [window_dict(pkg, synthetic, smalls[0]), window_dict(pkg, synthetic, smalls[1], lidar_keyframes=2),
             window_dict(pkg, synthetic, big, lidar_keyframes=4), window_dict(pkg, synthetic, smalls[2]), window_dict(pkg, synthetic, smalls[3]),
             window_dict(pkg, synthetic, smalls[4])]
    assert len(big["edges"]) > 4 * 256 and all(len(s["edges"]) <= 256 for s in smalls)  # several blocks of edges against one
    batch = pkg.capi.BaBatch(dicts, cam)
    assert batch.run_group(0) == len(dicts)
    for i, d in enumerate(dicts):
        assert_same(results_of(batch, i), alone(pkg, d, cam), i)
    # the large window against the oracle
    d = dicts[2]
    want = oracle.local_ba_lidar(big["poses"], big["fixed"], big["points"], big["edges"], cam, d["win_pose"], d["clouds"], synthetic.TCL7, 1.0)
    poses, pts, chi2, dpos, stats, ls = batch.result(2)
    assert batch.results[2] == want[4] and stats.trials == int(want[5]["trials"].sum()) and ls.n_planes == want[6]
    assert abs(stats.final_chi2 - want[5]["chi2"][-1]) <= 1e-6 * want[5]["chi2"][-1]
    for k in range(len(poses)):
        assert rel_pose_err(poses[k], want[0][k]) < POSE_RTOL, k
    assert np.allclose(pts, want[1], rtol=POSE_RTOL, atol=1e-6) and np.array_equal(dpos, want[3])


def test_a_wide_window_beside_a_narrow_one(pkg, synthetic):
    """22-24 free keyframes (two workgroups per part of the lean Schur product, the widest solve kernel) beside at most 6."""
    wide = narrow = None
    for seed in range(64):
        w = synthetic.ba_window_varied(seed)
        if wide is None and 22 <= w["params"]["n_opt"] <= 24:
            wide = w
        if narrow is None and w["params"]["n_opt"] <= 6:
            narrow = w
        if wide is not None and narrow is not None:
            break
    assert wide is not None and narrow is not None
    cam = wide["cam"]
    dicts = [varied_dict(pkg, synthetic, narrow), varied_dict(pkg, synthetic, wide)]
    batch = pkg.capi.BaBatch(dicts, cam)
    assert batch.run_group(0) == 2
    for i, d in enumerate(dicts):
        assert_same(results_of(batch, i), alone(pkg, d, cam), i)


def test_windows_at_different_paces(pkg, synthetic):
    """Heavy LiDAR edges whose steps are rejected (seeds 17 and 39 of the benched windows), a window interrupted after two iterations
    and an ordinary one: the windows of the group leave the linearisation and the trial lists at different rounds."""
    ws = [synthetic.ba_window_varied(s) for s in (17, 39, 1, 2)]
    assert ws[0]["weight"] > 1 and ws[1]["weight"] > 1
    cam = ws[0]["cam"]
    dicts = [varied_dict(pkg, synthetic, ws[0]), varied_dict(pkg, synthetic, ws[1]), varied_dict(pkg, synthetic, ws[2], iterations=2),
             varied_dict(pkg, synthetic, ws[3])]
    batch = pkg.capi.BaBatch(dicts, cam)
    assert batch.run_group(0) == len(dicts)
    got = [results_of(batch, i) for i in range(len(dicts))]
    assert any(g[6] > g[5] for g in got)                        # rejected steps: more trials than iterations
    assert got[2][5] == 2 and max(g[5] for g in got) > 2        # one window stops early, another goes on
    for i, d in enumerate(dicts):
        assert_same(got[i], alone(pkg, d, cam), i)


def test_zero_extents_and_pieces(pkg, synthetic):
    """200 tiny windows: more than a launch takes (192), so the list is cut in two pieces and the prefix starts again; window 5 has every
    pose fixed -- it owns no workgroup of the kernels over free poses -- and stands in the middle of the first piece."""
    n = 200
    bases = [synthetic.ba_window(100 + s, n_opt=2, n_fix=2, n_points=30, pose_noise=(0.1, 0.01)) for s in range(8)]
    cam = bases[0]["cam"]
    dicts = []
    for i in range(n):
        d = window_dict(pkg, synthetic, bases[i % len(bases)])
        if i == 5:
            d["fixed"] = np.ones_like(d["fixed"])
        dicts.append(d)
    batch = pkg.capi.BaBatch(dicts, cam)
    batch.run_group(0)
    assert (batch.results >= 0).sum() >= n - 1
    for i in sorted(set(range(0, n, 17)) | {5, 191, 192, 199}):
        assert_same(results_of(batch, i), alone(pkg, dicts[i], cam), i)
