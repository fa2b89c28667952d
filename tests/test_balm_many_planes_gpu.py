"""The LiDAR plane term (balm_kernels.hip, balm_cut_kernels.hip, balm_host.cpp) on windows of thousands of planes, at the limits of its
kernels and in every form of its Hessian kernel.  The windows are balm_cases.ROWS (their plane counts: test_balm_many_planes.py); every test
here asserts the count it relies on from the host extraction, and -- where the library's per-launch profile can show it -- that the kernels
it is named for were the ones launched."""
import numpy as np
import pytest

import balm_cases

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4
SWITCHES = ("TC2LI_BA_DEVICE_LM", "TC2LI_BA_DEVICE_SOLVE", "TC2LI_BA_FUSE_LIN", "TC2LI_BA_FUSE_TRIAL", "TC2LI_BALM_HESS_LEAN")


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def launched(pkg, call, prefix="k_balm"):
    """-> (the call's result, the names of the kernels starting with `prefix` it launched)."""
    pkg.capi.profile_enable(True)
    try:
        pkg.capi.profile_report()
        out = call()
        names = sorted(k for k in pkg.capi.profile_report() if k.startswith(prefix))
    finally:
        pkg.capi.profile_enable(False)
    return out, names


@pytest.fixture(scope="module")
def oracle_edge(pkg, oracle, synthetic):
    """{row: (n_planes, residual, J, H)} of oracle.lidar_window_evaluate, filled on demand and never written to."""
    cache = {}

    def get(name):
        if name not in cache:
            w, win, clouds = balm_cases.row(name)
            cache[name] = oracle.lidar_window_evaluate(w["poses"], win, clouds, synthetic.TCL7)
        return cache[name]
    return get


# what the row reaches: (side of the plane limits, residual kernels, Hessian kernel)
EDGE_ROWS = {
    "p2047": (lambda n: n == 2047, ["k_balm_residual_total"], "k_balm_hessian_small"),
    "p2048": (lambda n: n == 2048, ["k_balm_residual_total"], "k_balm_hessian_small"),
    "p2049": (lambda n: n == 2049, ["k_balm_residual_planes", "k_balm_sum"], "k_balm_hessian_small"),
    "w3_over": (lambda n: 2048 < n <= 8192, ["k_balm_residual_planes", "k_balm_sum"], "k_balm_hessian_small"),
    "w2_two": (lambda n: 8192 < n <= 16384, ["k_balm_residual_planes", "k_balm_sum"], "k_balm_hessian_small"),
    "w8_two": (lambda n: 4096 < n <= 8192, ["k_balm_residual_planes", "k_balm_sum"], "k_balm_hessian_large"),
    "w7": (lambda n: 50 < n <= 2048, ["k_balm_residual_total"], "k_balm_hessian_small"),
    "w8": (lambda n: 50 < n <= 2048, ["k_balm_residual_total"], "k_balm_hessian_large"),
}


@pytest.mark.parametrize("name", list(EDGE_ROWS))
def test_lidar_edge_alone_on_many_planes(pkg, oracle_edge, synthetic, name):
    """tc2li_lidar_window_evaluate against oracle.lidar_window_evaluate, at the bars of test_lidar_edge_alone (same planes; residual to
    1e-10 relative; J and H rtol 1e-8, atol 1e-9 max|.|; derivatives=False gives the same residual bit for bit), on the rows that reach what
    the windows of a few hundred planes do not:

      p2047 / p2048 / p2049   Residual, many-plane form: balm_launch_residual goes from k_balm_residual_total to k_balm_residual_planes +
                              k_balm_sum above 2048 planes -- both sides of the switch, and the sum of exactly 2048 plane terms in one workgroup.
      w3_over                 the window of the lock-step and engine tests below, on its own.
      w2_two (W = 2, > 8192)  Hessian, second pass of the plane-batch loop: planes_per_chunk = 2 PB in the small form (PB = 8) -- the LDS tables
      w8_two (W = 8, > 4096)  are reused, s_n is zeroed for the planes past the chunk's end, s_coe is reset, the closing barrier holds --
                              and the same in the large form (PB = 4), with n_i = 0 slots among the planes.
      w7 | w8                 Window widths: W = 7, the widest of the small form (1008 of its 1024 owned Hessian items), and W = 8, the
                              narrowest of k_balm_hessian_large; planes with empty slots in both.

    The oracle adds the planes' terms in one double-precision loop in plane order; the product adds chunk partials of 8 or 16 planes and
    then the chunks in order (J, H), and 256 strided partial sums and a tree (residual)."""
    side, residual_kernels, hessian_kernel = EDGE_ROWS[name]
    w, win, clouds = balm_cases.row(name)
    assert side(len(balm_cases.host_planes(name)[1])), len(balm_cases.host_planes(name)[1])
    n0, r0, J0, H0 = oracle_edge(name)
    (n1, r1, J1, H1), names = launched(pkg, lambda: pkg.capi.lidar_window_evaluate(w["poses"], win, clouds, synthetic.TCL7))
    assert names == sorted(residual_kernels + [hessian_kernel, "k_balm_combine"]), names
    assert n1 == n0 and side(n0)
    print("%s: planes %d  |r1 - r0| / |r0| = %.3g  J: max err %.3g of max %.3g  H: max err %.3g of max %.3g"
          % (name, n1, abs(r1 - r0) / abs(r0), np.abs(J1 - J0).max(), np.abs(J0).max(), np.abs(H1 - H0).max(), np.abs(H0).max()))
    assert abs(r1 - r0) <= 1e-10 * abs(r0)
    assert np.allclose(J1, J0, rtol=1e-8, atol=1e-9 * np.abs(J0).max())
    assert np.allclose(H1, H0, rtol=1e-8, atol=1e-9 * np.abs(H0).max())
    (n2, r2, _, _), names = launched(pkg, lambda: pkg.capi.lidar_window_evaluate(w["poses"], win, clouds, synthetic.TCL7, derivatives=False))
    assert n2 == n0 and r2 == r1 and names == sorted(residual_kernels), names


def test_lidar_edge_alone_on_one_keyframe(pkg, oracle, synthetic):
    """Window widths: W = 1 gives no plane at all (a plane must be seen from two keyframes) -- 0 planes, residual 0, J and H all zero, as
    the oracle; no plane-term kernel is launched."""
    w, win, clouds = balm_cases.row("w1")
    assert len(balm_cases.host_planes("w1")[1]) == 0
    n0, r0, J0, H0 = oracle.lidar_window_evaluate(w["poses"], win, clouds, synthetic.TCL7)
    assert n0 == 0 and r0 == 0 and not J0.any() and not H0.any()
    (n1, r1, J1, H1), names = launched(pkg, lambda: pkg.capi.lidar_window_evaluate(w["poses"], win, clouds, synthetic.TCL7))
    assert n1 == 0 and r1 == 0 and J1.shape == (6,) and H1.shape == (6, 6) and not J1.any() and not H1.any()
    assert names == [], names
    n2, r2, _, _ = pkg.capi.lidar_window_evaluate(w["poses"], win, clouds, synthetic.TCL7, derivatives=False)
    assert n2 == 0 and r2 == 0


def test_extraction_at_exactly_2048_planes(pkg, synthetic):
    """Exactly 2048 planes, the most the batched kernels take (kBalmCutMaxPlanes): k_balm_cut_walk fills plane_cell to its last entry and
    does not set `over`; the device's planes are the host's, every sum bit for bit."""
    w, win, clouds = balm_cases.row("p2048")
    hc, hcoe = balm_cases.host_planes("p2048")
    assert len(hcoe) == 2048
    dc, dcoe, info = pkg.capi.lidar_planes_device(w["poses"], win, clouds, synthetic.TCL7)
    assert info.tolist() == [2048, 0, 2048, 2048]   # planes, declined, root voxels (one per cell of the sheet), planes found
    assert np.array_equal(dcoe, hcoe) and np.array_equal(dc, hc)


def test_extraction_overflow_at_2049_planes(pkg, synthetic):
    """Extraction overflow: one plane more than kBalmCutMaxPlanes.  k_balm_cut_walk's guard `at < kBalmCutMaxPlanes` keeps the 2049th
    plane out of plane_cell and the kernel sets `over`: tc2li_device_lidar_planes declines the window and names the 2049 planes it found,
    while the host extraction gives all 2049."""
    w, win, clouds = balm_cases.row("p2049")
    assert len(balm_cases.host_planes("p2049")[1]) == 2049
    with pytest.raises(pkg.capi.Tc2liError, match="2049 planes found"):
        pkg.capi.lidar_planes_device(w["poses"], win, clouds, synthetic.TCL7)
    # the same work space sizes right after: a window inside the range is not disturbed
    w, win, clouds = balm_cases.row("p2047")
    dc, dcoe, info = pkg.capi.lidar_planes_device(w["poses"], win, clouds, synthetic.TCL7)
    hc, hcoe = balm_cases.host_planes("p2047")
    assert info.tolist() == [2047, 0, 2047, 2047] and np.array_equal(dcoe, hcoe) and np.array_equal(dc, hc)


def rel_pose_err(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def lidar_dict(pkg, synthetic, w, win, clouds, **kw):
    return dict(poses=w["poses"], fixed=w["fixed"], points=w["points"], edges=pkg.pack_ba_edges(w["edges"]), win_pose=win, clouds=clouds,
                Tcl7=synthetic.TCL7, weight=1.0, **kw)


def standard_window(pkg, synthetic, seed, W):
    """A window of the size of balm_cases.window() with the standard clouds alone over its last W keyframes."""
    w = synthetic.ba_window(seed, n_opt=6, n_fix=4, n_points=300, pose_noise=(0.1, 0.01))
    last = len(w["poses"]) - 1
    win = list(range(last, last - W, -1))
    return lidar_dict(pkg, synthetic, w, win, synthetic.ba_window_clouds(w, win, n_points=1200, seed=seed)), w["cam"]


def one_window(pkg, d, cam):
    """Snapshot of the one-window entry point (g2o's loop on the host) on a window dict."""
    if "win_pose" in d:
        poses, pts, chi2, dpos, st, ls = pkg.capi.local_lv_bundle_adjustment(d["poses"], d["fixed"], d["points"], d["edges"], cam, d["win_pose"], d["clouds"],
                                                                             d["Tcl7"], d["weight"])
        n_planes, residual = ls.n_planes, ls.residual
    else:
        poses, pts, chi2, dpos, st = pkg.local_bundle_adjustment(d["poses"], d["fixed"], d["points"], d["edges"], cam)
        n_planes, residual = 0, 0.0
    return dict(result=st.iterations, poses=poses.copy(), points=pts.copy(), chi2=chi2.copy(), dpos=dpos.copy(), iterations=st.iterations, trials=st.trials,
                n_free=st.n_free_poses, final_chi2=st.final_chi2, final_lambda=st.final_lambda, initial_chi2=st.initial_chi2, n_planes=n_planes,
                residual=residual)


def snapshot(batch, i):
    """As test_ba_solve_lds_gpu.snapshot, plus the LiDAR edge's residual."""
    poses, pts, chi2, dpos, st, ls = batch.result(i)
    return dict(result=int(batch.results[i]), poses=poses.copy(), points=pts.copy(), chi2=chi2.copy(), dpos=dpos.copy(), iterations=st.iterations,
                trials=st.trials, n_free=st.n_free_poses, final_chi2=st.final_chi2, final_lambda=st.final_lambda, initial_chi2=st.initial_chi2,
                n_planes=ls.n_planes, residual=ls.residual)


def same(a, b, tag):
    for k in ("result", "iterations", "trials", "n_free", "final_chi2", "final_lambda", "initial_chi2", "n_planes", "residual"):
        assert a[k] == b[k], (tag, k, a[k], b[k])
    for k in ("poses", "points", "chi2", "dpos"):
        assert np.array_equal(a[k], b[k]), (tag, k, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))


@pytest.fixture(scope="module")
def over_limit_batch(pkg, synthetic):
    """Three LiDAR windows, the middle one over the batched kernels' plane limit: (dicts, camera, one-window snapshots).  Not written to."""
    a, cam = standard_window(pkg, synthetic, 81, 4)
    w, win, clouds = balm_cases.row("w3_over")
    big = lidar_dict(pkg, synthetic, w, win, clouds)
    c, _ = standard_window(pkg, synthetic, 82, 3)
    dicts = [a, big, c]
    assert np.array_equal(cam, w["cam"])
    return dicts, cam, [one_window(pkg, d, cam) for d in dicts]


@pytest.mark.parametrize("device_lm", ["1", "0"])  # the LM decisions on the device / on the host between the phases
def test_lock_step_batch_with_one_window_over_the_plane_limit(pkg, oracle, synthetic, over_limit_batch, device_lm, monkeypatch):
    """Extraction overflow, in a lock-step batch: three LiDAR windows of which the second has more than 2048 planes (w3_over; W = 3 and
    45 000 points, so its extraction is queued on the device with the others').  k_balm_cut_walk sets `over`, BalmTerm::finish_cut extracts on
    the host, and lockstep_setup sends the batch through the one-window path, where the window's residual takes k_balm_residual_planes +
    k_balm_sum.  Every window equals its local_lv_bundle_adjustment call bit for bit (the shape of test_mixed_batch_falls_back_per_group),
    twice in a row; the big window also agrees with the oracle: same iterations and trials, same planes, poses <= 1e-4 relative."""
    dicts, cam, singles = over_limit_batch
    n_big = len(balm_cases.host_planes("w3_over")[1])
    assert 2048 < n_big <= 8192 and singles[1]["n_planes"] == n_big
    assert all(0 < s["n_planes"] <= 2048 for s in (singles[0], singles[2]))
    assert all(s["iterations"] > 0 and s["final_chi2"] < s["initial_chi2"] for s in singles)
    set_env(monkeypatch, {"TC2LI_BA_DEVICE_LM": device_lm})
    assert pkg.capi.ba_options()["device_lm"] == int(device_lm)
    batch = pkg.capi.BaBatch(dicts, cam)
    for rep in range(2):  # the second call starts from the same inputs: BaBatch.run resets them
        n_ok, names = launched(pkg, lambda: batch.run(max_concurrency=8))
        assert n_ok == len(dicts)
        # the extraction ran on the device, and the window over the limit went through the one-window kernels
        assert "k_balm_cut_walk" in names and "k_balm_residual_planes" in names and "k_balm_hessian_small" in names, names
        assert not any(k.startswith("k_balm_hessian") and k.endswith("_b") for k in names), names
        for i, s in enumerate(singles):
            same(snapshot(batch, i), s, "device_lm %s, run %d, window %d" % (device_lm, rep, i))
    set_env(monkeypatch, {})
    w, win, clouds = balm_cases.row("w3_over")
    want = oracle.local_ba_lidar(w["poses"], w["fixed"], w["points"], w["edges"], w["cam"], win, clouds, synthetic.TCL7, 1.0)
    got = singles[1]
    assert got["iterations"] == want[4] and got["trials"] == int(want[5]["trials"].sum()) and got["trials"] > got["iterations"]
    assert got["n_planes"] == want[6] and abs(got["residual"] - want[7]["residual"]) <= 1e-6 * abs(want[7]["residual"])
    for k in range(len(got["poses"])):
        assert rel_pose_err(got["poses"][k], want[0][k]) < POSE_RTOL, k
    assert np.array_equal(got["poses"][w["fixed"] > 0], w["poses"][w["fixed"] > 0])


def test_engine_with_one_window_over_the_plane_limit(pkg, synthetic, over_limit_batch):
    """Extraction overflow, through the engine: tc2li_ba_engine with three slots takes the same three windows.  The window of more than
    2048 planes is extracted on the host (finish_cut) and optimised by a one-window call on the engine thread (ba_engine.cpp): it equals
    local_lv_bundle_adjustment bit for bit, as window 0 of test_engine_edge_cases does.  Its two neighbours equal, bit for bit, what an
    engine gives them without the big window; and the engine takes the three again."""
    dicts, cam, singles = over_limit_batch
    assert singles[1]["n_planes"] > 2048
    alone = pkg.capi.BaEngine(cam, max_windows=3)
    ba = pkg.capi.BaBatch([dicts[0], dicts[2]], cam)
    assert alone.wait(alone.submit(ba)) == 2
    want = [snapshot(ba, 0), snapshot(ba, 1)]
    alone.close()
    assert all(s["iterations"] > 0 and s["final_chi2"] < s["initial_chi2"] and 0 < s["n_planes"] <= 2048 for s in want)
    eng = pkg.capi.BaEngine(cam, max_windows=3)
    b = pkg.capi.BaBatch(dicts, cam)
    for rep in range(2):
        assert eng.wait(eng.submit(b)) == 3
        same(snapshot(b, 1), singles[1], "the big window, run %d" % rep)
        same(snapshot(b, 0), want[0], "first neighbour, run %d" % rep)
        same(snapshot(b, 2), want[1], "second neighbour, run %d" % rep)
    eng.close()


@pytest.fixture(scope="module")
def edge_group(pkg, synthetic):
    """The lock-step group of the Hessian-form tests: (dicts, camera, one-window snapshots).  Not written to."""
    dicts, cam = [], None
    for name in ("p2048", "w7"):
        w, win, clouds = balm_cases.row(name)
        dicts.append(lidar_dict(pkg, synthetic, w, win, clouds))
    for seed, W in ((83, 2), (84, 5)):
        d, cam = standard_window(pkg, synthetic, seed, W)
        dicts.append(d)
    wc = synthetic.ba_window(85, n_opt=6, n_fix=4, n_points=300, pose_noise=(0.1, 0.01))
    dicts.append(dict(poses=wc["poses"], fixed=wc["fixed"], points=wc["points"], edges=pkg.pack_ba_edges(wc["edges"])))
    return dicts, cam, [one_window(pkg, d, cam) for d in dicts]


def run_forms(pkg, monkeypatch, edge_group, forms):
    """The group under every (TC2LI_BALM_HESS_LEAN, the Hessian kernel it must launch) of `forms`, each with TC2LI_BA_FUSE_LIN unset and 1:
    every run equals the first one and the one-window calls bit for bit."""
    dicts, cam, singles = edge_group
    n_w7 = len(balm_cases.host_planes("w7")[1])
    assert len(balm_cases.host_planes("p2048")[1]) == 2048 and 50 < n_w7 <= 2048
    assert [s["n_planes"] for s in singles[:2]] == [2048, n_w7] and singles[4]["n_planes"] == 0
    assert all(s["iterations"] > 0 and s["final_chi2"] < s["initial_chi2"] for s in singles)
    assert any(s["trials"] > s["iterations"] for s in singles[:2])   # rejected steps: the trial phases' residual runs more than once a round
    batch = pkg.capi.BaBatch(dicts, cam)
    first = None
    for lean, kernel in forms:
        for fuse in (None, "1"):
            env = {}
            if lean is not None:
                env["TC2LI_BALM_HESS_LEAN"] = lean
            if fuse is not None:
                env["TC2LI_BA_FUSE_LIN"] = fuse
            set_env(monkeypatch, env)
            tag = "TC2LI_BALM_HESS_LEAN=%s TC2LI_BA_FUSE_LIN=%s" % (lean, fuse)
            assert pkg.capi.ba_options()["fuse_linearize"] == int(fuse is not None), tag
            n_ok, names = launched(pkg, lambda: batch.run_group(0))
            assert n_ok == len(dicts), tag
            assert [k for k in names if k.startswith("k_balm_hessian")] == [kernel], (tag, names)
            assert ("k_balm_combine_b" in names) == (fuse is None or kernel == "k_balm_hessian_b"), (tag, names)
            assert "k_balm_residual_total_b" in names and "k_balm_residual_planes" not in names, (tag, names)
            got = [snapshot(batch, i) for i in range(len(dicts))]
            first = first or got
            for i, g in enumerate(got):
                same(g, first[i], "%s, window %d against the first run" % (tag, i))
                same(g, singles[i], "%s, window %d against the one-window call" % (tag, i))
    set_env(monkeypatch, {})


def test_every_hessian_form_at_the_batched_kernels_edges(pkg, synthetic, edge_group, monkeypatch):
    """Hessian forms: TC2LI_BALM_HESS_LEAN selects k_balm_hessian_b (0), k_balm_hessian_lean3_b (unset, 3) or k_balm_hessian_lean4_b (4: 128
    registers, 84 values in scratch), each with the chunks' sums in a launch of their own or, under TC2LI_BA_FUSE_LIN=1 and a lean form, by the
    window's last chunk.  One lock-step group holds

      the window of exactly 2048 planes (W = 2) through the whole Levenberg-Marquardt loop: 256 chunks, d_part exactly full,
        k_balm_residual_total_b adding 2048 plane terms in one workgroup;
      the W = 7 window (balm_cases w7: the widest the small form and the lock-step kernels take, planes with n_i = 0 slots);
      W = 2 and W = 5 windows of the standard clouds, and one camera-only window.

    The eight runs are identical bit for bit -- poses, points, per-edge chi2, depth flags, iterations, trials, chi2, lambda, planes, the
    LiDAR residual -- and equal to the one-window calls; the profile names the Hessian kernel each run launched, and k_balm_combine_b
    exactly where the sums are not fused."""
    run_forms(pkg, monkeypatch, edge_group, [(None, "k_balm_hessian_lean3_b"), ("0", "k_balm_hessian_b"), ("3", "k_balm_hessian_lean3_b"),
                                             ("4", "k_balm_hessian_lean4_b")])


def test_an_unnamed_hessian_form_keeps_its_combine_launch(pkg, synthetic, edge_group, monkeypatch):
    """Hessian forms: a value of TC2LI_BALM_HESS_LEAN other than 0, 3 and 4 (here 1 and 2) launches k_balm_hessian_b, as 0 does.  Under
    TC2LI_BA_FUSE_LIN=1 balm_batch_launch_hessian took such a value for a lean form, skipped k_balm_combine_b, and no kernel added the chunks'
    partial sums: the optimiser ran on a stale Hessian of the plane term.  The same group as above, the same bits as the default form."""
    run_forms(pkg, monkeypatch, edge_group, [(None, "k_balm_hessian_lean3_b"), ("1", "k_balm_hessian_b"), ("2", "k_balm_hessian_b")])
