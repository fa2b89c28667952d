"""The reduced camera system's solve on the device (k_ba_solve5_b / k_ba_solve_b / k_ba_solve9_b: 5 / 8 / 9 tile rows of 16) with L handed to
the backward sweep one tile row at a time, against the host's LDL^T.

Windows of 1, 2, 3, 13, 14, 21, 22 and 24 free keyframes (n = 6, 12, 18, 78, 84, 126, 132, 144 unknowns): below one tile, across a tile edge,
and both sides of each variant's limit (13 | 14 and 21 | 22; 24 is the widest the kernels take).  About 60 points per window, with and without a
LiDAR term.  Every window runs ONE Levenberg-Marquardt round in a lock-step batch: its result is then the first step applied to the poses and,
through the back-substitution, to the points.  The C ABI does not hand out the step itself; the poses, the points, the per-edge chi2, lambda
and the trial count after one round are functions of it and are compared bit for bit:

  host LM, host solve (TC2LI_BA_DEVICE_LM=0)  ==  host LM, device solve (+ TC2LI_BA_DEVICE_SOLVE=1)  ==  device LM (the default)  ==  the
  one-window call (host solve)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FREE = (1, 2, 3, 13, 14, 21, 22, 24)
LIDAR_FROM = 3      # windows of at least this many free keyframes also come with a LiDAR term over their last 3 or 4 keyframes
SWITCHES = ("TC2LI_BA_DEVICE_LM", "TC2LI_BA_DEVICE_SOLVE", "TC2LI_BA_FUSE_LIN", "TC2LI_BA_FUSE_TRIAL")
PLACES = {"host LM, host solve": {"TC2LI_BA_DEVICE_LM": "0"}, "host LM, device solve": {"TC2LI_BA_DEVICE_LM": "0", "TC2LI_BA_DEVICE_SOLVE": "1"},
          "device LM": {}}


def set_env(monkeypatch, env):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def make_window(pkg, synthetic, n_free, lidar, iterations=1):
    w = synthetic.ba_window(100 + n_free, n_opt=n_free, n_fix=2, n_points=75, pose_noise=(0.1, 0.01))
    d = dict(poses=w["poses"], fixed=w["fixed"], points=w["points"], edges=pkg.pack_ba_edges(w["edges"]), iterations=iterations, n_free=n_free)
    if lidar:
        last = len(w["poses"]) - 1
        win = list(range(last, last - min(4, n_free), -1))
        d.update(win_pose=win, clouds=synthetic.ba_window_clouds(w, win, n_points=600), Tcl7=synthetic.TCL7, weight=1.0)
    return d, w["cam"]


@pytest.fixture(scope="module")
def windows(pkg, synthetic):
    """[(name, window)], camera: every width without a LiDAR term, the widths from LIDAR_FROM on also with one."""
    out, cam = [], None
    for nf in FREE:
        for lidar in (False, True):
            if lidar and nf < LIDAR_FROM:
                continue
            d, cam = make_window(pkg, synthetic, nf, lidar)
            out.append(("%d free%s" % (nf, ", LiDAR" if lidar else ""), d))
    assert 50 <= np.median([len(d["points"]) for _, d in out]) <= 70
    return out, cam


def snapshot(batch, i):
    poses, pts, chi2, dpos, st, ls = batch.result(i)
    return dict(result=int(batch.results[i]), poses=poses.copy(), points=pts.copy(), chi2=chi2.copy(), dpos=dpos.copy(), iterations=st.iterations,
                trials=st.trials, n_free=st.n_free_poses, final_chi2=st.final_chi2, final_lambda=st.final_lambda, initial_chi2=st.initial_chi2,
                n_planes=ls.n_planes)


def same(a, b, tag):
    for k in ("result", "iterations", "trials", "n_free", "final_chi2", "final_lambda", "initial_chi2", "n_planes"):
        assert a[k] == b[k], (tag, k, a[k], b[k])
    for k in ("poses", "points", "chi2", "dpos"):
        assert np.array_equal(a[k], b[k]), (tag, k, float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max()))


def run_places(pkg, monkeypatch, wins, cam, run=lambda b: b.run(8)):
    """{place: [snapshot per window]} of one batch over `wins` under each set of switches."""
    batch = pkg.capi.BaBatch(wins, cam)
    got = {}
    for place, env in PLACES.items():
        set_env(monkeypatch, env)
        opt = pkg.capi.ba_options()
        assert opt["device_lm"] == int("TC2LI_BA_DEVICE_LM" not in env) and opt["device_solve"] == int("TC2LI_BA_DEVICE_SOLVE" in env)
        assert run(batch) == len(wins), place
        got[place] = [snapshot(batch, i) for i in range(len(wins))]
    set_env(monkeypatch, {})
    return got


def test_device_solve_equals_host_solve_over_the_widths(pkg, synthetic, windows, monkeypatch):
    named, cam = windows
    wins = [d for _, d in named]
    got = run_places(pkg, monkeypatch, wins, cam)
    host = got["host LM, host solve"]
    for (name, d), h in zip(named, host):
        # the window is what its name says, and its round moved something: one accepted or rejected trial over n = 6 n_free unknowns
        assert h["n_free"] == d["n_free"] and h["iterations"] == 1 and h["trials"] >= 1, name
        assert h["final_chi2"] < h["initial_chi2"], name
        assert not np.array_equal(h["poses"], d["poses"]), name
        assert (h["n_planes"] > 0) == ("win_pose" in d), name
    for place in ("host LM, device solve", "device LM"):
        for (name, _), h, g in zip(named, host, got[place]):
            same(g, h, "%s: %s" % (place, name))
    # and the one-window path (g2o's loop on the host, the host's LDL^T)
    for (name, d), h in zip(named, host):
        if "win_pose" in d:
            s = pkg.capi.local_lv_bundle_adjustment(d["poses"], d["fixed"], d["points"], d["edges"], cam, d["win_pose"], d["clouds"], d["Tcl7"], d["weight"],
                                                    iterations=1)
        else:
            s = pkg.capi.local_bundle_adjustment(d["poses"], d["fixed"], d["points"], d["edges"], cam, iterations=1)
        assert np.array_equal(s[0], h["poses"]) and np.array_equal(s[1], h["points"]), name


def test_a_narrow_window_in_the_widest_variant(pkg, synthetic, monkeypatch):
    """4 and 24 free keyframes in one batch: the launch takes the 9-tile-row variant, the 4-keyframe window (n = 24: two tile rows) rides in it
    and skips the other seven.  Each equals the batch of itself alone -- there the narrow window runs in the 5-tile-row variant -- bit for bit,
    one round and the full ten."""
    for iterations in (1, 10):
        a, cam = make_window(pkg, synthetic, 4, True, iterations)
        b, _ = make_window(pkg, synthetic, 24, False, iterations)
        for order in ((a, b), (b, a)):
            together = run_places(pkg, monkeypatch, list(order), cam)
            for i, w in enumerate(order):
                alone = run_places(pkg, monkeypatch, [w], cam)
                for place in PLACES:
                    assert together[place][i]["n_free"] == w["n_free"]
                    same(together[place][i], alone[place][0], "%d iterations, %s, %d free" % (iterations, place, w["n_free"]))
                    same(together[place][i], together["host LM, host solve"][i], "%d iterations, %s, %d free" % (iterations, place, w["n_free"]))


def test_a_system_without_a_usable_pivot(pkg, synthetic, monkeypatch):
    """A free pose without edges: it must come back as it went in, and the window must be the same in every place.  And a window whose edges
    all carry the information 0: H = 0, lambda = 0, the first pivot is 0 -- the solve reports ok = 0 and the zero step, the trials fail, and
    nothing moves; again the same in every place."""
    d, cam = make_window(pkg, synthetic, 3, False, iterations=3)
    w = synthetic.ba_window(103, n_opt=3, n_fix=2, n_points=75, pose_noise=(0.1, 0.01))
    lonely = len(w["poses"]) - 2
    e = w["edges"][w["edges"][:, 1] != lonely]
    bare = dict(d, edges=pkg.pack_ba_edges(e))
    got = run_places(pkg, monkeypatch, [bare], cam)
    for place in PLACES:
        g = got[place][0]
        same(g, got["host LM, host solve"][0], place)
        assert np.array_equal(g["poses"][lonely], w["poses"][lonely]), place
        assert g["final_chi2"] < g["initial_chi2"], place
    e0 = w["edges"].copy()
    e0[:, 5] = 0.0
    null = dict(d, edges=pkg.pack_ba_edges(e0))
    got = run_places(pkg, monkeypatch, [null], cam)
    for place in PLACES:
        g = got[place][0]
        same(g, got["host LM, host solve"][0], place)
        assert np.array_equal(g["poses"], w["poses"]) and np.array_equal(g["points"], w["points"]), place
