"""Directed tests of the local bundle adjustment's Levenberg-Marquardt loop against the oracle, on the hand-made windows of
ba_exit_cases.py, in every place the loop lives: the one-window host loop (ba_host.cpp / lvi_host.cpp), the lock-step batch with the
decisions on the device (k_ba_lm_begin_b / k_ba_lm_decide_b), the same batch with TC2LI_BA_DEVICE_LM=0 with and without
TC2LI_BA_DEVICE_SOLVE=1, BaEngine, and the inertial twin with TC2LI_LVI_DEVICE_SOLVE at 1 and 0; then the two shipped forms no other test
sets, TC2LI_BA_FUSE_LIN=1 and TC2LI_BA_FUSE_TRIAL=1.

The random windows of the other BA tests run their 10 iterations, in a world whose origin lies on the trajectory, with every depth
above 1 m.  That each window here reaches its branch is shown in test_ba_exit_cases.py from the oracle alone; this file only compares.

  case                  exit it reaches                                                      oracle: iterations, trials
  plain                 the cap of 10 iterations                                              10, 1 each
  converged             n_bad >= 3: three accepted steps below 1e-3 of chi2                   3, [1, 1, 1]
  rho_zero              rho == 0, ok = false: a step accepted, then one that changes nothing  2, [1, 1]
  stall_after_progress  n_bad >= 3 after three steps of real progress (Gauss-Newton)          6, 1 each
  rotated_a, _b, _c     the cap; qw down to 0.002, translations up to 600 m                   10, 1 each
  behind                the cap; edge_depth_positive == 0 on one edge                         10, 1 each
  close                 the cap; a landmark 0.05 m in front of a keyframe, all flags 1        10, 1 each
  lidar_converged       n_bad >= 3 with the LiDAR edge in the cost                            3, [1, 1, 1]
  inertial_converged    n_bad >= 3 in the inertial loop                                       3, [1, 1, 1]

Left out: the exit by qmax == 10 (ten rejected trials in one iteration).  No window with finite input reaches it other than by a
decision at the rounding level (the fully converged inertial window does: ten rejections at constant chi2, test_ba_exit_cases.py), and
a rejected trial of any kind at a stalled window is such a decision; the rejections the loop takes far from the optimum are in
test_balm_gpu.py's heavy LiDAR edges.  Also left out, as out of scope: a stop flag raised mid-run, tc2li_ba_window_solve_batch, the
sharded entry.

Bars.  Against the oracle: those of test_ba_gpu.py (visual), test_balm_gpu.py (LiDAR) and test_inertial_ba_gpu.py (inertial), plus
iterations and trials exactly, the depth flags and the outlier set exactly, final_lambda within 1e-9 in the exit cases (a product of the
same few factors), and the rotated windows' results, moved back, within 1e-4 of the plain window's.  Between the places: bit for bit, as
test_balm_gpu.py asserts for its windows.  TC2LI_BA_FUSE_LIN=1 gives the default's bits; TC2LI_BA_FUSE_TRIAL=1 fixes the order of two sums
(ba_device.hpp) and is held to 1e-9 of the default, the largest difference printed."""
import numpy as np
import pytest

import ba_exit_cases as bc

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4   # BASELINE.json's bar for optimised SE3 poses


# ---- results in one shape -------------------------------------------------------------------------------------------------------
def snapshot(r):
    """A result tuple of a one-window call or of BaBatch / LviBatch.result(i), copied: the arrays of a batch are written again by its next run."""
    out = dict(state=np.array(r[0], copy=True), points=np.array(r[1], copy=True), chi2=np.array(r[2], copy=True), dpos=np.array(r[3], copy=True),
               iterations=int(r[4].iterations), trials=int(r[4].trials), n_free_poses=int(r[4].n_free_poses), initial_chi2=float(r[4].initial_chi2),
               final_chi2=float(r[4].final_chi2), final_lambda=float(r[4].final_lambda))
    if len(r) > 5:
        out["lidar"] = (int(r[5].n_planes), int(r[5].hessian_evaluations), float(r[5].residual), float(r[5].chi2))
    return out


def difference(a, b, lidar):
    """The first field in which two snapshots differ in a bit, or None."""
    for k in ("state", "points", "chi2", "dpos"):
        if not np.array_equal(a[k], b[k]):
            return k
    for k in ("iterations", "trials", "n_free_poses", "initial_chi2", "final_chi2", "final_lambda") + (("lidar",) if lidar else ()):
        if a[k] != b[k]:
            return k
    return None


def run_alone(pkg, window, cam, calib24=None):
    """The window through its one-window entry point."""
    w = window
    kw = {k: w[k] for k in ("iterations", "lambda_init") if k in w}
    if "kf33" in w:
        return snapshot(pkg.capi.local_inertial_bundle_adjustment(w["kf33"], w["fixed"], w["has_imu"], calib24, w["points"], w["edges"], w["link4"], w["pre"], cam, **kw))
    if "win_pose" in w:
        return snapshot(pkg.capi.local_lv_bundle_adjustment(w["poses"], w["fixed"], w["points"], w["edges"], cam, w["win_pose"], w["clouds"], w["Tcl7"],
                                                            w["weight"], **kw))
    return snapshot(pkg.local_bundle_adjustment(w["poses"], w["fixed"], w["points"], w["edges"], cam, **kw))


# ---- the bars against the oracle ------------------------------------------------------------------------------------------------
def rel_pose_err(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


def check_against_oracle(name, got, c, exit_case):
    want, w, e = c["want"], c["window"], c["edges6"]
    n_trials = int(want[5]["trials"].sum())
    inertial, lidar = "kf33" in w, "win_pose" in w
    print("%s: iterations %d (%d), trials %d (%d), final chi2 %.3e off, final lambda %.3e off" % (
        name, got["iterations"], want[4], got["trials"], n_trials, abs(got["final_chi2"] / want[5]["chi2"][-1] - 1) if want[4] else 0.0,
        abs(got["final_lambda"] / want[5]["lam"][-1] - 1) if want[4] else 0.0))
    assert got["iterations"] == want[4] and got["trials"] == n_trials
    assert np.array_equal(got["dpos"], want[3])
    assert np.array_equal(bc.outliers(e, got["chi2"], got["dpos"]), bc.outliers(e, want[2], want[3]))
    if exit_case:
        assert abs(got["final_lambda"] - want[5]["lam"][-1]) <= 1e-9 * want[5]["lam"][-1]
    if inertial:   # test_inertial_ba_gpu.py::test_local_inertial_ba
        assert abs(got["initial_chi2"] - want[6][0]) <= 3e-6 * want[6][0] and abs(got["final_chi2"] - want[6][1]) <= 3e-6 * want[6][1]
        for k in range(len(want[0])):
            assert rel_pose_err(got["state"][k, :24], want[0][k, :24]) < POSE_RTOL
            assert np.allclose(got["state"][k, 24:], want[0][k, 24:], rtol=POSE_RTOL, atol=1e-6)
        assert np.array_equal(got["state"][0], w["kf33"][0])
        assert np.allclose(got["points"], want[1], rtol=POSE_RTOL, atol=1e-5)
        assert np.allclose(got["chi2"], want[2], rtol=5e-3, atol=1e-3)
        return
    assert abs(got["final_chi2"] - want[5]["chi2"][-1]) <= 1e-6 * want[5]["chi2"][-1]
    for k in range(len(want[0])):
        assert rel_pose_err(got["state"][k], want[0][k]) < POSE_RTOL
    assert np.array_equal(got["state"][w["fixed"] > 0], w["poses"][w["fixed"] > 0])
    assert np.allclose(got["points"], want[1], rtol=POSE_RTOL, atol=1e-6)
    if lidar:      # test_balm_gpu.py::test_local_lv_bundle_adjustment
        assert got["lidar"][0] == want[6] and abs(got["lidar"][2] - want[7]["residual"]) <= 1e-6 * abs(want[7]["residual"])
        assert np.allclose(got["chi2"], want[2], rtol=1e-4, atol=1e-6)
    else:          # test_ba_gpu.py::test_local_bundle_adjustment
        assert np.allclose(got["chi2"], want[2], rtol=1e-5, atol=1e-7)


# ---- the windows ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cases(pkg, oracle, synthetic):
    out = dict(bc.catalogue(pkg, oracle, synthetic))
    # two ordinary windows that run their 10 iterations, one of them with a LiDAR edge
    for name, seed, lidar in (("ordinary", 7, False), ("ordinary_lidar", 8, True)):
        w = synthetic.ba_window(seed, n_opt=5, n_fix=4, n_points=300, pose_noise=(0.1, 0.01))
        last = len(w["poses"]) - 1
        win = [last, last - 1, last - 2, last - 3]
        lw = dict(win_pose=win, clouds=synthetic.ba_window_clouds(w, win, n_points=900), Tcl7=synthetic.TCL7, weight=1.0) if lidar else None
        out[name] = bc.visual_case(pkg, oracle, w, lidar=lw)
    # a window with two and three edges between the same landmark and the same free keyframe: ba_kernels.hip takes the separate sums for it
    w = synthetic.ba_window(3, n_opt=5, n_fix=4, n_points=300)
    free = np.flatnonzero(w["fixed"] == 0)
    pose = w["edges"][:, 1].astype(int)
    ks = [int(np.flatnonzero(pose == int(free[0]))[0])] * 2 + [int(np.flatnonzero(pose == int(free[1]))[3]), int(np.flatnonzero(pose == int(free[-1]))[7])]
    dup = np.concatenate([w["edges"]] + [w["edges"][k:k + 1] for k in ks])
    dup[-1, 2] += 0.75
    dup[-2, 3] -= 0.5
    out["duplicates"] = bc.visual_case(pkg, oracle, dict(w, edges=dup), iterations=6)
    # an ordinary inertial window beside inertial_converged
    wi = bc.inertial_problem(pkg, oracle, synthetic, 5, n_opt=3, n_points=150)
    out["inertial_ordinary"] = dict(window=bc.inertial_window_dict(pkg, wi, wi["kf33"], wi["points"]), cam=wi["cam"], calib24=wi["calib24"], edges6=wi["edges"],
                                    want=bc.run_inertial_oracle(oracle, wi, wi["kf33"], wi["points"]), kw={})
    return out


ORDERS = {"exits first": ("converged", "rho_zero", "ordinary", "stall_after_progress", "lidar_converged", "plain", "rotated_a", "rotated_b", "rotated_c",
                          "behind", "close", "ordinary_lidar"),
          "exits last": ("ordinary_lidar", "close", "behind", "rotated_c", "ordinary", "rotated_b", "rotated_a", "plain", "lidar_converged",
                         "stall_after_progress", "rho_zero", "converged")}
INERTIAL_ORDER = ("inertial_converged", "inertial_ordinary")
PLACES = {"device LM": {}, "host LM": {"TC2LI_BA_DEVICE_LM": "0"}, "host LM, device solve": {"TC2LI_BA_DEVICE_LM": "0", "TC2LI_BA_DEVICE_SOLVE": "1"}}
FUSED = {"lin": {"TC2LI_BA_FUSE_LIN": "1"}, "trial": {"TC2LI_BA_FUSE_TRIAL": "1"}, "lin+trial": {"TC2LI_BA_FUSE_LIN": "1", "TC2LI_BA_FUSE_TRIAL": "1"}}


SWITCHES = ("TC2LI_BA_DEVICE_LM", "TC2LI_BA_DEVICE_SOLVE", "TC2LI_BA_FUSE_LIN", "TC2LI_BA_FUSE_TRIAL", "TC2LI_LVI_DEVICE_SOLVE")


def set_env(monkeypatch, env):
    """These switches and no others: the library reads them at the start of every call."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


class Alone(dict):
    """(switches, name) -> the one-window call's snapshot under those switches, computed on first use."""

    def __init__(self, pkg, cases):
        super().__init__()
        self.pkg, self.cases = pkg, cases

    def __missing__(self, key):
        env, name = key
        c = self.cases[name]
        with pytest.MonkeyPatch.context() as mp:
            set_env(mp, dict(env))
            self[key] = run_alone(self.pkg, c["window"], c["cam"], c.get("calib24"))
        return self[key]


@pytest.fixture(scope="module")
def alone(pkg, cases):
    return Alone(pkg, cases)


def key(env):
    return tuple(sorted(env.items()))


def assert_batch_equals(batch, names, wanted, what, cases):
    for i, name in enumerate(names):
        got = snapshot(batch.result(i))
        assert int(batch.results[i]) == wanted[name]["iterations"], (what, i, name)
        d = difference(got, wanted[name], "lidar" in wanted[name] and "win_pose" in cases[name]["window"])
        assert d is None, "%s, window %d (%s): %s differs from the one-window call" % (what, i, name, d)


# ---- against the oracle ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_case_against_the_oracle(cases, alone, name):
    check_against_oracle(name, alone[(), name], cases[name], name in bc.EXIT_CASES)


@pytest.mark.parametrize("name", sorted(bc.ROTATIONS))
def test_moved_world_frame_gives_the_plain_windows_result(cases, alone, name):
    """The product's result in the moved frame, moved back, against the product's result for the plain window."""
    got, plain = alone[(), name], alone[(), "plain"]
    Rm, tm, pts = bc.move_back(got["state"], got["points"], *cases[name]["transform"])
    Rp, tp = bc.pose_matrices(plain["state"])
    print("%s moved back: rotations %.2e, translations %.2e, points %.2e off the plain window's" % (name, np.abs(Rm - Rp).max(), bc.rel(tm, tp), bc.rel(pts, plain["points"])))
    assert (got["iterations"], got["trials"]) == (plain["iterations"], plain["trials"])
    assert np.abs(Rm - Rp).max() < POSE_RTOL and bc.rel(tm, tp) < POSE_RTOL and bc.rel(pts, plain["points"]) < POSE_RTOL
    assert np.array_equal(bc.outliers(cases[name]["edges6"], got["chi2"], got["dpos"]), bc.outliers(cases["plain"]["edges6"], plain["chi2"], plain["dpos"]))


def test_the_depth_flag_is_zero_where_the_oracle_has_it(cases, alone):
    got, c = alone[(), "behind"], cases["behind"]
    assert np.flatnonzero(got["dpos"] == 0).tolist() == [c["edge"]] and np.isfinite(got["state"]).all() and np.isfinite(got["points"]).all()
    assert (alone[(), "close"]["dpos"] == 1).all()


# ---- every place the loop lives -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", sorted(ORDERS))
@pytest.mark.parametrize("place", sorted(PLACES))
def test_every_window_of_a_batch_gets_the_bits_of_its_own_call(pkg, cases, alone, monkeypatch, place, order):
    names = ORDERS[order]
    wanted = {n: alone[(), n] for n in names}
    assert wanted["ordinary"]["iterations"] == wanted["ordinary_lidar"]["iterations"] == 10 and wanted["converged"]["iterations"] == 3
    set_env(monkeypatch, PLACES[place])
    opt = pkg.capi.ba_options()
    assert opt["device_lm"] == int("TC2LI_BA_DEVICE_LM" not in PLACES[place]) and opt["device_solve"] == int("TC2LI_BA_DEVICE_SOLVE" in PLACES[place])
    batch = pkg.capi.BaBatch([cases[n]["window"] for n in names], cases["plain"]["cam"])
    for what, run in (("run(8)", lambda: batch.run(8)), ("run(1)", lambda: batch.run(1)), ("run_group(0)", lambda: batch.run_group(0))):
        assert run() == len(names)
        assert_batch_equals(batch, names, wanted, "%s, %s, %s" % (place, order, what), cases)


@pytest.mark.parametrize("order", sorted(ORDERS))
def test_engine_with_fewer_slots_than_windows(pkg, cases, alone, monkeypatch, order):
    """Three slots for twelve windows: the windows that end after 2, 3 and 6 iterations free their slots for later ones."""
    names = ORDERS[order]
    wanted = {n: alone[(), n] for n in names}
    set_env(monkeypatch, {})
    cam = cases["plain"]["cam"]
    eng = pkg.capi.BaEngine(cam, max_windows=3)
    batch = pkg.capi.BaBatch([cases[n]["window"] for n in names], cam)
    try:
        for _ in range(2):   # the engine is reusable
            assert eng.wait(eng.submit(batch)) == len(names)
            assert_batch_equals(batch, names, wanted, "engine, %s" % order, cases)
    finally:
        eng.close()


def test_inertial_batch_on_the_device_and_on_the_host(pkg, cases, alone, monkeypatch):
    """inertial_converged beside an ordinary inertial window: every entry gives the one-window call's bits under either solver, and the two
    solvers agree within test_reduced_system_on_the_device_and_on_the_host's bars."""
    c0 = cases["inertial_converged"]
    per_mode = {}
    for mode in ("1", "0"):
        env = {"TC2LI_LVI_DEVICE_SOLVE": mode}
        set_env(monkeypatch, env)
        assert pkg.capi.ba_options()["lvi_device_solve"] == int(mode)
        wanted = {n: alone[key(env), n] for n in INERTIAL_ORDER}
        for names in (INERTIAL_ORDER, INERTIAL_ORDER[::-1]):
            batch = pkg.capi.LviBatch([cases[n]["window"] for n in names], c0["calib24"], c0["cam"])
            for what, run in (("run(8)", lambda: batch.run(8)), ("run(1)", lambda: batch.run(1)), ("run_group(0)", lambda: batch.run_group(0))):
                assert run() == len(names)
                assert_batch_equals(batch, names, wanted, "solve on the %s, %s" % ("device" if mode == "1" else "host", what), cases)
        per_mode[mode] = wanted
        check_against_oracle("inertial_converged", wanted["inertial_converged"], c0, True)
    assert per_mode["1"]["inertial_ordinary"]["iterations"] > per_mode["1"]["inertial_converged"]["iterations"] == 3
    for n in INERTIAL_ORDER:
        a, b = per_mode["1"][n], per_mode["0"][n]
        assert (a["iterations"], a["trials"]) == (b["iterations"], b["trials"])
        assert abs(a["final_chi2"] - b["final_chi2"]) <= 1e-9 * abs(b["final_chi2"])
        assert np.allclose(a["state"], b["state"], rtol=1e-9, atol=1e-10) and np.allclose(a["points"], b["points"], rtol=1e-9, atol=1e-9)


def test_a_slot_carries_nothing_over_from_the_call_before(pkg, cases, alone, monkeypatch):
    """A group's slot table is pinned memory that stays from call to call, and the forms of the loop use different fields of a slot: the
    device-side LM its state pointers and stop word (lm, lm_host, stop_host), the host-driven forms none of them.  A slot that kept a
    pointer of the call before sends a host-driven window through the device's decisions (the inertial batch did once).  In one process
    and on one group: two LiDAR windows under the device-side LM, then two inertial windows, each of which must have the bits of its own
    one-window call; then the other way round, the LiDAR windows checked.  The two drivers keep a context each, so the same LiDAR batch
    also follows itself with the decisions on the host (TC2LI_BA_DEVICE_LM=0): there the table's memory is the same for certain.
    Windows of at most 6 keyframes."""
    group = 5
    c0 = cases["inertial_converged"]
    lidar = {"lidar_converged": cases["lidar_converged"], "lidar_first": cases["lidar_converged"]["first"]}
    names = tuple(lidar)
    assert all(len(c["window"]["poses"]) <= 6 and "win_pose" in c["window"] for c in lidar.values())
    assert all(len(cases[n]["window"]["kf33"]) <= 6 for n in INERTIAL_ORDER)
    set_env(monkeypatch, {})
    assert pkg.capi.ba_options()["device_lm"] == 1
    wanted = {n: run_alone(pkg, c["window"], c["cam"]) for n, c in lidar.items()}
    wanted.update({n: alone[(), n] for n in INERTIAL_ORDER})
    all_cases = dict(cases, **lidar)
    lv = pkg.capi.BaBatch([lidar[n]["window"] for n in names], lidar["lidar_converged"]["cam"])
    lvi = pkg.capi.LviBatch([cases[n]["window"] for n in INERTIAL_ORDER], c0["calib24"], c0["cam"])
    for first, second in (((lv, names), (lvi, INERTIAL_ORDER)), ((lvi, INERTIAL_ORDER), (lv, names))):
        for batch, which in (first, second):
            assert batch.run_group(group) == len(which)
        assert_batch_equals(second[0], second[1], wanted, "after the other driver's batch on group %d" % group, all_cases)
    assert lv.run_group(group) == len(names)
    set_env(monkeypatch, {"TC2LI_BA_DEVICE_LM": "0"})
    assert lv.run_group(group) == len(names)
    assert_batch_equals(lv, names, wanted, "host LM after device LM on group %d" % group, all_cases)


# ---- the fused forms ------------------------------------------------------------------------------------------------------------
FUSE_TRIAL_RTOL = 1e-9


def against_default(got, ref):
    """A fused form against the default -> (states, points, per-edge chi2, final chi2): the largest |a - b| / max(1, |b|) of each."""
    r = lambda a, b: float((np.abs(a - b) / np.maximum(1.0, np.abs(b))).max())
    return r(got["state"], ref["state"]), r(got["points"], ref["points"]), r(got["chi2"], ref["chi2"]), r(got["final_chi2"], ref["final_chi2"])


@pytest.mark.parametrize("form", sorted(FUSED))
def test_fused_forms(pkg, cases, alone, monkeypatch, form):
    """TC2LI_BA_FUSE_LIN=1 (the linearisation's closing sums by the window's last workgroup) and TC2LI_BA_FUSE_TRIAL=1 (k_ba_trial_fused,
    k_ba_trial_fused_b, k_ba_trial_fused_imu_b): every window against the oracle, batch against one-window call under the same switch bit for
    bit, and against the default -- the same bits for FUSE_LIN, 1e-9 for FUSE_TRIAL."""
    env = FUSED[form]
    names = ORDERS["exits first"] + ("duplicates",)
    default = {n: alone[(), n] for n in names + INERTIAL_ORDER}
    set_env(monkeypatch, env)
    opt = pkg.capi.ba_options()
    assert opt["fuse_linearize"] == int("TC2LI_BA_FUSE_LIN" in env) and opt["fuse_trial"] == int("TC2LI_BA_FUSE_TRIAL" in env)
    wanted = {n: alone[key(env), n] for n in names + INERTIAL_ORDER}
    for n in names + INERTIAL_ORDER:
        check_against_oracle("%s, %s" % (form, n), wanted[n], cases[n], n in bc.EXIT_CASES)
    batch = pkg.capi.BaBatch([cases[n]["window"] for n in names], cases["plain"]["cam"])
    for what, run in (("run(8)", lambda: batch.run(8)), ("run_group(0)", lambda: batch.run_group(0))):
        assert run() == len(names)
        assert_batch_equals(batch, names, wanted, "%s, %s" % (form, what), cases)
    c0 = cases["inertial_converged"]
    lvi = pkg.capi.LviBatch([cases[n]["window"] for n in INERTIAL_ORDER], c0["calib24"], c0["cam"])
    assert lvi.run(8) == len(INERTIAL_ORDER)
    assert_batch_equals(lvi, INERTIAL_ORDER, wanted, "%s, inertial run(8)" % form, cases)
    worst = np.zeros(4)
    for n in names + INERTIAL_ORDER:
        got, ref = wanted[n], default[n]
        assert (got["iterations"], got["trials"]) == (ref["iterations"], ref["trials"]) and np.array_equal(got["dpos"], ref["dpos"]), n
        if "TC2LI_BA_FUSE_TRIAL" not in env:
            d = difference(got, ref, "lidar" in ref and "win_pose" in cases[n]["window"])
            assert d is None, "%s: %s differs from the default form" % (n, d)
        else:
            worst = np.maximum(worst, against_default(got, ref))
    if "TC2LI_BA_FUSE_TRIAL" in env:
        print("%s against the default, largest relative difference: states %.3g, points %.3g, per-edge chi2 %.3g, final chi2 %.3g" % (form, *worst))
        assert worst.max() <= FUSE_TRIAL_RTOL
