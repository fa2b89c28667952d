"""The windows of ba_exit_cases.py are what they claim to be: shown with the oracle alone, before any GPU sees them
(test_ba_exits_gpu.py compares the product with the oracle on the same windows).

What is read from the oracle's trace.  Iteration k starts at chi2[k] (chi2[0] from the oracle's own edge errors at the input) and leaves
chi2[k + 1]; its relative decrease is d[k] = (chi2[k] - chi2[k + 1]) / chi2[k].  The loop counts an iteration as stalled when
d[k] < 1e-3 and ends at three in a row; it ends at once when rho == 0, which with finite numbers means d[k] == 0 exactly.

Margins.  Product and oracle sum the same terms in different orders; on a visual window their final chi2 agrees to 1e-9 or better
(test_ba_gpu.py asks 1e-6), on an inertial window to 3e-6 (the product evaluates the bias-corrected pre-integration in float,
test_inertial_ba_gpu.py).  A decision both must share needs room for that:
  * every accepted step lowers chi2 by at least 1e-8 of it (visual) -- by at least 1e-5 on the inertial window, three times the 3e-6;
  * every stalled step stays at or below 1e-4, a tenth of the 1e-3 bar, and every step that counts as progress is at least 1.5e-3;
  * no trial is rejected in an exit case: a rejection at a stalled window is a decision at the rounding level;
  * every edge's chi2 is at least 1e-3 of its gate (5.991 / 7.815) away from it, a hundred times test_ba_gpu.py's bar for per-edge chi2,
    and every depth is at least 0.05 m from zero.

What was measured (d per iteration; lambda after the last one):
  plain                 10 iterations, d = 0.27 .. 1.9e-3, lambda 8.1e-4, 25 outliers
  converged             3, d = 9.7e-6, 3.0e-6, 9.8e-7, lambda 8.67
  rho_zero              2, d = 4.0e-8, 0 (seed 12), lambda 1.33e30
  stall_after_progress  6, d = 0.32, 4.7e-2, 2.5e-3, 9.3e-5, 2.1e-5, 7.6e-6
  rotated_a / _b / _c   as plain: 10 iterations, the same 25 outliers; final chi2 1.5e-6 / 6e-8 / 1.9e-5 from the plain window's (the
                        float32 rounding of coordinates of some 600 m is 3e-5 m)
  behind                10, one depth flag 0 (depth -1.65 m; the landmark's other depths 2.1 to 4.1 m), 36 outliers
  close                 10, all flags 1, final chi2 1.9e-6 from the plain window's
  lidar_converged       3, d = 3.1e-5, 1.7e-5, 1.6e-5, 27 planes
  inertial_converged    3, d = 4.1e-5, 3.2e-5, 5.5e-5

Two findings on the way.  The inertial window fed back after a FULL run (9 iterations, ended by n_bad) is no usable case: with
lambda_init = 1 the loop is Gauss-Newton at the scale of the inertial information (1e6 .. 1e9), the first step lowers chi2 by 4.7e-7 and
the second is rejected ten times at constant chi2 (d = 4e-16) -- the qmax == 10 exit, but reached by a decision at the rounding level,
which the product's float pre-integration cannot be asked to share.  The case is therefore the window after FIVE iterations of the
first run (as when the tracking thread interrupts it), from which three steps of 3e-5 to 6e-5 remain.  No window with finite input was
found that reaches qmax == 10 otherwise (LiDAR weights up to 1e9 let lambda outgrow the step first): that exit has no case.

What these margins rule out: n_bad reset from a count above zero.  A stalled step of 1e-4 or less followed by a step of 1.5e-3 or more
asks the decrease to grow fifteen-fold from one iteration to the next, and an accepted step lowers lambda by a factor of three at the
most; stall_after_progress therefore resets n_bad from zero only, and the count that starts again is seen in its last three steps."""
import numpy as np
import pytest

import ba_exit_cases as bc

CAP = bc.ITERATIONS
MIN_DECREASE = {"visual": 1e-8, "inertial": 1e-5}
MAX_STALL, STALL_BAR, MIN_PROGRESS = 1e-4, 1e-3, 1.5e-3
GATE_CLEARANCE, DEPTH_CLEARANCE = 1e-3, 0.05
# iterations and trials of every case: what test_ba_exits_gpu.py's docstring lists
EXPECTED = {"plain": (10, [1] * 10), "converged": (3, [1] * 3), "rho_zero": (2, [1] * 2), "stall_after_progress": (6, [1] * 6),
            "rotated_a": (10, [1] * 10), "rotated_b": (10, [1] * 10), "rotated_c": (10, [1] * 10), "behind": (10, [1] * 10), "close": (10, [1] * 10),
            "lidar_converged": (3, [1] * 3), "inertial_converged": (3, [1] * 3)}


@pytest.fixture(scope="module")
def cases(pkg, oracle, synthetic):
    return bc.catalogue(pkg, oracle, synthetic)


def decreases(c):
    _, _, chi2, _ = bc.trace(c)
    return (chi2[:-1] - chi2[1:]) / chi2[:-1]


def n_bad_counts(d):
    """n_bad after every iteration, as the loop counts it."""
    out, n = [], 0
    for x in d:
        n = n + 1 if x < STALL_BAR else 0
        out.append(n)
    return out


@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_case_takes_the_steps_it_is_named_for(cases, name):
    c = cases[name]
    bc.assert_clean(c)
    it, trials, chi2, lam = bc.trace(c)
    d = decreases(c)
    print(name, "iterations", it, "trials", trials, "d", d, "lambda", lam[-1])
    assert (it, trials) == EXPECTED[name]
    assert len(chi2) == it + 1 and np.isfinite(chi2).all() and np.isfinite(lam).all()
    low = MIN_DECREASE["inertial" if name == "inertial_converged" else "visual"]
    for k, x in enumerate(d):
        if x == 0.0:
            continue  # rho == 0: the step was not accepted
        assert x >= low, (k, x)
        assert x <= MAX_STALL or x >= MIN_PROGRESS, (k, x)
    if name in bc.EXIT_CASES:
        assert it < CAP and all(t == 1 for t in trials)


@pytest.mark.parametrize("name", ["converged", "lidar_converged", "inertial_converged"])
def test_converged_windows_end_by_three_stalled_steps(cases, name):
    d = decreases(cases[name])
    assert n_bad_counts(d) == [1, 2, 3] and (d > 0).all()


def test_rho_zero_ends_on_a_step_that_changes_nothing(cases):
    c = cases["rho_zero"]
    d = decreases(c)
    want = c["want"]
    assert d[0] >= bc.RHO_ZERO_ROOM * 1e-8 and d[1] == 0.0 and want[5]["chi2"][0] == want[5]["chi2"][1]
    # accepted (lambda x 2/3), then not accepted (lambda x 2); n_bad was 1, the loop ended through ok = false
    assert np.allclose(want[5]["lam"], [1e30 * 2 / 3, 1e30 * 4 / 3], rtol=1e-12)
    # what the first step did: the float32 quaternions became unit quaternions, nothing else moved
    w = c["window"]
    free = w["fixed"] == 0
    assert np.abs(np.linalg.norm(w["poses"][free, :4], axis=1) - 1).max() > 1e-9
    assert np.abs(np.linalg.norm(want[0][free, :4], axis=1) - 1).max() < 1e-15
    assert np.array_equal(want[1], w["points"]) and np.array_equal(want[0][:, 4:], w["poses"][:, 4:])
    assert np.abs(want[0] - w["poses"]).max() < 1e-7


def test_stall_after_progress_counts_from_zero_after_real_steps(cases):
    d = decreases(cases["stall_after_progress"])
    assert n_bad_counts(d) == [0, 0, 0, 1, 2, 3]
    assert cases["stall_after_progress"]["want"][5]["lam"][0] < 1e-300   # Gauss-Newton throughout


def test_plain_window_runs_to_the_cap(cases):
    d = decreases(cases["plain"])
    assert n_bad_counts(d) == [0] * CAP


@pytest.mark.parametrize("name", sorted(bc.ROTATIONS))
def test_moved_world_frame_is_the_same_problem(cases, name):
    c, plain = cases[name], cases["plain"]
    w, want, pw = c["window"], c["want"], plain["want"]
    assert bc.trace(c)[:2] == bc.trace(plain)[:2]
    assert np.array_equal(bc.outliers(c["edges6"], want[2], want[3]), bc.outliers(plain["edges6"], pw[2], pw[3]))
    assert abs(want[5]["chi2"][-1] - pw[5]["chi2"][-1]) <= 1e-4 * pw[5]["chi2"][-1]
    # the result, moved back, is the plain window's result
    Rm, tm, pts = bc.move_back(want[0], want[1], *c["transform"])
    Rp, tp = bc.pose_matrices(pw[0])
    print(name, "against the plain window: rotations %.2e, translations %.2e, points %.2e, final chi2 %.2e" % (
        np.abs(Rm - Rp).max(), bc.rel(tm, tp), bc.rel(pts, pw[1]), abs(want[5]["chi2"][-1] / pw[5]["chi2"][-1] - 1)))
    assert np.abs(Rm - Rp).max() < 1e-4 and bc.rel(tm, tp) < 1e-4 and bc.rel(pts, pw[1]) < 1e-4
    qw = np.abs(w["poses"][:, 3])
    if name == "rotated_b":
        assert qw.max() < 0.1
    if name == "rotated_c":
        assert np.abs(w["poses"][:, 4:]).max() > 300 and np.abs(w["points"]).max() > 300
    assert qw.max() < 0.7   # none of the three is near the identity


def test_behind_leaves_one_depth_flag_at_zero(cases):
    c = cases["behind"]
    want, e = c["want"], c["edges6"]
    assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and np.isfinite(want[2]).all()
    assert np.flatnonzero(want[3] == 0).tolist() == [c["edge"]]
    mine = np.flatnonzero(e[:, 0] == c["point"])
    assert len(mine) == 4 and mine[-1] == c["edge"] and want[3][mine].tolist() == [1, 1, 1, 0]
    z0 = bc.depths(c["window"]["poses"], c["window"]["points"], e)
    assert abs(z0[c["edge"]] + 0.5) < 1e-4 and (z0 < 1.0).sum() == 1   # the input: this edge alone, -0.5 m
    z = bc.depths(want[0], want[1], e)
    assert z[c["edge"]] < -DEPTH_CLEARANCE and np.delete(z, c["edge"]).min() > DEPTH_CLEARANCE
    # the flag decides: the edge is an outlier whatever its chi2
    assert bc.outliers(e, want[2], want[3])[c["edge"]]


def test_close_recovers_to_the_plain_optimum(cases):
    c, plain = cases["close"], cases["plain"]
    want, pw = c["want"], plain["want"]
    z0 = bc.depths(c["window"]["poses"], c["window"]["points"], c["edges6"])
    assert abs(z0[c["edge"]] - 0.05) < 1e-4 and z0.min() > 0
    assert (want[3] == 1).all() and bc.depths(want[0], want[1], c["edges6"]).min() > DEPTH_CLEARANCE
    assert np.array_equal(bc.outliers(c["edges6"], want[2], want[3]), bc.outliers(plain["edges6"], pw[2], pw[3]))
    assert abs(want[5]["chi2"][-1] - pw[5]["chi2"][-1]) <= 1e-4 * pw[5]["chi2"][-1]
    # the landmark is back where the plain window has it (neither run is converged to more than that after 10 iterations)
    assert bc.rel(want[1][c["point"]], pw[1][c["point"]]) < 1e-2 and bc.rel(want[0], pw[0]) < 1e-3


@pytest.mark.parametrize("name", bc.ALL_CASES)
def test_no_edge_sits_on_a_gate(cases, name):
    c = cases[name]
    want, e = c["want"], c["edges6"]
    gate = np.where(e[:, 4] >= 0, bc.TH_HUBER2[1], bc.TH_HUBER2[0])
    clearance = np.abs(want[2] / gate - 1).min()
    print(name, "closest chi2 to its gate: %.2e of the gate; outliers %d" % (clearance, bc.outliers(e, want[2], want[3]).sum()))
    assert clearance >= GATE_CLEARANCE
    if name != "inertial_converged":
        assert np.abs(bc.depths(want[0], want[1], e)).min() > DEPTH_CLEARANCE


def test_lidar_edge_takes_part(cases):
    c = cases["lidar_converged"]
    assert c["want"][6] > 10 and c["first"]["want"][4] == CAP
    # the fed-back window is the first run's result in float32
    assert np.array_equal(c["window"]["poses"], bc.f32(c["first"]["want"][0])) and np.array_equal(c["window"]["points"], bc.f32(c["first"]["want"][1]))
    assert np.abs(c["first"]["want"][0] - cases["plain"]["want"][0]).max() > 1e-8
