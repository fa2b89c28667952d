"""The two kernels behind Optimizer::PoseOptimization (pose_opt_kernel.hip) against the oracle: the global-memory form that a batch takes when
its largest frame has more correspondences than the LDS form stages, the LDS form at the edges of its block sizes, batches that mix trivial and
large frames, and rounds in which no edge is active.  Every threshold comes from tc2li_pose_optimization_limits, and every test asserts which kernel
its calls launched (last_form: 1 = LDS, 2 = global memory).  Bar: test_ba_gpu.py's -- same inlier count, same outlier mask, poses within 1e-4
relative and 1e-6 absolute of the double-precision oracle."""
import numpy as np
import pytest

from pose_opt_cases import frame_problem

pytestmark = pytest.mark.gpu

POSE_RTOL = 1e-4  # the tolerance BASELINE.json states for optimised SE3 poses
LDS_FORM, GLOBAL_FORM = 1, 2
KF = 3            # the keyframe the single-frame cases are cut from: free, so its initial pose carries the window's pose noise


@pytest.fixture(scope="module")
def window(synthetic):
    """Four keyframes of 2487-2589 correspondences each, 10 % gross outliers -> (window, [frame_problem of every keyframe])."""
    w = synthetic.ba_window(3, n_opt=2, n_fix=2, n_points=6500, outlier_frac=0.1)
    return w, [frame_problem(w, k) for k in range(len(w["poses"]))]


@pytest.fixture(scope="module")
def limits(pkg):
    lim = pkg.pose_optimization_limits()
    assert lim["lds_granule"] >= 2 and lim["lds_max_edges"] >= 2 * lim["lds_granule"] + 1 and lim["threads"] > 0
    return lim


def last_form(pkg):
    return pkg.pose_optimization_limits()["last_form"]


def agrees(got, want, tag):
    """test_ba_gpu.py's bar; -> the largest absolute pose difference."""
    pose, out, inl = got
    want_pose, want_out, want_inl = want[:3]
    diff = float(np.abs(pose - want_pose).max())
    print("%s: n %d inliers %d (oracle %d) max |pose - oracle| %.3e" % (tag, len(want_out), inl, want_inl, diff))
    assert inl == want_inl, tag
    assert np.array_equal(out, want_out), tag
    assert np.allclose(pose, want_pose, rtol=POSE_RTOL, atol=1e-7), tag
    assert diff < 1e-6, tag
    return diff


def clean_case(oracle, w, k, Xw, ed):
    """The oracle's result for an unmodified stretch of a keyframe; the case must be an optimisation worth the name: three quarters inliers."""
    want = oracle.pose_optimization(w["poses"][k], Xw, ed, w["cam"])
    assert want[2] >= 0.75 * len(ed), (len(ed), want[2])
    return want


def test_limits_call(pkg, limits):
    assert pkg.pose_optimization_limits()["last_form"] in (0, LDS_FORM, GLOBAL_FORM)
    import ctypes as C
    out = (C.c_int32 * 3)()
    assert pkg.lib().tc2li_pose_optimization_limits(out, 3) < 0 and pkg.lib().tc2li_pose_optimization_limits(None, 4) < 0


def test_global_form_against_the_oracle(pkg, oracle, window, limits):
    w, frames = window
    L = limits["lds_max_edges"]
    Xw, ed = frames[KF]
    n_mono = 2100
    assert len(ed) > n_mono > L + 1
    mono = ed[:n_mono].copy(); mono[:, 4] = -1
    for tag, X, e in (("whole frame", Xw, ed), ("L + 1", Xw[:L + 1], ed[:L + 1]), ("monocular", Xw[:n_mono], mono)):
        want = clean_case(oracle, w, KF, X, e)
        got = pkg.pose_optimization(w["poses"][KF], X, pkg.pack_ba_edges(e), w["cam"])
        assert last_form(pkg) == GLOBAL_FORM, tag
        agrees(got, want, tag)


def test_lds_capacity_edges(pkg, oracle, window, limits):
    w, frames = window
    L, g = limits["lds_max_edges"], limits["lds_granule"]
    Xw, ed = frames[KF]
    ten_trials = []
    assert 2 * g + 1 < 1024 and 1025 < L - 1
    for n in (g - 1, g, g + 1, 2 * g, 2 * g + 1, 1024, 1025, L - 1, L):
        want = clean_case(oracle, w, KF, Xw[:n], ed[:n])
        if (want[3]["trials"] == 10).any():
            ten_trials.append(n)
        got = pkg.pose_optimization(w["poses"][KF], Xw[:n], pkg.pack_ba_edges(ed[:n]), w["cam"])
        assert last_form(pkg) == LDS_FORM, n
        agrees(got, want, "N = %d" % n)
    # an iteration whose ten trials are all rejected ends its round (g2o: qmax == _maxTrialsAfterFailure): the LM loop's other exit
    assert ten_trials, "no case with a ten-trial iteration"


def test_forms_give_the_same_bits_and_a_frame_does_not_depend_on_its_batch(pkg, oracle, window, limits):
    """Batch A's largest frame has L correspondences (LDS form), batch B is A plus a frame of L + 1 (global-memory form for every frame): a frame's
    pose, outlier flags and inlier count are the same bytes in A, in B and in a call of its own.  The kernel's claim: same loops, same order of
    the sums; the chi2 kept as float in LDS and as double in global memory reaches the classification as the same float."""
    w, frames = window
    L, g = limits["lds_max_edges"], limits["lds_granule"]
    # (size, keyframe, first edge): different keyframes and offsets, none a prefix of another
    cuts = [(0, 0, 5), (2, 1, 17), (3, 2, 31), (9, 3, 43), (10, 0, 59), (g, 1, 71), (g + 1, 2, 83), (1025, 3, 97), (L, 2, 113)]
    extra = (L + 1, 3, 131)
    assert len({(k, o) for _, k, o in cuts + [extra]}) == len(cuts) + 1 and g + 1 < 1025 < L

    def batch(cs):
        probs = [(frames[k][0][o:o + n], frames[k][1][o:o + n].copy()) for n, k, o in cs]
        for (n, k, o), (_, e) in zip(cs, probs):
            assert len(e) == n, (n, k, o)
            e[:, 0] = np.arange(n)
        offs = np.concatenate([[0], np.cumsum([n for n, _, _ in cs])])
        poses = np.stack([w["poses"][k] for _, k, _ in cs])
        got = pkg.pose_optimization_batch(poses, offs, np.concatenate([x for x, _ in probs]), pkg.pack_ba_edges(np.concatenate([e for _, e in probs])),
                                          w["cam"])
        return probs, offs, got

    probs, offs_a, (poses_a, out_a, inl_a) = batch(cuts)
    assert last_form(pkg) == LDS_FORM
    cuts_b = cuts[:4] + [extra] + cuts[4:]   # in the middle: the frames after it also move in the edge arrays
    where = [i if i < 4 else i + 1 for i in range(len(cuts))]
    probs_b, offs_b, (poses_b, out_b, inl_b) = batch(cuts_b)
    assert last_form(pkg) == GLOBAL_FORM
    worst = 0.0
    for i, (n, k, o) in enumerate(cuts):
        j = where[i]
        tag = "frame of %d" % n
        a = (poses_a[i], out_a[offs_a[i]:offs_a[i + 1]], int(inl_a[i]))
        b = (poses_b[j], out_b[offs_b[j]:offs_b[j + 1]], int(inl_b[j]))
        Xw, ed = probs[i]
        alone = pkg.pose_optimization(w["poses"][k], Xw, pkg.pack_ba_edges(ed), w["cam"])
        assert last_form(pkg) == LDS_FORM, tag
        for other, name in ((b, "global-memory batch"), (alone, "call of its own")):
            same = a[0].tobytes() == other[0].tobytes()
            print("%s: LDS batch against %s: pose bits %s, max |difference| %.3e" % (tag, name, "equal" if same else "DIFFER",
                                                                                      float(np.abs(a[0] - other[0]).max())))
            assert a[2] == other[2], (tag, name)
            assert np.array_equal(a[1], other[1]), (tag, name)
            assert same, (tag, name)
        want = oracle.pose_optimization(w["poses"][k], Xw, ed, w["cam"])
        if n >= g:
            assert want[2] >= 0.75 * n, tag
        worst = max(worst, agrees(a, want, tag + " (LDS batch)"), agrees(b, want, tag + " (global-memory batch)"))
    j = 4
    want = clean_case(oracle, w, extra[1], *probs_b[j])
    worst = max(worst, agrees((poses_b[j], out_b[offs_b[j]:offs_b[j + 1]], int(inl_b[j])), want, "frame of %d (global-memory batch)" % extra[0]))
    print("largest pose difference to the oracle: %.3e" % worst)


def randomised(ed, which):
    """The observations of the edges `which` replaced by points drawn over the image, all stereo: almost none agrees with its map point."""
    rng = np.random.default_rng(0)
    m = len(ed[which])
    e = ed.copy()
    u, v = rng.uniform(0, 1200, m), rng.uniform(0, 370, m)
    e[which, 2], e[which, 3], e[which, 4] = u, v, u - rng.uniform(1, 40, m)
    return e


def test_round_without_active_edges(pkg, oracle, window, limits):
    """Round 0 classifies every edge as an outlier.  g2o then has no active vertex and optimize() returns at once; the kernel builds H = 0, b = 0,
    its solver fails, ten trials are rejected and the pose stays -- the results must be the same: the frame's initial pose, rounded through float."""
    w, frames = window
    L = limits["lds_max_edges"]
    Xw, ed = frames[KF]
    initial = w["poses"][KF].astype(np.float32).astype(np.float64)
    assert 300 <= L < 2100
    for n, form in ((300, LDS_FORM), (2100, GLOBAL_FORM)):
        e = randomised(ed[:n], slice(None))
        want_pose, want_out, want_inl, trace = oracle.pose_optimization(w["poses"][KF], Xw[:n], e, w["cam"])
        # the case is what it claims
        assert want_inl == 0 and want_out.all() and len(want_out) == n
        assert len(trace["trials"]) == 10   # one round of ten iterations ran, the other three did nothing
        assert want_pose.tobytes() == initial.tobytes()
        pose, out, inl = pkg.pose_optimization(w["poses"][KF], Xw[:n], pkg.pack_ba_edges(e), w["cam"])
        assert last_form(pkg) == form, n
        print("no active edge, n %d: inliers %d, pose bits %s" % (n, inl, "equal" if pose.tobytes() == initial.tobytes() else "DIFFER"))
        assert inl == 0 and out.all() and len(out) == n
        assert pose.tobytes() == initial.tobytes()
    # every second edge randomised: the optimisation goes on over the good half
    n = 2200
    e = randomised(ed[:n], slice(1, None, 2))
    want = oracle.pose_optimization(w["poses"][KF], Xw[:n], e, w["cam"])
    assert 0.3 * n < want[2] < 0.5 * n and want[1][1::2].sum() > 0.95 * (n // 2)
    assert (want[3]["trials"] == 10).any()
    got = pkg.pose_optimization(w["poses"][KF], Xw[:n], pkg.pack_ba_edges(e), w["cam"])
    assert last_form(pkg) == GLOBAL_FORM
    agrees(got, want, "every second edge randomised")
