"""Directed tests of k_pose_inertial / k_pose_inertial_batch (pose_inertial_kernel.hip) against the oracle, on the hand-made
frames of pose_inertial_cases.py.

The scene tests of test_pose_inertial_gpu.py reach a branch only where a random scene happens to put an edge.  Here every gate has
an edge on either side of it (A), the n_graph_edges < 10 break is straddled in both forms (B), the recovery pass is entered and not
entered at 29 / 30 inliers with and without bRecInit (C), the edge counts sit on the strides of the 128- and 256-lane loops (D), the
factorisation fails at once (E) and after accepted increments (F), the prior edge's Huber weight is active (G), and the
pre-integrated rotation takes the Jacobi sweeps of pi_normalize_rotation_f (H).  That each frame reaches its branch is shown in
test_pose_inertial_cases.py from the oracle alone; this file only compares: the check() that test_pose_inertial_gpu.py uses, with no slack on
the flags -- both states and the 21 mean values of the new prior within 1e-4, its H within 1e-4 of its scale, flags, counts, the
return value and solver_failed as the oracle has them.

Then the launch: all frames of B and D, the two failure frames and G in one launch give each frame the bits it gets alone (the kernel
has no atomics; an edge-less frame shares its edge_off with its neighbour), and the same list tiled past 256 frames gives them again
from k_pose_inertial_batch."""
import ctypes as C

import numpy as np
import pytest

import pose_inertial_cases as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def frames(pkg, oracle, synthetic):
    return pc.catalogue(pkg, oracle, synthetic)


@pytest.fixture(scope="module")
def wanted(frames, oracle):
    return {name: pc.run_oracle(oracle, w) for name, w in frames.items()}


@pytest.fixture(scope="module")
def alone(frames, pkg):
    """name -> the product's result for the frame in a launch of its own (computed once, on first use)."""
    class Alone(dict):
        def __missing__(self, name):
            w = frames[name]
            self[name] = pkg.capi.pose_inertial_optimization_batch([pc.item(w)], w["calib24"], w["cam"])[0]
            return self[name]
    return Alone()


def same_bits(a, b):
    return all(np.array_equal(a[k], b[k]) for k in range(4)) and a[4] == b[4] and a[5] == b[5] and a[6] == b[6]


def differences(got, want):
    H, wH = got[3][21:].reshape(15, 15), want[3][21:].reshape(15, 15)
    return pc.rel(got[0][:24], want[0][:24]), pc.rel(got[1][:24], want[1][:24]), np.abs(H - wH).max() / np.abs(wH).max()


@pytest.mark.parametrize("family", ["A", "B", "C", "D", "E", "F", "G", "H"])
def test_family_against_the_oracle(frames, wanted, alone, family):
    names = [n for n in frames if n.split("/")[0] == family]
    assert names
    worst = np.zeros(3)
    for name in names:
        got, want = alone[name], wanted[name]
        worst = np.maximum(worst, differences(got, want))
        try:
            pc.check(got, want, n_flag_slack=0, solver_failed=want[6]["solver_failed"])
        except AssertionError as e:
            raise AssertionError("frame %s: flags %s against %s, counts %s against %s, failed %s against %s, differences %s" % (
                name, np.nonzero(got[2])[0], np.nonzero(want[2])[0], got[5], want[5], got[6], want[6]["solver_failed"], differences(got, want))) from e
    print("family %s, %d frames: largest difference of the frame's state %.2e, of the other state %.2e, of the new prior's H %.2e of its scale" % (
        family, len(names), *worst))


def test_the_failure_frames_fail_and_the_others_do_not(frames, wanted, alone):
    for name in ("E", "F", "G", "B/pf/0", "B/kf/0"):
        assert alone[name][6] == wanted[name][6]["solver_failed"] == (name in ("E", "F"))
    # E: the zero increment was applied; F: the increment applied once more moved both states
    assert np.array_equal(alone["E"][0][21:24], frames["E"]["cur33"][21:24]) and np.array_equal(alone["E"][1][21:24], frames["E"]["other33"][21:24])
    assert np.linalg.norm(alone["F"][1][21:24] - frames["F"]["other33"][21:24]) > 100 * pc.RTOL


def test_zero_edge_previous_frame_form_in_full(frames, wanted, alone):
    """Both states, the whole prior, counts and return value of the previous-frame form without edges (30 unknowns, the inertial, the
    random-walk and the prior edge alone), not the frame's first 24 values only."""
    got, want = alone["B/pf/0"], wanted["B/pf/0"]
    pc.check(got, want)
    assert got[4] == 0 and got[5] == (0, 0, 0) and len(got[2]) == 0
    assert not np.array_equal(got[1], frames["B/pf/0"]["other33"])  # the previous state moved
    assert want[6]["rounds"] == (10, -1, -1, -1)


def mixed_list(frames):
    names = [n for n in frames if n[0] in "BD"]
    # an edge-less frame between two non-empty ones: its edge_off is the next frame's
    names += ["D/0/kf/129", "B/kf/0", "D/1/pf/257", "B/pf/0", "B/pf/1", "E", "F", "G"]
    return names


def test_one_mixed_launch_gives_every_frame_the_bits_it_gets_alone(pkg, frames, alone):
    names = mixed_list(frames)
    k = names.index("B/kf/0", len(names) - 8)
    assert len(frames[names[k - 1]]["edges"]) > 0 and len(frames[names[k + 1]]["edges"]) > 0 and len(names) <= 256
    w0 = frames[names[0]]
    got = pkg.capi.pose_inertial_optimization_batch([pc.item(frames[n]) for n in names], w0["calib24"], w0["cam"])
    for name, g in zip(names, got):
        assert same_bits(g, alone[name]), name


def test_the_batch_kernel_gives_the_same_bits(pkg, frames, alone):
    """More than 256 frames: k_pose_inertial_batch.  Compared in full: the failure frames, the 1-edge and the edge-less frames, and the
    frames around position 256."""
    names = mixed_list(frames)
    tiled = [names[k % len(names)] for k in range(258)]
    assert len(names) < 256
    w0 = frames[names[0]]
    got = pkg.capi.pose_inertial_optimization_batch([pc.item(frames[n]) for n in tiled], w0["calib24"], w0["cam"])
    must = {"E", "F", "G", "B/kf/0", "B/pf/0", "B/kf/1", "B/pf/1", "D/0/kf/1", "D/1/pf/257"}
    seen = set()
    for k, (name, g) in enumerate(zip(tiled, got)):
        assert same_bits(g, alone[name]), (k, name)
        seen.add(name)
    assert must <= seen


def raw_call(pkg, w, **override):
    """tc2li_pose_inertial_optimization_batch for one frame with the struct filled by hand, so that a field can be made invalid."""
    capi = pkg.capi
    Xw, e, cl = np.ascontiguousarray(w["Xw"], np.float64), np.ascontiguousarray(w["packed_edges"], capi.BA_EDGE_DTYPE), np.ascontiguousarray(w["close"], np.uint8)
    out = np.zeros(max(len(e), 1), np.uint8)
    prior_in, prior_out = capi.PoseImuPrior(), capi.PoseImuPrior()
    C.memmove(C.addressof(prior_in), np.ascontiguousarray(w["prior246"], np.float64).ctypes.data, 246 * 8)
    a = capi.PoseInertialProblem()
    C.memmove(a.frame, np.ascontiguousarray(w["cur33"], np.float64).ctypes.data, 33 * 8)
    C.memmove(a.other, np.ascontiguousarray(w["other33"], np.float64).ctypes.data, 33 * 8)
    a.prior, a.preintegrated, a.preintegrated_rw = C.addressof(prior_in), C.addressof(w["pre"].p), C.addressof(w["pre"].p)
    a.Xw, a.edges, a.close_point, a.outlier, a.prior_out = Xw.ctypes.data, e.ctypes.data, cl.ctypes.data, out.ctypes.data, C.addressof(prior_out)
    a.n_edges, a.last_frame, a.rec_init = len(e), 1, 0
    for k, v in override.items():
        setattr(a, k, v)
    res = np.zeros(1, np.int32)
    f = capi.lib().tc2li_pose_inertial_optimization_batch
    f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    return capi._check(f(C.addressof(a), 1, np.ascontiguousarray(w["calib24"], np.float64).ctypes.data, np.ascontiguousarray(w["cam"], np.float64).ctypes.data,
                         res.ctypes.data, C.c_void_p(0)))


@pytest.mark.parametrize("override", [dict(n_edges=-1), dict(Xw=None), dict(preintegrated_rw=None)], ids=["negative_n_edges", "null_Xw", "null_preintegrated_rw"])
def test_argument_errors(pkg, frames, override):
    w = frames["B/pf/10"]
    with pytest.raises(pkg.capi.Tc2liError, match="frame 0: invalid argument"):
        raw_call(pkg, w, **override)


def test_the_hand_filled_call_is_a_valid_call(pkg, frames, alone):
    """raw_call() without an invalid field is accepted: the errors above are due to the field each of them changes."""
    assert raw_call(pkg, frames["B/pf/10"]) == 1
