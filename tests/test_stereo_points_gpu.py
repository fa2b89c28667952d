"""GPU tests of tc2li_stereo_points_batch and tc2li_new_keyframe_batch against the host entries and the restatement
tests/stereo_points_ref.py, on every frame of tests/test_stereo_points.py, in several batch compositions.  Every output is an integer or a
float compared by its bits (stereo_points_cases.same): the criterion is equality, nothing is left out.  The sizes are the smallest at which
the kernel can go wrong: the wavefront boundary at 63 / 64 / 65 keypoints, the workgroup's at 257, the LDS limit at 4096, and max_point's
edge at 100 / 101 / 102 entries."""
import numpy as np
import pytest

import stereo_points_cases as K
import test_stereo_points as T

pytestmark = pytest.mark.gpu
U4 = K.UNPROJECT4


def _points(pkg, frames, want, what, **kw):
    got = pkg.stereo_points_batch(frames, U4, **kw)
    host = pkg.stereo_points_batch(frames, U4, host=True)
    assert len(got) == len(frames)
    for i, (g, h, w) in enumerate(zip(got, host, want)):
        K.assert_equal(g, h, "%s: frame %d, device against host" % (what, i))
        K.assert_equal(g, w, "%s: frame %d, device against the restatement" % (what, i))
    return got


def _decided(pkg, frames, decisions, want, what, **kw):
    got = pkg.new_keyframe_batch(frames, decisions, U4, **kw)
    host = pkg.new_keyframe_batch(frames, decisions, U4, host=True)
    assert len(got) == len(frames)
    for i, (g, h, w) in enumerate(zip(got, host, want)):
        K.assert_equal(g, h, "%s: frame %d, device against host" % (what, i), T.ALL_OUTPUTS)
        K.assert_equal(g, w, "%s: frame %d, device against the restatement" % (what, i), T.ALL_OUTPUTS)
    return got


class _Device:
    """the package with host=True turned into the device entry, for the hand-made tests of test_stereo_points.py"""

    def __init__(self, pkg):
        self.pkg = pkg

    def __getattr__(self, name):
        return getattr(self.pkg, name)

    def stereo_points_batch(self, frames, u4, host=False, **kw):
        return self.pkg.stereo_points_batch(frames, u4, host=False, **kw)

    def new_keyframe_batch(self, frames, decisions, u4, host=False, **kw):
        return self.pkg.new_keyframe_batch(frames, decisions, u4, host=False, **kw)


def test_device_hand_made_cases(pkg):
    """The rules one by one go through the kernel: the hand-made frames and decisions of test_stereo_points.py with the device entries,
    against the restatement and the expectations written by hand there, then against the host entries."""
    dev = _Device(pkg)
    T.test_hand_made_frames(dev)
    T.test_unprojection_by_hand(dev)
    T.test_hand_made_decisions(dev)
    _points(pkg, [f for _, f in K.hand_frames()], T.hand_frames_expected(), "hand-made")
    cases = K.hand_decisions()
    _decided(pkg, [c[1] for c in cases], [c[2] for c in cases], T.hand_decisions_expected(), "hand-made")


def test_device_one_batch(pkg):
    frames, decisions = K.family()
    points, decided = T.family_expected()
    _points(pkg, list(frames), points, "one batch")
    _decided(pkg, list(frames), list(decisions), decided, "one batch")


def test_device_batches_of_one(pkg):
    frames, decisions = K.family()
    points, decided = T.family_expected()
    for i in range(len(frames)):
        _points(pkg, [frames[i]], [points[i]], "frame %d alone" % i)
        _decided(pkg, [frames[i]], [decisions[i]], [decided[i]], "frame %d alone" % i)


def test_device_shuffled_and_reversed(pkg):
    frames, decisions = K.family()
    points, decided = T.family_expected()
    order = np.random.default_rng(5).permutation(len(frames))
    for what, o in (("shuffled", order), ("reversed", np.arange(len(frames))[::-1])):
        _points(pkg, [frames[i] for i in o], [points[i] for i in o], what)
        _decided(pkg, [frames[i] for i in o], [decisions[i] for i in o], [decided[i] for i in o], what)


def test_device_batch_of_512_mixed(pkg):
    """512 frames in one call, drawn from the hand-made ones and the family, every one at least once."""
    frames, decisions = K.family()
    points, decided = T.family_expected()
    fa, wa = [f for _, f in K.hand_frames()] + list(frames), T.hand_frames_expected() + points
    pick = np.random.default_rng(6).integers(0, len(fa), 512)
    pick[:len(fa)] = np.arange(len(fa))
    assert len(_points(pkg, [fa[i] for i in pick], [wa[i] for i in pick], "512")) == 512
    cases = K.hand_decisions()
    fb, db, wb = [c[1] for c in cases] + list(frames), [c[2] for c in cases] + list(decisions), T.hand_decisions_expected() + decided
    pick = np.random.default_rng(7).integers(0, len(fb), 512)
    pick[:len(fb)] = np.arange(len(fb))
    assert len(_decided(pkg, [fb[i] for i in pick], [db[i] for i in pick], [wb[i] for i in pick], "512")) == 512


def test_device_empty_batch(pkg):
    assert pkg.stereo_points_batch([], U4) == [] and pkg.new_keyframe_batch([], [], U4) == []


def test_device_on_a_callers_stream(pkg):
    import torch
    frames, decisions = K.family()
    points, decided = T.family_expected()
    s = torch.cuda.Stream()
    _points(pkg, list(frames[:16]), points[:16], "caller's stream", stream=s.cuda_stream)
    _decided(pkg, list(frames[:16]), list(decisions[:16]), decided[:16], "caller's stream", stream=s.cuda_stream)
    s.synchronize()


def test_device_batch_of_noes(pkg):
    """need is false in every frame: no created points, the counts still right."""
    frames, _ = K.family()
    frames = list(frames[:21])
    decisions = [K.decision(only_tracking=1) if i % 3 == 0 else K.decision(mapper_stopped=1) if i % 3 == 1 else K.decision(frame_id=10, last_keyframe_id=5, n_kfs=31) for i in range(21)]
    want = [T.ref.new_keyframe(f, d, U4) for f, d in zip(frames, decisions)]
    got = _decided(pkg, frames, decisions, want, "all no")
    for f, g in zip(frames, got):
        assert g["need"] == 0 and g["n_created"] == 0 and g["n_visited"] == 0 and len(g["created_keypoint"]) == 0
        assert g["n_with_depth"] == int((f["depth"] > 0).sum())
        close = (f["depth"] > 0) & (f["depth"] < f["th_depth"])
        assert g["n_tracked_close"] + g["n_non_tracked_close"] == int(close.sum())


# ---- the buffers kept between calls -------------------------------------------------------------------------------------------------------
def _tiny():
    """The family's frames of 63, 64 and 65 keypoints with their decisions, the first 16."""
    frames, decisions = K.family()
    pick = [k for k in range(len(frames)) if len(frames[k]["depth"]) <= 65][:16]
    return [frames[k] for k in pick], [decisions[k] for k in pick]


def _equal_host(pkg, frames, decisions, what):
    got = pkg.stereo_points_batch(frames, U4)
    host = pkg.stereo_points_batch(frames, U4, host=True)
    dec = pkg.new_keyframe_batch(frames, decisions, U4)
    dech = pkg.new_keyframe_batch(frames, decisions, U4, host=True)
    assert len(got) == len(host) == len(dec) == len(dech) == len(frames)
    for i in range(len(frames)):
        K.assert_equal(got[i], host[i], "%s: frame %d, points, device against host" % (what, i))
        K.assert_equal(dec[i], dech[i], "%s: frame %d, decision, device against host" % (what, i), T.ALL_OUTPUTS)
    return got, dec


def test_device_reuses_its_buffers_across_batch_sizes(pkg):
    """8 frames, then 1 other, then the 8 again through the same buffers, the two entries in turn: nothing of an earlier call shows in a
    later one."""
    frames, decisions = _tiny()
    _equal_host(pkg, frames, decisions, "fill")                                      # whatever the tests before left, the buffers are larger than the calls below need
    first = _equal_host(pkg, frames[:8], decisions[:8], "8")
    assert sum(g["n_created"] for g in first[0]) > 100 and {int(g["need"]) for g in first[1]} == {0, 1}
    _equal_host(pkg, frames[8:9], decisions[8:9], "1")
    again = _equal_host(pkg, frames[:8], decisions[:8], "8 again")
    for i in range(8):
        K.assert_equal(first[0][i], again[0][i], "frame %d, points, first against third call" % i)
        K.assert_equal(first[1][i], again[1][i], "frame %d, decision, first against third call" % i, T.ALL_OUTPUTS)


def test_device_empty_frame_inside_a_batch(pkg):
    """A frame without keypoints, decided without ref_nobs, between two ordinary ones: its tables are empty places in the concatenation."""
    frames, decisions = _tiny()
    empty, plain = K.frame([]), K.decision(frame_id=120)
    got, dec = _equal_host(pkg, [frames[0], empty, frames[1]], [decisions[0], plain, decisions[1]], "empty in the middle")
    assert got[1]["n_created"] == 0 and got[1]["n_with_depth"] == 0 and len(got[1]["created_keypoint"]) == 0 and dec[1]["n_created"] == 0
    _equal_host(pkg, [empty, frames[0], empty], [plain, decisions[0], plain], "empty at both ends")
    _equal_host(pkg, [empty], [plain], "empty alone")


def test_device_two_callers_at_once(pkg):
    """Two threads, four calls each on batches of four of their own: each gets its own results.  The two entries share their buffers, so
    one thread creates points and the other decides."""
    import two_callers
    frames, decisions = _tiny()
    batches = [[[8 * t + (2 * s + i) % 8 for i in range(4)] for s in range(4)] for t in (0, 1)]
    points = [[frames[k] for k in b] for b in batches[0]]
    decided = [([frames[k] for k in b], [decisions[k] for k in b]) for b in batches[1]]

    def call(b):
        return pkg.new_keyframe_batch(b[0], b[1], U4) if isinstance(b, tuple) else pkg.stereo_points_batch(b, U4)

    got = two_callers.run(call, points, decided)
    for c in range(4):
        want = pkg.stereo_points_batch(points[c], U4, host=True)
        wantd = pkg.new_keyframe_batch(decided[c][0], decided[c][1], U4, host=True)
        assert len(got[0][c]) == len(got[1][c]) == 4
        for i in range(4):
            K.assert_equal(got[0][c][i], want[i], "points, call %d, frame %d" % (c, i))
            K.assert_equal(got[1][c][i], wantd[i], "decision, call %d, frame %d" % (c, i), T.ALL_OUTPUTS)
