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
