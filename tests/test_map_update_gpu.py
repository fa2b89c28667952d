"""GPU tests of the map update of IMU initialisation: tc2li_apply_scaled_rotation_batch and tc2li_gba_map_correction_batch against the host
entries and the restatement tests/map_update_ref.py, on the case family of tests/test_map_update.py in several batch compositions.  Float
outputs are compared by bit pattern: the criterion is equality, nothing is left out, there is no tolerance."""
import numpy as np
import pytest

import map_update_cases as K
import map_update_ref as ref
from test_map_update import gba, gba_at_capacity, gba_family, rot, rot_family

pytestmark = pytest.mark.gpu


def _check(pkg, call, problems, want, what):
    got = call(pkg, problems, host=False)
    host = call(pkg, problems, host=True)
    assert len(got) == len(problems)
    for i, (g, h, w) in enumerate(zip(got, host, want)):
        K.assert_equal(g, h, "%s: problem %d, device against host" % (what, i))
        K.assert_equal(g, w, "%s: problem %d, device against the restatement" % (what, i))
    return got


FAMILIES = pytest.mark.parametrize("call,family", [(rot, rot_family), (gba, gba_family)], ids=["rotation", "correction"])


@FAMILIES
def test_device_one_batch(pkg, call, family):
    problems, want = family()
    _check(pkg, call, problems, want, "one batch")
    assert call(pkg, [], host=False) == []


@FAMILIES
def test_device_batches_of_one(pkg, call, family):
    problems, want = family()
    for i, (p, w) in enumerate(zip(problems, want)):
        _check(pkg, call, [p], [w], "problem %d alone" % i)


@FAMILIES
def test_device_shuffled_and_reversed(pkg, call, family):
    problems, want = family()
    order = np.random.default_rng(5).permutation(len(problems))
    _check(pkg, call, [problems[i] for i in order], [want[i] for i in order], "shuffled")
    _check(pkg, call, problems[::-1], want[::-1], "reversed")


def test_device_512_tiny_rotations(pkg):
    tiny = K.tiny_rot_problems(64)
    want = [ref.apply_scaled_rotation(p, K.FILL) for p in tiny]
    pick = np.random.default_rng(6).integers(0, 64, 512)
    pick[:64] = np.arange(64)
    assert len(_check(pkg, rot, [tiny[i] for i in pick], [want[i] for i in pick], "512")) == 512


def test_device_512_tiny_corrections(pkg):
    tiny = K.tiny_gba_problems(64)
    want = [ref.gba_map_correction(p) for p in tiny]
    pick = np.random.default_rng(7).integers(0, 64, 512)
    pick[:64] = np.arange(64)
    assert len(_check(pkg, gba, [tiny[i] for i in pick], [want[i] for i in pick], "512")) == 512


def test_device_correction_at_capacity(pkg):
    """4096 keyframes fill the walk's LDS state; a chain of 4097 is refused by the CPU test."""
    pr, want = gba_at_capacity()
    small = K.cut_tree()
    _check(pkg, gba, [small, pr, small], [ref.gba_map_correction(small), want, ref.gba_map_correction(small)], "4096 keyframes")


def test_device_reuses_its_buffers(pkg):
    """A large batch, then a small one, then the large one again through the same buffers: nothing of an earlier call shows in a later one."""
    for call, family in ((rot, rot_family), (gba, gba_family)):
        problems, want = family()
        first = _check(pkg, call, problems, want, "first")
        _check(pkg, call, problems[1:2], want[1:2], "small")
        again = call(pkg, problems, host=False)
        for i, (a, b) in enumerate(zip(first, again)):
            K.assert_equal(a, b, "problem %d, first against third call" % i)


def test_rotation_equals_map_points_refresh(pkg):
    """Normals and distances of the rotation equal tc2li_map_points_refresh run on the rotation's own output positions and camera centres,
    for the points within that entry's cap of 112 observations.  Here and not among the CPU tests because that entry has no host twin."""
    problems, _ = rot_family()
    rng = np.random.default_rng(8)
    for pr in (problems[2], problems[3], K.identity_problem()):
        got = rot(pkg, [pr], host=False)[0]
        n = np.diff(pr["obs_offsets"])
        keep = np.flatnonzero((n > 0) & (n <= 112) & (pr["point_bad"] == 0))
        assert len(keep) >= 3 and n[keep].max() >= (65 if len(pr["kf_pose7"]) >= 65 else 2)
        rows = np.concatenate([np.arange(pr["obs_offsets"][i], pr["obs_offsets"][i + 1]) for i in keep])
        off = np.concatenate([[0], np.cumsum(n[keep])]).astype(np.int32)
        centre = got["kf_inv_pose7_out"][:, 4:7]
        best, normals, mn, mx = pkg.capi.map_points_refresh(off, rng.integers(0, 256, (len(rows), 32)).astype(np.uint8), centre[pr["obs_kf"][rows]],
                                                            got["point_pos_out"][keep], centre[pr["point_ref_kf"][keep]],
                                                            pr["point_ref_level_scale"][keep], pr["last_level_scale"])
        assert (best >= 0).all()
        K.assert_equal(dict(normal=got["point_normal"][keep], mn=got["point_min_distance"][keep], mx=got["point_max_distance"][keep]),
                       dict(normal=normals, mn=mn, mx=mx), "against tc2li_map_points_refresh")


def test_device_two_callers_at_once(pkg):
    """Two threads, four calls each on batches of their own: each gets its own results."""
    import two_callers
    for call, tiny in ((rot, K.tiny_rot_problems(16)), (gba, K.tiny_gba_problems(16))):
        batches = [[[tiny[8 * t + (2 * s + i) % 8] for i in range(4)] for s in range(4)] for t in (0, 1)]
        want = [[call(pkg, b, host=True) for b in side] for side in batches]
        got = two_callers.run(lambda b: call(pkg, b, host=False), batches[0], batches[1])
        for t in (0, 1):
            for c, (g, w) in enumerate(zip(got[t], want[t])):
                assert len(g) == len(w) == 4
                for i in range(4):
                    K.assert_equal(g[i], w[i], "thread %d, call %d, problem %d" % (t, c, i))
