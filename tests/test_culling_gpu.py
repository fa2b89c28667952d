"""GPU tests of local mapping's culling stages: tc2li_keyframe_culling_batch and tc2li_map_point_culling_batch against the host entries and
the restatement tests/culling_ref.py, on every problem of tests/test_culling.py, in several batch compositions.  All outputs are integers:
the criterion is equality, nothing is left out."""
import functools

import numpy as np
import pytest

import culling_cases as K
import culling_ref as ref
from test_culling import family

pytestmark = pytest.mark.gpu


def _check(pkg, problems, want, what):
    got = pkg.keyframe_culling_batch(problems)
    host = pkg.keyframe_culling_batch(problems, host=True)
    assert len(got) == len(problems)
    for i, (g, h, w) in enumerate(zip(got, host, want)):
        K.assert_equal(g, h, "%s: problem %d, device against host" % (what, i))
        K.assert_equal(g, w, "%s: problem %d, device against the restatement" % (what, i))
    return got


def test_device_one_batch(pkg):
    problems, want = family()
    _check(pkg, problems, want, "one batch")


def test_device_batches_of_one(pkg):
    problems, want = family()
    for i, (p, w) in enumerate(zip(problems, want)):
        _check(pkg, [p], [w], "problem %d alone" % i)


def test_device_shuffled_batch(pkg):
    problems, want = family()
    order = np.random.default_rng(5).permutation(len(problems))
    _check(pkg, [problems[i] for i in order], [want[i] for i in order], "shuffled")
    _check(pkg, problems[::-1], want[::-1], "reversed")


@functools.lru_cache(maxsize=None)
def _small():
    rng = np.random.default_rng(11)
    problems = []
    for i in range(100):
        k = int(rng.integers(5, 49))
        problems.append(K.make_problem(300 + i, k, 40 * k, [(5, 9), (6, 10), (7, 12)][i % 3], inertial=bool(i % 2), abort_ba=i % 7 == 0))
    problems.append(K.hand([dict(slots=[])], [], []))                                 # no local keyframes, no points
    return problems, [ref.keyframe_culling(p) for p in problems]


def test_device_batch_of_512_mixed(pkg):
    """512 problems of mixed size, K from 1 to 130, in one call."""
    pa, wa = family()
    pb, wb = _small()
    problems, want = pa + pb, wa + wb
    pick = np.random.default_rng(6).integers(0, len(problems), 512)
    pick[:len(problems)] = np.arange(len(problems))                                    # every one at least once
    got = _check(pkg, [problems[i] for i in pick], [want[i] for i in pick], "512")
    assert len(got) == 512 and sum(w["culled"] for w in wb) > 50


def test_device_hand_made_cases(pkg):
    """The rules one by one go through the same kernels: the hand-made graphs of test_culling.py with the device entry."""
    import test_culling as T
    real = pkg.keyframe_culling_batch

    class Device:
        def __getattr__(self, name):
            return getattr(pkg, name)

        @staticmethod
        def keyframe_culling_batch(problems, host=False, **kw):
            return real(problems, host=False, **kw)

    dev = Device()
    for name in ("test_init_and_bad_keyframes_are_skipped", "test_no_map_points_is_not_redundant", "test_depth_gates", "test_observations_three_against_four",
                 "test_octave_gate", "test_threshold_edges", "test_point_in_two_slots_of_one_keyframe", "test_not_erase_without_imu", "test_not_erase_with_imu",
                 "test_inertial_gates", "test_keyframes_in_map_falls_to_21_within_the_call", "test_relink_changes_t_for_a_later_keyframe",
                 "test_abort_ba_and_continue_on_the_21st_keyframe", "test_count_above_100", "test_erasure_turns_points_bad_and_later_keyframes_see_it"):
        getattr(T, name)(dev)


def test_device_empty_batch(pkg):
    assert pkg.keyframe_culling_batch([]) == []
    assert len(pkg.map_point_culling_batch({k: np.zeros(0) for k in ("bad", "n_found", "n_visible", "first_kf_id", "n_obs", "current_kf_id")})) == 0


def test_device_map_point_culling(pkg):
    for th_obs in (2, 3):
        pt = K.random_points(20 + th_obs, 100000)
        want = ref.map_point_culling(pt, th_obs)
        got = pkg.map_point_culling_batch(pt, th_obs)
        assert np.array_equal(got, pkg.map_point_culling_batch(pt, th_obs, host=True))
        assert np.array_equal(got, want) and set(want.tolist()) == {0, 1, 2, 3, 4}


# ---- the buffers kept between calls -------------------------------------------------------------------------------------------------------
def _cascade():
    """test_culling.py's graph on which two culls follow one another: the first leaves point 10 with nObs = 3, the second turns it bad, and
    the third local keyframe counts no point any more.  The device keeps that state in the zeroed prefix of its work space."""
    kfs, points = K.star(10, 10)
    kfs.append(dict(slots=[(10, 5.0, 2)]))
    points.append(dict(obs=[(0, 2, 2), (1, 2, 1), (2, 2, 1), (6, 2, 1)]))
    for k in (0, 1, 2):
        kfs[k]["slots"].append((10, 5.0, 2))
    for p in points[:10]:
        p["obs"] += [(5, 2, 2)]
    return K.hand(kfs, points, [0, 1, 6])


@functools.lru_cache(maxsize=None)
def _tiny():
    """Problems of the smallest generated size (5 keyframes), the cascade among them."""
    return [_cascade()] + [K.make_problem(700 + i, 5, 375, inertial=bool(i % 2)) for i in range(15)]


def _equals_host(pkg, problems, what):
    got = pkg.keyframe_culling_batch(problems)
    host = pkg.keyframe_culling_batch(problems, host=True)
    assert len(got) == len(host) == len(problems)
    for i, (g, h) in enumerate(zip(got, host)):
        K.assert_equal(g, h, "%s: problem %d, device against host" % (what, i))
    return got


def test_device_reuses_its_buffers_across_batch_sizes(pkg):
    """8 problems, then 1 other, then the 8 again through the same buffers: nothing of an earlier call shows in a later one."""
    tiny = _tiny()
    eight, one = tiny[:8], [tiny[8]]
    # whatever the tests before left, the calls below meet buffers a larger batch has filled, with every point bad
    _equals_host(pkg, [dict(p, point_bad=np.ones_like(p["point_bad"])) for p in tiny], "fill")
    first = _equals_host(pkg, eight, "8")
    assert first[0]["verdict"].tolist() == [3, 3, 0] and first[0]["point_bad_after"][10] == 1 and first[0]["n_mps"][2] == 0
    _equals_host(pkg, one, "1")
    again = _equals_host(pkg, eight, "8 again")
    for i, (a, b) in enumerate(zip(first, again)):
        K.assert_equal(a, b, "problem %d, first against third call" % i)
    pt = K.random_points(31, 2000)
    for n in (2000, 1, 2000):
        cut = {k: v[:n] for k, v in pt.items()}
        assert np.array_equal(pkg.map_point_culling_batch(cut), pkg.map_point_culling_batch(cut, host=True)), n


def test_device_empty_problem_inside_a_batch(pkg):
    """A problem without keyframes, points or local list between two ordinary ones: its tables are empty places in the concatenation."""
    tiny = _tiny()
    empty = K.hand([], [], [])
    for middle in (empty, K.hand([dict(slots=[])], [], [])):
        got = _equals_host(pkg, [tiny[0], middle, tiny[1]], "empty in the middle")
        assert got[1]["n_visited"] == 0 and len(got[1]["verdict"]) == 0 and len(got[1]["point_bad_after"]) == 0
    _equals_host(pkg, [empty, tiny[0], empty], "empty at both ends")
    _equals_host(pkg, [empty], "empty alone")


def test_device_two_callers_at_once(pkg):
    """Two threads, four calls each on batches of four of their own: each gets its own results."""
    import two_callers
    tiny = _tiny()
    batches = [[[tiny[8 * t + (2 * s + i) % 8] for i in range(4)] for s in range(4)] for t in (0, 1)]
    want = [[pkg.keyframe_culling_batch(b, host=True) for b in side] for side in batches]
    got = two_callers.run(pkg.keyframe_culling_batch, batches[0], batches[1])
    for t in (0, 1):
        for c, (g, w) in enumerate(zip(got[t], want[t])):
            assert len(g) == len(w) == 4
            for i in range(4):
                K.assert_equal(g[i], w[i], "thread %d, call %d, problem %d" % (t, c, i))
    pts = [[K.random_points(40 + 4 * t + c, 500 + 100 * c) for c in range(4)] for t in (0, 1)]
    got = two_callers.run(pkg.map_point_culling_batch, pts[0], pts[1])
    for t in (0, 1):
        for c in range(4):
            assert np.array_equal(got[t][c], pkg.map_point_culling_batch(pts[t][c], host=True)), (t, c)
