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
