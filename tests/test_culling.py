"""CPU tests of local mapping's culling stages: tc2li_host_keyframe_culling_batch and tc2li_host_map_point_culling_batch against the
restatement tests/culling_ref.py, on generated graphs where culls cascade and on hand-made graphs, one per rule.  Every output is an
integer, so the criterion is equality.  No GPU needed."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import culling_cases as K
import culling_ref as ref


@functools.lru_cache(maxsize=None)
def family():
    problems = K.family()
    return problems, [ref.keyframe_culling(p) for p in problems]


def _host(pkg, problems):
    return pkg.keyframe_culling_batch(problems, host=True)


def _one(pkg, pr, host=True):
    got = pkg.keyframe_culling_batch([pr], host=host)[0]
    K.assert_equal(got, ref.keyframe_culling(pr))
    return got


# ---- generated graphs ----------------------------------------------------------------------------------------------------------------
def test_host_equals_restatement_on_generated_problems(pkg):
    problems, want = family()
    assert len(problems) >= 24
    assert {int(p["inertial"]) for p in problems} == {0, 1} and min(len(p["kf_flags"]) for p in problems) == 5 and max(len(p["kf_flags"]) for p in problems) == 130
    batch = _host(pkg, problems)
    for i, (g, w) in enumerate(zip(batch, want)):
        K.assert_equal(g, w, "problem %d in the batch" % i)
    for i, p in enumerate(problems):
        K.assert_equal(_host(pkg, [p])[0], batch[i], "problem %d alone" % i)
    # the events the set is there for
    flips = sum(int((w["verdict"] != ref.keyframe_culling(p, effects=False)["verdict"]).sum()) for p, w in zip(problems, want))
    turned_bad = sum(int(w["point_bad_after"].sum()) - int(p["point_bad"].sum()) for p, w in zip(problems, want))
    print("culls per problem %s, %d verdicts depend on the order, %d points turned bad" % ([w["culled"] for w in want], flips, turned_bad))
    assert max(w["culled"] for w in want) >= 3
    assert flips >= 10
    assert turned_bad >= 1
    assert any((w["verdict"] == ref.NOT_VISITED).any() for w in want)
    assert any(w["n_visited"] > 100 for w in want)                                   # count > 100
    assert any(((w["verdict"] >= 0) & (w["verdict"] & ref.MERGED > 0)).any() for w in want)
    # the norm of :1044 stays clear of its threshold, where the summation order would decide
    assert all(abs(n - 0.02) >= 1e-4 for w in want for n in w["norms"])


def test_golden(pkg, golden_dir):
    """The restatement itself against drift, and the host entry against the same file."""
    z = np.load(os.path.join(golden_dir, "culling_a.npz"))
    n = int(z["n_problems"])
    assert n >= 3
    for i in range(n):
        pr = {k[len("p%d_in_" % i):]: z[k] for k in z.files if k.startswith("p%d_in_" % i)}
        pr = {k: (int(v) if v.ndim == 0 else v) for k, v in pr.items()}
        want = {k: z["p%d_out_%s" % (i, k)] for k in K.OUTPUTS}
        K.assert_equal(ref.keyframe_culling(pr), want, "restatement, golden problem %d" % i)
        K.assert_equal(_host(pkg, [pr])[0], want, "host entry, golden problem %d" % i)
    pt = {k[len("mp_in_"):]: z[k] for k in z.files if k.startswith("mp_in_")}
    assert np.array_equal(ref.map_point_culling(pt), z["mp_out_action"])
    assert np.array_equal(pkg.map_point_culling_batch(pt, host=True), z["mp_out_action"])


# ---- hand-made graphs, one per rule ------------------------------------------------------------------------------------------------------
def test_init_and_bad_keyframes_are_skipped(pkg):
    kfs, points = K.star(10, 10)
    kfs[0]["flags"] = 2
    got = _one(pkg, K.hand(kfs, points, [0]))
    assert got["verdict"].tolist() == [ref.SKIPPED] and got["n_visited"] == 1
    kfs[0]["flags"] = 1
    assert _one(pkg, K.hand(kfs, points, [0]))["verdict"].tolist() == [ref.SKIPPED]
    kfs[0]["flags"] = 0
    assert _one(pkg, K.hand(kfs, points, [0]))["verdict"].tolist() == [3]


def test_no_map_points_is_not_redundant(pkg):
    kfs, points = K.star(4, 4)
    kfs.append(dict(slots=[(-1, 5.0, 0), (-1, -1.0, 0)]))
    got = _one(pkg, K.hand(kfs, points, [6]))
    assert (got["verdict"][0], got["n_mps"][0], got["n_redundant"][0]) == (0, 0, 0)     # 0 > 0.9f * 0 is false
    kfs.append(dict(slots=[]))
    assert _one(pkg, K.hand(kfs, points, [7, 6]))["verdict"].tolist() == [0, 0]


def test_depth_gates(pkg):
    kfs, points = K.star(4, 4)
    kfs[0]["slots"] = [(0, 40.0, 2), (1, 40.001, 2), (2, -0.001, 2), (3, 0.0, 2)]        # at th_depth, beyond, below zero, zero
    got = _one(pkg, K.hand(kfs, points, [0]))
    assert (got["n_mps"][0], got["n_redundant"][0], got["verdict"][0]) == (2, 2, 3)
    kfs[0]["th_depth"] = 35.0
    got = _one(pkg, K.hand(kfs, points, [0]))
    assert (got["n_mps"][0], got["n_redundant"][0]) == (1, 1)


def test_observations_three_against_four(pkg):
    """Observations() is nObs: a mono observation counts once, a stereo one twice (MapPoint.cc:171-174), and :977 asks for more than 3."""
    def graph(weights):
        kfs = [dict(slots=[(0, 10.0, 2)]) for _ in range(5)]
        return kfs, [dict(obs=[(k, 2, w) for k, w in enumerate(weights)])]
    # five mono observers, nObs forced to 3: the gate of :977 closes although four other keyframes see the point
    kfs, points = graph([1, 1, 1, 1, 1]); points[0]["nobs"] = 3
    got = _one(pkg, K.hand(kfs, points, [0]))
    assert (got["n_mps"][0], got["n_redundant"][0], got["verdict"][0]) == (1, 0, 0)
    points[0]["nobs"] = 4
    got = _one(pkg, K.hand(kfs, points, [0]))
    assert (got["n_mps"][0], got["n_redundant"][0], got["verdict"][0]) == (1, 1, 3)
    # one stereo and two mono observers: nObs = 4 passes :977, but only two OTHER keyframes see the point
    kfs, points = graph([2, 1, 1])
    got = _one(pkg, K.hand(kfs[:3], points, [0]))
    assert (got["n_mps"][0], got["n_redundant"][0]) == (1, 0)
    # erasing a stereo observer takes 2, a mono observer 1
    kfs, points = graph([2, 1, 1, 1, 1])
    got = _one(pkg, K.hand(kfs, points, [0, 1]))
    assert got["verdict"].tolist() == [3, 0] and got["point_nobs_after"].tolist() == [4] and got["point_bad_after"].tolist() == [0]
    got = _one(pkg, K.hand(kfs, points, [1, 0]))
    assert got["verdict"].tolist() == [3, 0] and got["point_nobs_after"].tolist() == [5]


def test_octave_gate(pkg):
    def graph(other_octave):
        kfs = [dict(slots=[(0, 10.0, 2)])] + [dict(slots=[(0, 10.0, other_octave)]) for _ in range(4)]
        return kfs, [dict(obs=[(0, 2, 2)] + [(k, other_octave, 2) for k in range(1, 5)])]
    got = _one(pkg, K.hand(*graph(3), [0]))                                             # own octave + 1: counted
    assert (got["n_redundant"][0], got["verdict"][0]) == (1, 3)
    got = _one(pkg, K.hand(*graph(4), [0]))                                             # own octave + 2: not
    assert (got["n_redundant"][0], got["verdict"][0]) == (0, 0)
    # three at + 1 and one at + 2: three is not more than 3
    kfs, points = graph(3)
    points[0]["obs"][4] = (4, 4, 2)
    assert _one(pkg, K.hand(kfs, points, [0]))["n_redundant"][0] == 0


def test_threshold_edges(pkg):
    for inertial, n_red, want in ((0, 9, 0), (0, 10, 1), (1, 5, 0), (1, 6, 1)):
        kfs, points = K.star(10, n_red)
        got = _one(pkg, K.hand(kfs, points, [0], inertial=inertial, keyframes_in_map=21))
        assert (got["n_mps"][0], got["n_redundant"][0], got["verdict"][0] & 1) == (10, n_red, want), (inertial, n_red)


def test_point_in_two_slots_of_one_keyframe(pkg):
    kfs, points = K.star(6, 6)
    kfs[0]["slots"] += [(0, 12.0, 2), (0, 50.0, 2)]                                     # point 0 three times, once beyond th_depth
    got = _one(pkg, K.hand(kfs, points, [0]))
    assert (got["n_mps"][0], got["n_redundant"][0], got["verdict"][0]) == (7, 7, 3)     # every slot counts
    assert got["point_nobs_after"].tolist() == [8] * 6                                  # the observation goes once


def test_not_erase_without_imu(pkg):
    kfs, points = K.star(10, 10, flags=4)
    got = _one(pkg, K.hand(kfs, points, [0]))
    assert got["verdict"][0] == ref.REDUNDANT | ref.SET_BAD | ref.DEFERRED
    assert got["point_nobs_after"].tolist() == [10] * 10 and not got["point_bad_after"].any()
    # keyframe 0 is still there: listed again it is decided again, and keyframe 5 still counts it among the observers of its points
    kfs[5]["slots"] = [(p, 10.0, 2) for p in range(10)]
    for p in points:
        p["obs"] = [o for o in p["obs"] if o[0] != 4] + [(5, 2, 2)]                     # observers 0, 1, 2, 3 and 5
    got = _one(pkg, K.hand(kfs, points, [0, 0, 5]))
    assert got["verdict"].tolist() == [11, 11, 3]
    kfs[0]["flags"] = 0
    assert _one(pkg, K.hand(kfs, points, [0, 0, 5]))["verdict"].tolist() == [3, ref.SKIPPED, 0]


def _inertial_star(**scalars):
    kfs, points = K.star(10, 10, n_kf=24)
    kfs = K.chain(kfs, 0.1)
    kw = dict(inertial=1, keyframes_in_map=30, current_id=1000, last_id=0)
    kw.update(scalars)
    return kfs, points, kw


def test_not_erase_with_imu(pkg):
    """mbNotErase: SetBadFlag erases nothing, but MergePrevious and the relink of :1037-1041 come before it and have happened."""
    kfs, points, kw = _inertial_star(inertial_ba2=1)
    for i, k in enumerate(kfs):
        k["time"] = 0.2 * i                                                             # t = 0.4 for every keyframe of the chain
    kfs[2]["flags"] = 4
    pr = K.hand(kfs, points, [2, 1], **kw)
    got = _one(pkg, pr)
    # keyframe 1 lies between 0 and 3 now: t = 0.6, no merge; between 0 and 2 it would have been merged
    assert got["verdict"].tolist() == [ref.REDUNDANT | ref.SET_BAD | ref.MERGED | ref.DEFERRED, ref.REDUNDANT]
    assert got["point_nobs_after"].tolist() == pr["point_nobs"].tolist() and not got["point_bad_after"].any()
    # keyframe 2 has lost its own links: listed again it falls through :1031
    assert _one(pkg, K.hand(kfs, points, [2, 2], **kw))["verdict"].tolist() == [15, 1]


def test_inertial_gates(pkg):
    kfs, points, kw = _inertial_star()
    kfs[0].update(prev=22, next=23, id=50)                                              # t = 0.1 between keyframes 22 and 23
    # :1025 KeyFramesInMap <= 21
    assert _one(pkg, K.hand(kfs, points, [0], **dict(kw, keyframes_in_map=21)))["verdict"].tolist() == [1]
    assert _one(pkg, K.hand(kfs, points, [0], **dict(kw, keyframes_in_map=22)))["verdict"].tolist() == [7]
    # :1028 mnId > current - 2, unsigned
    assert _one(pkg, K.hand(kfs, points, [0], **dict(kw, current_id=51)))["verdict"].tolist() == [1]
    assert _one(pkg, K.hand(kfs, points, [0], **dict(kw, current_id=52)))["verdict"].tolist() == [7]
    assert _one(pkg, K.hand(kfs, points, [0], **dict(kw, current_id=1)))["verdict"].tolist() == [7]     # 1 - 2 wraps to 2^64 - 1
    assert _one(pkg, K.hand(kfs, points, [0], **dict(kw, current_id=0)))["verdict"].tolist() == [7]
    # :1031 a missing link
    for miss in ("prev", "next"):
        k2 = [dict(k) for k in kfs]
        k2[0][miss] = -1
        assert _one(pkg, K.hand(k2, points, [0], **kw))["verdict"].tolist() == [1]
    # :1035 first condition: initialised, older than last_ID, t < 3
    k2 = [dict(k) for k in kfs]
    k2[23]["time"] = k2[22]["time"] + 2.9
    far = dict(kw, inertial_ba2=1)
    assert _one(pkg, K.hand(k2, points, [0], **dict(far, imu_initialized=1, last_id=51)))["verdict"].tolist() == [7]
    assert _one(pkg, K.hand(k2, points, [0], **dict(far, imu_initialized=1, last_id=50)))["verdict"].tolist() == [1]
    assert _one(pkg, K.hand(k2, points, [0], **dict(far, imu_initialized=0, last_id=51)))["verdict"].tolist() == [1]
    k2[23]["time"] = k2[22]["time"] + 3.0
    assert _one(pkg, K.hand(k2, points, [0], **dict(far, imu_initialized=1, last_id=51)))["verdict"].tolist() == [1]
    # :1035 second condition: t < 0.5
    k2[23]["time"] = k2[22]["time"] + 0.499
    assert _one(pkg, K.hand(k2, points, [0], **far))["verdict"].tolist() == [7]
    k2[23]["time"] = k2[22]["time"] + 0.5
    assert _one(pkg, K.hand(k2, points, [0], **far))["verdict"].tolist() == [1]
    # :1044 no second inertial BA yet, the keyframe has barely moved from its predecessor, t < 3
    k2[23]["time"] = k2[22]["time"] + 2.0
    k2[0]["pos"], k2[22]["pos"] = (1.0, 2.0, 3.0), (1.01, 2.01, 3.01)                   # 0.0173
    assert _one(pkg, K.hand(k2, points, [0], **kw))["verdict"].tolist() == [7]
    assert _one(pkg, K.hand(k2, points, [0], **dict(kw, inertial_ba2=1)))["verdict"].tolist() == [1]
    k2[22]["pos"] = (1.012, 2.012, 3.012)                                               # 0.0208
    assert _one(pkg, K.hand(k2, points, [0], **kw))["verdict"].tolist() == [1]
    k2[22]["pos"] = (1.01, 2.01, 3.01)
    k2[23]["time"] = k2[22]["time"] + 3.5
    assert _one(pkg, K.hand(k2, points, [0], **kw))["verdict"].tolist() == [1]


def test_keyframes_in_map_falls_to_21_within_the_call(pkg):
    kfs, points, kw = _inertial_star(keyframes_in_map=23)
    for p in points:
        p["obs"] += [(5, 2, 2), (6, 2, 2)]                                              # keyframes 1-4 are redundant as well
    got = _one(pkg, K.hand(kfs, points, [1, 2, 3], **kw))
    assert got["verdict"].tolist() == [7, 7, 1]                                         # 23 -> 22 -> 21: the third meets :1025


def test_relink_changes_t_for_a_later_keyframe(pkg):
    kfs, points, kw = _inertial_star(inertial_ba2=1)
    for p in points:
        p["obs"] += [(5, 2, 2), (6, 2, 2), (7, 2, 2)]
    for i, k in enumerate(kfs):
        k["time"] = 0.2 * i                                                             # t = 0.4 for every keyframe of the chain
    got = _one(pkg, K.hand(kfs, points, [2, 1], **kw))
    assert got["verdict"].tolist() == [7, 1]                                            # 1 now lies between 0 and 3: t = 0.6
    assert ref.keyframe_culling(K.hand(kfs, points, [2, 1], **kw), effects=False)["verdict"].tolist() == [7, 7]
    assert _one(pkg, K.hand(kfs, points, [1, 2], **kw))["verdict"].tolist() == [7, 1]


def _many(n_local, **scalars):
    """n_local keyframes none of which is redundant, plus what K.star gives"""
    kfs, points = K.star(10, 10, n_kf=6 + n_local)
    return kfs, points, list(range(6, 6 + n_local))


def test_abort_ba_and_continue_on_the_21st_keyframe(pkg):
    kfs, points, local = _many(30)
    got = _one(pkg, K.hand(kfs, points, local, abort_ba=1))
    assert got["n_visited"] == 21 and got["verdict"].tolist() == [0] * 21 + [ref.NOT_VISITED] * 9
    assert _one(pkg, K.hand(kfs, points, local))["n_visited"] == 30
    # the 21st is skipped (:955): its continue jumps over :1060 and the loop goes on to the 22nd
    kfs[local[20]]["flags"] = 1
    got = _one(pkg, K.hand(kfs, points, local, abort_ba=1))
    assert got["n_visited"] == 22 and got["verdict"][20] == ref.SKIPPED and got["verdict"][21] == 0 and got["verdict"][22] == ref.NOT_VISITED
    # the same through the inertial continue of :1025: keyframe 0 is redundant and listed 21st
    kfs[local[20]]["flags"] = 0
    local2 = local[:20] + [0] + local[20:]
    got = _one(pkg, K.hand(kfs, points, local2, abort_ba=1, inertial=1, keyframes_in_map=21))
    assert got["n_visited"] == 22 and got["verdict"][20] == 1
    got = _one(pkg, K.hand(kfs, points, local2, abort_ba=1, inertial=0))
    assert got["n_visited"] == 21 and got["verdict"][20] == 3


def test_count_above_100(pkg):
    kfs, points, local = _many(120)
    got = _one(pkg, K.hand(kfs, points, local))
    assert got["n_visited"] == 101 and (got["verdict"][:101] == 0).all() and (got["verdict"][101:] == ref.NOT_VISITED).all()
    kfs[local[100]]["flags"] = 2                                                        # the 101st continues: the 102nd is decided too
    assert _one(pkg, K.hand(kfs, points, local))["n_visited"] == 102


def test_erasure_turns_points_bad_and_later_keyframes_see_it(pkg):
    """Three mono observers and one stereo: culling the stereo keyframe leaves nObs = 3, culling a mono one then 2: bad (MapPoint.cc:203)."""
    kfs, points = K.star(10, 10)
    kfs.append(dict(slots=[(10, 5.0, 2)]))
    points.append(dict(obs=[(0, 2, 2), (1, 2, 1), (2, 2, 1), (6, 2, 1)]))
    kfs[0]["slots"].append((10, 5.0, 2)); kfs[1]["slots"].append((10, 5.0, 2)); kfs[2]["slots"].append((10, 5.0, 2))
    got = _one(pkg, K.hand(kfs, points, [0, 6]))
    assert got["verdict"].tolist() == [3, 0] and got["point_nobs_after"][10] == 3 and got["n_mps"][1] == 1
    for p in points[:10]:
        p["obs"] += [(5, 2, 2)]
    got = _one(pkg, K.hand(kfs, points, [0, 1, 6]))
    assert got["verdict"].tolist() == [3, 3, 0] and got["point_nobs_after"][10] == 2 and got["point_bad_after"][10] == 1 and got["n_mps"][2] == 0


# ---- MapPointCulling ---------------------------------------------------------------------------------------------------------------------
def test_map_point_culling_random(pkg):
    for th_obs in (2, 3):
        pt = K.random_points(3 + th_obs, 20000)
        want = ref.map_point_culling(pt, th_obs)
        assert set(want.tolist()) == {0, 1, 2, 3, 4}
        assert np.array_equal(pkg.map_point_culling_batch(pt, th_obs, host=True), want)


def test_map_point_culling_rule_order(pkg):
    rows = [  # bad, found, visible, first, obs, current -> action
        (1, 0, 10, 0, 0, 10, 1),          # bad first, whatever else holds
        (0, 2, 10, 0, 0, 10, 2),          # ratio before observations and age
        (0, 5, 10, 8, 3, 10, 3),          # two keyframes old, three observations
        (0, 5, 10, 8, 4, 10, 0),          # ... four: stays
        (0, 5, 10, 9, 3, 10, 0),          # one keyframe old
        (0, 5, 10, 7, 3, 10, 3),          # observations before age
        (0, 5, 10, 7, 4, 10, 4),          # three keyframes old
        (0, 0, 0, 9, 9, 10, 0),           # 0 / 0 is NaN: not below 0.25
        (0, 3, 0, 9, 9, 10, 0),           # 3 / 0 is inf
        (0, 1, 4, 9, 9, 10, 0),           # exactly 0.25
        (0, 5, 10, 10, 0, (1 << 32) + 12, 3),   # the ids go through int: 12 - 10
        (0, 5, 10, 12, 0, 10, 0),         # negative age
    ]
    pt = {k: np.array([r[j] for r in rows]) for j, k in enumerate(("bad", "n_found", "n_visible", "first_kf_id", "n_obs", "current_kf_id"))}
    want = np.array([r[6] for r in rows], np.uint8)
    assert np.array_equal(ref.map_point_culling(pt, 3), want)
    assert np.array_equal(pkg.map_point_culling_batch(pt, 3, host=True), want)
    got2 = pkg.map_point_culling_batch(pt, 2, host=True)
    assert np.array_equal(got2, ref.map_point_culling(pt, 2)) and got2[2] == 0 and got2[5] == 4     # three observations are enough for th_obs = 2
    assert len(pkg.map_point_culling_batch({k: v[:0] for k, v in pt.items()}, host=True)) == 0


# ---- errors, devices, resources ------------------------------------------------------------------------------------------------------
def test_invalid_arguments(pkg):
    kfs, points = K.star(4, 4)
    good = K.hand(kfs, points, [0, 1])
    assert len(_host(pkg, [good])) == 1
    for key, where, value, word in (("local", 1, 6, "local"), ("local", 0, -1, "local"), ("slot_point", 2, 4, "slot_point"), ("slot_point", 2, -2, "slot_point"),
                                    ("obs_kf", 3, 6, "obs_kf"), ("obs_kf", 3, -1, "obs_kf"), ("kf_prev", 1, 6, "kf_prev"), ("kf_next", 1, -2, "kf_prev"),
                                    ("slot_offsets", 0, 1, "slot_offsets"), ("slot_offsets", 2, 0, "slot_offsets"), ("obs_offsets", 1, 99, "obs_offsets")):
        bad = dict(good)
        bad[key] = good[key].copy()
        bad[key][where] = value
        for host in (True, False):
            with pytest.raises(pkg.Tc2liError, match=word) as e:
                pkg.keyframe_culling_batch([good, bad], host=host)
            assert e.value.code == -2 and "problem 1" in str(e.value)
    C = pkg.capi.C
    arr, outs, keep = pkg.capi.pack_culling_problems([good])
    f = pkg.lib().tc2li_host_keyframe_culling_batch
    f.argtypes = [C.c_void_p, C.c_int]
    assert f(C.addressof(arr), -1) == -2 and f(None, 1) == -2
    arr[0].verdict = None
    assert f(C.addressof(arr), 1) == -2
    arr, outs, keep = pkg.capi.pack_culling_problems([good])
    arr[0].n_points = -1
    assert f(C.addressof(arr), 1) == -2
    g = pkg.lib().tc2li_host_map_point_culling_batch
    g.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    assert g(None, None, None, None, None, None, 3, 3, None) == -2 and g(None, None, None, None, None, None, -1, 3, None) == -2
    assert b"tc2li_host_map_point_culling_batch" in pkg.lib().tc2li_last_error()


def test_device_entries_without_a_device_are_an_error(pkg):
    """No quiet fall-back to the host walk: without a GPU the device entries fail; with one they answer."""
    kfs, points = K.star(4, 4)
    pr = K.hand(kfs, points, [0])
    pt = K.random_points(0, 10)
    if pkg.device_count() > 0:
        assert pkg.keyframe_culling_batch([pr])[0]["verdict"].tolist() == [3]
        assert len(pkg.map_point_culling_batch(pt)) == 10
    else:
        with pytest.raises(Exception, match="no HIP device"):
            pkg.keyframe_culling_batch([pr])
        with pytest.raises(Exception, match="no HIP device"):
            pkg.map_point_culling_batch(pt)


def test_new_kernels_use_no_scratch(tmp_path):
    """The resource report of the compiler for csrc/culling_kernels.hip: three kernels, no private memory in any of them."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tc2li-slam_amd", "csrc", "culling_kernels.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "culling_kernels.o")],
                         capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    assert len(names) == 3 and all(any(k in n for n in names) for k in ("k_cull_count", "k_cull_resolve", "k_mp_cull")), names
    assert scratch == [0, 0, 0], list(zip(names, scratch))
