"""CPU tests of the inertial local-BA window: tc2li_host_inertial_window_batch and tc2li_inertial_window_outliers against the restatement
tests/inertial_window_ref.py, on generated graphs and on hand-made graphs, one per rule, whose expected lists are written out here so that
the restatement cannot drift.  Every output is an integer or a float widened to double, so the criterion is equality.  No GPU needed."""
import functools

import numpy as np
import pytest

import inertial_window_cases as K
import inertial_window_ref as ref

SENTINEL = -77
INVALID, CAPACITY = -2, -5


@functools.lru_cache(maxsize=None)
def family(lds_keyframes, lds_points):
    problems = K.family(lds_keyframes, lds_points)
    return problems, [ref.gather(p, K.WORLD, K.SIGMA) for p in problems]


def family_of(pkg):
    lim = pkg.inertial_window_limits()
    return family(lim["lds_keyframes"], lim["lds_points"])


def host_run(pkg):
    """problems -> results through the host entry; the GPU tests pass the device entry in its place"""
    return lambda problems, **kw: pkg.inertial_window_batch(problems, K.SIGMA, views=K.WORLD, **kw)


def _one(run, pr):
    got = run([pr])[0]
    K.assert_equal(got, ref.gather(pr, K.WORLD, K.SIGMA))
    return got


def _edges(got):
    return [tuple(e) for e in got["edges"].tolist()]


def _chain(n, **kw):
    """n keyframes, row i the predecessor of row i - 1, ids descending (row 0 is the current keyframe and has the highest), slot = row"""
    return [dict(dict(slot=i % 12, id=100 - i, prev=i + 1 if i + 1 < n else -1), **kw) for i in range(n)]


# ---- generated graphs ----------------------------------------------------------------------------------------------------------------
def test_family_reaches_every_branch(pkg):
    """The restatement alone: the generated graphs contain what the device tests count on."""
    lim = pkg.inertial_window_limits()
    problems, want = family_of(pkg)
    assert len(problems) >= 40
    small = [p for p in problems if 5 <= len(p["kf_slot"]) <= 40 and 20 <= len(p["point_flags"]) <= 400]
    assert len(small) == len(problems) - 4                                             # all but the graphs beyond the limits and the one for the cap
    beyond = {(len(p["kf_slot"]) > lim["lds_keyframes"], len(p["point_flags"]) > lim["lds_points"]) for p in problems}
    assert len(beyond) == 4                                                            # marks and keys: each in LDS and in global memory
    ok = [w for w in want if w["status"] == ref.OK]
    assert any(w["status"] == ref.EMPTY for w in want) and len(ok) >= 35
    assert any(w["popped"] for w in ok) and any(not w["popped"] for w in ok)          # both arms of :543-554
    assert any(w["n_bad_marked"] > 0 for w in ok)                                     # a bad observer marked at :597
    assert any(w["capped"] and w["n_fixed_kf"] == 200 for w in ok) and any(1 < w["n_fixed_kf"] < 200 for w in ok)   # :605
    capped = [(p, w) for p, w in zip(problems, want) if w["capped"]]
    assert all(len(np.unique(p["obs_kf"])) > 230 for p, w in capped)                  # the cap left candidates behind
    assert any(w["n_lidar"] == 6 for w in ok) and any(w["n_lidar"] == 0 and w["n_opt_kf"] > 5 for w in ok)       # LiDAR on, and off by the flag
    assert any(p["with_lidar"] and w["status"] == ref.OK and w["n_opt_kf"] <= 5 for p, w in zip(problems, want))  # off by the size
    assert {1, 10, 25} <= {w["n_opt_kf"] for w in ok}
    assert any(len(w["link4"]) < w["n_opt_kf"] for w in ok) and any(len(w["link4"]) == w["n_opt_kf"] > 1 for w in ok)
    assert any(w["link4"][:, 2].all() and len(w["link4"]) > 1 for w in ok) and any(not w["link4"][:, 2].all() for w in ok if len(w["link4"]))
    assert any(w["n_points_without_edge"] > 0 for w in ok) and any(w["n_vertices_under_3_edges"] > 0 for w in ok)
    assert any((e["u_right"] < 0).any() and (e["u_right"] >= 0).any() for e in (w["edges"] for w in ok))         # mono and stereo
    assert any((p["point_flags"][w["point_row"]] & 2).any() for p, w in zip(problems, want))                     # a point of another map listed
    assert any(len(w["point_row"]) > 256 for w in ok) and any((p["point_flags"] & 1).any() for p in problems)
    assert any((np.diff(w["kf_row"]) < 0).any() and (np.diff(w["kf_row"]) > 0).any() for w in ok)                 # id order is not row order
    assert any(len(np.unique(p["slot_point"][p["slot_point"] >= 0])) < (p["slot_point"] >= 0).sum() for p in problems)   # duplicate holders


def test_host_equals_restatement_on_generated_problems(pkg):
    problems, want = family_of(pkg)
    run = host_run(pkg)
    batch = run(problems)
    for i, (g, w) in enumerate(zip(batch, want)):
        K.assert_equal(g, w, "problem %d in the batch" % i)
    for i in (0, 7, 30, 38, 40, 41, 42, 43):
        K.assert_equal(run([problems[i]])[0], batch[i], "problem %d alone" % i)


# ---- hand-made graphs, one per rule --------------------------------------------------------------------------------------------------
def rule_nd_cuts_the_chain(run):
    """:493-519 -- Nd = min(KeyFramesInMap() - 2, large ? 25 : 10); the current keyframe is taken even with Nd <= 1"""
    kfs = _chain(5)
    for i, k in enumerate(kfs):
        k["holds"] = [i]
    points = [dict(obs={i: 0}) for i in range(5)]
    got = _one(run, K.hand(kfs, points, 0, in_map=5))                                  # Nd = 3
    assert (got["status"], got["n_opt_kf"], got["n_fixed_kf"]) == (0, 3, 1)
    assert got["kf_row"].tolist() == [3, 2, 1, 0] and got["fixed"].tolist() == [1, 0, 0, 0] and got["point_row"].tolist() == [0, 1, 2]
    assert got["kf33"].tolist() == [[r + 0.5] * 33 for r in (3, 2, 1, 0)] and got["points3"].tolist() == [[0, 0.5, 2], [1, 0.5, 2], [2, 0.5, 2]]
    assert _edges(got) == [K.edge(0, 3, 0, 0), K.edge(1, 2, 1, 0), K.edge(2, 1, 2, 0)]
    assert got["link4"].tolist() == [[2, 3, 0, 1.0], [1, 2, 0, 1.0], [0, 1, 1, 1e-2]] and got["link_kf2_row"].tolist() == [0, 1, 2]
    for in_map in (0, 2, 3):                                                           # Nd = -2, 0, 1
        got = _one(run, K.hand(kfs, points, 0, in_map=in_map))
        assert got["kf_row"].tolist() == [1, 0] and got["fixed"].tolist() == [1, 0] and got["point_row"].tolist() == [0]
        assert got["link4"].tolist() == [[0, 1, 1, 1e-2]] and got["n_opt_kf"] == 1
    long = _chain(27)
    got = _one(run, K.hand(long, [], 0, in_map=40, large=True))
    assert got["n_opt_kf"] == 25 and got["kf_row"].tolist() == list(range(25, -1, -1)) and got["fixed"].tolist() == [1] + [0] * 25
    got = _one(run, K.hand(long, [], 0, in_map=40, large=False))
    assert got["n_opt_kf"] == 10 and got["kf_row"].tolist() == list(range(10, -1, -1))
    got = _one(run, K.hand(long, [], 0, in_map=20, large=True))                        # the map is the smaller bound
    assert got["n_opt_kf"] == 18


def rule_chain_ends_early_and_the_oldest_keyframe_is_popped(run):
    """:512-518, :549-553 -- its points stay listed, it is fixed, and the link to it is the robust, down-weighted one"""
    kfs = [dict(slot=0, id=30, prev=1, holds=[1]), dict(slot=1, id=20, prev=2), dict(slot=2, id=10, holds=[0])]
    points = [dict(obs={0: 2, 2: 1}), dict(obs={0: 0, 1: 1})]
    got = _one(run, K.hand(kfs, points, 0))
    assert (got["status"], got["n_opt_kf"], got["n_fixed_kf"]) == (0, 2, 1)
    assert got["kf_row"].tolist() == [2, 1, 0] and got["fixed"].tolist() == [1, 0, 0] and got["has_imu"].tolist() == [1, 1, 1]
    assert got["point_row"].tolist() == [1, 0]                                         # point 0 is held by the popped keyframe alone
    assert _edges(got) == [K.edge(0, 2, 0, 0), K.edge(0, 1, 1, 1), K.edge(1, 2, 0, 2), K.edge(1, 0, 2, 1)]
    assert got["link4"].tolist() == [[1, 2, 0, 1.0], [0, 1, 1, 1e-2]] and got["link_kf2_row"].tolist() == [0, 1]


def rule_single_keyframe_without_predecessor_is_empty(run):
    """:549-553 with a window of one: nothing is left to optimise; counts only"""
    kfs = [dict(slot=0, id=1, holds=[0]), dict(slot=1, id=2)]
    pr = K.hand(kfs, [dict(obs={0: 0, 1: 0})], 0)
    got = _one(run, pr)
    assert got["status"] == ref.EMPTY and got["n_fixed_kf"] == 1 and len(got["kf_row"]) == len(got["point_row"]) == len(got["edges"]) == 0
    out = run([pr], raw=True, fill=SENTINEL)[0]
    assert out["counts"].tolist() == [ref.EMPTY, 1, 0, 0, 0, 0, 0, 0, 0, 0]
    for k in ("kf_row", "keyframes_out", "fixed", "has_imu", "point_row", "points3_out", "link_kf2_row", "lidar_pose_index"):
        assert (out[k] == np.array(SENTINEL).astype(out[k].dtype)).all(), k
    assert (out["edges"].view(np.uint8) == SENTINEL & 0xff).all() and (out["links"].view(np.uint8) == SENTINEL & 0xff).all()


def rule_point_of_another_map_is_listed(run):
    """:532 -- isBad() alone"""
    kfs = [dict(slot=0, id=2, prev=1, holds=[0, 1, 2, -1, 0]), dict(slot=1, id=1)]
    points = [dict(obs={0: 0, 1: 0}, flags=2), dict(obs={0: 1, 1: 1}, flags=1), dict(obs={0: 2, 1: 2}, flags=3)]
    got = _one(run, K.hand(kfs, points, 0, in_map=2))
    assert got["point_row"].tolist() == [0] and _edges(got) == [K.edge(0, 1, 0, 0), K.edge(0, 0, 1, 0)]


def rule_bad_observer_is_marked_and_the_next_one_taken(run):
    """:595-602 -- row 2 is bad: marked, no vertex, no edge; the point goes on to row 3; point 1 finds row 2 marked and takes row 4"""
    kfs = [dict(slot=0, id=10, prev=1, holds=[0, 1]), dict(slot=1, id=9), dict(slot=2, id=5, flags=K.BAD | K.IMU | K.PREINT), dict(slot=3, id=6),
           dict(slot=4, id=7)]
    points = [dict(obs={0: 0, 2: 1, 3: 2, 4: 3}), dict(obs={0: 1, 2: 0, 4: 2})]
    got = _one(run, K.hand(kfs, points, 0, in_map=2))
    assert got["n_fixed_kf"] == 3 and got["kf_row"].tolist() == [3, 4, 1, 0] and got["fixed"].tolist() == [1, 1, 1, 0]
    assert _edges(got) == [K.edge(0, 3, 0, 0), K.edge(0, 0, 3, 2), K.edge(0, 1, 4, 3), K.edge(1, 3, 0, 1), K.edge(1, 1, 4, 2)]


def rule_two_points_share_two_observers(run):
    """:595-601 -- the first point takes row 2 and stops; the second finds it marked and takes row 3"""
    kfs = [dict(slot=0, id=10, prev=1, holds=[0, 1]), dict(slot=1, id=9), dict(slot=2, id=3), dict(slot=3, id=4)]
    points = [dict(obs={0: 0, 2: 0, 3: 0}), dict(obs={0: 1, 2: 1, 3: 1})]
    got = _one(run, K.hand(kfs, points, 0, in_map=2))
    assert got["n_fixed_kf"] == 3 and got["kf_row"].tolist() == [2, 3, 1, 0] and got["fixed"].tolist() == [1, 1, 1, 0]
    kfs[0]["holds"] = [0]
    got = _one(run, K.hand(kfs, points[:1], 0, in_map=2))                              # alone, the first point leaves row 3 out
    assert got["n_fixed_kf"] == 2 and got["kf_row"].tolist() == [2, 1, 0] and len(got["edges"]) == 2


def rule_point_whose_every_observer_is_marked_adds_nothing(run):
    """:591-604 falls through, and the walk goes on with the next point"""
    kfs = [dict(slot=0, id=10, prev=1, holds=[0, 1, 2]), dict(slot=1, id=9), dict(slot=2, id=3), dict(slot=3, id=4), dict(slot=4, id=2)]
    points = [dict(obs={0: 0, 2: 0}), dict(obs={0: 1, 1: 1, 2: 1}), dict(obs={0: 2, 4: 0})]
    got = _one(run, K.hand(kfs, points, 0, in_map=2))
    assert got["n_fixed_kf"] == 3 and got["kf_row"].tolist() == [4, 2, 1, 0] and got["fixed"].tolist() == [1, 1, 1, 0]


def rule_cap_of_200_fixed_keyframes(run):
    """:605 -- the keyframe of :545 counts; the walk stops after the point that brought the list to 200, mid-list"""
    kfs = [dict(slot=0, id=1000, prev=1, holds=list(range(210))), dict(slot=1, id=999)] + [dict(slot=2 + i % 10, id=i) for i in range(210)]
    points = [dict(obs={0: i % 64, 2 + i: 0}) for i in range(210)]
    got = _one(run, K.hand(kfs, points, 0, in_map=2))
    assert got["n_fixed_kf"] == 200 and len(got["point_row"]) == 210
    assert got["kf_row"].tolist() == list(range(2, 201)) + [1, 0] and got["fixed"].tolist() == [1] * 200 + [0]
    assert len(got["edges"]) == 210 + 199 and got["edges"]["pose"].max() == 200


def rule_fixed_keyframe_of_another_map_has_a_vertex_and_no_edge(run):
    """:545 and :597-600 test no map, :865 does"""
    other = K.OTHER_MAP | K.IMU | K.PREINT
    kfs = [dict(slot=0, id=10, prev=1, holds=[0]), dict(slot=1, id=9, flags=other), dict(slot=2, id=3, flags=other)]
    got = _one(run, K.hand(kfs, [dict(obs={0: 0, 1: 0, 2: 0})], 0, in_map=2))
    assert got["kf_row"].tolist() == [2, 1, 0] and got["fixed"].tolist() == [1, 1, 0] and got["n_fixed_kf"] == 2
    assert _edges(got) == [K.edge(0, 2, 0, 0)] and got["n_vertices_under_3_edges"] == 3
    kfs[1]["flags"] = K.BAD | K.IMU | K.PREINT                                         # :545 does not test isBad() either
    got = _one(run, K.hand(kfs, [dict(obs={0: 0, 1: 0, 2: 0})], 0, in_map=2))
    assert got["kf_row"].tolist() == [2, 1, 0] and _edges(got) == [K.edge(0, 2, 0, 0)] and got["link4"].tolist() == [[1, 2, 1, 1e-2]]


def rule_lidar_keyframes_by_position(run):
    """:699-727 -- N > 5: vpOptimizableKFs[0 .. 6) whatever they carry (vLiDAROptKeyFrames is never used: there is no cloud bit to read)"""
    kfs = _chain(9)
    for n in (5, 6, 7):
        got = _one(run, K.hand(kfs, [], 0, in_map=n + 2, with_lidar=True))
        assert got["n_opt_kf"] == n and got["kf_row"].tolist() == list(range(n, -1, -1))
        assert got["lidar_pose_index"].tolist() == ([] if n == 5 else [n - r for r in range(6)]) and got["n_lidar"] == (0 if n == 5 else 6)
        got = _one(run, K.hand(kfs, [], 0, in_map=n + 2, with_lidar=False))
        assert got["n_opt_kf"] == n and got["n_lidar"] == 0 and len(got["lidar_pose_index"]) == 0
    got = _one(run, K.hand(_chain(9, flags=0), [], 0, in_map=9, with_lidar=True))      # no flag of a keyframe matters
    assert got["lidar_pose_index"].tolist() == [7, 6, 5, 4, 3, 2] and len(got["link4"]) == 0 and got["has_imu"].tolist() == [0] * 8


def rule_links_need_both_imu_bits_and_the_preintegration(run):
    """:738-743, :770, :778"""
    kfs = _chain(5)                                                                    # the window is rows 0 .. 3, row 4 is popped and fixed
    kfs[1]["flags"], kfs[2]["flags"], kfs[4]["flags"] = K.IMU, K.PREINT, K.IMU
    got = _one(run, K.hand(kfs, [], 0))
    assert got["kf_row"].tolist() == [4, 3, 2, 1, 0] and got["has_imu"].tolist() == [1, 1, 0, 1, 1]
    assert got["link4"].tolist() == [[3, 4, 0, 1.0], [0, 1, 1, 1e-2]] and got["link_kf2_row"].tolist() == [0, 3]
    got = _one(run, K.hand(kfs, [], 0, rec_init=True))                                 # bRecInit makes every link robust, not down-weighted
    assert got["link4"].tolist() == [[3, 4, 1, 1.0], [0, 1, 1, 1e-2]]
    kfs[1]["flags"] = K.IMU | K.PREINT                                                 # row 1 now fails for its predecessor's bImu alone
    got = _one(run, K.hand(kfs, [], 0))
    assert got["link_kf2_row"].tolist() == [0, 3]
    kfs[2]["flags"] = K.IMU                                                            # row 2 has bImu and no preintegration: row 1 links, row 2 not
    got = _one(run, K.hand(kfs, [], 0))
    assert got["link4"].tolist() == [[3, 4, 0, 1.0], [2, 3, 0, 1.0], [0, 1, 1, 1e-2]] and got["link_kf2_row"].tolist() == [0, 1, 3]
    kfs[3]["flags"] = 0                                                                # without the last link nothing is down-weighted
    got = _one(run, K.hand(kfs, [], 0))
    assert got["link4"].tolist() == [[3, 4, 0, 1.0], [2, 3, 0, 1.0]]


def rule_equal_ids_go_by_row(run):
    kfs = [dict(slot=0, id=5, prev=1, holds=[0]), dict(slot=1, id=5), dict(slot=2, id=5), dict(slot=3, id=1)]
    got = _one(run, K.hand(kfs, [dict(obs={0: 0, 2: 0}), dict(obs={3: 0})], 0, in_map=2))
    assert got["kf_row"].tolist() == [0, 1, 2] and got["fixed"].tolist() == [0, 1, 1]  # point 1 is not held: row 3 stays out
    kfs[0]["holds"] = [0, 1]
    got = _one(run, K.hand(kfs, [dict(obs={0: 0, 2: 0}), dict(obs={0: 1, 3: 0})], 0, in_map=2))
    assert got["kf_row"].tolist() == [3, 0, 1, 2] and got["fixed"].tolist() == [1, 0, 1, 1]
    assert got["link4"].tolist() == [[2, 1, 1, 1e-2]] and got["edges"]["pose"].tolist() == [1, 3, 1, 0]


def rule_index_minus_one_makes_no_edge(run):
    """:872, :902 -- mono and stereo by u_right, inv_sigma2 the table's value"""
    mono = int(np.flatnonzero(K.WORLD[0]["u_right"] < 0)[0])
    stereo = int(np.flatnonzero(K.WORLD[0]["u_right"] >= 0)[0])
    kfs = [dict(slot=0, id=2, prev=1, holds=[0, 1, 2]), dict(slot=0, id=1)]
    points = [dict(obs={0: -1, 1: mono}), dict(obs={0: -1}), dict(obs={0: stereo, 1: -1})]
    got = _one(run, K.hand(kfs, points, 0, in_map=2))
    assert got["point_row"].tolist() == [0, 1, 2] and got["n_points_without_edge"] == 1 and got["n_vertices_under_3_edges"] == 2
    assert _edges(got) == [K.edge(0, 0, 0, mono), K.edge(2, 1, 0, stereo)]
    assert got["edges"]["u_right"].tolist() == [-1.0, float(K.WORLD[0]["u_right"][stereo])]
    assert got["edges"]["inv_sigma2"].tolist() == [float(K.SIGMA[K.WORLD[0]["keys"]["octave"][i]]) for i in (mono, stereo)]


RULES = [rule_nd_cuts_the_chain, rule_chain_ends_early_and_the_oldest_keyframe_is_popped, rule_single_keyframe_without_predecessor_is_empty,
         rule_point_of_another_map_is_listed, rule_bad_observer_is_marked_and_the_next_one_taken, rule_two_points_share_two_observers,
         rule_point_whose_every_observer_is_marked_adds_nothing, rule_cap_of_200_fixed_keyframes,
         rule_fixed_keyframe_of_another_map_has_a_vertex_and_no_edge, rule_lidar_keyframes_by_position,
         rule_links_need_both_imu_bits_and_the_preintegration, rule_equal_ids_go_by_row, rule_index_minus_one_makes_no_edge]


@pytest.mark.parametrize("rule", RULES, ids=lambda r: r.__name__)
def test_rule(pkg, rule):
    rule(host_run(pkg))


# ---- contracts -------------------------------------------------------------------------------------------------------------------------
def _base():
    kfs = [dict(slot=0, id=3, prev=1, holds=[0, 1]), dict(slot=1, id=2, prev=2, holds=[1]), dict(slot=2, id=1)]
    return K.hand(kfs, [dict(obs={0: 0, 2: 1}), dict(obs={0: 1, 1: 7, 2: -1})], 0)


def invalid_problems():
    """(what, problem, views or None for the world's): every refusal the header lists"""
    def changed(**kw):
        pr = _base()
        pr.update(kw)
        return pr
    n0, n1 = len(K.WORLD[0]["keys"]), len(K.WORLD[1]["keys"])
    high = [dict(v) if v is not None else None for v in K.WORLD]
    high[2] = dict(high[2], keys=high[2]["keys"].copy())
    high[2]["keys"]["octave"][3] = K.N_LEVELS
    return [("current out of range", changed(current=3), None), ("current negative", changed(current=-1), None),
            ("prev_kf out of range", changed(prev_kf=[1, 3, -1]), None), ("prev_kf below -1", changed(prev_kf=[1, -2, -1]), None),
            ("prev_kf of a row outside the window out of range", changed(prev_kf=[1, 2, 7], keyframes_in_map=2), None),
            ("the chain returns to the current keyframe", changed(prev_kf=[1, 0, -1]), None),
            ("a keyframe is its own predecessor", changed(prev_kf=[0, 2, -1]), None),
            ("the keyframe behind the window is in the window", changed(prev_kf=[1, 2, 0]), None),
            ("the same when Nd cuts the chain", changed(prev_kf=[1, 0, -1], keyframes_in_map=4), None),
            ("negative keyframes_in_map", changed(keyframes_in_map=-1), None),
            ("slot_offsets do not start at 0", changed(slot_offsets=[1, 2, 3, 3]), None), ("slot_offsets descend", changed(slot_offsets=[0, 2, 1, 3]), None),
            ("obs_offsets descend", changed(obs_offsets=[0, 3, 2]), None), ("slot_point below -1", changed(slot_point=[0, -2, 1]), None),
            ("slot_point beyond the points", changed(slot_point=[0, 2, 1]), None), ("obs_kf out of range", changed(obs_kf=[0, 2, 0, 1, 3]), None),
            ("obs_kf negative", changed(obs_kf=[-1, 2, 0, 1, 2]), None), ("observation row not ascending", changed(obs_kf=[2, 0, 0, 1, 2]), None),
            ("observation row with a keyframe twice", changed(obs_kf=[0, 2, 0, 1, 1]), None),
            ("obs_index below -1", changed(obs_index=[0, 1, 1, 7, -2]), None), ("obs_index beyond the slot's keypoints", changed(obs_index=[n0, 1, 1, 7, -1]), None),
            ("obs_index beyond the keypoints of a smaller slot", changed(obs_index=[0, 1, 1, n1, -1]), None),
            ("empty slot", changed(kf_slot=[0, K.EMPTY_SLOT, 2]), None), ("slot out of range", changed(kf_slot=[0, 1, K.WORLD_SLOTS]), None),
            ("slot negative", changed(kf_slot=[0, -1, 2]), None), ("negative capacity", changed(edge_capacity=-1), None),
            ("negative link capacity", changed(link_capacity=-1), None), ("octave outside the levels", _base(), high)]


def test_invalid_is_refused(pkg):
    assert pkg.inertial_window_batch([_base()], K.SIGMA, views=K.WORLD)[0]["status"] == ref.OK
    assert pkg.inertial_window_batch([dict(_base(), prev_kf=[1, 2, 0], keyframes_in_map=3)], K.SIGMA, views=K.WORLD)[0]["n_opt_kf"] == 1   # a loop behind the window is never followed
    for what, pr, views in invalid_problems():
        for batch in ([pr], [_base(), pr]):
            with pytest.raises(pkg.Tc2liError) as e:
                pkg.inertial_window_batch(batch, K.SIGMA, views=views or K.WORLD)
            assert e.value.code == INVALID, what
    with pytest.raises(pkg.Tc2liError) as e:                                           # the same slot, fewer levels in the table
        pkg.inertial_window_batch([_base()], K.SIGMA[:int(K.WORLD[2]["keys"]["octave"].max())], views=K.WORLD)
    assert e.value.code == INVALID


_CAPACITY_OF = {"kf_capacity": "kf_row", "point_capacity": "point_row", "edge_capacity": "edges", "link_capacity": "link4"}


def capacity_contract(run):
    """needed sizes reported for every problem, no list of any problem written"""
    problems = [K.make_graph(900 + i, 12, 80, chain=6, in_map=30, bad=0.05, imu=1.0, preint=1.0, with_lidar=1) for i in range(6)]
    want = [ref.gather(p, K.WORLD, K.SIGMA) for p in problems]
    assert all(w["status"] == ref.OK and len(w["edges"]) > 3 and len(w["link4"]) > 1 for w in want)
    for short, name in _CAPACITY_OF.items():
        batch = [dict(p) for p in problems]
        n = len(want[3][name])
        batch[3][short] = n - 1
        with pytest.raises(Exception) as e:
            run(batch, raw=True, fill=SENTINEL)
        assert e.value.code == CAPACITY and "problem 3" in str(e.value), short
        batch[3][short] = n                                                             # exactly enough
        for g, w in zip(run(batch), want):
            K.assert_equal(g, w, short)

    import tc2li_slam_amd.capi as capi                                                  # keep the output arrays of a refused call
    batch = [dict(p) for p in problems]
    batch[3]["link_capacity"] = 1
    seen = {}
    real = capi.pack_inertial_window_problems

    def spy(problems_, fill=0):
        arr, outs, keep = real(problems_, fill)
        seen["outs"] = outs
        return arr, outs, keep
    capi.pack_inertial_window_problems = spy
    try:
        with pytest.raises(Exception) as e:
            run(batch, raw=True, fill=SENTINEL)
    finally:
        capi.pack_inertial_window_problems = real
    assert e.value.code == CAPACITY
    for o, w in zip(seen["outs"], want):
        assert o["counts"].tolist() == [w["status"], w["n_fixed_kf"], w["n_opt_kf"], len(w["kf_row"]), len(w["point_row"]), len(w["edges"]), len(w["link4"]),
                                        w["n_lidar"], w["n_points_without_edge"], w["n_vertices_under_3_edges"]]
        for k in ("kf_row", "keyframes_out", "fixed", "has_imu", "point_row", "points3_out", "link_kf2_row", "lidar_pose_index"):
            assert (o[k] == np.array(SENTINEL).astype(o[k].dtype)).all(), k
        assert (o["edges"].view(np.uint8) == SENTINEL & 0xff).all() and (o["links"].view(np.uint8) == SENTINEL & 0xff).all()


def test_capacity(pkg):
    capacity_contract(host_run(pkg))


def test_empty_batch_and_limits(pkg):
    assert pkg.inertial_window_batch([], K.SIGMA, views=K.WORLD) == []
    lim = pkg.inertial_window_limits()
    assert lim["threads"] % 64 == 0 and lim["lds_keyframes"] >= 256 and lim["lds_points"] >= 256


# ---- the outlier rule ------------------------------------------------------------------------------------------------------------------
def _between(literal):
    """a double between the decimal literal and the float the reference compares with"""
    f = float(np.float32(literal))
    assert f != literal
    return (f + literal) / 2, f > literal


def test_outliers_by_hand(pkg):
    mid_mono, mono_up = _between(5.991)
    mid_stereo, stereo_up = _between(7.815)
    close_th = float(np.float32(1.5) * np.float32(5.991))
    e = np.zeros(12, ref.EDGE_DTYPE)
    #             0  1  2  3  4  5  6  7  8  9 10 11
    e["point"] = [0, 0, 1, 1, 2, 2, 3, 4, 4, 0, 1, 0]
    e["pose"] = [0, 1, 0, 1, 0, 1, 1, 0, 1, 2, 2, 3]
    e["u_right"] = [-1, 5, -1, 5, -1, 5, -1, -1, 5, -1, -1, 5]
    chi2 = np.array([mid_mono, mid_stereo, 7.0, 100.0, 0.1, 0.1, 50.0, close_th, 9.0, 6.0, np.nextafter(close_th, 10.0), np.nextafter(float(np.float32(7.815)), 8.0)])
    dpos = np.array([1, 1, 1, 1, 0, 0, 1, 1, 1, 1, 1, 1], np.uint8)
    bad = np.array([0, 0, 0, 1, 0], np.uint8)
    depth = np.array([30.0, 9.5, 10.0, 5.0, 9.999], np.float32)                        # points 1 and 4 are close, point 2 (10.0) is not
    got, rejected = pkg.inertial_window_outliers(e, chi2, dpos, bad, depth, 100.0, 50.0)
    want = ref.outliers(e, chi2, dpos, bad, depth, 100.0, 50.0, False)
    assert not rejected and not want[1] and np.array_equal(got, want[0])
    # mono in creation order: edge 0 only if the float threshold lies below its chi2; edge 2 (7.0, close) stays; edge 4 has a negative depth;
    # edge 6 is of a bad point; edge 7 (exactly 1.5f * 5.991f, close) stays; edge 9 (6.0, far) goes; edge 10 (just above, close) goes.
    # stereo: edge 1 only if the float threshold lies below; edge 3 goes; edge 5 has a negative depth and STAYS; edge 8 goes; edge 11 goes.
    mono = ([] if mono_up else [[0, 0]]) + [[0, 2], [2, 0], [2, 1]]
    stereo = ([] if stereo_up else [[1, 0]]) + [[1, 1], [1, 4], [3, 0]]
    assert got.tolist() == mono + stereo
    literal = [[0, 0]] * (mid_mono > 5.991) + [[1, 0]] * (mid_stereo > 7.815)          # what the decimal literals would have erased
    assert sorted(literal) != sorted([p for p in got.tolist() if p in ([0, 0], [1, 0])])
    with pytest.raises(pkg.Tc2liError) as err:
        pkg.inertial_window_outliers(e, chi2, dpos, bad, depth, 100.0, 50.0, capacity=3)
    assert err.value.code == CAPACITY
    with pytest.raises(pkg.Tc2liError) as err:
        pkg.inertial_window_outliers(e, chi2, dpos, bad[:4], depth[:4], 100.0, 50.0)
    assert err.value.code == INVALID
    assert pkg.inertial_window_outliers(e[:0], chi2[:0], dpos[:0], bad, depth, 1.0, 1.0)[0].shape == (0, 2)


def test_outliers_rejection(pkg):
    """:1028 on floats, before any erasure"""
    e = np.zeros(2, ref.EDGE_DTYPE)
    e["u_right"] = [-1, 5]
    chi2, dpos, bad, depth = np.array([100.0, 100.0]), np.ones(2, np.uint8), np.zeros(1, np.uint8), np.array([30.0], np.float32)
    just = float(np.nextafter(np.float32(2.0), np.float32(3.0)))                       # the least float above 2
    for err0, err1, large, rejected in ((1.0, 2.0, False, False), (1.0, just, False, True), (1.0, just, True, False), (1.0, 2.0 + 1e-9, False, False),
                                        (float("nan"), 1.0, False, True), (1.0, float("nan"), False, True), (float("nan"), 1.0, True, False),
                                        (1e39, 1e39, False, False), (1.0, 1e39, False, True), (50.0, 10.0, False, False)):
        got, rej = pkg.inertial_window_outliers(e, chi2, dpos, bad, depth, err0, err1, large=large)
        want, wrej = ref.outliers(e, chi2, dpos, bad, depth, err0, err1, large)
        assert rej == wrej == rejected, (err0, err1, large)
        assert np.array_equal(got, want) and len(got) == (0 if rejected else 2)


def test_outliers_equal_restatement(pkg):
    problems, want = family_of(pkg)
    rng = np.random.default_rng(3)
    n = 0
    for w in [w for w in want if w["status"] == ref.OK][:12]:
        e = w["edges"]
        chi2 = rng.choice([0.5, 5.0, 5.991, 5.9911, 6.5, 7.815, 7.8151, 8.9, 9.0, 30.0], len(e))
        dpos = (rng.random(len(e)) < 0.9).astype(np.uint8)
        bad = (rng.random(len(w["point_row"])) < 0.1).astype(np.uint8)
        depth = rng.choice([2.0, 9.99, 10.0, 40.0], len(bad)).astype(np.float32)
        got, rej = pkg.inertial_window_outliers(e, chi2, dpos, bad, depth, 10.0, 12.0)
        assert not rej and np.array_equal(got, ref.outliers(e, chi2, dpos, bad, depth, 10.0, 12.0, False)[0])
        n += len(got)
    assert n > 50


# ---- what the optimiser is handed --------------------------------------------------------------------------------------------------------
def test_gathered_window_is_the_synthetic_one(pkg, synthetic):
    """No BA entry runs without a device, so the arrays are checked for what tc2li_local_inertial_bundle_adjustment asks of them, and
    against the window the graph was made from: its keyframes, fixed, has_imu, and its links (which it lists oldest first)."""
    w = synthetic.inertial_window(seed=3, n_opt=8, n_points=300)
    views, pr, sigma = K.from_inertial_window(w)
    got = pkg.inertial_window_batch([pr], sigma, views=views)[0]
    K.assert_equal(got, ref.gather(pr, views, sigma))
    e = got["edges"]
    assert got["status"] == ref.OK and got["n_opt_kf"] == 8 and got["n_fixed_kf"] == 1 and got["n_points_without_edge"] == 0
    assert got["kf_row"].tolist() == list(range(9)) and np.array_equal(got["kf33"], w["kf33"])
    assert np.array_equal(got["fixed"], w["fixed"]) and np.array_equal(got["has_imu"], w["has_imu"])
    assert np.array_equal(got["link4"][::-1], w["link4"]) and got["link_kf2_row"].tolist() == list(range(8, 0, -1))
    assert sorted(got["point_row"].tolist()) == list(range(len(w["points"]))) and len(e) == len(w["edges"])
    mine = {(int(got["point_row"][p]), int(k)): (u, v, ur) for p, k, u, v, ur, s in e.tolist()}
    theirs = {(int(p), int(k)): (u, v, ur if ur >= 0 else -1.0) for p, k, u, v, ur, s in w["edges"].tolist()}
    assert mine == theirs
