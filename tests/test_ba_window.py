"""CPU tests of the local-BA window: tc2li_host_ba_window_batch and tc2li_ba_window_outliers against the restatement
tests/ba_window_ref.py, on generated graphs and on hand-made graphs, one per rule, whose expected lists are written out here so that the
restatement cannot drift.  Every output is an integer or a float widened to double, so the criterion is equality.  No GPU needed."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import ba_window_cases as K
import ba_window_ref as ref

SENTINEL = -77
INVALID, CAPACITY = -2, -5


@functools.lru_cache(maxsize=None)
def family(lds_keyframes, lds_points):
    problems = K.family(lds_keyframes, lds_points)
    return problems, [ref.gather(p, K.WORLD, K.SIGMA) for p in problems]


def family_of(pkg):
    lim = pkg.ba_window_limits()
    return family(lim["lds_keyframes"], lim["lds_points"])


def host_run(pkg):
    """problems -> results through the host entry; the GPU tests pass the device entry in its place"""
    return lambda problems, **kw: pkg.ba_window_batch(problems, K.SIGMA, views=K.WORLD, **kw)


def _one(run, pr):
    got = run([pr])[0]
    K.assert_equal(got, ref.gather(pr, K.WORLD, K.SIGMA))
    return got


def _edges(got):
    return [tuple(e) for e in got["edges"].tolist()]


# ---- generated graphs ----------------------------------------------------------------------------------------------------------------
def test_family_reaches_every_branch(pkg):
    """The restatement alone: the generated graphs contain what the device tests count on."""
    lim = pkg.ba_window_limits()
    problems, want = family_of(pkg)
    assert len(problems) >= 40
    assert {lim["lds_keyframes"] + 1} <= {len(p["kf_slot"]) for p in problems} and {lim["lds_points"] + 1} <= {len(p["point_flags"]) for p in problems}
    small = [p for p in problems if 3 <= len(p["kf_slot"]) <= 12 and 20 <= len(p["point_flags"]) <= 300]
    assert len(small) == len(problems) - 3                                             # all but the three graphs beyond the limits
    beyond = {(len(p["kf_slot"]) > lim["lds_keyframes"], len(p["point_flags"]) > lim["lds_points"]) for p in problems}
    assert len(beyond) == 4                                                            # marks and keys: each in LDS and in global memory
    assert all(np.diff(p["obs_offsets"]).max() <= 6 for p in problems)
    assert any(w["status"] == ref.ABORTED for w in want) and sum(w["status"] == ref.OK for w in want) >= 30
    clouds = [sum(bool(p["kf_flags"][k] & 4) for k in w["pose_row"][w["fixed"] == 0]) for p, w in zip(problems, want)]
    assert any(w["status"] == ref.OK and w["n_lidar"] == 0 and 1 <= c <= 2 for w, c in zip(want, clouds))       # clouds, but too few
    assert any(w["n_lidar"] == 6 and c > 6 for w, c in zip(want, clouds)) and {3, 4, 5} & {w["n_lidar"] for w in want}
    assert any(w["n_points_without_edge"] > 0 for w in want) and any(w["n_fixed_without_edge"] > 0 for w in want)
    init_local = [bool(w["fixed"][np.isin(w["pose_row"], np.r_[p["current"], p["cov_kf"]])].any()) for p, w in zip(problems, want) if w["status"] == ref.OK]
    assert any(init_local) and not all(init_local)                                    # the initial keyframe is sometimes local (:85-88, :164)
    assert any((e["u_right"] < 0).any() and (e["u_right"] >= 0).any() for e in (w["edges"] for w in want))       # mono and stereo
    assert any((np.diff(p["kf_id"][w["pose_row"]]) > 0).all() and (np.diff(w["pose_row"]) < 0).any() for p, w in zip(problems, want) if len(w["pose_row"]) > 1)
    assert any(len(w["point_row"]) > 256 for w in want) and any(len(w["pose_row"]) > 256 for w in want) and any(len(p["cov_kf"]) > 256 for p in problems)
    assert any((p["kf_flags"][p["cov_kf"]] & 3).any() for p in problems) and any((p["point_flags"] & 3).any() for p in problems)
    assert any(len(np.unique(p["slot_point"][p["slot_point"] >= 0])) < (p["slot_point"] >= 0).sum() for p in problems)   # duplicate holders


def test_host_equals_restatement_on_generated_problems(pkg):
    problems, want = family_of(pkg)
    run = host_run(pkg)
    batch = run(problems)
    for i, (g, w) in enumerate(zip(batch, want)):
        K.assert_equal(g, w, "problem %d in the batch" % i)
    for i in (0, 7, 30, 39, 40, 41):
        K.assert_equal(run([problems[i]])[0], batch[i], "problem %d alone" % i)


# ---- hand-made graphs, one per rule --------------------------------------------------------------------------------------------------
def rule_current_is_local_whatever_its_flags(run):
    """:65 -- but its own observations make no edge (:281)"""
    kfs = [dict(slot=2, id=5, flags=3, holds=[0]), dict(slot=3, id=9)]
    got = _one(run, K.hand(kfs, [dict(obs={0: 1, 1: 2})], 0, []))
    assert (got["status"], got["num_opt_kf"], got["num_fixed_kf"]) == (0, 1, 1)
    assert got["pose_row"].tolist() == [0, 1] and got["fixed"].tolist() == [0, 1] and got["point_row"].tolist() == [0]
    assert got["poses7"].tolist() == [[0, 0, 0, 1, 0, 0, 0], [0, 0, 0, 1, 1, 0, 0]] and got["points3"].tolist() == [[0, 0.5, 2]]
    assert _edges(got) == [K.edge(0, 1, 3, 2)]


def rule_bad_neighbour_is_marked_local(run):
    """:73 before :74 -- a bad or other-map neighbour is neither local nor ever fixed (:115)"""
    kfs = [dict(slot=0, id=10, holds=[0]), dict(slot=1, id=11, flags=1, holds=[1]), dict(slot=2, id=12, flags=2, holds=[1]), dict(slot=3, id=13),
           dict(slot=4, id=14)]
    points = [dict(obs={0: 0, 1: 1, 2: 2, 3: 3, 4: 4}), dict(obs={1: 0, 2: 0})]
    got = _one(run, K.hand(kfs, points, 0, [1, 2, 3]))
    assert (got["num_opt_kf"], got["num_fixed_kf"]) == (2, 1)
    assert got["pose_row"].tolist() == [0, 3, 4] and got["fixed"].tolist() == [0, 0, 1]
    assert got["point_row"].tolist() == [0]                                            # the slots of rows 1 and 2 are never walked
    assert _edges(got) == [K.edge(0, 0, 0, 0), K.edge(0, 1, 3, 3), K.edge(0, 2, 4, 4)]
    # the same two rows outside the list: still no vertex (:118), and now they are the only other observers
    kfs = [dict(slot=0, id=10, holds=[0]), dict(slot=1, id=11, flags=1), dict(slot=2, id=12, flags=2)]
    got = _one(run, K.hand(kfs, [dict(obs={0: 0, 1: 1, 2: 2})], 0, [], init=10))
    assert (got["status"], got["num_fixed_kf"]) == (0, 1) and got["pose_row"].tolist() == [0] and got["fixed"].tolist() == [1]


def rule_bad_or_other_map_point_is_not_listed(run):
    """:94"""
    kfs = [dict(slot=0, id=1, holds=[0, 1, 2, 3]), dict(slot=1, id=2)]
    points = [dict(obs={0: 0, 1: 0}, flags=1), dict(obs={0: 1, 1: 1}, flags=2), dict(obs={0: 2, 1: 2}), dict(obs={0: 3, 1: 3}, flags=3)]
    got = _one(run, K.hand(kfs, points, 0, []))
    assert got["point_row"].tolist() == [2] and got["points3"].tolist() == [[2, 0.5, 2]]
    assert _edges(got) == [K.edge(0, 0, 0, 2), K.edge(0, 1, 1, 2)]


def rule_point_is_listed_once_at_its_first_occurrence(run):
    """:97-101 -- list order: the current keyframe, then cov_kf in its order; slots ascending"""
    kfs = [dict(slot=0, id=1, holds=[5, 4]), dict(slot=1, id=2, holds=[1, 0, 3]), dict(slot=2, id=3, holds=[2, -1, 0, 2]), dict(slot=3, id=4, holds=[3, 6, 2]),
           dict(slot=4, id=0)]
    points = [dict(obs={4: 0}) for _ in range(7)]
    got = _one(run, K.hand(kfs, points, 2, [3, 1]))
    assert got["point_row"].tolist() == [2, 0, 3, 6, 1] and got["num_opt_kf"] == 3      # row 0 is not in the list: points 4 and 5 stay out
    assert got["pose_row"].tolist() == [4, 1, 2, 3] and got["fixed"].tolist() == [1, 0, 0, 0]
    assert _edges(got) == [K.edge(i, 0, 4, 0) for i in range(5)]


def rule_every_observer_becomes_a_fixed_camera(run):
    """:115-119 -- whatever its index: row 2 is fixed and has no edge; a bad observer and one of another map are not (:118)"""
    kfs = [dict(slot=0, id=7, holds=[0, 1]), dict(slot=1, id=3), dict(slot=2, id=5), dict(slot=3, id=4, flags=1), dict(slot=5, id=6, flags=2)]
    points = [dict(obs={0: 0, 1: 1, 2: -1, 3: 0}), dict(obs={0: 1, 2: -1, 4: 0})]
    got = _one(run, K.hand(kfs, points, 0, []))
    assert got["pose_row"].tolist() == [1, 2, 0] and got["fixed"].tolist() == [1, 1, 0] and got["num_fixed_kf"] == 2
    assert _edges(got) == [K.edge(0, 2, 0, 0), K.edge(0, 0, 1, 1), K.edge(1, 2, 0, 1)]
    assert 1 not in got["edges"]["pose"].tolist()                                      # the fixed pose without an edge


def rule_edges_skip_bad_observers_and_missing_indices(run):
    """:281, :286, :313 -- and a point whose observations all fall away is listed without an edge"""
    mono = int(np.flatnonzero(K.WORLD[0]["u_right"] < 0)[0])
    stereo = int(np.flatnonzero(K.WORLD[0]["u_right"] >= 0)[0])
    kfs = [dict(slot=0, id=1, holds=[0, 1, 2]), dict(slot=0, id=2), dict(slot=6, id=3, flags=1)]
    points = [dict(obs={0: mono, 1: stereo, 2: 0}), dict(obs={0: -1, 2: 1}), dict(obs={0: stereo, 1: -1})]
    got = _one(run, K.hand(kfs, points, 0, []))
    assert got["point_row"].tolist() == [0, 1, 2] and got["n_points_without_edge"] == 1
    assert _edges(got) == [K.edge(0, 0, 0, mono), K.edge(0, 1, 0, stereo), K.edge(2, 0, 0, stereo)]
    assert got["edges"]["u_right"].tolist() == [-1.0, float(K.WORLD[0]["u_right"][stereo]), float(K.WORLD[0]["u_right"][stereo])]
    assert got["edges"]["inv_sigma2"].tolist() == [float(K.SIGMA[K.WORLD[0]["keys"]["octave"][i]]) for i in (mono, stereo, stereo)]


def rule_poses_go_by_id_and_the_initial_keyframe_is_fixed(run):
    """:163-164, :180-181"""
    kfs = [dict(slot=0, id=50, holds=[0]), dict(slot=1, id=10, holds=[0]), dict(slot=2, id=(1 << 40) + 30), dict(slot=3, id=30)]
    points = [dict(obs={0: 0, 1: 0, 2: 0, 3: 0})]
    got = _one(run, K.hand(kfs, points, 0, [1], init=10))
    assert got["pose_row"].tolist() == [1, 3, 0, 2] and got["fixed"].tolist() == [1, 1, 0, 1]
    assert (got["num_fixed_kf"], got["num_opt_kf"]) == (3, 2)                          # two fixed cameras and the 1 of :85-88
    assert got["edges"]["pose"].tolist() == [2, 0, 3, 1]                               # observations ascend by row, poses by id
    got = _one(run, K.hand(kfs, points, 0, [1], init=30))                              # a fixed camera with the initial id adds nothing
    assert got["fixed"].tolist() == [0, 1, 0, 1] and got["num_fixed_kf"] == 2


def rule_no_fixed_keyframe_aborts(run):
    """:126-130"""
    kfs = [dict(slot=0, id=1, holds=[0]), dict(slot=1, id=2, holds=[0])]
    points = [dict(obs={0: 0, 1: 0})]
    got = _one(run, K.hand(kfs, points, 0, [1]))
    assert got["status"] == ref.ABORTED and got["num_fixed_kf"] == 0 and len(got["pose_row"]) == len(got["point_row"]) == len(got["edges"]) == 0
    got = _one(run, K.hand(kfs, points, 0, [1], init=2))                               # the 1 of :85-88 alone keeps it alive
    assert got["status"] == ref.OK and got["num_fixed_kf"] == 1 and got["fixed"].tolist() == [0, 1] and len(got["edges"]) == 2


def rule_lidar_keyframes(run):
    """:226-253 -- the local keyframes in list order that carry a cloud: none unless more than two, six at the most"""
    def graph(cloud_rows, cov):
        kfs = [dict(slot=i % 12, id=100 - i, flags=4 if i in cloud_rows else 0, holds=[0] if i == 0 else []) for i in range(10)]
        kfs[9]["flags"] |= 1                                                           # a bad neighbour with a cloud does not count
        return K.hand(kfs, [dict(obs={0: 0, 8: 0})], 0, cov)
    got = _one(run, graph({0, 3}, [1, 2, 3, 9]))
    assert got["n_lidar"] == 0 and len(got["lidar_pose_index"]) == 0
    got = _one(run, graph({0, 3, 9, 8}, [1, 2, 3, 9]))                                 # row 8 is fixed, row 9 bad: two clouds
    assert got["n_lidar"] == 0 and got["pose_row"].tolist() == [8, 3, 2, 1, 0]
    got = _one(run, graph({0, 1, 3}, [3, 2, 1, 9]))
    assert got["n_lidar"] == 3 and got["lidar_pose_index"].tolist() == [4, 1, 3]       # rows 0, 3, 1 in list order, as places among the poses
    got = _one(run, graph(set(range(10)), [7, 6, 5, 4, 3, 2, 1, 9]))
    assert got["n_lidar"] == 6 and got["pose_row"].tolist() == [8, 7, 6, 5, 4, 3, 2, 1, 0]
    assert got["lidar_pose_index"].tolist() == [8, 1, 2, 3, 4, 5]                      # rows 0, 7, 6, 5, 4, 3


RULES = [rule_current_is_local_whatever_its_flags, rule_bad_neighbour_is_marked_local, rule_bad_or_other_map_point_is_not_listed,
         rule_point_is_listed_once_at_its_first_occurrence, rule_every_observer_becomes_a_fixed_camera,
         rule_edges_skip_bad_observers_and_missing_indices, rule_poses_go_by_id_and_the_initial_keyframe_is_fixed, rule_no_fixed_keyframe_aborts,
         rule_lidar_keyframes]


@pytest.mark.parametrize("rule", RULES, ids=lambda r: r.__name__)
def test_rule(pkg, rule):
    rule(host_run(pkg))


# ---- contracts -------------------------------------------------------------------------------------------------------------------------
def _base():
    kfs = [dict(slot=0, id=1, holds=[0, 1]), dict(slot=1, id=2, holds=[1]), dict(slot=2, id=3)]
    return K.hand(kfs, [dict(obs={0: 0, 2: 1}), dict(obs={0: 1, 1: 7, 2: -1})], 0, [1])


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
            ("cov_kf out of range", changed(cov_kf=[3]), None), ("cov_kf twice", changed(cov_kf=[1, 1]), None),
            ("cov_kf names the current keyframe", changed(cov_kf=[0]), None),
            ("slot_offsets do not start at 0", changed(slot_offsets=[1, 2, 3, 3]), None), ("slot_offsets descend", changed(slot_offsets=[0, 2, 1, 3]), None),
            ("obs_offsets descend", changed(obs_offsets=[0, 3, 2]), None), ("slot_point below -1", changed(slot_point=[0, -2, 1]), None),
            ("slot_point beyond the points", changed(slot_point=[0, 2, 1]), None), ("obs_kf out of range", changed(obs_kf=[0, 2, 0, 1, 3]), None),
            ("obs_kf negative", changed(obs_kf=[-1, 2, 0, 1, 2]), None), ("observation row not ascending", changed(obs_kf=[2, 0, 0, 1, 2]), None),
            ("observation row with a keyframe twice", changed(obs_kf=[0, 2, 0, 1, 1]), None),
            ("obs_index below -1", changed(obs_index=[0, 1, 1, 7, -2]), None), ("obs_index beyond the slot's keypoints", changed(obs_index=[n0, 1, 1, 7, -1]), None),
            ("obs_index beyond the keypoints of a smaller slot", changed(obs_index=[0, 1, 1, n1, -1]), None),
            ("empty slot", changed(kf_slot=[0, K.EMPTY_SLOT, 2]), None), ("slot out of range", changed(kf_slot=[0, 1, K.WORLD_SLOTS]), None),
            ("slot negative", changed(kf_slot=[0, -1, 2]), None), ("negative capacity", changed(edge_capacity=-1), None),
            ("octave outside the levels", _base(), high)]


def test_invalid_is_refused(pkg):
    assert pkg.ba_window_batch([_base()], K.SIGMA, views=K.WORLD)[0]["status"] == ref.OK
    for what, pr, views in invalid_problems():
        for batch in ([pr], [_base(), pr]):
            with pytest.raises(pkg.Tc2liError) as e:
                pkg.ba_window_batch(batch, K.SIGMA, views=views or K.WORLD)
            assert e.value.code == INVALID, what
    with pytest.raises(pkg.Tc2liError) as e:                                           # the same slot, fewer levels in the table
        pkg.ba_window_batch([_base()], K.SIGMA[:int(K.WORLD[2]["keys"]["octave"].max())], views=K.WORLD)
    assert e.value.code == INVALID


def capacity_contract(run):
    """needed sizes reported for every problem, no list of any problem written"""
    problems = [K.make_graph(500 + i, 8, 50, n_cov=3, bad=0.05, init="other") for i in range(6)]
    want = [ref.gather(p, K.WORLD, K.SIGMA) for p in problems]
    assert all(w["status"] == ref.OK and len(w["edges"]) > 3 for w in want)
    for short in ("pose_capacity", "point_capacity", "edge_capacity"):
        batch = [dict(p) for p in problems]
        n = {"pose_capacity": len(want[3]["pose_row"]), "point_capacity": len(want[3]["point_row"]), "edge_capacity": len(want[3]["edges"])}[short]
        batch[3][short] = n - 1
        with pytest.raises(Exception) as e:
            run(batch, raw=True, fill=SENTINEL)
        assert e.value.code == CAPACITY and "problem 3" in str(e.value), short
        batch[3][short] = n                                                             # exactly enough
        for g, w in zip(run(batch), want):
            K.assert_equal(g, w, short)

    import tc2li_slam_amd.capi as capi                                                  # keep the output arrays of a refused call
    batch = [dict(p) for p in problems]
    batch[3]["edge_capacity"] = 2
    seen = {}
    real = capi.pack_ba_window_problems

    def spy(problems_, fill=0):
        arr, outs, keep = real(problems_, fill)
        seen["outs"] = outs
        return arr, outs, keep
    capi.pack_ba_window_problems = spy
    try:
        with pytest.raises(Exception) as e:
            run(batch, raw=True, fill=SENTINEL)
    finally:
        capi.pack_ba_window_problems = real
    assert e.value.code == CAPACITY
    for o, w in zip(seen["outs"], want):
        c = o["counts"].tolist()
        assert c[:3] == [w["status"], w["num_fixed_kf"], w["num_opt_kf"]] and c[3:6] == [len(w["pose_row"]), len(w["point_row"]), len(w["edges"])]
        assert c[6:] == [w["n_lidar"], w["n_points_without_edge"]]
        for k in ("pose_row", "poses7_out", "fixed", "point_row", "points3_out", "lidar_pose_index"):
            assert (o[k] == np.array(SENTINEL).astype(o[k].dtype)).all(), k
        assert (o["edges"].view(np.uint8) == SENTINEL & 0xff).all()


def test_capacity(pkg):
    capacity_contract(host_run(pkg))


def test_aborted_writes_counts_only(pkg):
    kfs = [dict(slot=0, id=1, holds=[0]), dict(slot=1, id=2, holds=[0])]
    out = host_run(pkg)([K.hand(kfs, [dict(obs={0: 0, 1: 0})], 0, [1])], raw=True, fill=SENTINEL)[0]
    assert out["counts"].tolist() == [ref.ABORTED, 0, 0, 0, 0, 0, 0, 0]
    assert (out["pose_row"] == SENTINEL).all() and (out["point_row"] == SENTINEL).all() and (out["lidar_pose_index"] == SENTINEL).all()


def test_empty_batch_and_limits(pkg):
    assert pkg.ba_window_batch([], K.SIGMA, views=K.WORLD) == []
    lim = pkg.ba_window_limits()
    assert lim["threads"] % 64 == 0 and lim["lds_keyframes"] >= 256 and lim["lds_points"] >= 256


# ---- the outlier rule ------------------------------------------------------------------------------------------------------------------
def test_outliers_by_hand(pkg):
    e = np.zeros(7, ref.EDGE_DTYPE)
    e["point"], e["pose"] = [0, 0, 1, 1, 2, 2, 3], [0, 1, 0, 1, 0, 1, 1]
    e["u_right"] = [5, -1, 5, -1, -1, 5, -1]
    chi2 = np.array([7.815, 5.9911, 7.8151, 5.991, 0.1, 100.0, 0.1])
    dpos = np.array([1, 1, 1, 1, 0, 1, 0], np.uint8)
    bad = np.array([0, 0, 0, 1], np.uint8)
    got = pkg.ba_window_outliers(e, chi2, dpos, bad)
    assert got.tolist() == [[1, 0], [0, 2], [0, 1], [1, 2]]                           # mono first (:406-419), then stereo (:436-449); point 3 is bad
    assert np.array_equal(got, ref.outliers(e, chi2, dpos, bad))
    with pytest.raises(pkg.Tc2liError) as err:
        pkg.ba_window_outliers(e, chi2, dpos, bad, capacity=3)
    assert err.value.code == CAPACITY
    with pytest.raises(pkg.Tc2liError) as err:
        pkg.ba_window_outliers(e, chi2, dpos, bad[:3])
    assert err.value.code == INVALID
    assert pkg.ba_window_outliers(e[:0], chi2[:0], dpos[:0], bad).shape == (0, 2)


def test_outliers_equal_restatement(pkg):
    problems, want = family_of(pkg)
    rng = np.random.default_rng(3)
    n = 0
    for w in want[:12]:
        e = w["edges"]
        chi2 = rng.choice([0.5, 5.0, 5.991, 5.9911, 6.5, 7.815, 7.8151, 30.0], len(e))
        dpos = (rng.random(len(e)) < 0.9).astype(np.uint8)
        bad = (rng.random(len(w["point_row"])) < 0.1).astype(np.uint8)
        got = pkg.ba_window_outliers(e, chi2, dpos, bad)
        assert np.array_equal(got, ref.outliers(e, chi2, dpos, bad))
        n += len(got)
    assert n > 50


# ---- what the optimiser is handed --------------------------------------------------------------------------------------------------------
def test_gathered_window_is_a_well_formed_ba_problem(pkg, synthetic):
    """No BA entry runs without a device, so the arrays are checked for what tc2li_local_bundle_adjustment asks of them: indices in range,
    poses ascending by id, every point with an edge unless it is counted as without one; and they are the window the graph was made from."""
    w = synthetic.ba_window(seed=3, n_opt=4, n_fix=4, n_points=150)
    views, pr, sigma = K.from_window(w)
    got = pkg.ba_window_batch([pr], sigma, views=views)[0]
    K.assert_equal(got, ref.gather(pr, views, sigma))
    e = got["edges"]
    assert got["status"] == ref.OK and len(e) and e["point"].min() >= 0 and e["point"].max() < len(got["point_row"])
    assert e["pose"].min() >= 0 and e["pose"].max() < len(got["pose_row"]) and (np.diff(pr["kf_id"][got["pose_row"]]) > 0).all()
    assert len(got["point_row"]) - len(np.unique(e["point"])) == got["n_points_without_edge"] == 0
    assert (np.diff(e["point"]) >= 0).all() and got["fixed"].tolist() == np.asarray(w["fixed"])[got["pose_row"]].tolist()
    # the window's own edges, in the gather's point order
    mine = {(int(got["point_row"][p]), int(got["pose_row"][k])): (u, v, ur, s) for p, k, u, v, ur, s in e.tolist()}
    theirs = {(int(p), int(k)): (u, v, ur if ur >= 0 else -1.0, s) for p, k, u, v, ur, s in w["edges"].tolist()}   # any negative is monocular (:286)
    listed = set(got["point_row"].tolist())
    assert mine == {k: v for k, v in theirs.items() if k[0] in listed} and len(listed) > 100


def test_gather_kernels_keep_their_resources(tmp_path):
    """The resource report of the compiler for the kernels of the two window gathers and of the structure build: the two gathers, the one
    edge kernel they share and the three k_bas_* kernels, no private memory in any of them, and no less occupancy than before the gathers
    were put on one core (3 waves per SIMD for the gathers, whose 41 KB of LDS allow one workgroup per 64 KB; 8 for the edge kernel)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    report = {}
    for name in ("ba_window_kernels", "inertial_window_kernels", "ba_structure_kernels"):
        src = os.path.join(root, "tc2li-slam_amd", "csrc", name + ".hip")
        out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                              "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / (name + ".o"))],
                             capture_output=True, text=True, check=True).stderr
        names = re.findall(r"Function Name: (\S+)", out)
        scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
        occupancy = [int(v) for v in re.findall(r"Occupancy \[waves/SIMD\]: (\d+)", out)]
        lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out)]
        assert len(names) == len(scratch) == len(occupancy) == len(lds), out
        for n, s, o, l in zip(names, scratch, occupancy, lds):
            kernel = re.search(r"k_[a-z_]+", n).group(0)
            assert kernel not in report, names
            report[kernel] = (s, o, l)
    print(report)
    assert sorted(report) == ["k_bas_blocks", "k_bas_outliers", "k_bas_structure", "k_baw_gather", "k_iw_gather", "k_window_edges"], report
    assert all(s == 0 for s, _, _ in report.values()), report
    assert report["k_baw_gather"][1] >= 3 and report["k_iw_gather"][1] >= 3 and report["k_window_edges"][1] >= 8, report
    assert all(l <= 65536 for _, _, l in report.values()), report
