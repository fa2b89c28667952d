"""CPU tests of the map update of IMU initialisation: tc2li_host_apply_scaled_rotation_batch and tc2li_host_gba_map_correction_batch against
the numpy restatement tests/map_update_ref.py on the case family of tests/map_update_cases.py, the refusals of all four entries, and the
limits.  Float outputs are compared by bit pattern: the criterion is equality, nothing is left out, there is no tolerance.  No GPU needed
(the comparison with tc2li_map_points_refresh, which has no host twin, is in test_map_update_gpu.py)."""
import functools

import numpy as np
import pytest

import map_update_cases as K
import map_update_ref as ref


@functools.lru_cache(maxsize=None)
def rot_family():
    problems = K.rot_family()
    return problems, [ref.apply_scaled_rotation(p, K.FILL) for p in problems]


@functools.lru_cache(maxsize=None)
def gba_family():
    problems = K.gba_family()
    return problems, [ref.gba_map_correction(p) for p in problems]


@functools.lru_cache(maxsize=None)
def gba_at_capacity():
    """4096 keyframes, the most a problem may have, in a random tree"""
    pr = K.random_gba_problem(31, 4096, 300)
    return pr, ref.gba_map_correction(pr)


def rot(pkg, problems, host=True):
    return pkg.apply_scaled_rotation_batch(problems, host=host, fill=K.FILL)


def gba(pkg, problems, host=True):
    return pkg.gba_map_correction_batch(problems, host=host, fill=K.FILL)


# ---- Map::ApplyScaledRotation ---------------------------------------------------------------------------------------------------------
def test_host_rotation_equals_restatement(pkg):
    problems, want = rot_family()
    counts = [np.diff(p["obs_offsets"]) for p in problems]
    assert {0, 1, 2, 63, 64, 65, 200} <= set(np.concatenate(counts).tolist())
    assert {len(p["kf_pose7"]) for p in problems} >= {0, 1, 65, 300} and {float(p["s"]) for p in problems} == {float(np.float32(v)) for v in (0.1, 1.0, 7.3)}
    assert {(int(p["scaled_vel"]), int(p["has_tcb"])) for p in problems} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    batch = rot(pkg, problems)
    for i, (g, w) in enumerate(zip(batch, want)):
        K.assert_equal(g, w, "problem %d in the batch" % i)
    for i, p in enumerate(problems):
        K.assert_equal(rot(pkg, [p])[0], want[i], "problem %d alone" % i)
    assert rot(pkg, []) == []


def test_rotation_leaves_what_the_reference_leaves(pkg):
    """A bad point is moved but keeps normal and distances; a point without observations likewise; without mTcb no IMU position."""
    problems, _ = rot_family()
    pr = problems[2]
    got = rot(pkg, [pr])[0]
    sentinel = np.frombuffer(bytes([K.FILL] * 4), np.float32)[0]
    bad, none = 6, 0
    assert pr["point_bad"][bad] and pr["obs_offsets"][bad + 1] > pr["obs_offsets"][bad] and pr["obs_offsets"][none + 1] == pr["obs_offsets"][none]
    for i in (bad, none):
        assert (got["point_normal"][i] == sentinel).all() and got["point_min_distance"][i] == sentinel and got["point_max_distance"][i] == sentinel
        assert not (got["point_pos_out"][i] == pr["point_pos"][i]).any()
    touched = np.ones(len(pr["point_bad"]), bool)
    touched[[bad, none]] = False
    assert not (got["point_max_distance"][touched] == sentinel).any()
    assert not (got["kf_imu_pos_out"] == sentinel).any()
    got = rot(pkg, [problems[3]])[0]
    assert (got["kf_imu_pos_out"] == sentinel).all()


def test_identity_rotation_returns_the_positions(pkg):
    pr = K.identity_problem()
    got = rot(pkg, [pr])[0]
    K.assert_equal(got, ref.apply_scaled_rotation(pr, K.FILL))
    assert np.array_equal(got["point_pos_out"].view(np.uint32), pr["point_pos"].view(np.uint32))
    assert np.array_equal(got["kf_inv_pose7_out"][0, 4:], pr["point_pos"][0])           # point 0 lies on keyframe 0's camera centre
    assert np.isnan(got["point_normal"][0]).all() and got["point_max_distance"][0] == 0
    assert not np.isnan(got["point_normal"][[1, 3, 5]]).any()


def _refused(pkg, pack, name, problems, code, word, device_too=True):
    """The host entry and the device entry both refuse `problems` with `code` before touching any output."""
    C = pkg.capi.C
    for entry, host in ((name % "host_", True), (name % "", False)):
        if not host and not device_too:
            continue
        arr, outs, keep = pack(problems, K.FILL)
        f = getattr(pkg.lib(), entry)
        f.argtypes = [C.c_void_p, C.c_int] + ([] if host else [C.c_void_p])
        rc = f(C.addressof(arr), len(problems), *([] if host else [None]))
        assert rc == code, (entry, rc)
        message = pkg.lib().tc2li_last_error().decode()
        assert entry in message and word in message, message
        for o in outs:
            for k, v in o.items():
                assert (v.view(np.uint8) == K.FILL).all(), (entry, k)


def _with(pr, key, where, value):
    bad = dict(pr)
    bad[key] = np.array(pr[key], copy=True)
    bad[key][where] = value
    return bad


def test_rotation_refusals(pkg):
    good = K.rot_problem(40, 4, [2, 0, 3, 1], bad=[3])
    pack = pkg.capi.pack_scaled_rotation_problems
    name = "tc2li_%sapply_scaled_rotation_batch"
    for key, where, value, word in (("obs_offsets", 0, 1, "obs_offsets"), ("obs_offsets", 2, 1, "obs_offsets"), ("obs_kf", 1, 4, "obs_kf"), ("obs_kf", 0, -1, "obs_kf"),
                                    ("point_ref_kf", 0, 4, "point_ref_kf"), ("point_ref_kf", 2, -2, "point_ref_kf"), ("point_ref_kf", 0, -1, "point_ref_kf")):
        _refused(pkg, pack, name, [good, _with(good, key, where, value)], -2, word)
        assert "problem 1" in pkg.lib().tc2li_last_error().decode()
    # -1 is a reference keyframe only for a bad point or one without observations
    assert len(rot(pkg, [_with(_with(good, "point_ref_kf", 3, -1), "point_ref_kf", 1, -1)])) == 1
    C = pkg.capi.C
    for host, entry in ((True, name % "host_"), (False, name % "")):
        f = getattr(pkg.lib(), entry)
        f.argtypes = [C.c_void_p, C.c_int] + ([] if host else [C.c_void_p])
        tail = [] if host else [None]
        for field in ("kf_pose7", "kf_vel", "point_pos", "point_bad", "obs_offsets", "obs_kf", "point_ref_kf", "point_ref_level_scale", "kf_pose7_out",
                      "kf_inv_pose7_out", "kf_vel_out", "point_pos_out", "point_normal", "point_min_distance", "point_max_distance"):
            arr, outs, keep = pack([good], K.FILL)
            setattr(arr[0], field, None)
            assert f(C.addressof(arr), 1, *tail) == -2, (entry, field)
            assert all((v.view(np.uint8) == K.FILL).all() for v in outs[0].values()), (entry, field)
        for field in ("n_keyframes", "n_points"):
            arr, outs, keep = pack([good], K.FILL)
            setattr(arr[0], field, -1)
            assert f(C.addressof(arr), 1, *tail) == -2, (entry, field)
        arr, outs, keep = pack([good], K.FILL)
        assert f(C.addressof(arr), -1, *tail) == -2 and f(None, 1, *tail) == -2
        arr[0].kf_imu_pos_out = None                                                     # optional
        if host:
            assert f(C.addressof(arr), 1) == 1


# ---- the map update after a global BA -----------------------------------------------------------------------------------------------------
def test_host_correction_equals_restatement(pkg):
    problems, want = gba_family()
    batch = gba(pkg, problems)
    for i, (g, w) in enumerate(zip(batch, want)):
        K.assert_equal(g, w, "problem %d in the batch" % i)
    for i, p in enumerate(problems):
        K.assert_equal(gba(pkg, [p])[0], want[i], "problem %d alone" % i)
    assert gba(pkg, []) == []
    # the chains are walked to their ends, every keyframe of them by the chain of poses
    for i, depth in ((3, 1), (4, 2), (5, 70), (6, 300)):
        assert len(problems[i]["kf_parent"]) == depth + 1 and want[i]["kf_visited"].all() and want[i]["kf_in_gba_out"].all()
    big = want[10]
    assert 0 < big["kf_visited"].sum() < 500 and set(big["point_moved"].tolist()) == {0, 1, 2}


def test_correction_paths_one_by_one(pkg):
    pr = K.cut_tree()
    got = gba(pkg, [pr])[0]
    K.assert_equal(got, ref.gba_map_correction(pr))
    same = lambda a, b: np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))
    assert got["kf_visited"].tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 0, 0, 0]             # the bad child cuts 3, 4, 5; 8, 9, 10 are not below an origin
    assert got["kf_in_gba_out"].tolist() == [1, 1, 1, 0, 0, 0, 1, 1, 0, 1, 0]
    assert same(got["kf_pose7_out"][0], pr["kf_gba_pose7"][0]) and same(got["kf_bef_gba_pose7_out"][0], pr["kf_pose7"][0])
    assert same(got["kf_pose7_out"][6], pr["kf_gba_pose7"][6])                           # in the GBA: its own pose
    assert not same(got["kf_pose7_out"][7], pr["kf_gba_pose7"][7])                       # its child follows it
    for k in (3, 4, 5, 8, 9, 10):                                                        # untouched
        assert same(got["kf_pose7_out"][k], pr["kf_pose7"][k]) and same(got["kf_bef_gba_pose7_out"][k], pr["kf_bef_gba_pose7"][k])
        assert same(got["kf_vel_out"][k], pr["kf_vel"][k]) and same(got["kf_bias_out"][k], pr["kf_bias"][k])
    # bImu == false keeps velocity and bias (1 and 7); a child without velocity takes its stored mVwbGBA (2), its bias its own
    for k in (1, 7):
        assert same(got["kf_vel_out"][k], pr["kf_vel"][k]) and same(got["kf_bias_out"][k], pr["kf_bias"][k])
    assert same(got["kf_vel_out"][2], pr["kf_gba_vel"][2]) and same(got["kf_bias_out"][2], pr["kf_bias"][2])
    assert same(got["kf_vel_out"][6], pr["kf_gba_vel"][6]) and same(got["kf_bias_out"][6], pr["kf_gba_bias"][6])
    assert got["point_moved"].tolist() == [1, 2, 2, 0, 0, 2, 0, 0, 1]
    assert same(got["point_pos_out"][0], pr["point_gba_pos"][0]) and same(got["point_pos_out"][3], pr["point_pos"][3])
    assert same(got["point_pos_out"][6], pr["point_pos"][6])
    # point 5: by the stored mTcwBefGBA of keyframe 9 and its unchanged pose
    Xc = ref.se3_point(ref.pose_of(pr["kf_bef_gba_pose7"][9]), ref.vec_of(pr["point_pos"][5]))
    assert same(got["point_pos_out"][5], np.array(ref.se3_point(ref.se3_inverse(ref.pose_of(pr["kf_pose7"][9])), Xc), np.float32))


def test_correction_capacity(pkg):
    pr, want = gba_at_capacity()
    assert pkg.map_update_limits()["max_keyframes"] == 4096 == len(pr["kf_parent"])
    K.assert_equal(gba(pkg, [pr])[0], want, "4096 keyframes")
    parent, origin = K.chain(4096)
    over = K.gba_problem(32, parent, origin, 3)
    _refused(pkg, pkg.capi.pack_gba_correction_problems, "tc2li_%sgba_map_correction_batch", [K.cut_tree(), over], -5, "4096")


def test_correction_refusals(pkg):
    good = K.cut_tree()
    pack = pkg.capi.pack_gba_correction_problems
    name = "tc2li_%sgba_map_correction_batch"
    cycle = _with(_with(good, "kf_parent", 8, 10), "kf_parent", 9, 8)                    # 8 -> 10 -> 9 -> 8, apart from the tree
    for bad, word in ((_with(good, "kf_parent", 2, 11), "kf_parent"), (_with(good, "kf_parent", 2, -2), "kf_parent"), (_with(good, "kf_parent", 0, 5), "origin"),
                      (_with(good, "kf_parent", 1, 5), "cycle"), (_with(good, "kf_parent", 4, 4), "cycle"), (cycle, "cycle"),
                      (_with(good, "point_ref_kf", 1, 11), "point_ref_kf"), (_with(good, "point_ref_kf", 1, -1), "point_ref_kf"),
                      (_with(good, "point_ref_kf", 6, -2), "point_ref_kf")):
        _refused(pkg, pack, name, [good, bad], -2, word)
        assert "problem 1" in pkg.lib().tc2li_last_error().decode()
    C = pkg.capi.C
    for host, entry in ((True, name % "host_"), (False, name % "")):
        f = getattr(pkg.lib(), entry)
        f.argtypes = [C.c_void_p, C.c_int] + ([] if host else [C.c_void_p])
        tail = [] if host else [None]
        for field, _ in pkg.capi.GbaCorrectionProblem._fields_[:26]:
            arr, outs, keep = pack([good], K.FILL)
            setattr(arr[0], field, None)
            assert f(C.addressof(arr), 1, *tail) == -2, (entry, field)
            assert all((v.view(np.uint8) == K.FILL).all() for v in outs[0].values()), (entry, field)
        for field in ("n_keyframes", "n_points"):
            arr, outs, keep = pack([good], K.FILL)
            setattr(arr[0], field, -1)
            assert f(C.addressof(arr), 1, *tail) == -2, (entry, field)
        arr, outs, keep = pack([good], K.FILL)
        assert f(C.addressof(arr), -1, *tail) == -2 and f(None, 1, *tail) == -2


def test_limits_and_missing_device(pkg):
    lim = pkg.map_update_limits()
    assert lim == dict(max_keyframes=4096, walk_threads=256, keyframe_tile=64, point_tile=256)
    C = pkg.capi.C
    f = pkg.lib().tc2li_map_update_limits
    f.argtypes = [C.c_void_p, C.c_int]
    assert f(None, 4) == -2 and f((C.c_int32 * 3)(), 3) == -2
    if pkg.device_count() == 0:                                                          # no quiet fall-back to the host twins
        with pytest.raises(Exception, match="no HIP device"):
            pkg.apply_scaled_rotation_batch([K.identity_problem()])
        with pytest.raises(Exception, match="no HIP device"):
            pkg.gba_map_correction_batch([K.cut_tree()])
