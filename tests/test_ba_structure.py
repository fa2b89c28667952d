"""CPU tests of tc2li_host_ba_structure: the index structure the local BA builds from (fixed, edges), against lists written out by hand and
against the restatement tests/ba_structure_ref.py on gathered windows.  Integers only, so the criterion is equality.  No GPU needed."""
import functools

import numpy as np
import pytest

import ba_structure_ref as sref
import ba_window_cases as K
import ba_window_ref as wref

INVALID = -2
WINDOWS = [(n_opt, n_points) for n_opt in (1, 4, 21, 22, 24) for n_points in (40, 150, 700)]


def edges_of(pairs):
    e = np.zeros(len(pairs), wref.EDGE_DTYPE)
    if len(pairs):
        e["point"], e["pose"] = np.array(pairs).T
    return e


def assert_structure(got, want, what=""):
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, int):
            assert g == w, (what, k, g, w)
        else:
            assert np.asarray(g).tolist() == list(w), (what, k, np.asarray(g).tolist(), list(w))


def extra_used(n_poses, lidar_pose_index):
    x = np.zeros(n_poses, np.uint8)
    x[np.asarray(lidar_pose_index, np.int64)] = 1
    return x


def check_gathered(pkg, got, what=""):
    """A gathered window through the entry and the restatement -> the structure, or None where both refuse it."""
    e, fixed, n_points = got["edges"], got["fixed"], len(got["point_row"])
    xu = extra_used(len(fixed), got["lidar_pose_index"]) if got["n_lidar"] else None
    used = np.bincount(e["pose"], minlength=len(fixed)) + (0 if xu is None else xu)
    if ((fixed == 0) & (used > 0)).sum() > sref.LEAN_MAX_FREE:
        return "wide"                                                                   # beyond the sparse path: not the restatement's ground
    try:
        want = sref.structure(fixed.tolist(), n_points, e["point"].tolist(), e["pose"].tolist(), None if xu is None else xu.tolist())
    except sref.Invalid:
        with pytest.raises(pkg.Tc2liError) as err:
            pkg.capi.host_ba_structure(fixed, n_points, e, xu)
        assert err.value.code == INVALID, what
        return None
    s = pkg.capi.host_ba_structure(fixed, n_points, e, xu)
    assert_structure(s, want, what)
    return s


@functools.lru_cache(maxsize=None)
def gathered_windows(pkg, synthetic):
    out = []
    for seed, (n_opt, n_points) in enumerate(WINDOWS):
        w = synthetic.ba_window(seed, n_opt=n_opt, n_fix=5, n_points=n_points)
        if n_opt >= 4 and seed % 2:
            w["win_pose"] = list(range(len(w["poses"]) - 4, len(w["poses"])))       # the LiDAR keyframes count as used
        views, pr, sigma = K.from_window(w)
        out.append((views, pr, sigma))
    return out


# ---- by hand ---------------------------------------------------------------------------------------------------------------------------
def test_three_poses_three_points(pkg):
    """pose 0 fixed; edges in creation order, not point-major"""
    e = edges_of([(0, 0), (1, 1), (0, 1), (2, 2), (1, 2), (2, 0)])
    s = pkg.capi.host_ba_structure([1, 0, 0], 3, e)
    want = dict(n_free=2, n_slots=4, n_free_pose_edges=4, n_dups=0, n_blocks=1, n_groups=1, max_group_landmarks=3, np=12, np_pad=16, n_schur_slices=1,
                n_slices=1, k_per_slice=0, schur_group=8, sparse=1, schur_rd=5, schur_ro=2,
                pose_var=[-1, 0, 1], pt_off=[0, 2, 4, 6], pt_edges=[0, 2, 1, 4, 3, 5], pv_off=[0, 2, 4], pv_edges=[1, 2, 3, 4],
                fl_off=[0, 1, 1, 3, 3, 4], fl_pose=[0, 0, 1, 1], fl_lm=[0, 1, 1, 2], fl_place=[0, 1, 1, 2], fl_edge=[2, 1, 4, 3],
                w_slot=[-1, 1, 0, 3, 2, -1], slice_off=[0, 4], dup_off=[0, 0, 0], dup_edge=[], dup_slot=[],
                blk_off=[0, 2, 4], blk_rows=[0, 1, 2, 3] + [0] * 252, grp_k0=[0, 6], grp_l0=[0, 3], chunk_mask=[])
    assert_structure(s, want)
    assert_structure(s, sref.structure([1, 0, 0], 3, e["point"].tolist(), e["pose"].tolist()))


def test_point_seen_from_fixed_poses_only(pkg):
    e = edges_of([(0, 0), (0, 2), (1, 0), (1, 1), (2, 1)])
    s = pkg.capi.host_ba_structure([1, 0, 1], 3, e)
    assert s["fl_off"].tolist() == [0, 0, 0, 1, 1, 2]                                  # point 0: an empty range, and no place in a slice
    assert (s["fl_lm"].tolist(), s["fl_place"].tolist(), s["fl_edge"].tolist(), s["w_slot"].tolist()) == ([1, 2], [0, 1], [3, 4], [-1, -1, -1, 0, 1])
    assert s["pose_var"].tolist() == [-1, 0, -1] and s["pv_off"].tolist() == [0, 2] and s["slice_off"].tolist() == [0, 2]
    assert_structure(s, sref.structure([1, 0, 1], 3, e["point"].tolist(), e["pose"].tolist()))


def test_free_pose_without_an_edge(pkg):
    e = edges_of([(0, 0), (0, 1)])
    s = pkg.capi.host_ba_structure([1, 0, 0], 1, e)
    assert s["pose_var"].tolist() == [-1, 0, -1] and s["n_free"] == 1                   # pose 2 is free and unused: no variable
    x = pkg.capi.host_ba_structure([1, 0, 0], 1, e, extra_used=[0, 0, 1])
    assert x["pose_var"].tolist() == [-1, 0, 1] and x["n_free"] == 2 and x["pv_off"].tolist() == [0, 1, 1] and x["np"] == 12
    assert x["blk_off"].tolist() == [0, 1, 1] and x["fl_pose"].tolist() == [0]
    f = pkg.capi.host_ba_structure([1, 0, 0], 1, e, extra_used=[1, 0, 0])              # a fixed pose stays without one
    assert f["pose_var"].tolist() == [-1, 0, -1]
    for xu, got in ((None, s), ([0, 0, 1], x), ([1, 0, 0], f)):
        assert_structure(got, sref.structure([1, 0, 0], 1, [0, 0], [0, 1], xu))
    none = pkg.capi.host_ba_structure([1, 1], 1, edges_of([(0, 0), (0, 1)]))            # no free pose at all
    assert (none["n_free"], none["n_slots"], none["n_blocks"], none["n_schur_slices"]) == (0, 0, 0, 0)
    assert none["slice_off"].tolist() == [0] and none["blk_off"].tolist() == [0] and none["blk_rows"].tolist() == [0] * 256
    assert_structure(none, sref.structure([1, 1], 1, [0, 0], [0, 1]))


def test_duplicate_pair(pkg):
    """the second edge of a (point, free pose) pair gets no slot and is listed with the first one's"""
    e = edges_of([(0, 1), (0, 0), (0, 1), (1, 1), (1, 2), (1, 2)])
    s = pkg.capi.host_ba_structure([1, 0, 0], 2, e)
    assert (s["n_slots"], s["n_free_pose_edges"], s["n_dups"]) == (3, 5, 2)
    assert s["w_slot"].tolist() == [0, -1, -1, 1, 2, -1] and s["fl_edge"].tolist() == [0, 3, 4] and s["fl_off"].tolist() == [0, 1, 1, 3]
    assert (s["dup_off"].tolist(), s["dup_edge"].tolist(), s["dup_slot"].tolist()) == ([0, 1, 2], [2, 5], [0, 2])
    assert s["pv_off"].tolist() == [0, 2, 3] and s["pv_edges"].tolist() == [0, 3, 4]     # the slots' edges only
    assert_structure(s, sref.structure([1, 0, 0], 2, e["point"].tolist(), e["pose"].tolist()))


# ---- gathered windows ------------------------------------------------------------------------------------------------------------------
def test_gathered_windows_equal_restatement(pkg, synthetic):
    seen = []
    for (views, pr, sigma), (n_opt, n_points) in zip(gathered_windows(pkg, synthetic), WINDOWS):
        got = pkg.ba_window_batch([pr], sigma, views=views)[0]
        assert got["status"] == wref.OK
        s = check_gathered(pkg, got, "n_opt %d, %d points" % (n_opt, n_points))
        assert s is not None and s["n_free"] == n_opt and s["n_dups"] == 0
        assert s["pt_off"].tolist() == np.r_[0, np.cumsum(np.bincount(got["edges"]["point"], minlength=len(got["point_row"])))].tolist()
        assert s["pt_edges"].tolist() == list(range(len(got["edges"])))                 # the gather's edges are point-major already
        seen.append(s)
    assert max(s["n_schur_slices"] for s in seen) > 2 * 8 and max(s["n_groups"] for s in seen) > 2 and max(s["n_blocks"] for s in seen) > 2
    assert {s["schur_ro"] for s in seen} == {1, 2} and any(s["n_free"] > 21 and s["np_pad"] > 128 for s in seen)


def test_family_equals_restatement(pkg):
    lim = pkg.ba_window_limits()
    problems = K.family(lim["lds_keyframes"], lim["lds_points"])
    n_ok = n_refused = 0
    for i, got in enumerate(pkg.ba_window_batch(problems, K.SIGMA, views=K.WORLD)):
        if got["status"] != wref.OK:
            continue
        s = check_gathered(pkg, got, "family graph %d" % i)
        if isinstance(s, str):
            continue
        assert (s is None) == (got["n_points_without_edge"] > 0), i                      # what the family's graphs are refused for
        n_ok, n_refused = n_ok + (s is not None), n_refused + (s is None)
    assert n_ok >= 5 and n_refused >= 5


def test_error_returns(pkg):
    ok = [(0, 0), (0, 1), (1, 1)]
    pkg.capi.host_ba_structure([1, 0], 2, edges_of(ok))
    many = [(0, k) for k in range(257)] + [(1, 0)]
    cases = [("point without an edge", [1, 0], 3, ok), ("pose out of range", [1, 0], 2, ok + [(1, 2)]), ("point out of range", [1, 0], 2, ok + [(2, 1)]),
             ("negative pose", [1, 0], 2, ok + [(1, -1)]), ("257 edges on one point", [0, 0] + [1] * 255, 2, many)]
    for what, fixed, n_points, pairs in cases:
        e = edges_of(pairs)
        with pytest.raises(pkg.Tc2liError) as err:
            pkg.capi.host_ba_structure(fixed, n_points, e)
        assert err.value.code == INVALID, what
        with pytest.raises(sref.Invalid):
            sref.structure(fixed, n_points, e["point"].tolist(), e["pose"].tolist())
    s = pkg.capi.host_ba_structure([0, 0] + [1] * 255, 2, edges_of(many[:256] + [(1, 0)]))    # 256 edges on one point are fine
    assert s["n_groups"] == 2 and s["grp_k0"].tolist() == [0, 256, 257] and s["grp_l0"].tolist() == [0, 1, 2]
