"""The CPU restatement of velodyne_handler's feature branch (tests/feature_classifier_ref.py) on hand-built lines, and the C ABI of the
switch (header declarations, library exports).  No GPU needed."""
import os
import re
import subprocess

import numpy as np
import pytest

import feature_classifier_ref as ref
from feature_classifier_ref import EDGE_JUMP, EDGE_PLANE, NOR, POSS_PLANE, REAL_PLANE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def wall(n=40, x=5.0, y0=-1.0, dy=0.05, z=-1.0):
    """Points along a flat wall x = const at one height: one ring's trace."""
    return np.stack([np.full(n, x), y0 + dy * np.arange(n), np.full(n, z)], 1)


def depth_step():
    """A rough (non-planar) near surface, then a far one behind it along the same rays."""
    k = np.arange(40)
    th = 0.01 * k
    r = np.where(k < 16, 5.0, 8.0) + 0.05 * (-1.0) ** k
    return np.stack([r * np.cos(th), r * np.sin(th), np.full(40, -0.5)], 1)


def corner():
    """Two walls at 90 degrees: x = 5, then y = 1."""
    a = np.stack([np.full(22, 5.0), 1.0 - 0.05 * np.arange(22)[::-1] - 0.05, np.full(22, -1.0)], 1)
    b = np.stack([5.0 - 0.05 * np.arange(30), np.full(30, 1.0), np.full(30, -1.0)], 1)
    return np.concatenate([a, b])


def run(points, pfn=1, blind=0.5, n_lines=1, dis_b=0.0):
    return ref.classify(ref.make_raw(points), n_lines, pfn, blind, 1e-3, dis_b)


def edge_case_scan():
    """The hand-built lines as one scan, a case per ring, interleaved in input order; rings past every n_lines tested are dropped."""
    cases = [wall(), depth_step(), corner(), wall(5), np.full((12, 3), 0.05), np.repeat(wall(20), 2, axis=0), wall(64, dy=0.02),
             wall(23, dy=0.04), depth_step()[::-1].copy()]
    raws = [ref.make_raw(p, ring=k) for k, p in enumerate(cases)]
    raws.append(ref.make_raw(wall(10, x=6.0), ring=40))    # dropped with n_lines = 32
    raws.append(ref.make_raw(wall(10, x=7.0), ring=200))   # beyond pl_buff[128]
    raw = np.concatenate(raws)
    order = np.argsort(np.concatenate([np.arange(len(r)) * 1.0 + 0.01 * k for k, r in enumerate(raws)]), kind="stable")
    return raw[order].copy()


def test_flat_wall_is_a_plane():
    surf, corn, lab, off = run(wall())
    assert lab[0] == POSS_PLANE and lab[33] == POSS_PLANE  # the first and the last plane group's ends
    assert set(lab[1:33]) == {REAL_PLANE}
    assert len(corn) == 0 and len(surf) == 38  # the last two points are Nor


def test_depth_step_is_an_edge_jump():
    surf, corn, lab, off = run(depth_step())
    assert list(np.nonzero(lab == EDGE_JUMP)[0]) == [15]
    assert len(corn) == 1 and corn[0, 0] == np.float32(depth_step()[15, 0])


def test_two_walls_at_right_angles_give_an_edge_plane():
    surf, corn, lab, off = run(corner())
    assert list(np.nonzero(lab == EDGE_PLANE)[0]) == [22]
    assert len(corn) == 1


def test_line_shorter_than_a_group():
    surf, corn, lab, off = run(wall(7))
    assert POSS_PLANE not in lab and EDGE_PLANE not in lab  # pass 1 does not run (plsize2 = 0); pass 3 still finds small planes
    surf, corn, lab, off = run(wall(1))  # fewer than 2 points: nothing
    assert len(lab) == 1 and len(surf) == 0


def test_all_blind_line_gives_nothing():
    surf, corn, lab, off = run(np.full((12, 3), 0.05), blind=0.5)
    assert len(surf) == 0 and len(corn) == 0 and set(lab) == {NOR}


def test_duplicate_points_hit_the_gates():
    # every other dista is 0: plane_judge's second-smallest disarr element is 0 (< 1e-16), pass 2 skips (1e-16), pass 3 skips (1e-8)
    surf, corn, lab, off = run(np.repeat(wall(20), 2, axis=0))
    assert set(lab) == {NOR} and len(surf) == 0
    # all points equal: leng_wid = 0 and two_dis = 0 -> 0 / 0 = NaN, which fails `< p2l_ratio`; the walk reaches the end
    L = ref._Line(*(np.full(12, v, np.float32) for v in (5.0, 0.0, -1.0)), np.zeros(12, np.float32), np.zeros(12, np.float32))
    t, i_nex, cd = ref.plane_judge(L, 0, 0.5, 0.0)
    assert t == 0 and i_nex == 12


def test_small_plane_alternation_on_a_run_of_three():
    # three consecutive points satisfy pass 3's test: the first fires and relabels the second, which is skipped; the third fires
    L = ref._Line(*(np.zeros(7, np.float32) for _ in range(5)))
    L.n = 7
    L.range = [5.0] * 7
    L.dista = [0.01] * 7
    L.ftype = [NOR] * 7
    L.intersect = [2.0, 2.0, -1.0, -1.0, -1.0, 2.0, 2.0]
    fired = []
    # pass 3 alone, as give_feature runs it (head = 0)
    for i in range(1, L.n - 1):
        if L.ftype[i] == NOR and L.intersect[i] < ref.SMALLP_INTERSECT:
            fired.append(i)
            for k in (i - 1, i, i + 1):
                if L.ftype[k] == NOR:
                    L.ftype[k] = REAL_PLANE
    assert fired == [2, 4]  # fired[i] = c[i] and not fired[i - 1]
    assert L.ftype == [NOR, REAL_PLANE, REAL_PLANE, REAL_PLANE, REAL_PLANE, REAL_PLANE, NOR]
    # the same through the restatement on a real line: a collinear, evenly spaced run that pass 1 leaves Nor
    surf, corn, lab, off = run(wall(64, dy=0.02), blind=0.5)
    assert (lab == REAL_PLANE).sum() > 0


@pytest.mark.parametrize("pfn", [1, 2, 3, 4])
def test_point_filter_num_groups_and_averages(pfn):
    pts = wall()
    surf, corn, lab, off = run(pts, pfn=pfn)
    isurf = np.nonzero((lab == POSS_PLANE) | (lab == REAL_PLANE))[0]
    assert list(isurf) == list(range(38))  # one run of 38 surface points, then 2 Nor points end it
    want = []
    for g in range(0, 38, pfn):
        grp = list(range(g, min(g + pfn, 38)))
        P = ref.make_raw(pts)
        if len(grp) == pfn:
            want.append(np.float32(P["x"][grp[-1]]) * 0 + np.float32(P["y"][grp[-1]]))
        else:  # the remainder, averaged in float in line order
            s = np.float32(0)
            for k in grp:
                s = np.float32(s + P["y"][k])
            want.append(np.float32(s / np.float32(len(grp))))
    assert len(surf) == len(want) and np.array_equal(surf[:, 1], np.array(want, np.float32))
    assert np.all(surf[:, 3] == 1.0) and np.all(surf[:, 4:8] == 0)


def test_run_reaching_the_line_end_is_dropped():
    # pass 3 labels the collinear tail: all 64 points are one surface run that reaches the line's end
    pts = wall(64, dy=0.02)
    lab = run(pts)[2]
    assert np.all((lab == POSS_PLANE) | (lab == REAL_PLANE))
    for pfn in (3, 5, 7):  # 64 % pfn points left over: no average for them
        surf = run(pts, pfn=pfn)[0]
        assert len(surf) == 64 // pfn
        assert np.array_equal(surf[:, 1], ref.make_raw(pts)["y"][pfn - 1::pfn][:64 // pfn])


def test_rings_past_n_lines_are_dropped():
    raw = edge_case_scan()
    for n_lines in (64, 32, 128):
        surf, corn, lab, off = ref.classify(raw, n_lines, 1, 0.5)
        kept = int((raw["ring"] < n_lines).sum())
        assert off[-1] == kept == len(lab) and len(off) == n_lines + 1
        assert (kept == len(raw) - 10) if n_lines == 128 else True  # ring 200 always goes
    assert ref.classify(raw, 32, 1, 0.5)[3][-1] == ref.classify(raw, 64, 1, 0.5)[3][-1] - 10


def test_last_point_dista_is_zero_and_reachable():
    # a wall walked to the line's end by plane_judge: the last point's dista (never written by the reference) is pushed into disarr
    L = ref._Line(*(np.asarray(c, np.float32) for c in wall(23, dy=0.04).T), np.zeros(23, np.float32), np.zeros(23, np.float32))
    assert L.dista[-1] == 0.0
    t, i_nex, cd = ref.plane_judge(L, 14, 0.5, 0.0)
    assert i_nex == 23 and t == 1  # the walk reached the end (disarr holds the 0.0, and it is the smallest: the second-smallest decides)
    surf, corn, lab, off = run(wall(23, dy=0.04))
    assert lab[-1] == REAL_PLANE  # types[n] (the walk's end) is out of the line; the last point is inside the group


def test_header_declares_and_library_exports_the_entries():
    text = open(os.path.join(ROOT, "include", "tc2li_hip.h")).read()
    names = ["tc2li_lidar_set_preprocess_features", "tc2li_lidar_corner_points", "tc2li_lidar_point_labels"]
    for n in names:
        assert re.search(r"\bint %s\(" % n, text), n
    assert "tc2li_preprocess_features" in text
    lib = os.path.join(ROOT, "tc2li-slam_amd", "lib", "libtc2li_hip.so")
    if not os.path.exists(lib):
        import __graft_entry__ as ge
        ge.build_native()
    out = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
    for n in names:
        assert re.search(r"\bT %s$" % n, out, re.M), n
