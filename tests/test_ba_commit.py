"""CPU tests of tc2li_host_ba_window_commit_log, the closing step of LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:455-485) as an
edit log of the map graph: against literal edit lists on a hand-made window, against the restatement tests/ba_commit_ref.py, and
refusal for refusal.  The log applied by the host twin of the graph must leave the tables the restatement writes directly.  Everything is
an integer or a double carried through (or rounded through float, exactly): the criterion is equality.  No GPU."""
import numpy as np
import pytest

import ba_commit_cases as CC
import ba_commit_ref as cref
import map_graph_cases as M
import map_graph_ref as ref

SENTINEL = -77


def rows(e):
    return [tuple(r) for r in np.asarray(e).view(np.int32).reshape(-1, 4).tolist()]


def caps_of(g):
    return M.capacities_for(g, np.zeros(0, M.EDIT_DTYPE))


def test_main_case_literal(pkg):
    g, w = CC.main_graph(), CC.main_window()
    e, v = pkg.host_ba_window_commit_log(g, w)
    assert rows(e) == CC.MAIN_EDITS                                                    # pair order, the stored index in SET_SLOT, the fixed pose skipped, every point
    assert v.tobytes() == CC.main_values(w).tobytes()
    re_, rv = cref.commit_log(g, w)
    assert re_ == CC.MAIN_EDITS and np.array(rv).tobytes() == v.tobytes()
    # the erased observation's index is not its place in the row: point row 4 is [(0, 5), (1, 2), (3, 0)]
    o = int(g["obs_offsets"][4])
    assert g["obs_kf"][o + 2] == 3 and g["obs_index"][o + 2] == 0 and rows(e)[0] == (ref.OP["SET_SLOT"], 3, 0, -1)


def test_a_keyframe_row_without_resident_slots(pkg):
    g, w = CC.main_graph(without_slots=(1,)), CC.main_window()
    e, v = pkg.host_ba_window_commit_log(g, w)
    assert rows(e) == CC.EDITS_WITHOUT_SLOTS_OF_ROW_1 == cref.commit_log(g, w)[0] and len(e) == len(CC.MAIN_EDITS) - 1
    assert v.tobytes() == CC.main_values(w).tobytes()
    ref.assert_same_tables(pkg.host_map_graph_apply(g, e, v, caps_of(g)), cref.commit(g, w), "a row without slots")


def test_float_flag(pkg):
    g, w = CC.main_graph(), CC.main_window()
    e, v = pkg.host_ba_window_commit_log(g, w, flags=pkg.BA_COMMIT_POSITIONS_F32)
    assert rows(e) == CC.MAIN_EDITS
    assert v[21] == 0.10000000149011612 and w["points3"][0, 0] == 0.1                   # (double)(float)0.1
    assert v[21:].tobytes() == w["points3"].astype(np.float32).astype(np.float64).tobytes()
    assert v[:21].tobytes() == w["poses7"][[0, 2, 3]].tobytes()                         # poses are never rounded
    assert np.array(cref.commit_log(g, w, cref.POSITIONS_F32)[1]).tobytes() == v.tobytes()


@pytest.mark.parametrize("flags", [0, 1])
def test_twin_of_the_log_equals_the_restatement(pkg, flags):
    cases = [("main", CC.main_graph(), CC.main_window())] + CC.random_windows()
    assert sum(len(w["erase"]) > 0 for _, _, w in cases) >= 5 and any(len(w["erase"]) == 0 for _, _, w in cases)
    assert any(w["fixed"].any() and not w["fixed"].all() for _, _, w in cases)
    has_slot = [[0 <= i < n for k, p, i in cref._checked(g, w, 0)[1] for n in [int(np.diff(g["slot_offsets"])[k])]] for _, g, w in cases]
    assert any(any(h) for h in has_slot) and any(not all(h) for h in has_slot)           # pairs with a slot to clear and pairs without
    for name, g, w in cases:
        e, v = pkg.host_ba_window_commit_log(g, w, flags=flags)
        re_, rv = cref.commit_log(g, w, flags)
        assert rows(e) == re_ and v.tobytes() == np.array(rv, np.float64).tobytes(), name
        got = pkg.host_map_graph_apply(g, e, v, caps_of(g))
        ref.assert_same_tables(got, cref.commit(g, w, flags), name)
        ref.assert_same_tables(got, ref.apply(g, np.array(re_, np.int32).reshape(-1, 4), rv, caps_of(g)), name + ": the log through the graph's restatement")
        assert int(got["obs_offsets"][-1]) == int(g["obs_offsets"][-1]) - len(w["erase"]), name


def test_refusals_write_nothing(pkg):
    g = CC.main_graph()
    for what, w, flags, room, code in CC.refused():
        if room is None:                                                               # (the restatement has no arrays to be short of room)
            with pytest.raises(cref.Refused) as r:
                cref.commit_log(g, w, flags)
            assert r.value.code == code, what
        ne, nv = room if room is not None else (64, 64)
        edits, values, sizes = np.full(64, SENTINEL, np.int32).repeat(4).view(M.EDIT_DTYPE), np.full(64, float(SENTINEL)), np.full(2, SENTINEL, np.int32)
        with pytest.raises(pkg.Tc2liError) as r:
            pkg.host_ba_window_commit_log(g, w, flags=flags, edit_capacity=ne, value_capacity=nv, into=(edits, values), sizes=sizes)
        assert r.value.code == code, what
        assert (edits.view(np.int32) == SENTINEL).all() and (values == SENTINEL).all(), what
        if code == cref.CAPACITY:                                                      # the sizes needed are reported
            n_erase = int(w.get("n_erase", len(w["erase"])))
            assert sizes.tolist() == [2 * n_erase + 3 + 6, 7 * 3 + 3 * 6], what
        else:
            assert (sizes == SENTINEL).all(), what


def test_a_window_that_is_not_committed_gives_no_edit(pkg):
    g, w = CC.main_graph(), CC.main_window()
    for what, solved in (("ABORTED", dict(w, status=cref.ABORTED, result=0)), ("refused by the BA", dict(w, result=-2))):
        e, v = pkg.host_ba_window_commit_log(g, solved)
        assert len(e) == 0 and len(v) == 0 and cref.commit_log(g, solved) == ([], []), what
    e, v = pkg.host_ba_window_commit_log(g, dict(w, result=0))                          # iterations == 0 or a raised stop flag: committed
    assert rows(e) == CC.MAIN_EDITS


def test_kernel_resources(tmp_path):
    """The compiler's resource report for csrc/map_graph_commit_kernels.hip: the erase-log kernel and the scatter kernel, no private memory
    and no LDS in either, few registers."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tc2li-slam_amd", "csrc", "map_graph_commit_kernels.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "map_graph_commit_kernels.o")],
                         capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", out)]
    assert len(names) == 2 and "k_mgc_erase_log" in names[0] and "k_mgc_scatter" in names[1], names
    assert scratch == [0, 0] and lds == [0, 0] and max(vgprs) <= 64, (scratch, lds, vgprs)
