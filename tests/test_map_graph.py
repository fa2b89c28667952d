"""CPU tests of the edit log of the resident map graph: tc2li_host_map_graph_apply, the plain sequential twin that defines what
tc2li_map_graph_apply_batch must leave on the device, against the Python restatement tests/map_graph_ref.py -- array for array on random
and directed logs, and refusal for refusal.  Everything is an integer or a double carried through: the criterion is equality.  No GPU."""
import functools

import numpy as np
import pytest

import ba_window_cases as K
import map_graph_cases as M
import map_graph_ref as ref

INVALID, CAPACITY = ref.INVALID, ref.CAPACITY
SENTINEL = -77


@functools.lru_cache(maxsize=None)
def cases(lds_row):
    """(name, graph, (edits, values), the tables the restatement gives) for every random and directed log"""
    out = []
    for name, g, (e, v) in M.random_graphs() + M.directed(lds_row):
        out.append((name, g, (e, v), ref.apply(g, e.view(np.int32).reshape(-1, 4), v, M.capacities_for(g, e), M.N_KEYS)))
    return out


def cases_of(pkg):
    return cases(pkg.map_graph_limits()["lds_row"])


def test_limits(pkg):
    lim = pkg.map_graph_limits()
    assert lim["lds_row"] >= 64 and lim["threads"] % 64 == 0 and lim["apply_record_bytes"] <= 64 and lim["gather_record_bytes"] > 0 and lim["max_walk"] >= 1 << 16


def test_cases_reach_every_rule(pkg):
    """The restatement alone: the logs contain what the device tests count on."""
    lim = pkg.map_graph_limits()
    all_cases = cases_of(pkg)
    assert sum(name.startswith("random") for name, *_ in all_cases) == 30
    ops = np.concatenate([e["op"] for _, _, (e, _), _ in all_cases])
    assert set(ops.tolist()) == set(range(len(ref.OPS)))
    assert {0, 1, 63, 64, 65, 256, 257} <= {len(e) for _, _, (e, _), _ in all_cases}
    grown = [(np.diff(g["obs_offsets"]), np.diff(w["obs_offsets"])[:len(g["obs_offsets"]) - 1]) for _, g, _, w in all_cases]
    assert any(((a == 0) & (b == 1)).any() for a, b in grown) and any(((a == 1) & (b == 0)).any() for a, b in grown)
    assert any(((a <= 64) & (b > 64)).any() for a, b in grown)
    assert any(((b > a) & (b == a + 7)).any() and a.max() + 8 == lim["lds_row"] + 1 for a, b in grown)   # the row one beyond the LDS limit


def test_twin_equals_restatement(pkg):
    for name, g, (e, v), want in cases_of(pkg):
        got = pkg.host_map_graph_apply(g, e, v, M.capacities_for(g, e))
        ref.assert_same_tables(got, want, name)


def test_twin_on_an_empty_graph(pkg):
    empty = dict(kf_slot=[], kf_id=[], kf_flags=[], poses7=[], slot_offsets=[0], slot_point=[], point_flags=[], positions=[], obs_offsets=[0], obs_kf=[], obs_index=[])
    L = M.Log(ref.tables_of(empty))
    k = L.add_keyframe(0, 3, 5, 4, range(7))
    p = L.add_point(0, (1, 2, 3))
    L.set_slot(k, 1, p); L.add_observation(p, k, 2)
    e, v = L.done()
    ref.assert_same_tables(pkg.host_map_graph_apply(empty, e, v, (2, 3, 2, 1)), ref.apply(empty, e.view(np.int32).reshape(-1, 4), v, (2, 3, 2, 1)))


def refused_logs():
    """(what, graph, build(Log), capacities or None, the code) for every refusal of the log: INVALID and CAPACITY.  The twin has no store, so
    the two checks against the store's slots are in store_refusals() for the device entry."""
    g = M.wide_graph(n_kf=12)
    n_kf, n_pt, n_slot, n_obs = 12, 12, 48, int(g["obs_offsets"][-1])
    room = np.array([n_kf + 2, n_slot + 8, n_pt + 2, n_obs + 2], np.int32)
    pose = (0, 0, 0, 1, 0, 0, 0)
    out = [("an unknown op", lambda L: L.edits.append((10, 0, 0, 0))), ("a negative op", lambda L: L.edits.append((-1, 0, 0, 0))),
           ("a keyframe row out of range", lambda L: L.set_keyframe_flags(n_kf, 1)), ("a negative keyframe row", lambda L: L.set_pose(-1, pose)),
           ("a point row out of range", lambda L: L.set_point_flags(n_pt, 1)), ("a negative point row", lambda L: L.set_position(-1, (0, 0, 0))),
           ("a keyframe named before its append", lambda L: (L.set_keyframe_flags(n_kf, 1), L.add_keyframe(0, 1, 9, 0, pose))),
           ("a point named before its append", lambda L: (L.add_observation(n_pt, 0, 0), L.add_point(0, (0, 0, 0)))),
           ("a slot out of range", lambda L: L.set_slot(3, 4, 0)), ("a negative slot", lambda L: L.set_slot(3, -1, 0)),
           ("a slot of a new row out of range", lambda L: L.set_slot(L.add_keyframe(0, 2, 9, 0, pose), 2, 0)),
           ("a point below -1 in a slot", lambda L: L.set_slot(3, 0, -2)), ("a point out of range in a slot", lambda L: L.set_slot(3, 0, n_pt)),
           ("an observation index below -1", lambda L: L.add_observation(0, 0, -2)),
           ("an observation of a keyframe out of range", lambda L: L.add_observation(0, n_kf, 0)),
           ("an erase of a keyframe out of range", lambda L: L.erase_observation(0, n_kf)), ("a clear of a point out of range", lambda L: L.clear_observations(n_pt)),
           ("a values offset out of range", lambda L: L.edits.append((ref.OP["SET_POSE"], 0, 1, 0))),
           ("a negative values offset", lambda L: L.edits.append((ref.OP["SET_POSITION"], 0, -1, 0))),
           ("values one short for a keyframe", lambda L: (L.add_keyframe(0, 1, 9, 0, pose), L.values.pop())),
           ("a negative store slot", lambda L: L.add_keyframe(-1, 1, 9, 0, pose)), ("a negative slot count", lambda L: L.add_keyframe(0, -1, 9, 0, pose)),
           ("a keyframe id that is no integer", lambda L: L.add_keyframe(0, 1, 9.5, 0, pose)), ("keyframe flags outside a byte", lambda L: L.add_keyframe(0, 1, 9, 256, pose)),
           ("flags outside a byte", lambda L: L.set_keyframe_flags(0, 256)), ("negative point flags", lambda L: L.add_point(-1, (0, 0, 0)))]
    out = [(what, g, build, room, INVALID) for what, build in out]

    def three_keyframes(L):
        for i in range(3):
            L.add_keyframe(0, 0, 9 + i, 0, pose)
    out += [("keyframe rows beyond the capacity", g, three_keyframes, room, CAPACITY),
            ("slot entries beyond the capacity", g, lambda L: L.add_keyframe(0, 9, 9, 0, pose), room, CAPACITY),
            ("point rows beyond the capacity", g, lambda L: [L.add_point(0, (0, 0, 0)) for _ in range(3)], room, CAPACITY),
            # conservative and exact: the resident entries + the ADD edits, whether they grow a row or not (here all three hit one present pair)
            ("observations at capacity + 1", g, lambda L: [L.add_observation(0, 2, 1) for _ in range(3)], room, CAPACITY)]
    return out


def test_twin_refuses_and_writes_nothing(pkg):
    C = pkg.capi.C
    for what, g, build, room, code in refused_logs():
        L = M.Log(g)
        build(L)
        e, v = L.done()
        with pytest.raises(ref.Refused) as r:
            ref.apply(g, e.view(np.int32).reshape(-1, 4), v, room)
        assert r.value.code == code, what
        tin = pkg.capi.MapGraphTables()
        keep = pkg.capi._pack_map_graph_tables(g, tin)
        tout, arrays = pkg.capi._room_for_map_graph_tables(room, SENTINEL)
        counts = np.full(4, SENTINEL, np.int32)
        f = pkg.lib().tc2li_host_map_graph_apply
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = f(C.addressof(tin), e.ctypes.data, len(e), v.ctypes.data, len(v), C.addressof(tout), room.ctypes.data, counts.ctypes.data)
        assert rc == code, (what, rc)
        assert all((a.astype(np.int64) == np.int64(SENTINEL).astype(a.dtype).astype(np.int64)).all() for a in arrays.values()), what
        assert (counts == SENTINEL).all(), what
        del keep


def test_observation_bound_at_exactly_capacity(pkg):
    """resident + ADD edits == capacity passes (two of the three ADDs hit a present pair, so the row grows by one only)."""
    g = M.wide_graph(n_kf=12)
    caps = np.array([12, 48, 12, int(g["obs_offsets"][-1]) + 3], np.int32)
    L = M.Log(g)
    L.add_observation(0, 2, 1); L.add_observation(0, 4, 1); L.add_observation(0, 2, 5)
    e, v = L.done()
    got = pkg.host_map_graph_apply(g, e, v, caps)
    ref.assert_same_tables(got, ref.apply(g, e.view(np.int32).reshape(-1, 4), v, caps))
    assert int(got["obs_offsets"][-1]) == int(g["obs_offsets"][-1]) + 1
    caps[3] -= 1
    with pytest.raises(pkg.Tc2liError) as r:
        pkg.host_map_graph_apply(g, e, v, caps)
    assert r.value.code == CAPACITY


def test_kernel_resources(tmp_path):
    """The compiler's resource report for csrc/map_graph_kernels.hip: two kernels, no private memory; the apply kernel's LDS is the rows
    under merge (two ints per entry and wavefront), the cells of a step and little else, the write kernel has none."""
    import os
    import re
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = os.path.join(root, "tc2li-slam_amd", "csrc", "map_graph_kernels.hip")
    out = subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off",
                          "-Rpass-analysis=kernel-resource-usage", "-c", src, "-o", str(tmp_path / "map_graph_kernels.o")],
                         capture_output=True, text=True, check=True).stderr
    names = re.findall(r"Function Name: (\S+)", out)
    scratch = [int(v) for v in re.findall(r"ScratchSize \[bytes/lane\]: (\d+)", out)]
    lds = [int(v) for v in re.findall(r"LDS Size \[bytes/block\]: (\d+)", out)]
    vgprs = [int(v) for v in re.findall(r" VGPRs: (\d+)", out)]
    assert len(names) == 2 and "k_mg_apply" in names[0] and "k_mg_write" in names[1], names
    rows_bytes = 2 * 4 * 4 * 256 + 3 * 4 * 256                                         # four wavefronts' rows, the cells of a step
    assert scratch == [0, 0] and rows_bytes <= lds[0] <= rows_bytes + 256 and lds[1] == 0 and max(vgprs) <= 64, (scratch, lds, vgprs)
