"""GPU tests of LocalMapping::ProcessNewKeyFrame in one call: tc2li_process_new_keyframe_batch against its host twin on every case of
process_new_keyframe_cases.py (integers exactly, floats bit for bit) and against the cases' literal lists; the batch alone, shuffled and
reversed; one store slot in two problems; normals, distances and the chosen descriptor against tc2li_map_points_refresh on the end state;
the connection half against tc2li_update_connections_batch on the end state; the chosen descriptor against what
tc2li_search_in_neighbors_batch's refresh chooses on the same observations; the observation limit (finished by the host twin inside the
call); 64 problems in one call; and the INVALID and CAPACITY contracts on the device entry."""
import numpy as np
import pytest

import mapping_cases as mc
import process_new_keyframe_cases as pc
import search_in_neighbors_cases as sc
from test_process_new_keyframe import (CONN_OUTPUTS, bits, check_capacity_contract, check_expect, end_state_problem, invalid_problems, run_raw, same,
                                       untouched)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(pkg):
    """every case's keyframes in one store, every case's host result"""
    cases = pc.all_cases()
    views, problems = pc.on_one_store(cases)
    store = pkg.KeyframeStore(len(views) + 1, 320)
    store.put_batch(np.arange(len(views)), views, mc.BOUNDS0)
    host = pkg.process_new_keyframe_batch(problems, views=views)
    yield dict(cases=cases, store=store, views=views, problems=problems, host=host, names=[c["name"] for c in cases])
    store.close()


def device(pkg, w, problems, **kw):
    return pkg.process_new_keyframe_batch(problems, store=w["store"], **kw)


def test_device_equals_the_host_twin(pkg, world):
    got = device(pkg, world, world["problems"])
    for c, g, h in zip(world["cases"], got, world["host"]):
        same(g, h, c["name"])
        assert g["status"] == (pkg.PROCESS_KEYFRAME_ON_HOST if c["name"] == "limit" else pkg.PROCESS_KEYFRAME_ON_DEVICE), c["name"]
        assert dict(g["counts"], status=0) == dict(h["counts"], status=0), c["name"]
        check_expect(c, g)
        same(g, pc.want_of(c), c["name"])   # and so equals the Python restatement


def small(world):
    return [i for i, c in enumerate(world["cases"]) if c["name"] not in ("limit", "many_rows")]


def test_arrangements_give_the_same_bits(pkg, world):
    """the batch as a whole, one by one, shuffled and reversed"""
    idx = small(world)
    problems = [world["problems"][i] for i in idx]
    batch = device(pkg, world, problems)
    for k, pr in enumerate(problems):
        same(device(pkg, world, [pr])[0], batch[k], ("alone", k))
    order = np.random.default_rng(5).permutation(len(problems))
    for k, g in zip(order, device(pkg, world, [problems[k] for k in order])):
        same(g, batch[k], ("shuffled", int(k)))
    for k, g in zip(range(len(problems) - 1, -1, -1), device(pkg, world, problems[::-1])):
        same(g, batch[k], ("reversed", k))
    for i, g in zip(idx, batch):
        same(g, world["host"][i], world["names"][i])


def test_one_store_slot_in_two_problems(pkg, world):
    """the same keyframes under two graphs: the second has its camera centres elsewhere and one observer bad"""
    i = world["names"].index("random_3")
    a = world["problems"][i]
    b = dict(a, centres=(np.asarray(a["centres"], np.float32) + np.float32(0.5)), kf_flags=np.array(a["kf_flags"], np.uint8).copy())
    others = [k for k in range(len(b["kf_flags"])) if k != a["current"]]
    b["kf_flags"][others[0]] ^= 1
    got = device(pkg, world, [a, b, a])
    host = pkg.process_new_keyframe_batch([a, b], views=world["views"])
    same(got[0], host[0], "a"); same(got[1], host[1], "b"); same(got[2], host[0], "a again")
    on = got[0]["refreshed"].astype(bool)
    assert on.any() and not np.array_equal(bits(got[0]["normals_out"][on]), bits(got[1]["normals_out"][on]))


def test_refresh_equals_map_points_refresh(pkg, world):
    """normals, distances and the chosen descriptor of the associated points equal tc2li_map_points_refresh on the end-state rows.  That
    entry is handed the observations it should use, so the descriptor is compared where no observer is bad."""
    picked = small(world)
    got = device(pkg, world, [world["problems"][i] for i in picked])
    checked = 0
    for i, g in zip(picked, got):
        pr, c = world["problems"][i], world["cases"][i]
        local = c["problem"]["kf_slot"]
        rows = np.flatnonzero(g["refreshed"])
        if not len(rows):
            continue
        assert rows.tolist() == sorted(g["associated_point"].tolist()), c["name"]
        off, okf, oidx = g["obs_offsets_out"], g["obs_kf_out"], g["obs_index_out"]
        sel = np.concatenate([np.arange(off[p], off[p + 1]) for p in rows])
        desc = np.array([c["views"][local[okf[o]]]["descriptors"][oidx[o]] for o in sel], np.uint8)
        new_off = np.concatenate([[0], np.cumsum(off[rows + 1] - off[rows])]).astype(np.int32)
        centres = np.asarray(pr["centres"], np.float32).reshape(-1, 3)
        positions = np.asarray(pr["positions"], np.float32).reshape(-1, 3)
        best, normals, mn, mx = pkg.capi.map_points_refresh(new_off, desc, centres[okf[sel]], positions[rows], centres[pr["point_ref_kf"][rows]],
                                                            pr["point_ref_level_scale"][rows], pr["last_level_scale"])
        for a, b, k in ((g["normals_out"][rows], normals, "normal"), (g["min_distance_out"][rows], mn, "min"), (g["max_distance_out"][rows], mx, "max")):
            assert np.array_equal(bits(a), bits(b)), (c["name"], k)
        if not (np.asarray(pr["kf_flags"]) & 1).any():
            assert np.array_equal(okf[off[rows] + best], g["desc_kf"][rows]) and np.array_equal(oidx[off[rows] + best], g["desc_index"][rows]), c["name"]
            checked += 1
    assert checked >= 8


def test_connections_equal_update_connections_batch_on_the_end_state(pkg, world):
    got = device(pkg, world, world["problems"])
    want = pkg.update_connections_batch([end_state_problem(pr, g) for pr, g in zip(world["problems"], got)])
    for name, g, w in zip(world["names"], got, want):
        for k in CONN_OUTPUTS:
            assert np.array_equal(g["connections"][k], w[k]), (name, k)
    assert any(g["connections"]["status"] == 0 for g in got) and sum(len(g["connections"]["changed_kf"]) > 0 for g in got) >= 8


def test_descriptor_choice_equals_search_in_neighbors(pkg, world, synthetic):
    """the refresh at the end of tc2li_search_in_neighbors_batch (no targets, so nothing is fused) runs ComputeDistinctiveDescriptors on every
    point of the current keyframe's slot row that is not bad; handed this entry's end state it chooses the same observations"""
    env = sc.env_of(synthetic)
    picked = [i for i in small(world) if len(world["host"][i]["associated_point"])]
    got = device(pkg, world, [world["problems"][i] for i in picked])
    checked = 0
    for i, g in zip(picked, got):
        pr, c = world["problems"][i], world["cases"][i]
        nk, npts, cur = len(pr["kf_flags"]), len(pr["point_bad"]), int(pr["current"])
        n_keys = [len(c["views"][s]["keys"]) for s in c["problem"]["kf_slot"]]
        so = np.concatenate([[0], np.cumsum(n_keys)]).astype(np.int32)
        slot_point = np.full(int(so[-1]), -1, np.int32)
        slot_point[so[cur]:so[cur + 1]] = pr["slot_point"]
        points = np.zeros(npts, mc.MP)
        points["pos"] = np.asarray(pr["positions"], np.float32).reshape(-1, 3)
        nb = dict(kf_slot=pr["kf_slot"], kf_flags=np.asarray(pr["kf_flags"], np.uint8) & 1, prev_kf=np.full(nk, -1, np.int32),
                  poses7=np.tile(pc.IDENTITY7, (nk, 1)), covis_offsets=np.zeros(nk + 1, np.int32), covis=np.zeros(0, np.int32), slot_offsets=so,
                  slot_point=slot_point, points=points, point_flags=pr["point_bad"], point_nobs=g["point_nobs_out"], point_found=np.ones(npts, np.int32),
                  point_visible=np.ones(npts, np.int32), point_ref_kf=np.zeros(npts, np.int32), point_ref_level_scale=np.ones(npts, np.float32),
                  obs_offsets=g["obs_offsets_out"], obs_kf=g["obs_kf_out"], obs_index=g["obs_index_out"], current=cur, last_level_scale=pr["last_level_scale"])
        r = pkg.search_in_neighbors_batch([nb], env.cam4, env.bf, env.sf, env.isg, env.logsf, store=world["store"])[0]
        assert r["status"] == pkg.NEIGHBORS_ON_DEVICE and len(r["ops"]) == 0, c["name"]
        rows = g["associated_point"]
        assert np.array_equal(r["desc_kf"][rows], g["desc_kf"][rows]) and np.array_equal(r["desc_index"][rows], g["desc_index"][rows]), c["name"]
        checked += len(rows)
    assert checked > 100


def test_a_point_past_the_observation_limit_is_finished_by_the_host_twin(pkg, world):
    i, j = world["names"].index("limit"), world["names"].index("insert")
    lim = pkg.process_new_keyframe_limits()["observations"]
    got = device(pkg, world, [world["problems"][j], world["problems"][i]])
    assert got[0]["status"] == pkg.PROCESS_KEYFRAME_ON_DEVICE and got[1]["status"] == pkg.PROCESS_KEYFRAME_ON_HOST
    same(got[1], world["host"][i], "limit"); same(got[0], world["host"][j], "beside the limit")
    off = got[1]["obs_offsets_out"]
    assert (off[1:] - off[:-1]).max() == lim + 1
    # exactly at the limit the device computes it: the same point with one observer fewer
    g = pc.Graph(lim, seed=32)
    for kf in range(1, lim):
        g.kp(kf)
    g.kp(0)
    g.hold(0, g.pt(obs=[(kf, 0) for kf in range(1, lim)]))
    c = g.finish("at_the_limit")
    with pkg.KeyframeStore(lim, 8) as store:
        store.put_batch(np.arange(lim), c["views"], mc.BOUNDS0)
        at = pkg.process_new_keyframe_batch([c["problem"]], store=store)[0]
    assert at["status"] == pkg.PROCESS_KEYFRAME_ON_DEVICE and at["obs_offsets_out"][1] == lim
    same(at, pc.want_of(c), "at the limit")


def test_64_problems_in_one_call(pkg, world):
    idx = small(world)
    pick = [idx[k % len(idx)] for k in range(64)]
    got = device(pkg, world, [world["problems"][i] for i in pick])
    for i, g in zip(pick, got):
        same(g, world["host"][i], world["names"][i])
        assert g["status"] == pkg.PROCESS_KEYFRAME_ON_DEVICE


def test_capacity_and_invalid_on_the_device_entry(pkg, world):
    def run(cases, caps):
        problems = [world["problems"][world["names"].index(c["name"])] for c in cases]
        rc, outs, _, _ = run_raw(pkg, problems, None, caps, store=world["store"])
        return rc, outs
    check_capacity_contract(pkg, run)
    i = world["names"].index("insert")
    good = world["problems"][i]
    bads = invalid_problems(good, len(world["views"]), empty_slot=len(world["views"]))
    assert "slot_empty" in bads and len(bads) == 20
    for name, bad in bads.items():
        rc, outs, _, _ = run_raw(pkg, [good, bad], None, store=world["store"])
        assert rc == -2 and untouched(outs[0]) and untouched(outs[1]), name
