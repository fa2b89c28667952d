"""GPU tests of LocalMapping::SearchInNeighbors in one call: tc2li_search_in_neighbors_batch against its host twin on every case of
search_in_neighbors_cases.py (integers exactly, floats bit for bit), the refreshed normals and distances against tc2li_map_points_refresh on
the final observation lists, 64 problems in four arrangements, one store slot in two problems with different poses, stage 1 of a
one-target problem against tc2li_fuse_search_batch, a stage-2 list longer than the piece the kernel searches at once, a point driven past the observation limit and a winner left outside its target (both finished by the host twin inside the call), and the INVALID cases on the device entry."""
import copy

import numpy as np
import pytest

import search_in_neighbors_cases as sc
import search_in_neighbors_ref as ref
from test_search_in_neighbors import INT_OUTPUTS, ops_table

pytestmark = pytest.mark.gpu
FLOAT_OUTPUTS = ("normals_out", "min_distance_out", "max_distance_out")


@pytest.fixture(scope="module")
def env(synthetic):
    return sc.env_of(synthetic)


@pytest.fixture(scope="module")
def world(pkg, env):
    """every case's keyframes in one store, every case's host result: (cases, store, views, problems on store slots, host results)"""
    cases = sc.hand_made(env) + sc.random_cases(env) + [sc.the_limit_case(env)]
    views, problems = [], []
    for c in cases:
        pr = dict(c["problem"])
        pr["kf_slot"] = (np.asarray(pr["kf_slot"]) + len(views)).astype(np.int32)
        views += c["views"]
        problems.append(pr)
    store = pkg.KeyframeStore(len(views) + 1, 128)
    store.put_batch(np.arange(len(views)), views, cases[0]["bounds"])
    host = pkg.search_in_neighbors_batch(problems, env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=cases[0]["bounds"])
    yield dict(cases=cases, store=store, views=views, problems=problems, host=host, bounds=cases[0]["bounds"])
    store.close()


def device(pkg, env, w, problems):
    return pkg.search_in_neighbors_batch(problems, env.cam4, env.bf, env.sf, env.isg, env.logsf, store=w["store"])


def same(got, want, name, status=True):
    for k in INT_OUTPUTS:
        assert np.array_equal(got[k], want[k]), (name, k)
    assert np.array_equal(ops_table(got["ops"]), ops_table(want["ops"])), (name, "ops")
    for k in FLOAT_OUTPUTS:
        assert np.array_equal(got[k].view(np.uint32), want[k].view(np.uint32)), (name, k)
    gc, wc = dict(got["counts"]), dict(want["counts"])
    if not status:
        gc.pop("status"); wc.pop("status")
    assert gc == wc, name


def test_device_equals_the_host_twin(pkg, env, world):
    got = device(pkg, env, world, world["problems"])
    for c, g, h in zip(world["cases"], got, world["host"]):
        same(g, h, c["name"], status=False)
        assert g["status"] == (pkg.NEIGHBORS_ON_HOST if c["name"] == "limit" else pkg.NEIGHBORS_ON_DEVICE), c["name"]
        want = sc.want_of(c, env)   # and so equals the Python restatement
        assert np.array_equal(ops_table(g["ops"]), want["ops"]) and np.array_equal(g["slot_point_out"], want["slot_point_out"]), c["name"]


def test_refresh_equals_map_points_refresh(pkg, env, world):
    """normals and distances of the refreshed points equal, bit for bit, tc2li_map_points_refresh on the final observation lists"""
    picked = [i for i, c in enumerate(world["cases"]) if c["name"] != "limit"]
    got = device(pkg, env, world, [world["problems"][i] for i in picked])
    for i, g in zip(picked, got):
        pr, c = world["problems"][i], world["cases"][i]
        rows = np.nonzero(g["refreshed"])[0]
        if not len(rows):
            continue
        centres = np.array([ref.centre_f32(p) for p in np.asarray(pr["poses7"], np.float32).reshape(-1, 7)], np.float32)
        off, okf, oidx = g["obs_offsets_out"], g["obs_kf_out"], g["obs_index_out"]
        sel = np.concatenate([np.arange(off[p], off[p + 1]) for p in rows])
        desc = np.array([c["views"][okf[o]]["descriptors"][oidx[o]] for o in sel], np.uint8)
        new_off = np.concatenate([[0], np.cumsum(off[rows + 1] - off[rows])]).astype(np.int32)
        best, normals, mn, mx = pkg.capi.map_points_refresh(new_off, desc, centres[okf[sel]], pr["points"]["pos"][rows], centres[pr["point_ref_kf"][rows]],
                                                            pr["point_ref_level_scale"][rows], pr["last_level_scale"])
        for a, b, k in ((g["normals_out"][rows], normals, "normal"), (g["min_distance_out"][rows], mn, "min"), (g["max_distance_out"][rows], mx, "max")):
            assert np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32)), (c["name"], k)
        # the descriptor choice too, where no observer is bad (map_points_refresh is handed the observations of keyframes that are not bad)
        if not (np.asarray(pr["kf_flags"]) & 1).any():
            assert np.array_equal(okf[off[rows] + best], g["desc_kf"][rows]) and np.array_equal(oidx[off[rows] + best], g["desc_index"][rows]), c["name"]


def test_arrangements_give_the_same_bits(pkg, env, world):
    """64 problems as one batch, one by one, shuffled, and with one problem repeated"""
    pool = [i for i, c in enumerate(world["cases"]) if c["name"] != "limit" and len(c["views"]) <= 14]
    idx = [pool[k % len(pool)] for k in range(64)]
    problems = [world["problems"][i] for i in idx]
    batch = device(pkg, env, world, problems)
    for k in range(64):   # one by one
        same(device(pkg, env, world, [problems[k]])[0], batch[k], ("alone", k))
    order = np.random.default_rng(5).permutation(64)
    for k, g in zip(order, device(pkg, env, world, [problems[k] for k in order])):
        same(g, batch[k], ("shuffled", int(k)))
    twice = device(pkg, env, world, problems + [problems[9]])
    for k, g in enumerate(twice):
        same(g, batch[k if k < 64 else 9], ("repeated", k))
    for i, g in zip(idx, batch):
        same(g, world["host"][i], world["cases"][i]["name"], status=False)


def test_one_slot_in_two_problems_with_different_poses(pkg, env, world):
    i = [c["name"] for c in world["cases"]].index("stage2_identity")
    a = world["problems"][i]
    b = copy.deepcopy(a)
    b["poses7"] = np.array(b["poses7"], np.float32)
    b["poses7"][1, 4] += np.float32(0.25)   # the target a quarter of a metre aside: its keypoints no longer lie where the points project
    got = device(pkg, env, world, [a, b, a])
    host = pkg.search_in_neighbors_batch([a, b], env.cam4, env.bf, env.sf, env.isg, env.logsf, views=world["views"], bounds=world["bounds"])
    same(got[0], host[0], "a", status=False); same(got[1], host[1], "b", status=False); same(got[2], host[0], "a again", status=False)
    # the pose counts: with the target aside, stage 1 no longer merges pa and qa there (stage 2 meets them in the current keyframe instead)
    assert not np.array_equal(ops_table(got[1]["ops"]), ops_table(got[0]["ops"])) and got[1]["counts"]["fused_stage1"] < got[0]["counts"]["fused_stage1"]


def test_stage_1_of_one_target_equals_fuse_search_batch(pkg, env, world):
    """pins the search body that moved into the shared header: a random graph cut to one target, with abort so that only stage 1 runs; the
    reference's walk over tc2li_fuse_search_batch's results for that target gives the ops the device entry gives"""
    for i, c in enumerate(world["cases"]):
        if not c["name"].startswith("random_"):
            continue
        pr = copy.deepcopy(world["problems"][i])
        co = np.asarray(pr["covis_offsets"])
        T = int(pr["covis"][co[0]])
        pr["covis"] = np.array([T], np.int32)
        pr["covis_offsets"] = np.concatenate([[0], np.ones(len(co) - 1)]).astype(np.int32)
        pr["abort"] = True
        pr["kf_flags"] = np.array(pr["kf_flags"], np.uint8) & 1
        pr["kf_flags"][T] = 0
        got = device(pkg, env, world, [pr])[0]
        assert got["targets"].tolist() == [T] and got["status"] == pkg.NEIGHBORS_ON_DEVICE
        so = pr["slot_offsets"]
        plist = pr["slot_point"][so[0]:so[1]]
        in_T = np.zeros(len(pr["points"]), bool)
        for p in range(len(pr["points"])):
            in_T[p] = T in pr["obs_kf"][pr["obs_offsets"][p]:pr["obs_offsets"][p + 1]]
        valid = np.array([p >= 0 and not (pr["point_flags"][p] & 1) and not in_T[p] for p in plist], np.uint8)
        pts = pr["points"][np.maximum(plist, 0)]
        item = dict(keyframe=int(pr["kf_slot"][T]), first_point=0, first_valid=0, n_points=len(plist), pose7=pr["poses7"][T], th=3.0)
        n_fused, best_idx, _ = pkg.fuse_search_batch(world["store"], [item], env.cam4, env.bf, env.sf, env.isg, env.logsf, pts, valid)
        assert n_fused[0] > 0
        found = {int(p): int(b) for p, b, v in zip(plist, best_idx, valid) if v}
        local = dict(pr, kf_slot=np.arange(len(c["views"]), dtype=np.int32))
        want = ref.search_in_neighbors(local, c["views"], c["bounds"], env, search=lambda kf, p: found[p])
        assert np.array_equal(ops_table(got["ops"]), want["ops"]) and len(want["ops"]) > 0, c["name"]
        assert got["target_fused"].tolist() == want["target_fused"].tolist() and np.array_equal(got["slot_point_out"], want["slot_point_out"]), c["name"]


def test_a_point_past_the_observation_limit_is_finished_by_the_host_twin(pkg, env, world):
    i = [c["name"] for c in world["cases"]].index("limit")
    lim = pkg.search_in_neighbors_limits()["observations"]
    got = device(pkg, env, world, [world["problems"][1], world["problems"][i]])
    assert got[0]["status"] == pkg.NEIGHBORS_ON_DEVICE and got[1]["status"] == pkg.NEIGHBORS_ON_HOST
    same(got[1], world["host"][i], "limit")
    same(got[0], world["host"][1], "beside the limit", status=False)
    off = got[1]["obs_offsets_out"]
    assert (off[1:] - off[:-1]).max() == lim + 1


def test_stage_2_list_longer_than_one_piece(pkg, env):
    """3 600 candidates: the device path searches and applies them in pieces of 3 072; ops of the second piece included, the results are the host twin's"""
    c = sc.the_many_candidates_case(env)
    assert len(sc.want_of(c, env)["candidates"]) > pkg.search_in_neighbors_limits()["keypoints"]
    args = ([c["problem"]], env.cam4, env.bf, env.sf, env.isg, env.logsf)
    host = pkg.search_in_neighbors_batch(*args, views=c["views"], bounds=c["bounds"])[0]
    with pkg.KeyframeStore(len(c["views"]), 512) as store:
        store.put_batch(np.arange(len(c["views"])), c["views"], c["bounds"])
        got = pkg.search_in_neighbors_batch(*args, store=store)[0]
    assert got["status"] == pkg.NEIGHBORS_ON_DEVICE
    same(got, host, c["name"], status=False)
    assert np.array_equal(ops_table(got["ops"]), sc.want_of(c, env)["ops"])


def test_capacity_and_invalid_on_the_device_entry(pkg, env, world):
    from test_search_in_neighbors import CAPACITY_KEYS, run_raw, untouched
    problems = [world["problems"][1], world["problems"][2]]
    need = [[int(world["host"][k]["counts"][n]) for n in ("targets", "candidates", "ops", "observations")] for k in (1, 2)]
    caps = [dict(zip(CAPACITY_KEYS, need[0])), dict(zip(CAPACITY_KEYS, need[1]), ops=need[1][2] - 1)]
    rc, outs, _ = run_raw(pkg, env, problems, None, None, caps, store=world["store"])
    assert rc == -5 and [o["counts"][1:5].tolist() for o in outs] == need
    assert all((o["slot_point_out"] == -2).all() and (o["targets"] == -1).all() and not o["ops"]["kind"].any() for o in outs)
    caps[1]["ops"] += 1
    rc, outs, _ = run_raw(pkg, env, problems, None, None, caps, store=world["store"])
    assert rc == 2 and np.array_equal(outs[1]["slot_point_out"], world["host"][2]["slot_point_out"])
    # every INVALID case of the host entry on the device entry too, the empty store slot among them: nothing written, no device work
    from test_search_in_neighbors import invalid_problems
    assert world["cases"][0]["name"] == "order_identity"
    bads = invalid_problems(world["cases"][0], problem=world["problems"][0], empty_slot=len(world["views"]))
    assert "slot_empty" in bads and "slot_offsets_descend" in bads
    for name, bad in bads.items():
        rc, outs, _ = run_raw(pkg, env, [problems[0], bad], None, None, None, store=world["store"])
        assert rc == -2 and untouched(outs[0]) and untouched(outs[1]), name


def test_a_winner_left_outside_the_target_goes_to_the_host_twin(pkg, env):
    """a slot that holds a point without the matching observation: the winner of a Replace stays outside the target with its entry still ahead,
    and the reference searches that entry with the new descriptor.  The device path notices and the host twin finishes the problem."""
    c = sc.the_stale_winner_case(env)
    args = ([c["problem"]], env.cam4, env.bf, env.sf, env.isg, env.logsf)
    host = pkg.search_in_neighbors_batch(*args, views=c["views"], bounds=c["bounds"])[0]
    with pkg.KeyframeStore(len(c["views"]), 16) as store:
        store.put_batch(np.arange(len(c["views"])), c["views"], c["bounds"])
        got = pkg.search_in_neighbors_batch(*args, store=store)[0]
    assert got["status"] == pkg.NEIGHBORS_ON_HOST
    same(got, host, c["name"])
    assert np.array_equal(ops_table(got["ops"]), sc.want_of(c, env)["ops"])
