"""CPU tests of LocalMapping::SearchInNeighbors in one call: tc2li_host_search_in_neighbors_batch against the Python restatement
(search_in_neighbors_ref.py) on every case of search_in_neighbors_cases.py -- all integer outputs exactly, the ops entry for entry; the
refreshed normals and distances to a few float32 roundings (the restatement is float32 in the same order, numpy's evaluation of it is
not promised to be the compiler's) -- and the contracts of the entry: every TC2LI_ERR_INVALID case with nothing written, TC2LI_ERR_CAPACITY
with the sizes needed and no list written, the repeat with those sizes, and the limits entry.  (The device entry: test_search_in_neighbors_gpu.py.)"""
import copy

import numpy as np
import pytest

import search_in_neighbors_cases as sc

INT_OUTPUTS = ("targets", "target_fused", "candidates", "slot_point_out", "point_bad_out", "point_replaced", "point_nobs_out", "point_found_out",
               "point_visible_out", "obs_offsets_out", "obs_kf_out", "obs_index_out", "desc_kf", "desc_index", "refreshed")
OP_FIELDS = ("kind", "stage_target", "point", "occupant", "winner", "kf", "idx")


@pytest.fixture(scope="module")
def env(synthetic):
    return sc.env_of(synthetic)


def ops_table(ops):
    return np.stack([ops[f] for f in OP_FIELDS], 1).astype(np.int32).reshape(-1, 7)


def check_integers(got, want, name):
    for k in INT_OUTPUTS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (name, k)
    assert np.array_equal(ops_table(got["ops"]), want["ops"]), (name, "ops")
    assert got["fused_current"] == want["fused_current"] and got["counts"]["fused_stage1"] == int(want["target_fused"].sum()), name
    assert got["counts"]["refreshed"] == int(want["refreshed"].sum()), name


def host_run(pkg, env, cases, **kw):
    """one host call per group of cases that share their views (a case brings its own keyframes)"""
    return [pkg.search_in_neighbors_batch([c["problem"]], env.cam4, env.bf, env.sf, env.isg, env.logsf, views=c["views"], bounds=c["bounds"], **kw)[0] for c in cases]


def all_cases(env):
    return sc.hand_made(env) + sc.random_cases(env) + [sc.the_limit_case(env), sc.the_many_candidates_case(env), sc.the_stale_winner_case(env)]


def test_host_twin_equals_the_reference(pkg, env):
    cases = all_cases(env)
    for c, got in zip(cases, host_run(pkg, env, cases)):
        want = sc.want_of(c, env)
        assert got["status"] == pkg.NEIGHBORS_ON_HOST
        check_integers(got, want, c["name"])
        on = want["refreshed"].astype(bool)
        # the sum of N unit vectors, each good to 4 roundings, divided by N; a distance times a scale: 4 roundings
        assert np.abs(got["normals_out"][on] - want["normals_out"][on]).max(initial=0) <= 8 * 2.0 ** -24, c["name"]
        for k in ("min_distance_out", "max_distance_out"):
            assert np.abs(got[k][on] / want[k][on] - 1).max(initial=0) <= 4 * 2.0 ** -24, (c["name"], k)
        assert not got["normals_out"][~on].any() and not got["max_distance_out"][~on].any(), c["name"]


def test_the_order_case_differs_from_the_entry_state_search(pkg, env):
    """Stage 1 searched with the entry-state descriptors gives target 2 the keypoint ka; the reference's order gives kb (asserted when the case is
    built); the host twin must give kb."""
    for c in sc.hand_made(env):
        if not c["name"].startswith("order_") or "abort" in c["name"]:
            continue
        got = host_run(pkg, env, [c])[0]
        op = ops_table(got["ops"])[1]
        assert op.tolist() == [pkg.NEIGHBORS_ADD_OBSERVATION, 1, c["p"], -1, -1, 2, c["kb"]] and c["kb"] != c["ka"], c["name"]
        so = c["problem"]["slot_offsets"]
        assert got["slot_point_out"][so[2] + c["kb"]] == c["p"] and got["slot_point_out"][so[2] + c["ka"]] == -1


def test_one_call_for_many_problems(pkg, env):
    """the problems of a batch are independent: the cases of one world in one call (their keyframes side by side in views) give what they give alone"""
    cases = sc.hand_made(env)[:6]
    views, problems, first = [], [], 0
    for c in cases:
        pr = dict(c["problem"])
        pr["kf_slot"] = (np.asarray(pr["kf_slot"]) + first).astype(np.int32)
        first += len(c["views"])
        views += c["views"]
        problems.append(pr)
    got = pkg.search_in_neighbors_batch(problems, env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=cases[0]["bounds"])
    for c, g in zip(cases, got):
        check_integers(g, sc.want_of(c, env), c["name"])


def test_limits(pkg):
    lim = pkg.search_in_neighbors_limits()
    assert lim == dict(observations=112, keypoints=3072, lds_points=16384, lds_keyframes=2048, threads=256)
    f = pkg.lib().tc2li_search_in_neighbors_limits
    assert f(None, 4) == -2
    two = np.full(3, -7, np.int32)
    assert f(two.ctypes.data, 2) == 5 and two.tolist() == [112, 3072, -7]


def broken(case, **changes):
    pr = copy.deepcopy(case["problem"])
    for k, v in changes.items():
        if callable(v):
            v(pr[k])
        else:
            pr[k] = v
    return pr


def invalid_problems(case, problem=None, empty_slot=None):
    """name -> problem: one broken table each.  problem: the case's problem on other slots (a store's); empty_slot: a slot in range that
    holds no keyframe (a store has such slots, a list of views has none)"""
    case = dict(case, problem=case["problem"] if problem is None else problem)
    pr = case["problem"]
    nk, npts = len(pr["kf_slot"]), len(pr["points"])

    def put(i, v):
        def f(a):
            a[i] = v
        return f
    out = {
        "current_out_of_range": broken(case, current=nk),
        "covis_offsets_descend": broken(case, covis_offsets=put(1, 99)),
        "covis_out_of_range": broken(case, covis=put(0, nk)),
        "prev_kf_out_of_range": broken(case, prev_kf=put(0, nk)),
        "slot_out_of_range": broken(case, kf_slot=put(1, 10 ** 6)),
        "slot_negative": broken(case, kf_slot=put(1, -1)),
        "slot_offsets_descend": broken(case, slot_offsets=put(3, 1)),
        "slot_point_out_of_range": broken(case, slot_point=put(0, npts)),
        "obs_offsets_descend": broken(case, obs_offsets=put(1, 99)),
        "obs_kf_out_of_range": broken(case, obs_kf=put(0, nk)),
        "obs_row_not_strict": broken(case, obs_kf=put(1, int(pr["obs_kf"][0]))),
        "obs_index_out_of_range": broken(case, obs_index=put(0, 999)),
        "ref_kf_out_of_range": broken(case, point_ref_kf=put(0, -1)),
        "last_level_scale": broken(case, last_level_scale=0.0),
    }
    chain = broken(case, inertial=True)
    chain["prev_kf"][:] = -1
    chain["prev_kf"][0], chain["prev_kf"][3], chain["prev_kf"][4] = 3, 4, 3     # 0 -> 3 -> 4 -> 3 ...: fewer than 20 targets, so the walk never ends
    out["prev_kf_chain_returns"] = chain
    if empty_slot is not None:
        out["slot_empty"] = broken(case, kf_slot=put(1, empty_slot))
    return out


def run_raw(pkg, env, problems, views, bounds, capacities=None, store=None):
    arr, outs, keep = pkg.pack_neighbors_problems(problems, capacities)
    rc = pkg.run_search_in_neighbors_batch(arr, len(problems), env.cam4, env.bf, env.sf, env.isg, env.logsf, store=store, views=None if store else views,
                                           bounds=bounds)
    return rc, outs, arr


def untouched(o):
    return (o["counts"] == 0).all() and (o["slot_point_out"] == -2).all() and (o["point_replaced"] == -2).all() and (o["desc_kf"] == -2).all() and \
        (o["targets"] == -1).all() and not o["ops"]["kind"].any()


def test_invalid_problems_are_refused_with_nothing_written(pkg, env):
    case = sc.hand_made(env)[0]   # order_identity: 5 keyframes, 2 points, observations [0, 3] and [1, 4]
    good = case["problem"]
    views = case["views"]
    for name, bad in invalid_problems(case).items():
        rc, outs, _ = run_raw(pkg, env, [good, bad], views, case["bounds"])
        assert rc == -2, name
        assert untouched(outs[0]) and untouched(outs[1]), name
    # a slot row that is not as long as the stored keypoint count
    short = copy.deepcopy(good)
    short["slot_offsets"] = short["slot_offsets"].copy()
    short["slot_offsets"][-1] -= 1
    short["slot_point"] = short["slot_point"][:-1]
    assert run_raw(pkg, env, [short], views, case["bounds"])[0] == -2
    # NULL tables, negative sizes, a list with a capacity and no array
    arr, outs, keep = pkg.pack_neighbors_problems([good])
    f = lambda: pkg.run_search_in_neighbors_batch(arr, 1, env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=case["bounds"])
    for field in ("kf_slot", "kf_flags", "prev_kf", "poses7", "covis_offsets", "slot_offsets", "slot_point", "points", "point_flags", "point_nobs", "obs_offsets",
                  "obs_kf", "counts", "ops", "targets", "obs_kf_out"):
        saved = getattr(arr[0], field)
        setattr(arr[0], field, None)
        assert f() == -2, field
        setattr(arr[0], field, saved)
    for field in ("n_keyframes", "n_points", "op_capacity", "obs_capacity"):
        saved = getattr(arr[0], field)
        setattr(arr[0], field, -1)
        assert f() == -2, field
        setattr(arr[0], field, saved)
    assert untouched(outs[0])
    assert f() == 1 and not untouched(outs[0])
    assert pkg.run_search_in_neighbors_batch(arr, -1, env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=case["bounds"]) == -2
    assert pkg.run_search_in_neighbors_batch(arr, 1, env.cam4, env.bf, env.sf, env.isg, 0.0, views=views, bounds=case["bounds"]) == -2
    assert pkg.run_search_in_neighbors_batch(arr, 0, env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=case["bounds"]) == 0
    del keep


CAPACITY_KEYS = ("targets", "candidates", "ops", "observations")


def test_capacity_reports_the_sizes_and_the_repeat_succeeds(pkg, env):
    """each list short in turn, in the second problem of a batch: counts for every problem, no list of any problem, then the repeat"""
    cases = [sc.hand_made(env)[1], sc.hand_made(env)[2]]   # direction and stage 2 of one world: targets, candidates, ops, observations all > 0
    views = cases[0]["views"] + cases[1]["views"]
    problems = [dict(cases[0]["problem"]), dict(cases[1]["problem"])]
    problems[1]["kf_slot"] = (np.asarray(problems[1]["kf_slot"]) + len(cases[0]["views"])).astype(np.int32)
    wants = [sc.want_of(c, env) for c in cases]
    need = [dict(targets=len(w["targets"]), candidates=len(w["candidates"]), ops=len(w["ops"]), observations=len(w["obs_kf_out"])) for w in wants]
    assert all(v > 0 for n in need for v in n.values())
    for short in CAPACITY_KEYS:
        caps = [dict(need[0]), dict(need[1], **{short: need[1][short] - 1})]
        rc, outs, _ = run_raw(pkg, env, problems, views, cases[0]["bounds"], caps)
        assert rc == -5, short
        for o, n in zip(outs, need):
            assert o["counts"][1:5].tolist() == [n[k] for k in CAPACITY_KEYS], short
            assert (o["slot_point_out"] == -2).all() and (o["targets"] == -1).all() and not o["ops"]["kind"].any() and (o["obs_kf_out"] == -1).all(), short
        again = [dict(zip(CAPACITY_KEYS, [int(v) for v in o["counts"][1:5]])) for o in outs]
        got = pkg.search_in_neighbors_batch(problems, env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=cases[0]["bounds"], capacities=again)
        for c, g in zip(cases, got):
            check_integers(g, sc.want_of(c, env), (short, c["name"]))
    # zero capacities with NULL arrays: the sizing call
    zero = [dict.fromkeys(CAPACITY_KEYS, 0)] * 2
    rc, outs, _ = run_raw(pkg, env, problems, views, cases[0]["bounds"], zero)
    assert rc == -5 and [o["counts"][1:5].tolist() for o in outs] == [[n[k] for k in CAPACITY_KEYS] for n in need]
    # and the default of the wrapper repeats by itself
    got = pkg.search_in_neighbors_batch(problems, env.cam4, env.bf, env.sf, env.isg, env.logsf, views=views, bounds=cases[0]["bounds"],
                                        capacities=None)
    check_integers(got[1], wants[1], "default capacities")
