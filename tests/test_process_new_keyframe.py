"""CPU tests of LocalMapping::ProcessNewKeyFrame in one call: tc2li_host_process_new_keyframe_batch against the Python restatement
(process_new_keyframe_ref.py) on every case of process_new_keyframe_cases.py -- integers exactly, floats bit for bit (the restatement is
float32 in the same order) -- the hand-made cases' literal lists, the connection half against tc2li_host_update_connections_batch fed with
the entry's own end state, and the contracts of the entry: every TC2LI_ERR_INVALID case with nothing written, TC2LI_ERR_CAPACITY with the
sizes needed and no list written, the repeat with those sizes, and the limits entry.  (The device entry: test_process_new_keyframe_gpu.py.)"""
import copy

import numpy as np
import pytest

import process_new_keyframe_cases as pc

INT_OUTPUTS = ("associated_slot", "associated_point", "recent", "point_nobs_out", "obs_offsets_out", "obs_kf_out", "obs_index_out", "desc_kf", "desc_index",
               "refreshed")
FLOAT_OUTPUTS = ("normals_out", "min_distance_out", "max_distance_out")
CONN_OUTPUTS = ("status", "parent", "counter_kf", "counter_weight", "ordered_kf", "ordered_weight", "touched_kf", "touched_changed", "changed_offsets",
                "changed_kf", "changed_weight")
CAPACITY_KEYS = ("associated", "recent", "observations", "counter", "ordered", "changed")


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(got, want, name):
    """every output of one problem: integers equal, floats as their bits, the connection half list by list"""
    for k in INT_OUTPUTS:
        assert np.array_equal(np.asarray(got[k]).astype(np.int64), np.asarray(want[k]).astype(np.int64)), (name, k)
    for k in FLOAT_OUTPUTS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (name, k)
    for k in CONN_OUTPUTS:
        assert np.array_equal(np.asarray(got["connections"][k]), np.asarray(want["connections"][k])), (name, "connections", k)


def host_run(pkg, cases, **kw):
    return [pkg.process_new_keyframe_batch([c["problem"]], views=c["views"], **kw)[0] for c in cases]


@pytest.fixture(scope="module")
def host(pkg):
    cases = pc.all_cases()
    return cases, host_run(pkg, cases)


def test_host_twin_equals_the_reference(pkg, host):
    for c, got in zip(*host):
        assert got["status"] == pkg.PROCESS_KEYFRAME_ON_HOST
        want = pc.want_of(c)
        same(got, want, c["name"])
        assert got["counts"] == dict(status=1, associated=len(want["associated_slot"]), recent=len(want["recent"]), observations=len(want["obs_kf_out"])), c["name"]
        off = ~got["refreshed"].astype(bool)
        assert (got["desc_kf"][off] == -1).all() and (got["desc_index"][off] == -1).all() and not got["normals_out"][off].any(), c["name"]


def check_expect(case, got):
    e, name = case["expect"], case["name"]
    for k in ("associated_slot", "associated_point", "recent"):
        if k in e:
            assert got[k].tolist() == e[k], (name, k)
    for p, rows in e.get("rows", {}).items():
        assert pc.rows_of(got, p) == rows, (name, "row", p)
        assert all(a[0] < b[0] for a, b in zip(rows, rows[1:]))
    for p, n in e.get("nobs", {}).items():
        assert got["point_nobs_out"][p] == n, (name, "nobs", p)
    for p, (kf, idx) in e.get("desc", {}).items():
        assert (int(got["desc_kf"][p]), int(got["desc_index"][p])) == (kf, idx), (name, "descriptor", p)
    for p, normal in e.get("normal", {}).items():
        assert np.array_equal(bits(got["normals_out"][p]), bits(normal)), (name, "normal", p)
    if "refreshed" in e:
        assert np.flatnonzero(got["refreshed"]).tolist() == sorted(e["refreshed"]), (name, "refreshed")
    for k, v in e.get("conn", {}).items():
        assert np.asarray(got["connections"][k]).tolist() == v, (name, "connections", k)


def test_the_literal_lists(host):
    """what each rule gives on the smallest graph that can get it wrong, written out by hand in the case"""
    names = []
    for c, got in zip(*host):
        if c["expect"]:
            check_expect(c, got)
            names.append(c["name"])
    assert {"order", "order_observed", "in", "skips", "insert", "nobs", "median_winner", "median_tie", "bad_observer", "first_observation", "threshold",
            "nobody_reaches_15", "only_nulls", "limit", "many_rows"} <= set(names)


def test_the_order_case_tells_slot_order_apart():
    """the association loop walked in another slot order (here: backwards) gives other lists than the case expects"""
    c = pc.order_case(False)
    pr = c["problem"]
    oo, okf = pr["obs_offsets"], pr["obs_kf"]

    def walk(slots):
        inside = {p for p in range(len(pr["point_bad"])) if pr["current"] in okf[oo[p]:oo[p + 1]]}
        associated, recent = [], []
        for i in slots:
            p = int(pr["slot_point"][i])
            if p < 0 or pr["point_bad"][p]:
                continue
            if p in inside:
                recent.append(i)
            else:
                associated.append(i)
                inside.add(p)
        return associated, recent
    n = len(pr["slot_point"])
    assert walk(range(n)) == ([3], [7]) and c["expect"]["associated_slot"] == [3] and c["expect"]["rows"][0][0] == (0, 3)
    assert walk(range(n - 1, -1, -1)) == ([7], [3])


def test_the_threshold_case_counts_the_points_associated_in_the_call():
    """keyframe 1 reaches 15 only with the points that gain their observation in the call: the points the current keyframe observes on entry
    give it fewer, and nobody would be connected by the threshold"""
    c = pc.threshold_case()
    pr = c["problem"]
    oo, okf = pr["obs_offsets"], pr["obs_kf"]
    on_entry = [p for p in pr["slot_point"] if pr["current"] in okf[oo[p]:oo[p + 1]]]
    votes = lambda pts, kf: sum(kf in okf[oo[p]:oo[p + 1]] for p in pts)
    assert votes(on_entry, 1) < 15 and votes(pr["slot_point"], 1) == 15 and votes(pr["slot_point"], 2) == 14
    assert pc.want_of(c)["connections"]["ordered_weight"].tolist() == [15]


def end_state_problem(pr, got):
    return dict({k: pr[k] for k in ("kf_flags", "conn_offsets", "conn_kf", "conn_weight", "slot_point", "point_bad", "current", "first_connection", "is_init_kf")},
                obs_offsets=got["obs_offsets_out"], obs_kf=got["obs_kf_out"])


def test_connections_equal_update_connections_on_the_end_state(pkg, host):
    cases, results = host
    want = pkg.update_connections_batch([end_state_problem(c["problem"], g) for c, g in zip(cases, results)], host=True)
    for c, g, w in zip(cases, results, want):
        for k in CONN_OUTPUTS:
            assert np.array_equal(g["connections"][k], w[k]), (c["name"], k)


def test_one_call_for_many_problems(pkg):
    """the problems of a batch are independent: all cases in one call, their keyframes side by side in views, give what they give alone"""
    cases = pc.all_cases()
    views, problems = pc.on_one_store(cases)
    for c, g in zip(cases, pkg.process_new_keyframe_batch(problems, views=views)):
        same(g, pc.want_of(c), c["name"])


def test_limits(pkg):
    assert pkg.process_new_keyframe_limits() == dict(observations=112, keypoints=3072, threads=256, refresh_waves=4)
    f = pkg.lib().tc2li_process_new_keyframe_limits
    assert f(None, 4) == -2
    two = np.full(3, -7, np.int32)
    assert f(two.ctypes.data, 2) == 4 and two.tolist() == [112, 3072, -7]


# ---- the contracts ---------------------------------------------------------------------------------------------------------------------------
def run_raw(pkg, problems, views, capacities=None, store=None):
    arr, outs, keep = pkg.pack_process_keyframe_problems(problems, capacities)
    rc = pkg.run_process_new_keyframe_batch(arr, len(problems), store=store, views=None if store is not None else views)
    return rc, outs, arr, keep


def untouched(o):
    return (o["counts"] == 0).all() and (o["conn_counts"] == -2).all() and all((o[k] == -2).all() for k in INT_OUTPUTS if k != "refreshed") and \
        not o["refreshed"].any() and (o["counter_kf"] == -2).all() and (o["ordered_kf"] == -2).all() and (o["changed_offsets"] == -2).all()


def lists_untouched(o):
    return all((o[k] == -2).all() for k in INT_OUTPUTS if k != "refreshed") and (o["counter_kf"] == -2).all() and (o["ordered_kf"] == -2).all() and \
        (o["changed_kf"] == -2).all() and (o["changed_offsets"] == -2).all()


def broken(pr, **changes):
    pr = copy.deepcopy(pr)
    for k, v in changes.items():
        if callable(v):
            pr[k] = np.array(pr[k]).copy()
            v(pr[k])
        else:
            pr[k] = v
    return pr


def put(i, v):
    def f(a):
        a.reshape(-1)[i] = v
    return f


def invalid_problems(pr, n_stored, empty_slot=None):
    """name -> problem: one broken table each, from the insert case's problem (5 keyframes, current row 2, three points with two observations
    each in slots 0, 6, 9).  n_stored: slots in range; empty_slot: a slot in range that holds no keyframe (a store has such slots)"""
    nk, npts = len(pr["kf_flags"]), len(pr["point_bad"])
    shorter = broken(pr)
    shorter["slot_point"] = shorter["slot_point"][:-1]
    out = {
        "current_out_of_range": broken(pr, current=nk),
        "conn_offsets_descend": broken(pr, conn_offsets=put(1, 99)),
        "obs_offsets_descend": broken(pr, obs_offsets=put(1, 99)),
        "obs_offsets_not_from_0": broken(pr, obs_offsets=put(0, 1)),
        "obs_kf_out_of_range": broken(pr, obs_kf=put(0, nk)),
        "obs_row_not_strict": broken(pr, obs_kf=put(1, int(pr["obs_kf"][0]))),
        "obs_index_out_of_range": broken(pr, obs_index=put(0, 10)),
        "obs_index_negative": broken(pr, obs_index=put(0, -1)),
        "slot_point_out_of_range": broken(pr, slot_point=put(0, npts)),
        "slot_point_below_minus_1": broken(pr, slot_point=put(1, -2)),
        "n_slots_not_the_stored_count": shorter,
        "current_without_slot": broken(pr, kf_slot=put(int(pr["current"]), -1)),
        "observer_without_slot": broken(pr, kf_slot=put(int(pr["obs_kf"][0]), -1)),
        "slot_out_of_range": broken(pr, kf_slot=put(0, n_stored + 10 ** 6)),
        "slot_below_minus_1": broken(pr, kf_slot=put(0, -2)),
        "ref_kf_out_of_range": broken(pr, point_ref_kf=put(0, nk)),
        "ref_kf_negative": broken(pr, point_ref_kf=put(1, -1)),
        "last_level_scale": broken(pr, last_level_scale=0.0),
    }
    conn = broken(pr)
    conn["conn_offsets"] = np.array([0, 2, 2, 2, 2, 2], np.int32)
    conn["conn_kf"], conn["conn_weight"] = np.array([3, 3], np.int32), np.array([1, 1], np.int32)
    out["conn_row_not_strict"] = conn
    if empty_slot is not None:
        out["slot_empty"] = broken(pr, kf_slot=put(0, empty_slot))
    return out


def test_invalid_problems_are_refused_with_nothing_written(pkg):
    case = pc.insert_case()
    good, views = case["problem"], case["views"]
    bads = invalid_problems(good, len(views))
    assert len(bads) == 19
    for name, bad in bads.items():
        rc, outs, _, _ = run_raw(pkg, [good, bad], views)
        assert rc == -2, name
        assert untouched(outs[0]) and untouched(outs[1]), name
    # an empty view where a slot is needed
    rc, outs, _, _ = run_raw(pkg, [good], views[:1] + [None] + views[2:])
    assert rc == -2 and untouched(outs[0])
    # a ref_kf out of range is no error for a point that cannot be associated: one that is in no slot, one that is bad, one that is observed already
    g = pc.Graph(2, seed=3)
    for kf in (0, 1):
        for _ in range(4):
            g.kp(kf)
    g.pt(obs=[(1, 0)], ref_kf=77)
    g.hold(0, g.pt(obs=[(1, 1)], ref_kf=77, bad=1))
    g.hold(1, g.pt(obs=[(0, 1), (1, 2)], ref_kf=-5))
    c = g.finish("ref_kf_unused")
    assert run_raw(pkg, [c["problem"]], c["views"])[0] == 1
    # NULL tables, negative sizes, a list with a capacity and no array
    arr, outs, keep = pkg.pack_process_keyframe_problems([good])
    f = lambda: pkg.run_process_new_keyframe_batch(arr, 1, views=views)
    for field in ("kf_slot", "centres", "positions", "point_nobs", "point_ref_kf", "point_ref_level_scale", "obs_index", "counts", "associated_slot",
                  "associated_point", "recent", "obs_kf_out", "obs_index_out"):
        saved = getattr(arr[0], field)
        setattr(arr[0], field, None)
        assert f() == -2, field
        setattr(arr[0], field, saved)
    for field in ("kf_flags", "conn_offsets", "slot_point", "point_bad", "obs_offsets", "obs_kf", "counts", "counter_kf", "ordered_kf", "touched_changed",
                  "changed_offsets"):
        saved = getattr(arr[0].conn, field)
        setattr(arr[0].conn, field, None)
        assert f() == -2, "conn." + field
        setattr(arr[0].conn, field, saved)
    for field in ("associated_capacity", "recent_capacity", "obs_capacity"):
        saved = getattr(arr[0], field)
        setattr(arr[0], field, -1)
        assert f() == -2, field
        setattr(arr[0], field, saved)
    for field in ("n_keyframes", "n_points", "n_slots", "counter_capacity"):
        saved = getattr(arr[0].conn, field)
        setattr(arr[0].conn, field, -1)
        assert f() == -2, "conn." + field
        setattr(arr[0].conn, field, saved)
    assert untouched(outs[0])
    assert f() == 1 and not untouched(outs[0])
    assert pkg.run_process_new_keyframe_batch(arr, -1, views=views) == -2
    assert pkg.run_process_new_keyframe_batch(arr, 0, views=views) == 0
    del keep


def needs_of(want):
    k = want["connections"]
    return dict(associated=len(want["associated_slot"]), recent=len(want["recent"]), observations=len(want["obs_kf_out"]), counter=len(k["counter_kf"]),
                ordered=len(k["ordered_kf"]), changed=len(k["changed_kf"]))


def reported(o):
    return dict(zip(CAPACITY_KEYS, [int(o["counts"][1]), int(o["counts"][2]), int(o["counts"][3]), int(o["conn_counts"][1]), int(o["conn_counts"][2]),
                                    int(o["conn_counts"][4])]))


def capacity_cases():
    """two random graphs in which every list has entries"""
    cases = [c for c in pc.random_cases() if all(v > 0 for v in needs_of(pc.want_of(c)).values())][:2]
    assert len(cases) == 2
    return cases


def check_capacity_contract(pkg, run):
    """run(cases, capacities) -> (rc, outs).  Each list short in turn, in the second problem of a batch: counts for every problem, no list
    of any problem, then the repeat with the sizes reported.  The connection half keeps tc2li_connections_problem's own rule: the size of
    the changed lists is reported once counter and ordered fit, and is 0 until then, so those two take one more round."""
    cases = capacity_cases()
    need = [needs_of(pc.want_of(c)) for c in cases]
    for short in CAPACITY_KEYS:
        caps = [dict(need[0]), dict(need[1], **{short: need[1][short] - 1})]
        rc, outs = run(cases, caps)
        assert rc == -5, short
        two_rounds = short in ("counter", "ordered")
        for k, (o, n) in enumerate(zip(outs, need)):
            assert reported(o) == (dict(n, changed=0) if two_rounds and k == 1 else n), (short, k)
            assert lists_untouched(o), (short, k)
        rc, outs = run(cases, [reported(o) for o in outs])
        if two_rounds:
            assert rc == -5 and [reported(o) for o in outs] == need and all(lists_untouched(o) for o in outs), short
            rc, outs = run(cases, [reported(o) for o in outs])
        assert rc == 2 and not any(lists_untouched(o) for o in outs), short
    zero = [dict(n, associated=0, recent=0, observations=0) for n in need]
    rc, outs = run(cases, zero)   # zero capacities with NULL arrays: the sizing call
    assert rc == -5 and [reported(o) for o in outs] == need


def test_capacity_reports_the_sizes_and_the_repeat_succeeds(pkg):
    def run(cases, caps):
        views, problems = pc.on_one_store(cases)
        rc, outs, _, _ = run_raw(pkg, problems, views, caps)
        return rc, outs
    check_capacity_contract(pkg, run)
    cases = capacity_cases()
    need = [needs_of(pc.want_of(c)) for c in cases]
    views, problems = pc.on_one_store(cases)
    for c, g in zip(cases, pkg.process_new_keyframe_batch(problems, views=views, capacities=need)):   # exactly the sizes needed
        same(g, pc.want_of(c), c["name"])
