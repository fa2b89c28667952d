"""CPU tests of UpdateLocalMap for many sequences in one call: tc2li_host_local_map_update_batch against oracle.update_local_map on the
cases of tests/localmap_batch_cases.py.  Every output is an integer list in the reference's order, so the criterion is equality.  The
contracts (refusals that write nothing, the capacity rule) are checked on outputs prefilled with a sentinel.  No GPU needed; the device
entry runs the same checks through tests/test_localmap_batch_gpu.py."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import localmap_batch_cases as K

SENTINEL = -77
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def family(pkg, oracle):
    cases = K.all_cases(pkg.local_map_limits()["lds_keyframes"])
    return cases, [K.want_of(oracle, c) for c in cases]


def run_host(pkg, cases):
    return pkg.host_local_map_update_batch(cases)


def check_orders(run, cases, want):
    """as one batch, one by one, shuffled, reversed: every problem's result is the oracle's each time"""
    n = len(cases)
    batch = run(cases)
    assert len(batch) == n
    for c, g, w in zip(cases, batch, want):
        K.assert_equal(g, w, c["name"] + " in the batch")
    for c, g in zip(cases, batch):
        K.same_results(run([c])[0], g, c["name"] + " alone")
    for name, order in (("shuffled", np.random.default_rng(5).permutation(n)), ("reversed", np.arange(n)[::-1])):
        got = run([cases[i] for i in order])
        for j, i in enumerate(order):
            K.same_results(got[j], batch[i], "%s, %s" % (cases[i]["name"], name))


def check_chain_table(family):
    cases, want = family
    for (V, temporal, bad_kf, n_kf, n_pts), w in zip(K.CHAIN_TABLE, want):
        assert (len(w["keyframes"]), len(w["points"])) == (n_kf, n_pts), (V, temporal, bad_kf)


def test_limits(pkg):
    lim = pkg.local_map_limits()
    assert lim["lds_keyframes"] >= 81 and lim["point_workgroups"] >= 1 and lim["threads"] % 64 == 0
    out = (pkg.capi.C.c_int32 * 2)()
    assert pkg.lib().tc2li_local_map_limits(out, 2) == -2


def test_cases_reach_the_rules(family):
    """The oracle alone: the chain reaches the limit of 80 keyframes with the sizes worked out by hand, the other cases reach what they are for."""
    cases, want = family
    check_chain_table(family)
    by_name = {c["name"]: w for c, w in zip(cases, want)}
    assert len(by_name["only -1 t=-1"]["keyframes"]) == 0 and by_name["only -1 t=-1"]["reference_kf"] == -1
    assert len(by_name["only -1 t=7"]["keyframes"]) == 8 and len(by_name["only -1 t=7"]["points"]) > 0      # the temporal block alone (a bad keyframe is pushed too)
    assert by_name["only bad points"]["cleared"].all() and len(by_name["only bad points"]["cleared"]) > 5
    assert len(by_name["no frame points"]["keyframes"]) == 4
    assert len(by_name["chain V=10 t=5"]["keyframes"]) == 21 and len(by_name["chain V=10 t=15"]["keyframes"]) == 26
    assert any(w["cleared"].any() and not w["cleared"].all() for w in want)
    assert max(len(w["points"]) for w in want) > 1500


def test_host_batch_in_every_order(pkg, family):
    cases, want = family
    check_orders(lambda cs: run_host(pkg, cs), cases, want)


def test_host_counts_block(pkg, family):
    cases, want = family
    arr, outs, keep = pkg.pack_local_map_problems(cases[:6], fill=SENTINEL)
    assert pkg.run_local_map_update_batch(arr, 6, host=True) == 6
    for o, w, (V, _, _, _, _) in zip(outs, want, K.CHAIN_TABLE):
        n_kf, n_pts = len(w["keyframes"]), len(w["points"])
        assert o["counts"].tolist() == [n_kf, V, 0, n_pts, 0, 0, 0, 0]
        assert (o["local_keyframes"][n_kf:] == SENTINEL).all() and (o["local_points"][n_pts:] == SENTINEL).all()     # beyond the counts: untouched
    assert pkg.run_local_map_update_batch(arr, 0, host=True) == 0


_BUDGET_CODE = """
import json, sys
sys.path.insert(0, %r)
import numpy as np
import localmap_batch_cases as K
pkg.capi.set_host_thread_budget(%d)
cases = K.all_cases(pkg.local_map_limits()["lds_keyframes"])
got = pkg.host_local_map_update_batch(cases)
print(json.dumps([[g["keyframes"].tolist(), g["reference_kf"], g["points"].tolist(), g["cleared"].tolist(), g["n_voted"]] for g in got]))
"""


@pytest.mark.parametrize("budget", [1, 16])
def test_host_thread_budgets(pkg, family, budget):
    """The budget is fixed before a process makes its first pool, so each one runs in a process of its own."""
    cases, want = family
    env = dict(os.environ)
    env.pop("TC2LI_HOST_THREAD_BUDGET", None)
    code = "import sys; sys.path.insert(0, %r)\nimport tc2li_loader\npkg = tc2li_loader.load()\n" % ROOT + _BUDGET_CODE % (os.path.join(ROOT, "tests"), budget)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    got = json.loads(r.stdout.strip().splitlines()[-1])
    here = run_host(pkg, cases)
    assert len(got) == len(want)
    for c, g, w, h in zip(cases, got, want, here):
        assert g[0] == w["keyframes"].tolist() and g[1] == w["reference_kf"] and g[2] == w["points"].tolist() and g[3] == w["cleared"].tolist(), c["name"]
        assert g[4] == h["n_voted"], c["name"]


def untouched(outs):
    return all((v == np.array(SENTINEL).astype(v.dtype)).all() for o in outs for v in o.values())


def check_invalid_rules(pkg, make, host):
    """make(case) -> the problem dict of the entry under test.  Every rule: TC2LI_ERR_INVALID with the problem's number, nothing written."""
    g, fp = K.chain_graph(20, 5)
    good = K.case("good", g, fp, 3)
    P, nK = len(g["point_bad"]), len(g["kf_bad"])

    def refused(change, word, number=1):
        problems = [make(good), make(good)]
        arr, outs, keep = pkg.pack_local_map_problems(problems, fill=SENTINEL)
        change(arr[1])
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.run_local_map_update_batch(arr, 2, host=host)
        assert e.value.code == -2 and "problem %d" % number in str(e.value) and word in str(e.value), e.value
        assert untouched(outs), word

    def setter(**fields):
        def change(a):
            for k, v in fields.items():
                setattr(a, k, v)
        return change

    refused(setter(counts=None), "counts")
    refused(setter(frame_points=None), "frame_points")
    refused(setter(frame_point_cleared=None), "frame_point_cleared")
    refused(setter(local_keyframes=None), "local_keyframes")
    refused(setter(local_points=None), "local_points")
    refused(setter(**{"graph" if host else "map": None}), "graph" if host else "map")
    refused(setter(n_frame_points=-1), "n_frame_points")
    refused(setter(keyframe_capacity=-1), "capacity")
    refused(setter(point_capacity=-3), "capacity")
    refused(setter(temporal_last_kf=-2), "temporal_last_kf")
    refused(setter(temporal_last_kf=nK), "temporal_last_kf")
    for bad_point in (-2, P):
        fp2 = fp.copy(); fp2[3] = bad_point
        refused(setter(frame_points=fp2.ctypes.data), "frame point")
    # the pointer to the array itself
    arr, outs, keep = pkg.pack_local_map_problems([make(good)], fill=SENTINEL)
    for f, args in ((pkg.lib().tc2li_host_local_map_update_batch, (None, 1)), (pkg.lib().tc2li_host_local_map_update_batch, (pkg.capi.C.addressof(arr), -1))):
        f.argtypes = [pkg.capi.C.c_void_p, pkg.capi.C.c_int]
        assert f(*args) == -2
    assert untouched(outs)


def test_host_invalid_problems_are_refused(pkg):
    check_invalid_rules(pkg, lambda c: c, host=True)
    # a graph that tc2li_local_map_set_graph would refuse
    g, fp = K.chain_graph(20, 5)
    broken = dict(g, children=g["children"].copy()); broken["children"][0] = 99
    arr, outs, keep = pkg.pack_local_map_problems([K.case("good", g, fp), K.case("broken", broken, fp)], fill=SENTINEL)
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.run_local_map_update_batch(arr, 2, host=True)
    assert e.value.code == -2 and "problem 1" in str(e.value) and "children" in str(e.value)
    assert untouched(outs)


def check_capacity(pkg, family, make, host):
    """one problem a single entry short: counts for ALL problems hold the sizes needed, no list is written, the retry at those sizes succeeds"""
    cases, want = family
    pick = [2, 14, 22, 5]      # a chain case, two random cases, the bad child
    sub, sub_want = [cases[i] for i in pick], [want[i] for i in pick]
    sizes = [(len(w["keyframes"]), len(w["points"])) for w in sub_want]
    assert all(nk > 1 and npts > 1 for nk, npts in sizes)
    for short, field in ((1, "keyframe_capacity"), (2, "point_capacity")):
        problems = [dict(make(c), keyframe_capacity=nk, point_capacity=npts) for c, (nk, npts) in zip(sub, sizes)]
        problems[short][field] -= 1
        arr, outs, keep = pkg.pack_local_map_problems(problems, fill=SENTINEL)
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.run_local_map_update_batch(arr, len(problems), host=host)
        assert e.value.code == -5 and "problem %d" % short in str(e.value), e.value
        for o, (nk, npts), w in zip(outs, sizes, sub_want):
            assert o["counts"][0] == nk and o["counts"][3] == npts and o["counts"][2] == w["reference_kf"]
            assert untouched([{k: v for k, v in o.items() if k != "counts"}])
        # the retry at the sizes the counts name
        retry = [dict(make(c), keyframe_capacity=int(o["counts"][0]), point_capacity=int(o["counts"][3])) for c, o in zip(sub, outs)]
        got = pkg.local_map_update_batch(retry, host=host)
        for c, r, w in zip(sub, got, sub_want):
            K.assert_equal(r, w, c["name"] + " at exactly its sizes")


def test_host_capacity_one_short(pkg, family):
    check_capacity(pkg, family, lambda c: c, host=True)
