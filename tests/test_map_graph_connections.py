"""CPU tests of the covisibility graph on the map graph: the host twins tc2li_host_map_graph_update_connections and
tc2li_host_map_graph_erase_connections against tests/connections_ref.py (its result written into the tables by
map_graph_connections_cases.updated) and against the restatement of KeyFrame::SetBadFlag's covisibility part there.  The problems are
those of tests/connections_cases.py turned into graph tables plus connection tables, and the directed cases.  Integers: equality.  No GPU
needed."""
import functools

import numpy as np
import pytest

import connections_cases as K
import connections_ref as ref
import map_graph_connections_cases as G


@functools.lru_cache(maxsize=None)
def cases_of(lds_keyframes):
    """-> [(name, graph, connections, current, init_kf_id, first_connection, counts wanted, connections wanted)], shared with the GPU tests"""
    out = []

    def add(name, pr, ordered=None):
        g, c, init = G.graph_of(pr, seed=len(out), ordered=ordered)
        counts, want = G.update_ref(g, c, pr["current"], pr["first_connection"], init)
        out.append((name, g, c, int(pr["current"]), init, int(pr["first_connection"]), counts, want))

    for i, pr in enumerate(K.family(lds_keyframes)):
        add("family %d" % i, pr)
    for seed in (3, 4):
        add("workload %d" % seed, K.workload(seed))
    kfs, points, slots = K.votes(6, 2, {0: 15, 1: 14, 3: 16, 4: 15, 5: 1})
    add("hand: the threshold", K.hand(kfs, points, slots, 2, first_connection=1))
    for name, pr, ordered, check in G.directed():
        assert check is None or check(ref.update_connections(pr)), name
        add(name, pr, ordered)
    return out


def cases(pkg):
    return cases_of(pkg.connections_limits()["lds_keyframes"])


def test_the_conversion_keeps_the_problem(pkg):
    """graph tables + connection tables stand for the problem they were made from: the restatement gives the same result on both"""
    for pr in K.family(pkg.connections_limits()["lds_keyframes"])[:12] + [p for _, p, _, _ in G.directed()]:
        g, c, init = G.graph_of(pr)
        back = G.problem_of(g, c, pr["current"], pr["first_connection"], init)
        K.assert_equal(ref.update_connections(back), ref.update_connections(pr))
        assert back["is_init_kf"] == pr["is_init_kf"]


def test_update_twin_equals_restatement(pkg):
    seen = set()
    for name, g, c, cur, init, first, counts, want in cases(pkg):
        got_counts, got = pkg.capi.host_map_graph_update_connections(g, c, cur, first, init)
        assert np.array_equal(got_counts, counts), (name, got_counts, counts)
        G.assert_same(got, want, name)
        seen.add(int(counts[0]))
    assert seen == {0, 1}


def test_update_twin_of_rows_appended_since(pkg):
    """connection tables that end before the graph's keyframe rows: the rows beyond are empty, and may be the current keyframe's"""
    kfs, points, slots = K.votes(6, 5, {0: 15, 4: 16})
    kfs[0]["conn"] = {1: 3}
    pr = K.hand(kfs, points, slots, 5, first_connection=1)
    g, c, init = G.graph_of(pr)
    short = dict(c, conn_offsets=c["conn_offsets"][:5], ord_offsets=c["ord_offsets"][:5])      # four rows: 4 and 5 were appended since
    assert short["conn_offsets"][-1] == len(c["conn_kf"])
    counts, want = G.update_ref(g, short, 5, 1, init)
    got_counts, got = pkg.capi.host_map_graph_update_connections(g, short, 5, 1, init)
    assert np.array_equal(got_counts, counts) and counts[5] == 4
    G.assert_same(got, want)
    assert len(got["conn_offsets"]) == 7 and np.diff(got["conn_offsets"]).tolist() == [2, 0, 0, 0, 1, 2]


def test_update_twin_five_in_a_row(pkg):
    """state to state: every keyframe of a small graph takes its turn as the current one"""
    pr = K.make_problem(77, 30, 0, 0)
    rng = np.random.default_rng(5)
    nk, npts = 30, 120
    obs = [np.sort(rng.choice(nk, rng.integers(2, 9), replace=False)) for _ in range(npts)]
    pr.update(obs_offsets=np.r_[0, np.cumsum([len(o) for o in obs])].astype(np.int32), obs_kf=np.concatenate(obs).astype(np.int32),
              point_bad=(rng.random(npts) < 0.05).astype(np.uint8), kf_flags=(rng.random(nk) < 0.1).astype(np.uint8))
    g, c, _ = G.graph_of(pr)
    # every keyframe holds the points that it observes
    held = [[p for p in range(npts) if k in obs[p]] for k in range(nk)]
    g["slot_offsets"] = np.r_[0, np.cumsum([len(h) for h in held])].astype(np.int32)
    g["slot_point"] = np.array([p for h in held for p in h], np.int32)
    for cur in (3, 9, 3, 17, 28):
        counts, want = G.update_ref(g, c, cur, 0, -1)
        got_counts, got = pkg.capi.host_map_graph_update_connections(g, c, cur, 0, -1)
        assert np.array_equal(got_counts, counts)
        G.assert_same(got, want, "current %d" % cur)
        c = want


def test_erase_twin_equals_restatement(pkg):
    for name, pr, row, ordered in G.erase_cases(pkg.map_graph_limits()["lds_row"]):
        g, c, _ = G.graph_of(pr, ordered=ordered, stale=0)
        want = G.erased(g, c, row)
        G.assert_same(pkg.capi.host_map_graph_erase_connections(g, c, row), want, name)
        w, o = G.rows_of(want)
        assert not w[row] and not o[row][0] and all(row not in x for x in w)
        if ordered:
            for k, v in ordered.items():
                assert o[k] == (list(v[0]), list(v[1])), name                          # it did not hold the entry: untouched
    # and on the generated graphs, every touched keyframe's row among them
    for name, g, c, cur, init, first, counts, want in cases(pkg)[:24]:
        row = int(np.argmax(np.diff(want["conn_offsets"])))
        G.assert_same(pkg.capi.host_map_graph_erase_connections(g, want, row), G.erased(g, want, row), name)


def test_twins_refuse(pkg):
    kfs, points, slots = K.votes(4, 0, {1: 15, 2: 3})
    g, c, init = G.graph_of(K.hand(kfs, points, slots, 0))
    E = pkg.capi.Tc2liError
    with pytest.raises(E) as e:                                                      # room for one weight entry short
        pkg.capi.host_map_graph_update_connections(g, c, 0, 0, -1, capacities=[2, 8])
    assert e.value.code == -5 and e.value.sizes.tolist() == [3, 2], (e.value.code, e.value.sizes)
    for bad in (dict(c, conn_offsets=np.array([0, 1, 1, 1, 1], np.int32), conn_kf=np.array([0], np.int32), conn_weight=np.array([1], np.int32)),   # its own keyframe
                dict(c, ord_offsets=np.array([0, 2, 2, 2, 2], np.int32), ord_kf=np.array([1, 1], np.int32), ord_weight=np.array([1, 1], np.int32)),   # twice
                dict(c, conn_offsets=np.array([0, 2, 2, 2, 2], np.int32), conn_kf=np.array([2, 1], np.int32), conn_weight=np.array([1, 1], np.int32)),   # descending
                dict(c, conn_offsets=np.array([0, 1, 1, 1, 1], np.int32), conn_kf=np.array([4], np.int32), conn_weight=np.array([1], np.int32))):   # out of range
        with pytest.raises(E) as e:
            pkg.capi.host_map_graph_erase_connections(g, bad, 0)
        assert e.value.code == -2
    with pytest.raises(E):
        pkg.capi.host_map_graph_update_connections(g, c, 4, 0, -1)
    with pytest.raises(E):                                                           # more rows than the graph has
        pkg.capi.host_map_graph_erase_connections(g, G.with_rows(c, 5), 0)
