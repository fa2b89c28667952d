"""GPU tests of UpdateLocalMap for many sequences in one call: tc2li_local_map_update_batch and tc2li_local_map_set_graph_batch on the
cases of tests/localmap_batch_cases.py, against oracle.update_local_map and against tc2li_local_map_update on the same handles.  Equality
throughout; the contracts are those of tests/test_localmap_batch.py, run through the device entry."""
import numpy as np
import pytest

import localmap_batch_cases as K
import test_localmap_batch as host_tests

pytestmark = pytest.mark.gpu

SENTINEL = host_tests.SENTINEL


@pytest.fixture(scope="module")
def family(pkg, oracle):
    cases = K.all_cases(pkg.local_map_limits()["lds_keyframes"])
    return cases, [K.want_of(oracle, c) for c in cases]


@pytest.fixture(scope="module")
def mirrors(pkg, family):
    """one mirror per case (a call may name a map once), each with its case's graph; the tests that change a mirror make their own"""
    cases, _ = family
    maps = [pkg.LocalMap() for _ in cases]
    pkg.local_map_set_graph_batch(maps, [c["graph"] for c in cases])
    yield maps
    for m in maps:
        m.close()


def on(maps, cases):
    return [dict(c, map=m) for c, m in zip(cases, maps)]


def test_device_batch_in_every_order(pkg, family, mirrors):
    cases, want = family
    host_tests.check_orders(lambda ps: pkg.local_map_update_batch(ps), on(mirrors, cases), want)


def test_device_batch_equals_single_calls(pkg, family, mirrors):
    """the batch against tc2li_local_map_update on the same handles; a single call between two batch calls changes neither"""
    cases, want = family
    problems = on(mirrors, cases)
    before = pkg.local_map_update_batch(problems)
    for c, m, b in zip(cases, mirrors, before):
        kfs, ref, pts, cleared = m.update(c["frame_points"], c["temporal_last_kf"])
        assert np.array_equal(kfs, b["keyframes"]) and ref == b["reference_kf"] and np.array_equal(pts, b["points"]) and np.array_equal(cleared, b["cleared"]), c["name"]
    after = pkg.local_map_update_batch(problems)
    for c, a, b, w in zip(cases, after, before, want):
        K.same_results(a, b, c["name"] + " after the single calls")
        K.assert_equal(a, w, c["name"])


def test_device_state_does_not_leak(pkg, oracle):
    """frame A, then B, then A again on the same handles; set_graph to a smaller and to a larger graph between calls"""
    graphs = [K.random_graph(21, 50, 1200), K.random_graph(22, 90, 2500), K.chain_graph(200, 40)[0]]
    rng = np.random.default_rng(7)
    frames_a = [K.frame_points_near(rng, graphs[0], 10), K.frame_points_near(rng, graphs[1], 80), K.chain_graph(200, 40)[1]]
    frames_b = [K.frame_points_near(rng, graphs[0], 40), K.frame_points_near(rng, graphs[1], 5), K.chain_graph(200, 120)[1]]
    maps = [pkg.LocalMap() for _ in graphs]
    pkg.local_map_set_graph_batch(maps, graphs)

    def run(gs, frames, temporal):
        cases = [K.case("leak %d" % i, g, f, t) for i, (g, f, t) in enumerate(zip(gs, frames, temporal))]
        got = pkg.local_map_update_batch(on(maps, cases))
        for c, r in zip(cases, got):
            K.assert_equal(r, K.want_of(oracle, c), c["name"])
        return got

    a1 = run(graphs, frames_a, (-1, 20, 199))
    run(graphs, frames_b, (49, -1, 199))
    a2 = run(graphs, frames_a, (-1, 20, 199))
    for x, y in zip(a1, a2):
        K.same_results(x, y, "A again")
    # a smaller graph in mirror 1, a larger one in mirror 0, then back
    small, large = K.random_graph(23, 7, 60, 50), K.random_graph(24, 300, 5000, 120)
    maps[1].set_graph(small)
    maps[0].set_graph(large)
    rng = np.random.default_rng(8)
    run([large, small, graphs[2]], [K.frame_points_near(rng, large, 150), K.frame_points_near(rng, small, 3, 80), frames_b[2]], (299, 6, -1))
    pkg.local_map_set_graph_batch(maps[:2], graphs[:2])
    a3 = run(graphs, frames_a, (-1, 20, 199))
    for x, y in zip(a1, a3):
        K.same_results(x, y, "A after the graphs came back")
    for m in maps:
        m.close()


def test_device_512_small_problems(pkg, oracle):
    cases = K.many_small(512)
    maps = [pkg.LocalMap() for _ in cases]
    pkg.local_map_set_graph_batch(maps, [c["graph"] for c in cases])
    got = pkg.local_map_update_batch(on(maps, cases))
    sizes = set()
    for c, g in zip(cases, got):
        K.assert_equal(g, K.want_of(oracle, c), c["name"])
        sizes.add((g["n_keyframes"], g["n_points"]))
    assert len(sizes) > 5
    for m in maps:
        m.close()


def test_device_invalid_problems_are_refused(pkg):
    g, fp = K.chain_graph(20, 5)
    maps = [pkg.LocalMap(), pkg.LocalMap()]
    pkg.local_map_set_graph_batch(maps, [g, g])
    use = iter(maps * 100)
    host_tests.check_invalid_rules(pkg, lambda c: dict(c, map=next(use)), host=False)
    # the same map named by two problems
    arr, outs, keep = pkg.pack_local_map_problems([dict(K.case("a", g, fp), map=maps[0]), dict(K.case("b", g, fp), map=maps[1]),
                                                   dict(K.case("c", g, fp), map=maps[0])], fill=SENTINEL)
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.run_local_map_update_batch(arr, 3)
    assert e.value.code == -2 and "problem 2" in str(e.value) and "problem 0" in str(e.value), e.value
    assert host_tests.untouched(outs)
    # a map without a graph
    empty = pkg.LocalMap()
    arr, outs, keep = pkg.pack_local_map_problems([dict(K.case("a", g, fp), map=maps[0]), dict(K.case("b", g, fp), map=empty, keyframe_capacity=20, point_capacity=81)],
                                                  fill=SENTINEL)
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.run_local_map_update_batch(arr, 2)
    assert e.value.code == -2 and "problem 1" in str(e.value) and "no graph" in str(e.value), e.value
    assert host_tests.untouched(outs)
    assert pkg.run_local_map_update_batch(arr, 0) == 0
    for m in maps + [empty]:
        m.close()


def test_device_capacity_one_short(pkg, family, mirrors):
    cases, _ = family
    by_name = {c["name"]: m for c, m in zip(cases, mirrors)}
    host_tests.check_capacity(pkg, family, lambda c: dict(c, map=by_name[c["name"]]), host=False)


def test_device_counts_block(pkg, family, mirrors):
    cases, want = family
    arr, outs, keep = pkg.pack_local_map_problems(on(mirrors, cases)[:6], fill=SENTINEL)
    assert pkg.run_local_map_update_batch(arr, 6) == 6
    for o, w, (V, _, _, _, _) in zip(outs, want, K.CHAIN_TABLE):
        n_kf, n_pts = len(w["keyframes"]), len(w["points"])
        assert o["counts"].tolist() == [n_kf, V, 0, n_pts, 0, 0, 0, 0]
        assert (o["local_keyframes"][n_kf:] == SENTINEL).all() and (o["local_points"][n_pts:] == SENTINEL).all()


def test_set_graph_batch(pkg, oracle):
    """equal to per-map set_graph, judged by the updates that follow; an invalid graph in the middle leaves every mirror as it was; a map
    named twice is refused"""
    graphs = [K.random_graph(31, 40, 900), K.chain_graph(120, 39)[0], K.random_graph(32, 5, 50, 40)]
    rng = np.random.default_rng(9)
    frames = [K.frame_points_near(rng, graphs[0], 20), K.chain_graph(120, 39)[1], K.frame_points_near(rng, graphs[2], 2, 50)]
    cases = [K.case("graph %d" % i, g, f, t) for i, (g, f, t) in enumerate(zip(graphs, frames, (39, 119, -1)))]
    want = [K.want_of(oracle, c) for c in cases]
    one_by_one, at_once = [pkg.LocalMap() for _ in graphs], [pkg.LocalMap() for _ in graphs]
    for m, g in zip(one_by_one, graphs):
        m.set_graph(g)
    pkg.local_map_set_graph_batch(at_once, graphs)
    for maps in (one_by_one, at_once):
        for c, r, w in zip(cases, pkg.local_map_update_batch(on(maps, cases)), want):
            K.assert_equal(r, w, c["name"])
    for c, m, w in zip(cases, at_once, want):
        kfs, ref, pts, cleared = m.update(c["frame_points"], c["temporal_last_kf"])
        assert np.array_equal(kfs, w["keyframes"]) and ref == w["reference_kf"] and np.array_equal(pts, w["points"]), c["name"]
    # other graphs, the middle one invalid: refused with its number, and the mirrors still answer for the graphs they hold
    other = [K.random_graph(33, 12, 100), dict(graphs[1], obs_kf=graphs[1]["obs_kf"].copy()), K.random_graph(34, 9, 80, 60)]
    other[1]["obs_kf"][7] = 120
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.local_map_set_graph_batch(at_once, other)
    assert e.value.code == -2 and "map 1" in str(e.value) and "observations" in str(e.value), e.value
    assert [(m.n_keyframes, m.n_points) for m in at_once] == [(len(g["kf_bad"]), len(g["point_bad"])) for g in graphs]
    for c, r, w in zip(cases, pkg.local_map_update_batch(on(at_once, cases)), want):
        K.assert_equal(r, w, c["name"] + " after the refused call")
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.local_map_set_graph_batch([at_once[0], at_once[1], at_once[0]], graphs)
    assert e.value.code == -2 and "map 2" in str(e.value), e.value
    for c, r, w in zip(cases, pkg.local_map_update_batch(on(at_once, cases)), want):
        K.assert_equal(r, w, c["name"] + " after the map named twice")
    for m in one_by_one + at_once:
        m.close()
