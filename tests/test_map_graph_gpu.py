"""GPU tests of the resident map graph: set / download, tc2li_map_graph_apply_batch against the host twin and the restatement
tests/map_graph_ref.py on the logs of tests/test_map_graph.py, the bytes an apply and a graph-reading gather put on the bus, and
tc2li_ba_window_graph_batch / tc2li_ba_window_solve_graph_batch against the entries that take host arrays, given the downloaded tables.
Everything is an integer or a double carried through, and the graph entries run the same kernels on the same layout: the criterion is
equality of every array."""
import numpy as np
import pytest

import ba_window_cases as K
import ba_window_ref as wref
import map_graph_cases as M
import map_graph_ref as ref
import test_ba_window as TW
import test_ba_window_solve_gpu as S
import test_map_graph as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def store(pkg):
    """the world of ba_window_cases.py resident on the device; slot EMPTY_SLOT stays empty"""
    with pkg.KeyframeStore(K.WORLD_SLOTS, 64) as s:
        slots = [i for i, v in enumerate(K.WORLD) if v is not None]
        s.put_batch(slots, [K.WORLD[i] for i in slots], K.BOUNDS, n_levels=K.N_LEVELS)
        yield s


def rows(e):
    return e.view(np.int32).reshape(-1, 4)


def room_for(cases):
    return np.max([M.capacities_for(g, e) for _, g, (e, _), _ in cases], 0).astype(np.int32)


def test_set_then_download_and_set_again(pkg, store):
    cases = T.cases_of(pkg)
    with pkg.ResidentMapGraph(store, len(cases), room_for(cases)) as graph:
        assert graph.info(0)["applies"] == -1
        graph.set_batch(range(len(cases)), [g for _, g, _, _ in cases])
        for s, (name, g, _, _) in enumerate(cases):
            ref.assert_same_tables(graph.download(s, fill=T.SENTINEL), ref.tables_of(g), name)
            assert graph.info(s)["applies"] == 0
        order = np.roll(np.arange(len(cases)), 7)                                      # every sequence gets another graph
        graph.set_batch(order[::2], [cases[(s + 3) % len(cases)][1] for s in order[::2]])
        for s in range(len(cases)):
            ref.assert_same_tables(graph.download(s, fill=T.SENTINEL), ref.tables_of(cases[(s + 3) % len(cases) if s in order[::2] else s][1]), "set again, %d" % s)


def test_apply_equals_twin_and_restatement(pkg, store):
    """every random and directed log, one sequence each, in ONE apply_batch; the bytes of the apply are exactly record + edits + values"""
    cases, lim = T.cases_of(pkg), pkg.map_graph_limits()
    caps = room_for(cases)
    with pkg.ResidentMapGraph(store, len(cases), caps) as graph:
        graph.set_batch(range(len(cases)), [g for _, g, _, _ in cases])
        graph.apply_batch([(s, e, v) for s, (_, _, (e, v), _) in enumerate(cases)])
        for s, (name, g, (e, v), want) in enumerate(cases):
            got = graph.download(s, fill=T.SENTINEL)
            ref.assert_same_tables(got, want, name + ": device against the restatement")
            ref.assert_same_tables(got, pkg.host_map_graph_apply(g, e, v, caps), name + ": device against the twin")
            info = graph.info(s)
            assert info["apply_bytes"] == 16 * len(e) + 8 * len(v) + lim["apply_record_bytes"] <= 16 * len(e) + 8 * len(v) + 64, name
            assert (info["applies"], info["n_observations"], info["n_keyframes"], info["n_points"], info["n_slots"]) == \
                (1, len(want["obs_kf"]), len(want["kf_slot"]), len(want["point_flags"]), len(want["slot_point"])), name


def test_five_applies_in_a_row(pkg, store):
    """the two generations of the observation CSR each written and read more than once"""
    g = K.make_graph(620, 10, 200)
    caps = np.array([40, 4000, 400, 4000], np.int32)
    with pkg.ResidentMapGraph(store, 3, caps) as graph:
        graph.set_batch([1], [g])
        now = ref.tables_of(g)
        for i in range(5):
            e, v = M.random_log(630 + i, now, 150)
            graph.apply_batch([(1, e, v)])
            want = ref.apply(now, rows(e), v, caps, M.N_KEYS)
            got = graph.download(1, fill=T.SENTINEL)
            ref.assert_same_tables(got, want, "apply %d: restatement" % i)
            ref.assert_same_tables(got, pkg.host_map_graph_apply(now, e, v, caps), "apply %d: twin" % i)
            assert graph.info(1)["applies"] == i + 1
            now = want


def test_512_sequences_beside_512_left_alone(pkg, store):
    g = K.make_graph(640, 4, 24)
    caps = np.array([8, 200, 40, 200], np.int32)
    with pkg.ResidentMapGraph(store, 1024, caps) as graph:
        graph.set_batch(range(1024), [g] * 1024)
        logs = [M.random_log(1000 + s, g, 20 + s % 30) for s in range(512)]
        graph.apply_batch([(2 * s, e, v) for s, (e, v) in enumerate(logs)])
        same = ref.tables_of(g)
        for s, (e, v) in enumerate(logs):
            ref.assert_same_tables(graph.download(2 * s, fill=T.SENTINEL), ref.apply(g, rows(e), v, caps, M.N_KEYS), "sequence %d" % (2 * s))
            ref.assert_same_tables(graph.download(2 * s + 1, fill=T.SENTINEL), same, "sequence %d, left alone" % (2 * s + 1))


def sound_log(g):
    L = M.Log(g)
    L.set_pose(1, range(7)); L.set_slot(2, 0, 5); L.erase_observation(0, 2)
    return L.done()


def test_refused_calls_leave_the_graph_unchanged(pkg, store):
    g = M.wide_graph(n_kf=12)
    for what, _, build, room, code in T.refused_logs() + store_refusals():
        with pkg.ResidentMapGraph(store, 2, room) as graph:
            graph.set_batch([0, 1], [g, g])
            L = M.Log(g)
            build(L)
            e, v = L.done()
            ok = sound_log(g)
            with pytest.raises(pkg.Tc2liError) as r:
                graph.apply_batch([(1, ok[0], ok[1]), (0, e, v)])                      # the sound log of the same call is not applied either
            assert r.value.code == code, what
            for s in (0, 1):
                ref.assert_same_tables(graph.download(s), ref.tables_of(g), what)
                assert graph.info(s)["applies"] == 0
    with pkg.ResidentMapGraph(store, 2, [12, 48, 12, 40]) as graph:
        graph.set_batch([0], [g])
        ok = sound_log(g)
        for deltas in ([(0, ok[0], ok[1]), (0, ok[0], ok[1])], [(1, ok[0], ok[1])], [(2, ok[0], ok[1])]):   # named twice, never set, out of range
            with pytest.raises(pkg.Tc2liError) as r:
                graph.apply_batch(deltas)
            assert r.value.code == T.INVALID
        bad = dict(g, obs_kf=g["obs_kf"][::-1].copy())                                 # rows no longer ascending
        with pytest.raises(pkg.Tc2liError) as r:
            graph.set_batch([1, 0], [g, bad])
        assert r.value.code == T.INVALID and graph.info(1)["applies"] == -1
        with pytest.raises(pkg.Tc2liError) as r:
            graph.set_batch([1], [M.wide_graph(n_kf=13)])
        assert r.value.code == T.CAPACITY
        ref.assert_same_tables(graph.download(0), ref.tables_of(g), "after refused sets")


def store_refusals():
    """what only the device entry can refuse: it knows the store"""
    g = M.wide_graph(n_kf=12)
    room = np.array([14, 56, 14, 40], np.int32)
    pose = (0, 0, 0, 1, 0, 0, 0)
    slot_of_row_3 = int(g["kf_slot"][3])
    return [("an empty store slot", g, lambda L: L.add_keyframe(K.EMPTY_SLOT, 1, 9, 0, pose), room, T.INVALID),
            ("a store slot out of range", g, lambda L: L.add_keyframe(K.WORLD_SLOTS, 1, 9, 0, pose), room, T.INVALID),
            ("an index at the keypoints of the observer's slot", g, lambda L: L.add_observation(0, 3, M.N_KEYS[slot_of_row_3]), room, T.INVALID),
            ("an index at the keypoints of a new row's slot", g, lambda L: L.add_observation(0, L.add_keyframe(1, 1, 9, 0, pose), M.N_KEYS[1]), room, T.INVALID)]


# ---- the gather ------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def edited_family(pkg, store):
    """The graphs of ba_window_cases.family, each in a sequence of its own and after a random log: (graph, problems with the downloaded
    tables, what the restatement gathers from them)."""
    problems, _ = TW.family_of(pkg)
    logs = [M.random_log(1100 + i, p, 120) for i, p in enumerate(problems)]
    caps = np.max([M.capacities_for(p, e) for p, (e, _) in zip(problems, logs)], 0).astype(np.int32)
    with pkg.ResidentMapGraph(store, len(problems), caps) as graph:
        graph.set_batch(range(len(problems)), problems)
        graph.apply_batch([(s, e, v) for s, (e, v) in enumerate(logs)])
        now = [dict(graph.download(s), current=p["current"], cov_kf=p["cov_kf"], init_kf_id=p["init_kf_id"]) for s, p in enumerate(problems)]
        for s, (p, (e, v)) in enumerate(zip(problems, logs)):
            ref.assert_same_tables(now[s], ref.apply(p, rows(e), v, caps, M.N_KEYS), "family %d" % s)
        yield graph, now, [wref.gather(p, K.WORLD, K.SIGMA) for p in now]


def gather_bytes(pkg, problems):
    """what a graph-reading gather uploads: the problem records, the level table, cov_kf -- and nothing else"""
    return len(problems) * pkg.map_graph_limits()["gather_record_bytes"] + 4 * len(K.SIGMA) + 4 * sum(len(p["cov_kf"]) for p in problems)


def test_gather_from_the_graph(pkg, store, edited_family):
    graph, now, want = edited_family
    seq = np.arange(len(now))
    from_arrays = pkg.ba_window_batch(now, K.SIGMA, store=store)
    from_graph = pkg.ba_window_graph_batch(now, seq, K.SIGMA, store, graph)
    for i, (a, b, w) in enumerate(zip(from_graph, from_arrays, want)):
        K.assert_equal(a, b, "problem %d: the graph against host arrays" % i)
        K.assert_equal(a, w, "problem %d: the graph against the restatement" % i)
    assert sum(w["status"] == wref.ABORTED for w in want) >= 5 and sum(w["status"] == wref.OK for w in want) >= 20
    lim = pkg.ba_window_limits()
    assert len({(len(p["kf_slot"]) > lim["lds_keyframes"], len(p["point_flags"]) > lim["lds_points"]) for p in now}) == 4
    assert all(graph.info(int(s))["gather_bytes"] == gather_bytes(pkg, now) for s in seq)
    table_bytes = sum(sum(np.asarray(p[k]).nbytes for k, _ in ref.TABLES) for p in now)
    assert gather_bytes(pkg, now) * 20 < table_bytes                                   # no table crossed the bus
    order = np.random.default_rng(5).permutation(len(now))
    shuffled = pkg.ba_window_graph_batch([now[i] for i in order], order, K.SIGMA, store, graph)
    for k, i in enumerate(order):
        K.assert_equal(shuffled[k], from_arrays[i], "problem %d in the shuffled batch" % i)
    one = pkg.ba_window_graph_batch([now[3]], [3], K.SIGMA, store, graph)
    K.assert_equal(one[0], from_arrays[3], "a batch of one")
    assert graph.info(3)["gather_bytes"] == gather_bytes(pkg, [now[3]]) and graph.info(4)["gather_bytes"] == gather_bytes(pkg, now)


def windows_of_one_sequence(base, n):
    """n problems on one graph: the current keyframe moves on by one row each, all other rows are its neighbours (but for the last i % 3)"""
    n_kf = len(base["kf_slot"])
    out = []
    for i in range(n):
        cur = (base["current"] + i) % n_kf
        out.append(dict(base, current=cur, cov_kf=np.array([k for k in np.roll(np.arange(n_kf), i) if k != cur][:n_kf - 1 - i % 3], np.int32)))
    return out


@pytest.mark.parametrize("n", [2, 8])
def test_problems_of_one_sequence(pkg, store, edited_family, n):
    graph, now, _ = edited_family
    for s, base in enumerate(now):                                                     # the first graph on which most of the n windows are alive and all of those differ
        if not 8 <= len(base["kf_slot"]) <= 12:
            continue
        problems = windows_of_one_sequence(base, n)
        want = [wref.gather(p, K.WORLD, K.SIGMA) for p in problems]
        alive = [w for w in want if w["status"] == wref.OK]
        if len(alive) > n // 2 and len({bytes(w["pose_row"]) + bytes(w["point_row"]) for w in alive}) == len(alive):
            break
    else:
        raise AssertionError("no graph of the family gives %d different windows" % n)
    got = pkg.ba_window_graph_batch(problems, [s] * n, K.SIGMA, store, graph)
    from_arrays = pkg.ba_window_batch(problems, K.SIGMA, store=store)
    for i, (a, b, w) in enumerate(zip(got, from_arrays, want)):
        K.assert_equal(a, b, "problem %d of sequence %d" % (i, s))
        K.assert_equal(a, w, "problem %d of sequence %d, restatement" % (i, s))


def test_gather_capacity_and_contracts(pkg, store, edited_family):
    graph, now, want = edited_family
    pick = [i for i, w in enumerate(want) if w["status"] == wref.OK][:3]
    batch = [dict(now[i]) for i in pick]
    batch[1]["point_capacity"] = len(want[pick[1]]["point_row"]) - 1
    outs = []
    for run in (lambda **kw: pkg.ba_window_graph_batch(batch, pick, K.SIGMA, store, graph, **kw), lambda **kw: pkg.ba_window_batch(batch, K.SIGMA, store=store, **kw)):
        import tc2li_slam_amd.capi as capi
        seen, real = {}, capi.pack_ba_window_problems

        def spy(problems_, fill=0):
            seen["packed"] = real(problems_, fill)
            return seen["packed"]
        capi.pack_ba_window_problems = spy
        try:
            with pytest.raises(pkg.Tc2liError) as e:
                run(fill=T.SENTINEL)
        finally:
            capi.pack_ba_window_problems = real
        assert e.value.code == T.CAPACITY
        outs.append(seen["packed"][1])
    for a, b, i in zip(outs[0], outs[1], pick):
        assert a["counts"].tolist() == b["counts"].tolist() and a["counts"][4] == len(want[i]["point_row"])
        for k in ("pose_row", "point_row", "lidar_pose_index"):
            assert (a[k] == T.SENTINEL).all() and (b[k] == T.SENTINEL).all(), k          # counts for every problem, no list for any
    for bad in (dict(now[0], current=len(now[0]["kf_slot"])), dict(now[0], cov_kf=np.array([now[0]["current"]], np.int32))):
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.ba_window_graph_batch([bad], [0], K.SIGMA, store, graph)
        assert e.value.code == T.INVALID
    with pytest.raises(pkg.Tc2liError) as e:                                           # a sequence out of range
        pkg.ba_window_graph_batch([now[0]], [len(now)], K.SIGMA, store, graph)
    assert e.value.code == T.INVALID
    with pytest.raises(pkg.Tc2liError) as e:                                           # the slots hold higher octaves than this table has
        pkg.ba_window_graph_batch([now[0]], [0], K.SIGMA[:1], store, graph)
    assert e.value.code == T.INVALID
    assert pkg.ba_window_graph_batch([], [], K.SIGMA, store, graph) == []


# ---- the solve -------------------------------------------------------------------------------------------------------------------------
def same_solve(a, b, what):
    """two results of the solve entries: bytes"""
    assert a["result"] == b["result"] and a["status"] == b["status"], (what, a["result"], b["result"])
    for k in ("num_fixed_kf", "num_opt_kf", "n_lidar", "n_points_without_edge", "n_erase"):
        assert a[k] == b[k], (what, k)
    for k in ("pose_row", "fixed", "point_row", "lidar_pose_index", "poses7", "points3", "edges", "chi2", "depth_positive", "erase"):
        assert (a[k] is None) == (b[k] is None) and (a[k] is None or S.bits(a[k]) == S.bits(b[k])), (what, k)
    for k in ("stats", "lidar_stats"):
        assert bytes(a[k]) == bytes(b[k]), (what, k)


def test_solve_from_the_graph(pkg, synthetic):
    """the smallest two visual windows, a LiDAR window and one beyond the device range (finished on the host path), bit for bit"""
    w = S.World(pkg, synthetic)
    size = lambda i: len(w.problems[i]["point_flags"])
    visual = sorted((i for i, p in enumerate(w.problems) if p.get("clouds") is None), key=size)[:2]
    lidar = min((i for i, p in enumerate(w.problems) if p.get("clouds") is not None), key=size)
    problems = [w.problems[visual[0]], w.problems[visual[1]], w.problems[lidar], w.wide]
    caps = np.max([M.capacities_for(p, np.zeros(0, M.EDIT_DTYPE)) for p in problems], 0).astype(np.int32)
    with w.store(pkg) as s, pkg.ResidentMapGraph(s, len(problems) + 1, caps) as graph:
        seq = [3, 0, 4, 1]
        graph.set_batch(seq, problems)
        want = S.solve(pkg, s, w, problems)
        got = pkg.ba_window_solve_graph_batch(problems, seq, w.sigma, s, graph, w.cam, group=S.GROUP)
        for i, (a, b) in enumerate(zip(got, want)):
            same_solve(a, b, "window %d" % i)
        assert all(b["result"] > 0 for b in want) and want[2]["n_lidar"] >= 3 and want[2]["lidar_stats"].n_planes > 0
        assert want[3]["stats"].n_free_poses == 30                                     # beyond tc2li_ba_window_solve_limits: the host path
        records = len(problems) * pkg.map_graph_limits()["gather_record_bytes"] + 4 * len(w.sigma) + 4 * sum(len(p["cov_kf"]) for p in problems)
        assert all(graph.info(q)["gather_bytes"] == records for q in seq)
        # after an edit the solve reads the edited graph: a pose moved by the log moves the result as it does through host arrays
        L = M.Log(problems[0])
        L.set_pose(int(problems[0]["current"]), problems[0]["poses7"][int(problems[0]["current"])] + np.array([0, 0, 0, 0, 0.01, 0, 0]))
        e, v = L.done()
        graph.apply_batch([(3, e, v)])
        moved = dict(problems[0], **graph.download(3))
        same_solve(pkg.ba_window_solve_graph_batch([moved, problems[1]], [3, 0], w.sigma, s, graph, w.cam, group=S.GROUP)[0],
                   S.solve(pkg, s, w, [moved, problems[1]])[0], "after a SET_POSE")


# ---- what keeps the kernels inside their bounds ---------------------------------------------------------------------------------------
def test_a_scattered_log_is_refused(pkg, store):
    """Every point added to early and erased from late: each touched row would walk half the log.  The sum of the walks is beyond
    tc2li_map_graph_limits' max_walk, the call is TC2LI_ERR_CAPACITY and the graph unchanged; the same edits with every point's two
    together pass."""
    n_pt = 3000
    assert n_pt * (n_pt + 1) > pkg.map_graph_limits()["max_walk"] >= 2 * n_pt
    g = K.hand([dict(slot=0, id=1), dict(slot=1, id=2)], [dict(obs={}) for _ in range(n_pt)], 0, [1])
    scattered, together = M.Log(g), M.Log(g)
    for p in range(n_pt):
        scattered.add_observation(p, 0, 1)
    for p in range(n_pt):
        scattered.erase_observation(p, 1)
        together.add_observation(p, 0, 1); together.erase_observation(p, 1)
    caps = [2, 1, n_pt, n_pt]
    with pkg.ResidentMapGraph(store, 1, caps) as graph:
        graph.set_batch([0], [g])
        e, v = scattered.done()
        with pytest.raises(pkg.Tc2liError) as r:
            graph.apply_batch([(0, e, v)])
        assert r.value.code == T.CAPACITY and graph.info(0)["applies"] == 0
        ref.assert_same_tables(graph.download(0), ref.tables_of(g), "after the refused log")
        e2, v2 = together.done()
        graph.apply_batch([(0, e2, v2)])
        got = graph.download(0)
        ref.assert_same_tables(got, ref.apply(g, rows(e2), v2, caps, M.N_KEYS), "every point's edits together")
        ref.assert_same_tables(got, ref.apply(g, rows(e), v, caps, M.N_KEYS), "the scattered log says the same")


def test_a_store_slot_put_again_with_fewer_keypoints_is_refused(pkg):
    """The resident obs_index were checked against the keypoints the slot held then: the gather refuses rather than read beyond a slot."""
    views = [K.make_view(np.random.default_rng(3), 32), K.make_view(np.random.default_rng(4), 32)]
    g = K.hand([dict(slot=0, id=1, holds=[0]), dict(slot=1, id=2, holds=[0])], [dict(obs={0: 31, 1: 5})], 0, [1], init=1)
    with pkg.KeyframeStore(2, 64) as s, pkg.ResidentMapGraph(s, 1, [4, 8, 4, 8]) as graph:
        s.put_batch([0, 1], views, K.BOUNDS, n_levels=K.N_LEVELS)
        graph.set_batch([0], [g])
        want = pkg.ba_window_batch([g], K.SIGMA, store=s)[0]
        K.assert_equal(pkg.ba_window_graph_batch([g], [0], K.SIGMA, s, graph)[0], want, "before the put")
        assert want["status"] == wref.OK and len(want["edges"]) == 2
        s.put_batch([0], [K.make_view(np.random.default_rng(5), 48)], K.BOUNDS, n_levels=K.N_LEVELS)      # more keypoints: fine
        assert pkg.ba_window_graph_batch([g], [0], K.SIGMA, s, graph)[0]["status"] == wref.OK
        s.put_batch([0], [K.make_view(np.random.default_rng(6), 16)], K.BOUNDS, n_levels=K.N_LEVELS)      # index 31 is beyond these
        for run in (lambda: pkg.ba_window_graph_batch([g], [0], K.SIGMA, s, graph), lambda: pkg.ba_window_batch([g], K.SIGMA, store=s)):
            with pytest.raises(pkg.Tc2liError) as r:
                run()
            assert r.value.code == T.INVALID
