"""GPU tests of the covisibility graph on the resident map graph: tc2li_map_graph_connections_reserve / set_connections_batch /
download_connections, tc2li_map_graph_update_connections_batch and tc2li_map_graph_erase_connections_batch against the host twins, the
restatements of tests/map_graph_connections_cases.py (tests/connections_ref.py written into the tables; KeyFrame::SetBadFlag's
covisibility part) and tc2li_update_connections_batch fed the downloaded tables.  Everything is an integer: the criterion is equality of
every array.  The sizes at which a kernel changes path come from tc2li_connections_limits and tc2li_map_graph_limits."""
import numpy as np
import pytest

import ba_window_cases as W
import connections_cases as K
import connections_ref as ref
import map_graph_cases as M
import map_graph_connections_cases as G
import map_graph_ref as MR
import test_ba_window as TW
import test_ba_window_solve_gpu as S
import test_map_graph_connections as T
import test_map_graph_gpu as MG

pytestmark = pytest.mark.gpu
SENTINEL = -77
SLOT = M.OCCUPIED[0]
ERR_INVALID, ERR_CAPACITY = -2, -5


@pytest.fixture(scope="module")
def store(pkg):
    """the world of ba_window_cases.py resident on the device: every keyframe row of these tests names one of its slots"""
    with pkg.KeyframeStore(W.WORLD_SLOTS, 64) as s:
        slots = [i for i, v in enumerate(W.WORLD) if v is not None]
        s.put_batch(slots, [W.WORLD[i] for i in slots], W.BOUNDS, n_levels=W.N_LEVELS)
        yield s


def on_slot(g):
    return dict(g, kf_slot=np.full(len(g["kf_slot"]), SLOT, np.int32))


def capacities(graphs, more=(0, 0, 0, 0)):
    return (np.max([[len(g["kf_slot"]), len(g["slot_point"]), len(g["point_flags"]), len(g["obs_kf"])] for g in graphs], 0) + np.array(more)).clip(1).astype(np.int32)


def entries(tables):
    return max(1, max(max(len(c["conn_kf"]), len(c["ord_kf"])) for c in tables))


def resident(pkg, store, graphs, conns, reserve, n_sequences=None, more=(0, 0, 0, 0)):
    graph = pkg.ResidentMapGraph(store, n_sequences or len(graphs), capacities(graphs, more))
    graph.connections_reserve(reserve)
    graph.set_batch(range(len(graphs)), [on_slot(g) for g in graphs])
    graph.set_connections_batch(range(len(graphs)), conns)
    return graph


def check_against_three(pkg, graph, cases, what):
    """the state after ONE update_connections_batch over all cases, one sequence each, against the twin, the restatement and the entry
    that takes host arrays"""
    n = len(cases)
    before = [graph.download_connections(s, fill=SENTINEL) for s in range(n)]
    for (name, g, c, *_), b in zip(cases, before):
        G.assert_same(b, G.with_rows(c, len(g["kf_flags"])), name + ": set, then downloaded")
    counts = graph.update_connections_batch(range(n), [c[3] for c in cases], [c[5] for c in cases], [c[4] for c in cases])
    problems = [G.problem_of(g, b, cur, first, init) for (_, g, _, cur, init, first, _, _), b in zip(cases, before)]
    flat = pkg.update_connections_batch(problems)
    for s, (name, g, c, cur, init, first, want_counts, want) in enumerate(cases):
        got = graph.download_connections(s, fill=SENTINEL)
        assert np.array_equal(counts[s], want_counts), (what, name, counts[s], want_counts)
        G.assert_same(got, want, "%s, %s: device against the restatement" % (what, name))
        twin_counts, twin = pkg.capi.host_map_graph_update_connections(g, c, cur, first, init)
        assert np.array_equal(counts[s], twin_counts), (what, name)
        G.assert_same(got, twin, "%s, %s: device against the twin" % (what, name))
        # the rows that changed are the lists of tc2li_update_connections_batch, every other row is as it was
        G.assert_same(got, G.updated(before[s], problems[s], flat[s]), "%s, %s: device against tc2li_update_connections_batch" % (what, name))
        assert np.array_equal(counts[s, :6], G.counts_of(flat[s])[:6]), (what, name)
        info = graph.connections_info(s)
        assert (info["weight_entries"], info["ordered_entries"], info["updates"]) == (len(want["conn_kf"]), len(want["ord_kf"]), 1), (what, name)


# ---- 1 ---------------------------------------------------------------------------------------------------------------------------------
def test_set_download_set_again(pkg, store):
    cases = T.cases(pkg)[4:12]
    graphs, conns = [c[1] for c in cases], [c[2] for c in cases]
    caps = capacities(graphs, more=(2, 8, 0, 8))
    with pkg.ResidentMapGraph(store, len(cases), caps) as graph:
        graph.set_batch(range(len(cases)), [on_slot(g) for g in graphs])
        for call in (lambda: graph.set_connections_batch([0], conns[:1]), lambda: graph.download_connections(0), lambda: graph.connections_info(0),
                     lambda: graph.update_connections_batch([0], [0], [0], [-1]), lambda: graph.erase_connections_batch([0], [0])):
            with pytest.raises(pkg.capi.Tc2liError) as e:                            # every entry is refused before the reserve
                call()
            assert e.value.code == ERR_INVALID
        with pytest.raises(pkg.capi.Tc2liError):
            graph.connections_reserve(0)
        graph.connections_reserve(entries(conns) + 4)
        with pytest.raises(pkg.capi.Tc2liError) as e:
            graph.connections_reserve(entries(conns) + 4)
        assert e.value.code == ERR_INVALID
        for s, g in enumerate(graphs):                                              # a set sequence without connections: empty rows
            got = graph.download_connections(s, fill=SENTINEL)
            assert len(got["conn_offsets"]) == len(g["kf_flags"]) + 1 and not got["conn_offsets"].any() and not got["ord_offsets"].any()
        graph.set_connections_batch(range(len(cases)), conns)
        for s, (g, c) in enumerate(zip(graphs, conns)):
            G.assert_same(graph.download_connections(s, fill=SENTINEL), c, cases[s][0])
        order = np.roll(np.arange(len(cases)), 3)[::2]                              # set again: connections of fewer rows than the graph has
        short = []
        for s in order:
            w, o = G.rows_of(conns[s])
            keep = max(1, len(w) // 2)
            short.append(G.tables_of([{k: v for k, v in r.items() if k < keep} for r in w[:keep]],
                                     [([k for k in r[0] if k < keep], [x for k, x in zip(*r) if k < keep]) for r in o[:keep]]))
        graph.set_connections_batch(order, short)
        for s, c in zip(order, short):
            G.assert_same(graph.download_connections(s, fill=SENTINEL), G.with_rows(c, len(graphs[s]["kf_flags"])), "set again, %d" % s)
        # refusals leave the state
        w, o = G.rows_of(conns[1])
        first = next(k for k in range(len(w)) if w[k])
        for bad, code in ((dict(conns[1], conn_kf=np.where(np.arange(len(conns[1]["conn_kf"])) == conns[1]["conn_offsets"][first], first, conns[1]["conn_kf"])), ERR_INVALID),
                          (G.with_rows(conns[1], len(graphs[1]["kf_flags"]) + 1), ERR_INVALID)):
            with pytest.raises(pkg.capi.Tc2liError) as e:
                graph.set_connections_batch([1], [bad])
            assert e.value.code == code
        G.assert_same(graph.download_connections(1, fill=SENTINEL), G.with_rows(graph_state(conns, order, short, 1), len(graphs[1]["kf_flags"])), "after the refusals")
        # rows that ADD_KEYFRAME appends read as empty
        log = M.Log(graph.download(0))
        log.add_keyframe(SLOT, 3, 9001, 0, G.POSE7)
        log.add_keyframe(SLOT, 0, 9002, 0, G.POSE7)
        graph.apply_batch([(0, *log.done())])
        rows0 = graph.info(0)["n_keyframes"]
        now0 = graph.download_connections(0, fill=SENTINEL)
        G.assert_same(now0, G.with_rows(graph_state(conns, order, short, 0), rows0), "after two appends")
        assert rows0 == len(graphs[0]["kf_flags"]) + 2
        # ... and an update on the appended keyframe without slots finds an empty counter: UNCHANGED, the rows are still what they were
        counts = graph.update_connections_batch([0], [rows0 - 1], [1], [-1])
        assert counts[0].tolist() == [0, 0, 0, 0, 0, -1, 0, 0]
        G.assert_same(graph.download_connections(0, fill=SENTINEL), now0, "UNCHANGED after two appends")
        assert graph.connections_info(0)["weight_entries"] == len(now0["conn_kf"])
        # set_batch empties the connections of the sequences it names, and of no other
        graph.set_batch([2], [on_slot(graphs[2])])
        got = graph.download_connections(2, fill=SENTINEL)
        assert not got["conn_offsets"].any() and not got["ord_offsets"].any() and len(got["conn_kf"]) == 0
        assert graph.connections_info(2)["weight_entries"] == 0
        G.assert_same(graph.download_connections(0, fill=SENTINEL), now0, "sequence 0 beside the set")
        nk3 = len(graphs[3]["kf_flags"])                                             # beyond the reserve
        with pkg.ResidentMapGraph(store, 1, caps) as small:
            small.connections_reserve(1)
            small.set_batch([0], [on_slot(graphs[3])])
            with pytest.raises(pkg.capi.Tc2liError) as e:
                small.set_connections_batch([0], [G.tables_of([{1: 1}, {0: 2}] + [{}] * (nk3 - 2), [([], [])] * nk3)])
            assert e.value.code == ERR_CAPACITY
            assert small.connections_info(0)["weight_entries"] == 0


def graph_state(conns, order, short, s):
    return short[list(order).index(s)] if s in order else conns[s]


# ---- 2 ---------------------------------------------------------------------------------------------------------------------------------
def test_update_against_three_references(pkg, store):
    """every generated, hand-made and directed case, one sequence each, in ONE batch"""
    cases = T.cases(pkg)
    graph = resident(pkg, store, [c[1] for c in cases], [c[2] for c in cases], entries([c[2] for c in cases] + [c[7] for c in cases]))
    with graph:
        check_against_three(pkg, graph, cases, "all cases")
    assert {0, 1} == {int(c[6][0]) for c in cases}


# ---- 3 ---------------------------------------------------------------------------------------------------------------------------------
def test_path_boundaries(pkg, store):
    L, row = pkg.connections_limits()["lds_keyframes"], pkg.map_graph_limits()["lds_row"]
    lens = (63, 64, 65, 255, 257, row + 1)
    problems = [K.make_problem(900 + i, n_kf, 300, n_seen, "high", rl, None, first=True, special=False)   # every observer passes 15 votes
                for i, (n_kf, n_seen, rl) in enumerate([(L, 60, lens), (L + 1, 60, lens)] + [(400, n, (9,)) for n in (63, 64, 65, 255, 257)])]
    n = 70
    kfs, points, slots = K.votes(n, 7, {3: 15, 5: 16})
    kfs[3]["conn"] = {k: 1 + k % 5 for k in range(n) if k not in (3, 7)}             # full up to one entry
    kfs[5]["conn"] = {k: 2 + k % 3 for k in range(n) if k != 5}                      # full: the overwrite
    problems.append(K.hand(kfs, points, slots, 7))
    cases = []
    for i, pr in enumerate(problems):
        g, c, init = G.graph_of(pr, seed=i)
        counts, want = G.update_ref(g, c, pr["current"], pr["first_connection"], init)
        cases.append(("boundary %d" % i, g, c, int(pr["current"]), init, int(pr["first_connection"]), counts, want))
    # the cases are what they are meant to be
    assert [len(c[1]["kf_flags"]) for c in cases[:2]] == [L, L + 1]
    assert [int(c[6][2]) for c in cases[2:7]] == [63, 64, 65, 255, 257]              # the current keyframe's own lists
    for c in cases[:2]:
        res = ref.update_connections(G.problem_of(c[1], c[2], c[3], c[5], c[4]))
        touched_rows = {int(np.diff(c[2]["conn_offsets"])[k]) for k in res["touched_kf"]}
        assert {63, 64, 65, 255, 257, row + 1} <= touched_rows, sorted(touched_rows)
    assert np.diff(cases[-1][7]["conn_offsets"])[[3, 5]].tolist() == [n - 1, n - 1]
    graph = resident(pkg, store, [c[1] for c in cases], [c[2] for c in cases], entries([c[2] for c in cases] + [c[7] for c in cases]))
    with graph:
        check_against_three(pkg, graph, cases, "boundaries")


# ---- 4 ---------------------------------------------------------------------------------------------------------------------------------
def test_directed_cases(pkg, store):
    cases = []
    for i, (name, pr, ordered, check) in enumerate(G.directed()):
        g, c, init = G.graph_of(pr, seed=i, ordered=ordered, stale=0)
        counts, want = G.update_ref(g, c, pr["current"], pr["first_connection"], init)
        cases.append((name, g, c, int(pr["current"]), init, int(pr["first_connection"]), counts, want))
    by_name = {c[0]: c for c in cases}
    graph = resident(pkg, store, [c[1] for c in cases], [c[2] for c in cases], entries([c[2] for c in cases] + [c[7] for c in cases]) + 3)
    with graph:
        check_against_three(pkg, graph, cases, "directed")
        got = {c[0]: graph.download_connections(s) for s, c in enumerate(cases)}
    # ... and the expectations written out, so that the restatement cannot drift
    name = "an empty counter"
    assert by_name[name][6].tolist() == [0, 0, 0, 0, 0, -1, 0, 0]
    G.assert_same(got[name], by_name[name][2], name)
    w, o = G.rows_of(got["nobody reaches 15: the lone best, the lowest row among equals"])
    assert w[2] == {1: 7, 3: 7, 4: 5} and o[2] == ([1], [7]) and w[1] == {2: 7} and o[1] == ([2], [7]) and not w[3] and not w[4]
    w, o = G.rows_of(got["a point in two slots votes twice"])
    assert w[0] == {1: 16, 2: 14} and o[0] == ([1], [16]) and w[1] == {0: 16} and not w[2]
    w, o = G.rows_of(got["a bad voter and an other-map voter"])
    assert w[0] == {1: 20, 4: 16} and o[0] == ([1, 4], [20, 16]) and not w[2] and not w[3]
    w, o = G.rows_of(got["a neighbour holds (current, same weight) and keeps its stale list; another holds a different weight"])
    assert w[0] == {1: 20, 3: 9, 4: 11} and o[0] == ([3, 1], [9, 2])                  # stale before, stale after (:209-210)
    assert w[2] == {1: 17, 4: 2} and o[2] == ([1, 4], [17, 2]) and w[1] == {0: 20, 2: 17, 3: 3} and o[1] == ([0, 2], [20, 17])
    w, o = G.rows_of(got["a bad keyframe inside a neighbour's weight row"])
    assert w[0] == {2: 40, 3: 40, 4: 1, 5: 15} and o[0] == ([2, 5, 4], [40, 15, 1]) and o[5] == ([1, 0], [15, 15])
    assert [int(by_name["current is the init keyframe, first_connection %d" % f][6][5]) for f in (1, 0)] == [-1, -1]
    assert int(by_name["first_connection, not the init keyframe"][6][5]) == 2


# ---- 5 ---------------------------------------------------------------------------------------------------------------------------------
def test_five_updates_in_a_row_between_applies(pkg, store):
    """one sequence; before every update a log adds a keyframe and its observations.  Both generations of both CSRs are read and
    written more than once, and the new keyframe's rows are the empty ones of a row appended since."""
    rng = np.random.default_rng(11)
    nk, npts = 12, 90
    obs = [np.sort(rng.choice(nk, rng.integers(2, 7), replace=False)) for _ in range(npts)]
    pr = K.make_problem(78, nk, 0, 0)
    pr.update(obs_offsets=np.r_[0, np.cumsum([len(o) for o in obs])].astype(np.int32), obs_kf=np.concatenate(obs).astype(np.int32),
              point_bad=(rng.random(npts) < 0.05).astype(np.uint8), kf_flags=np.zeros(nk, np.uint8))
    g, c, _ = G.graph_of(pr)
    held = [[p for p in range(npts) if k in obs[p]] for k in range(nk)]
    g["slot_offsets"] = np.r_[0, np.cumsum([len(h) for h in held])].astype(np.int32)
    g["slot_point"] = np.array([p for h in held for p in h], np.int32)
    caps = np.array([nk + 5, len(g["slot_point"]) + 5 * 40, npts, len(g["obs_kf"]) + 5 * 40], np.int32)
    with pkg.ResidentMapGraph(store, 2, caps) as graph:
        graph.connections_reserve(2 * (nk + 5) * (nk + 5))
        graph.set_batch([1], [on_slot(g)])
        graph.set_connections_batch([1], [c])
        statuses = []
        for i in range(5):
            log = M.Log(graph.download(1))
            points = rng.choice(npts, 40, replace=False)
            new = log.add_keyframe(SLOT, 40, 500 + i, 0, G.POSE7)
            for j, p in enumerate(points):
                log.set_slot(new, j, int(p))
            for p in np.sort(points):
                log.add_observation(int(p), new, -1)
            graph.apply_batch([(1, *log.done())])
            tables = graph.download(1)
            assert len(tables["kf_flags"]) == nk + i + 1
            before = graph.download_connections(1, fill=SENTINEL)
            G.assert_same(before, G.with_rows(c, nk + i + 1), "rows appended before update %d" % i)
            cur = new if i != 2 else 4                                               # once an old keyframe
            first, init = int(i in (0, 3)), 500 + i if i == 3 else -1                # once the current keyframe is the init keyframe
            counts = graph.update_connections_batch([1], [cur], [first], [init])[0]
            want_counts, want = G.update_ref(tables, c, cur, first, init)
            got = graph.download_connections(1, fill=SENTINEL)
            assert np.array_equal(counts, want_counts), (i, counts, want_counts)
            G.assert_same(got, want, "update %d: restatement" % i)
            twin_counts, twin = pkg.capi.host_map_graph_update_connections(tables, c, cur, first, init)
            assert np.array_equal(counts, twin_counts)
            G.assert_same(got, twin, "update %d: twin" % i)
            assert graph.connections_info(1)["updates"] == i + 1
            statuses.append(int(counts[0]))
            assert (counts[5] >= 0) == (i == 0)
            c = want
        assert statuses == [1] * 5


# ---- 6, 7 ------------------------------------------------------------------------------------------------------------------------------
def test_atomic_on_capacity_and_bus_bytes(pkg, store):
    cases = [c for c in T.cases(pkg) if c[0] in ("family 6", "family 7", "workload 3", "hand: the threshold")]
    assert len(cases) == 4 and all(int(c[6][0]) == 1 for c in cases)
    need = entries([c[7] for c in cases])
    tight = max(range(len(cases)), key=lambda s: max(len(cases[s][7]["conn_kf"]), len(cases[s][7]["ord_kf"])))
    assert need > entries([c[2] for c in cases])                                     # the update grows the CSRs beyond what was set
    lim = pkg.capi.map_graph_connections_limits()
    assert 0 < lim["record_bytes"] <= 64 and 0 < lim["status_bytes"] <= 16
    args = (range(4), [c[3] for c in cases], [c[5] for c in cases], [c[4] for c in cases])
    for reserve in (need - 1, need):
        graph = resident(pkg, store, [c[1] for c in cases], [c[2] for c in cases], reserve)
        with graph:
            if reserve < need:
                counts = np.full((4, 8), SENTINEL, np.int32)
                with pytest.raises(pkg.capi.Tc2liError) as e:
                    graph.update_connections_batch(*args, counts_into=counts)
                assert e.value.code == ERR_CAPACITY
                for s, c in enumerate(cases):                                        # the sizes needed, and nothing changed anywhere
                    assert np.array_equal(counts[s, :6], c[6][:6]) and counts[s, 6:].tolist() == [len(c[7]["conn_kf"]), len(c[7]["ord_kf"])], (s, counts[s])
                    G.assert_same(graph.download_connections(s, fill=SENTINEL), G.with_rows(c[2], len(c[1]["kf_flags"])), "refused: %s" % c[0])
                    info = graph.connections_info(s)
                    assert (info["updates"], info["update_bytes"], info["weight_entries"]) == (0, 0, len(c[2]["conn_kf"]))
                assert max(counts[tight, 6:]) == need
                # ... the refused call left nothing behind: the other three go through
                rest = [s for s in range(4) if s != tight]
                graph.update_connections_batch(rest, [cases[s][3] for s in rest], [cases[s][5] for s in rest], [cases[s][4] for s in rest])
                for s, c in enumerate(cases):
                    G.assert_same(graph.download_connections(s, fill=SENTINEL), c[7] if s != tight else G.with_rows(c[2], len(c[1]["kf_flags"])), "after: %s" % c[0])
            else:
                counts = graph.update_connections_batch(*args)
                for s, c in enumerate(cases):
                    assert np.array_equal(counts[s], c[6])
                    G.assert_same(graph.download_connections(s, fill=SENTINEL), c[7], "with room: %s" % c[0])
                    assert graph.connections_info(s)["update_bytes"] == lim["record_bytes"] * 1      # one record, no table, list or row
                graph.erase_connections_batch([1, 2], [cases[1][3], cases[2][3]])
                for s in range(4):
                    info = graph.connections_info(s)
                    assert info["update_bytes"] == lim["record_bytes"] and info["updates"] == (2 if s in (1, 2) else 1)
                    assert graph.info(s)["apply_bytes"] == 0 and graph.info(s)["applies"] == 0        # the graph's own tables saw no edit


# ---- 8 ---------------------------------------------------------------------------------------------------------------------------------
def test_erase(pkg, store):
    cases = []
    for name, pr, row, ordered in G.erase_cases(pkg.map_graph_limits()["lds_row"]):
        g, c, _ = G.graph_of(pr, ordered=ordered, stale=0)
        cases.append((name, g, c, row, ordered))
    for name, g, c, cur, init, first, counts, want in T.cases(pkg)[:24:3]:           # generated graphs after their update: asymmetric rows, bad keyframes
        cases.append((name, g, want, int(np.argmax(np.diff(want["conn_offsets"]))), None))
    graph = resident(pkg, store, [c[1] for c in cases], [c[2] for c in cases], entries([c[2] for c in cases]))
    with graph:
        graph.erase_connections_batch(range(len(cases)), [c[3] for c in cases])
        for s, (name, g, c, row, ordered) in enumerate(cases):
            got = graph.download_connections(s, fill=SENTINEL)
            want = G.erased(g, c, row)
            G.assert_same(got, want, name + ": device against the restatement")
            G.assert_same(got, pkg.capi.host_map_graph_erase_connections(g, c, row), name + ": device against the twin")
            w, o = G.rows_of(got)
            for k, v in (ordered or {}).items():
                assert o[k] == (list(v[0]), list(v[1])) and row not in G.rows_of(c)[0][k], name   # it did not hold the entry: its odd list stays
            info = graph.connections_info(s)
            assert (info["weight_entries"], info["ordered_entries"], info["updates"]) == (len(want["conn_kf"]), len(want["ord_kf"]), 1)
        # a second erase of the same rows finds nothing to do
        graph.erase_connections_batch(range(len(cases)), [c[3] for c in cases])
        for s, (name, g, c, row, ordered) in enumerate(cases):
            G.assert_same(graph.download_connections(s, fill=SENTINEL), G.erased(g, c, row), name + ": erased twice")
    big = [c for c in cases if c[0].startswith("65 ")][0]
    w, o = G.rows_of(G.erased(big[1], big[2], big[3]))
    assert len(w[2]) == len(big[1]["kf_flags"]) - 2 and len(o[2]) and len(big[1]["kf_flags"]) - 1 not in o[2][0]   # the other bad keyframe is not in the new list


# ---- 11 --------------------------------------------------------------------------------------------------------------------------------
def test_512_sequences_beside_512_left_alone(pkg, store):
    kfs, points, slots = K.votes(6, 2, {0: 15, 1: 14, 3: 16, 4: 15, 5: 1})
    kfs[0]["conn"], kfs[4]["conn"], kfs[5]["conn"] = {1: 4, 2: 15}, {2: 3, 5: 9}, {4: 9}
    g, c, init = G.graph_of(K.hand(kfs, points, slots, 2, first_connection=1), stale=2)
    want_counts, want = G.update_ref(g, c, 2, 1, init)
    with pkg.ResidentMapGraph(store, 1024, capacities([g])) as graph:
        graph.connections_reserve(entries([want]) + 1)
        graph.set_batch(range(1024), [on_slot(g)] * 1024)
        graph.set_connections_batch(range(1024), [c] * 1024)
        named = np.random.default_rng(5).permutation(1024)[:512]
        counts = graph.update_connections_batch(named, [2] * 512, [1] * 512, [init] * 512)
        assert np.array_equal(counts, np.tile(want_counts, (512, 1)))
        twin = pkg.capi.host_map_graph_update_connections(g, c, 2, 1, init)[1]
        G.assert_same(twin, want)
        updated = set(named.tolist())
        for s in range(1024):
            G.assert_same(graph.download_connections(s, fill=SENTINEL), want if s in updated else c, "sequence %d" % s)
        assert graph.connections_info(int(named[0]))["updates"] == 1 and graph.connections_info(int(min(set(range(1024)) - updated)))["updates"] == 0


# ---- 9 ---------------------------------------------------------------------------------------------------------------------------------
def list_as_connections(n_kf, current, cov_kf):
    """connection tables in which the ordered row of `current` is cov_kf (weights descending) and every other row is empty"""
    lists = [([], [])] * n_kf
    lists[current] = ([int(k) for k in cov_kf], list(range(len(cov_kf) + 7, 7, -1)))
    return G.tables_of([{}] * n_kf, lists)


def test_gather_reads_the_resident_list(pkg, store):
    """tc2li_ba_window_graph_cov_batch against tc2li_ba_window_graph_batch given the downloaded ordered row, on the graphs of
    ba_window_cases.family: every output equal, GATHER_BYTES smaller by 4 * n_cov"""
    problems, _ = TW.family_of(pkg)
    caps = np.max([M.capacities_for(p, np.zeros(0, M.EDIT_DTYPE)) for p in problems], 0).astype(np.int32)
    caps[0] += 1
    seq = np.arange(len(problems))
    with pkg.ResidentMapGraph(store, len(problems), caps) as graph:
        graph.set_batch(seq, problems)
        with pytest.raises(pkg.capi.Tc2liError) as e:                                # no reserve, no resident list
            pkg.ba_window_graph_cov_batch(problems[:1], [0], W.SIGMA, store, graph)
        assert e.value.code == ERR_INVALID
        graph.connections_reserve(max(1, max(len(p["cov_kf"]) for p in problems)))
        graph.set_connections_batch(seq, [list_as_connections(len(p["kf_slot"]), int(p["current"]), p["cov_kf"]) for p in problems])
        rows = [graph.download_connections(s, fill=SENTINEL) for s in seq]
        now = []
        for p, c in zip(problems, rows):
            cur = int(p["current"])
            now.append(dict(p, cov_kf=c["ord_kf"][c["ord_offsets"][cur]:c["ord_offsets"][cur + 1]].copy()))
            assert np.array_equal(now[-1]["cov_kf"], np.asarray(p["cov_kf"], np.int32))
        flags_named = [p["kf_flags"][np.asarray(p["cov_kf"], np.int64)] for p in problems]
        assert any((f & 1).any() for f in flags_named) and any((f & 2).any() for f in flags_named)   # a bad and an other-map keyframe in a list
        want = pkg.ba_window_graph_batch(now, seq, W.SIGMA, store, graph)
        sent = graph.info(0)["gather_bytes"]
        got = pkg.ba_window_graph_cov_batch(now, seq, W.SIGMA, store, graph)
        for i, (a, b) in enumerate(zip(got, want)):
            W.assert_equal(a, b, "problem %d: the resident list against the uploaded one" % i)
        n_cov = sum(len(p["cov_kf"]) for p in now)
        assert n_cov > 100 and all(graph.info(int(s))["gather_bytes"] == sent - 4 * n_cov for s in seq)
        assert sent - 4 * n_cov == len(now) * pkg.map_graph_limits()["gather_record_bytes"] + 4 * len(W.SIGMA)   # records and the level table
        statuses = {int(b["status"]) for b in want}
        assert len(statuses) >= 2
        raw_a = pkg.ba_window_graph_cov_batch(now, seq, W.SIGMA, store, graph, raw=True, fill=SENTINEL)   # and nothing beyond the counts is written
        raw_b = pkg.ba_window_graph_batch(now, seq, W.SIGMA, store, graph, raw=True, fill=SENTINEL)
        for i, (a, b) in enumerate(zip(raw_a, raw_b)):
            for k in a:
                assert (a[k] is None and b[k] is None) or np.array_equal(a[k], b[k]), (i, k)
        with pytest.raises(pkg.capi.Tc2liError) as e:                                # a list of the caller's is refused
            pkg.ba_window_graph_cov_batch([p for p in now if len(p["cov_kf"])][:1], [int(next(s for s in seq if len(now[s]["cov_kf"])))], W.SIGMA, store, graph, keep_cov=True)
        assert e.value.code == ERR_INVALID
        # a keyframe row appended since the connections were set has an empty list
        s = int(next(s for s in seq if len(now[s]["cov_kf"]) and want[s]["status"] == 0))
        log = M.Log(now[s])
        src = int(now[s]["current"])
        new = log.add_keyframe(int(now[s]["kf_slot"][src]), 0, 7777, 0, np.asarray(now[s]["poses7"], np.float64).reshape(-1, 7)[src])
        graph.apply_batch([(s, *log.done())])
        alone = dict(now[s], **graph.download(s))
        alone.update(current=new, cov_kf=np.zeros(0, np.int32))
        W.assert_equal(pkg.ba_window_graph_cov_batch([alone], [s], W.SIGMA, store, graph)[0], pkg.ba_window_graph_batch([alone], [s], W.SIGMA, store, graph)[0],
                       "a row appended since")


# ---- 10 --------------------------------------------------------------------------------------------------------------------------------
def test_solve_and_commit_read_the_resident_list(pkg, synthetic):
    """tc2li_ba_window_solve_graph_commit_cov_batch on the two smallest visual windows of tests/test_ba_window_solve_gpu.py: results,
    outputs and the graph afterwards are those of the commit entry that is given the lists"""
    w = S.World(pkg, synthetic)
    size = lambda i: len(w.problems[i]["point_flags"])
    two = [w.problems[i] for i in sorted((i for i, p in enumerate(w.problems) if p.get("clouds") is None), key=size)[:2]]
    assert all(len(p["cov_kf"]) for p in two)
    caps = np.max([M.capacities_for(p, np.zeros(0, M.EDIT_DTYPE)) for p in two], 0).astype(np.int32)
    seq = [2, 0]
    with w.store(pkg) as s, pkg.ResidentMapGraph(s, 3, caps) as plain, pkg.ResidentMapGraph(s, 3, caps) as graph:
        for g in (plain, graph):
            g.set_batch(seq, two)
        graph.connections_reserve(max(len(p["cov_kf"]) for p in two))
        conns = [list_as_connections(len(p["kf_slot"]), int(p["current"]), p["cov_kf"]) for p in two]
        graph.set_connections_batch(seq, conns)
        want = pkg.ba_window_solve_graph_commit_batch(two, seq, w.sigma, s, plain, w.cam, group=S.GROUP)
        got = pkg.ba_window_solve_graph_commit_cov_batch(two, seq, w.sigma, s, graph, w.cam, group=S.GROUP)
        assert all(b["result"] > 0 for b in want)
        for i, (a, b) in enumerate(zip(got, want)):
            MG.same_solve(a, b, "window %d" % i)
        for q, c in zip(seq, conns):
            MR.assert_same_tables(graph.download(q, fill=SENTINEL), plain.download(q, fill=SENTINEL), "sequence %d after the commit" % q)
            G.assert_same(graph.download_connections(q, fill=SENTINEL), c, "the commit leaves the connections, sequence %d" % q)
            assert graph.info(q)["applies"] == plain.info(q)["applies"] == 1
            assert graph.info(q)["gather_bytes"] == plain.info(q)["gather_bytes"] - 4 * sum(len(p["cov_kf"]) for p in two)
