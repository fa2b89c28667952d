"""GPU tests of tc2li_ba_window_solve_graph_commit_batch: the solve from the resident map graph followed by the closing step of
LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:455-485) on the resident tables.  The outputs must be those of
tc2li_ba_window_solve_graph_batch bit for bit, and every sequence must end up as the host twin leaves its tables under the log of
tc2li_host_ba_window_commit_log.  Everything is an integer or a double carried through: the criterion is equality of every array."""
import copy

import numpy as np
import pytest

import ba_window_cases as K
import map_graph_cases as M
import map_graph_ref as ref
import test_ba_window_solve_gpu as S
import test_map_graph_gpu as G

pytestmark = pytest.mark.gpu
INVALID, CAPACITY = ref.INVALID, ref.CAPACITY


def plant_outlier(w, problem):
    """moves the keypoint behind one observation of the current keyframe by 30 px in the store's views: an edge the outlier rule erases"""
    cur = int(problem["current"])
    so, oo = problem["slot_offsets"], problem["obs_offsets"]
    for p in problem["slot_point"][so[cur]:so[cur + 1]]:
        if p < 0:
            continue
        for o in range(oo[p], oo[p + 1]):
            keys = w.views[int(problem["kf_slot"][cur])]["keys"]
            if problem["obs_kf"][o] == cur and problem["obs_index"][o] >= 0 and keys["x"][problem["obs_index"][o]] < 1100:
                keys["x"][problem["obs_index"][o]] += 30.0
                return
    raise AssertionError("no observation to move")


@pytest.fixture(scope="module")
def world(pkg, synthetic):
    """the windows of test_solve_from_the_graph -- the two smallest visual ones, the smallest LiDAR one, the one beyond the device range --
    with an outlier planted in the first and the last, and an ABORTED graph"""
    w = S.World(pkg, synthetic)
    w.views = copy.deepcopy(w.views)
    size = lambda i: len(w.problems[i]["point_flags"])
    visual = sorted((i for i, p in enumerate(w.problems) if p.get("clouds") is None), key=size)[:2]
    lidar = min((i for i, p in enumerate(w.problems) if p.get("clouds") is not None), key=size)
    w.four = [w.problems[visual[0]], w.problems[visual[1]], w.problems[lidar], w.wide]
    plant_outlier(w, w.four[0]); plant_outlier(w, w.four[3])
    w.aborted = w.hand([dict(slot=0, id=1, holds=[0]), dict(slot=1, id=2, holds=[0])], [dict(obs={0: 0, 1: 0})], 0, [1])
    w.caps = np.max([M.capacities_for(p, np.zeros(0, M.EDIT_DTYPE)) for p in w.four + [w.aborted]], 0).astype(np.int32)
    with w.store(pkg) as s:
        yield w, s


def commit(pkg, s, w, graph, problems, seq, **kw):
    return pkg.ba_window_solve_graph_commit_batch(problems, seq, w.sigma, s, graph, w.cam, group=S.GROUP, **kw)


def twin(pkg, before, solved, caps, flags=0):
    """the tables the commit must leave: the log of the host entry applied by the graph's host twin to the tables before the call"""
    e, v = pkg.host_ba_window_commit_log(before, solved, flags=flags)
    return pkg.host_map_graph_apply(before, e, v, caps), len(e), len(v)


def gather_bytes(pkg, w, problems):
    return len(problems) * pkg.map_graph_limits()["gather_record_bytes"] + 4 * len(w.sigma) + 4 * sum(len(p["cov_kf"]) for p in problems)


def test_four_windows_and_a_second_round(pkg, world):
    w, s = world
    problems, seq, lim = w.four, [3, 0, 4, 1], pkg.map_graph_limits()
    with pkg.ResidentMapGraph(s, 5, w.caps) as plain, pkg.ResidentMapGraph(s, 5, w.caps) as graph:
        for g in (plain, graph):
            g.set_batch(seq + [2], problems + [problems[0]])
        want = pkg.ba_window_solve_graph_batch(problems, seq, w.sigma, s, plain, w.cam, group=S.GROUP)
        got = commit(pkg, s, w, graph, problems, seq)
        for i, (a, b) in enumerate(zip(got, want)):
            G.same_solve(a, b, "window %d" % i)
        assert all(b["result"] > 0 for b in want) and want[3]["stats"].n_free_poses == 30     # three solved on the device, one on the host path
        assert want[0]["n_erase"] >= 1 and want[3]["n_erase"] >= 1, [b["n_erase"] for b in want]
        for i, (q, p) in enumerate(zip(seq, problems)):
            after, n_edits, n_values = twin(pkg, p, got[i], w.caps)
            ref.assert_same_tables(graph.download(q, fill=-77), after, "sequence %d" % q)
            ref.assert_same_tables(plain.download(q), ref.tables_of(p), "the plain solve writes nothing, sequence %d" % q)
            info = graph.info(q)
            assert info["applies"] == 1 and info["n_observations"] == int(p["obs_offsets"][-1]) - got[i]["n_erase"], (q, info)
            assert info["gather_bytes"] == gather_bytes(pkg, w, problems)
            if i < 3:                                                                  # solved on the device: one record, no value, no edit
                assert info["apply_bytes"] <= lim["apply_record_bytes"] <= 64, (q, info)
            else:                                                                      # the host path: its log goes through the apply
                assert info["apply_bytes"] == lim["apply_record_bytes"] + 16 * n_edits + 8 * n_values, (q, info)
        ref.assert_same_tables(graph.download(2, fill=-77), ref.tables_of(problems[0]), "the sequence left alone")
        assert graph.info(2)["applies"] == 0
        # a second round reads the committed tables: the generation flip and the starts
        now = [dict(p, **graph.download(q)) for q, p in zip(seq, problems)]
        again = pkg.ba_window_solve_graph_batch(now, seq, w.sigma, s, graph, w.cam, group=S.GROUP)
        for i, (a, b) in enumerate(zip(again, S.solve(pkg, s, w, now))):
            G.same_solve(a, b, "second round, window %d" % i)
        # ... and a second commit on top of the first
        got2 = commit(pkg, s, w, graph, now, seq)
        for i, (q, p) in enumerate(zip(seq, now)):
            G.same_solve(got2[i], again[i], "second commit, window %d" % i)
            ref.assert_same_tables(graph.download(q, fill=-77), twin(pkg, p, got2[i], w.caps)[0], "second commit, sequence %d" % q)
            assert graph.info(q)["applies"] == 2


def test_a_batch_of_one_takes_the_host_path_to_the_same_state(pkg, world):
    w, s = world
    with pkg.ResidentMapGraph(s, 2, w.caps) as graph:
        graph.set_batch([0, 1], [w.four[0], w.four[0]])
        got = commit(pkg, s, w, graph, [w.four[0]], [1])
        G.same_solve(got[0], S.solve(pkg, s, w, [w.four[0]])[0], "a batch of one")
        assert got[0]["n_erase"] >= 1
        ref.assert_same_tables(graph.download(1, fill=-77), twin(pkg, w.four[0], got[0], w.caps)[0], "a batch of one")
        ref.assert_same_tables(graph.download(0), ref.tables_of(w.four[0]), "the other sequence")
        assert graph.info(1)["applies"] == 1 and graph.info(0)["applies"] == 0


def test_the_mirror_counts_the_erased_observations(pkg, world):
    """observation capacity == the resident total: after a commit that erased k pairs an apply may add k observations and no more"""
    w, s = world
    p = w.four[0]
    caps = w.caps.copy()
    caps[3] = int(p["obs_offsets"][-1])
    with pkg.ResidentMapGraph(s, 2, caps) as graph:
        graph.set_batch([0, 1], [p, p])
        got = commit(pkg, s, w, graph, [p, p], [0, 1])
        k = got[0]["n_erase"]
        assert k >= 1 and graph.info(0)["n_observations"] == caps[3] - k and graph.info(0)["apply_bytes"] <= 64
        L = M.Log(p)
        for ep, et in got[0]["erase"]:                                                 # the erased pairs again, into rows that exist
            kf, pt = int(got[0]["pose_row"][ep]), int(got[0]["point_row"][et])
            o = int(p["obs_offsets"][pt]) + p["obs_kf"][p["obs_offsets"][pt]:p["obs_offsets"][pt + 1]].tolist().index(kf)
            L.add_observation(pt, kf, int(p["obs_index"][o]))
        e, v = L.done()
        L.add_observation(int(got[0]["point_row"][0]), int(p["obs_kf"][p["obs_offsets"][got[0]["point_row"][0]]]), 0)
        e1, v1 = L.done()
        before = graph.download(0)
        with pytest.raises(pkg.Tc2liError) as r:
            graph.apply_batch([(0, e1, v1)])                                            # k + 1
        assert r.value.code == CAPACITY
        ref.assert_same_tables(graph.download(0), before, "after the refused apply")
        graph.apply_batch([(0, e, v)])                                                  # k
        assert graph.info(0)["n_observations"] == caps[3]
        ref.assert_same_tables(graph.download(0), pkg.host_map_graph_apply(before, e, v, caps), "the erased pairs added again")


def test_refusals_change_no_sequence(pkg, world):
    import tc2li_slam_amd.capi as capi
    w, s = world
    problems, seq = w.four[:3], [2, 0, 1]
    real = capi.pack_ba_window_solve_problems
    seen = {}

    def spy(null_n_erase):
        def pack(problems_, fill=0):
            arr, outs, keep = real(problems_, fill)
            if null_n_erase:
                arr[1].n_erase = None
            seen["outs"] = outs
            return arr, outs, keep
        return pack

    with pkg.ResidentMapGraph(s, 3, w.caps) as graph:
        graph.set_batch(seq, problems)
        n_erase = [r["n_erase"] for r in pkg.ba_window_solve_graph_batch(problems, seq, w.sigma, s, graph, w.cam, group=S.GROUP)]
        assert n_erase[0] >= 1
        short = [dict(problems[0], erase_capacity=n_erase[0] - 1)] + problems[1:]
        cases = [("a sequence named twice", problems, [2, 0, 2], {}, False, INVALID), ("n_erase == NULL", problems, seq, {}, True, INVALID),
                 ("an unknown flag bit", problems, seq, dict(flags=2), False, INVALID),
                 ("an erase_capacity one short", short, seq, {}, False, CAPACITY)]
        for what, batch, sq, kw, null_n_erase, code in cases:
            capi.pack_ba_window_solve_problems = spy(null_n_erase)
            try:
                with pytest.raises(pkg.Tc2liError) as r:
                    commit(pkg, s, w, graph, batch, sq, fill=-77, **kw)
                outs = seen["outs"]
                if code == CAPACITY:                                                   # every other output as the solve entry writes it
                    with pytest.raises(pkg.Tc2liError) as r2:
                        pkg.ba_window_solve_graph_batch(batch, sq, w.sigma, s, graph, w.cam, group=S.GROUP, fill=-77)
                    assert r2.value.code == CAPACITY
                    for a, b in zip(outs, seen["outs"]):
                        for key in ("counts", "pose_row", "poses7_out", "fixed", "point_row", "points3_out", "erase_pose", "erase_point", "n_erase", "edge_chi2"):
                            assert S.bits(a[key]) == S.bits(b[key]), (what, key)
                    assert outs[0]["n_erase"][0] == n_erase[0] and outs[0]["poses7_out"][0] != -77
            finally:
                capi.pack_ba_window_solve_problems = real
            assert r.value.code == code, what
            for q, p in zip(seq, problems):
                ref.assert_same_tables(graph.download(q), ref.tables_of(p), what)
                assert graph.info(q)["applies"] == 0, what


def test_an_aborted_window_beside_committed_ones(pkg, world):
    w, s = world
    problems, seq = [w.four[0], w.aborted, w.four[1]], [1, 2, 0]
    with pkg.ResidentMapGraph(s, 3, w.caps) as graph:
        graph.set_batch(seq, problems)
        got = commit(pkg, s, w, graph, problems, seq)
        assert got[1]["status"] == 1 and got[1]["result"] == 0 and got[0]["result"] > 0 and got[2]["result"] > 0
        ref.assert_same_tables(graph.download(2, fill=-77), ref.tables_of(w.aborted), "the ABORTED window's sequence")
        assert [graph.info(q)["applies"] for q in seq] == [1, 0, 1]
        for i in (0, 2):
            ref.assert_same_tables(graph.download(seq[i], fill=-77), twin(pkg, problems[i], got[i], w.caps)[0], "beside an ABORTED window, %d" % i)


def test_positions_through_float(pkg, world):
    w, s = world
    problems, seq = w.four[:2], [1, 0]
    with pkg.ResidentMapGraph(s, 2, w.caps) as graph:
        graph.set_batch(seq, problems)
        got = commit(pkg, s, w, graph, problems, seq, flags=pkg.BA_COMMIT_POSITIONS_F32)
        for q, p, r in zip(seq, problems, got):
            t = graph.download(q, fill=-77)
            assert S.bits(t["positions"][r["point_row"]]) == S.bits(r["points3"].astype(np.float32).astype(np.float64))
            assert S.bits(t["positions"][r["point_row"]]) != S.bits(r["points3"])
            free = r["fixed"] == 0
            assert free.any() and S.bits(t["poses7"][r["pose_row"][free]]) == S.bits(r["poses7"][free])    # poses are never rounded
            ref.assert_same_tables(t, twin(pkg, p, r, w.caps, flags=pkg.BA_COMMIT_POSITIONS_F32)[0], "sequence %d" % q)
