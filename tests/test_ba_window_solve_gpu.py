"""GPU tests of the local BA from the flat graph.  The device-built index structure of the windows: tc2li_ba_window_structure_batch against
tc2li_host_ba_window_batch followed by tc2li_host_ba_structure, array for array, on the windows of tests/test_ba_structure.py in several
batch compositions, on the generated graphs and on the hand-made rule graphs of tests/test_ba_window.py.  The one call:
tc2li_ba_window_solve_batch against tc2li_ba_window_batch + tc2li_local_bundle_adjustment_batch_group + tc2li_ba_window_outliers on the same
inputs, bit for bit, with LiDAR edges, a window that rejects trials, every kind of window of the contract in one batch, a capacity one
short, edges not asked for, and a stop flag that is already set.  Integers are compared for equality, floats by their bytes."""
import numpy as np
import pytest

import ba_window_cases as K
import ba_window_ref as ref
import test_ba_structure as S
import test_ba_window as T

pytestmark = pytest.mark.gpu

IN_BLOCK = ("pose_var", "pt_off", "pt_edges", "pv_off", "fl_off", "fl_pose", "fl_lm", "fl_place", "fl_edge", "slice_off", "blk_off", "blk_rows",
            "grp_k0", "grp_l0")
NOT_IN_BLOCK = ("pv_edges", "w_slot", "dup_off", "dup_edge", "dup_slot", "chunk_mask")


def expect(pkg, g, lidar):
    """What the device must answer for the gathered window g: the host structure, or a result code."""
    lim = pkg.ba_window_solve_limits()
    if g["status"] != ref.OK:
        return 0
    fixed, e = g["fixed"], g["edges"]
    xu = S.extra_used(len(fixed), g["lidar_pose_index"]) if lidar and g["n_lidar"] else None
    used = np.bincount(e["pose"], minlength=len(fixed)) + (0 if xu is None else xu)
    if len(fixed) > lim["max_poses"] or len(g["point_row"]) > lim["max_points"] or ((fixed == 0) & (used > 0)).sum() > lim["max_free"]:
        return pkg.capi.BA_STRUCTURE_DECLINED
    try:
        return pkg.capi.host_ba_structure(fixed, len(g["point_row"]), e, xu)
    except pkg.Tc2liError as err:
        assert err.code == S.INVALID
        return S.INVALID


def check(pkg, store, problems, host, what, lidar=True, sigma=K.SIGMA):
    """host: the problems through the host gather.  -> what the device answered per problem"""
    flags = None if lidar is True else np.asarray(lidar, np.uint8)
    gathered, structures = pkg.ba_window_structure_batch(problems, sigma, store, with_lidar=flags)
    assert len(gathered) == len(structures) == len(problems)
    for i, (g, s, h) in enumerate(zip(gathered, structures, host)):
        K.assert_equal(g, h, "%s: problem %d, the gather" % (what, i))
        want = expect(pkg, h, True if lidar is True else bool(lidar[i]))
        if isinstance(want, int):
            assert s == want, (what, i, s if isinstance(s, int) else "built", want)
            continue
        assert isinstance(s, dict), (what, i, s)
        for k in pkg.capi.BA_STRUCTURE_SCALARS:
            assert s[k] == want[k], (what, i, k, s[k], want[k])
        for k in IN_BLOCK:
            assert np.array_equal(s[k], want[k]), (what, i, k, s[k].tolist(), want[k].tolist())
        assert all(len(s[k]) == 0 for k in NOT_IN_BLOCK) and s["n_dups"] == 0 and s["sparse"] == 1
    return structures


@pytest.fixture(scope="module")
def store(pkg):
    with pkg.KeyframeStore(K.WORLD_SLOTS, 64) as s:
        slots = [i for i, v in enumerate(K.WORLD) if v is not None]
        s.put_batch(slots, [K.WORLD[i] for i in slots], K.BOUNDS, n_levels=K.N_LEVELS)
        yield s


@pytest.fixture(scope="module")
def windows(pkg, synthetic):
    """the windows of test_ba_structure.py behind one store: (store, problems, their host gather, the windows' own sigma table)"""
    views, problems = [], []
    for v, pr, sigma in S.gathered_windows(pkg, synthetic):
        problems.append(dict(pr, kf_slot=pr["kf_slot"] + len(views)))
        views += v
    host = pkg.ba_window_batch(problems, sigma, views=views)
    with pkg.KeyframeStore(len(views), max(len(v["keys"]) for v in views)) as s:
        s.put_batch(list(range(len(views))), views, K.BOUNDS, n_levels=K.N_LEVELS)
        yield s, problems, host, sigma


def test_limits(pkg):
    lim = pkg.ba_window_solve_limits()
    assert lim["max_free"] == 24 and lim["threads"] == 256 and lim["max_poses"] >= 256 and lim["max_points"] >= 1024


def test_windows_one_batch_and_reversed(pkg, windows):
    s, problems, host, sigma = windows
    built = check(pkg, s, problems, host, "one batch", sigma=sigma)
    assert all(isinstance(b, dict) for b in built) and [b["n_free"] for b in built] == [n for n, _ in S.WINDOWS]
    assert max(b["n_schur_slices"] for b in built) > 16 and max(b["n_groups"] for b in built) > 2 and max(b["n_blocks"] for b in built) > 2
    again = check(pkg, s, problems[::-1], host[::-1], "reversed", sigma=sigma)
    for a, b in zip(again[::-1], built):
        assert all(np.array_equal(a[k], b[k]) for k in IN_BLOCK)


def test_windows_one_by_one(pkg, windows):
    s, problems, host, sigma = windows
    for i, (p, h) in enumerate(zip(problems, host)):
        check(pkg, s, [p], [h], "window %d alone" % i, sigma=sigma)


def test_lidar_keyframes_count_as_used_only_when_asked(pkg, windows):
    s, problems, host, sigma = windows
    with_cloud = [i for i, h in enumerate(host) if h["n_lidar"]]
    assert with_cloud
    flags = [i % 2 for i in range(len(problems))]
    check(pkg, s, problems, host, "LiDAR for every second window", lidar=flags, sigma=sigma)
    check(pkg, s, problems, host, "no LiDAR", lidar=[0] * len(problems), sigma=sigma)


def test_generated_graphs(pkg, store):
    problems, _ = T.family_of(pkg)
    host = T.host_run(pkg)(problems)
    got = check(pkg, store, problems, host, "family")
    kinds = {"built" if isinstance(g, dict) else g for g in got}
    assert kinds == {"built", 0, S.INVALID, pkg.capi.BA_STRUCTURE_DECLINED}, kinds      # every return path, in one batch
    clean = [p for p, h in zip(problems, host) if h["status"] == ref.OK][:6]
    for i, p in enumerate(clean):
        check(pkg, store, [p], T.host_run(pkg)([p]), "family graph %d alone" % i)


@pytest.mark.parametrize("rule", T.RULES, ids=lambda r: r.__name__)
def test_rule_graphs(pkg, store, rule):
    """the hand-made graphs of test_ba_window.py: the rule's own assertions on the gather, and the structure of every graph it makes"""
    def run(problems, **kw):
        assert not kw
        host = T.host_run(pkg)(problems)
        check(pkg, store, problems, host, rule.__name__)
        return pkg.ba_window_structure_batch(problems, K.SIGMA, store)[0]
    rule(run)


def test_a_point_with_257_observers_is_refused_on_the_device(pkg):
    """more than 256 edges on one point: TC2LI_ERR_INVALID as the BA answers, decided by the kernels; 256 are fine"""
    rng = np.random.default_rng(9)
    views = [K.make_view(rng, 8) for _ in range(258)]
    with pkg.KeyframeStore(len(views), 8) as s:
        s.put_batch(list(range(len(views))), views, K.BOUNDS, n_levels=K.N_LEVELS)
        for n_obs, want in ((257, S.INVALID), (256, "built")):
            kfs = [dict(slot=i, id=10 + i, holds=[0, 1] if i == 0 else []) for i in range(258)]
            points = [dict(obs={k: 1 for k in range(n_obs)}), dict(obs={0: 2, 257: 3})]
            pr = K.hand(kfs, points, 0, [])
            host = pkg.ba_window_batch([pr], K.SIGMA, views=views)
            assert len(host[0]["edges"]) == n_obs + 2
            got = check(pkg, s, [pr], host, "%d observers" % n_obs)[0]
            assert (got if isinstance(got, int) else "built") == want


def test_out_stride_too_small(pkg, windows):
    s, problems, host, sigma = windows
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.ba_window_structure_batch(problems[:3], sigma, s, out_stride=64)
    assert e.value.code == T.CAPACITY


# ---- gather, BA and outlier rule in one call against the three calls ---------------------------------------------------------------------
# (seed, n_opt, n_fix, n_points, LiDAR keyframes, pose noise, lambda_init): window 3 starts far off with little damping, so that trials are
# rejected; windows 1, 4 and 6 carry the LiDAR edge over 3, 6 and 4 keyframes
SOLVE_WINDOWS = [(40, 2, 3, 150, 0, (0.5, 0.05), 0.0), (41, 3, 4, 250, 3, (0.5, 0.05), 0.0), (42, 4, 3, 400, 0, (0.3, 0.03), 100.0),
                 (32, 5, 4, 200, 0, (40, 4.0), 1e-6), (44, 6, 5, 300, 6, (0.5, 0.05), 0.0), (45, 7, 3, 350, 0, (1.0, 0.1), 0.0),
                 (46, 8, 4, 400, 4, (0.2, 0.02), 0.0), (47, 3, 6, 150, 0, (0.5, 0.05), 0.0)]
GROUP = 1


def bits(a):
    return np.ascontiguousarray(a).tobytes()


class World:
    """The synthetic windows and the hand-made graphs' world behind ONE store: (problem dicts for the solve entry, cam)."""

    def __init__(self, pkg, synthetic):
        self.views, self.problems, self.cam = [], [], None
        for seed, n_opt, n_fix, n_points, n_cloud, noise, lam in SOLVE_WINDOWS:
            self.add_window(synthetic, synthetic.ba_window(seed, n_opt=n_opt, n_fix=n_fix, n_points=n_points, pose_noise=noise), n_cloud, lambda_init=lam)
        self.add_window(synthetic, synthetic.ba_window(50, n_opt=30, n_fix=3, n_points=150), 0)
        self.wide = self.problems.pop()                                                 # 30 free keyframes: beyond the device range
        self.sigma = self._sigma                                                        # the windows' own table; the hand-made graphs take it too
        self.hand_at = len(self.views)                                                  # the slots of ba_window_cases.WORLD
        self.views += [v if v is not None else K.make_view(np.random.default_rng(1), 8) for v in K.WORLD]

    def add_window(self, synthetic, w, n_cloud, **kw):
        views, pr, sigma = K.from_window(dict(w, win_pose=list(range(len(w["poses"]) - n_cloud, len(w["poses"])))))
        self._sigma = sigma
        assert self.cam is None or np.array_equal(self.cam, w["cam"])
        self.cam = np.asarray(w["cam"], np.float64)
        pr = dict(pr, kf_slot=pr["kf_slot"] + len(self.views), **kw)
        if n_cloud:
            rows = list(range(len(w["poses"]) - n_cloud, len(w["poses"])))
            got = synthetic.ba_window_clouds(w, rows, n_points=800)
            pr.update(clouds=[got[rows.index(k)] if k in rows else None for k in range(len(w["poses"]))], Tcl7=synthetic.TCL7, weight=1.0)
        self.views += views
        self.problems.append(pr)
        return pr

    def hand(self, *args, **kw):
        pr = K.hand(*args, **kw)
        return dict(pr, kf_slot=pr["kf_slot"] + self.hand_at)

    def store(self, pkg):
        s = pkg.KeyframeStore(len(self.views), max(len(v["keys"]) for v in self.views))
        s.put_batch(list(range(len(self.views))), self.views, K.BOUNDS, n_levels=K.N_LEVELS)
        return s


@pytest.fixture(scope="module")
def world(pkg, synthetic):
    w = World(pkg, synthetic)
    with w.store(pkg) as s:
        yield w, s


def two_step(pkg, store, world, problems):
    """tc2li_ba_window_batch, tc2li_local_bundle_adjustment_batch_group over the windows that are not ABORTED, tc2li_ba_window_outliers"""
    gathered = pkg.ba_window_batch(problems, world.sigma, store=store)
    alive = [i for i, g in enumerate(gathered) if g["status"] == ref.OK]
    windows = []
    for i in alive:
        g, p = gathered[i], problems[i]
        w = dict(poses=g["poses7"], fixed=g["fixed"], points=g["points3"], edges=g["edges"], iterations=p.get("iterations", 10),
                 lambda_init=p.get("lambda_init", 0.0), stop_flag=p.get("stop_flag"))
        if p.get("clouds") is not None and g["n_lidar"]:
            w.update(win_pose=g["lidar_pose_index"], clouds=[p["clouds"][g["pose_row"][k]] for k in g["lidar_pose_index"]], Tcl7=p["Tcl7"],
                     weight=p.get("weight", 1.0))
        windows.append(w)
    out = [dict(g, result=0, n_erase=0) for g in gathered]
    if not windows:
        return out
    batch = pkg.capi.BaBatch(windows, world.cam)
    batch.run_group(GROUP)
    for k, i in enumerate(alive):
        poses, pts, chi2, dpos, stats, lstats = batch.result(k)
        g = gathered[i]
        rc = int(batch.results[k])
        erase = pkg.ba_window_outliers(g["edges"], chi2, dpos, np.zeros(len(pts), np.uint8)) if rc >= 0 else np.zeros((0, 2), np.int32)
        out[i].update(result=rc, poses7=poses.copy(), points3=pts.copy(), chi2=chi2.copy(), depth_positive=dpos.copy(), erase=erase, n_erase=len(erase),
                      stats={f: getattr(stats, f) for f, _ in stats._fields_}, lidar_stats={f: getattr(lstats, f) for f, _ in lstats._fields_}, batch=batch)
    return out


def assert_same(got, want, what):
    """one window of the solve entry against the two-step path: bytes"""
    assert got["result"] == want["result"] and got["status"] == want["status"], (what, got["result"], want["result"])
    if want["status"] != ref.OK:
        return
    for k in ("pose_row", "fixed", "point_row", "lidar_pose_index"):
        assert np.array_equal(got[k], want[k]), (what, k)
    if got["edges"] is not None:
        assert bits(got["edges"]) == bits(want["edges"]), (what, "edges")
    for k in ("poses7", "points3"):
        assert bits(got[k]) == bits(want[k]), (what, k, np.abs(got[k] - want[k]).max())
    if want["result"] < 0:
        assert got["n_erase"] == 0
        return
    for f in ("iterations", "trials", "n_free_poses", "initial_chi2", "final_chi2", "final_lambda"):
        assert bits(np.float64(getattr(got["stats"], f))) == bits(np.float64(want["stats"][f])), (what, f, getattr(got["stats"], f), want["stats"][f])
    for f in ("n_planes", "hessian_evaluations", "residual", "chi2"):
        assert bits(np.float64(getattr(got["lidar_stats"], f))) == bits(np.float64(want["lidar_stats"][f])), (what, f)
    if got["chi2"] is not None:
        assert bits(got["chi2"]) == bits(want["chi2"]) and bits(got["depth_positive"]) == bits(want["depth_positive"]), (what, "chi2 / depth")
    assert got["n_erase"] == want["n_erase"] and np.array_equal(got["erase"], want["erase"]), (what, "erase", got["n_erase"], want["n_erase"])


def solve(pkg, store, world, problems, **kw):
    return pkg.ba_window_solve_batch(problems, world.sigma, store, world.cam, group=GROUP, **kw)


def test_solve_equals_the_three_calls(pkg, world):
    w, s = world
    want = two_step(pkg, s, w, w.problems)
    got = solve(pkg, s, w, w.problems)
    for i, (g, t) in enumerate(zip(got, want)):
        assert_same(g, t, "window %d" % i)
    assert all(t["result"] > 0 for t in want)
    assert want[3]["stats"]["trials"] > want[3]["stats"]["iterations"]                # the window that starts far off rejects trials
    assert [t["n_lidar"] for t in want] == [0, 3, 0, 0, 6, 0, 4, 0] and all(t["lidar_stats"]["n_planes"] > 0 for t in want if t["n_lidar"])
    moved = [np.abs(g["poses7"] - h["poses7"]).max() for g, h in zip(got, pkg.ba_window_batch(w.problems, w.sigma, store=s))]
    assert min(moved) > 0 and sum(t["n_erase"] for t in want) > 10                     # the optimiser moved something, the rule found something
    order = np.random.default_rng(11).permutation(len(w.problems))
    again = solve(pkg, s, w, [w.problems[i] for i in order])
    for k, i in enumerate(order):
        assert_same(again[k], want[i], "window %d in the shuffled batch" % i)
        assert bits(again[k]["poses7"]) == bits(got[i]["poses7"]) and bits(again[k]["points3"]) == bits(got[i]["points3"])


def contract_batch(w, synthetic):
    kfs = [dict(slot=0, id=1, holds=[0]), dict(slot=1, id=2, holds=[0])]
    aborted = w.hand(kfs, [dict(obs={0: 0, 1: 0})], 0, [1])
    only_initial = w.hand([dict(slot=0, id=5, holds=[0, 1]), dict(slot=1, id=6), dict(slot=2, id=7)],
                          [dict(obs={0: 0, 1: 1, 2: 2}), dict(obs={0: 1, 1: 2, 2: 3})], 0, [], init=5)
    no_edge = w.hand([dict(slot=0, id=1, holds=[0, 1]), dict(slot=1, id=2), dict(slot=2, id=3)],
                     [dict(obs={0: 0, 1: 1, 2: 2}), dict(obs={0: -1, 1: -1})], 0, [])
    many = w.hand([dict(slot=0, id=10 + i, holds=[0, 1] if i == 0 else []) for i in range(258)],
                  [dict(obs={k: 1 for k in range(257)}), dict(obs={0: 2, 257: 3})], 0, [])
    return [w.problems[0], aborted, only_initial, w.problems[1], no_edge, many, w.problems[5]]


def test_contract_cases_in_one_batch(pkg, world, synthetic):
    w, s2 = world
    batch = contract_batch(w, synthetic) + [w.wide]
    want = two_step(pkg, s2, w, batch)
    got = solve(pkg, s2, w, batch)
    assert [t["result"] for t in want][1] == 0 and want[1]["status"] == ref.ABORTED
    assert want[2]["result"] >= 0 and want[2]["stats"]["n_free_poses"] == 0           # the only local keyframe is the initial one: fixed
    assert want[4]["result"] == S.INVALID and want[5]["result"] == S.INVALID and want[7]["result"] > 0 and want[7]["stats"]["n_free_poses"] == 30
    for i, (g, t) in enumerate(zip(got, want)):
        assert_same(g, t, "contract case %d" % i)
    alone = solve(pkg, s2, w, [w.problems[0], w.problems[1], w.problems[5]])        # the neighbours' results do not depend on the company
    for k, i in enumerate((0, 3, 6)):
        assert bits(alone[k]["poses7"]) == bits(got[i]["poses7"]) and bits(alone[k]["points3"]) == bits(got[i]["points3"])
    one = solve(pkg, s2, w, [w.problems[4]])                                        # a batch of one: the one-window path in both forms
    assert_same(one[0], two_step(pkg, s2, w, [w.problems[4]])[0], "a batch of one")


def test_pose_capacity_one_short(pkg, world):
    import tc2li_slam_amd.capi as capi
    w, s = world
    gathered = pkg.ba_window_batch(w.problems[:3], w.sigma, store=s)
    batch = [dict(p) for p in w.problems[:3]]
    batch[1]["pose_capacity"] = len(gathered[1]["pose_row"]) - 1
    seen = {}
    real = capi.pack_ba_window_solve_problems

    def spy(problems_, fill=0):
        arr, outs, keep = real(problems_, fill)
        seen["outs"] = outs
        return arr, outs, keep
    capi.pack_ba_window_solve_problems = spy
    try:
        with pytest.raises(pkg.Tc2liError) as e:
            solve(pkg, s, w, batch, fill=T.SENTINEL)
    finally:
        capi.pack_ba_window_solve_problems = real
    assert e.value.code == T.CAPACITY
    for o, g in zip(seen["outs"], gathered):
        assert o["counts"].tolist()[3:6] == [len(g["pose_row"]), len(g["point_row"]), len(g["edges"])]
        for k in ("pose_row", "poses7_out", "fixed", "point_row", "points3_out", "lidar_pose_index", "erase_pose", "erase_point", "n_erase", "edge_depth_positive"):
            assert (o[k] == np.array(T.SENTINEL).astype(o[k].dtype)).all(), k             # no list, no BA result
        assert (o["edge_chi2"] == float(T.SENTINEL)).all() and o["stats"].iterations == 0


def test_edges_null_and_stop_flag(pkg, world):
    w, s = world
    pick = [w.problems[i] for i in (1, 2, 6)]
    want = two_step(pkg, s, w, pick)
    with_edges = solve(pkg, s, w, pick)
    without = solve(pkg, s, w, [dict(p, want_edges=False, want_chi2=False) for p in pick])
    for i, (a, b, t) in enumerate(zip(with_edges, without, want)):
        assert_same(a, t, "edges asked for, window %d" % i)
        assert_same(b, t, "edges == NULL, window %d" % i)
        assert b["edges"] is None and b["chi2"] is None and bits(a["edges"]) == bits(t["edges"])
    stop = np.ones(1, np.uint8)                                                        # *pbStopFlag already set
    stopped = [dict(p, stop_flag=stop) if i != 1 else p for i, p in enumerate(pick)]
    want = two_step(pkg, s, w, stopped)
    got = solve(pkg, s, w, stopped)
    for i, (g, t) in enumerate(zip(got, want)):
        assert_same(g, t, "stop flag set, window %d" % i)
    assert want[0]["result"] < want[1]["result"] and want[2]["result"] < want[1]["result"]
