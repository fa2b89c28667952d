"""The product on the hand-made keyframes of mapping_cases.py (test_mapping_cases.py shows on the CPU what each case is): k_tri_search,
k_tri_points, k_fuse_search through the single-keyframe entries, their batch forms and k_new_points_compact through a KeyframeStore.
Decisions must equal mapping_ref.py (float64, from the reference text) and the oracle exactly, un-projected points the oracle bit for
bit; triangulated points meet the existing bar against the oracle and mapping_cases.PRODUCT_TRI_BAR against mapping_ref."""
import numpy as np
import pytest

import mapping_cases as mc
import mapping_ref as ref

ERR_CAPACITY = -5


@pytest.fixture(scope="module")
def env(synthetic):
    return mc.Env(synthetic)


def product_points(pkg, env, scene, **kw):
    return pkg.capi.create_new_map_points(scene.current, scene.neighbours, env.cam5, env.mb, env.sf, env.sg, **kw)


def ref_points(env, scene, **kw):
    return ref.create_new_map_points(scene.current, scene.neighbours, env.cam4, env.mb, env.bf, env.sf, env.sg, **kw)


def oracle_points(oracle, env, scene, **kw):
    return oracle.create_new_map_points(scene.current, scene.neighbours, env.cam4, env.mb, env.bf, env.sf, env.sg, **kw)


def check_points_three_ways(scene, got, want, owant, what):
    idx, x3 = got
    assert np.array_equal(idx, want[0]) and np.array_equal(idx, owant[0]), what
    stereo = idx[:, 3] == 1
    assert np.array_equal(x3[stereo], owant[1][stereo]), what                                    # un-projections: bit for bit
    assert np.allclose(x3[~stereo], owant[1][~stereo], rtol=1e-4, atol=1e-5), what              # triangulations: the existing bar
    assert np.allclose(x3[stereo], want[1][stereo], rtol=1e-5, atol=1e-5), what                  # and float32 of the float64 answer
    keep = mc.well_conditioned(scene, idx, want[1])
    dev = mc.deviation(x3[keep], want[1][keep])
    print("%s: %d triangulated records, product against mapping_ref %.3e (bar %.3e)" % (what, keep.sum(), dev, mc.PRODUCT_TRI_BAR))
    assert dev <= mc.PRODUCT_TRI_BAR, (what, dev)


@pytest.mark.gpu
@pytest.mark.parametrize("world", mc.WORLDS)
def test_search_for_triangulation_cases(pkg, oracle, env, world):
    for name, (scene, runs) in mc.pair_scenes(env, world).items():
        for run, kw in runs.items():
            for j in range(len(scene.neighbours)):
                n, match = pkg.capi.search_for_triangulation(scene.current, scene.neighbours[j], env.cam5, env.sf, env.sg, **kw)
                mc.check_matches(scene, run, j, match)
                wn, wm = ref.search_for_triangulation(scene.current, scene.neighbours[j], env.cam4, env.sf, env.sg, **kw)
                on, om = oracle.search_for_triangulation(scene.current, scene.neighbours[j], env.cam4, env.sf, env.sg, **kw)
                assert n == wn == on and np.array_equal(match, wm) and np.array_equal(match, om), (world, name, run, j)
    # under a rotated pose t12 of two equal poses is rounding noise: the float64 reference has no say, product and oracle share the float32 arithmetic
    s = mc.same_pose_scene(env, world)
    got = pkg.capi.search_for_triangulation(s.current, s.neighbours[0], env.cam5, env.sf, env.sg)
    want = oracle.search_for_triangulation(s.current, s.neighbours[0], env.cam4, env.sf, env.sg)
    assert got[0] == want[0] and np.array_equal(got[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("world", mc.WORLDS)
def test_create_new_map_points_cases(pkg, oracle, env, world):
    for name, (scene, runs) in mc.point_scenes(env, world).items():
        for run, kw in runs.items():
            got = product_points(pkg, env, scene, **kw)
            mc.check_points(scene, run, got[0])
            check_points_three_ways(scene, got, ref_points(env, scene, **kw), oracle_points(oracle, env, scene, **kw), (world, name, run))


def single_fuse(pkg, env, s, run):
    return pkg.capi.fuse_search(s.kf["keys"], s.kf["descriptors"], s.kf["u_right"], mc.W, mc.H, s.pose7, env.cam4, env.bf, env.sf, env.isg, env.logsf, s.points,
                                s.valid_for(run), th=mc.FUSE_RUNS[run])


def ref_fuse(env, s, run):
    return ref.fuse_search(s.kf["keys"], s.kf["descriptors"], s.kf["u_right"], s.bounds, s.pose7, env.cam4, env.bf, env.sf, env.isg, env.logsf, s.points,
                           s.valid_for(run), th=mc.FUSE_RUNS[run])


def check_fuse(s, run, got, what):
    wi, wd = s.expected(run)
    for c, a, b, x, y in zip(s.cases, got[1], got[2], wi, wd):
        assert (a, b) == (x, y), (what, c["name"], (a, b), (x, y))
    assert got[0] == (wi >= 0).sum()


@pytest.mark.gpu
@pytest.mark.parametrize("world", mc.FUSE_WORLDS)
def test_fuse_cases(pkg, oracle, env, world):
    s = mc.fuse_scene(env, world, mc.BOUNDS0)
    for run in mc.FUSE_RUNS:
        got = single_fuse(pkg, env, s, run)
        check_fuse(s, run, got, (world, run))
        want = ref_fuse(env, s, run)
        owant = oracle.fuse_search(s.kf["keys"], s.kf["descriptors"], s.kf["u_right"], mc.W, mc.H, s.pose7, env.cam4, env.bf, env.sf, env.isg, env.logsf, s.points,
                                   s.valid_for(run), th=mc.FUSE_RUNS[run])
        for w in (want, owant):
            assert got[0] == w[0] and np.array_equal(got[1], w[1]) and np.array_equal(got[2], w[2]), (world, run)


@pytest.mark.gpu
def test_batch_entries_equal_the_single_calls(pkg, env):
    """every CreateNewMapPoints scene of both worlds as one batch, every Fuse scene as items of one call: record for record the single calls"""
    jobs = [(w, name, scene, run, kw) for w in mc.WORLDS for name, (scene, runs) in mc.point_scenes(env, w).items() for run, kw in runs.items()]
    scenes = []
    for job in jobs:
        if not any(job[2] is s for s in scenes):
            scenes.append(job[2])
    fuse = [mc.fuse_scene(env, w, b) for b in (mc.BOUNDS0, mc.BOUNDS1, mc.BOUNDS2) for w in mc.FUSE_WORLDS]
    first_slot, kfs, bounds = {}, [], []
    for s in scenes:
        first_slot[id(s)] = len(kfs)
        kfs += [s.current] + s.neighbours
    fuse_slot = len(kfs)
    kfs += [f.kf for f in fuse]
    bounds = [mc.BOUNDS0] * fuse_slot + [f.bounds for f in fuse]
    with pkg.KeyframeStore(len(kfs), 256) as store:
        store.put_batch(list(range(len(kfs))), kfs, bounds)
        problems = []
        for w, name, s, run, kw in jobs:
            at = first_slot[id(s)]
            all_kf = [s.current] + s.neighbours
            problems.append(dict(current=at, neighbours=list(range(at + 1, at + len(all_kf))), poses7=np.stack([k["pose7"] for k in all_kf]),
                                 has_point=[k["has_point"] for k in all_kf], **kw))
        out = pkg.capi.create_new_map_points_batch(store, problems, env.cam5, env.mb, env.sf, env.sg)
        assert sum(len(o[0]) for o in out) > 60
        for (w, name, s, run, kw), o in zip(jobs, out):
            one = product_points(pkg, env, s, **kw)
            assert np.array_equal(o[0], one[0]) and o[1].tobytes() == one[1].tobytes(), (w, name, run)
            mc.check_points(s, run, o[0])
        # Fuse: one item per (scene, run); the scenes with bounds that do not start at 0 have no single call and no oracle entry: mapping_ref
        items, points, valid, at = [], [], [], 0
        for k, f in enumerate(fuse):
            for run in mc.FUSE_RUNS:
                items.append(dict(keyframe=fuse_slot + k, first_point=at, first_valid=len(valid), n_points=len(f.points), pose7=f.pose7, th=mc.FUSE_RUNS[run]))
                valid += list(f.valid_for(run))
            points.append(f.points)
            at += len(f.points)
        nf, bi, bd = pkg.capi.fuse_search_batch(store, items, env.cam4, env.bf, env.sf, env.isg, env.logsf, np.concatenate(points), np.array(valid, np.uint8))
        k = 0
        for f in fuse:
            for run in mc.FUSE_RUNS:
                r = slice(items[k]["first_valid"], items[k]["first_valid"] + items[k]["n_points"])
                got = (nf[k], bi[r], bd[r])
                check_fuse(f, run, got, (f.world, f.bounds, run))
                want = ref_fuse(env, f, run)
                assert got[0] == want[0] and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (f.world, f.bounds, run)
                if f.bounds == tuple(float(b) for b in mc.BOUNDS0):
                    one = single_fuse(pkg, env, f, run)
                    assert got[0] == one[0] and np.array_equal(got[1], one[1]) and np.array_equal(got[2], one[2]), (f.world, run)
                k += 1


@pytest.mark.gpu
def test_compaction_beyond_four_neighbours_and_one_scan_round(pkg, oracle, env):
    """k_new_points_compact with 130 keypoints (64 + 64 + 2) and 70 neighbours (64 + 6; up to 18 per wavefront): records, their order, the
    counts per neighbour and n_points against mapping_ref; one record short of room is the capacity error with the full count"""
    s = mc.compaction_problem(env)
    want, owant = ref_points(env, s), oracle_points(oracle, env, s)
    all_kf = [s.current] + s.neighbours
    with pkg.KeyframeStore(len(all_kf), 256) as store:
        store.put_batch(list(range(len(all_kf))), all_kf, mc.BOUNDS0)
        problem = dict(current=0, neighbours=list(range(1, len(all_kf))), poses7=np.stack([k["pose7"] for k in all_kf]), has_point=[k["has_point"] for k in all_kf])
        got = pkg.capi.create_new_map_points_batch(store, [problem], env.cam5, env.mb, env.sf, env.sg)[0]
        check_points_three_ways(s, got, want, owant, "compaction")
        first = np.full(mc.COMPACT_KEYS, -1)
        first[got[0][:, 0]] = got[0][:, 1]
        assert np.array_equal(first, s.first)
        assert np.array_equal(np.bincount(got[0][:, 1], minlength=mc.COMPACT_NEIGHBOURS), np.bincount(want[0][:, 1], minlength=mc.COMPACT_NEIGHBOURS))
        one = product_points(pkg, env, s)
        assert np.array_equal(got[0], one[0]) and got[1].tobytes() == one[1].tobytes()
        n = len(want[0])
        rc, n_points, recs = pkg.capi.create_new_map_points_batch(store, [problem], env.cam5, env.mb, env.sf, env.sg, capacities=[n], raw=True)
        assert rc == n and list(n_points) == [n] and len(recs[0]) == n
        rc, n_points, recs = pkg.capi.create_new_map_points_batch(store, [problem], env.cam5, env.mb, env.sf, env.sg, capacities=[n - 1], raw=True)
        assert rc == ERR_CAPACITY and list(n_points) == [n]
        assert np.array_equal(recs[0]["idx1"], want[0][:n - 1, 0]) and np.array_equal(recs[0]["neighbour"], want[0][:n - 1, 1])


@pytest.mark.gpu
def test_random_rotated_scene_against_the_true_points(pkg, oracle, env):
    s, X, index = mc.random_scene(env)
    got = product_points(pkg, env, s)
    check_points_three_ways(s, got, ref_points(env, s), oracle_points(oracle, env, s), "random scene")
    point_of = {int(i): p for p, i in enumerate(index[0])}
    assert len(got[0]) > 120
    for row, x in zip(*got):
        p = point_of[int(row[0])]
        assert index[1 + row[1]][p] == row[2]
        assert np.linalg.norm(x.astype(np.float64) - X[p]) <= mc.true_point_tolerance(env, s, X[p], row[1]), (row, np.linalg.norm(x - X[p]))
    for k in range(4):
        kf, pts = mc.random_fuse_points(env, s, X, index, k)
        nf, bi, bd = pkg.capi.fuse_search(kf["keys"], kf["descriptors"], kf["u_right"], mc.W, mc.H, kf["pose7"], env.cam4, env.bf, env.sf, env.isg, env.logsf, pts,
                                          np.ones(len(pts), np.uint8))
        hit = bi >= 0
        assert hit.sum() > 40 and np.array_equal(bi[hit], index[k][hit]) and np.all(bd[hit] == 0)
        of, oi, od = oracle.fuse_search(kf["keys"], kf["descriptors"], kf["u_right"], mc.W, mc.H, kf["pose7"], env.cam4, env.bf, env.sf, env.isg, env.logsf, pts,
                                        np.ones(len(pts), np.uint8))
        assert nf == of and np.array_equal(bi, oi) and np.array_equal(bd, od)
