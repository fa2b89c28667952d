"""The hand-made keyframes of mapping_cases.py are what they claim to be, shown on the CPU before any GPU sees them: every targeted
quantity keeps its margin from its gate, cases cannot interact, mapping_ref.py (float64, written from the reference text) produces the
outcome each case names, and the oracle decides as mapping_ref does.  A random rotated scene with a known answer checks mapping_ref
itself.  test_mapping_gates_gpu.py runs the product on the same dicts."""
import numpy as np
import pytest

import mapping_cases as mc
import mapping_ref as ref


@pytest.fixture(scope="module")
def env(synthetic):
    return mc.Env(synthetic)


def ref_sft(env, scene, j, **kw):
    return ref.search_for_triangulation(scene.current, scene.neighbours[j], env.cam4, env.sf, env.sg, **kw)


def ref_points(env, scene, **kw):
    return ref.create_new_map_points(scene.current, scene.neighbours, env.cam4, env.mb, env.bf, env.sf, env.sg, **kw)


def oracle_points(oracle, env, scene, **kw):
    return oracle.create_new_map_points(scene.current, scene.neighbours, env.cam4, env.mb, env.bf, env.sf, env.sg, **kw)


def ref_fuse(env, s, run):
    return ref.fuse_search(s.kf["keys"], s.kf["descriptors"], s.kf["u_right"], s.bounds, s.pose7, env.cam4, env.bf, env.sf, env.isg, env.logsf, s.points,
                           s.valid_for(run), th=mc.FUSE_RUNS[run])


@pytest.mark.parametrize("world", mc.FUSE_WORLDS)
def test_margins_and_isolation(env, world):
    scenes = []
    if world in mc.WORLDS:
        scenes = [s for s, _ in list(mc.pair_scenes(env, world).values()) + list(mc.point_scenes(env, world).values())]
    n = 0
    for s in scenes:
        assert mc.nodes_disjoint(s), s.cases[0]["name"]
        for c in s.cases:
            assert mc.margins_ok(c), (world, c["name"], c["gates"])
            n += len(c["gates"])
    for bounds in (mc.BOUNDS0, mc.BOUNDS1, mc.BOUNDS2):
        s = mc.fuse_scene(env, world, bounds)
        assert mc.fuse_isolated(s)
        origin = [c["name"] for c in s.cases if c["name"].startswith("window_origin")]
        assert len(origin) == {mc.BOUNDS0: 0, mc.BOUNDS1: 1, mc.BOUNDS2: 2}[bounds]
        for c in s.cases:
            assert mc.margins_ok(c), (world, c["name"], c["gates"])
        assert np.all((s.kf["u_right"] >= 0) == np.array([r["ur"] >= 0 for r in s.b.rows]))
    assert world == "turned" or n >= 50, n
    assert mc.current_pose7("turned")[3] < 0 and mc.neighbour_pose7("rotated", mc.current_pose7("rotated"), mc.SIDE2)[3] < 0


@pytest.mark.parametrize("world", mc.WORLDS)
def test_search_for_triangulation_cases(env, oracle, world):
    for name, (scene, runs) in mc.pair_scenes(env, world).items():
        for run, kw in runs.items():
            for j in range(len(scene.neighbours)):
                n, match = ref_sft(env, scene, j, **kw)
                mc.check_matches(scene, run, j, match)
                on, om = oracle.search_for_triangulation(scene.current, scene.neighbours[j], env.cam4, env.sf, env.sg, **kw)
                assert on == n and np.array_equal(om, match), (world, name, run, j)


def test_same_pose_has_a_zero_fundamental_matrix_only_in_the_identity_world(env):
    for world in mc.WORLDS:
        s = mc.same_pose_scene(env, world)
        assert np.array_equal(s.current["pose7"], s.neighbours[0]["pose7"])
    R, t = ref.pose_Rt(mc.current_pose7("identity"))
    assert np.array_equal(R, np.eye(3)) and np.all(t - R @ R.T @ t == 0)


@pytest.mark.parametrize("world", mc.WORLDS)
def test_create_new_map_points_cases(env, oracle, world):
    kinds = set()
    for name, (scene, runs) in mc.point_scenes(env, world).items():
        for run, kw in runs.items():
            idx, x3 = ref_points(env, scene, **kw)
            mc.check_points(scene, run, idx)
            oidx, ox3 = oracle_points(oracle, env, scene, **kw)
            assert np.array_equal(oidx, idx), (world, name, run)
            assert np.allclose(ox3, x3, rtol=1e-4, atol=1e-5), (world, name, run)
            kinds |= {(int(r[3]), int(r[1])) for r in idx}
    assert {(0, 0), (1, 1)} <= kinds


def test_the_unprojection_sides_differ(env):
    """both_stereo_neighbour_depth_smaller: un-projecting from the neighbour would give another point, further than any tolerance here"""
    for world in mc.WORLDS:
        s = mc.cnmp_scene(env, world)
        c = [c for c in s.cases if c["name"].startswith("both_stereo")][0]
        nb = s.neighbours[c["nb"]]
        z2 = float(nb["depth"][c["idx2"][0]])
        assert z2 < 0.85 * env.project(s.nb_pose[c["nb"]], c["X"])[1] and z2 < float(s.current["depth"][c["idx1"]])


@pytest.mark.parametrize("bounds", [mc.BOUNDS0, mc.BOUNDS1, mc.BOUNDS2])
@pytest.mark.parametrize("world", mc.FUSE_WORLDS)
def test_fuse_cases(env, oracle, world, bounds):
    s = mc.fuse_scene(env, world, bounds)
    for run in mc.FUSE_RUNS:
        nf, bi, bd = ref_fuse(env, s, run)
        wi, wd = s.expected(run)
        for c, a, b, x, y in zip(s.cases, bi, bd, wi, wd):
            assert (a, b) == (x, y), (world, run, c["name"], (a, b), (x, y))
        assert nf == (wi >= 0).sum() > 1
        if bounds == mc.BOUNDS0:      # the oracle's entry takes cols, rows: bounds that start at 0
            of, oi, od = oracle.fuse_search(s.kf["keys"], s.kf["descriptors"], s.kf["u_right"], mc.W, mc.H, s.pose7, env.cam4, env.bf, env.sf, env.isg, env.logsf,
                                            s.points, s.valid_for(run), th=mc.FUSE_RUNS[run])
            assert of == nf and np.array_equal(oi, bi) and np.array_equal(od, bd), (world, run)


def test_compaction_problem_is_the_prescribed_one(env, oracle):
    s = mc.compaction_problem(env)
    assert len(s.current["keys"]) == 130 and len(s.neighbours) == 70
    idx, x3 = ref_points(env, s)
    got = np.full(130, -1)
    got[idx[:, 0]] = idx[:, 1]
    assert np.array_equal(got, s.first)
    owners = set(idx[:, 1])
    assert {0, 3, 4, 63, 64, 69} <= owners and len(owners) <= 70 - 8
    assert sum(len(nb["keys"]) == 0 for nb in s.neighbours) >= 3
    mine = idx[idx[:, 1] == 4, 0]
    assert (mine < 64).any() and ((mine >= 64) & (mine < 128)).any() and (mine >= 128).any()
    assert not set(mc.COMPACT_SKIPPED) & owners and all(len(s.neighbours[j]["keys"]) > 0 for j in mc.COMPACT_SKIPPED)
    oidx, ox3 = oracle_points(oracle, env, s)
    assert np.array_equal(oidx, idx) and np.allclose(ox3, x3, rtol=1e-4, atol=1e-5)


def test_reference_on_a_random_rotated_scene_with_a_known_answer(env):
    s, X, index = mc.random_scene(env)
    idx, x3 = ref_points(env, s)
    assert len(idx) > 120 and (idx[:, 3] == 0).sum() > 10 and (idx[:, 3] == 1).sum() > 20
    point_of = {int(i): p for p, i in enumerate(index[0])}
    for row, got in zip(idx, x3):
        p = point_of[int(row[0])]
        assert index[1 + row[1]][p] == row[2]
        assert np.linalg.norm(got - X[p]) <= mc.true_point_tolerance(env, s, X[p], row[1]), (row, np.linalg.norm(got - X[p]))
    for k in range(4):
        kf, pts = mc.random_fuse_points(env, s, X, index, k)
        nf, bi, bd = ref.fuse_search(kf["keys"], kf["descriptors"], kf["u_right"], mc.BOUNDS0, kf["pose7"], env.cam4, env.bf, env.sf, env.isg, env.logsf, pts,
                                     np.ones(len(pts), np.uint8))
        hit = bi >= 0
        assert hit.sum() > 40 and np.array_equal(bi[hit], index[k][hit]) and np.all(bd[hit] == 0)


def test_oracle_deviation_is_the_recorded_one(env, oracle):
    """the largest deviation of the oracle's triangulated points from mapping_ref on the well-conditioned records: the figure behind
    mapping_cases.ORACLE_TRI_DEVIATION (printed; the constant may not lie below it)"""
    worst, n = 0.0, 0
    scenes = [sr for w in mc.WORLDS for sr in mc.point_scenes(env, w).values()] + [(mc.compaction_problem(env), {"default": {}}), (mc.random_scene(env)[0], {"default": {}})]
    for scene, runs in scenes:
        for kw in runs.values():
            idx, x3 = ref_points(env, scene, **kw)
            oidx, ox3 = oracle_points(oracle, env, scene, **kw)
            assert np.array_equal(oidx, idx)
            keep = mc.well_conditioned(scene, idx, x3)
            worst, n = max(worst, mc.deviation(ox3[keep], x3[keep])), n + int(keep.sum())
    print("oracle against mapping_ref over %d triangulated records: %.3e" % (n, worst))
    assert n > 100 and worst <= mc.ORACLE_TRI_DEVIATION
    assert worst >= mc.ORACLE_TRI_DEVIATION / 4, "the recorded figure is stale: measured %.3e" % worst


# ---- each of these gates decides a case: mapping_ref with the gate taken out gives another answer ------------------------------------------
def ref_without(old, new):
    """mapping_ref with one piece of its text replaced"""
    import inspect
    src = inspect.getsource(ref)
    assert src.count(old) == 1, old
    ns = {}
    exec(compile(src.replace(old, new), "mapping_ref_mutant", "exec"), ns)
    return ns


def fuse_with(ns, env, s, run):
    return ns["fuse_search"](s.kf["keys"], s.kf["descriptors"], s.kf["u_right"], s.bounds, s.pose7, env.cam4, env.bf, env.sf, env.isg, env.logsf, s.points,
                             s.valid_for(run), th=mc.FUSE_RUNS[run])


@pytest.mark.parametrize("world", mc.FUSE_WORLDS)
def test_only_the_depth_test_keeps_the_point_behind_the_camera_out(env, world):
    ns = ref_without("if z < 0.0:", "if False:")
    for bounds in (mc.BOUNDS0, mc.BOUNDS1):
        s = mc.fuse_scene(env, world, bounds)
        k = [c["name"] for c in s.cases].index("behind_the_camera_z_negative")
        _, bi, bd = fuse_with(ns, env, s, "th3")
        assert (bi[k], bd[k]) == (s.cases[k]["keys"][0], 0) and ref_fuse(env, s, "th3")[1][k] == -1


@pytest.mark.parametrize("world", mc.WORLDS)
def test_only_the_cosine_test_drops_the_head_on_rays(env, world):
    ns = ref_without("cos_rays < cos_s and cos_rays > 0 and", "cos_rays < cos_s and")
    s = mc.cnmp_scene(env, world)
    c = [c for c in s.cases if c["name"] == "mono_mono_rays_head_on_only_the_cos_gate_drops_it"][0]
    idx, x3 = ns["create_new_map_points"](s.current, s.neighbours, env.cam4, env.mb, env.bf, env.sf, env.sg)
    row = idx[idx[:, 0] == c["idx1"]]
    assert len(row) == 1 and tuple(row[0]) == (c["idx1"], mc.FACING, c["idx2"][0], 0)
    assert np.linalg.norm(x3[idx[:, 0] == c["idx1"]][0] - c["X"]) < 1e-4      # both depths positive, both reprojections exact: the point itself
    assert c["idx1"] not in ref_points(env, s)[0][:, 0]


@pytest.mark.parametrize("world", mc.FUSE_WORLDS)
def test_the_window_needs_the_grid_origin(env, world):
    for old, new, bounds, name in (("(u - min_x + r) * inv_w", "(u + r) * inv_w", mc.BOUNDS1, "window_origin_x_keypoint_in_the_last_cell"),
                                   ("(u - min_x + r) * inv_w", "(u + r) * inv_w", mc.BOUNDS2, "window_origin_x_keypoint_in_the_last_cell"),
                                   ("(v - min_y + r) * inv_h", "(v + r) * inv_h", mc.BOUNDS2, "window_origin_y_keypoint_in_the_last_cell")):
        s = mc.fuse_scene(env, world, bounds)
        k = [c["name"] for c in s.cases].index(name)
        assert fuse_with(ref_without(old, new), env, s, "th1.5")[1][k] == -1 and ref_fuse(env, s, "th1.5")[1][k] == s.cases[k]["keys"][0]


def test_the_baseline_needs_the_camera_centres(env):
    ns = ref_without("np.linalg.norm(O2 - O1) < mb", "np.linalg.norm(t2 - t1) < mb")
    for factor in (0.9, 1.1):
        s = mc.baseline_scene(env, "rotated", factor)
        got = ns["create_new_map_points"](s.current, s.neighbours, env.cam4, env.mb, env.bf, env.sf, env.sg)[0]
        assert len(got) != len(ref_points(env, s)[0]), factor
