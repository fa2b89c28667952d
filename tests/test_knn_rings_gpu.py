"""Directed tests of the LiDAR 5-NN search (k_knn_plane / k_knn_hard, lidar_kernels.hip) against a brute force (knn_ref.py)
and the oracle.  The state is the identity, so world == body exactly; `sqdist`, `nearest` and `nfound` are compared with the
brute force over LidarMap.points(), `selected` / `normvec` (and `nearest` again) with oracle.feature_extraction on a tree built
from the same points.  Every case asserts from the brute force alone that the 5th and 6th distances differ (the tie cases
excepted), so the expected neighbours do not depend on an order the search is free to choose.

How a query travels (read from the kernels): pass 1 scans the cubes of ring 1 and ring 2 around the query's cell with four
lanes; a cube's answer is taken when it holds five points and the fifth is closer than the nearest face of the cube
(knn_complete).  Queries left over go to k_knn_hard, one wavefront each: ring 4 if n_points / 3 > 81, ring 8 if > 289, ring 16
if > 1089, ring 32 if > 4225, each with the same test, and at last every entry of the map.

Not covered on purpose: maps whose points lie closer together than the voxel filter leaves them (0.5 m) in bulk -- the hand-made
points here are few -- and distances below 1e-3 m^2, where the search's 1e-10 tolerance would make unequal distances tie."""
import numpy as np
import pytest

import knn_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
IDENT = np.concatenate([np.eye(3).ravel(), np.zeros(3), np.eye(3).ravel(), np.zeros(3)]).astype(np.float64)
POINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("pad0", "<f4"), ("normal_x", "<f4"), ("normal_y", "<f4"), ("normal_z", "<f4"),
                        ("pad1", "<f4"), ("intensity", "<f4"), ("curvature", "<f4"), ("pad2", "<f4"), ("pad3", "<f4")])


def P(xyz):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    a = np.zeros(len(xyz), POINT_DTYPE)
    a["x"], a["y"], a["z"], a["pad0"] = xyz[:, 0], xyz[:, 1], xyz[:, 2], 1
    return a


@pytest.fixture(scope="module")
def fe(pkg):
    assert pkg.device_count() >= 1
    f = pkg.LidarFrontEnd(max_points_per_scan=4096, max_scans=1)
    yield f
    f.close()


def xyz_rows(a):
    return np.ascontiguousarray(np.stack([a["x"], a["y"], a["z"]], -1))


def xyz_bytes(a):
    return xyz_rows(a).tobytes()


def check_map(pkg, fe, oracle, gmap, queries, ties="none"):
    """One search of `queries` in `gmap` against the brute force and the oracle; returns (result, reference indices).
    ties: "none" -- the 5th and 6th distances differ everywhere; "x" -- ties are decided by x (still one right answer);
    "free" -- ties with equal x: only the distances are defined."""
    pts = gmap.points() if gmap.size() else P(np.zeros((0, 3)))
    d5, idx, nfound, gap = knn_ref.knn5(pts, queries)
    if ties == "none":
        assert (gap > 0).all(), "the reference itself must be unambiguous"
    got = fe.feature_extraction(gmap, queries, IDENT)
    assert xyz_bytes(got["world"]) == xyz_bytes(queries)
    assert np.array_equal(got["nfound"], nfound)
    assert np.array_equal(got["sqdist"], d5)
    tree = oracle.KdTree(pts)
    want = oracle.feature_extraction(tree, queries, IDENT)
    assert np.array_equal(want["nfound"], nfound)
    if ties != "free":
        for j in range(5):
            ok = idx[:, j] >= 0
            assert xyz_bytes(got["nearest"][ok, j]) == xyz_bytes(pts[idx[ok, j]]), "neighbour %d" % j
        assert got["nearest"].tobytes() == want["nearest"].tobytes()
        assert np.array_equal(got["selected"], want["selected"])
        sel = want["selected"] > 0
        for name in ("x", "y", "z", "intensity"):
            assert np.array_equal(got["normvec"][name][sel], want["normvec"][name][sel]), name
    return got, idx


def check(pkg, fe, oracle, map_points, queries, ties="none"):
    gmap = pkg.LidarMap()
    assert gmap.Build(map_points) == len(map_points)
    try:
        return check_map(pkg, fe, oracle, gmap, queries, ties)
    finally:
        gmap.close()


# ---- 1. a closer point just outside the cube ------------------------------------------------------------------------
CELL0 = np.array([-7.0, 12.0, 3.0])  # the query's cell (a negative cell index among them)
DECOYS = (0.25, 0.35, 0.45, 0.6, 0.75)


def ballast(n, origin):
    """n points on a 0.75 m lattice: the bulk of the map, far from everything else."""
    i = np.arange(n)
    return np.stack([i % 24, (i // 24) % 24, i // 576], 1) * 0.75 + 0.3 + np.asarray(origin)


def ring_layout(ring, axis, sign, near, corner, n_points):
    """-> (map, query, expected indices).  The query sits at offset 0.9 (sign +) or 0.1 (sign -) along `axis` in its cell and 0.5
    (corner: 0.9) along the others.  Five decoys lie on the far side at ring + 0.25 ... ring + 0.75 cells along the axis: in the
    outermost cells of the ring's cube.  One more point lies on the near side, ring + 0.15 cells away (near) -- just beyond the face
    of that cube, 0.1 cells past it, and closer than every decoy -- or ring + 1.0 cells away (not near: farther than every decoy).
    The rest of the n_points is ballast 50 cells away along another axis."""
    off = np.full(3, 0.9 if corner else 0.5)
    off[axis] = 0.9 if sign > 0 else 0.1
    q = CELL0 + off
    e = np.zeros(3); e[axis] = sign
    jitter = np.zeros((5, 3))
    jitter[:, (axis + 1) % 3] = (-0.25, 0.0, -0.1, -0.3, -0.2)  # not collinear; every decoy stays in the query's row of cells
    jitter[:, (axis + 2) % 3] = (0.0, -0.2, -0.3, -0.05, -0.15)
    decoys = q - e * (ring + np.array(DECOYS))[:, None] + jitter
    outside = q + e * (ring + (0.15 if near else 1.0))
    far = np.zeros(3); far[(axis + 1) % 3] = 50.0
    pts = np.concatenate([decoys, outside[None], ballast(n_points - 6, CELL0 + far - np.array([9.0, 9.0, 8.0]) * (np.arange(3) != (axis + 1) % 3))])
    expected = [5, 0, 1, 2, 3] if near else [0, 1, 2, 3, 4]
    return P(pts), P(q), expected


# n_points per ring: n_points / 3 just above the threshold of the ring itself, and of the next ring where that changes who answers
RING_CASES = [(1, 3 * 82), (2, 3 * 82), (4, 3 * 82), (4, 3 * 290), (8, 3 * 290), (8, 3 * 1090), (16, 3 * 1090), (16, 3 * 4226),
              (16, 3 * 1089 + 2), (32, 3 * 4226)]


@pytest.mark.parametrize("ring,n_points", RING_CASES)
def test_closer_point_just_outside_the_cube(pkg, fe, oracle, ring, n_points):
    """ring_layout for the three axes, both directions, the far twin, and the query near a cell corner.

    Why ring r decides.  All six hand-made points differ from the query's cell by r or r + 1 cells along the axis, the ballast by
    40 or more, so every cube of a ring below r is empty: t.b4 is the empty candidate and knn_complete returns false at its first
    line.  The cube of ring r holds exactly the five decoys (cell c -+ r along the axis) and not the sixth point (cell c +- (r + 1)).
    Its nearest face is (r + 0.1) cells from the query, the fifth decoy more than (r + 0.75): knn_complete must say no, and the search
    goes on to the next ring that n_points / 3 enables (2r holds all six; (r + 0.8)^2 < 0.999 (2r + 0.1)^2, so it completes) or to
    the whole map.  A completeness test that is too generous at ring r keeps the five decoys and loses the closer sixth point.
    Rings 4 to 32 run only when n_points / 3 > (2r + 1)^2, which n_points = 3 ((2r + 1)^2 + 1) just satisfies; (16, 3 * 1089 + 2) is
    just below, so ring 16 is skipped there and the whole map must give the same answer."""
    assert ring < 4 or (n_points // 3 > (2 * ring + 1) ** 2) == (n_points != 3 * 1089 + 2)
    variants = [(axis, sign, near, False) for axis in range(3) for sign in (1, -1) for near in (True, False)] + [(0, 1, True, True), (0, 1, False, True)]
    for axis, sign, near, corner in variants:
        m, q, expected = ring_layout(ring, axis, sign, near, corner, n_points)
        cells = np.floor(np.stack([m["x"], m["y"], m["z"]], 1)[:6]).astype(int) - CELL0.astype(int)
        assert np.all(np.abs(cells[:5, axis]) == ring) and abs(cells[5, axis]) == ring + 1 and np.all(np.delete(cells, axis, 1) == 0)
        rest = np.floor(np.stack([m["x"], m["y"], m["z"]], 1)[6:]) - CELL0
        assert np.abs(rest).max(axis=1).min() >= 40, "the ballast stays out of every ring"
        got, idx = check(pkg, fe, oracle, m, q)
        assert list(idx[0]) == expected, (axis, sign, near, corner)
        assert got["nfound"][0] == 5


# ---- 2. the whole-map fallback --------------------------------------------------------------------------------------
def far_queries(rng, lo, hi, n, dist=(35.0, 60.0)):
    """Queries more than 34 cells (Chebyshev) from the box [lo, hi]: the cube of ring 32 around them holds no point."""
    q = rng.uniform(lo, hi, (n, 3))
    axis, side = rng.integers(0, 3, n), rng.integers(0, 2, n)
    d = rng.uniform(*dist, n)
    q[np.arange(n), axis] = np.where(side == 1, hi[axis] + d, lo[axis] - d)
    return q


def test_whole_map_fallback(pkg, fe, oracle):
    """A 13 000-point map (n_points / 3 = 4333: all four rings are tried and are empty) and queries farther than 34 cells from all
    of it, next to queries inside it: the fallback walks all n_slots entries, the segments' spare room (index -1) included.  The
    same after Delete_Point_Boxes (which rebuilds the grid over the remaining points) and after an in-place map_incremental: scan
    points on the centres of occupied voxels replace the points there (a tombstone where the old point stood until its segment is
    rewritten), others fill the emptied box.  Expected values come from points() each time."""
    rng = np.random.default_rng(21)
    lo, hi = np.array([-20.0, 5.0, -2.0]), np.array([16.0, 41.0, 8.0])
    xyz = rng.uniform(lo, hi, (13000, 3))
    q = P(np.concatenate([far_queries(rng, lo, hi, 150), rng.uniform(lo, hi, (100, 3))]))
    gmap = pkg.LidarMap()
    gmap.Build(P(xyz))
    check_map(pkg, fe, oracle, gmap, q)
    removed = gmap.Delete_Point_Boxes(np.array([[-10, 10, -2, -4, 22, 8], [5, 5, 0, 9, 15, 3]], f32))
    assert 500 < removed < 1000 and gmap.size() == 13000 - removed
    check_map(pkg, fe, oracle, gmap, q)
    updates = gmap.stats()["grid_updates"]
    centres = (np.floor(xyz[rng.choice(13000, 300, replace=False)] / 0.5) + 0.5) * 0.5
    scan = P(np.concatenate([centres, rng.uniform(np.array([-9.5, 10.5, -1.5]), np.array([-4.5, 21.5, 7.5]), (300, 3))]))
    fe.feature_extraction(gmap, scan, IDENT)
    before = gmap.points()
    n, n_add, _ = gmap.map_incremental(fe, 0, IDENT, ekf_inited=False)
    assert n_add == 600 and gmap.stats()["grid_updates"] == updates + 1, "the insertion was meant to happen in place"
    after = gmap.points()
    assert len(set(map(bytes, xyz_rows(before))) - set(map(bytes, xyz_rows(after)))) > 100, "points were meant to be replaced"
    check_map(pkg, fe, oracle, gmap, q)
    gmap.close()


@pytest.mark.parametrize("n_map", [5, 4, 1])
def test_tiny_maps(pkg, fe, oracle, n_map):
    """Maps of 5, 4 and 1 points: nfound < 5 leaves -1 / 0 in the empty slots, near and far queries alike."""
    rng = np.random.default_rng(22)
    m = P(rng.uniform(-3, 3, (n_map, 3)))
    q = P(np.concatenate([rng.uniform(-3, 3, (40, 3)), rng.uniform(-80, 80, (60, 3))]))
    got, idx = check(pkg, fe, oracle, m, q)
    assert np.all(got["nfound"] == n_map)
    assert np.all(got["sqdist"][:, n_map:] == 0)


# ---- 3. segments and the edges of the box ---------------------------------------------------------------------------
def lattice_map(rng, nx=40, ny=20, nz=6):
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    return g + rng.uniform(0.1, 0.9, g.shape), np.array([nx, ny, nz], float)


def lattice_queries(rng, size):
    lines = [np.stack([np.arange(-3, size[0] + 3) + 0.37, np.full(int(size[0]) + 6, y), np.full(int(size[0]) + 6, z)], 1)
             for y, z in ((3.5, 2.5), (10.3, 0.2), (19.8, 5.7))]
    outside = []
    for d in np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3):
        if not d.any():
            continue
        for dist in (0.6, 1.7, 5.5, 12.5, 20.5):  # within one and two cells of the box, inside its margin (8, 8, 2 cells), beyond it
            base = np.where(d > 0, size, np.where(d < 0, 0.0, rng.uniform(0.2, 0.8, 3) * size))
            outside.append(base + d * dist)
    return np.concatenate(lines + [np.array(outside)])


def test_segments_and_box_edges(pkg, fe, oracle):
    """A jittered lattice of 40 x 20 x 6 cells, one point a cell.  Queries in every cell of three lines along x: cx - x0 takes every
    value mod 16, so the runs of rings 1 and 2 lie in one 16-cell segment or straddle two at every possible place.  Queries outside
    the box beyond all six faces, twelve edges and eight corners, 0.6 to 20.5 m out: clipped xa / xb, rows outside the grid, and
    xa > xb once the cube has left the grid altogether."""
    rng = np.random.default_rng(23)
    pts, size = lattice_map(rng)
    check(pkg, fe, oracle, P(pts), P(lattice_queries(rng, size)))


# ---- 4. 1.5 m cells -------------------------------------------------------------------------------------------------
def test_coarse_cells(pkg, fe, oracle):
    """Three clusters spanning 300 x 300 x 50 m: more than 4 Mi one-metre cells, so grid_geometry takes 1.5 m cells."""
    rng = np.random.default_rng(24)
    centres = np.array([[5.0, 5.0, 5.0], [295.0, 5.0, 45.0], [5.0, 295.0, 40.0]])
    pts = np.concatenate([c + rng.uniform(-5, 5, (300, 3)) for c in centres])
    q = np.concatenate([c + rng.uniform(-6, 6, (40, 3)) for c in centres] +
                       [rng.uniform([0, 0, 0], [300, 300, 50], (60, 3)), rng.uniform([-40, -40, -20], [340, 340, 70], (60, 3))])
    m = P(pts)
    gmap = pkg.LidarMap()
    gmap.Build(m)
    check_map(pkg, fe, oracle, gmap, P(q))

    def cells(cell):
        inv = f32(1.0) / f32(cell)
        dims = [int(np.floor(m[a].max() * inv)) - int(np.floor(m[a].min() * inv)) + 1 for a in "xyz"]
        with_margin = [d + 2 * k for d, k in zip(dims, (8, 8, 2))]
        return int(np.prod(dims)), int(np.prod(with_margin))
    assert cells(1.0)[0] > 4 << 20 and cells(1.5)[1] <= 4 << 20
    assert gmap.stats()["cells"] == cells(1.5)[1], "the grid was meant to have 1.5 m cells"
    gmap.close()


# ---- 5. ties across lanes -------------------------------------------------------------------------------------------
def tie_layout(reach, same_x, n_points):
    """Coordinates in multiples of 1/8, so every distance is exact.  Four distinct nearest points, then two candidates for fifth place at
    exactly the same distance, `reach` cells away in rows y - reach and y + reach of the grid (runs of different lanes)."""
    q = np.array([10.5, 10.5, 10.5])
    s = float(reach)
    first = q + np.array([[0.125, 0, s - 1], [0, 0.25, 1 - s], [-0.375, s - 1, 0.375], [0.5, 1 - s, -0.125]])
    a = q + np.array([0.25, s, 0.0])
    b = q + np.array([0.25 if same_x else -0.25, -s, 0.0])
    sixth = q + np.array([0.0, 0.0, s + 0.75])
    pts = np.concatenate([first, a[None], b[None], sixth[None], ballast(n_points - 7, q + np.array([-9.0, 50.0, -8.0]))])
    return P(pts), P(q)


@pytest.mark.parametrize("reach,n_points", [(1, 3 * 82), (6, 3 * 290)])
def test_ties_across_lanes(pkg, fe, oracle, reach, n_points):
    """Two candidates for fifth place at exactly equal distance with different x, held by different lanes (reach 1: the quad of pass 1;
    reach 6: the wavefront of ring 8): the smaller x is kept, as in the oracle and the brute force.  With equal x only the distances
    are defined and compared."""
    m, q = tie_layout(reach, False, n_points)
    d = knn_ref.sqdist(m, (q["x"][0], q["y"][0], q["z"][0]))
    assert d[4] == d[5] and m["x"][5] < m["x"][4] and np.all(d[:4] < d[4]) and d[6] > d[4]
    got, idx = check(pkg, fe, oracle, m, q, ties="x")
    assert idx[0, 4] == 5
    m, q = tie_layout(reach, True, n_points)
    check(pkg, fe, oracle, m, q, ties="free")


# ---- 6. the 5 m^2 gate ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dy,selected", [(2.0, 1), (2.0625, 0)])
def test_five_square_metre_gate(pkg, fe, oracle, dy, selected):
    """Four neighbours about 0.25 m away and a fifth at offset (1, dy, 0), all on the plane z = 3 (not through the origin): a squared
    distance of exactly 5 passes `!(d > 5)` and the plane is accepted, 5.2539 fails it."""
    q = np.array([10.5, 20.5, 3.0])
    pts = q + np.array([[0.25, 0, 0], [0, 0.2578125, 0], [-0.265625, 0, 0], [0, -0.2734375, 0], [1.0, dy, 0]])
    m = P(np.concatenate([pts, ballast(300, q + np.array([-9.0, 50.0, -8.0]))]))
    d = knn_ref.sqdist(m, q)
    assert (d[4] == 5.0) == (selected == 1) and np.all(d[:4] < 0.08)
    tree = oracle.KdTree(m)
    assert oracle.feature_extraction(tree, P(q), IDENT)["selected"][0] == selected
    got, idx = check(pkg, fe, oracle, m, P(q))
    assert got["selected"][0] == selected and list(idx[0]) == [0, 1, 2, 3, 4]


# ---- 7. every kind of query in one launch ---------------------------------------------------------------------------
def test_mixed_launch(pkg, fe, oracle):
    """One map (a lattice, a ring-16 layout 120 cells away from it, 13 000 points in all) and one call whose queries end in pass 1, in
    the rings of k_knn_hard and in the whole map: the same results as one call per kind."""
    rng = np.random.default_rng(27)
    pts, size = lattice_map(rng)
    ring_map, ring_q, expected = ring_layout(16, 0, 1, True, False, 13000 - len(pts))
    shift = np.array([0.0, 150.0, 0.0])
    ring_xyz = np.stack([ring_map["x"], ring_map["y"], ring_map["z"]], 1) + shift
    m = P(np.concatenate([pts, ring_xyz]))
    groups = [P(lattice_queries(rng, size)[:160]),
              P(np.stack([ring_q["x"], ring_q["y"], ring_q["z"]], 1) + shift),
              P(far_queries(rng, np.array([-20.0, -20.0, -10.0]), np.array([60.0, 230.0, 20.0]), 60, dist=(40.0, 70.0)))]
    gmap = pkg.LidarMap()
    gmap.Build(m)
    parts = [check_map(pkg, fe, oracle, gmap, g)[0] for g in groups]
    assert list(knn_ref.knn5(m, groups[1])[1][0] - len(pts)) == expected
    whole, _ = check_map(pkg, fe, oracle, gmap, np.concatenate(groups))
    for name in ("sqdist", "nearest", "nfound", "selected", "normvec"):
        assert whole[name].tobytes() == np.concatenate([p[name] for p in parts]).tobytes(), name
    gmap.close()
