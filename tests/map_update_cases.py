"""Generators for the tests of the map update of IMU initialisation (tc2li_apply_scaled_rotation_batch, tc2li_gba_map_correction_batch) and
the comparison by bit pattern.  The shapes are the smallest at which the kernels can still go wrong: a keyframe tile is 64 lanes, a point
tile 256, the walk's workgroup 256."""
import numpy as np

F = np.float32
FILL = 0xA5   # the byte the outputs are prefilled with: what a call leaves untouched keeps it


def assert_equal(got, want, what=""):
    """Equality of two output dicts: float arrays by bit pattern, except that a NaN equals a NaN."""
    assert set(got) == set(want), (what, sorted(got), sorted(want))
    for k in sorted(want):
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, "%s: %s is %s %s, expected %s %s" % (what, k, g.dtype, g.shape, w.dtype, w.shape)
        if g.dtype == np.float32:
            same = (g.view(np.uint32) == w.view(np.uint32)) | (np.isnan(g) & np.isnan(w))
        else:
            same = g == w
        if not same.all():
            at = np.argwhere(~same)[0]
            raise AssertionError("%s: %s differs in %d of %d entries, first at %s: %r against %r" % (what, k, (~same).sum(), same.size, tuple(at), g[tuple(at)], w[tuple(at)]))


def random_poses(rng, n, spread=5.0):
    """[n, 7]: quaternions normalised in float32 (unit only up to rounding, as a caller's are), translations within `spread`"""
    q = rng.normal(size=(n, 4)).astype(F)
    q = q / np.sqrt((q * q).sum(axis=1, dtype=F))[:, None]
    return np.concatenate([q, rng.uniform(-spread, spread, (n, 3)).astype(F)], axis=1).astype(F)


IDENTITY7 = np.array([0, 0, 0, 1, 0, 0, 0], F)


# ---- Map::ApplyScaledRotation ---------------------------------------------------------------------------------------------------------
def rot_problem(seed, n_kf, obs_counts, s=1.0, scaled_vel=0, has_tcb=0, bad=(), T7=None, poses=None):
    """n_kf keyframes and one point per entry of obs_counts with that many observations, in keyframes drawn without repetition and in
    random order (mObservations iterates in address order: any order can occur); the reference keyframe is one of the observers."""
    rng = np.random.default_rng(seed)
    n = len(obs_counts)
    assert max(list(obs_counts) + [0]) <= n_kf
    off = np.zeros(n + 1, np.int32)
    off[1:] = np.cumsum(obs_counts)
    obs_kf = np.concatenate([rng.permutation(n_kf)[:c] for c in obs_counts] + [np.zeros(0, np.int64)]).astype(np.int32)
    ref = np.array([obs_kf[off[i] + rng.integers(0, c)] if c else -1 for i, c in enumerate(obs_counts)], np.int32).reshape(n)
    point_bad = np.zeros(n, np.uint8)
    point_bad[list(bad)] = 1
    return dict(T7=random_poses(rng, 1, 2.0)[0] if T7 is None else np.asarray(T7, F), s=F(s), scaled_vel=scaled_vel, has_tcb=has_tcb,
                tcb3=rng.uniform(-0.1, 0.1, 3).astype(F), last_level_scale=F(1.2) ** 7,
                kf_pose7=random_poses(rng, n_kf) if poses is None else np.asarray(poses, F).reshape(n_kf, 7), kf_vel=rng.normal(size=(n_kf, 3)).astype(F),
                point_pos=rng.uniform(-8, 8, (n, 3)).astype(F), point_bad=point_bad, obs_offsets=off, obs_kf=obs_kf, point_ref_kf=ref,
                point_ref_level_scale=(F(1.2) ** rng.integers(0, 8, n)).astype(F))


def identity_problem():
    """Tyw = identity and s = 1: the positions come back as they are.  Keyframe 0 has the identity rotation, so its camera centre is exactly
    -t, and point 0 lies exactly there: its normal is 0 / 0."""
    pr = rot_problem(77, 5, [1, 3, 0, 5, 2, 2], s=1.0, scaled_vel=1, has_tcb=1, bad=[4], T7=IDENTITY7)
    pr["kf_pose7"][0] = [0, 0, 0, 1, 0.5, -1.25, 2.0]
    pr["point_pos"][0] = [-0.5, 1.25, -2.0]
    pr["obs_kf"][0] = 0
    pr["point_ref_kf"][0] = 0
    return pr


EDGE_COUNTS = [0, 1, 2, 63, 64, 65]


def rot_family():
    rng = np.random.default_rng(3)
    many = [int(c) for c in rng.integers(1, 7, 600)]
    return [
        rot_problem(1, 0, []),                                                              # nothing at all
        rot_problem(2, 1, [1], s=7.3, has_tcb=1),                                           # one keyframe, one point
        rot_problem(3, 65, EDGE_COUNTS + [4, 3], s=0.1, scaled_vel=0, has_tcb=1, bad=[6]),  # a wavefront and one keyframe; a bad point with observations
        rot_problem(4, 300, EDGE_COUNTS + [200] + many, s=7.3, scaled_vel=1, has_tcb=0, bad=[9, 300]),   # several tiles of keyframes and of points
        identity_problem(),
        rot_problem(5, 3, [2] * 10, s=1.0, scaled_vel=1),
        rot_problem(6, 7, []),                                                              # keyframes without points
        rot_problem(7, 0, [0, 0, 0], s=0.1, bad=[1]),                                       # points without keyframes
    ]


def tiny_rot_problems(n):
    return [rot_problem(1000 + i, 1 + i % 4, [(i + j) % (2 + i % 4) for j in range(i % 5)], s=[0.1, 1.0, 7.3][i % 3], scaled_vel=i & 1, has_tcb=(i >> 1) & 1,
                        bad=[0] if i % 5 == 4 else []) for i in range(n)]


# ---- the map update after a global BA -----------------------------------------------------------------------------------------------------
def gba_problem(seed, parent, origin, n_points=0, in_gba=None, bad=None, imu=None, vel_set=None, points=None):
    """A tree given by parent / origin rows; flags default to: nothing in the GBA but the origins, nothing bad, everything inertial with a
    velocity.  points: rows (bad, in_gba, ref_kf) placed first; n_points more are drawn."""
    rng = np.random.default_rng(seed)
    parent, origin = np.asarray(parent, np.int32), np.asarray(origin, np.uint8)
    n = len(parent)
    flag = lambda v, d: np.full(n, d, np.uint8) if v is None else np.asarray(v, np.uint8)
    rows = list(points or [])
    for _ in range(n_points):
        kind = rng.integers(0, 8)
        rows.append((int(kind == 0), int(kind in (1, 2)), int(rng.integers(0, n)) if n else -1))
    if n == 0:
        rows = [(b, g, -1) for b, g, _ in rows if b or g]
    m = len(rows)
    return dict(kf_parent=parent, kf_origin=origin, kf_bad=flag(bad, 0), kf_in_gba=origin.copy() if in_gba is None else np.asarray(in_gba, np.uint8),
                kf_imu=flag(imu, 1), kf_vel_set=flag(vel_set, 1), kf_pose7=random_poses(rng, n), kf_gba_pose7=random_poses(rng, n),
                kf_bef_gba_pose7=random_poses(rng, n), kf_vel=rng.normal(size=(n, 3)).astype(F), kf_gba_vel=rng.normal(size=(n, 3)).astype(F),
                kf_bias=rng.normal(size=(n, 6)).astype(F), kf_gba_bias=rng.normal(size=(n, 6)).astype(F),
                point_bad=np.array([r[0] for r in rows], np.uint8).reshape(m), point_in_gba=np.array([r[1] for r in rows], np.uint8).reshape(m),
                point_pos=rng.uniform(-8, 8, (m, 3)).astype(F), point_gba_pos=rng.uniform(-8, 8, (m, 3)).astype(F),
                point_ref_kf=np.array([r[2] for r in rows], np.int32).reshape(m))


def chain(depth):
    """origin 0, then `depth` keyframes each the child of the one before -> (parent, origin)"""
    return np.arange(-1, depth, dtype=np.int32), np.array([1] + [0] * depth, np.uint8)


def random_tree(seed, n, n_origins=1):
    """keyframe k > n_origins hangs below a random earlier one, then the rows are shuffled: a parent may come after its child"""
    rng = np.random.default_rng(seed)
    parent = np.array([-1] * n_origins + [int(rng.integers(0, k)) for k in range(n_origins, n)], np.int32)
    order = rng.permutation(n)                       # new row of old row k is order[k]
    new_parent = np.full(n, -1, np.int32)
    new_parent[order] = np.where(parent >= 0, order[np.maximum(parent, 0)], -1)
    origin = np.zeros(n, np.uint8)
    origin[order[:n_origins]] = 1
    return new_parent, origin


def random_gba_problem(seed, n, n_points, n_origins=1):
    rng = np.random.default_rng(seed + 50000)
    parent, origin = random_tree(seed, n, n_origins)
    return gba_problem(seed, parent, origin, n_points, in_gba=(rng.random(n) < 0.4) | (origin > 0), bad=rng.random(n) < 0.05, imu=rng.random(n) < 0.8,
                       vel_set=rng.random(n) < 0.8)


def cut_tree():
    """0 origin - 1 - 2 - 3(bad) - 4 - 5;  6 hangs below 1 and is in the GBA, 7 below 6;  8 has no parent and is no origin (unreachable, not
    in the GBA);  9 likewise but flagged;  10 below 9.  Points: one per way through :1399-1425."""
    parent = [-1, 0, 1, 2, 3, 4, 1, 6, -1, -1, 9]
    origin = [1] + [0] * 10
    in_gba = [1, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0]
    bad = [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0]
    points = [(0, 1, 2),      # in the GBA
              (0, 0, 2),      # its reference keyframe got the flag from the walk
              (0, 0, 6),      # ... had it already and kept its own pose
              (0, 0, 4),      # ... lies below the bad child: not reached, not flagged -> untouched
              (0, 0, 8),      # ... unreachable, not flagged -> untouched
              (0, 0, 9),      # ... unreachable but flagged -> moves by kf_bef_gba_pose7 and its unchanged pose
              (1, 0, 2), (1, 1, -1),   # bad
              (0, 1, -1)]
    return gba_problem(21, parent, origin, 0, in_gba=in_gba, bad=bad, imu=[1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1], vel_set=[1, 1, 0, 1, 1, 1, 1, 0, 1, 1, 1],
                       points=points)


def gba_family():
    star = ([-1] + [0] * 20, [1] + [0] * 20)
    two = ([-1, -1, 0, 1, 1, 3], [1, 1, 0, 0, 0, 0])
    return [
        gba_problem(10, [-1], [1], points=[(0, 1, 0), (0, 0, 0), (1, 0, 0)]),               # the origin only
        gba_problem(11, *two, n_points=12),
        gba_problem(12, *star, n_points=30, bad=[1] + [0] * 20),                            # a bad origin is walked all the same
        gba_problem(13, *chain(1), n_points=5),
        gba_problem(14, *chain(2), n_points=5),
        gba_problem(15, *chain(70), n_points=80),                                           # more rounds than a wavefront has lanes
        gba_problem(16, *chain(300), n_points=300),                                         # ... than a workgroup has threads; two point tiles
        cut_tree(),
        gba_problem(17, [], [], points=[(1, 0, -1), (0, 1, -1)]),                           # points without keyframes
        gba_problem(18, [], []),
        random_gba_problem(19, 500, 700, n_origins=2),
        gba_problem(20, *chain(5), n_points=10, in_gba=[0] * 6),                            # an origin outside the GBA still hands on its stored pose
    ]


def tiny_gba_problems(n):
    return [random_gba_problem(2000 + i, 1 + i % 6, i % 4) for i in range(n)]
