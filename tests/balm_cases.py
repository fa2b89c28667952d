"""LiDAR windows with a chosen number of planes, for test_balm_many_planes.py (host extraction, no GPU) and test_balm_many_planes_gpu.py.

synthetic.ba_window_clouds gives a ground plane and two walls around every keyframe: a few hundred planes at most.  The reference's clouds
are whole scans cut into 1 m root voxels (kVoxelSize), thousands of planes per window.  tiled_clouds() lays one flat sheet of 1 m cells
over the window, one root voxel per cell; a voxel then holds W * per_cell points and becomes a plane when that is more than 15 (kMinPoints)
and lambda0 / lambda1 < 1/36 -- with the default noise of 4 mm against a spread of 0.26 m in x and y the ratio is ~2e-4, so the number of
planes is the number of cells.  with_standard() adds the standard clouds to it: a ground plane and two walls around every keyframe, so a
second normal direction, and planes that some keyframes do not see (n_i = 0 slots of their clusters); with z = 3.5 the sheet shares no voxel
with them.

ROWS names the windows the tests use (the plane counts are asserted by every test that relies on them, from lidar_planes_host):

  name      W  cells x per_cell                            clouds         pose_noise       planes
  p2047     2  2047 x 9                                    tiles, z=-1.7  (0, 0)           2047   k_balm_residual_total, below its limit
  p2048     2  2048 x 9                                    tiles, z=-1.7  (0, 0)           2048   the most the batched kernels take
  p2049     2  2049 x 9                                    tiles, z=-1.7  (0, 0)           2049   k_balm_residual_planes + k_balm_sum; extraction overflow
  w3_over   3  2300 x 6                                    + standard     (0.02, 0.002)    > 2048 the lock-step batch's and the engine's window over the limit
  w2_two    2  8300 x 9, width 128, origin (-64, -40)      + standard     (0.02, 0.002)    > 8192 small Hessian form, two passes of the plane-batch loop
  w8_two    8  4200 x 2, width 80, origin (-40, -30)       + standard     (0.02, 0.002)    > 4096 large Hessian form, two passes
  w7        7  300 x 3                                     + standard     (0.02, 0.002)    < 2048 widest window of the small form (1008 of 1024 items)
  w8        8  300 x 3                                     + standard     (0.02, 0.002)    < 4096 narrowest window of the large form
  w1        1  300 x 20                                    tiles          (0, 0)           0      a plane must be seen from two keyframes

Every builder's result is made once per session and must not be written to."""
import functools

import numpy as np

ROWS = {
    "p2047": dict(W=2, n_cells=2047, per_cell=9, z=-1.7, standard=False, pose_noise=(0.0, 0.0)),
    "p2048": dict(W=2, n_cells=2048, per_cell=9, z=-1.7, standard=False, pose_noise=(0.0, 0.0)),
    "p2049": dict(W=2, n_cells=2049, per_cell=9, z=-1.7, standard=False, pose_noise=(0.0, 0.0)),
    "w3_over": dict(W=3, n_cells=2300, per_cell=6, standard=True, pose_noise=(0.02, 0.002)),
    "w2_two": dict(W=2, n_cells=8300, per_cell=9, width=128, origin=(-64, -40), standard=True, pose_noise=(0.02, 0.002)),
    "w8_two": dict(W=8, n_cells=4200, per_cell=2, width=80, origin=(-40, -30), standard=True, pose_noise=(0.02, 0.002)),
    "w7": dict(W=7, n_cells=300, per_cell=3, standard=True, pose_noise=(0.02, 0.002)),
    "w8": dict(W=8, n_cells=300, per_cell=3, standard=True, pose_noise=(0.02, 0.002)),
    "w1": dict(W=1, n_cells=300, per_cell=20, standard=False, pose_noise=(0.0, 0.0)),
}


def _synthetic():
    from tc2li_slam_amd import synthetic   # (importable once the package is loaded: the tests' pkg / synthetic fixtures)
    return synthetic


def _quat_R(q):
    x, y, z, w = [float(v) for v in q]
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def lidar_poses(poses7, win):
    """[(R, p)] of T_wl = T_cw^-1 * T_cl for the rows `win` of poses7 (qx, qy, qz, qw, tx, ty, tz = Tcw), in float64."""
    tcl7 = _synthetic().TCL7
    Rcl, tcl = _quat_R(tcl7[:4]), tcl7[4:].astype(np.float64)
    out = []
    for k in win:
        Rcw, tcw = _quat_R(poses7[k][:4]), np.asarray(poses7[k][4:], np.float64)
        out.append((Rcw.T @ Rcl, Rcw.T @ (tcl - tcw)))
    return out


def tiled_clouds(poses7, win, n_cells, per_cell, width=64, origin=(-32, -32), z=3.5, noise=0.004, seed=0):
    """One cloud per keyframe of `win` (float32 [n_cells * per_cell, 3], each in its keyframe's own LiDAR frame): a flat sheet at height
    z in the LiDAR frame of win[0].  Cell c has its corner at (c % width + origin[0], c // width + origin[1]) and takes per_cell points per
    keyframe, x and y = corner + U(0.05, 0.95), height z + N(0, noise): every cell lies inside one 1 m root voxel."""
    rng = np.random.default_rng([0xBA1A, seed])
    Twl = lidar_poses(poses7, win)
    R0, p0 = Twl[0]
    c = np.repeat(np.arange(n_cells), per_cell)
    corner = np.stack([c % width + origin[0], c // width + origin[1]], 1).astype(np.float64)
    clouds = []
    for R, p in Twl:
        X0 = np.concatenate([corner + rng.uniform(0.05, 0.95, corner.shape), z + rng.normal(0, noise, (len(c), 1))], 1)
        Xw = X0 @ R0.T + p0
        clouds.append(((Xw - p) @ R).astype(np.float32))   # R^T (Xw - p)
    return clouds


def with_standard(w, win, tiles, n_points=1200, seed=3):
    """The tiles plus synthetic.ba_window_clouds(w, win, n_points, seed=seed), keyframe by keyframe (the standard clouds first)."""
    std = _synthetic().ba_window_clouds(w, win, n_points=n_points, seed=seed)
    return [np.concatenate([s, t]) for s, t in zip(std, tiles)]


def window(W, pose_noise):
    """(w, win): synthetic.ba_window(3, n_opt=max(6, W), n_fix=4, n_points=300, pose_noise) and its last W poses, newest first."""
    return _window(W, tuple(pose_noise))


@functools.lru_cache(maxsize=None)
def _window(W, pose_noise):
    w = _synthetic().ba_window(3, n_opt=max(6, W), n_fix=4, n_points=300, pose_noise=pose_noise)
    last = len(w["poses"]) - 1
    return w, list(range(last, last - W, -1))


@functools.lru_cache(maxsize=None)
def row(name):
    """(w, win, clouds) of ROWS[name]."""
    r = dict(ROWS[name])
    W, standard, pose_noise = r.pop("W"), r.pop("standard"), r.pop("pose_noise")
    w, win = window(W, pose_noise)
    clouds = tiled_clouds(w["poses_true"], win, **r)
    if standard:
        clouds = with_standard(w, win, clouds)
    return w, win, clouds


@functools.lru_cache(maxsize=None)
def host_planes(name):
    """(clusters, coe) of the row from the library's host extraction (no GPU)."""
    from tc2li_slam_amd import capi
    w, win, clouds = row(name)
    return capi.lidar_planes_host(w["poses"], win, clouds, _synthetic().TCL7)


def empty_slots(clusters):
    """How many planes have a keyframe that does not see them (n_i = 0)."""
    return int((clusters[:, :, 9] == 0).any(1).sum())
