"""The many-plane LiDAR windows of balm_cases.py through the library's host extraction (tc2li_host_lidar_planes; no GPU): the generator gives
the plane counts the GPU tests of test_balm_many_planes_gpu.py rely on, and at 2049 planes -- one more than the batched kernels take, the
window BalmTerm::finish_cut extracts on the host -- the host's planes are the oracle's."""
import numpy as np
import pytest

import balm_cases


@pytest.mark.parametrize("name,want", [("p2047", 2047), ("p2048", 2048), ("p2049", 2049)])
def test_tiles_only_rows_give_one_plane_per_cell(pkg, synthetic, name, want):
    """2 keyframes x 9 points in every 1 m cell of a flat sheet: 18 points (> kMinPoints = 15) that pass the plane test, so exactly one plane
    per cell -- 2047 / 2048 / 2049 planes, the two sides of kBalmCutMaxPlanes and of the residual's switch of form."""
    w, win, clouds = balm_cases.row(name)
    assert [c.shape for c in clouds] == [(want * 9, 3)] * 2 and all(c.dtype == np.float32 for c in clouds)
    clusters, coe = balm_cases.host_planes(name)
    assert len(coe) == want and clusters.shape == (want, 2, 10)
    assert np.array_equal(coe, np.full(want, 18.0)) and np.array_equal(clusters[:, :, 9], np.full((want, 2), 9.0))


@pytest.mark.parametrize("name,lo,hi,W,points", [("w3_over", 2048, 4096, 3, 45000), ("w2_two", 8192, 16384, 2, 151800), ("w8_two", 4096, 8192, 8, 76800),
                                                 ("w7", 50, 2048, 7, 14700), ("w8", 50, 4096, 8, 16800)])
def test_rows_with_the_standard_clouds_lie_on_their_side_of_the_limits(pkg, synthetic, name, lo, hi, W, points):
    """The rows that add synthetic.ba_window_clouds to the sheet: more than 2048 planes (w3_over: the extraction's overflow), more than
    8192 at W = 2 and more than 4096 at W = 8 (set_planes then gives planes_per_chunk = 2 PB: a second pass of the plane-batch loop), and the
    W = 7 | 8 pair below every limit.  The standard clouds bring planes that some keyframe does not see (n_i = 0 slots)."""
    w, win, clouds = balm_cases.row(name)
    assert len(win) == W and sum(len(c) for c in clouds) == points
    clusters, coe = balm_cases.host_planes(name)
    assert lo < len(coe) <= hi, len(coe)
    plane_batch = 8 if W <= 7 else 4   # BalmTerm::set_planes
    per_chunk = plane_batch * max(1, (len(coe) + plane_batch * 1024 - 1) // (plane_batch * 1024))
    assert per_chunk == (2 * plane_batch if name in ("w2_two", "w8_two") else plane_batch)
    if W > 2:
        assert balm_cases.empty_slots(clusters) > 0
    # horizontal planes (sheet, ground: normal along the LiDAR's z) and the two walls (along its y): the smallest eigenvector of the
    # covariance of each plane's best-filled cluster with at least 6 points, in that keyframe's LiDAR frame (the frames differ by 0.03 rad)
    best = clusters[np.arange(len(coe)), clusters[:, :, 9].argmax(1)]
    best = best[best[:, 9] >= 6]
    P, v, n = best[:, :6], best[:, 6:9], best[:, 9]
    idx = [[0, 1, 2], [1, 3, 4], [2, 4, 5]]
    C = P[:, idx] / n[:, None, None] - (v / n[:, None])[:, :, None] * (v / n[:, None])[:, None, :]
    normal = np.linalg.eigh(C)[1][:, :, 0]
    assert (np.abs(normal[:, 2]) > 0.9).sum() > 50 and (np.abs(normal[:, 1]) > 0.9).sum() > 20


def test_one_keyframe_gives_no_plane(pkg, synthetic):
    """W = 1: 300 cells of 20 points each pass the plane test, and none is a plane (VOX_HESS::push_voxel: a plane must be seen from two
    keyframes)."""
    w, win, clouds = balm_cases.row("w1")
    assert len(win) == 1 and clouds[0].shape == (6000, 3)
    clusters, coe = balm_cases.host_planes("w1")
    assert len(coe) == 0 and clusters.shape == (0, 1, 10)


def test_host_extraction_at_2049_planes_matches_the_oracle(pkg, oracle, synthetic):
    """The window finish_cut hands to the host extraction (2049 planes: k_balm_cut_walk sets `over`): the same planes as the oracle's
    cut_voxel / recut / tras_opt with bit-identical cluster sums, compared as test_host_plane_extraction_matches_the_oracle does (the
    reference walks an unordered map: as sets).  The planes' content alone does not order 2049 cells of one sheet uniquely to six digits, so
    the sort key here is the whole row; the comparison itself is array_equal as there."""
    w, win, clouds = balm_cases.row("p2049")
    oc, ocoe = oracle.lidar_planes(w["poses"], win, clouds, synthetic.TCL7)
    pc, pcoe = balm_cases.host_planes("p2049")
    assert len(ocoe) == len(pcoe) == 2049
    o10 = np.concatenate([oc[:, :, [0, 1, 2, 4, 5, 8]], oc[:, :, 9:13]], 2)
    assert np.array_equal(oc[:, :, [1, 2, 5]], oc[:, :, [3, 6, 7]])  # P is symmetric

    def canon(c, q):
        order = np.lexsort(np.concatenate([c.reshape(len(q), -1).T, q[None]], 0))
        return c[order], q[order]
    a, ac = canon(o10, ocoe)
    b, bc = canon(pc, pcoe)
    assert np.array_equal(ac, bc)
    assert np.array_equal(a, b)
