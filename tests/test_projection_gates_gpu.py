"""The projection matcher on the device against the plain references, on the directed cases of projection_cases.py and
projection_local_cases.py: the claim rounds (k_match_by_projection, k_match_resolve) on chains as long as the query count, the ratio test
and the thresholds at equality, the static gates at equality, the rotation filter on the host (tc2li_search_by_projection) and on the
device (k_track_count), PredictScale on the boundaries between levels (the amb_* list, resolve_ambiguous_levels and both patch kernels),
the candidate stages of k_match_candidates at every lane width the library ships, and the frustum gates of SearchLocalPoints.
Every comparison is array_equal on integers plus the match counts: there are no tolerances."""
import numpy as np
import pytest

import projection_cases as PC
import projection_local_cases as LC
import projection_ref as P
import reloc_ref as R

pytestmark = pytest.mark.gpu

RAW = PC.raw_cases()
LANES = ("2", "4", "8", "16", "32")


# ---- raw queries: tc2li_search_by_projection (the one-kernel form, the host's rotation filter) -------------------------------------------
@pytest.mark.parametrize("case", RAW, ids=lambda c: c["name"])
def test_raw_queries(pkg, oracle, case):
    """Both modes, with and without orientation: match_of_query, nmatches and query_of_keypoint (the reference's mvpMapPoints)."""
    for mode in (0, 1):
        both = P.search_queries_both(oracle, case["keys"], case["desc"], case["u_right"], case["occupied"], PC.W, PC.H, case["queries"], mode, PC.NN_RATIO)
        for orientation in (False, True):
            wn, wmatch, wpoint = both[orientation]
            if mode in case["modes"]:      # the case's own statement, where it makes one for this mode
                want = case["want"].get((mode, orientation), case["want"][(mode, False)])
                assert wn == want[0] and np.array_equal(wmatch, want[1]) and np.array_equal(wpoint, want[2])
            n, match, of_key = pkg.search_by_projection(case["keys"], case["desc"], case["u_right"], case["occupied"], PC.W, PC.H, case["queries"], mode,
                                                        PC.NN_RATIO, orientation)
            assert np.array_equal(match, wmatch), (mode, orientation, np.flatnonzero(match != wmatch)[:10])
            assert n == wn and np.array_equal(of_key, wpoint), (mode, orientation, n, wn)


# ---- the keyframe overload: the list form ------------------------------------------------------------------------------------------------
def kf_reference(oracle, item, cam4, th, orb_dist, check_orientation):
    frame = dict(keys=item["keys"], descriptors=item["descriptors"], held=item["held"], pose7=item["pose7"], cols=PC.W, rows=PC.H)
    want, n, _ = R.search_by_projection_keyframe(oracle, frame, item, cam4, PC.SF, PC.LOG_SF, th, orb_dist, check_orientation)
    return want, n


def kf_check(pkg, items, refs, cam4, th, orb_dist, check_orientation, alone=True):
    """All items in one call, then (alone) one item at a time: both equal the references."""
    match, nm = pkg.search_by_projection_keyframe_batch(items, cam4, PC.SF, PC.LOG_SF, th, orb_dist, check_orientation)
    for f, (want, n) in enumerate(refs):
        N = len(want)
        assert np.array_equal(match[f, :N], want), (f, np.flatnonzero(match[f, :N] != want)[:10])
        assert (match[f, N:] == -1).all() and nm[f] == n, (f, nm[f], n)
    if alone:
        for f, it in enumerate(items):
            m1, n1 = pkg.search_by_projection_keyframe_batch([it], cam4, PC.SF, PC.LOG_SF, th, orb_dist, check_orientation)
            N = len(it["keys"])
            assert np.array_equal(m1[0, :N], match[f, :N]) and n1[0] == nm[f], f


@pytest.fixture(scope="module")
def level_group(oracle):
    items, ratios, octaves, cam4, th = PC.level_items()
    return items, [kf_reference(oracle, it, cam4, th, 100, False) for it in items], cam4, th


@pytest.mark.parametrize("lanes", LANES)
def test_level_on_a_boundary(pkg, level_group, monkeypatch, lanes):
    """max_distance_raw / dist = 1.2^k and its neighbours up to 8 floats away, k = 0 .. 7, and the clamps at both ends: the level is
    MapPoint::PredictScale's with the C library's logf, whichever side of the integer the device's double quotient falls on."""
    monkeypatch.setenv("TC2LI_MATCH_LANES", lanes)
    items, refs, cam4, th = level_group
    assert 0 < sum(n for _, n in refs[:17 * 7]) < 17 * 7
    kf_check(pkg, items, refs, cam4, th, 100, False)


@pytest.fixture(scope="module")
def chain_group(oracle):
    out = {}
    for L in (30, 600):
        item, assigned = PC.kf_chain_item(L)
        want, n = kf_reference(oracle, item, PC.CAM_CORNER, 40.0, 100, False)
        assert n == L and np.array_equal(want, assigned)
        out[L] = (item, (want, n))
    return out


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("L,pool", [(30, None), (600, "3072"), (600, None)])
def test_chain_on_the_list_form(pkg, chain_group, monkeypatch, lanes, L, pool):
    """L points on one pixel with one descriptor, L keys in their window: point k ends on the k-th key of the scan, and k_match_resolve
    needs L rounds, its query count.  30 fit the default pool (32 per query); 600 need 3072 per query, and at the default the pool
    overflows and the one-kernel form answers: the same result."""
    monkeypatch.setenv("TC2LI_MATCH_LANES", lanes)
    if pool:
        monkeypatch.setenv("TC2LI_MATCH_POOL_PER_QUERY", pool)
    item, ref = chain_group[L]
    kf_check(pkg, [item], [ref], PC.CAM_CORNER, 40.0, 100, False, alone=False)


@pytest.mark.parametrize("lanes", LANES)
@pytest.mark.parametrize("orb_dist", [64, 100])
def test_orb_dist_at_equality(pkg, oracle, monkeypatch, lanes, orb_dist):
    monkeypatch.setenv("TC2LI_MATCH_LANES", lanes)
    items = PC.orb_dist_items(orb_dist)
    refs = [kf_reference(oracle, it, PC.CAM_CORNER, 10.0, orb_dist, False) for it in items]
    assert [n for _, n in refs] == [1, 0]
    kf_check(pkg, items, refs, PC.CAM_CORNER, 10.0, orb_dist, False)


@pytest.fixture(scope="module")
def stage_group(oracle):
    items = [PC.stage_item(n)[0] for n in PC.STAGE_COUNTS]
    return items, [kf_reference(oracle, it, PC.CAM_CORNER, 10.0, 100, False) for it in items]


@pytest.mark.parametrize("lanes", LANES)
def test_candidate_counts_around_the_stage(pkg, stage_group, monkeypatch, lanes):
    """15, 16, 17, 31, 32 and 33 candidates in one window: the sizes around the 16 (2 and 4 lanes) and 32 (8 lanes and more) entries a
    sub-group stages in LDS.  The wanted key is the last candidate, and the next query's single candidate sits in the neighbouring stage."""
    monkeypatch.setenv("TC2LI_MATCH_LANES", lanes)
    items, refs = stage_group
    assert all(n == 2 for _, n in refs)
    kf_check(pkg, items, refs, PC.CAM_CORNER, 10.0, 100, False)


@pytest.fixture(scope="module")
def rotation_group(oracle):
    items = PC.rotation_items()
    return items, [kf_reference(oracle, it, PC.CAM_CORNER, 3.0, 100, True) for it in items], [kf_reference(oracle, it, PC.CAM_CORNER, 3.0, 100, False) for it in items]


@pytest.mark.parametrize("lanes", LANES)
def test_rotation_filter_on_the_device(pkg, rotation_group, monkeypatch, lanes):
    """The rotation cases through k_track_count: a second and third maximum of exactly a tenth of the first, tied bins, one bin, no match,
    the wrap of a negative difference; among them an item with keys and no points and one with points and no keys."""
    monkeypatch.setenv("TC2LI_MATCH_LANES", lanes)
    items, turned, plain = rotation_group
    assert sum(n for _, n in plain) - sum(n for _, n in turned) == 25
    kf_check(pkg, items, turned, PC.CAM_CORNER, 3.0, 100, True, alone=lanes == "2")
    kf_check(pkg, items, plain, PC.CAM_CORNER, 3.0, 100, False, alone=False)


# ---- SearchLocalPoints on extracted features -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def local_group(pkg, oracle, synthetic):
    """One 640 x 240 stereo pair twice in a batch of two frames, 1000 features; the directed points built on the downloaded features, the
    same list for both frames, and the reference's answer for every run."""
    import torch
    w, h = 640, 240
    pair = np.stack(synthetic.stereo_pair(40, w, h))
    dev = torch.from_numpy(np.concatenate([pair, pair])).cuda()
    ext = pkg.OrbExtractor(nfeatures=1000, max_width=w, max_height=h, max_images=4)
    kps, desc, counts, _ = ext.extract_batch_dev(dev.data_ptr(), 4, w, h, w, w * h)
    bf = np.float32(synthetic.BF)
    u_right, _, _ = pkg.stereo_match_batch(ext, 2, float(bf), float(bf / np.float32(synthetic.FX)))
    n = int(counts[0])
    assert counts[2] == n and np.array_equal(kps[0], kps[2]) and np.array_equal(u_right[0], u_right[1])
    cam = np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY, bf])
    scales = ext.GetScaleFactors()
    log_scale = PC.LOG_SF
    frame = dict(keys=kps[0, :n], descriptors=desc[0, :n], u_right=u_right[0, :n], held=np.zeros(n, np.uint8), cols=w, rows=h)
    case = LC.build(frame, cam, scales)
    refs = [P.search_local_points(oracle, frame, case["points"], PC.IDENTITY, cam, scales, log_scale, th, far, th_far) for th, far, th_far in LC.runs(case)]
    return dict(ext=ext, dev=dev, kps=kps, u_right=u_right, n=n, cam5=cam.astype(np.float64), case=case, refs=refs)


@pytest.mark.parametrize("lanes", ["2", "32"])
@pytest.mark.parametrize("run", [0, 1, 2, 3])
def test_local_points(pkg, local_group, monkeypatch, lanes, run):
    """isInFrustum's gates at equality, the level on both sides of every 1.2^k, the window factor on both sides of 0.998, th == 1 and 3,
    the far-points threshold on a point's depth, and the ratio pairs, through tc2li_search_local_points_batch and
    tc2li_track_local_map_batch: local_of_keypoint and n_matches of projection_ref.search_local_points, for both frames of the batch."""
    monkeypatch.setenv("TC2LI_MATCH_LANES", lanes)
    g = local_group
    th, far, th_far = LC.runs(g["case"])[run]
    want, wn = g["refs"][run]
    n, cap = g["n"], g["kps"].shape[1]
    pts = np.concatenate([g["case"]["points"]] * 2)
    off = np.int32([0, len(pts) // 2, len(pts)])
    poses = np.stack([PC.IDENTITY] * 2)
    held, held_Xw = np.zeros((2, cap), np.uint8), np.zeros((2, cap, 3), np.float32)
    assert wn >= 10      # enough edges for the pose optimisation behind tc2li_track_local_map_batch
    lk, nm = pkg.capi.search_local_points_batch(g["ext"], 2, g["kps"], g["u_right"], poses, held, held_Xw, pts, off, g["cam5"], th=th, far_points=far, th_far=th_far)
    got = pkg.capi.track_local_map_batch(g["ext"], 2, g["kps"], g["u_right"], poses, held, held_Xw, pts, off, g["cam5"], th=th, far_points=far, th_far=th_far)
    for f in range(2):
        for k, m in ((lk, nm), (got[1], got[3])):
            assert np.array_equal(k[f, :n], want), (f, np.flatnonzero(k[f, :n] != want)[:10])
            assert (k[f, n:] == -1).all() and m[f] == wn, (f, m[f], wn)
