"""The list form of the projection search (k_match_grid -> k_match_candidates -> k_match_resolve) with directed inputs: scan order and
ties, windows larger than a round of lanes, ragged batches, window clamping, the static tests, the feature grid kept per extraction in the
extractor handle, and the retry pass.  Every comparison is array_equal: the matches are integers.

Crafted frames go through tc2li_search_by_projection_keyframe_batch (caller-supplied keys, descriptors and bounds) with the identity pose,
fx = fy = 128, and points at depth 1 whose x and y are multiples of 1 / 128: they project onto whole pixels exactly, so the reference
(reloc_ref.search_by_projection_keyframe over the oracle's grid) sees the same windows bit for bit.  A point's level is chosen through
max_distance_raw = dist * 1.2^(level - 0.5).  The handle path goes through the two tracking entry points against the oracle's
track_motion_model / track_local_map (the helpers of test_tracking_gpu.py)."""
import threading

import numpy as np
import pytest

import reloc_ref as R
import test_tracking_gpu as T
import two_callers

pytestmark = pytest.mark.gpu

FX = np.float32(128.0)
SF = (np.float32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
LOG_SF = float(np.log(np.float32(1.2)))
IDENTITY = np.float32([0, 0, 0, 1, 0, 0, 0])
W, H = 320, 240  # cells of 5 x 5 pixels


def _keys(pkg, xy, octave):
    k = np.zeros(len(xy), pkg.capi.KEYPOINT_DTYPE)
    if len(xy):
        k["x"], k["y"], k["octave"], k["size"] = xy[:, 0], xy[:, 1], octave, 31
    return k


def _points(uv, level, desc, shift=(0, 0)):
    """Points at depth 1 that project onto pixel uv of a camera with principal point `shift`, searched on `level`."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    n = len(uv)
    Xw = np.stack([(uv[:, 0] - np.float32(shift[0])) / FX, (uv[:, 1] - np.float32(shift[1])) / FX, np.ones(n, np.float32)], 1).astype(np.float32)
    dist = np.sqrt((Xw.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    raw = (dist * np.float32(1.2) ** (np.asarray(level, np.float32).reshape(n) - np.float32(0.5))).astype(np.float32)
    return dict(has_point=np.ones(n, np.uint8), found=np.zeros(n, np.uint8), Xw=Xw, point_descriptors=np.asarray(desc, np.uint8).reshape(n, 32),
                min_distance=np.zeros(n, np.float32), max_distance=np.full(n, 1e9, np.float32), max_distance_raw=raw, angle=np.zeros(n, np.float32))


def _item(pkg, xy, octave, desc, held, pts, bounds=(0, W, 0, H)):
    return dict(keys=_keys(pkg, np.asarray(xy, np.float32).reshape(-1, 2), octave), descriptors=np.asarray(desc, np.uint8).reshape(-1, 32),
                held=np.asarray(held, np.uint8), pose7=IDENTITY, bounds=list(bounds), **pts)


def _reference(oracle, item, th, orb_dist=100):
    """reloc_ref.py on the item; a frame whose bounds start at (min_x, min_y) is the frame moved by (-min_x, -min_y) with the principal point
    moved along (whole pixels: every coordinate and every grid position stays exact)."""
    sx, sy = -float(item["bounds"][0]), -float(item["bounds"][2])
    keys = item["keys"].copy()
    keys["x"] += np.float32(sx); keys["y"] += np.float32(sy)
    frame = dict(keys=keys, descriptors=item["descriptors"], held=item["held"], pose7=IDENTITY, cols=int(item["bounds"][1] + sx),
                 rows=int(item["bounds"][3] + sy))
    want, n, _ = R.search_by_projection_keyframe(oracle, frame, item, np.float32([FX, FX, sx, sy]), SF, LOG_SF, th, orb_dist, False)
    return want, n


def _search(pkg, items, th, orb_dist=100):
    return pkg.search_by_projection_keyframe_batch(items, np.float32([FX, FX, 0, 0]), SF, LOG_SF, th, orb_dist, False)


def _same(pkg, oracle, items, th, refs=None):
    match, nm = _search(pkg, items, th)
    for f, it in enumerate(items):
        want, n = refs[f] if refs is not None else _reference(oracle, it, th)
        N = len(want)
        assert np.array_equal(match[f, :N], want), (f, np.flatnonzero(match[f, :N] != want)[:10])
        assert (match[f, N:] == -1).all() and nm[f] == n, (f, nm[f], n)
    return match, nm


# ---- 1. scan order and ties -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_first_of_equal_distances_in_scan_order(pkg, oracle, seed):
    """One query at (160, 120), level 0, th = 5: the window is cells 31..33 x 23..25.  40 keys inside it; six carry the query's exact
    descriptor, two of them in one cell.  The match is the first of them in (ix, iy, key index) order; the seeds permute the keys."""
    rng = np.random.default_rng(seed)
    cells = [(cx, cy) for cx in (31, 32, 33) for cy in (23, 24, 25)]
    grid = [(x, y) for x in range(156, 165) for y in range(116, 125)]
    xy = np.float32([grid[i] for i in rng.permutation(len(grid))[:40]])
    cell_of = [(int(np.rint(x * np.float32(0.2))), int(np.rint(y * np.float32(0.2)))) for x, y in xy]
    assert set(cell_of) <= set(cells) and len(set(cell_of)) >= 6
    qdesc = rng.integers(0, 256, 32, dtype=np.uint8)
    desc = rng.integers(0, 256, (40, 32), dtype=np.uint8)
    by_cell = {}
    for i, c in enumerate(cell_of):
        by_cell.setdefault(c, []).append(i)
    twice = [c for c in by_cell if len(by_cell[c]) >= 2][0]
    equal = list(by_cell[twice][:2]) + [by_cell[c][-1] for c in list(by_cell) if c != twice][:4]
    desc[equal] = qdesc
    first = min(equal, key=lambda i: (cell_of[i][0], cell_of[i][1], i))
    item = _item(pkg, xy, rng.integers(0, 2, 40), desc, np.zeros(40, np.uint8), _points([[160, 120]], [0], qdesc))
    match, nm = _same(pkg, oracle, [item], 5.0)
    assert nm[0] == 1 and match[0, first] == 0
    # the library's one-kernel form on the same query
    q = np.zeros(1, pkg.capi.QUERY_DTYPE)
    q["u"], q["v"], q["radius"], q["u_right"], q["min_level"], q["max_level"], q["valid"], q["has_observations"] = 160, 120, 5, -1, -1, 1, 1, 1
    q["descriptor"][0] = qdesc
    n, of_query, _ = pkg.capi.search_by_projection(item["keys"], desc, np.full(40, -1, np.float32), None, W, H, q, 0)
    assert n == 1 and of_query[0] == first


# ---- 2. a window larger than any round ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def whole_image(pkg, oracle):
    rng = np.random.default_rng(7)
    n = 3072
    xy = np.stack([rng.integers(0, W, n), rng.integers(0, H, n)], 1).astype(np.float32)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    src = rng.integers(0, n, 5)
    pdesc = desc[src].copy()
    pdesc[:, 0] ^= 1
    item = _item(pkg, xy, rng.integers(0, 3, n), desc, rng.random(n) < 0.1, _points(xy[src], np.ones(5), pdesc))
    return item, _reference(oracle, item, 400.0)


@pytest.mark.parametrize("per_query", ["3072", None])
def test_window_over_the_whole_image(pkg, oracle, whole_image, monkeypatch, per_query):
    """3072 keys (kMaxMatchKeys) and five queries whose radius covers the image: about 2700 candidates each.  With 3072 pool entries per
    query the list form holds them all (lists far longer than the LDS stage: the second walk); at the default 32 the pool overflows and
    the one-kernel form answers.  Both equal the reference."""
    if per_query:
        monkeypatch.setenv("TC2LI_MATCH_POOL_PER_QUERY", per_query)
    item, ref = whole_image
    _, nm = _same(pkg, oracle, [item], 400.0, [ref])
    assert nm[0] == 5


# ---- 3. ragged batches ----------------------------------------------------------------------------------------------------------------
def _random_item(pkg, rng, n_keys, n_points, bounds=(0, W, 0, H)):
    x0, y0 = bounds[0], bounds[2]
    xy = np.stack([rng.integers(x0, x0 + W, n_keys), rng.integers(y0, y0 + H, n_keys)], 1).astype(np.float32)
    octave = rng.integers(0, 8, n_keys)
    desc = rng.integers(0, 256, (n_keys, 32), dtype=np.uint8)
    if n_keys and n_points:
        src = rng.integers(0, n_keys, n_points)
        uv = xy[src] + rng.integers(-6, 7, (n_points, 2)).astype(np.float32)
        uv[:, 0] = np.clip(uv[:, 0], x0, x0 + W); uv[:, 1] = np.clip(uv[:, 1], y0, y0 + H)
        level = np.clip(octave[src] + rng.integers(-1, 2, n_points), 0, 7)
        pdesc = desc[src].copy()
        pdesc[np.arange(n_points), rng.integers(0, 32, n_points)] ^= (1 << rng.integers(0, 8, n_points)).astype(np.uint8)
        pdesc[::5] = desc[src[::5]]  # exact copies: equal distances inside a window when a key was drawn twice
    else:
        uv = np.stack([rng.integers(x0, x0 + W, n_points), rng.integers(y0, y0 + H, n_points)], 1).astype(np.float32)
        level, pdesc = rng.integers(0, 8, n_points), rng.integers(0, 256, (n_points, 32), dtype=np.uint8)
    return _item(pkg, xy, octave, desc, rng.random(n_keys) < 0.1, _points(uv, level, pdesc, (0, 0)), bounds)


@pytest.fixture(scope="module")
def ragged(pkg, oracle):
    """17 items: key counts 0, 1, 63, 64, 65, 500 and query counts 1, 33, 257 in turn, item 4 without points; their references once."""
    rng = np.random.default_rng(11)
    n_keys, n_points = [0, 1, 63, 64, 65, 500], [1, 33, 257]
    items = [_random_item(pkg, rng, n_keys[i % 6], 0 if i == 4 else n_points[i % 3]) for i in range(17)]
    return items, [_reference(oracle, it, 10.0) for it in items]


@pytest.mark.parametrize("n_items", [1, 7, 8, 9, 17])
def test_ragged_batches(pkg, oracle, ragged, n_items):
    """1, 7, 8, 9 and 17 items per call: the remainders of the split over the eight XCDs, workgroups that straddle items (257 and 33
    queries beside 1), items without keys and without points."""
    items, refs = ragged
    first = 5 if n_items == 1 else 0  # the single item: 500 keys, 257 queries
    _, nm = _same(pkg, oracle, items[first:first + n_items], 10.0, refs[first:first + n_items])
    assert n_items < 7 or nm.sum() > 100


# ---- 4. window clamping ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bounds", [(0, W, 0, H), (-16, W - 16, -8, H - 8)])
def test_windows_on_the_border(pkg, oracle, bounds):
    """Queries in the four corners and on the four edges of the bounds, also of bounds that start below zero as undistorted ones do, keys
    all around them, and on a coarse level so that the windows reach far past the grid.  A window that lies wholly outside the grid
    needs a projection outside the bounds, which this entry point rejects before the search: the last point is such a one."""
    rng = np.random.default_rng(5)
    x0, x1, y0, y1 = bounds
    where = [(x, y) for x in (x0, (x0 + x1) // 2, x1) for y in (y0, (y0 + y1) // 2, y1) if (x, y) != ((x0 + x1) // 2, (y0 + y1) // 2)]
    xy, octave = [], []
    level = [0, 7, 3, 1, 6, 2, 7, 0, 4]
    for g, (x, y) in enumerate(where):
        # the first key of a group is the one its query has to find: inside the last cell (a key that rounds to column 64 or row 48 is in no cell)
        xy.append((np.clip(x, x0 + 2, x1 - 4), np.clip(y, y0 + 2, y1 - 4)))
        octave.append(level[g])
        for j in range(11):
            xy.append((np.clip(x + rng.integers(-9, 10), x0, x1 - 1), np.clip(y + rng.integers(-9, 10), y0, y1 - 1)))
            octave.append(rng.integers(0, 8))
    xy = np.float32(xy)
    n = len(xy)
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    uv = np.float32(where + [(x1 + 40, y0)])
    item = _item(pkg, xy, octave, desc, np.zeros(n, np.uint8), _points(uv, level, desc[::12][:8].tolist() + [desc[0].tolist()]), bounds)
    match, nm = _same(pkg, oracle, [item], 10.0)
    assert nm[0] == 8 and np.array_equal(match[0, :n:12], np.arange(8))


# ---- 5. the static tests ---------------------------------------------------------------------------------------------------------------
def test_held_keys_and_the_level_window(pkg, oracle):
    """Every query sits on four keys with its exact descriptor: one held, one two levels below, one two levels above, and one on the
    neighbouring level, which is the only one it may take."""
    rng = np.random.default_rng(3)
    xy, octave, desc, held, uv, level, pdesc = [], [], [], [], [], [], []
    for q in range(24):
        x, y, lv = 20 + 12 * q, 30 + 8 * (q % 20), 2 + q % 4
        d = rng.integers(0, 256, 32, dtype=np.uint8)
        for dx, o, h in ((0, lv, 1), (1, lv - 2, 0), (2, lv + 2, 0), (3, lv + (1 if q % 2 else -1), 0)):
            xy.append((x + dx, y)); octave.append(o); desc.append(d); held.append(h)
        uv.append((x, y)); level.append(lv); pdesc.append(d)
    item = _item(pkg, np.float32(xy), octave, desc, held, _points(np.float32(uv), level, pdesc))
    match, nm = _same(pkg, oracle, [item], 10.0)
    assert nm[0] == 24 and np.array_equal(np.flatnonzero(match[0, :96] >= 0), np.arange(24) * 4 + 3)


@pytest.fixture(scope="module")
def small_tracking(pkg, oracle, synthetic):
    return T.local_map_scenario(pkg, oracle, synthetic, [30, 31], nfeatures=1000)


def _moved(sc, z):
    """The predicted camera z further along its axis, the last frames' points with it: they project where they did."""
    preds = sc["preds"].copy()
    preds[:, 6] += np.float32(z)
    lasts = [dict(L, Xw=(L["Xw"] - np.float32([0, 0, z])).astype(np.float32)) for L in sc["lasts"]]
    return dict(sc, preds=preds, lasts=lasts)


@pytest.mark.parametrize("case", ["forward", "backward", "stereo"])
def test_tracking_level_limits_and_stereo_window(pkg, oracle, synthetic, small_tracking, case):
    """TrackWithMotionModel against the oracle with the camera moved by 1.5 baselines forward (levels >= the last octave), backward
    (levels <= it), and with u_right moved by up to +-12 pixels, so that keys fall out of the stereo window on either side of r."""
    sc = small_tracking
    if case == "stereo":
        rng = np.random.default_rng(9)
        ur = sc["u_right"].copy()
        ur[ur > 0] += rng.uniform(-12, 12, int((ur > 0).sum())).astype(np.float32)
        plain = pkg.capi.track_motion_model_batch(sc["ext"], 2, sc["kps"], sc["u_right"], pkg.capi.pack_last_frames(sc["lasts"]), sc["preds"],
                                                  np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY, sc["bf"]]).astype(np.float64), sc["b"])
        sc = dict(sc, u_right=ur)
        res = T.check(pkg, oracle, synthetic, sc)
        assert all(nm < p for (nm, _), p in zip(res, plain[2]))  # the stereo test rejected candidates
    else:
        res = T.check(pkg, oracle, synthetic, _moved(sc, (-1.5 if case == "forward" else 1.5) * sc["b"]))
    assert all(nm >= 20 for nm, _ in res)


# ---- 6. the grid of an extraction ------------------------------------------------------------------------------------------------------
def _both_searches(pkg, synthetic, ext, sc, streams=(0, 0), threads=False):
    cam5 = np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY, sc["bf"]]).astype(np.float64)
    out = [None, None]

    def motion():
        out[0] = pkg.capi.track_motion_model_batch(ext, 2, sc["kps"], sc["u_right"], pkg.capi.pack_last_frames(sc["lasts"]), sc["preds"], cam5, sc["b"],
                                                   stream=streams[0])

    def local():
        out[1] = pkg.capi.track_local_map_batch(ext, 2, sc["kps"], sc["u_right"], sc["poses"], sc["held"], sc["held_Xw"], sc["local"], sc["local_off"],
                                                cam5, stream=streams[1])
    for fn in (motion, local):
        if threads:
            t = threading.Thread(target=fn)
            t.start(); t.join()
        else:
            fn()
    return list(out[0]) + list(out[1])


def _equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def test_grid_is_built_once_per_extraction(pkg, oracle, synthetic, small_tracking, monkeypatch):
    import torch
    sc = small_tracking
    w, h = sc["w"], sc["h"]
    ext = pkg.OrbExtractor(nfeatures=1000, max_width=w, max_height=h, max_images=4)
    kps, _, counts, _ = ext.extract_batch_dev(sc["dev"].data_ptr(), 4, w, h, w, w * h)
    assert np.array_equal(counts, sc["counts"]) and np.array_equal(kps, sc["kps"]) and ext.match_grid_builds() == 0
    got = _both_searches(pkg, synthetic, ext, sc)
    assert ext.match_grid_builds() == 1  # motion model, perhaps its retry pass, local map: one build
    monkeypatch.setenv("TC2LI_MATCH_GRID_CACHE", "0")
    assert _equal(_both_searches(pkg, synthetic, ext, sc), got) and ext.match_grid_builds() == 1
    monkeypatch.delenv("TC2LI_MATCH_GRID_CACHE")
    assert (got[2] > 20).all() and (got[7] > 20).all()
    # other images on the same handle: the results follow the new keypoints
    sc2 = T.local_map_scenario(pkg, oracle, synthetic, [32, 33], nfeatures=1000)
    kps2, _, counts2, _ = ext.extract_batch_dev(sc2["dev"].data_ptr(), 4, w, h, w, w * h)
    assert np.array_equal(kps2, sc2["kps"]) and not np.array_equal(counts2, counts)
    got2 = _both_searches(pkg, synthetic, ext, sc2)
    assert ext.match_grid_builds() == 2
    assert _equal(got2, _both_searches(pkg, synthetic, sc2["ext"], sc2)) and not _equal(got2[1:3], got[1:3])
    T.check(pkg, oracle, synthetic, dict(sc2, ext=ext))
    assert ext.match_grid_builds() == 2
    # the two searches on two streams from two host threads, one after the other
    ext.extract_batch_dev(sc["dev"].data_ptr(), 4, w, h, w, w * h)
    s0, s1 = torch.cuda.Stream(), torch.cuda.Stream()
    assert _equal(_both_searches(pkg, synthetic, ext, sc, (s0.cuda_stream, s1.cuda_stream), threads=True), got)
    assert ext.match_grid_builds() == 3


# ---- 7. the retry pass -------------------------------------------------------------------------------------------------------------------
def test_retry_pass_reads_its_frames_grid_rows(pkg, oracle, synthetic):
    """Three frames; the middle one's last frame has 12 points, so only it goes through the retry pass, as frame 0 of that pass reading grid
    row 1.  Every frame's result equals the oracle's and that frame searched alone on a handle of its own."""
    sc = T.scenario(pkg, synthetic, [34, 35, 36], w=640, h=240, variants={1: "few"}, nfeatures=1000)
    cam5 = np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY, sc["bf"]]).astype(np.float64)
    T.check(pkg, oracle, synthetic, sc)
    assert sc["ext"].match_grid_builds() == 1
    poses, mp, nm, inl = pkg.capi.track_motion_model_batch(sc["ext"], 3, sc["kps"], sc["u_right"], pkg.capi.pack_last_frames(sc["lasts"]), sc["preds"],
                                                           cam5, sc["b"])
    assert nm[1] < 20 and nm[0] >= 20 and nm[2] >= 20
    for f in range(3):
        ext = pkg.OrbExtractor(nfeatures=1000, max_width=640, max_height=240, max_images=2)
        kps, _, counts, _ = ext.extract_batch_dev(sc["dev"][2 * f:2 * f + 2].data_ptr(), 2, 640, 240, 640, 640 * 240)
        assert np.array_equal(kps, sc["kps"][2 * f:2 * f + 2])
        alone = pkg.capi.track_motion_model_batch(ext, 1, kps, sc["u_right"][f:f + 1], pkg.capi.pack_last_frames(sc["lasts"][f:f + 1]),
                                                  sc["preds"][f:f + 1], cam5, sc["b"])
        assert np.array_equal(alone[1][0], mp[f]) and alone[2][0] == nm[f] and alone[3][0] == inl[f] and np.array_equal(alone[0][0], poses[f])


# ---- 8. the tables of a call: every one has its place in the call's block, whatever the call before left there -------------------------
def test_keyframe_overload_grows_shrinks_and_reuses_its_buffers(pkg, oracle, ragged):
    """On one thread, through the same per-thread buffers: the 17 items, an item of 1 key and 1 query alone, the 17 again."""
    items, refs = ragged
    one = _random_item(pkg, np.random.default_rng(12), 1, 1)
    first, _ = _same(pkg, oracle, items, 10.0, refs)
    _same(pkg, oracle, [one], 10.0)
    again, _ = _same(pkg, oracle, items, 10.0, refs)
    assert np.array_equal(first, again)


def test_keyframe_overload_with_empty_and_with_full_tables(pkg, oracle):
    """A call whose items all have no keys and no points: every table of the block has no row.  And one whose tables are all full and none
    a multiple of 256 bytes long: 65 keys (capacity 65), 33 points."""
    rng = np.random.default_rng(13)
    match, nm = _search(pkg, [_random_item(pkg, rng, 0, 0) for _ in range(3)], 10.0)
    assert (match == -1).all() and (nm == 0).all()
    items = [_random_item(pkg, rng, 65, 33) for _ in range(2)]
    for width in (12, 32, 4, 1):   # MatchKey, descriptor, float / int32, flag: bytes per key and per point
        assert (65 * width) % 256 and (33 * width) % 256 and (2 * 65 * width) % 256 and (2 * 33 * width) % 256
    match, _ = _same(pkg, oracle, items, 10.0)
    assert match.shape == (2, 65)
    for f, it in enumerate(items):   # the items alone: what a neighbour's table could have overwritten
        alone, _ = _search(pkg, [it], 10.0)
        assert np.array_equal(alone[0], match[f])


@pytest.fixture(scope="module")
def one_frame_tracking(pkg, oracle, synthetic):
    return T.local_map_scenario(pkg, oracle, synthetic, [37], nfeatures=1000, w=640, h=240)


def _track_both(pkg, synthetic, sc, streams=(0, 0)):
    return list(T.run_motion_model(pkg, synthetic, sc, stream=streams[0])) + list(T.run_local_map(pkg, synthetic, sc, 1.0, False, stream=streams[1]))


def test_tracking_grows_shrinks_and_reuses_its_buffers(pkg, oracle, synthetic, small_tracking, one_frame_tracking):
    """Two frames of 1242 x 375, one frame of 640 x 240 on a handle of its own, the two frames again: on one thread, through both entries
    and the same per-thread buffers.  The first two runs equal the oracle, the third the first."""
    runs = [_track_both(pkg, synthetic, sc) for sc in (small_tracking, one_frame_tracking, small_tracking)]
    for sc, got in ((small_tracking, runs[0]), (one_frame_tracking, runs[1])):
        T.check(pkg, oracle, synthetic, sc, got=got[:4])
        T.check_local_map(pkg, oracle, synthetic, sc, 1.0, False, got=got[4:], at_least=(20, 20))
    assert _equal(runs[2], runs[0])


def test_two_threads_in_track_local_map(pkg, synthetic, small_tracking, one_frame_tracking):
    """Two host threads in tc2li_track_local_map_batch at once, each with its own extractor and stream, three calls each: the work spaces
    are per thread, so each thread's results are the single-threaded ones."""
    import torch
    scs = (small_tracking, one_frame_tracking)
    alone = [T.run_local_map(pkg, synthetic, sc, 1.0, False) for sc in scs]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    call = lambda k: T.run_local_map(pkg, synthetic, scs[k], 1.0, False, stream=streams[k].cuda_stream)
    a, b = two_callers.run(call, [0] * 3, [1] * 3)
    assert all(_equal(got, alone[0]) for got in a) and all(_equal(got, alone[1]) for got in b)
