"""Directed inputs for the projection matcher: the parts of it that are algorithms of their own (the claim rounds that replace the
reference's sequential loop, the ratio test, the level on a boundary of PredictScale, the rotation filter, the candidate stages of the
list form).  Every case is a function that returns its inputs together with the property it exists for, stated from the reference source
(SF/src/ORBmatcher.cc:52-222, 1685-1896) by hand, not from any implementation; tests/test_projection_cases.py checks that property with
projection_ref alone, tests/test_projection_gates_gpu.py runs the cases on the device.

Frames are 320 x 240 with 64 x 48 grid cells of 5 x 5 pixels, as in test_projection_lists_gpu.py.  A raw case is a dict: keys, desc,
u_right, occupied, queries (tc2li_proj_query records), modes (the matcher modes it is meant for), and per mode the expectation
want[(mode, check_orientation)] = (nmatches, match_of_query, point_of_keypoint); a missing entry with orientation means "as without"."""
import numpy as np

import reloc_ref

KEYPOINT_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])   # tc2li_keypoint
QUERY_DTYPE = np.dtype([("u", "<f4"), ("v", "<f4"), ("radius", "<f4"), ("u_right", "<f4"), ("min_level", "<i4"), ("max_level", "<i4"),
                        ("angle", "<f4"), ("valid", "<i2"), ("has_observations", "<i2"), ("descriptor", "u1", (32,))])          # tc2li_proj_query
W, H = 320, 240
F32 = np.float32
NN_RATIO = 0.8


def make_keys(xy, octave=0, angle=0.0):
    xy = np.asarray(xy, np.float32).reshape(-1, 2)
    k = np.zeros(len(xy), KEYPOINT_DTYPE)
    if len(xy):
        k["x"], k["y"], k["octave"], k["angle"], k["size"] = xy[:, 0], xy[:, 1], octave, angle, 31
    return k


def make_queries(uv, radius, desc, min_level=-1, max_level=-1, u_right=-1.0, angle=0.0, has_observations=1):
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    q = np.zeros(len(uv), QUERY_DTYPE)
    q["u"], q["v"], q["radius"], q["u_right"], q["min_level"], q["max_level"] = uv[:, 0], uv[:, 1], radius, u_right, min_level, max_level
    q["angle"], q["valid"], q["has_observations"] = angle, 1, has_observations
    q["descriptor"] = np.asarray(desc, np.uint8).reshape(-1, 32)
    return q


def flip(desc, first, count):
    """desc with bits first .. first + count - 1 inverted: Hamming distance `count` from desc."""
    out = np.array(desc, np.uint8).copy()
    for b in range(first, first + count):
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def scan_order(keys):
    """Key indices in the order GetFeaturesInArea returns them for a window that holds them all: grid column, grid row, key index."""
    cx = np.rint(keys["x"] * F32(64.0 / W)).astype(int)
    cy = np.rint(keys["y"] * F32(48.0 / H)).astype(int)
    return sorted(range(len(keys)), key=lambda i: (cx[i], cy[i], i))


def raw_case(name, keys, desc, queries, want, u_right=None, occupied=None, modes=(0, 1), why=""):
    n = len(keys)
    return dict(name=name, keys=keys, desc=np.asarray(desc, np.uint8).reshape(n, 32), queries=queries, modes=tuple(modes), want=want, why=why,
                u_right=np.full(n, -1, np.float32) if u_right is None else np.asarray(u_right, np.float32),
                occupied=None if occupied is None else np.asarray(occupied, np.uint8))


def expectation(n_keys, match, cleared=()):
    """(nmatches, match_of_query, point_of_keypoint) of a search whose query q wrote keypoint match[q] (in query order, a later write
    replaces an earlier one) and whose rotation filter then removed the histogram entries `cleared` (keypoints, one per rejected entry)."""
    match = np.asarray(match, np.int32).copy()
    point = np.full(n_keys, -1, np.int32)
    for q, k in enumerate(match):
        if k >= 0:
            point[k] = q
    n = int((match >= 0).sum()) - len(cleared)
    for k in cleared:
        point[k] = -1
    match[np.isin(match, list(cleared))] = -1
    return n, match, point


# ---- chains ---------------------------------------------------------------------------------------------------------------------------
# 513 is the smallest chain that crosses the 512-thread stride of the rounds kernels; each round of the one-kernel form walks the whole
# window again, so a longer raw chain (600) only costs time: the list form runs its 600 in kf_chain_item
CHAIN_LENGTHS = (1, 2, 63, 64, 65, 513)
CHAIN_VARIANTS = ("plain", "reverse", "no_observations_first", "no_observations_middle", "no_observations_last", "occupied_middle", "u_right_gate",
                  "two_chains")


def _lattice(n, x0, y0, per_row=25):
    """n whole-pixel positions from (x0, y0) on, per_row to a row."""
    return np.float32([(x0 + i % per_row, y0 + i // per_row) for i in range(n)]).reshape(-1, 2)


def chain(L, variant, octaves="one", flipped=0):
    """L queries and L keys in one window (centre (160, 120), radius 40), all with one descriptor, so the scan order alone decides: with
    every query holding observations, query k ends on the k-th free key of the scan.  M = L: in the rounds form query k is final after
    round k + 1, so the last change happens in round L and round L + 1, the cap, confirms it.
    octaves = "alternate": the keys lie on octaves 0, 1, 0, ... in scan order and differ from the queries by `flipped` bits: in mode 1
    best and second best are equal and on different levels."""
    rng = np.random.default_rng(1000 + L)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    if variant == "two_chains":
        la = L - L // 2
        xy = np.concatenate([_lattice(la, 40, 60), _lattice(L // 2, 230, 150)])
    else:
        xy = _lattice(L, 148, 108)
    keys = make_keys(xy)
    if variant == "reverse":
        keys = keys[::-1].copy()
    order = scan_order(keys)
    if octaves == "alternate":
        keys["octave"][order] = np.arange(L) % 2
    desc = np.tile(flip(d, 0, flipped), (L, 1))
    q = make_queries(np.tile(np.float32([160, 120]), (L, 1)), 40.0, np.tile(d, (L, 1)))
    u_right, occupied = np.full(L, -1, np.float32), np.zeros(L, np.uint8)
    match = np.full(L, -1, np.int32)
    if variant in ("plain", "reverse"):
        match[:] = order
    elif variant.startswith("no_observations"):
        p = dict(first=0, middle=L // 2, last=L - 1)[variant.split("_")[-1]]
        q["has_observations"][p] = 0
        # query p's key stays free: query p + 1 takes it too, and every later query is one key behind
        match[:] = [order[k] if k <= p else order[k - 1] for k in range(L)]
    elif variant == "occupied_middle":
        occupied[order[L // 2]] = 1
        free = [k for k in order if not occupied[k]]
        match[:len(free)] = free
    elif variant == "u_right_gate":
        # the key in the middle of the scan has a right coordinate that only even queries accept (|100 - 100| <= 40 < |200 - 100|)
        m = L // 2
        u_right[order[m]] = 100.0
        q["u_right"] = np.where(np.arange(L) % 2 == 0, 100.0, 200.0)
        free = list(order)
        for k in range(L):
            take = next((j for j in free if not (j == order[m] and k % 2 == 1)), -1)
            match[k] = take
            if take >= 0:
                free.remove(take)
    elif variant == "two_chains":
        la = L - L // 2
        side = np.arange(L) % 2                     # even queries walk the first chain, odd ones the second
        q["u"], q["v"] = np.where(side == 0, 52.0, 242.0), np.where(side == 0, 72.0, 162.0)
        oa, ob = [k for k in order if k < la], [k for k in order if k >= la]
        match[:] = [oa[k // 2] if k % 2 == 0 else ob[k // 2] for k in range(L)]
    want = expectation(L, match)
    modes = (1,) if octaves == "alternate" else (0, 1)
    return raw_case("chain-%d-%s%s" % (L, variant, "-alternate" if octaves == "alternate" else ""), keys, desc, q, {(m, False): want for m in modes},
                    u_right=u_right, occupied=occupied, modes=modes, why="query k ends on the k-th free key of the scan")


def chain_cases():
    out = [chain(L, v) for L in CHAIN_LENGTHS for v in CHAIN_VARIANTS]
    out += [chain(L, "plain", "alternate", 10) for L in CHAIN_LENGTHS]
    return out


# ---- ratio test and thresholds ----------------------------------------------------------------------------------------------------------
def _pair(name, best, second, octaves=(0, 0), accept=True, modes=(1,)):
    """One query at (100, 100), radius 5; key 0 at distance `best` from it, key 1 (when second is not None) at distance `second`."""
    rng = np.random.default_rng(7)
    d = rng.integers(0, 256, 32, dtype=np.uint8)
    xy, desc = [(100, 100)], [flip(d, 0, best)]
    if second is not None:
        xy.append((102, 101)); desc.append(flip(d, 128, second))
    keys = make_keys(xy, list(octaves[:len(xy)]))
    want = expectation(len(xy), [0 if accept else -1])
    if isinstance(accept, dict):
        wants = {(m, False): expectation(len(xy), [0 if accept[m] else -1]) for m in modes}
    else:
        wants = {(m, False): want for m in modes}
    return raw_case(name, keys, desc, make_queries([(100, 100)], 5.0, [d]), wants, modes=modes)


def ratio_cases():
    """float32(0.8) * 50 rounds to 40.0 and float32(0.8) * 45 to 36.0: `bestDist > mfNNratio * bestDist2` is false at equality."""
    out = [_pair("ratio-40-50", 40, 50, accept=True), _pair("ratio-41-50", 41, 50, accept=False), _pair("ratio-36-45", 36, 45, accept=True),
           _pair("ratio-0-0", 0, 0, accept=True), _pair("ratio-10-10-one-level", 10, 10, accept=False),
           _pair("ratio-10-10-two-levels", 10, 10, octaves=(0, 1), accept=True), _pair("ratio-second-absent", 30, None, accept=True),
           # TH_HIGH = 100 in both modes; beside a key at 101 mode 0 takes the one at 100, mode 1 rejects it (100 > 0.8 * 101 on one level)
           _pair("th-high-100", 100, None, accept=True, modes=(0, 1)), _pair("th-high-101", 101, None, accept=False, modes=(0, 1)),
           _pair("th-high-100-beside-101", 100, 101, accept={0: True, 1: False}, modes=(0, 1))]
    # the second best held by an earlier query: key A = 41 from query 1, key B = 50 from it; query 0 carries B's descriptor
    rng = np.random.default_rng(8)
    d1 = rng.integers(0, 256, 32, dtype=np.uint8)
    A, B = flip(d1, 0, 41), flip(d1, 100, 50)
    keys = make_keys([(100, 100), (102, 101)])
    for obs, name in ((1, "ratio-second-claimed"), (0, "ratio-second-claimed-without-observations")):
        q = make_queries([(100, 100)] * 2, 5.0, [B, d1], has_observations=[obs, 1])
        # with observations B is gone when query 1 looks: A alone, accepted; without, 41 > 0.8 * 50 on one level: rejected
        out.append(raw_case(name, keys, [A, B], q, {(1, False): expectation(2, [1, 0] if obs else [1, -1])}, modes=(1,)))
    # three queries: 0 takes B; so 1, which had A (41) against B (50), takes A; so 2, which had A (41) against C (50), takes C
    a = rng.integers(0, 256, 32, dtype=np.uint8)
    d1, d2 = flip(a, 0, 41), flip(a, 50, 41)
    B, C = flip(d1, 100, 50), flip(d2, 150, 50)
    keys = make_keys([(100, 100), (102, 101), (98, 99)])
    q = make_queries([(100, 100)] * 3, 5.0, [B, d1, d2])
    out.append(raw_case("ratio-verdicts-flip-in-turn", keys, [a, B, C], q, {(1, False): expectation(3, [1, 0, 2])}, modes=(1,),
                        why="rounds: 0 -> B; then 1 -> A; then 2 -> C"))
    return out


# ---- static gates at equality -----------------------------------------------------------------------------------------------------------
def _gate(name, key_xy, found, q_uv=(160, 120), radius=5.0, octave=0, levels=(-1, -1), key_ur=-1.0, q_ur=-1.0):
    d = np.random.default_rng(9).integers(0, 256, 32, dtype=np.uint8)
    keys = make_keys([key_xy], octave)
    q = make_queries([q_uv], radius, [d], min_level=levels[0], max_level=levels[1], u_right=q_ur)
    want = expectation(1, [0 if found else -1])
    return raw_case(name, keys, [d], q, {(0, False): want, (1, False): want}, u_right=[key_ur])


def gate_cases():
    out = [_gate("gate-dx-equals-r", (165, 120), False), _gate("gate-dx-inside", (164.5, 120), True), _gate("gate-dy-equals-r", (160, 115), False),
           _gate("gate-dy-inside", (160, 115.5), True),
           _gate("gate-u-right-equals-r", (160, 120), True, key_ur=100.0, q_ur=105.0), _gate("gate-u-right-beyond-r", (160, 120), False, key_ur=100.0, q_ur=105.5),
           _gate("gate-u-right-zero-skips", (160, 120), True, key_ur=0.0, q_ur=1000.0), _gate("gate-u-right-negative-skips", (160, 120), True, key_ur=-1.0, q_ur=1000.0),
           _gate("gate-levels-none", (160, 120), True, octave=5, levels=(-1, -1)), _gate("gate-levels-forward-on-octave-0", (160, 120), True, octave=5, levels=(0, -1)),
           _gate("gate-levels-0-to-o-at-o", (160, 120), True, octave=3, levels=(0, 3)), _gate("gate-levels-0-to-o-above", (160, 120), False, octave=4, levels=(0, 3)),
           _gate("gate-levels-from-o-at-o", (160, 120), True, octave=3, levels=(3, -1)), _gate("gate-levels-from-o-below", (160, 120), False, octave=2, levels=(3, -1)),
           # round(318 * 0.2) = 64 and round(238 * 0.2) = 48: in no cell, so never found; one pixel less and the key is in the last cell
           _gate("gate-cell-past-last-column", (318, 120), False, q_uv=(318, 120)), _gate("gate-cell-last-column", (317, 120), True, q_uv=(318, 120)),
           _gate("gate-cell-past-last-row", (160, 238), False, q_uv=(160, 238)), _gate("gate-cell-last-row", (160, 237), True, q_uv=(160, 238))]
    return out


# ---- rotation ---------------------------------------------------------------------------------------------------------------------------
def planted(bins_counts, extra=()):
    """One key per match on a 16-pixel lattice, one query on top of it with the key's own descriptor and radius 3; the matches of
    bins_counts = [(bin, count), ...] get the angle difference 30 * bin degrees (the histogram's bin is round(rot / 30)).  extra: further
    (query angle, key angle) pairs.  -> (keys, desc, queries, bin of every match)."""
    pairs = [(F32(30.0 * b), F32(0.0)) for b, c in bins_counts for _ in range(c)] + [(F32(a), F32(k)) for a, k in extra]
    n = len(pairs)
    rng = np.random.default_rng(20 + n)
    xy = np.float32([(8 + 16 * (i % 20), 8 + 16 * (i // 20)) for i in range(n)])
    assert n <= 20 * 15
    desc = rng.integers(0, 256, (n, 32), dtype=np.uint8)
    keys = make_keys(xy, 0, [k for _, k in pairs] if n else 0.0)
    q = make_queries(xy, 3.0, desc, angle=[a for a, _ in pairs] if n else 0.0)
    return keys, desc, q


def _rotation(name, bins_counts, rejected_bins, extra=(), extra_bins=()):
    keys, desc, q = planted(bins_counts, extra)
    n = len(keys)
    bin_of = [b for b, c in bins_counts for _ in range(c)] + list(extra_bins)
    cleared = [i for i in range(n) if bin_of[i] in rejected_bins]
    want = {(m, False): expectation(n, np.arange(n)) for m in (0, 1)}
    want.update({(m, True): expectation(n, np.arange(n), cleared) for m in (0, 1)})
    return raw_case(name, keys, desc, q, want, why="bins %s: %s rejected" % (bins_counts, sorted(rejected_bins)))


def rotation_cases():
    """float32(0.1) * 10, * 20 and * 100 round to 1.0, 2.0 and 10.0, so a second or third maximum of exactly a tenth stays
    (`max2 < 0.1f * (float)max1` is false).  Equal bins: the strict comparisons keep the first three in bin order."""
    return [_rotation("rotation-10-1-1", [(2, 10), (5, 1), (7, 1)], set()),
            _rotation("rotation-10-1-0", [(2, 10), (5, 1)], set()),
            _rotation("rotation-20-2-1", [(2, 20), (5, 2), (7, 1)], {7}),
            _rotation("rotation-100-10-9", [(2, 100), (5, 10), (7, 9)], {7}),
            _rotation("rotation-ties-5-5-5-5", [(1, 5), (4, 5), (6, 5), (9, 5)], {9}),
            _rotation("rotation-7-7-3-3", [(8, 7), (3, 7), (10, 3), (5, 3)], {10}),      # bin 5 comes before bin 10: it is the third
            _rotation("rotation-single-bin", [(4, 6)], set()),
            _rotation("rotation-no-match", [], set()),
            # -0.5 degrees wraps to 359.5 -> bin 12; 14.9 -> bin 0 and 15.0 -> bin 1 (15 * float32(1 / 30) rounds to 0.5, away from zero)
            _rotation("rotation-wrap-and-half-bin", [(3, 4), (6, 4), (12, 3)], {0, 1}, extra=[(10.0, 10.5), (14.9, 0.0), (15.0, 0.0)], extra_bins=[12, 0, 1]),
            _rotation("rotation-wrap-joins-bin-12", [(3, 4), (6, 4), (12, 3), (9, 4)], {9}, extra=[(10.0, 10.5), (100.25, 100.75)], extra_bins=[12, 12])]


def duplicate_case(mirror):
    """Two queries on one keypoint K: query 0's point has no observations, so query 1 takes K as well and the histogram holds K twice.
    30 further matches fix the three maxima at bins 2, 4, 6.  Plain: query 0's entry lies in bin 9 (rejected), query 1's in bin 2 (kept);
    mirror: the other way round.  The reference clears mvpMapPoints[K] for the rejected ENTRY (ORBmatcher.cc:1800, 1886-1889): K ends
    empty in both, and nmatches is the 32 matches less one."""
    keys, desc, q = planted([(2, 10), (4, 10), (6, 10)], extra=[(0.0, 0.0)])
    n = len(keys)
    K = n - 1
    dup = q[K:].copy()
    q = np.concatenate([q, dup])
    q["has_observations"][K] = 0
    q["angle"][K], q["angle"][K + 1] = (60.0, 270.0) if mirror else (270.0, 60.0)
    match = np.concatenate([np.arange(n), [K]])
    want = {(m, False): expectation(n, match) for m in (0, 1)}
    want.update({(m, True): expectation(n, match, [K]) for m in (0, 1)})
    return raw_case("duplicate-%s" % ("mirror" if mirror else "plain"), keys, desc, q, want)


def raw_cases():
    return chain_cases() + ratio_cases() + gate_cases() + rotation_cases() + [duplicate_case(False), duplicate_case(True)]


# ---- the keyframe overload ------------------------------------------------------------------------------------------------------------
FX = F32(128.0)
SF = (F32(1.2) ** np.arange(8, dtype=np.float32)).astype(np.float32)
LOG_SF = float(reloc_ref.logf(F32(1.2)))       # mfLogScaleFactor = log(mfScaleFactor), the C library's logf (numpy's float32 log is one unit off)
N_LEVELS = 8
IDENTITY = np.float32([0, 0, 0, 1, 0, 0, 0])
CAM_CORNER = np.float32([FX, FX, 0, 0])        # whole-pixel projections of points at depth 1 whose x, y are multiples of 1 / 128
CAM_CENTRE = np.float32([FX, FX, 160, 120])    # the point (0, 0, 1) lands on (160, 120)


def kf_points(uv, level, desc, angle=0.0, raw=None):
    """Points at depth 1 that project onto pixel uv under CAM_CORNER, searched on `level` (max_distance_raw = dist * 1.2^(level - 0.5):
    the level is never in doubt), or with the given max_distance_raw."""
    uv = np.asarray(uv, np.float32).reshape(-1, 2)
    n = len(uv)
    Xw = np.stack([uv[:, 0] / FX, uv[:, 1] / FX, np.ones(n, np.float32)], 1).astype(np.float32)
    dist = np.sqrt((Xw.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    if raw is None:
        raw = (dist * F32(1.2) ** (np.asarray(level, np.float32).reshape(n) - F32(0.5))).astype(np.float32)
    ang = np.zeros(n, np.float32)
    ang[:] = angle
    return dict(has_point=np.ones(n, np.uint8), found=np.zeros(n, np.uint8), Xw=Xw, point_descriptors=np.asarray(desc, np.uint8).reshape(n, 32),
                min_distance=np.zeros(n, np.float32), max_distance=np.full(n, 1e9, np.float32), max_distance_raw=np.asarray(raw, np.float32).reshape(n), angle=ang)


def kf_item(keys, desc, pts, held=None):
    n = len(keys)
    return dict(keys=keys, descriptors=np.asarray(desc, np.uint8).reshape(n, 32), held=np.zeros(n, np.uint8) if held is None else np.asarray(held, np.uint8),
                pose7=IDENTITY, bounds=[0, W, 0, H], **pts)


def ulp_neighbour(x, steps):
    x = F32(x)
    for _ in range(abs(steps)):
        x = np.nextafter(x, F32(np.inf if steps > 0 else -np.inf))
    return F32(x)


def boundary_centre(k):
    """1.2^k as the levels see it: the power of the float scale factor (mfScaleFactor = 1.2f, mfLogScaleFactor = log(1.2f)), as a float."""
    return F32(float(F32(1.2)) ** k)


def level_items():
    """One item per ratio: the camera at the identity and the point (0, 0, 1), so dist == 1 and max_distance_raw / dist is
    max_distance_raw itself.  Ratios: float32(1.2^k) for k = 0 .. 7 and its neighbours at -8 .. +8 ulps (the level is k or k + 1), two
    below 1 (the level clamps to 0) and two far above 1.2^7 (clamps to 7).  The item's one keypoint sits on the projection, on an octave
    that only one of the two candidate levels reaches (window level - 1 .. level + 1), so the match tells the level.
    -> (items, ratios, octaves, cam4, th)."""
    d = np.random.default_rng(31).integers(0, 256, 32, dtype=np.uint8)
    ratios, octaves = [], []
    for k in range(8):
        for s in range(-8, 9):
            ratios.append(ulp_neighbour(boundary_centre(k), s))
            octaves.append(2 if k == 0 else k - 1)     # k == 0: octave 2 is reached from level 1 only; else octave k - 1 from level k only
    for r, o in ((0.5, 2), (0.999, 2), (1.2 ** 9.5, 7), (1.2 ** 9.5, 5), (1e6, 7)):   # level 0: octave 2 is out; level 7: octave 7 in, 5 out
        ratios.append(F32(r)); octaves.append(o)
    items = []
    for r, o in zip(ratios, octaves):
        pts = dict(has_point=np.ones(1, np.uint8), found=np.zeros(1, np.uint8), Xw=np.float32([[0, 0, 1]]), point_descriptors=d.reshape(1, 32),
                   min_distance=np.zeros(1, np.float32), max_distance=np.full(1, 1e9, np.float32), max_distance_raw=np.float32([r]), angle=np.zeros(1, np.float32))
        items.append(kf_item(make_keys([(160, 120)], o), [d], pts))
    return items, ratios, octaves, CAM_CENTRE, 10.0


def kf_chain_item(L):
    """The chain of `chain(L, "plain")` through the keyframe overload: L points on pixel (160, 120), level 0, th = 40."""
    d = np.random.default_rng(2000 + L).integers(0, 256, 32, dtype=np.uint8)
    keys = make_keys(_lattice(L, 148, 108))
    item = kf_item(keys, np.tile(d, (L, 1)), kf_points(np.tile(np.float32([160, 120]), (L, 1)), np.zeros(L), np.tile(d, (L, 1))))
    return item, np.argsort(np.asarray(scan_order(keys))).astype(np.int32)   # keypoint i holds the point whose turn it was taken in


def orb_dist_items(orb_dist):
    """One point on one keypoint at Hamming distance orb_dist (a match) and orb_dist + 1 (none)."""
    d = np.random.default_rng(33).integers(0, 256, 32, dtype=np.uint8)
    return [kf_item(make_keys([(100, 100)]), [flip(d, 0, n)], kf_points([(100, 100)], [0], [d])) for n in (orb_dist, orb_dist + 1)]


STAGE_COUNTS = (15, 16, 17, 31, 32, 33)


def stage_item(n):
    """Point 0's window (pixel (160, 120), level 2, th = 10: radius 14.4) holds n candidates after the static tests, beside three keys
    that fail them (one held, one two octaves below, one two above); its descriptor is that of the LAST candidate of the scan, all others
    are far.  Point 1, the next query of the same workgroup, has one candidate, its own, in the first grid column of its window (so it
    is staged before point 0's walk reaches its last candidate).  n = 15, 16, 17, 31, 32, 33 surround the 16 and 32 entries a sub-group
    stages in LDS: the entry past the stage belongs to the neighbour."""
    rng = np.random.default_rng(40 + n)
    xy = _lattice(n + 3, 154, 114, per_row=9)
    keys = make_keys(xy, 2)
    desc = rng.integers(0, 256, (n + 4, 32), dtype=np.uint8)
    order = scan_order(keys)
    held = np.zeros(n + 4, np.uint8)
    fail = [order[1], order[5], order[len(order) // 2]]
    held[fail[0]] = 1
    keys["octave"][fail[1]], keys["octave"][fail[2]] = 0, 4
    last = [k for k in order if k not in fail][-1]
    keys = np.concatenate([keys, make_keys([(27, 40)], 2)])     # cell column 5, the first of the window 25.6 .. 54.4
    pts = kf_points([(160, 120), (40, 40)], [2, 2], [desc[last], desc[n + 3]])
    return kf_item(keys, desc, pts, held), last


def rotation_items():
    """The rotation cases as keyframe items (check_orientation = True: k_track_count), an item with keys and no points and one with
    points and no keys among them."""
    items = []
    for c in rotation_cases() + [duplicate_case(False)]:
        q = c["queries"]
        if c["name"].startswith("duplicate"):
            q = q[:-1]       # the keyframe overload's points all have observations: no duplicate there
        uv = np.stack([q["u"], q["v"]], 1)
        items.append(kf_item(c["keys"], c["desc"], kf_points(uv, np.zeros(len(q)), q["descriptor"], angle=q["angle"])))
    d = np.random.default_rng(50).integers(0, 256, (4, 32), dtype=np.uint8)
    items.insert(3, kf_item(make_keys([(30, 30), (60, 60), (90, 90), (120, 120)]), d, kf_points(np.zeros((0, 2)), np.zeros(0), np.zeros((0, 32)))))
    items.insert(6, kf_item(make_keys(np.zeros((0, 2))), np.zeros((0, 32)), kf_points([(30, 30), (60, 60)], [0, 0], d[:2])))
    return items
