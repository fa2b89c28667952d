"""GPU parity of relocalisation: TemplatedVocabulary::score, DetectRelocalizationCandidates and the keyframe overload of SearchByProjection
against the line-by-line restatement tests/reloc_ref.py, byte for byte (doubles and floats compared as bits), and the refinement ladder stage by
stage (searches byte for byte, each PoseOptimization against the oracle)."""
import numpy as np
import pytest

import bow_ref as B
import reloc_ref as R

pytestmark = pytest.mark.gpu

W, H = 640, 240
N_VOC = 10 ** 4


@pytest.fixture(scope="module")
def tree():
    return B.random_tree(10, 4, seed=21, stop_frac=0.0)


def _voc(pkg, tree, scoring):
    p, lf, d, w = tree
    return pkg.Vocabulary.from_arrays(10, 4, scoring, B.TF_IDF, p, lf, d, w)


def _bits(x, dtype):
    return np.ascontiguousarray(x, dtype).tobytes()


# ---- score ---------------------------------------------------------------------------------------------------------------------------
def _score_pairs(rng):
    big1, big2 = R.random_bow(rng, N_VOC, 4096), R.random_bow(rng, N_VOC, 4096)
    a = R.random_bow(rng, N_VOC, 300)
    one = (np.array([a[0][17], N_VOC - 1], np.int32), np.array([0.25, 0.75]))
    lo = (np.arange(0, 200, 2, dtype=np.int32), np.full(100, 0.01))
    hi = (np.arange(1, 200, 2, dtype=np.int32), np.full(100, 0.01))
    empty = (np.zeros(0, np.int32), np.zeros(0))
    heavy = (np.arange(5, dtype=np.int32), np.full(5, 0.6))                       # L2: the sum passes 1
    signed1 = (np.arange(64, dtype=np.int32), np.where(np.arange(64) % 3 == 0, -0.5, 0.25))
    signed2 = (np.arange(64, dtype=np.int32), np.where(np.arange(64) % 3 == 0, 0.5, 0.125))   # chi-square: vi + wi == 0 on every third word
    pairs = [(empty, empty), (empty, a), (a, empty), (lo, hi), (a, a), (a, one), (one, a), (big1, big2), (big2, big1), (big1, big1),
             (heavy, heavy), (signed1, signed2), (signed2, signed1)]
    for _ in range(40):
        base = R.random_bow(rng, N_VOC, int(rng.integers(1, 1500)))[0]
        pairs.append((R.random_bow(rng, N_VOC, int(rng.integers(1, 1500)), base, 0.7), R.random_bow(rng, N_VOC, int(rng.integers(1, 1500)), base, 0.5)))
    return pairs


@pytest.mark.parametrize("scoring", [R.L1_NORM, R.L2_NORM, R.CHI_SQUARE, R.BHATTACHARYYA, R.DOT_PRODUCT])
def test_score_random_vectors(pkg, tree, scoring):
    voc = _voc(pkg, tree, scoring)
    pairs = _score_pairs(np.random.default_rng(scoring))
    if scoring == R.BHATTACHARYYA:   # sqrt of a negative product is NaN on both sides, and NaN has more than one bit pattern
        pairs = [p for p in pairs if (p[0][1] >= 0).all() and (p[1][1] >= 0).all()]
    got = voc.score(pairs)
    want = np.array([R.score(scoring, p[0], p[1]) for p in pairs])
    assert got.dtype == np.float64 and _bits(got, np.float64) == _bits(want, np.float64), np.flatnonzero(got != want)
    assert len(set(want.tolist())) > 10
    if scoring == R.L1_NORM:
        assert want[0] == 0 and np.signbit(got[0])                                 # -0.0 / 2
    if scoring == R.L2_NORM:
        assert got[10] == 1.0


def _drive_descriptors(pkg, synthetic, xs, seed=5):
    import torch
    sc = synthetic.Scene(seed)
    imgs = []
    for k, x in enumerate(xs):
        imgs.append(sc.render(float(x), W, H, noise_seed=2 * k + 1)[0])
        imgs.append(sc.render(float(x) + synthetic.BASELINE, W, H, noise_seed=2 * k + 2)[0])
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    ext = pkg.OrbExtractor(nfeatures=1000, max_width=W, max_height=H, max_images=len(imgs))
    _, desc, counts, _ = ext.extract_batch_dev(dev.data_ptr(), len(imgs), W, H, W, W * H)
    torch.cuda.synchronize()
    return [desc[2 * f][:counts[2 * f]].copy() for f in range(len(xs))]


@pytest.fixture(scope="module")
def real_descriptors(pkg, synthetic):
    return _drive_descriptors(pkg, synthetic, [0.0, 0.1, 0.2, 0.4, 0.8, 1.6])


@pytest.mark.parametrize("scoring", [R.L1_NORM, R.L2_NORM, R.CHI_SQUARE, R.BHATTACHARYYA, R.DOT_PRODUCT])
def test_score_real_frames(pkg, tree, real_descriptors, scoring):
    voc = _voc(pkg, tree, scoring)
    bows = voc.transform(real_descriptors, levelsup=2)
    vecs = [(b["bow_word"], b["bow_value"]) for b in bows]
    assert min(len(v[0]) for v in vecs) > 200
    pairs = [(a, b) for a in vecs for b in vecs]
    got = voc.score(pairs)
    want = np.array([R.score(scoring, a, b) for a, b in pairs])
    assert _bits(got, np.float64) == _bits(want, np.float64)
    assert (want != 0).sum() > len(vecs)                                           # frames of one scene share words


def test_kl_is_rejected(pkg, tree):
    voc = _voc(pkg, tree, R.KL)
    with pytest.raises(pkg.Tc2liError) as e:
        voc.score([(([1], [1.0]), ([1], [1.0]))])
    assert e.value.code == -2 and "KL" in str(e.value)
    db = pkg.KeyFrameDatabase(voc)
    db.add(1, 0, [1], [1.0])
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.detect_relocalization_candidates_batch([(db, 0, [1], [1.0])])
    assert e.value.code == -2 and "KL" in str(e.value)


# ---- DetectRelocalizationCandidates -----------------------------------------------------------------------------------------------------
class Mirror:
    """One database on the device and its restatement, driven by the same calls."""

    def __init__(self, pkg, voc, scoring=R.L1_NORM):
        self.pkg, self.dev, self.ref = pkg, pkg.KeyFrameDatabase(voc), R.KeyFrameDatabase(scoring)

    def add(self, kf_id, map_id, bow, neighbours=None):
        seq = self.dev.add(kf_id, map_id, *bow)
        assert seq == self.ref.add(kf_id, map_id, *bow).sequence
        if neighbours is not None:
            self.set_covisibility(kf_id, neighbours)

    def erase(self, kf_id):
        self.dev.erase(kf_id)
        self.ref.erase(kf_id)

    def clear_map(self, map_id):
        self.dev.clear_map(map_id)
        self.ref.clear_map(map_id)

    def set_covisibility(self, kf_id, ids):
        self.dev.set_covisibility(kf_id, ids)
        self.ref.set_covisibility(kf_id, ids)

    def check_entries(self):
        e = self.dev.entries()
        live = sorted(self.ref.live.values(), key=lambda kf: kf.sequence)
        assert e["kf_id"].tolist() == [kf.kf_id for kf in live] and e["sequence"].tolist() == [kf.sequence for kf in live]
        assert _bits(e["score"], np.float32) == _bits([kf.reloc_score for kf in live], np.float32)   # mRelocScore

    def query(self, map_id, bow):
        cands, scored = self.pkg.detect_relocalization_candidates_batch([(self.dev, map_id, *bow)], scored_capacity=max(len(self.dev), 1))
        want = self.ref.detect_relocalization_candidates(map_id, *bow)
        _same_result(cands[0], scored[0], want)
        self.check_entries()
        return want


def _same_result(cands, scored, want, what=""):
    wc, ws = want
    assert cands.tolist() == wc, what
    assert scored["kf_id"].tolist() == [s[0] for s in ws], what
    assert scored["words"].tolist() == [s[1] for s in ws], what
    assert _bits(scored["si"], np.float32) == _bits([s[2] for s in ws], np.float32), what
    assert _bits(scored["acc_score"], np.float32) == _bits([s[3] for s in ws], np.float32), what
    assert scored["best_kf_id"].tolist() == [s[4] for s in ws], what


def _places(rng, n_places, n_base=150):
    return [np.unique(rng.integers(0, N_VOC, n_base)).astype(np.int32) for _ in range(n_places)]


def _fill(m, rng, places, n_kf, n_words=200, maps=1, first_id=0):
    """n_kf keyframes, each of a random place, each with up to ten neighbours among the keyframes added before it (and now and then an id
    that is no entry)."""
    place_of = {}
    for i in range(n_kf):
        kf_id = first_id + i
        p = int(rng.integers(len(places)))
        place_of[kf_id] = p
        near = [k for k, q in place_of.items() if q == p and k != kf_id]
        far = [k for k in place_of if k != kf_id]
        neigh = [int(k) for k in rng.permutation(near)[:int(rng.integers(0, 8))]] + [int(k) for k in rng.permutation(far)[:int(rng.integers(0, 4))]]
        if rng.random() < 0.1:
            neigh.insert(0, 10 ** 6 + i)
        m.add(kf_id, int(rng.integers(maps)), R.random_bow(rng, N_VOC, n_words, places[p], rng.uniform(0.75, 1.0)), neigh[:10])
    return place_of


@pytest.mark.parametrize("n_kf,scoring", [(1, R.L1_NORM), (50, R.L1_NORM), (2000, R.L1_NORM), (50, R.L2_NORM), (50, R.CHI_SQUARE),
                                          (50, R.BHATTACHARYYA), (50, R.DOT_PRODUCT)])
def test_query_equals_restatement(pkg, tree, n_kf, scoring):
    rng = np.random.default_rng(100 + n_kf + scoring)
    voc = _voc(pkg, tree, scoring)
    places = _places(rng, 1 if n_kf == 1 else 6)
    m = Mirror(pkg, voc, scoring)
    _fill(m, rng, places, n_kf)
    n_cand = 0
    for q in range(4):
        cands, scored = m.query(0, R.random_bow(rng, N_VOC, 200, places[q % len(places)], 0.9))
        n_cand += len(cands)
        assert len(scored) >= 1
    assert n_cand >= 4
    cands, scored = m.query(0, (np.zeros(0, np.int32), np.zeros(0)))               # a frame without words
    assert cands == [] and scored == []


def test_query_sequence_with_stale_scores(pkg, tree):
    """Four and more queries on one handle with erase / add / set_covisibility between them: the accumulated scores depend on what
    earlier queries stored in keyframes that share a word with the frame but fail the word gate."""
    rng = np.random.default_rng(5)
    voc = _voc(pkg, tree, R.L1_NORM)
    # a small range of noise words, so that keyframes of different places share a few words
    places = [np.unique(rng.integers(0, 2000, 150)).astype(np.int32) for _ in range(3)]
    bow = lambda p, keep=0.9: R.random_bow(rng, 2000, 210, places[p], keep)
    m = Mirror(pkg, voc)
    place_of = {}
    for kf_id in range(60):
        place_of[kf_id] = kf_id % 3
        m.add(kf_id, 0, bow(kf_id % 3), [k for k in range(max(0, kf_id - 7), kf_id)])   # neighbours of every place
    fresh_differs = 0

    def query(p):
        nonlocal fresh_differs
        frame = bow(p)
        # what a database with the same content but no history gives
        fresh = R.KeyFrameDatabase()
        for kf in sorted(m.ref.live.values(), key=lambda kf: kf.sequence):
            fresh.add(kf.kf_id, kf.map_id, kf.words, kf.values)
            fresh.set_covisibility(kf.kf_id, kf.neighbours)
        _, want = m.query(0, frame)
        _, clean = fresh.detect_relocalization_candidates(0, *frame)
        assert [s[0] for s in want] == [s[0] for s in clean]
        fresh_differs += sum(1 for a, b in zip(want, clean) if a[3] != b[3])

    query(0)
    query(1)
    m.erase(4); m.erase(10)
    m.add(100, 0, bow(1), [1, 7, 13, 0, 3])
    query(1)
    m.set_covisibility(5, [100, 2, 8, 0, 1])
    m.add(4, 0, bow(2), [2, 5, 8, 100])                  # an erased id comes back: a new entry, score state 0
    query(2)
    query(0)
    for k in range(20, 45):
        m.erase(k)
    for k in range(45, 60):
        m.erase(k)                                       # the dead rows pass half of the pool on the way: compaction
    m.add(200, 0, bow(0), [0, 1, 2, 3])
    query(0)
    query(2)
    assert fresh_differs > 0, "no stale score reached an accumulated score: the case tests nothing"


def test_two_maps_in_one_database(pkg, tree):
    rng = np.random.default_rng(9)
    voc = _voc(pkg, tree, R.L1_NORM)
    places = _places(rng, 3)
    m = Mirror(pkg, voc)
    _fill(m, rng, places, 120, maps=2)
    seen = set()
    for q in range(6):
        cands, scored = m.query(q % 2, R.random_bow(rng, N_VOC, 200, places[q % 3], 0.9))
        assert all(m.ref.live[k].map_id == q % 2 for k in cands)
        seen.update(m.ref.live[s[4]].map_id for s in scored)
    assert seen == {0, 1}
    m.clear_map(1)
    cands, _ = m.query(1, R.random_bow(rng, N_VOC, 200, places[0], 0.9))
    assert cands == []
    cands, _ = m.query(0, R.random_bow(rng, N_VOC, 200, places[0], 0.9))
    assert len(cands) > 0


def test_512_databases_in_one_call_equal_512_calls(pkg, tree):
    voc = _voc(pkg, tree, R.L1_NORM)
    n = 512

    def make():
        rng = np.random.default_rng(77)
        ms, frames = [], []
        for d in range(n):
            places = _places(rng, 2, 80)
            m = Mirror(pkg, voc)
            _fill(m, rng, places, int(rng.integers(0, 24)), n_words=100)
            ms.append(m)
            frames.append(R.random_bow(rng, N_VOC, 100, places[0], 0.9))
        return ms, frames

    a, frames = make()
    b, _ = make()
    for rounds in range(2):   # the second round meets stored scores
        cands, scored = pkg.detect_relocalization_candidates_batch([(m.dev, 0, *f) for m, f in zip(a, frames)], capacity=32, scored_capacity=32)
        for d in range(n):
            c1, s1 = pkg.detect_relocalization_candidates_batch([(b[d].dev, 0, *frames[d])], capacity=32, scored_capacity=32)
            assert c1[0].tolist() == cands[d].tolist(), d
            for key in s1[0]:
                assert s1[0][key].tobytes() == scored[d][key].tobytes(), (d, key)
            if d % 16 == 0:
                _same_result(cands[d], scored[d], a[d].ref.detect_relocalization_candidates(0, *frames[d]), d)
                a[d].check_entries()
        assert sum(len(c) for c in cands) > n // 2


def test_duplicate_handle_and_capacity(pkg, tree):
    rng = np.random.default_rng(13)
    voc = _voc(pkg, tree, R.L1_NORM)
    places = _places(rng, 1)
    m = Mirror(pkg, voc)
    for kf_id in range(12):
        m.add(kf_id, 0, R.random_bow(rng, N_VOC, 200, places[0], 0.95), [])
    frame = R.random_bow(rng, N_VOC, 200, places[0], 0.95)
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.detect_relocalization_candidates_batch([(m.dev, 0, *frame), (m.dev, 0, *frame)])
    assert e.value.code == -2 and "twice" in str(e.value)
    m.check_entries()                                                              # refused before anything ran
    want, _ = m.ref.detect_relocalization_candidates(0, *frame)
    assert len(want) >= 3
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.detect_relocalization_candidates_batch([(m.dev, 0, *frame)], capacity=len(want) - 1)
    assert e.value.code == -5  # TC2LI_ERR_CAPACITY
    with pytest.raises(pkg.Tc2liError) as e:
        pkg.detect_relocalization_candidates_batch([(m.dev, 0, *frame)], capacity=len(want), scored_capacity=1)
    assert e.value.code == -5
    cands, _ = pkg.detect_relocalization_candidates_batch([(m.dev, 0, *frame)], capacity=len(want))
    assert cands[0].tolist() == want


# ---- SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) ------------------------------------------------------------------
def _extract(pkg, synthetic, xs, seed):
    """Stereo frames of one scene from camera positions xs: keys, descriptors and stereo depth of the left images."""
    import torch
    sc = synthetic.Scene(seed)
    imgs = []
    for k, x in enumerate(xs):
        imgs.append(sc.render(float(x), W, H, noise_seed=2 * k + 1)[0])
        imgs.append(sc.render(float(x) + synthetic.BASELINE, W, H, noise_seed=2 * k + 2)[0])
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    ext = pkg.OrbExtractor(nfeatures=1000, max_width=W, max_height=H, max_images=len(imgs))
    kps, desc, counts, _ = ext.extract_batch_dev(dev.data_ptr(), len(imgs), W, H, W, W * H)
    torch.cuda.synchronize()
    bf = np.float32(synthetic.BF); b = np.float32(bf / np.float32(synthetic.FX))
    u_right, depth, _ = pkg.stereo_match_batch(ext, len(xs), float(bf), float(b))
    frames = [dict(keys=kps[2 * f][:counts[2 * f]].copy(), descriptors=desc[2 * f][:counts[2 * f]].copy(), depth=depth[f, :counts[2 * f]].copy(),
                   u_right=u_right[f, :counts[2 * f]].copy()) for f in range(len(xs))]
    return ext, dev, frames


def _candidate_keyframe(synthetic, kf, x_kf, scale_factors, rng, spoil=True):
    """The keyframe's points in keypoint order, as MapPoint's constructor and UpdateNormalAndDepth leave them (SF/src/MapPoint.cc:444-503):
    mfMaxDistance = dist * mvScaleFactors[octave], mfMinDistance = mfMaxDistance / mvScaleFactors[nLevels - 1], the invariance range 0.8 /
    1.2 of those.  spoil: a few points moved far away, with a range the frame is outside of, with another descriptor, or with another angle,
    so that every gate of the search rejects something."""
    fx, fy, cx, cy = [np.float32(v) for v in (synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY)]
    n = len(kf["keys"])
    z = kf["depth"]
    zz = np.where(z > 0, z, 1).astype(np.float32)
    Xc = np.stack([(kf["keys"]["x"] - cx) * zz / fx, (kf["keys"]["y"] - cy) * zz / fy, zz], 1).astype(np.float32)
    dist = np.sqrt((Xc.astype(np.float32) ** 2).sum(1)).astype(np.float32)
    Xw = Xc.copy()
    Xw[:, 0] += np.float32(x_kf)                       # world = the camera frame at x = 0, cameras along x
    sf = np.asarray(scale_factors, np.float32)
    max_raw = (dist * sf[kf["keys"]["octave"]]).astype(np.float32)
    min_raw = (max_raw / sf[-1]).astype(np.float32)
    has_point = ((z > 0) & (rng.random(n) < 0.9)).astype(np.uint8)
    found = (rng.random(n) < 0.1).astype(np.uint8)
    desc = kf["descriptors"].copy()
    flip = rng.random(n) < 0.5                         # the map point's descriptor: another observation's, a few bits away
    desc[flip, rng.integers(0, 32, flip.sum())] ^= (1 << rng.integers(0, 8, flip.sum())).astype(np.uint8)
    angle = kf["keys"]["angle"].astype(np.float32).copy()
    max_d, min_d = (np.float32(1.2) * max_raw).astype(np.float32), (np.float32(0.8) * min_raw).astype(np.float32)
    if spoil:
        kind = rng.random(n)
        Xw[kind < 0.04, 0] += np.float32(30.0)
        far = (kind >= 0.04) & (kind < 0.10)
        max_d[far] *= np.float32(0.3)
        other = (kind >= 0.10) & (kind < 0.20)
        desc[other] = rng.integers(0, 256, (int(other.sum()), 32), dtype=np.uint8)
        turned = (kind >= 0.20) & (kind < 0.28)
        angle[turned] = np.mod(angle[turned] + np.float32(100.0), np.float32(360.0)).astype(np.float32)
    return dict(has_point=has_point, found=found, Xw=Xw, point_descriptors=desc, min_distance=min_d, max_distance=max_d, max_distance_raw=max_raw,
                angle=angle, keys=kf["keys"], depth=z)


@pytest.fixture(scope="module")
def reloc_scene(pkg, synthetic):
    xs = [0.0, 0.2, 0.4]
    ext_kf, _, kfs = _extract(pkg, synthetic, [x - 0.1 for x in xs], seed=8)      # keyframes 0.1 m from every frame
    ext, dev, frames = _extract(pkg, synthetic, xs, seed=8)
    return dict(xs=xs, ext=ext, dev=dev, frames=frames, kfs=kfs, scale_factors=np.asarray(ext.GetScaleFactors(), np.float32))


def _cam4(synthetic):
    return np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY])


def _check_search_by_projection_keyframe(pkg, oracle, synthetic, S):
    """Runs the search for both windows with and without the rotation filter and checks every result against reloc_ref.py.  Returns the
    results and, per search, (th, the window candidates of all items, the queries of the batch): with one pool entry per query a search
    overflows the pool when it has more candidates than queries."""
    got, pool = [], []
    sf = S["scale_factors"]
    log_sf = float(np.log(np.float32(sf[1])))          # mfLogScaleFactor = log(mfScaleFactor)
    rng = np.random.default_rng(31)
    items, ref_frames, ref_kfs = [], [], []
    for f, x in enumerate(S["xs"]):
        fr = S["frames"][f]
        held = (rng.random(len(fr["keys"])) < 0.1).astype(np.uint8)
        pose = np.array([0, 0, 0, 1, -x + 0.01, 0.004, -0.008], np.float32)
        kf = _candidate_keyframe(synthetic, S["kfs"][f], x - 0.1, sf, rng)
        items.append(dict(keys=fr["keys"], descriptors=fr["descriptors"], held=held, pose7=pose, bounds=[0, W, 0, H],
                          **{k: kf[k] for k in ("has_point", "found", "Xw", "point_descriptors", "min_distance", "max_distance", "max_distance_raw", "angle")}))
        ref_frames.append(dict(keys=fr["keys"], descriptors=fr["descriptors"], held=held, pose7=pose, cols=W, rows=H))
        ref_kfs.append(kf)
    cam4 = _cam4(synthetic)
    for th, orb_dist in ((10, 100), (3, 64)):
        for orient in (True, False):
            match, nm = pkg.search_by_projection_keyframe_batch(items, cam4, sf, log_sf, th, orb_dist, orient, capacity=S["ext"].capacity)
            got += [match, nm]
            total = dict(bounds=0, distance=0, orb_dist=0, histogram=0, candidates=0)
            for f in range(len(items)):
                want, n, rejected = R.search_by_projection_keyframe(oracle, ref_frames[f], ref_kfs[f], cam4, sf, log_sf, th, orb_dist, orient)
                N = len(want)
                assert np.array_equal(match[f, :N], want), (th, orb_dist, orient, f, np.flatnonzero(match[f, :N] != want)[:10])
                assert (match[f, N:] == -1).all() and nm[f] == n and n > 0, (th, orb_dist, orient, f, nm[f], n)
                assert not (want[ref_frames[f]["held"].astype(bool)] >= 0).any()
                for k in total:
                    total[k] += rejected[k]
            print("th %d ORBdist %d orientation %s: matches %s, rejected %s" % (th, orb_dist, orient, nm.tolist(), total))
            assert total["bounds"] > 0 and total["distance"] > 0 and total["orb_dist"] > 0, total
            assert (total["histogram"] > 0) == orient, total
            pool.append((th, total["candidates"], sum(len(kf["has_point"]) for kf in ref_kfs)))
    return got, pool


def test_search_by_projection_keyframe_batch(pkg, oracle, synthetic, reloc_scene):
    _check_search_by_projection_keyframe(pkg, oracle, synthetic, reloc_scene)


def test_search_by_projection_keyframe_pool_overflow_takes_the_one_kernel_path(pkg, oracle, synthetic, reloc_scene, monkeypatch):
    """With a candidate pool of one entry per query the list form overflows and the batch falls back to the one-kernel matcher: the
    results equal reloc_ref.py's (checked inside) and the default run's, array for array.  That the pool overflows is reloc_ref.py's count:
    the th = 10 searches have more window candidates than the batch has queries."""
    ref, _ = _check_search_by_projection_keyframe(pkg, oracle, synthetic, reloc_scene)
    monkeypatch.setenv("TC2LI_MATCH_POOL_PER_QUERY", "1")
    got, pool = _check_search_by_projection_keyframe(pkg, oracle, synthetic, reloc_scene)
    print("(th, window candidates, queries):", pool)
    assert all(cand > queries for th, cand, queries in pool if th == 10) and [th for th, _, _ in pool] == [10, 10, 3, 3], pool
    assert len(got) == len(ref) and all(np.array_equal(a, b) for a, b in zip(got, ref))


# ---- the refinement ladder ---------------------------------------------------------------------------------------------------------------
def _restrict(kf, keep):
    """The candidate with points only at the keypoints `keep` (a keyframe whose other points are bad or missing)."""
    hp = np.zeros_like(kf["has_point"])
    hp[keep] = kf["has_point"][keep]
    return dict(kf, has_point=hp)


def _check_relocalization_refine(pkg, oracle, synthetic, S, dense=False, batch=None):
    """Hypotheses from SearchByBoW matches (ratio 0.75), a true pose a few centimetres off and only the first k matches flagged as inliers;
    candidates with few points steer the searches, so that the batch reaches every exit of the ladder.  Every stage is checked from the
    device's own pose of the previous stage: searches byte for byte, each PoseOptimization against the oracle on the same edges.  `dense`
    keeps only hypotheses whose candidate has all its points, so that nearly every query of the batch is a live one.  Returns the batch's
    outputs and, per search, (its window candidates over all hypotheses, the queries of the batch): with one pool entry per query a
    search overflows the pool when it has more candidates than queries.  batch: a dict that receives the call's inputs (hyps, u_right,
    cam5) and check(hyps, refs, got), the comparison below for any list of these hypotheses and the outputs of a call on it."""
    sf = S["scale_factors"]
    log_sf = float(np.log(np.float32(sf[1])))
    ext = S["ext"]
    inv_sigma2 = ext.GetInverseScaleSigmaSquares()
    bf = np.float32(synthetic.BF)
    cam4 = _cam4(synthetic)
    cam5 = np.float32(list(cam4) + [bf]).astype(np.float64)
    rng = np.random.default_rng(17)
    p, lf, d, w = B.trained_tree(np.concatenate([k["descriptors"] for k in S["kfs"][:2]]), k=6, L=4, seed=3)
    voc = pkg.Vocabulary.from_arrays(6, 4, B.L1_NORM, B.TF_IDF, p, lf, d, w)
    nF = len(S["xs"])
    bows = voc.transform([k["descriptors"] for k in S["kfs"]] + [f["descriptors"] for f in S["frames"]], levelsup=2)
    u_right = np.full((nF, ext.capacity), -1, np.float32)
    hyps, refs = [], []
    for f, x in enumerate(S["xs"]):
        fr, kfr = S["frames"][f], S["kfs"][f]
        u_right[f, :len(fr["keys"])] = fr["u_right"]
        kf = _candidate_keyframe(synthetic, kfr, x - 0.1, sf, rng, spoil=False)
        kf["has_point"] = (kfr["depth"] > 0).astype(np.uint8)
        view = lambda a, b, hp=None: dict(keys=a["keys"], descriptors=a["descriptors"], fv_node=b["fv_node"], fv_offset=b["fv_offset"],
                                          fv_index=b["fv_index"], **({} if hp is None else dict(has_point=hp)))
        m, nm = pkg.search_by_bow_batch([dict(keyframe=view(kfr, bows[f], kf["has_point"]), frame=view(fr, bows[nF + f]), nn_ratio=0.75,
                                              check_orientation=True)], capacity=ext.capacity)
        match = m[0, :len(fr["keys"])]
        ids = np.flatnonzero(match >= 0)
        assert nm[0] == len(ids) and len(ids) >= 80, len(ids)
        pose = np.array([0, 0, 0, 1, -x + 0.02, 0.01, -0.015], np.float32)
        others = np.setdiff1d(np.flatnonzero(kf["has_point"]), match[ids])     # the keyframe's points SearchByBoW did not match
        rng.shuffle(others)

        def hyp(k, cand):
            inl = np.zeros(len(match), np.uint8)
            inl[ids[:k]] = 1
            hyps.append(dict(frame_index=f, pose7=pose, match=match, inlier=inl, **{n: cand[n] for n in (
                "has_point", "Xw", "point_descriptors", "min_distance", "max_distance", "max_distance_raw", "angle")}))
            refs.append((f, cand, inl))
        if dense:
            hyp(14, kf)
            for shift in (0.3, 0.6):                                             # as below, with every point
                moved = dict(kf, Xw=kf["Xw"].copy())
                moved["Xw"][match[ids[:14]], 0] += np.float32(shift)
                hyp(14, moved)
            continue
        hyp(5, kf)                                                               # rejected
        hyp(len(ids), kf)                                                        # success without a search
        hyp(14, _restrict(kf, np.concatenate([match[ids[:14]], others[:10]])))   # the first search is not enough
        hyp(14, kf)                                                              # the second optimisation reaches 50
        for extra in (38, 42, 46, 50, 54, 60, 70):                               # 30 < nGood < 50 after the second: the narrow search runs
            hyp(14, _restrict(kf, np.concatenate([match[ids[:14]], others[:extra]])))
        # With good inliers the (10, 100) search finds whatever the (3, 64) search could find, so the third optimisation is out of reach.  It
        # is reached the way the reference meets it: by a pose that improves in between.  The 14 inlier points have moved by 0.2 to 0.6 m, the first
        # optimisation follows them, the wide search finds the distant points only, the second optimisation (no discard) lands on those,
        # and the narrow search collects the near ones.
        for shift in (0.2, 0.3, 0.45, 0.6):
            moved = dict(kf, Xw=kf["Xw"].copy())
            moved["Xw"][match[ids[:14]], 0] += np.float32(shift)
            for extra in (70, 100, 140):
                hyp(14, _restrict(moved, np.concatenate([match[ids[:14]], others[:extra]])))
    got = pkg.relocalization_refine_batch(ext, hyps, u_right, cam5)
    seen = set()
    by_hand = {0: [], 1: []}

    def check(hyps, refs, got, seen, by_hand):
        for h, (f, cand, inl) in enumerate(refs):
            fr = S["frames"][f]
            N = len(fr["keys"])
            frame = dict(keys=fr["keys"], descriptors=fr["descriptors"], u_right=u_right[f, :N], cols=W, rows=H)
            ref = R.relocalization_refine(oracle, frame, cand, hyps[h]["pose7"], hyps[h]["match"], inl, cam5, inv_sigma2, sf, log_sf, device_poses=got["poses7"][h])
            print("hypothesis %d (frame %d): status %d (want %d), nGood %d (%d), nadditional %s (%s)" % (
                h, f, got["status"][h], ref["status"], got["n_good"][h], ref["n_good"], got["n_additional"][h].tolist(), ref["n_additional"]))
            assert got["status"][h] == ref["status"], h
            assert got["n_good"][h] == ref["n_good"] and got["n_additional"][h].tolist() == ref["n_additional"], h
            for stage in range(3):
                if ref["outliers"][stage] is None:
                    assert not got["poses7"][h, stage].any()
                else:   # the tolerance test_track_reference_keyframe_batch uses for this kernel against this oracle
                    assert np.allclose(got["poses7"][h, stage], ref["poses"][stage], rtol=1e-4, atol=1e-6), (h, stage, got["poses7"][h, stage], ref["poses"][stage])
            assert np.array_equal(got["kf_keypoint_of_keypoint"][h, :N], ref["assign"]), h
            assert (got["kf_keypoint_of_keypoint"][h, N:] == -1).all()
            assert np.array_equal(got["outlier"][h, :N], ref["outlier"]), h
            for which in range(2):
                if ref["searches"][which] is not None:
                    by_hand[which].append((h, f, cand, ref["searches"][which]))
            st = int(got["status"][h])
            seen.add("rejected" if st & R.REJECTED else "success without search" if st == R.OPT1 | R.SUCCESS else
                     "first search not enough" if st == R.OPT1 | R.SEARCH1 else "second optimisation" if st == R.OPT1 | R.SEARCH1 | R.OPT2 | R.SUCCESS else
                     "third optimisation" if st & R.OPT3 else "final failure" if not st & R.SUCCESS else "other")
            if st & R.OPT3 and not st & R.SUCCESS:
                seen.add("final failure")
    check(hyps, refs, got, seen, by_hand)
    if batch is not None:
        batch.update(hyps=hyps, refs=refs, u_right=u_right, cam5=cam5, check=lambda hy, rf, gt: check(hy, rf, gt, set(), {0: [], 1: []}))
    assert dense or {"rejected", "success without search", "first search not enough", "second optimisation", "third optimisation", "final failure"} <= seen, seen
    queries = sum(len(h["has_point"]) for h in hyps)
    pool = [(sum(s[5] for _, _, _, s in by_hand[which]), queries) for which in range(2)]
    # the chain's searches are tc2li_search_by_projection_keyframe_batch with the same inputs
    for which, (th, orb_dist) in enumerate(((10, 100), (3, 64))):
        assert by_hand[which] or (dense and which == 1)
        if not by_hand[which]:
            continue
        items = [dict(keys=S["frames"][f]["keys"], descriptors=S["frames"][f]["descriptors"], held=s[2], pose7=s[4], bounds=[0, W, 0, H],
                      **dict({n: cand[n] for n in ("has_point", "Xw", "point_descriptors", "min_distance", "max_distance", "max_distance_raw", "angle")},
                             found=s[3])) for h, f, cand, s in by_hand[which]]
        match, nm = pkg.search_by_projection_keyframe_batch(items, cam4, sf, log_sf, th, orb_dist, True, capacity=ext.capacity)
        for k, (h, f, cand, s) in enumerate(by_hand[which]):
            assert np.array_equal(match[k, :len(s[0])], s[0]) and nm[k] == s[1] == got["n_additional"][h, which], (which, h)
    return got, pool


def test_relocalization_refine_batch(pkg, oracle, synthetic, reloc_scene):
    _check_relocalization_refine(pkg, oracle, synthetic, reloc_scene)


def test_relocalization_refine_pool_overflow_takes_the_one_kernel_path(pkg, oracle, synthetic, reloc_scene, monkeypatch):
    """The ladder with a candidate pool of one entry per query: every output equals the default run's (and, inside the check, the oracle's /
    reloc_ref.py's).  The pool is sized from the points of all hypotheses, so the batch is the dense one, and that its first search
    overflows the pool is reloc_ref.py's count: more window candidates than the batch has queries."""
    ref, _ = _check_relocalization_refine(pkg, oracle, synthetic, reloc_scene, dense=True)
    monkeypatch.setenv("TC2LI_MATCH_POOL_PER_QUERY", "1")
    got, pool = _check_relocalization_refine(pkg, oracle, synthetic, reloc_scene, dense=True)
    print("(window candidates, queries) of the two searches:", pool)
    assert pool[0][0] > pool[0][1], pool
    assert sorted(got) == sorted(ref) and all(np.array_equal(got[k], ref[k]) for k in ref)


# ---- the tables of a call: every one has its place in the call's block, whatever the call before left there -----------------------------
def _rows(got, rows):
    return {k: v[rows] for k, v in got.items()}


def _same_outputs(a, b):
    return sorted(a) == sorted(b) and all(np.array_equal(a[k], b[k]) for k in a)


def test_refine_grows_shrinks_and_reuses_its_buffers(pkg, oracle, synthetic, reloc_scene):
    """All hypotheses (checked against the reference inside the helper), one of them alone, all again, through the same per-thread buffers;
    then a hypothesis whose keyframe has no point between two ordinary ones.  The hypotheses are independent: a hypothesis' rows are the
    same in every batch, and the pointless one is checked against the reference as the others were."""
    B_ = {}
    got, _ = _check_relocalization_refine(pkg, oracle, synthetic, reloc_scene, batch=B_)
    hyps, refs, run = B_["hyps"], B_["refs"], lambda hy: pkg.relocalization_refine_batch(reloc_scene["ext"], hy, B_["u_right"], B_["cam5"])
    k = 3                                                                         # "the second optimisation reaches 50": both searches run
    assert _same_outputs(run([hyps[k]]), _rows(got, [k]))
    assert _same_outputs(run(hyps), got)
    f, cand, inl = refs[1]
    none = {n: np.zeros((0,) + np.asarray(cand[n]).shape[1:], np.asarray(cand[n]).dtype) for n in (
        "has_point", "Xw", "point_descriptors", "min_distance", "max_distance", "max_distance_raw", "angle")}
    empty = dict(hyps[1], match=np.full_like(hyps[1]["match"], -1), inlier=np.zeros_like(hyps[1]["inlier"]), **none)
    three = run([hyps[k], empty, hyps[-1]])
    assert _same_outputs(_rows(three, [0, 2]), _rows(got, [k, len(hyps) - 1]))
    B_["check"]([empty], [(f, none, empty["inlier"])], _rows(three, [1]))
    assert three["status"][1] & R.REJECTED and (three["kf_keypoint_of_keypoint"][1] == -1).all()


def test_three_databases_whose_scored_lists_end_off_a_boundary(pkg, tree):
    """Databases of 5, 70 and 9 keyframes in one call with a scored list: 3 queries x 70 list entries x 4 bytes = 840, no multiple of 256,
    so the scored tables lie off the boundaries a table starts on.  Against the restatement and against the three one-database calls on
    fresh copies."""
    voc = _voc(pkg, tree, R.L1_NORM)

    def make():
        rng = np.random.default_rng(78)
        ms, frames = [], []
        for n_kf in (5, 70, 9):
            places = _places(rng, 2, 80)
            m = Mirror(pkg, voc)
            _fill(m, rng, places, n_kf, n_words=100)
            ms.append(m)
            frames.append(R.random_bow(rng, N_VOC, 100, places[0], 0.9))
        return ms, frames

    a, frames = make()
    b, _ = make()
    for rounds in range(2):   # the second round meets stored scores
        cands, scored = pkg.detect_relocalization_candidates_batch([(m.dev, 0, *f) for m, f in zip(a, frames)], capacity=70, scored_capacity=70)
        for d in range(3):
            c1, s1 = pkg.detect_relocalization_candidates_batch([(b[d].dev, 0, *frames[d])], capacity=70, scored_capacity=70)
            assert c1[0].tolist() == cands[d].tolist(), d
            for key in s1[0]:
                assert s1[0][key].tobytes() == scored[d][key].tobytes(), (d, key)
            _same_result(cands[d], scored[d], a[d].ref.detect_relocalization_candidates(0, *frames[d]), d)
            a[d].check_entries()
        assert all(len(s["kf_id"]) > 0 for s in scored) and len(scored[1]["kf_id"]) > 9


def test_score_pairs_of_0_1_and_200_words(pkg, tree):
    voc = _voc(pkg, tree, R.L1_NORM)
    rng = np.random.default_rng(6)
    base = R.random_bow(rng, N_VOC, 200)[0]
    big = [R.random_bow(rng, N_VOC, 200, base, 0.8) for _ in range(2)]
    empty = (np.zeros(0, np.int32), np.zeros(0))
    one = (np.array([big[0][0][5]], np.int32), np.array([0.5]))
    pairs = [(empty, empty), (one, one), (big[0], big[1]), (one, big[0]), (empty, big[1]), (big[1], one)]
    assert all(len(w) == 200 for w, _ in big)
    got = voc.score(pairs)
    want = np.array([R.score(R.L1_NORM, p[0], p[1]) for p in pairs])
    assert _bits(got, np.float64) == _bits(want, np.float64) and len(set(want.tolist())) >= 4
