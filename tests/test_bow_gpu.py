"""GPU parity of the ORB vocabulary: ComputeBoW (tc2li_orb_compute_bow_batch on the device-resident features, and the host-descriptor
entry) and SearchByBoW(KeyFrame*, Frame&) against the line-by-line restatement tests/bow_ref.py, byte for byte."""
import numpy as np
import pytest

import bow_ref as R

pytestmark = pytest.mark.gpu

W, H = 640, 240


def _drive(pkg, synthetic, xs, seed=5, nfeatures=1000):
    """Left / right images of one scene seen from camera positions xs along the baseline axis, extracted on the device."""
    import torch
    sc = synthetic.Scene(seed)
    imgs = []
    for k, x in enumerate(xs):
        imgs.append(sc.render(float(x), W, H, noise_seed=2 * k + 1)[0])
        imgs.append(sc.render(float(x) + synthetic.BASELINE, W, H, noise_seed=2 * k + 2)[0])
    dev = torch.from_numpy(np.stack(imgs)).cuda()
    ext = pkg.OrbExtractor(nfeatures=nfeatures, max_width=W, max_height=H, max_images=len(imgs))
    kps, desc, counts, _ = ext.extract_batch_dev(dev.data_ptr(), len(imgs), W, H, W, W * H)
    torch.cuda.synchronize()
    frames = [dict(keys=kps[2 * f][:counts[2 * f]].copy(), descriptors=desc[2 * f][:counts[2 * f]].copy()) for f in range(len(xs))]
    return ext, dev, frames, counts[0::2].copy()


@pytest.fixture(scope="module")
def drive(pkg, synthetic):
    return _drive(pkg, synthetic, [0.0, 0.15, 0.3, 0.6])


@pytest.fixture(scope="module")
def full_voc(pkg):
    p, lf, d, w = R.random_tree(10, 6, seed=11)
    ref = R.Voc(10, 6, R.L1_NORM, R.TF_IDF, p, lf, d, w)
    return ref, pkg.Vocabulary.from_arrays(10, 6, R.L1_NORM, R.TF_IDF, p, lf, d, w)


@pytest.fixture(scope="module")
def trained(drive):
    descs = np.concatenate([f["descriptors"] for f in drive[2][:2]])
    return R.trained_tree(descs, k=5, L=3, seed=2)


def _same(got, want, what=""):
    for key in ("word", "node", "bow_word", "fv_node", "fv_offset", "fv_index"):
        assert np.array_equal(got[key], want[key]), (what, key)
    assert got["bow_value"].dtype == np.float64
    assert got["bow_value"].tobytes() == want["bow_value"].tobytes(), what


def test_compute_bow_full_vocabulary(pkg, drive, full_voc):
    ext, _, frames, counts = drive
    ref, h = full_voc
    assert h.info() == dict(k=10, L=6, scoring=0, weighting=0, nodes=1111111, words=10 ** 6)
    got = h.transform_orb(ext, counts, levelsup=4)
    for f, fr in enumerate(frames):
        assert len(fr["descriptors"]) > 300
        _same(got[f], R.transform(ref, fr["descriptors"], 4), "frame %d" % f)
    # levelsup 0 .. L on one frame (nid_level from L down to the root)
    d0 = frames[0]["descriptors"][:200]
    for lu in range(0, 7):
        _same(h.transform([d0], levelsup=lu)[0], R.transform(ref, d0, lu), "levelsup %d" % lu)


def test_host_entry_equals_device_entry_and_repeats(pkg, drive, full_voc):
    ext, _, frames, counts = drive
    _, h = full_voc
    a = h.transform_orb(ext, counts, levelsup=4, raw=True)
    b = h.transform_orb(ext, counts, levelsup=4, raw=True)
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), k
    dev = h.transform_orb(ext, counts, levelsup=4)
    host = h.transform([fr["descriptors"] for fr in frames], levelsup=4)
    for f in range(len(frames)):
        for k in dev[f]:
            assert dev[f][k].tobytes() == host[f][k].tobytes(), (f, k)


@pytest.mark.parametrize("scoring", range(6))
@pytest.mark.parametrize("weighting", range(4))
def test_trained_vocabulary_from_text(pkg, tmp_path, drive, trained, scoring, weighting):
    _, _, frames, _ = drive
    p, lf, d, w = trained
    ref = R.Voc(5, 3, scoring, weighting, p, lf, d, w)
    path = tmp_path / "voc.txt"
    R.write_text(path, ref)
    ref.weight = np.array([R.read_weight_6(x) for x in ref.weight])   # what the file holds
    h = pkg.Vocabulary.load_text(str(path))
    descs = [frames[2]["descriptors"], np.zeros((0, 32), np.uint8), frames[3]["descriptors"][:300]]   # a frame without keypoints
    got = h.transform(descs, levelsup=1)
    for f, dd in enumerate(descs):
        _same(got[f], R.transform(ref, dd, 1), "frame %d" % f)
    assert len(got[1]["fv_offset"]) == 1 and got[1]["fv_offset"][0] == 0 and len(got[1]["bow_word"]) == 0


def test_k20_vocabulary(pkg, drive):
    _, _, frames, _ = drive
    p, lf, d, w = R.random_tree(20, 3, seed=4, flips=30, stop_frac=0.1)
    ref = R.Voc(20, 3, R.L2_NORM, R.TF, p, lf, d, w)
    h = pkg.Vocabulary.from_arrays(20, 3, R.L2_NORM, R.TF, p, lf, d, w)
    descs = [frames[1]["descriptors"][:400]]
    for lu in (0, 1, 2):
        _same(h.transform(descs, levelsup=lu)[0], R.transform(ref, descs[0], lu), "levelsup %d" % lu)


def _view(fr, bow, has_point=None):
    v = dict(keys=fr["keys"], descriptors=fr["descriptors"], fv_node=bow["fv_node"], fv_offset=bow["fv_offset"], fv_index=bow["fv_index"])
    if has_point is not None:
        v["has_point"] = has_point
    return v


def _ref_view(fr, bow, has_point=None):
    return dict(angle=fr["keys"]["angle"], descriptors=fr["descriptors"], fv_node=bow["fv_node"], fv_offset=bow["fv_offset"],
                fv_index=bow["fv_index"], has_point=has_point)


def test_search_by_bow_batch(pkg, drive, trained):
    ext, _, frames, counts = drive
    p, lf, d, w = trained
    h = pkg.Vocabulary.from_arrays(5, 3, R.L1_NORM, R.TF_IDF, p, lf, d, w)
    bows = h.transform_orb(ext, counts, levelsup=1)
    rng = np.random.default_rng(3)
    pairs, refs = [], []
    for kf in range(len(frames)):
        for f in range(len(frames)):
            if kf == f:
                continue
            n = len(frames[kf]["keys"])
            hp = (rng.random(n) > (0.0 if (kf + f) % 2 else 0.3)).astype(np.uint8)   # keyframes with missing / bad points
            ratio, orient = (0.7, True) if (kf + 2 * f) % 4 < 2 else (0.75, bool((kf + f) % 2))
            pairs.append(dict(keyframe=_view(frames[kf], bows[kf], hp), frame=_view(frames[f], bows[f]), nn_ratio=ratio, check_orientation=orient))
            refs.append(R.search_by_bow(_ref_view(frames[kf], bows[kf], hp), _ref_view(frames[f], bows[f]), ratio, orient))
    match, nm = pkg.search_by_bow_batch(pairs, capacity=ext.capacity)
    total = 0
    for i, (m, n) in enumerate(refs):
        N = len(m)
        assert np.array_equal(match[i][:N], m), i
        assert (match[i][N:] == -1).all()
        assert nm[i] == n, (i, nm[i], n)
        total += n
    assert total > 100
    assert any(p["check_orientation"] for p in pairs) and any(not p["check_orientation"] for p in pairs)


def test_host_entry_frame_beyond_one_tile(pkg, drive, full_voc):
    """More than 1024 descriptors (the LDS tile of the per-frame assembly) and more than 1024 distinct words in one frame."""
    _, _, frames, _ = drive
    ref, h = full_voc
    rows = np.random.default_rng(9).integers(0, 256, (2500, 32), dtype=np.uint8)
    descs = [frames[0]["descriptors"], rows, frames[1]["descriptors"][:5]]
    got = h.transform(descs, levelsup=4)
    for f, dd in enumerate(descs):
        want = R.transform(ref, dd, 4)
        _same(got[f], want, "frame %d" % f)
    assert len(got[1]["bow_word"]) > 1024
    for scoring, weighting in ((R.L2_NORM, R.TF), (R.DOT_PRODUCT, R.TF_IDF)):
        p, lf, d, w = R.random_tree(4, 6, seed=6, flips=25, stop_frac=0.05)
        r2 = R.Voc(4, 6, scoring, weighting, p, lf, d, w)
        h2 = pkg.Vocabulary.from_arrays(4, 6, scoring, weighting, p, lf, d, w)
        _same(h2.transform([rows], levelsup=2)[0], R.transform(r2, rows, 2), "scoring %d" % scoring)


def test_slices_feed_search_for_triangulation(pkg, oracle, synthetic):
    """A transform's FeatureVector slices, handed to tc2li_keyframe_view as they are, give SearchForTriangulation the oracle's matches."""
    import test_mapping as M
    kfs = M.make_keyframes(synthetic, M.oracle_features(oracle, synthetic), None, 2)
    p, lf, d, w = R.trained_tree(np.concatenate([k["descriptors"] for k in kfs]), k=6, L=4, seed=1)
    h = pkg.Vocabulary.from_arrays(6, 4, R.L1_NORM, R.TF_IDF, p, lf, d, w)
    raw = h.transform([k["descriptors"] for k in kfs], levelsup=2)
    for k, b in zip(kfs, raw):
        k["fv_node"], k["fv_offset"], k["fv_index"] = b["fv_node"], b["fv_offset"], b["fv_index"]
    cam4, mbf, _ = M.cam_of(synthetic)
    cam5 = np.float32([cam4[0], cam4[1], cam4[2], cam4[3], mbf]).astype(np.float64)
    sf, sg = M.tables()
    for kw in (dict(), dict(check_orientation=True)):
        want = oracle.search_for_triangulation(kfs[0], kfs[1], cam4, sf, sg, **kw)
        got = pkg.capi.search_for_triangulation(kfs[0], kfs[1], cam5, sf, sg, **kw)
        assert got[0] == want[0] and np.array_equal(got[1], want[1]), kw
        assert want[0] > 20


def test_search_by_bow_rejects_malformed_feature_vectors(pkg, drive, trained):
    ext, _, frames, counts = drive
    p, lf, d, w = trained
    h = pkg.Vocabulary.from_arrays(5, 3, R.L1_NORM, R.TF_IDF, p, lf, d, w)
    b = h.transform_orb(ext, counts[:2], levelsup=1)
    good = _view(frames[1], b[1])
    for bad_field in ("offset", "node"):
        bb = dict(b[0])
        if bad_field == "offset":  # up and down, with a sane last entry
            off = bb["fv_offset"].copy(); off[1], off[2] = off[2], off[1]; bb["fv_offset"] = off
        else:
            nodes = bb["fv_node"].copy(); nodes[0], nodes[1] = nodes[1], nodes[0]; bb["fv_node"] = nodes
        kf = _view(frames[0], bb, np.ones(len(frames[0]["keys"]), np.uint8))
        with pytest.raises(pkg.Tc2liError) as e:
            pkg.search_by_bow_batch([dict(keyframe=kf, frame=good, nn_ratio=0.7, check_orientation=True)], capacity=ext.capacity)
        assert e.value.code == -2


@pytest.fixture(scope="module")
def reference_scene(pkg, synthetic):
    """Four frames and their reference keyframes: 0.1 m behind every frame, own extractor, depth from the stereo match; the third keyframe
    with so few points that the search finds fewer than 15 matches."""
    xs = [0.0, 0.2, 0.4, 0.6]
    bf = np.float32(synthetic.BF); b = np.float32(bf / np.float32(synthetic.FX))
    fx, fy, cx, cy = [np.float32(v) for v in (synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY)]
    ext_kf, dev_kf, kfs, kcounts = _drive(pkg, synthetic, [x - 0.1 for x in xs], seed=8)
    _, kdepth, _ = pkg.stereo_match_batch(ext_kf, len(xs), float(bf), float(b))
    ext, dev, frames, counts = _drive(pkg, synthetic, xs, seed=8)
    keypoints = np.zeros((2 * len(xs), ext.capacity), pkg.capi.KEYPOINT_DTYPE)
    for f, fr in enumerate(frames):
        keypoints[2 * f, :len(fr["keys"])] = fr["keys"]
    u_right, _, _ = pkg.stereo_match_batch(ext, len(xs), float(bf), float(b))
    p, lf, d, w = R.trained_tree(np.concatenate([k["descriptors"] for k in kfs[:2]]), k=6, L=6, seed=3)
    voc_ref = R.Voc(6, 6, R.L1_NORM, R.TF_IDF, p, lf, d, w)
    h = pkg.Vocabulary.from_arrays(6, 6, R.L1_NORM, R.TF_IDF, p, lf, d, w)
    kbows = h.transform([k["descriptors"] for k in kfs], levelsup=4)
    rng = np.random.default_rng(4)
    refs = []
    for f, kf in enumerate(kfs):
        n = len(kf["keys"])
        z = kdepth[f, :n]
        hp = ((z > 0) & (rng.random(n) < 0.85)).astype(np.uint8)
        if f == 2:  # too few points: the search finds fewer than 15 matches
            hp[np.flatnonzero(hp)[10:]] = 0
        zz = np.where(z > 0, z, 1).astype(np.float32)
        Xw = np.stack([(kf["keys"]["x"] - cx) * zz / fx, (kf["keys"]["y"] - cy) * zz / fy, zz], 1).astype(np.float32)
        Xw[:, 0] += np.float32(xs[f] - 0.1)   # world = the first keyframe's camera frame, cameras along x
        last = np.array([0, 0, 0, 1, -xs[f] + 0.01, 0.004, -0.008], np.float32)
        refs.append(dict(keys=kf["keys"], descriptors=kf["descriptors"], has_point=hp, fv_node=kbows[f]["fv_node"],
                         fv_offset=kbows[f]["fv_offset"], fv_index=kbows[f]["fv_index"], Xw=Xw,
                         observed=(rng.random(n) < 0.9).astype(np.uint8), last_pose7=last))
    cam5 = np.float32([fx, fy, cx, cy, bf]).astype(np.float64)
    return dict(ext=ext, dev=dev, keep=(ext_kf, dev_kf), frames=frames, keypoints=keypoints, u_right=u_right, refs=refs, cam5=cam5, voc=h, voc_ref=voc_ref)


def _track_reference(pkg, sc, refs, with_bow=True):
    """the first len(refs) frames of the scene against `refs`"""
    F = len(refs)
    return pkg.capi.track_reference_keyframe_batch(sc["ext"], sc["voc"], sc["keypoints"][:2 * F], sc["u_right"][:F], refs, sc["cam5"], with_bow=with_bow)


def _check_track_reference(pkg, oracle, sc, refs, got):
    """The outputs of _track_reference(sc, refs) against 'restatement ComputeBoW -> SearchByBoW(0.7, true) -> oracle.pose_optimization ->
    discard' -> per frame the inliers, None below 15 matches."""
    poses, mp, nm, inl, nmap, braw = got
    ext, u_right, cam5 = sc["ext"], sc["u_right"], sc["cam5"]
    inv_sigma2 = ext.GetInverseScaleSigmaSquares()
    cap = ext.capacity
    results = []
    for f, r in enumerate(refs):
        fr = sc["frames"][f]
        n = len(fr["keys"])
        fb = R.transform(sc["voc_ref"], fr["descriptors"], 4)
        assert np.array_equal(braw["fv_node"][f * cap:f * cap + braw["n_nodes"][f]], fb["fv_node"])
        assert braw["bow_value"][f * cap:f * cap + braw["n_words"][f]].tobytes() == fb["bow_value"].tobytes()
        m, nmatch = R.search_by_bow(dict(angle=r["keys"]["angle"], descriptors=r["descriptors"], has_point=r["has_point"], fv_node=r["fv_node"],
                                         fv_offset=r["fv_offset"], fv_index=r["fv_index"]),
                                    dict(angle=fr["keys"]["angle"], descriptors=fr["descriptors"], **{k: fb[k] for k in ("fv_node", "fv_offset", "fv_index")}),
                                    0.7, True)
        assert nm[f] == nmatch, (f, nm[f], nmatch)
        assert np.all(mp[f, n:] == -1)
        if nmatch < 15:
            assert inl[f] == -1 and nmap[f] == 0 and np.all(mp[f] == -1)
            assert np.array_equal(poses[f], r["last_pose7"].astype(np.float64))
            results.append(None)
            continue
        ids = np.flatnonzero(m >= 0)
        edges6 = np.array([[e, 0, fr["keys"]["x"][i], fr["keys"]["y"][i], u_right[f, i], inv_sigma2[fr["keys"]["octave"][i]]]
                           for e, i in enumerate(ids)], np.float64)
        Xe = r["Xw"][m[ids]].astype(np.float64)
        pose, outl, ninl, _ = oracle.pose_optimization(r["last_pose7"].astype(np.float64), Xe, edges6, cam5)
        want = m.copy()
        want[ids[outl.astype(bool)]] = -1
        assert np.array_equal(mp[f, :n], want), f
        assert inl[f] == ninl
        assert nmap[f] == int(sum(r["observed"][want[i]] for i in np.flatnonzero(want >= 0)))
        assert np.allclose(poses[f], pose, rtol=1e-4, atol=1e-6), (poses[f], pose)
        results.append(ninl)
    return results


def test_track_reference_keyframe_batch(pkg, oracle, reference_scene):
    """The batch against 'restatement ComputeBoW -> SearchByBoW(0.7, true) -> oracle.pose_optimization -> discard', frames above and below
    15 matches in one batch."""
    sc = reference_scene
    got = _track_reference(pkg, sc, sc["refs"])
    results = _check_track_reference(pkg, oracle, sc, sc["refs"], got)
    assert results[2] is None and sum(x is not None and x > 50 for x in results) >= 2, (got[2], got[3])


# ---- the tables of a call: every one has its place in the call's block, whatever the call before left there -----------------------------
def _same_outputs(a, b, rows=None):
    """two results of _track_reference, `rows` of b; the bow arrays only where both have them"""
    for x, y in zip(a[:5], b[:5]):
        assert np.array_equal(x, y if rows is None else y[rows])
    if rows is None and len(a) > 5 and len(b) > 5:
        for k in a[5]:
            assert a[5][k].tobytes() == b[5][k].tobytes(), k


def test_track_reference_grows_shrinks_and_reuses_its_buffers(pkg, oracle, reference_scene):
    """Four frames (checked against the reference), the first alone, the four again, through the same per-thread buffers; the call without
    the bow output; and a reference keyframe without keypoints and without nodes between two ordinary ones."""
    sc = reference_scene
    refs = sc["refs"]
    got = _track_reference(pkg, sc, refs)
    _check_track_reference(pkg, oracle, sc, refs, got)
    _same_outputs(_track_reference(pkg, sc, refs[:1]), got, rows=[0])
    _same_outputs(_track_reference(pkg, sc, refs), got)
    _same_outputs(_track_reference(pkg, sc, refs, with_bow=False), got)
    none = dict(refs[1], keys=refs[1]["keys"][:0], descriptors=refs[1]["descriptors"][:0], has_point=refs[1]["has_point"][:0], Xw=refs[1]["Xw"][:0],
                observed=refs[1]["observed"][:0], fv_node=refs[1]["fv_node"][:0], fv_offset=np.zeros(1, np.int32), fv_index=refs[1]["fv_index"][:0])
    three = [refs[0], none, refs[2]]
    got3 = _track_reference(pkg, sc, three)
    results = _check_track_reference(pkg, oracle, sc, three, got3)
    assert results[1] is None and got3[2][1] == 0 and results[0] is not None
    for x, y in zip(got3[:5], got[:5]):
        assert np.array_equal(x[[0, 2]], y[[0, 2]])


def test_search_by_bow_with_an_empty_frame_between_two(pkg, drive, trained):
    ext, _, frames, counts = drive
    p, lf, d, w = trained
    h = pkg.Vocabulary.from_arrays(5, 3, R.L1_NORM, R.TF_IDF, p, lf, d, w)
    bows = h.transform_orb(ext, counts, levelsup=1)
    hp = [np.ones(len(fr["keys"]), np.uint8) for fr in frames]
    nothing = dict(keys=frames[0]["keys"][:0], descriptors=frames[0]["descriptors"][:0])
    no_bow = dict(fv_node=np.zeros(0, np.int32), fv_offset=np.zeros(1, np.int32), fv_index=np.zeros(0, np.int32))
    sides = [((frames[0], bows[0]), (frames[1], bows[1])), ((frames[2], bows[2]), (nothing, no_bow)), ((frames[1], bows[1]), (frames[3], bows[3]))]
    pairs = [dict(keyframe=_view(*kf, has_point=hp[k] if len(kf[0]["keys"]) else None), frame=_view(*fr), nn_ratio=0.7, check_orientation=True)
             for k, (kf, fr) in zip((0, 2, 1), sides)]
    match, nm = pkg.search_by_bow_batch(pairs, capacity=ext.capacity)
    for i, (k, (kf, fr)) in enumerate(zip((0, 2, 1), sides)):
        m, n = R.search_by_bow(_ref_view(*kf, has_point=hp[k]), _ref_view(*fr), 0.7, True)
        assert np.array_equal(match[i][:len(m)], m) and (match[i][len(m):] == -1).all() and nm[i] == n, i
    assert nm[1] == 0 and nm[0] > 20 and nm[2] > 20


def test_transform_with_a_frame_of_no_descriptors_between_two(pkg, drive, full_voc):
    _, _, frames, _ = drive
    ref, h = full_voc
    descs = [frames[0]["descriptors"], np.zeros((0, 32), np.uint8), frames[1]["descriptors"][:65]]
    for n in (3, 1, 3):   # and through the same buffers: three frames, one, three
        got = h.transform(descs[:n], levelsup=4)
        for f in range(n):
            _same(got[f], R.transform(ref, descs[f], 4), "frame %d of %d" % (f, n))
    assert len(got[1]["bow_word"]) == 0 and got[1]["fv_offset"].tolist() == [0]
