"""GPU tests of the MLPnP RANSAC stage: tc2li_mlpnp_ransac_batch against the restatement (tests/mlpnp_ref.py) and against the host entry by
the rule tests/mlpnp_cases.py states, in one batch of mixed problem sizes; then the relocalisation chain SearchByBoW -> MLPnP -> ladder."""
import numpy as np
import pytest

import bow_ref as B
import mlpnp_cases as K
import mlpnp_ref as ref
import reloc_ref as R

pytestmark = pytest.mark.gpu


def _run(pkg, problems, host, **kw):
    return pkg.mlpnp_ransac_batch(problems, K.LEVEL_SIGMA2, K.CAM5, params=pkg.mlpnp_params(), host=host, **kw)


def _device_equals_host(dev, host, p, n_kp, bound):
    for name in ("found", "no_more", "n_inliers", "iterations", "best_inliers"):
        assert int(dev[name][p]) == int(host[name][p]), (p, name)
    assert np.array_equal(dev["inlier"][p], host["inlier"][p]) and np.array_equal(dev["best_inlier"][p][:n_kp], host["best_inlier"][p][:n_kp]), p
    a, b = dev["Rt12"][p].reshape(3, 4), host["Rt12"][p].reshape(3, 4)
    d = K._rt_diff(a, b)
    assert d <= bound, (p, d, bound)
    return d


def _mixed_batch():
    rng = np.random.default_rng(77)
    problems = []
    for i in range(400):
        problems.append(K.easy(10000 + i, int(rng.integers(15, 301))))
    for i in range(88):
        problems.append(K.hard(20000 + i, int(rng.integers(15, 301))))
    for i in range(12):
        problems.append(K.make_problem(30000 + i, int(rng.integers(15, 200)), 0.15, 0.3, planar=True))
    for i in range(4):
        problems.append(K.easy(31000 + i, 6 + i))                                   # N below min_inliers
    for i in range(4):
        problems.append(K.make_problem(32000 + i, 10, 0.0, 0.1))                    # N equal to min_inliers
    for i in range(4):
        problems.append(K.make_problem(33000 + i, 50 + 20 * i, 0.15, 0.3, n_unmatched=200))   # matches skip most keypoints
    order = rng.permutation(len(problems))                                          # problems of different length share launches
    return [problems[k] for k in order]


def test_mixed_batch_against_restatement_and_host_entry(pkg):
    problems = _mixed_batch()
    assert len(problems) >= 512
    dev = _run(pkg, problems, host=False)
    host = _run(pkg, problems, host=True, capacity=dev["inlier"].shape[1])
    report, dh = K.new_report(), []
    solvers = []
    for p, pr in enumerate(problems):
        sv = K.solvers_for(pr)
        solvers.append(sv)
        res = K.compare_call(sv, pr["n_iterations"], pr["draws"], dev, p, report)
        if not res["left_out"]:
            dh.append(_device_equals_host(dev, host, p, len(pr["keys"]), res["bound"]))
    K.check_left_out(report)
    print("mixed batch of %d: s max %.3g, device-restatement max %.3g, device-host max %.3g, left out %d; found %d, no_more %d, both %d"
          % (len(problems), max(report["s"]), max(report["dist"]), max(dh), sum(report["left_out"]), int(dev["found"].sum()), int(dev["no_more"].sum()),
             int((dev["found"] & dev["no_more"]).sum())))
    assert dev["found"].sum() > 300 and (dev["no_more"] & ~dev["found"].astype(bool)).sum() > 0 and (dev["no_more"] & dev["found"]).sum() > 0
    # ---- a second and a third call on the same solvers, past max_iterations ----
    live = [p for p in range(len(problems)) if not report["left_out"][p]][:128]
    used = {p: 6 * int(dev["iterations"][p]) for p in live}
    state = {p: K.state_of(dev, p, problems[p]) for p in live}
    for call in (1, 2):
        batch = [dict(state[p], draws=problems[p]["draws"][used[p]:]) for p in live]
        got = _run(pkg, batch, host=False)
        goth = _run(pkg, batch, host=True, capacity=got["inlier"].shape[1])
        rep = K.new_report()
        for k, p in enumerate(live):
            before = solvers[p][0].iterations
            res = K.compare_call(solvers[p], problems[p]["n_iterations"], batch[k]["draws"], got, k, rep)
            if not res["left_out"]:
                _device_equals_host(got, goth, k, len(problems[p]["keys"]), res["bound"])
            used[p] += 6 * (solvers[p][0].iterations - before)
            state[p] = K.state_of(got, k, problems[p])
        K.check_left_out(rep)
        live = [p for k, p in enumerate(live) if not rep["left_out"][k]]


def test_invalid_arguments_before_any_launch(pkg):
    pr = K.easy(7000, 40)
    with pytest.raises(Exception, match="min_set"):
        pkg.mlpnp_ransac_batch([pr], K.LEVEL_SIGMA2, K.CAM5, params=pkg.mlpnp_params(min_set=5))
    with pytest.raises(Exception, match="draws"):
        _run(pkg, [dict(pr, draws=pr["draws"][:100])], host=False)
    bad = pr["match"].copy(); bad[np.nonzero(bad >= 0)[0][0]] = 40
    with pytest.raises(Exception, match="match"):
        _run(pkg, [dict(pr, match=bad)], host=False)


def test_relocalisation_chain(pkg, oracle, synthetic):
    """Frames and keyframes of one scene: SearchByBoW's matches go into the PnP stage, its pose7 and inlier into the ladder.  Every stage is
    checked against its restatement fed with the previous stage's device output.  One candidate carries another keyframe's geometry (its
    points in the wrong order): no pose explains half of its matches, so its solver runs out and the candidate is discarded."""
    from test_reloc_gpu import H, W, _cam4, _candidate_keyframe, _extract
    xs = [0.0, 0.2, 0.4, 0.6]
    ext_kf, _, kfs = _extract(pkg, synthetic, [x - 0.1 for x in xs], seed=8)
    ext, dev_imgs, frames = _extract(pkg, synthetic, xs, seed=8)
    sf = np.asarray(ext.GetScaleFactors(), np.float32)
    log_sf = float(np.log(np.float32(sf[1])))
    sigma2 = np.asarray(ext.GetScaleSigmaSquares(), np.float32)
    inv_sigma2 = ext.GetInverseScaleSigmaSquares()
    cam4 = _cam4(synthetic)
    cam5 = np.float32(list(cam4) + [np.float32(synthetic.BF)]).astype(np.float64)
    rng = np.random.default_rng(23)
    p, lf, d, w = B.trained_tree(np.concatenate([k["descriptors"] for k in kfs[:2]]), k=6, L=4, seed=3)
    voc = pkg.Vocabulary.from_arrays(6, 4, B.L1_NORM, B.TF_IDF, p, lf, d, w)
    nF = len(xs)
    bows = voc.transform([k["descriptors"] for k in kfs] + [f["descriptors"] for f in frames], levelsup=2)
    u_right = np.full((nF, ext.capacity), -1, np.float32)
    view = lambda a, b, hp=None: dict(keys=a["keys"], descriptors=a["descriptors"], fv_node=b["fv_node"], fv_offset=b["fv_offset"],
                                      fv_index=b["fv_index"], **({} if hp is None else dict(has_point=hp)))
    rview = lambda a, b, hp=None: dict(angle=a["keys"]["angle"], descriptors=a["descriptors"], fv_node=b["fv_node"], fv_offset=b["fv_offset"],
                                       fv_index=b["fv_index"], has_point=hp)
    cands, pairs = [], []
    for f, x in enumerate(xs):
        u_right[f, :len(frames[f]["keys"])] = frames[f]["u_right"]
        kf = _candidate_keyframe(synthetic, kfs[f], x - 0.1, sf, rng, spoil=False)
        kf["has_point"] = (kfs[f]["depth"] > 0).astype(np.uint8)
        cands.append((f, kf))
        pairs.append(dict(keyframe=view(kfs[f], bows[f], kf["has_point"]), frame=view(frames[f], bows[nF + f]), nn_ratio=0.75, check_orientation=True))
    wrong = dict(cands[0][1], Xw=cands[0][1]["Xw"][rng.permutation(len(cands[0][1]["Xw"]))].copy())
    cands.append((0, wrong))
    pairs.append(pairs[0])
    # ---- stage 1: SearchByBoW (Tracking.cc:3517) ----
    m, nm = pkg.search_by_bow_batch(pairs, capacity=ext.capacity)
    problems = []
    for i, (f, kf) in enumerate(cands):
        fr = frames[f]
        want, n = B.search_by_bow(rview(kfs[f], bows[f], kf["has_point"]), rview(fr, bows[nF + f]), 0.75, True)
        match = m[i, :len(fr["keys"])]
        assert np.array_equal(match, want) and nm[i] == n >= 15, (i, nm[i], n)
        problems.append(dict(keys=fr["keys"], match=match, Xw=kf["Xw"], draws=rng.integers(0, 2 ** 31, 6 * 400, dtype=np.uint32), n_iterations=5))
    # ---- stage 2: MLPnP RANSAC (Tracking.cc:3525-3552), repeated while a candidate neither has a pose nor is discarded ----
    pose7 = [None] * len(cands)
    inlier = [None] * len(cands)
    discarded = [False] * len(cands)
    solvers = [K.solvers_for(pr, level_sigma2=sigma2, cam4=cam4) for pr in problems]
    report = K.new_report()
    live = list(range(len(cands)))
    used = [0] * len(cands)
    state = list(problems)
    for _ in range(4):
        if not live:
            break
        batch = [dict(state[i], draws=problems[i]["draws"][used[i]:]) for i in live]
        got = pkg.mlpnp_ransac_batch(batch, sigma2, cam5, capacity=ext.capacity)
        nxt = []
        for k, i in enumerate(live):
            before = solvers[i][0].iterations
            res = K.compare_call(solvers[i], 5, batch[k]["draws"], got, k, report)
            assert not res["left_out"], i
            used[i] += 6 * (solvers[i][0].iterations - before)
            state[i] = K.state_of(got, k, problems[i])
            if got["no_more"][k]:
                discarded[i] = True
            if got["found"][k]:
                pose7[i], inlier[i] = got["pose7"][k].copy(), got["inlier"][k][:len(problems[i]["keys"])].copy()
            elif not got["no_more"][k]:
                nxt.append(i)
        live = nxt
    assert not live
    assert discarded[-1] and pose7[-1] is None, "the candidate with the wrong geometry must run out of iterations"
    # ---- stage 3: the ladder (Tracking.cc:3562-3631) on the PnP stage's pose and inliers ----
    hyps, refs = [], []
    for i, (f, kf) in enumerate(cands):
        if pose7[i] is None:
            continue
        hyps.append(dict(frame_index=f, pose7=pose7[i], match=problems[i]["match"], inlier=inlier[i], **{n: kf[n] for n in (
            "has_point", "Xw", "point_descriptors", "min_distance", "max_distance", "max_distance_raw", "angle")}))
        refs.append((f, kf))
    assert len(hyps) >= 3
    got = pkg.relocalization_refine_batch(ext, hyps, u_right, cam5)
    n_success = 0
    for h, (f, kf) in enumerate(refs):
        fr = frames[f]
        N = len(fr["keys"])
        frame = dict(keys=fr["keys"], descriptors=fr["descriptors"], u_right=u_right[f, :N], cols=W, rows=H)
        want = R.relocalization_refine(oracle, frame, kf, hyps[h]["pose7"], hyps[h]["match"], hyps[h]["inlier"], cam5, inv_sigma2, sf, log_sf,
                                       device_poses=got["poses7"][h])
        print("frame %d: PnP inliers %d, ladder status %d (want %d), nGood %d (%d)" % (f, int(hyps[h]["inlier"].sum()), got["status"][h], want["status"],
                                                                                      got["n_good"][h], want["n_good"]))
        assert got["status"][h] == want["status"] and got["n_good"][h] == want["n_good"], h
        assert np.array_equal(got["kf_keypoint_of_keypoint"][h, :N], want["assign"]) and np.array_equal(got["outlier"][h, :N], want["outlier"]), h
        n_success += bool(want["status"] & R.SUCCESS)
    assert n_success >= len(refs) - 1 and n_success >= 3, n_success


# ---- the buffers kept between calls -------------------------------------------------------------------------------------------------------
import functools


@functools.lru_cache(maxsize=None)
def _tiny(pkg):
    """-> (problems, bounds): 16 problems of the mixed batch's smallest size, 15 correspondences, every fourth a hard one, with the bound on
    device against host that the restatement's variants give (mlpnp_cases.compare_call, here on the host entry's result).  Problems 7 and 15 are too small to iterate and come with a
    state: the solver hands best_inlier, iterations and best_Tcw back as they came, so what went up must be what comes down."""
    problems = [(K.hard if i % 4 == 1 else K.easy)(41000 + i, 15) for i in range(16)]
    for i in (7, 15):
        pr = K.easy(41100 + i, 6)
        n = len(pr["keys"])
        problems[i] = dict(pr, iterations=2, best_inliers=3, best_Tcw=np.arange(12, dtype=np.float32), best_inlier=(np.arange(n) % 2).astype(np.uint8))
    bounds = []
    for pr in problems:
        if "best_inlier" in pr:
            bounds.append(1e-12)
            continue
        solvers = K.solvers_for(pr)
        res = K.compare_call(solvers, pr["n_iterations"], pr["draws"], _run(pkg, [pr], host=True), 0, K.new_report())
        assert not res["left_out"]
        bounds.append(res["bound"])
    return problems, bounds


def _equals_host(pkg, problems, bounds, what):
    dev = _run(pkg, problems, host=False)
    host = _run(pkg, problems, host=True, capacity=dev["inlier"].shape[1])
    for p, pr in enumerate(problems):
        _device_equals_host(dev, host, p, len(pr["keys"]), bounds[p])
        assert np.array_equal(dev["best_Tcw"][p], host["best_Tcw"][p]) and np.array_equal(dev["pose7"][p], host["pose7"][p]), (what, p)
        if "best_inlier" in pr:
            assert np.array_equal(dev["best_inlier"][p][:len(pr["keys"])], pr["best_inlier"]) and dev["iterations"][p] == pr["iterations"], (what, p)
    return dev


def _same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def test_device_reuses_its_buffer_across_batch_sizes(pkg):
    """8 problems, then 1 other, then the 8 again through the same buffer: nothing of an earlier call shows in a later one."""
    problems, bounds = _tiny(pkg)
    _equals_host(pkg, problems, bounds, "fill")                                      # whatever the tests before left, the buffer is larger than the calls below need
    first = _equals_host(pkg, problems[:8], bounds[:8], "8")
    assert first["found"].sum() >= 3 and first["no_more"][7] == 1
    _equals_host(pkg, problems[8:9], bounds[8:9], "1")
    _same(first, _equals_host(pkg, problems[:8], bounds[:8], "8 again"), "first against third call")


def test_device_empty_problem_inside_a_batch(pkg):
    """A problem without keypoints, points or draws between two ordinary ones: its tables are empty places in the concatenation, and its
    row of the inlier flags stays zero."""
    problems, bounds = _tiny(pkg)
    empty = dict(keys=np.zeros(0, K.KEYPOINT_DTYPE), match=np.zeros(0, np.int32), Xw=np.zeros((0, 3), np.float32), draws=np.zeros(0, np.uint32))
    dev = _equals_host(pkg, [problems[0], empty, problems[1]], [bounds[0], 1e-12, bounds[1]], "empty in the middle")
    assert dev["found"][1] == 0 and dev["no_more"][1] == 1 and not dev["inlier"][1].any() and not dev["best_inlier"][1].any()
    _equals_host(pkg, [empty, problems[0], empty], [1e-12, bounds[0], 1e-12], "empty at both ends")
    _equals_host(pkg, [empty], [1e-12], "empty alone")


def test_device_two_callers_at_once(pkg):
    """Two threads, four calls each on batches of four of their own: each gets its own results."""
    import two_callers
    problems, bounds = _tiny(pkg)
    index = [[[8 * t + (2 * s + i) % 8 for i in range(4)] for s in range(4)] for t in (0, 1)]
    batches = [[[problems[k] for k in b] for b in side] for side in index]
    got = two_callers.run(lambda b: _run(pkg, b, host=False), batches[0], batches[1])
    for t in (0, 1):
        for c in range(4):
            host = _run(pkg, batches[t][c], host=True, capacity=got[t][c]["inlier"].shape[1])
            for i, k in enumerate(index[t][c]):
                _device_equals_host(got[t][c], host, i, len(problems[k]["keys"]), bounds[k])
