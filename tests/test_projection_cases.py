"""The directed cases of projection_cases.py do what their names say -- checked with projection_ref (the plain restatement of
SF/src/ORBmatcher.cc:52-222, 1685-1896) and reloc_ref alone, no device -- and projection_ref agrees with the oracle wherever the two
restate the same lines: on every raw-query case, and on the random scene of matcher_scenario.make through SearchLocalPoints."""
import numpy as np
import pytest

import projection_cases as PC
import projection_local_cases as LC
import projection_ref as P
import reloc_ref as R

RAW = PC.raw_cases()


def wanted(case, mode, orientation):
    want = case["want"]
    return want.get((mode, orientation), want[(mode, False)])


def run_ref(oracle, case, mode, orientation):
    return P.search_queries(oracle, case["keys"], case["desc"], case["u_right"], case["occupied"], PC.W, PC.H, case["queries"], mode, PC.NN_RATIO, orientation)


@pytest.fixture(scope="module")
def raw_results(oracle):
    """projection_ref on every raw case, every mode it is meant for, with and without orientation: computed once."""
    return {(c["name"], m, o): run_ref(oracle, c, m, o) for c in RAW for m in c["modes"] for o in (False, True)}


def test_case_names_are_unique_and_lists_complete():
    names = [c["name"] for c in RAW]
    assert len(set(names)) == len(names)
    assert len([n for n in names if n.startswith("chain-")]) == len(PC.CHAIN_LENGTHS) * (len(PC.CHAIN_VARIANTS) + 1)


@pytest.mark.parametrize("case", RAW, ids=lambda c: c["name"])
def test_raw_case_shows_its_property(raw_results, case):
    """The reference gives what the case states by hand: the matches, mvpMapPoints and the count."""
    for mode in case["modes"]:
        for orientation in (False, True):
            n, match, point = raw_results[(case["name"], mode, orientation)]
            wn, wmatch, wpoint = wanted(case, mode, orientation)
            assert np.array_equal(match, wmatch), (mode, orientation, np.flatnonzero(match != wmatch)[:10])
            assert np.array_equal(point, wpoint) and n == wn, (mode, orientation, n, wn)


@pytest.mark.parametrize("L", PC.CHAIN_LENGTHS)
def test_chain_takes_L_distinct_keys_in_chain_order(raw_results, L):
    case = next(c for c in RAW if c["name"] == "chain-%d-plain" % L)
    order = PC.scan_order(case["keys"])
    for mode in (0, 1):
        n, match, point = raw_results[(case["name"], mode, False)]
        assert n == L and len(set(match.tolist())) == L and match.tolist() == order
        assert np.array_equal(point[match], np.arange(L))
    assert len(case["queries"]) == L      # M == L: the rounds form ends on its cap


def test_ratio_cases_are_accepted_or_rejected_as_listed(raw_results):
    verdict = {n: raw_results[("ratio-" + n, 1, False)][0] for n in ("40-50", "41-50", "36-45", "0-0", "10-10-one-level", "10-10-two-levels", "second-absent")}
    assert verdict == {"40-50": 1, "41-50": 0, "36-45": 1, "0-0": 1, "10-10-one-level": 0, "10-10-two-levels": 1, "second-absent": 1}
    assert raw_results[("ratio-second-claimed", 1, False)][0] == 2 and raw_results[("ratio-second-claimed-without-observations", 1, False)][0] == 1
    assert raw_results[("ratio-verdicts-flip-in-turn", 1, False)][1].tolist() == [1, 0, 2]
    for mode in (0, 1):
        assert raw_results[("th-high-100", mode, False)][0] == 1 and raw_results[("th-high-101", mode, False)][0] == 0


def test_duplicate_case_clears_the_keypoint(raw_results):
    """ORBmatcher.cc:1800 pushes the KEYPOINT index, :1886-1889 clear that keypoint and count down once per entry: whichever of the two
    entries of K is rejected, K ends without a point, and nmatches is the 32 matches less one."""
    for name in ("duplicate-plain", "duplicate-mirror"):
        for mode in (0, 1):
            n, match, point = raw_results[(name, mode, True)]
            K = len(point) - 1
            assert point[K] == -1 and n == 31 and match[K] == -1 and match[K + 1] == -1
            n, match, point = raw_results[(name, mode, False)]
            assert point[K] == K + 1 and n == 32 and match[K] == K and match[K + 1] == K


@pytest.mark.parametrize("case", RAW, ids=lambda c: c["name"])
def test_reference_equals_oracle_on_raw_cases(oracle, raw_results, case):
    """oracle.search_by_projection restates the same lines in C++: counts and matches agree on every raw case, the duplicate cases
    included (both clear by keypoint, ORBmatcher.cc:1873-1892)."""
    for mode in case["modes"]:
        for orientation in (False, True):
            n, match, _ = raw_results[(case["name"], mode, orientation)]
            on, omatch = oracle.search_by_projection(case["keys"], case["desc"], case["u_right"], case["occupied"], PC.W, PC.H, case["queries"], mode,
                                                     PC.NN_RATIO, orientation)
            assert on == n and np.array_equal(omatch, match), (mode, orientation)


# ---- keyframe items ---------------------------------------------------------------------------------------------------------------------
def kf_reference(oracle, item, cam4, th, orb_dist=100, check_orientation=False):
    frame = dict(keys=item["keys"], descriptors=item["descriptors"], held=item["held"], pose7=item["pose7"], cols=PC.W, rows=PC.H)
    want, n, _ = R.search_by_projection_keyframe(oracle, frame, item, cam4, PC.SF, PC.LOG_SF, th, orb_dist, check_orientation)
    return want, n


def ulps_between(a, b):
    ia, ib = int(np.float32(a).view(np.int32)), int(np.float32(b).view(np.int32))
    return abs(ia - ib)


def test_level_items_sit_on_the_boundaries(oracle):
    items, ratios, octaves, cam4, th = PC.level_items()
    levels = [R.predict_scale(r, np.float32(1), PC.LOG_SF, PC.N_LEVELS) for r in ratios]
    sides = 0
    for k in range(8):
        centre = PC.boundary_centre(k)
        assert ulps_between(centre, np.float32(1.2 ** k)) <= 4      # the float scale factor's power and float32(1.2^k): neighbours
        mine = levels[17 * k:17 * (k + 1)]
        for s, r, lv in zip(range(-8, 9), ratios[17 * k:], mine):
            assert ulps_between(r, centre) == abs(s) and ulps_between(r, np.float32(1.2 ** k)) <= 12
            assert lv in (k, min(k + 1, 7))
        assert mine == sorted(mine) and mine[0] == k and mine[-1] == min(k + 1, 7)
        sides += mine[0] != mine[-1]
    assert sides == 7       # on both sides of every 1.2^k below the clamp the levels differ
    assert levels[17 * 8:] == [0, 0, 7, 7, 7]
    # the match tells the level: the single keypoint is reached from exactly one of the two
    for it, lv, o in zip(items, levels, octaves):
        want, n = kf_reference(oracle, it, cam4, th)
        assert n == (1 if lv - 1 <= o <= lv + 1 else 0) and want[0] == (0 if n else -1)
    found = [kf_reference(oracle, it, cam4, th)[1] for it in items[:17 * 7]]
    assert 0 < sum(found) < len(found)


@pytest.mark.parametrize("L", [30, 600])
def test_keyframe_chain(oracle, L):
    item, assigned = PC.kf_chain_item(L)
    want, n = kf_reference(oracle, item, PC.CAM_CORNER, 40.0)
    assert n == L and np.array_equal(want, assigned)


def test_orb_dist_items(oracle):
    for orb_dist in (64, 100):
        at, above = PC.orb_dist_items(orb_dist)
        assert kf_reference(oracle, at, PC.CAM_CORNER, 10.0, orb_dist)[1] == 1 and kf_reference(oracle, above, PC.CAM_CORNER, 10.0, orb_dist)[1] == 0


@pytest.mark.parametrize("n", PC.STAGE_COUNTS)
def test_stage_item_holds_n_candidates(oracle, n):
    item, last = PC.stage_item(n)
    frame = dict(keys=item["keys"], descriptors=item["descriptors"], held=item["held"], pose7=item["pose7"], cols=PC.W, rows=PC.H)
    want, nm, info = R.search_by_projection_keyframe(oracle, frame, item, PC.CAM_CORNER, PC.SF, PC.LOG_SF, 10.0, 100, False)
    assert nm == 2 and want[last] == 0 and want[len(want) - 1] == 1
    # the candidates of point 0 after the static tests (level window, search window, not held): n, the last of them in scan order is `last`
    idx = oracle.features_in_area(item["keys"], PC.W, PC.H, 160.0, 120.0, float(np.float32(10.0) * PC.SF[2]), 1, 3)
    idx = [int(i) for i in idx if not item["held"][i]]
    assert len(idx) == n and idx[-1] == last and info["candidates"] == n + 1


def test_rotation_items(oracle):
    items = PC.rotation_items()
    assert len(items[3]["has_point"]) == 0 and len(items[3]["keys"]) == 4 and len(items[6]["keys"]) == 0 and len(items[6]["has_point"]) == 2
    removed = []
    for it in items:
        plain = kf_reference(oracle, it, PC.CAM_CORNER, 3.0, 100, False)
        turned = kf_reference(oracle, it, PC.CAM_CORNER, 3.0, 100, True)
        assert plain[1] == min(len(it["keys"]), len(it["has_point"]))
        removed.append(plain[1] - turned[1])
    assert removed == [0, 0, 1, 0, 9, 5, 0, 3, 0, 0, 2, 4, 1]


# ---- SearchLocalPoints ------------------------------------------------------------------------------------------------------------------
def test_search_local_points_equals_oracle_on_the_random_scene(oracle, synthetic):
    """projection_ref.search_local_points against oracle.track_local_map (isInFrustum, PredictScale, window and matching in C++) on the
    frame and the local points of matcher_scenario: the same local_of_keypoint and the same n_matches."""
    import matcher_scenario
    sc = matcher_scenario.make(oracle, synthetic, seed=1, nfeat=1000)
    pts = matcher_scenario.local_map_points(sc, oracle, np.random.default_rng(11), n_extra=200)
    n = len(sc["keys"])
    rng = np.random.default_rng(12)
    held = np.where(sc["occupied"] > 0, 1, np.where(rng.random(n) < 0.05, 2, 0)).astype(np.uint8)
    cam5 = np.float32(list(sc["cam4"]) + [sc["bf"]]).astype(np.float64)
    log_scale = PC.LOG_SF
    inv_sigma2 = (1.0 / (sc["scales"].astype(np.float32) ** 2)).astype(np.float32)
    frame = dict(keys=sc["keys"], descriptors=sc["desc"], u_right=sc["u_right"], held=held, cols=sc["cols"], rows=sc["rows"])
    for th, far, th_far in ((1.0, False, 0.0), (3.0, True, 40.0)):
        want = oracle.track_local_map(sc["keys"], sc["desc"], sc["u_right"], sc["cols"], sc["rows"], sc["scales"], inv_sigma2, log_scale, sc["pose_cur"], cam5,
                                      held, np.zeros((n, 3), np.float32), pts, th=th, far_points=far, th_far=th_far)
        lk, nm = P.search_local_points(oracle, frame, pts, sc["pose_cur"], cam5, sc["scales"], log_scale, th, far, th_far)
        assert nm == want[3] and nm > 200 and np.array_equal(lk, want[1])


@pytest.fixture(scope="module")
def local_case(oracle, synthetic):
    """One 640 x 240 stereo pair, 1000 features, extracted and matched by the oracle; the directed points on it and, per run, the
    reference's queries, frustum records and search result."""
    left, right = synthetic.stereo_pair(40, 640, 240)
    ol, orr = oracle.OrbOracle(nfeatures=1000), oracle.OrbOracle(nfeatures=1000)
    _, kl, dl = ol.extract(left)
    _, kr, dr = orr.extract(right)
    bf = np.float32(synthetic.BF)
    u_right, _, _ = oracle.stereo_match(ol, orr, kl, dl, kr, dr, float(bf), float(bf / np.float32(synthetic.FX)))
    cam = np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY, bf])
    scales = ol.tables()[0]
    log_scale = PC.LOG_SF
    frame = dict(keys=kl, descriptors=dl, u_right=u_right, held=np.zeros(len(kl), np.uint8), cols=640, rows=240)
    case = LC.build(frame, cam, scales)
    out = []
    for th, far, th_far in LC.runs(case):
        qs, views = P.local_queries(oracle, case["points"], PC.IDENTITY, cam, scales, log_scale, 640, 240, th, far, th_far)
        lk, nm = P.search_local_points(oracle, frame, case["points"], PC.IDENTITY, cam, scales, log_scale, th, far, th_far)
        out.append(dict(th=th, far=far, th_far=th_far, queries=qs, views=views, local_of_keypoint=lk, n_matches=nm))
    return dict(case=case, frame=frame, cam=cam, scales=scales, runs=out)


def test_local_points_land_on_the_side_they_name(oracle, local_case):
    case, frame, scales = local_case["case"], local_case["frame"], local_case["scales"]
    notes, points = case["notes"], case["points"]
    first, wide = local_case["runs"][0], local_case["runs"][1]
    matched = set(int(k) for k in first["local_of_keypoint"][first["local_of_keypoint"] >= 0])
    groups = [nt["group"] for nt in notes]
    assert groups.count("level") == 7 * len(LC.LEVEL_STEPS) and groups.count("ratio") >= 6
    levels = {}
    for k, nt in enumerate(notes):
        view, q = first["views"][k], first["queries"][k]
        assert (view is not None) == nt["valid"], nt          # every frustum case lands on the side it names
        assert bool(q["valid"]) == nt["valid"]
        if nt["group"] == "level":
            ratio = np.float32(points["max_distance_raw"][k] / view["dist"])
            assert ratio == nt["ratio"] and ulps_between(ratio, PC.boundary_centre(nt["k"])) == abs(nt["step"])
            assert view["level"] in (nt["k"], nt["k"] + 1)
            levels.setdefault(nt["k"], []).append(view["level"])
            # the keypoint's octave is in the window of one of the two levels: whether the point ends on its own keypoint tells which
            assert (first["local_of_keypoint"][nt["key"]] == k) == (view["level"] - 1 <= nt["octave"] <= view["level"]), nt
        elif nt["group"].startswith("cos-") and nt["valid"]:
            assert nt["view_cos"] is None or view["view_cos"] == nt["view_cos"]
            for run in (first, wide):
                th = np.float32(run["th"])
                r = np.float32(nt["radius_factor"]) if run["th"] == 1.0 else np.float32(np.float32(nt["radius_factor"]) * th)
                assert run["queries"][k]["radius"] == np.float32(r * scales[nt["level"]]), nt
            # the keypoint lies between the two windows: found with the factor 4.0 only
            assert (first["local_of_keypoint"][nt["key"]] == k) == (nt["radius_factor"] == 4.0), nt
        elif nt["group"].startswith("distance-") and nt["valid"]:
            assert view["dist"] in (points["min_distance"][k], points["max_distance"][k]) and first["local_of_keypoint"][nt["key"]] == k
        elif nt["group"] == "u-at-cols":
            assert view["u"] == np.float32(640)
        elif nt["group"] == "ratio":
            d = points["descriptor"][k]
            assert oracle.descriptor_distance(d, frame["descriptors"][nt["key"]]) == nt["best"]
            assert oracle.descriptor_distance(d, frame["descriptors"][nt["second"]]) == 50
            assert frame["keys"]["octave"][nt["key"]] == frame["keys"]["octave"][nt["second"]] == view["level"]
    assert all(min(v) == k and max(v) == k + 1 for k, v in levels.items()) and len(levels) == 7    # both sides of every 1.2^k
    kinds = {nt["best"]: [] for nt in notes if nt["group"] == "ratio"}
    for k, nt in enumerate(notes):
        if nt["group"] == "ratio":
            kinds[nt["best"]].append(k in matched)
    assert set(kinds) == {40, 41} and any(kinds[40]) and not all(kinds[41])
    # th == 3.0 multiplies every window; far points: the threshold on a point's own depth keeps it, one unit in the last place less drops it
    assert all(np.array_equal(run["queries"]["valid"], first["queries"]["valid"]) for run in local_case["runs"][:2])
    at, under = local_case["runs"][2], local_case["runs"][3]
    fp = case["far_point"]
    assert first["views"][fp]["depth"] == np.float32(at["th_far"]) and at["queries"][fp]["valid"] == 1 and under["queries"][fp]["valid"] == 0
    assert 0 < under["queries"]["valid"].sum() < first["queries"]["valid"].sum()


def test_local_points_reference_equals_oracle(oracle, local_case):
    """The same points through oracle.track_local_map: the oracle restates the same lines, the double constant of RadiusByViewingCos
    (ORBmatcher.cc:226) included."""
    frame, cam = local_case["frame"], local_case["cam"]
    scales = local_case["scales"]
    n = len(frame["keys"])
    inv_sigma2 = (1.0 / (scales.astype(np.float32) ** 2)).astype(np.float32)
    for run in local_case["runs"]:
        want = oracle.track_local_map(frame["keys"], frame["descriptors"], frame["u_right"], 640, 240, scales, inv_sigma2, PC.LOG_SF,
                                      PC.IDENTITY, cam.astype(np.float64), frame["held"], np.zeros((n, 3), np.float32), local_case["case"]["points"],
                                      th=run["th"], far_points=run["far"], th_far=run["th_far"])
        assert want[3] == run["n_matches"] and np.array_equal(want[1], run["local_of_keypoint"]), (run["th"], run["far"])
