"""Plain Python restatement of relocalisation's data-parallel stages -- the checker of tests/test_reloc*.py: DBoW2's scoring functions
(SF/Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311) with the reference's iterator walk, KeyFrameDatabase with real per-word lists
(SF/src/KeyFrameDatabase.cc:40-107) and DetectRelocalizationCandidates (:742-854), ORBmatcher::SearchByProjection(Frame&, KeyFrame*,
sAlreadyFound, th, ORBdist) (SF/src/ORBmatcher.cc:1898-2019) on top of the oracle's GetFeaturesInArea and DescriptorDistance, and the
refinement ladder of Tracking::Relocalization (SF/src/Tracking.cc:3562-3631) on top of the oracle's PoseOptimization.  Line by line, no
shortcuts: doubles are Python floats, float steps numpy float32 scalars."""
import bisect
import math

import numpy as np

L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)


# ---- TemplatedVocabulary::score ----------------------------------------------------------------------------------------------------
def _walk(v1, v2, term):
    """The loop every scoring function shares (e.g. ScoringObject.cpp:29-59): two map iterators, lower_bound on the map that lags.
    term(vi, wi) returns the addend or None (no addition)."""
    w1, x1 = [int(w) for w in v1[0]], [float(x) for x in v1[1]]
    w2, x2 = [int(w) for w in v2[0]], [float(x) for x in v2[1]]
    i = j = 0
    score = 0.0
    while i < len(w1) and j < len(w2):
        if w1[i] == w2[j]:
            t = term(x1[i], x2[j])
            if t is not None:
                score += t
            i += 1
            j += 1
        elif w1[i] < w2[j]:
            i = bisect.bisect_left(w1, w2[j])   # v1.lower_bound(v2_it->first)
        else:
            j = bisect.bisect_left(w2, w1[i])
    return score


def score_l1(v1, v2):
    """L1Scoring::score (:23-68)."""
    score = _walk(v1, v2, lambda vi, wi: math.fabs(vi - wi) - math.fabs(vi) - math.fabs(wi))
    return -score / 2.0


def score_l2(v1, v2):
    """L2Scoring::score (:73-120)."""
    score = _walk(v1, v2, lambda vi, wi: vi * wi)
    if score >= 1:
        return 1.0
    return 1.0 - math.sqrt(1.0 - score)


def score_chi_square(v1, v2):
    """ChiSquareScoring::score (:125-170)."""
    score = _walk(v1, v2, lambda vi, wi: vi * wi / (vi + wi) if vi + wi != 0.0 else None)
    return 2. * score


def score_bhattacharyya(v1, v2):
    """BhattacharyyaScoring::score (:226-266)."""
    return _walk(v1, v2, lambda vi, wi: math.sqrt(vi * wi))


def score_dot_product(v1, v2):
    """DotProductScoring::score (:271-311)."""
    return _walk(v1, v2, lambda vi, wi: vi * wi)


SCORE = {L1_NORM: score_l1, L2_NORM: score_l2, CHI_SQUARE: score_chi_square, BHATTACHARYYA: score_bhattacharyya, DOT_PRODUCT: score_dot_product}


def score(scoring, v1, v2):
    return SCORE[scoring](v1, v2)


# ---- KeyFrameDatabase --------------------------------------------------------------------------------------------------------------
class KeyFrame:
    """What the database reads of a KeyFrame: mnId, GetMap(), mBowVec, GetBestCovisibilityKeyFrames(10) (ids), and the three fields of
    KeyFrame.h:347-349.  mRelocScore is uninitialised in the reference; here it starts at 0.0f."""

    def __init__(self, kf_id, map_id, words, values):
        self.kf_id, self.map_id = int(kf_id), int(map_id)
        self.words = [int(w) for w in words]
        self.values = [float(v) for v in values]
        self.neighbours = []
        self.reloc_query = -1
        self.reloc_words = 0
        self.reloc_score = np.float32(0)
        self.sequence = -1

    @property
    def bow(self):
        return self.words, self.values


class KeyFrameDatabase:
    """mvInvertedFile as a list of KeyFrames per word (made on demand: the reference sizes it to the vocabulary, :44)."""

    def __init__(self, scoring=L1_NORM):
        self.scoring = scoring
        self.inverted = {}
        self.live = {}        # kf_id -> KeyFrame, for the neighbour ids and erase(kf_id)
        self.next_sequence = 0
        self.next_query = 0

    def add(self, kf_id, map_id, words, values):
        """:48-54"""
        assert kf_id not in self.live
        kf = KeyFrame(kf_id, map_id, words, values)
        kf.sequence = self.next_sequence
        self.next_sequence += 1
        for w in kf.words:
            self.inverted.setdefault(w, []).append(kf)
        self.live[kf.kf_id] = kf
        return kf

    def erase(self, kf_id):
        """:56-75"""
        kf = self.live.pop(kf_id, None)
        if kf is None:
            return
        for w in kf.words:
            lst = self.inverted[w]
            for pos, other in enumerate(lst):
                if other is kf:
                    del lst[pos]
                    break

    def clear(self):
        """:77-81"""
        self.inverted = {}
        self.live = {}

    def clear_map(self, map_id):
        """:83-107"""
        for lst in self.inverted.values():
            lst[:] = [kf for kf in lst if kf.map_id != map_id]
        self.live = {k: kf for k, kf in self.live.items() if kf.map_id != map_id}

    def set_covisibility(self, kf_id, ids):
        self.live[kf_id].neighbours = [int(i) for i in ids]

    def sharing_words(self, frame_id, words):
        """:744-766 -> lKFsSharingWords; sets mnRelocQuery / mnRelocWords."""
        sharing = []
        for w in words:
            for kf in self.inverted.get(int(w), []):
                if kf.reloc_query != frame_id:
                    kf.reloc_words = 0
                    kf.reloc_query = frame_id
                    sharing.append(kf)
                kf.reloc_words += 1
        return sharing

    def detect_relocalization_candidates(self, map_id, words, values):
        """:742-854 -> (candidate kf_ids, scored list of (kf_id, words, si, accScore, best kf_id) in lScoreAndMatch order)."""
        self.next_query += 1
        frame_id = self.next_query   # F->mnId: a new frame per query
        sharing = self.sharing_words(frame_id, words)
        if not sharing:
            return [], []
        max_common = 0
        for kf in sharing:
            if kf.reloc_words > max_common:
                max_common = kf.reloc_words
        min_common = int(np.float32(max_common) * np.float32(0.8))
        score_and_match = []
        for kf in sharing:
            if kf.reloc_words > min_common:
                si = np.float32(score(self.scoring, (words, values), kf.bow))
                kf.reloc_score = si
                score_and_match.append((si, kf))
        if not score_and_match:
            return [], []
        acc_and_match = []
        best_acc = np.float32(0)
        scored = []
        for si, kf in score_and_match:
            best_score = si
            acc = si
            best = kf
            for nid in kf.neighbours:
                kf2 = self.live.get(nid)
                if kf2 is None or kf2.reloc_query != frame_id:
                    continue
                acc = np.float32(acc + kf2.reloc_score)
                if kf2.reloc_score > best_score:
                    best = kf2
                    best_score = kf2.reloc_score
            acc_and_match.append((acc, best))
            scored.append((kf.kf_id, kf.reloc_words, si, acc, best.kf_id))
            if acc > best_acc:
                best_acc = acc
        min_score = np.float32(np.float32(0.75) * best_acc)
        added = set()
        out = []
        for acc, kf in acc_and_match:
            if acc > min_score:
                if kf.map_id != map_id:
                    continue
                if kf.kf_id not in added:
                    out.append(kf.kf_id)
                    added.add(kf.kf_id)
        return out, scored


def order_by_key(db, words):
    """The order the device design rests on: live keyframes that share a word with the frame, by (smallest shared word, sequence)."""
    ws = set(int(w) for w in words)
    keyed = []
    for kf in db.live.values():
        common = [w for w in kf.words if w in ws]
        if common:
            keyed.append((min(common), kf.sequence, kf.kf_id))
    return [k[2] for k in sorted(keyed)]


# ---- test data ----------------------------------------------------------------------------------------------------------------------
def random_bow(rng, n_voc_words, n, base=None, keep=1.0):
    """A BowVector of about n words: a fraction `keep` of `base` (the words of a place) plus random ones, values positive with L1 norm 1."""
    words = set()
    if base is not None:
        words.update(int(w) for w in base[rng.random(len(base)) < keep])
    while len(words) < n:
        words.update(int(w) for w in rng.integers(0, n_voc_words, n - len(words)))
    words = np.array(sorted(words), np.int32)
    values = rng.uniform(0.1, 1.0, len(words))
    values = values / values.sum()
    return words, values


# ---- ORBmatcher::SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) ----------------------------------------------------------
F32 = np.float32
_libm = None


def logf(x):
    """The C library's logf: what log(float) of MapPoint::PredictScale (SF/src/MapPoint.cc:548) calls."""
    global _libm
    if _libm is None:
        import ctypes
        import ctypes.util
        _libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
        _libm.logf.restype = ctypes.c_float
        _libm.logf.argtypes = [ctypes.c_float]
    return F32(_libm.logf(float(x)))


def _cross(a, b):
    return [F32(a[1] * b[2] - a[2] * b[1]), F32(a[2] * b[0] - a[0] * b[2]), F32(a[0] * b[1] - a[1] * b[0])]


def quat_rotate(q, v):
    """Eigen::Quaternionf::_transformVector: uv = q.vec x v; uv += uv; v + q.w * uv + q.vec x uv (q = x y z w)."""
    uv = _cross(q[:3], v)
    uv = [F32(c + c) for c in uv]
    c2 = _cross(q[:3], uv)
    return [F32(F32(v[k] + F32(q[3] * uv[k])) + c2[k]) for k in range(3)]


def predict_scale(max_distance_raw, dist, log_scale_factor, n_levels):
    """MapPoint::PredictScale(currentDist, Frame*) (SF/src/MapPoint.cc:540-555)."""
    ratio = F32(F32(max_distance_raw) / F32(dist))
    n = int(math.ceil(F32(logf(ratio) / F32(log_scale_factor))))
    return 0 if n < 0 else (n_levels - 1 if n >= n_levels else n)


def search_by_projection_keyframe(oracle, frame, kf, cam4, scale_factors, log_scale_factor, th, orb_dist, check_orientation):
    """SF/src/ORBmatcher.cc:1898-2019 with the frame's image bounds 0 .. cols, 0 .. rows (what oracle.features_in_area's grid covers).
    frame: keys, descriptors, held, pose7 (float32), cols, rows; kf: has_point, found, Xw, point_descriptors, min_distance, max_distance,
    max_distance_raw, angle -> (kf_keypoint_of_keypoint [N] for the new matches, nmatches, how many points every gate rejected; under
    "candidates" the keypoints in the points' windows that the frame did not hold on entry: what a candidate pool has to take)."""
    keys = frame["keys"]
    N = len(keys)
    assigned = np.full(N, -1, np.int32)
    held = np.asarray(frame["held"]).astype(bool).copy()
    held_on_entry = held.copy()
    q = [F32(x) for x in frame["pose7"]]
    fx, fy, cx, cy = [F32(x) for x in cam4]
    min_x, max_x, min_y, max_y = F32(0), F32(frame["cols"]), F32(0), F32(frame["rows"])
    Ow = quat_rotate([F32(-q[0]), F32(-q[1]), F32(-q[2]), q[3]], [F32(q[4] * F32(-1)), F32(q[5] * F32(-1)), F32(q[6] * F32(-1))])
    rot_hist = [[] for _ in range(30)]
    nmatches = 0
    rejected = dict(bounds=0, distance=0, orb_dist=0, histogram=0, candidates=0)
    for i in range(len(kf["has_point"])):
        if not kf["has_point"][i] or kf["found"][i]:
            continue
        X = [F32(x) for x in kf["Xw"][i]]
        pc = quat_rotate(q, X)
        pc = [F32(pc[k] + q[4 + k]) for k in range(3)]
        u = F32(F32(F32(fx * pc[0]) / pc[2]) + cx)
        v = F32(F32(F32(fy * pc[1]) / pc[2]) + cy)
        if u < min_x or u > max_x or v < min_y or v > max_y:
            rejected["bounds"] += 1
            continue
        po = [F32(X[k] - Ow[k]) for k in range(3)]
        dist = F32(np.sqrt(F32(F32(F32(po[0] * po[0]) + F32(po[1] * po[1])) + F32(po[2] * po[2]))))
        if dist < F32(kf["min_distance"][i]) or dist > F32(kf["max_distance"][i]):
            rejected["distance"] += 1
            continue
        level = predict_scale(kf["max_distance_raw"][i], dist, log_scale_factor, len(scale_factors))
        radius = F32(F32(th) * F32(scale_factors[level]))
        idx = oracle.features_in_area(keys, frame["cols"], frame["rows"], float(u), float(v), float(radius), level - 1, level + 1)
        if len(idx) == 0:
            continue
        rejected["candidates"] += int((~held_on_entry[np.asarray(idx, np.int64)]).sum())
        best_dist, best_idx = 256, -1
        for i2 in idx:
            if held[i2]:
                continue
            d = oracle.descriptor_distance(kf["point_descriptors"][i], frame["descriptors"][i2])
            if d < best_dist:
                best_dist, best_idx = d, int(i2)
        if best_dist <= orb_dist:
            held[best_idx] = True
            assigned[best_idx] = i
            nmatches += 1
            if check_orientation:
                import bow_ref
                rot_hist[bow_ref.rot_bin(kf["angle"][i], keys["angle"][best_idx])].append(best_idx)
        elif best_idx >= 0:
            rejected["orb_dist"] += 1
    if check_orientation:
        import bow_ref
        inds = bow_ref.compute_three_maxima([len(h) for h in rot_hist])
        for b in range(30):
            if b in inds:
                continue
            for j in rot_hist[b]:
                assigned[j] = -1
                nmatches -= 1
                rejected["histogram"] += 1
    return assigned, nmatches, rejected


# ---- the refinement ladder of Tracking::Relocalization (SF/src/Tracking.cc:3562-3631) ------------------------------------------------------
OPT1, REJECTED, SEARCH1, OPT2, SEARCH2, OPT3, SUCCESS = 1, 2, 4, 8, 16, 32, 64


def relocalization_refine(oracle, frame, kf, pose7, match, inlier, cam5, inv_sigma2, scale_factors, log_scale_factor, device_poses=None):
    """One hypothesis.  frame: keys, descriptors, u_right, cols, rows; kf: the candidate as search_by_projection_keyframe takes it (found is
    made here); match / inlier per frame keypoint.  device_poses [3][7]: when given, every stage after a PoseOptimization goes on from the
    device's pose of that stage instead of the oracle's (the searches then see the device's float pose exactly).
    -> dict(status, n_good, n_additional [2], poses [3][7] (the oracle's), outliers [3] (per keypoint, None for a stage that did not run),
    searches [2] ((assignment, nmatches, held, found, pose, window candidates) of the search alone, None when it did not run), assign,
    outlier)."""
    keys = frame["keys"]
    N = len(keys)
    cam4 = [cam5[0], cam5[1], cam5[2], cam5[3]]
    assign = np.where(np.asarray(inlier[:N]).astype(bool), np.asarray(match[:N], np.int32), -1).astype(np.int32)
    found = np.zeros(len(kf["has_point"]), np.uint8)
    found[assign[assign >= 0]] = 1                      # sFound
    out = dict(status=0, n_good=0, n_additional=[0, 0], poses=np.zeros((3, 7)), outliers=[None] * 3, searches=[None] * 2, outlier=np.zeros(N, np.uint8))
    pose = np.asarray(pose7, np.float32)

    def optimise(stage):
        nonlocal pose
        ids = np.flatnonzero(assign >= 0)
        edges6 = np.array([[e, 0, keys["x"][i], keys["y"][i], frame["u_right"][i], inv_sigma2[keys["octave"][i]]] for e, i in enumerate(ids)],
                          np.float64).reshape(-1, 6)
        Xe = np.asarray(kf["Xw"], np.float32)[assign[ids]].astype(np.float64).reshape(-1, 3)
        new_pose, outl, n_good, _ = oracle.pose_optimization(pose.astype(np.float64), Xe, edges6, cam5)
        flags = np.zeros(N, np.uint8)
        flags[ids] = outl
        out["poses"][stage] = new_pose
        out["outliers"][stage] = flags
        out["outlier"] = flags
        out["status"] |= (OPT1, OPT2, OPT3)[stage]
        pose = np.asarray(device_poses[stage] if device_poses is not None else new_pose, np.float64).astype(np.float32)   # Frame::SetPose
        return n_good, flags

    def search(th, orb_dist, which):
        fr = dict(keys=keys, descriptors=frame["descriptors"], held=(assign >= 0).astype(np.uint8), pose7=pose, cols=frame["cols"], rows=frame["rows"])
        new, n, rej = search_by_projection_keyframe(oracle, fr, dict(kf, found=found), cam4, scale_factors, log_scale_factor, th, orb_dist, True)
        out["searches"][which] = (new.copy(), n, fr["held"].copy(), found.copy(), pose.copy(), rej["candidates"])
        out["n_additional"][which] = n
        out["status"] |= (SEARCH1, SEARCH2)[which]
        assign[new >= 0] = new[new >= 0]
        return n

    n_good, flags = optimise(0)
    out["n_good"] = n_good
    if n_good < 10:
        out["status"] |= REJECTED
        out["assign"] = assign
        return out
    assign[flags.astype(bool)] = -1
    if n_good < 50:
        nadd = search(10, 100, 0)
        if nadd + n_good >= 50:
            n_good, flags = optimise(1)
            out["n_good"] = n_good
            if 30 < n_good < 50:
                found[:] = 0
                found[assign[assign >= 0]] = 1
                nadd = search(3, 64, 1)
                if n_good + nadd >= 50:
                    n_good, flags = optimise(2)
                    out["n_good"] = n_good
                    assign[flags.astype(bool)] = -1
    if n_good >= 50:
        out["status"] |= SUCCESS
    out["assign"] = assign
    return out
