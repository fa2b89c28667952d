"""Plain Python restatement of the ORB vocabulary (DBoW2's TemplatedVocabulary<FORB>, SF/Thirdparty/DBoW2/DBoW2/) and of
ORBmatcher::SearchByBoW(KeyFrame*, Frame&) (SF/src/ORBmatcher.cc:232-434) -- the checker of tests/test_bow*.py.  Line by line, no
shortcuts: map / set order is restated with sorted dicts, float32 arithmetic with numpy scalars."""
import math

import numpy as np

TF_IDF, TF, IDF, BINARY = 0, 1, 2, 3
L1_NORM, L2_NORM, CHI_SQUARE, KL, BHATTACHARYYA, DOT_PRODUCT = range(6)
TH_LOW, HISTO_LENGTH = 50, 30

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def hamming(a, b):
    """FORB::distance of a [32] with every row of b [n, 32]."""
    return _POP[np.bitwise_xor(np.asarray(b, np.uint8).reshape(-1, 32), np.asarray(a, np.uint8).reshape(1, 32))].sum(axis=1)


class Voc:
    """The content of a vocabulary: nodes 1 .. n in file order (parent, isLeaf flag, descriptor, weight); node 0 is the root."""

    def __init__(self, k, L, scoring, weighting, parent, is_leaf, desc, weight):
        n = len(parent)
        self.k, self.L, self.scoring, self.weighting = k, L, scoring, weighting
        self.file_parent = np.asarray(parent, np.int32)
        self.file_leaf = np.asarray(is_leaf, np.int32)
        self.parent = np.concatenate([[-1], self.file_parent]).astype(np.int32)
        self.desc = np.concatenate([np.zeros((1, 32), np.uint8), np.asarray(desc, np.uint8).reshape(n, 32)])
        self.weight = np.concatenate([[0.0], np.asarray(weight, np.float64)])
        self.children = [[] for _ in range(n + 1)]
        self.word = np.full(n + 1, -1, np.int32)
        nw = 0
        for i in range(n):
            self.children[int(parent[i])].append(i + 1)
            if is_leaf[i] > 0:
                self.word[i + 1] = nw
                nw += 1
        self.n_words = nw
        self.children = [np.asarray(c, np.int64) for c in self.children]


def write_text(path, voc, newline="\n", sep=" ", weights_text=None):
    """TemplatedVocabulary::saveToTextFile (TemplatedVocabulary.h:1441-1461): the header with its double space, per node
    "parent isLeaf d0 .. d31  weight" with the weight at 6 significant digits (ostream's default), endl after every line."""
    lines = ["%d%s%d%s%s%d%s%d" % (voc.k, sep, voc.L, sep, sep, voc.scoring, sep, voc.weighting)]
    for i in range(len(voc.file_parent)):
        w = weights_text[i] if weights_text is not None else "%g" % voc.weight[i + 1]
        lines.append(sep.join([str(int(voc.file_parent[i])), "1" if voc.file_leaf[i] > 0 else "0"] + [str(int(b)) for b in voc.desc[i + 1]])
                     + sep + sep + w)
    with open(path, "w", newline="") as f:
        f.write(newline.join(lines) + newline)


def read_weight_6(w):
    """The double a text round trip gives: 6 significant digits."""
    return float("%g" % w)


def transform_one(voc, d, levelsup):
    """TemplatedVocabulary::transform(feature, word_id, weight, &nid, levelsup) (:1230-1271); the leaf itself when it lies above
    nid_level (the reference leaves nid unset there)."""
    nid_level = voc.L - levelsup
    nid = 0 if nid_level <= 0 else None
    final, level = 0, 0
    while True:
        level += 1
        ch = voc.children[final]
        dist = hamming(d, voc.desc[ch])
        final = int(ch[int(np.argmin(dist))])  # argmin: the first minimum (strict < in child order)
        if level == nid_level:
            nid = final
        if len(voc.children[final]) == 0:
            break
    return int(voc.word[final]), float(voc.weight[final]), (final if nid is None else nid)


def transform(voc, descs, levelsup=4):
    """TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (:1139-1206) ->
    dict(word, node [n] (-1 stopped), bow_word, bow_value, fv_node, fv_offset, fv_index)."""
    descs = np.asarray(descs, np.uint8).reshape(-1, 32)
    n = len(descs)
    word, node = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    bow, fv = {}, {}
    if voc.n_words > 0:
        for i in range(n):
            wid, w, nid = transform_one(voc, descs[i], levelsup)
            if w > 0:
                word[i], node[i] = wid, nid
                if voc.weighting in (TF, TF_IDF):
                    bow[wid] = bow[wid] + w if wid in bow else w   # BowVector::addWeight
                elif wid not in bow:
                    bow[wid] = w                                    # addIfNotExist
                fv.setdefault(nid, []).append(i)
    words = sorted(bow)
    vals = [bow[w] for w in words]
    must = voc.scoring != DOT_PRODUCT
    if voc.weighting in (TF, TF_IDF) and vals and not must:
        nd = float(len(vals))
        vals = [v / nd for v in vals]
    if must:  # BowVector::normalize
        norm = 0.0
        if voc.scoring == L2_NORM:
            for v in vals:
                norm += v * v
            norm = math.sqrt(norm)
        else:
            for v in vals:
                norm += math.fabs(v)
        if norm > 0.0:
            vals = [v / norm for v in vals]
    nodes = sorted(fv)
    off = np.concatenate([[0], np.cumsum([len(fv[k]) for k in nodes])]).astype(np.int32)
    idx = np.asarray([i for k in nodes for i in fv[k]], np.int32)
    return dict(word=word, node=node, bow_word=np.asarray(words, np.int32), bow_value=np.asarray(vals, np.float64),
                fv_node=np.asarray(nodes, np.int32), fv_offset=off, fv_index=idx)


def compute_three_maxima(hist):
    """ORBmatcher::ComputeThreeMaxima (:2021-2062) over the bin sizes."""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(hist):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if max2 < np.float32(0.1) * np.float32(max1):
        ind2 = ind3 = -1
    elif max3 < np.float32(0.1) * np.float32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def rot_bin(kf_angle, f_angle):
    rot = np.float32(kf_angle) - np.float32(f_angle)
    if rot < 0.0:
        rot = np.float32(rot + np.float32(360.0))
    x = float(np.float32(rot * np.float32(np.float32(1.0) / np.float32(HISTO_LENGTH))))
    b = int(math.floor(x + 0.5))  # roundf of x >= 0 (exact in double)
    return 0 if b == HISTO_LENGTH else b


def search_by_bow(kf, fr, nn_ratio=0.7, check_orientation=True):
    """ORBmatcher::SearchByBoW(KeyFrame*, Frame&) with F.Nleft == -1.  kf: angle, descriptors, has_point, fv_node / fv_offset /
    fv_index; fr: angle, descriptors, fv_*.  -> (kf_keypoint_of_keypoint [F.N], nmatches)."""
    N = len(fr["angle"])
    match = np.full(N, -1, np.int32)
    nmatches = 0
    hist = [[] for _ in range(HISTO_LENGTH)]
    ratio = np.float32(nn_ratio)
    a = b = 0
    while a < len(kf["fv_node"]) and b < len(fr["fv_node"]):
        if kf["fv_node"][a] == fr["fv_node"][b]:
            ik = kf["fv_index"][kf["fv_offset"][a]:kf["fv_offset"][a + 1]]
            jf = fr["fv_index"][fr["fv_offset"][b]:fr["fv_offset"][b + 1]]
            for kfi in ik:
                if not kf["has_point"][kfi]:
                    continue
                best1, best_idx, best2 = 256, -1, 256
                for fi in jf:
                    if match[fi] >= 0:
                        continue
                    dist = int(hamming(kf["descriptors"][kfi], fr["descriptors"][fi])[0])
                    if dist < best1:
                        best2, best1, best_idx = best1, dist, fi
                    elif dist < best2:
                        best2 = dist
                if best1 <= TH_LOW and np.float32(best1) < ratio * np.float32(best2):
                    match[best_idx] = kfi
                    if check_orientation:
                        hist[rot_bin(kf["angle"][kfi], fr["angle"][best_idx])].append(best_idx)
                    nmatches += 1
            a += 1
            b += 1
        elif kf["fv_node"][a] < fr["fv_node"][b]:
            a += 1
        else:
            b += 1
    if check_orientation:
        inds = compute_three_maxima([len(h) for h in hist])
        for i in range(HISTO_LENGTH):
            if i in inds:
                continue
            for j in hist[i]:
                match[j] = -1
                nmatches -= 1
    return match, nmatches


# ---- vocabulary builders -----------------------------------------------------------------------------------------------------------
def random_tree(k=10, L=6, seed=0, flips=6, stop_frac=0.02):
    """A full k-ary tree of depth L in breadth-first file order: every child flips `flips` random bits of its parent's descriptor;
    word weights (idf-like) in (0, 4], a fraction of them 0 (stopped)."""
    rng = np.random.default_rng(seed)
    parents, leaves, descs = [], [], []
    level_desc = rng.integers(0, 256, (1, 32), dtype=np.uint8)
    level_ids = np.zeros(1, np.int64)
    next_id = 1
    for lev in range(1, L + 1):
        m = len(level_ids) * k
        par = np.repeat(level_ids, k)
        d = np.repeat(level_desc, k, axis=0)
        bits = rng.integers(0, 256, (m, flips))
        rows = np.repeat(np.arange(m), flips)
        np.bitwise_xor.at(d, (rows, (bits // 8).ravel()), (1 << (bits % 8)).astype(np.uint8).ravel())
        parents.append(par); descs.append(d); leaves.append(np.full(m, 1 if lev == L else 0, np.int32))
        level_ids = np.arange(next_id, next_id + m)
        level_desc = d
        next_id += m
    parent = np.concatenate(parents).astype(np.int32)
    is_leaf = np.concatenate(leaves)
    w = np.where(is_leaf > 0, rng.uniform(0.05, 4.0, len(parent)), 0.0)
    w[(is_leaf > 0) & (rng.random(len(parent)) < stop_frac)] = 0.0
    return parent, is_leaf, np.concatenate(descs), w


def mean_value(descs):
    """FORB::meanValue: the majority bit of every position (ties -> 1 when the count reaches half, rounded up)."""
    bits = np.unpackbits(np.asarray(descs, np.uint8), axis=1)
    n = len(descs)
    return np.packbits((bits.sum(axis=0) >= (n + 1) // 2).astype(np.uint8))


def trained_tree(descs, k=5, L=3, seed=0, iters=3):
    """A small vocabulary "trained" from descriptors: random seeds and majority-bit means per node (HKmeansStep-like), depth-first
    node numbering, idf weights log(N / n_i) of the leaves."""
    rng = np.random.default_rng(seed)
    descs = np.asarray(descs, np.uint8).reshape(-1, 32)
    parent, leaf, dd, members = [], [], [], []

    def grow(pid, idx, level):
        if len(idx) == 0:
            return
        kk = min(k, len(idx))
        centers = descs[rng.choice(idx, kk, replace=False)]
        for _ in range(iters):
            assign = np.array([int(np.argmin(hamming(descs[i], centers))) for i in idx])
            centers = np.array([mean_value(descs[idx[assign == c]]) if (assign == c).any() else centers[c] for c in range(kk)])
        assign = np.array([int(np.argmin(hamming(descs[i], centers))) for i in idx])
        ids = []
        for c in range(kk):
            parent.append(pid); leaf.append(1 if level == L else 0); dd.append(centers[c]); members.append(idx[assign == c])
            ids.append(len(parent))
        if level < L:
            for c in range(kk):
                if len(members[ids[c] - 1]) == 0:
                    leaf[ids[c] - 1] = 1
                else:
                    grow(ids[c], members[ids[c] - 1], level + 1)
                    if not any(p == ids[c] for p in parent):
                        leaf[ids[c] - 1] = 1

    grow(0, np.arange(len(descs)), 1)
    parent = np.asarray(parent, np.int32)
    leaf = np.asarray(leaf, np.int32)
    n = len(descs)
    w = np.array([math.log(n / max(len(m), 1)) if lf else 0.0 for lf, m in zip(leaf, members)])
    return parent, leaf, np.asarray(dd, np.uint8), w
