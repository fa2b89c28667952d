"""Generators for the tests of UpdateLocalMap over many sequences (tc2li_local_map_update_batch and its host twin): graphs as dicts of
flat arrays (what LocalMap.set_graph and oracle.update_local_map take), frames on them, and the list of cases both test files run.  The
expected lists always come from the oracle; this file only says which sizes the directed cases must reach."""
import numpy as np


def _csr(lists):
    off = np.concatenate([[0], np.cumsum([len(l) for l in lists])]).astype(np.int32)
    val = np.concatenate([np.asarray(l, np.int32) for l in lists]) if off[-1] else np.zeros(0, np.int32)
    return off, val.astype(np.int32)


def _graph(kf_bad, point_bad, covis, children, parent, prev_kf, matches, obs):
    co, cv = _csr(covis); ho, hv = _csr(children); mo, mv = _csr(matches); oo, ov = _csr(obs)
    return dict(kf_bad=np.asarray(kf_bad, np.uint8), covis_off=co, covis=cv, child_off=ho, children=hv, parent=np.asarray(parent, np.int32),
                prev_kf=np.asarray(prev_kf, np.int32), match_off=mo, matches=mv, point_bad=np.asarray(point_bad, np.uint8), obs_off=oo, obs_kf=ov)


def random_graph(seed, K, P, slots=300, bad_frac=0.05, max_obs=9, chain=None):
    """A trajectory-like map: keyframe k sees points around its stretch of the map (40 % of its slots empty), a point is observed by at
    most max_obs keyframes, up to 15 covisibles within 12 keyframes, 5 % bad keyframes and points.  The parent of k is k-1 (chain; the
    default for even seeds) or a random keyframe among the 6 before it (odd seeds)."""
    chain = seed % 2 == 0 if chain is None else chain
    rng = np.random.default_rng(seed)
    kf_bad = (rng.random(K) < bad_frac).astype(np.uint8)
    point_bad = (rng.random(P) < bad_frac).astype(np.uint8)
    centre = np.linspace(0, P, K)
    matches = []
    for k in range(K):
        ids = np.clip((centre[k] + rng.normal(0, max(P / K * 4, 8), slots)).astype(int), 0, P - 1)
        ids[rng.random(slots) < 0.4] = -1
        matches.append(ids)
    obs = [[] for _ in range(P)]
    for k in range(K):
        for p in np.unique(matches[k][matches[k] >= 0]):
            if len(obs[p]) < max_obs:
                obs[p].append(k)
    covis = []
    for k in range(K):
        n = rng.integers(0, 16)
        cand = np.clip(k + rng.permutation(np.arange(-12, 13))[:n], 0, K - 1)
        covis.append([c for c in dict.fromkeys(cand.tolist()) if c != k])
    parent = np.full(K, -1, np.int32)
    for k in range(1, K):
        parent[k] = k - 1 if chain else rng.integers(max(0, k - 6), k)
    children = [sorted(np.nonzero(parent == k)[0].tolist()) for k in range(K)]
    return _graph(kf_bad, point_bad, covis, children, parent, np.arange(-1, K - 1), matches, obs)


def frame_points_near(rng, g, kf, n=400):
    """a frame that tracks points of keyframe kf: n draws from its slots, 30 % of them emptied"""
    m = g["matches"][g["match_off"][kf]:g["match_off"][kf + 1]]
    fp = rng.choice(m, n)
    fp[rng.random(n) < 0.3] = -1
    return fp.astype(np.int32)


def chain_graph(K, V, far=100, bad_kf=None):
    """-> (graph, frame points).  Keyframe k has parent k-1, child k+1 and prev_kf k-1; its slots are [4k, 4k+1, -1, 4k+2, 4k+3, 4k+4, 4k+1]
    (a NULL slot, a point held twice, point 4k+4 shared with the next keyframe); observations follow from the slots; its only covisible is
    k+far where that keyframe exists.  The frame holds point 4k+1 for k < V, so exactly keyframes 0 .. V-1 are voted, one vote each."""
    P = 4 * K + 1
    matches = [[4 * k, 4 * k + 1, -1, 4 * k + 2, 4 * k + 3, 4 * k + 4, 4 * k + 1] for k in range(K)]
    obs = [[] for _ in range(P)]
    for k in range(K):
        for p in sorted(set(matches[k]) - {-1}):
            obs[p].append(k)
    kf_bad = np.zeros(K, np.uint8)
    if bad_kf is not None:
        kf_bad[bad_kf] = 1
    g = _graph(kf_bad, np.zeros(P, np.uint8), [[k + far] if k + far < K else [] for k in range(K)], [[k + 1] if k + 1 < K else [] for k in range(K)],
               np.arange(-1, K - 1), np.arange(-1, K - 1), matches, obs)
    return g, (4 * np.arange(V) + 1).astype(np.int32)


# chain_graph(200, V, bad_kf=bad_kf) with temporal_last_kf: the local keyframes and points the reference's loops end with
CHAIN_TABLE = [
    # V, temporal, bad_kf, local keyframes, local points
    (38, -1, None, 77, 310),    # 38 covisible and 1 child extension, no parent break
    (39, -1, None, 79, 318),
    (39, 199, None, 99, 399),   # 79 < 80: the temporal block adds 20
    (40, -1, None, 81, 326),    # the last visit pushes two; temporal skipped
    (40, 199, None, 81, 326),
    (40, -1, 40, 80, 322),      # a bad child is skipped; exactly 80: temporal skipped
    (40, 199, 40, 80, 322),
    (41, 199, None, 81, 326),   # `> 80` stops the loop at the 41st visit
    (79, 199, None, 81, 326),
    (80, 199, None, 81, 326),
    (81, 199, None, 81, 325),   # stops before the first visit
    (120, 199, None, 120, 481), # more voted keyframes than 80: no extension at all
]

# random_graph(seed, K, P, slots) and temporal_last_kf; the frames track the points of keyframes 0, K // 3, K // 2 and K - 1 in turn
RANDOM_CASES = [
    ((0, 40, 900, 300), -1),     # near 0 / 13 / 20 / 39: the parent break at the third or the first visit
    ((4, 12, 100, 300), 5),      # the temporal walk stalls on a marked keyframe
    ((16, 64, 1000, 257), 63),   # near 32: 17 temporal pushes, then a stall
    ((11, 3, 40, 40), 1),
    ((15, 1, 20, 30), 0),
    ((13, 260, 6000, 200), 200),
]


def case(name, graph, frame_points, temporal=-1):
    return dict(name=name, graph=graph, frame_points=np.ascontiguousarray(frame_points, np.int32), temporal_last_kf=int(temporal))


def all_cases(lds_keyframes):
    """Every case of the issue's list; lds_keyframes = local_map_limits()['lds_keyframes']: graphs at and one above it."""
    out = []
    for V, temporal, bad_kf, _, _ in CHAIN_TABLE:
        g, fp = chain_graph(200, V, bad_kf=bad_kf)
        out.append(case("chain V=%d t=%d bad=%s" % (V, temporal, bad_kf), g, fp, temporal))
    for args, temporal in RANDOM_CASES:
        g = random_graph(*args)
        rng = np.random.default_rng(100 + args[0])
        for kf in (0, args[1] // 3, args[1] // 2, args[1] - 1):
            out.append(case("random%s near %d" % (args, kf), g, frame_points_near(rng, g, kf), temporal))
    for temporal in (5, 15):
        g, fp = chain_graph(200, 10)
        out.append(case("chain V=10 t=%d" % temporal, g, fp, temporal))
    g = random_graph(9, 30, 500)
    for temporal in (-1, 7):
        out.append(case("only -1 t=%d" % temporal, g, np.full(50, -1, np.int32), temporal))
    out.append(case("no frame points", g, np.zeros(0, np.int32), 3))
    out.append(case("only bad points", g, np.nonzero(g["point_bad"])[0], -1))
    for K in (lds_keyframes, lds_keyframes + 1):
        gg, fp = chain_graph(K, 39)
        out.append(case("chain K=%d V=39" % K, gg, fp, K - 1))
    return out


def many_small(n, seed0=1000):
    """n problems of (K = 3, P = 40) with different seeds"""
    out = []
    for i in range(n):
        g = random_graph(seed0 + i, 3, 40, 40)
        out.append(case("small %d" % i, g, frame_points_near(np.random.default_rng(i), g, i % 3, 60), (i % 4) - 1))
    return out


def want_of(oracle, c):
    kfs, ref, pts, cleared = oracle.update_local_map(c["graph"], c["frame_points"], c["temporal_last_kf"])
    return dict(keyframes=kfs, reference_kf=ref, points=pts, cleared=cleared)


def assert_equal(got, want, what=""):
    assert np.array_equal(got["keyframes"], want["keyframes"]), "local keyframes: " + what
    assert got["reference_kf"] == want["reference_kf"], "reference keyframe: " + what
    assert np.array_equal(got["points"], want["points"]), "local points: " + what
    assert np.array_equal(got["cleared"], want["cleared"]), "cleared frame points: " + what
    assert got["n_keyframes"] == len(want["keyframes"]) and got["n_points"] == len(want["points"]) and got["n_cleared"] == int(want["cleared"].sum()), what


def same_results(a, b, what=""):
    for k in ("keyframes", "points", "cleared"):
        assert np.array_equal(a[k], b[k]), "%s: %s" % (k, what)
    for k in ("reference_kf", "n_voted", "n_keyframes", "n_points", "n_cleared"):
        assert a[k] == b[k], "%s: %s" % (k, what)
