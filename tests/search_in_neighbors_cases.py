"""Cases for the tests of LocalMapping::SearchInNeighbors in one call (tc2li_search_in_neighbors_batch and its host twin): small flat graphs
built with mapping_cases' Env, KfBuilder and poses, each made for one rule of include/tc2li_hip.h, and random graphs.

This module builds inputs; what the code under test should make of them is search_in_neighbors_ref.search_in_neighbors, run once per case
(`want`, cached) with a hook that looks at every search the reference runs: every float gate the search evaluates -- depth, image bounds,
distance range, viewing angle, the predicted level's distance from an integer, the window and the chi-square of every keypoint of the
keyframe -- stays clear of its threshold by mapping_cases.margin_ok's margin, so that integer results do not hang on a last bit.  A case
whose build violates a margin fails when it is built, on the CPU.

Geometry.  Row 0 is the current keyframe (mapping_cases.current_pose7 of the world); the other keyframes stand within a third of a metre of
it and look the same way (turned by a degree or two in the rotated world).  A location is a world point given by its pixel in the current
keyframe and its depth; every keyframe that sees it gets a keypoint at the exact projection (rounded to float32) with the octave the
search predicts there, and all map points at a location share max_distance_raw.  Descriptors of one location are a random base with a few
bits flipped, so distances are known exactly.

Hand-made cases use at most 6 keyframes of at most 16 keypoints; the exceptions are the target lists that must exceed 10 and 20 entries
(targets_wide, inertial_fill, inertial_full: one keypoint per keyframe) and the observation limit (113 keyframes of 4 keypoints)."""
import numpy as np

import mapping_cases as mc
import mapping_ref
import search_in_neighbors_ref as ref

BAD, MARKED = 1, 2
_cache = {}


def env_of(synthetic):
    if "env" not in _cache:
        _cache["env"] = mc.Env(synthetic)
    return _cache["env"]


# ---- the margin hook ---------------------------------------------------------------------------------------------------------------------
def assert_margins(env, view, bounds, pose7, P, where=""):
    """the gates ORBmatcher::Fuse evaluates for map point P in the keyframe, in float64 (every keypoint of the keyframe, not only the cells walked)"""
    def clear(*gate):
        assert mc.margin_ok(gate), (where, gate)
    R, t = mc.pose_Rt(pose7)
    Xw = np.asarray(P["pos"], np.float64)
    x, y, z = R @ Xw + t
    clear("rel", z, 0.0, 1.0)
    if z < 0:
        return
    u, v = env.fx * x / z + env.cx, env.fy * y / z + env.cy
    b = [float(np.float32(q)) for q in bounds]
    for val, th, ext in ((u, b[0], b[1] - b[0]), (u, b[1], b[1] - b[0]), (v, b[2], b[3] - b[2]), (v, b[3], b[3] - b[2])):
        clear("rel", val, th, ext)
    if not (b[0] <= u < b[1] and b[2] <= v < b[3]):
        return
    PO = Xw - mc.centre((R, t))
    dist = np.linalg.norm(PO)
    clear("rel", dist, float(P["min_distance"])); clear("rel", dist, float(P["max_distance"]))
    if dist < float(P["min_distance"]) or dist > float(P["max_distance"]):
        return
    cosv = PO @ np.asarray(P["normal"], np.float64) / dist
    clear("cos", cosv, 0.5)
    if cosv < 0.5:
        return
    lv = np.log(float(P["max_distance_raw"]) / dist) / env.logsf
    clear("rel", lv, float(np.round(lv)), 1.0)
    level = min(max(int(np.ceil(lv)), 0), len(env.sf) - 1)
    r = 3.0 * float(env.sf[level])
    ur = u - env.bf / z
    for k in range(len(view["keys"])):
        kx, ky, ko = float(view["keys"]["x"][k]), float(view["keys"]["y"][k]), int(view["keys"]["octave"][k])
        clear("rel", abs(kx - u), r)
        if not abs(kx - u) < r:
            continue
        clear("rel", abs(ky - v), r)
        if not abs(ky - v) < r or ko < level - 1 or ko > level:
            continue
        e2 = (u - kx) ** 2 + (v - ky) ** 2
        if view["u_right"][k] >= 0:
            clear("rel", (e2 + (ur - float(view["u_right"][k])) ** 2) * float(env.isg[ko]), 7.8)
        else:
            clear("rel", e2 * float(env.isg[ko]), 5.99)


# ---- the builder -------------------------------------------------------------------------------------------------------------------------
class Graph:
    def __init__(self, env, world, n_kf, seed=0, bounds=mc.BOUNDS0, spread=0.3):
        self.env, self.world, self.n_kf, self.bounds = env, world, n_kf, bounds
        self.rng = np.random.default_rng(seed)
        cur7 = mc.current_pose7(world)
        self.poses7 = [cur7]
        for k in range(1, n_kf):
            a = 2.399963 * k   # the golden angle: centres on a spiral, no two alike
            c = (spread * np.cos(a) * (0.3 + 0.7 * k / n_kf), 0.25 * spread * np.sin(a), 0.4 * spread * np.sin(1.7 * a))
            self.poses7.append(mc.neighbour_pose7(world, cur7, mc.SIDE, c=c, turn=0.0 if world == "identity" else 1.0 + (k % 3)))
        self.poses = [mc.pose_Rt(p) for p in self.poses7]
        self.b = [mc.KfBuilder() for _ in range(n_kf)]
        self.kf_flags = np.zeros(n_kf, np.uint8)
        self.prev_kf = np.full(n_kf, -1, np.int32)
        self.covis = [[] for _ in range(n_kf)]
        self.slots = [dict() for _ in range(n_kf)]
        self.points = []
        self._lattice = 0

    def descriptor(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def loc(self, uv0=None, z=9.0, level=2):
        """a world point at pixel uv0 (default: the next lattice place) and depth z of the current keyframe"""
        if uv0 is None:
            k = self._lattice
            self._lattice += 1
            assert k < 13 * 5
            uv0 = (110.0 + 44.0 * (k % 13), 50.0 + 43.0 * (k // 13))
        e = self.env
        R, t = self.poses[0]
        xc = np.array([(uv0[0] - e.cx) * z / e.fx, (uv0[1] - e.cy) * z / e.fy, z])
        X = (R.T @ (xc - t)).astype(np.float32)
        dist = np.linalg.norm(X.astype(np.float64) - mc.centre(self.poses[0]))
        return dict(X=X, dist=dist, max_raw=np.float32(dist * 1.2 ** (level - 0.5)), base=self.descriptor())

    def level_in(self, kf, L):
        d = np.linalg.norm(L["X"].astype(np.float64) - mc.centre(self.poses[kf]))
        return min(max(int(np.ceil(np.log(float(L["max_raw"]) / d) / self.env.logsf)), 0), len(self.env.sf) - 1)

    def kp(self, kf, L, desc=None, stereo=True, d=(0.0, 0.0), octave=None):
        """a keypoint of keyframe kf at the projection of location L (+ d pixels) -> its index"""
        e = self.env
        uv, z = e.project(self.poses[kf], L["X"].astype(np.float64))
        b = self.bounds
        assert b[0] + 8 < uv[0] < b[1] - 8 and b[2] + 8 < uv[1] < b[3] - 8 and z > 1, (kf, uv, z)
        kw = dict(ur=uv[0] - e.bf / z, depth=z) if stereo else {}
        return self.b[kf].add(uv + np.asarray(d, np.float64), 0, L["base"] if desc is None else desc, octave=self.level_in(kf, L) if octave is None else octave, **kw)

    def pt(self, L, desc=None, obs=(), flags=0, nobs=None, found=1, visible=1, ref_kf=None, slots=True, extra_slots=()):
        """a map point at L observed at obs = [(kf, keypoint)] (ascending by kf); extra_slots: slots that hold it without an observation"""
        e = self.env
        obs = sorted(obs)
        PO = L["X"].astype(np.float64) - mc.centre(self.poses[0])
        rec = np.zeros((), mc.MP)
        rec["pos"], rec["normal"] = L["X"], (PO / np.linalg.norm(PO)).astype(np.float32)
        rec["min_distance"], rec["max_distance"], rec["max_distance_raw"] = np.float32(0.5 * L["dist"]), np.float32(2.0 * L["dist"]), L["max_raw"]
        rec["descriptor"] = L["base"] if desc is None else desc
        if nobs is None:
            nobs = sum(2 if self.b[kf].rows[i]["ur"] >= 0 else 1 for kf, i in obs)
        ref_kf = (obs[0][0] if obs else 0) if ref_kf is None else ref_kf
        oct_ref = dict(obs).get(ref_kf)
        scale = float(e.sf[self.b[ref_kf].rows[oct_ref]["octave"]]) if oct_ref is not None else 1.0
        self.points.append(dict(rec=rec, obs=obs, flags=flags, nobs=nobs, found=found, visible=visible, ref_kf=ref_kf, ref_scale=scale))
        p = len(self.points) - 1
        for kf, i in (list(obs) if slots else []) + list(extra_slots):
            assert i not in self.slots[kf], (kf, i)
            self.slots[kf][i] = p
        return p

    def finish(self, name, current=0, inertial=False, abort=False):
        views = [b.finish(p7, 0, shuffle=False) if b.rows else mc.empty_keyframe(p7) for b, p7 in zip(self.b, self.poses7)]
        n = [len(v["keys"]) for v in views]
        so = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        slot_point = np.full(int(so[-1]), -1, np.int32)
        for kf, s in enumerate(self.slots):
            for i, p in s.items():
                slot_point[so[kf] + i] = p
        P = self.points
        pr = dict(kf_slot=np.arange(self.n_kf, dtype=np.int32), kf_flags=self.kf_flags.copy(), prev_kf=self.prev_kf.copy(),
                  poses7=np.array(self.poses7, np.float32), covis_offsets=np.concatenate([[0], np.cumsum([len(c) for c in self.covis])]).astype(np.int32),
                  covis=np.array([k for c in self.covis for k in c], np.int32), slot_offsets=so, slot_point=slot_point,
                  points=np.array([p["rec"] for p in P], mc.MP) if P else np.zeros(0, mc.MP), point_flags=np.array([p["flags"] for p in P], np.uint8),
                  point_nobs=np.array([p["nobs"] for p in P], np.int32), point_found=np.array([p["found"] for p in P], np.int32),
                  point_visible=np.array([p["visible"] for p in P], np.int32), point_ref_kf=np.array([p["ref_kf"] for p in P], np.int32),
                  point_ref_level_scale=np.array([p["ref_scale"] for p in P], np.float32),
                  obs_offsets=np.concatenate([[0], np.cumsum([len(p["obs"]) for p in P])]).astype(np.int32),
                  obs_kf=np.array([kf for p in P for kf, _ in p["obs"]], np.int32), obs_index=np.array([i for p in P for _, i in p["obs"]], np.int32),
                  current=current, inertial=inertial, abort=abort, last_level_scale=float(self.env.sf[-1]))
        return dict(name=name, problem=pr, views=views, bounds=np.float32(self.bounds), world=self.world)


def want_of(case, env):
    """the reference's outputs for a case, computed once, with the margin condition asserted on every search it runs"""
    if "want" not in case:
        pr, views = case["problem"], case["views"]
        poses = np.asarray(pr["poses7"]).reshape(-1, 7)

        def hook(T, p, P):
            assert_margins(env, views[int(pr["kf_slot"][T])], case["bounds"], poses[T], P, (case["name"], T, p))
        case["want"] = ref.search_in_neighbors(pr, views, case["bounds"], env, hook)
    return case["want"]


def ops_of(case, env):
    return [tuple(int(v) for v in o) for o in want_of(case, env)["ops"]]


# ---- hand-made cases ---------------------------------------------------------------------------------------------------------------------
def order_case(env, world, abort=False):
    """Rule 2 / 3: p absorbs target 1's occupant, its median descriptor becomes the occupant's, and in target 2 it is fused with another keypoint
    than its entry descriptor finds.  Rows: 0 current, 1 and 2 targets, 3 and 4 further observers."""
    g = Graph(env, world, 5, seed=11)
    g.covis[0] = [1, 2]
    L = g.loc()
    A = L["base"]
    B = mc.flip(A, 30, 100)
    p = g.pt(L, A, obs=[(0, g.kp(0, L, A)), (3, g.kp(3, L, mc.flip(A, 40, 0)))])
    q = g.pt(L, B, obs=[(1, g.kp(1, L, B)), (4, g.kp(4, L, mc.flip(B, 2, 200)))])
    ka = g.kp(2, L, mc.flip(A, 5, 0))
    kb = g.kp(2, L, mc.flip(B, 5, 150), d=(1.0, 0.0))
    case = g.finish("order" + ("_abort" if abort else "") + "_" + world, abort=abort)
    case.update(p=p, q=q, ka=ka, kb=kb)
    # the case is what it is made for: the entry state finds ka in target 2, the reference's order finds kb
    v, pr = case["views"][2], case["problem"]
    _, bi, _ = mapping_ref.fuse_search(v["keys"], v["descriptors"], v["u_right"], case["bounds"], pr["poses7"][2], env.cam4, env.bf, env.sf, env.isg, env.logsf,
                                       pr["points"][p:p + 1], [1])
    assert int(bi[0]) == ka
    assert ops_of(case, env)[:2] == [(ref.REPLACE, 0, p, q, p, 1, 0), (ref.ADD_OBSERVATION, 1, p, -1, -1, 2, kb)]
    return case


def direction_case(env, world):
    """Rule 3 / 4, one target (row 1); rows 2 .. 5 only observe.  Every scenario has its own location; see the asserts for what each gives."""
    g = Graph(env, world, 6, seed=12)
    g.covis[0] = [1]
    c = {}
    # a: equal counts -- the occupant is replaced
    L = g.loc(); c["pa"] = g.pt(L, obs=[(0, g.kp(0, L))]); c["qa"] = g.pt(L, obs=[(1, g.kp(1, L))])
    # b: stereo weights decide, not the number of observations: 3 mono observations (nObs 3) against 2 stereo ones (nObs 4)
    L = g.loc(); c["pb"] = g.pt(L, obs=[(0, g.kp(0, L, stereo=False)), (2, g.kp(2, L, stereo=False)), (3, g.kp(3, L, stereo=False))])
    c["qb"] = g.pt(L, obs=[(1, g.kp(1, L)), (4, g.kp(4, L))])
    # c: an occupant that turned bad earlier in the same target: qc is observed at t1 and also sits, without an observation, in the slot t2
    L1, L2 = g.loc(), g.loc()
    t1, t2 = g.kp(1, L1), g.kp(1, L2)
    c["pc1"] = g.pt(L1, obs=[(0, g.kp(0, L1))]); c["pc2"] = g.pt(L2, obs=[(0, g.kp(0, L2))])
    c["qc"] = g.pt(L1, obs=[(1, t1)], extra_slots=[(1, t2)])
    # d: a list point that turns bad through an earlier entry: pd2 sits, without an observation, in the slot that pd1 reaches
    L1, L2 = g.loc(), g.loc()
    c["pd1"] = g.pt(L1, obs=[(0, g.kp(0, L1))])
    c["pd2"] = g.pt(L2, obs=[(0, g.kp(0, L2))], extra_slots=[(1, g.kp(1, L1))])
    c["td2"] = g.kp(1, L2)   # free, and pd2's search finds it: the apply step must not use it
    # e: a list point that enters the target through an earlier entry: pe holds two slots of the current keyframe
    L = g.loc(); k0 = g.kp(0, L); c["pe"] = g.pt(L, obs=[(0, k0)], extra_slots=[(0, g.kp(0, L, d=(0.5, 0.5)))]); c["te"] = g.kp(1, L)
    # f: two list points reach one free slot; the second Replace meets a keyframe (the current one) that the winner is already in
    L = g.loc(); c["pf1"] = g.pt(L, obs=[(0, g.kp(0, L))]); c["kf2"] = g.kp(0, L, d=(0.5, -0.5)); c["pf2"] = g.pt(L, obs=[(0, c["kf2"])]); c["tf"] = g.kp(1, L)
    # g: x == w: pg sits in the target's slot without an observation there
    L = g.loc(); c["pg"] = g.pt(L, obs=[(0, g.kp(0, L))], extra_slots=[(1, g.kp(1, L))])
    case = g.finish("direction_" + world)
    case.update(c)
    w = want_of(case, env)
    ops = {(o[2], o[3]): o for o in ops_of(case, env) if o[1] == 0}
    assert ops[(c["pa"], c["qa"])][4] == c["pa"] and ops[(c["pb"], c["qb"])][4] == c["qb"]
    assert ops[(c["pc1"], c["qc"])][4] == c["pc1"] and not any(o[2] == c["pc2"] and o[1] == 0 for o in ops.values())
    assert ops[(c["pd1"], c["pd2"])][4] == c["pd1"] and w["slot_point_out"][case["problem"]["slot_offsets"][1] + c["td2"]] == -1
    assert ops[(c["pe"], -1)][0] == ref.ADD_OBSERVATION and ops[(c["pf1"], -1)][0] == ref.ADD_OBSERVATION
    assert ops[(c["pf2"], c["pf1"])][4] == c["pf1"] and w["slot_point_out"][c["kf2"]] == -1 and w["point_nobs_out"][c["pf1"]] == 4
    assert not any(o[2] == c["pg"] for o in ops.values())
    assert int(w["target_fused"][0]) == 9   # a, b, c1, c2 (bad occupant), d1, e, f1, f2, g (x == w)
    return case


def stage2_case(env, world):
    """Rule 6: rows 0 current, 1 target, 2 and 3 observers."""
    g = Graph(env, world, 4, seed=13)
    g.covis[0] = [1]
    c = {}
    # a: stage 1 moves pa into the target, so pa is a candidate (and is skipped: it is in the current keyframe); its loser qa is not one
    L = g.loc(); c["pa"] = g.pt(L, obs=[(0, g.kp(0, L))]); c["qa"] = g.pt(L, obs=[(1, g.kp(1, L))])
    # b: a point marked on entry, which would otherwise be fused into the free keypoint of the current keyframe
    L = g.loc(); c["rb"] = g.pt(L, obs=[(1, g.kp(1, L)), (2, g.kp(2, L))], flags=MARKED); c["kb"] = g.kp(0, L)
    # c: a candidate that gains the current keyframe
    L = g.loc(); c["sc"] = g.pt(L, obs=[(1, g.kp(1, L)), (2, g.kp(2, L))]); c["kc"] = g.kp(0, L)
    # d: a candidate that absorbs a point of the current keyframe which stage 1 did not reach (its descriptor is 90 bits from the target's)
    L = g.loc(); D = mc.flip(L["base"], 10, 100)
    c["sd"] = g.pt(L, D, obs=[(1, g.kp(1, L, D)), (3, g.kp(3, L, D))]); c["kd"] = g.kp(0, L); c["ud"] = g.pt(L, mc.flip(L["base"], 80, 0), obs=[(0, c["kd"])])
    case = g.finish("stage2_" + world)
    case.update(c)
    w = want_of(case, env)
    assert w["candidates"].tolist() == [c["pa"], c["sc"], c["sd"]] and int(w["fused_current"]) == 2
    ops = [o for o in ops_of(case, env) if o[1] == 1]
    assert ops == [(ref.ADD_OBSERVATION, 1, c["sc"], -1, -1, 0, c["kc"]), (ref.REPLACE, 1, c["sd"], c["ud"], c["sd"], 0, c["kd"])]
    assert w["slot_point_out"][c["kb"]] == -1
    return case


def median_case(env, world):
    """Rule 4 / 7, the descriptor choice, through the refresh of a keyframe without targets: N = 1, 2, 3, an even N with a tie that the first
    row takes, an even N whose choice is not the first row, and an observer keyframe that is bad (row 5)."""
    g = Graph(env, world, 6, seed=14)
    g.kf_flags[5] = BAD
    c = {}

    def point(name, flips, rows=None):
        """flips: per observation the (bits, first bit) pairs inverted in the location's base descriptor, one after the other"""
        L = g.loc()
        obs = []
        for kf, fl in zip(range(len(flips)) if rows is None else rows, flips):
            d = L["base"]
            for n, start in fl:
                d = mc.flip(d, n, start)
            obs.append((kf, g.kp(kf, L, d)))
        c[name] = g.pt(L, obs=obs)
    point("n1", [[]])
    point("n2", [[], [(9, 0)]])
    point("n3", [[], [(30, 0)], [(30, 0), (2, 100)]])                              # medians 30, 2, 2: row 1
    point("tie", [[], [(10, 0)], [(20, 50)], [(4, 100)]])                          # medians 4, 10, 20, 4: row 0
    point("even", [[], [(40, 0)], [(42, 0)], [(60, 100)]])                         # medians 40, 2, 2, 60: row 1
    # row 5 is bad: without it as n3 (row 1); with it the medians would be 30, 2, 1, 1 and row 2 would win
    point("badkf", [[], [(30, 0)], [(30, 0), (2, 100)], [(30, 0), (2, 100), (1, 150)]], rows=[0, 1, 2, 5])
    case = g.finish("median_" + world)
    case.update(c)
    w = want_of(case, env)
    assert [int(w["desc_kf"][c[k]]) for k in ("n1", "n2", "n3", "tie", "even", "badkf")] == [0, 0, 1, 0, 1, 1]
    assert w["refreshed"].tolist() == [1] * 6
    return case


def targets_case(env, world):
    """Rule 1 on 6 keyframes: row 2 bad, row 3 marked on entry; the second-ring list of row 1 holds the current keyframe, row 1 itself, the bad
    row; row 5 is reachable only through the second-ring keyframe 4, whose own neighbours are not visited."""
    g = Graph(env, world, 6, seed=15)
    g.kf_flags[2], g.kf_flags[3] = BAD, MARKED
    g.covis[0], g.covis[1], g.covis[4] = [2, 1, 3], [0, 1, 4, 2], [5]
    L = g.loc()
    for kf in range(6):
        g.kp(kf, L)
    g.pt(L, obs=[(0, 0)])
    case = g.finish("targets_" + world)
    assert want_of(case, env)["targets"].tolist() == [1, 4]
    return case


def many_keyframes(env, world, n_kf, seed):
    g = Graph(env, world, n_kf, seed=seed)
    L = g.loc(uv0=(400.0, 150.0))
    for kf in range(n_kf):
        g.kp(kf, L)
    g.pt(L, obs=[(0, 0)])
    return g


def targets_wide_case(env, world):
    """12 first-ring entries (10 are read), 24 second-ring entries of the first target (20 are read)"""
    g = many_keyframes(env, world, 40, 16)
    g.covis[0], g.covis[1] = list(range(1, 13)), list(range(13, 37))
    case = g.finish("targets_wide_" + world)
    assert want_of(case, env)["targets"].tolist() == list(range(1, 11)) + list(range(13, 33))
    return case


def inertial_cases(env, world):
    """inertial: mPrevKF fills up to 20 targets past a bad and a marked keyframe; with 22 targets from the lists it adds nothing"""
    g = many_keyframes(env, world, 26, 17)
    g.covis[0] = [1, 2]
    chain = [0] + list(range(3, 26))
    for a, b in zip(chain[:-1], chain[1:]):
        g.prev_kf[a] = b
    g.kf_flags[4], g.kf_flags[5] = BAD, MARKED
    fill = g.finish("inertial_fill_" + world, inertial=True)
    assert want_of(fill, env)["targets"].tolist() == [1, 2, 3] + list(range(6, 23))
    g = many_keyframes(env, world, 26, 18)
    g.covis[0], g.covis[1] = [1, 2], list(range(3, 23))
    g.prev_kf[0] = 23
    g.prev_kf[23] = 24
    full = g.finish("inertial_full_" + world, inertial=True)
    assert len(want_of(full, env)["targets"]) == 22 and 23 not in want_of(full, env)["targets"]
    return [fill, full]


def abort_case(env, world):
    """Rule 1 / 5 with abort: the second ring stops after i = 0 (row 3 through target 1 is taken, row 4 through target 2 is not), stage 1 runs,
    nothing after it."""
    g = Graph(env, world, 5, seed=19)
    g.covis[0], g.covis[1], g.covis[2] = [1, 2], [3], [4]
    L = g.loc(); p = g.pt(L, obs=[(0, g.kp(0, L))]); g.kp(1, L)
    L = g.loc(); g.pt(L, obs=[(2, g.kp(2, L)), (3, g.kp(3, L))]); g.kp(0, L); g.kp(4, L)
    case = g.finish("abort_" + world, abort=True)
    w = want_of(case, env)
    assert w["targets"].tolist() == [1, 2, 3] and ops_of(case, env) == [(ref.ADD_OBSERVATION, 0, p, -1, -1, 1, 0)]
    assert len(w["candidates"]) == 0 and not w["refreshed"].any() and (w["desc_kf"] == -1).all()
    return case


def limit_case(env, limit=112):
    """One point driven past the observation limit by a merge: p is seen by rows 0, 2 .. 57 (57 observations), q by rows 1, 58 .. 112 (56);
    equal-or-fewer nObs on q's side, so q.Replace(p) and p reaches 113."""
    n_kf = limit + 1
    g = Graph(env, "identity", n_kf, seed=20, spread=0.2)
    g.covis[0] = [1]
    L = g.loc(uv0=(400.0, 150.0))
    ks = [g.kp(kf, L) for kf in range(n_kf)]
    for kf in range(n_kf):   # 4 keypoints per keyframe
        for d in ((60.0, 0.0), (0.0, 50.0), (-60.0, 0.0)):
            g.kp(kf, L, desc=g.descriptor(), d=d)
    half = (n_kf + 1) // 2
    p = g.pt(L, obs=[(0, ks[0])] + [(kf, ks[kf]) for kf in range(2, half + 1)])
    q = g.pt(L, obs=[(1, ks[1])] + [(kf, ks[kf]) for kf in range(half + 1, n_kf)])
    case = g.finish("limit")
    w = want_of(case, env)
    assert w["point_bad_out"][q] == 1 and w["obs_offsets_out"][p + 1] - w["obs_offsets_out"][p] == limit + 1
    return case


def stale_winner_case(env, world="identity"):
    """A slot that holds a point without the matching observation, placed so that the side-by-side search of a target's list would go wrong:
    q sits in the target's slot t1 without observing the target; p reaches t1, q has more observations and wins (p.Replace(q)); q gains p's
    observation in row 3, its median descriptor becomes that one, it is still not in the target and its own entry comes later in the list.
    The reference searches q with the new descriptor and finds kb; the descriptor q had when the target started finds ka.
    Rows: 0 current, 1 target, 2 .. 4 observers."""
    g = Graph(env, world, 5, seed=22)
    g.covis[0] = [1]
    L1, L2 = g.loc(), g.loc()
    A = L2["base"]
    B = mc.flip(A, 30, 100)
    p = g.pt(L1, obs=[(0, g.kp(0, L1)), (3, g.kp(3, L1, B))])
    t1 = g.kp(1, L1)
    q = g.pt(L2, A, obs=[(0, g.kp(0, L2, A)), (2, g.kp(2, L2, mc.flip(A, 40, 0))), (4, g.kp(4, L2, mc.flip(B, 2, 200)))], extra_slots=[(1, t1)])
    ka = g.kp(1, L2, mc.flip(A, 5, 0))
    kb = g.kp(1, L2, mc.flip(B, 5, 150), d=(1.0, 0.0))
    case = g.finish("stale_winner_" + world)
    v, pr = case["views"][1], case["problem"]
    _, bi, _ = mapping_ref.fuse_search(v["keys"], v["descriptors"], v["u_right"], case["bounds"], pr["poses7"][1], env.cam4, env.bf, env.sf, env.isg, env.logsf,
                                       pr["points"][q:q + 1], [1])
    assert int(bi[0]) == ka
    assert ops_of(case, env)[:2] == [(ref.REPLACE, 0, p, q, q, 1, t1), (ref.ADD_OBSERVATION, 0, q, -1, -1, 1, kb)]
    return case


def many_candidates_case(env, per_target=400, n_targets=9):
    """Stage 2 with more candidates than the device path searches in one piece (3 072): 9 targets of 400 keypoints, each holding a point of its
    own; the current keyframe has free keypoints for 8 points of the first target and 8 of the last (list positions beyond 3 200), and one
    keypoint whose point the last target's candidate absorbs (its descriptor is 80 bits from the target's, so stage 1 does not reach it)."""
    g = Graph(env, "rotated", 1 + n_targets, seed=21)
    g.covis[0] = list(range(1, 1 + n_targets))
    picked = {}
    for t in range(1, 1 + n_targets):
        for k in range(per_target):
            L = g.loc(uv0=(100.0 + 14.0 * (k % 40) + 1.3 * t, 40.0 + 22.0 * (k // 40) + 2.1 * t))
            p = g.pt(L, obs=[(t, g.kp(t, L))])
            if t in (1, n_targets) and k % 50 == 7:
                picked[p] = g.kp(0, L)
            if t == n_targets and k == 333:
                D = mc.flip(L["base"], 80, 0)
                k_absorbed = g.kp(0, L)
                absorbed = g.pt(L, D, obs=[(0, k_absorbed)])
                last = p
    case = g.finish("many_candidates")
    w = want_of(case, env)
    ops = ops_of(case, env)
    assert len(w["candidates"]) == per_target * n_targets > 3072 and not any(o[1] < n_targets for o in ops)
    assert [(o[0], o[2], o[6]) for o in ops if o[0] == ref.ADD_OBSERVATION] == [(ref.ADD_OBSERVATION, p, k) for p, k in sorted(picked.items())]
    assert [o for o in ops if o[0] == ref.REPLACE] == [(ref.REPLACE, n_targets, last, absorbed, last, 0, k_absorbed)]
    assert max(list(w["candidates"]).index(o[2]) for o in ops) > 3200
    return case


# ---- random graphs -----------------------------------------------------------------------------------------------------------------------
RANDOM_SEEDS = (1, 3, 4, 5)   # seeds whose graphs keep every margin and produce every kind of op (random_case asserts both)


def random_case(env, world, seed):
    """8 to 14 keyframes of 40 to 120 keypoints, 60 to 300 points: locations seen by two or three tracks (map points) with disjoint observers,
    so that the searches merge them; some keypoints hold no point.  The generator checks what the seed produces (see below)."""
    rng = np.random.default_rng(1000 + seed)
    n_kf = int(rng.integers(8, 15))
    g = Graph(env, world, n_kf, seed=2000 + seed)
    n_loc = int(rng.integers(65, 106))
    used = set()
    for _ in range(n_loc):
        while True:   # pixels at least 24 apart in the current keyframe, so that neighbours in the image belong to one location
            cell = (int(rng.integers(0, 22)), int(rng.integers(0, 9)))
            if cell not in used:
                used.add(cell)
                break
        uv0 = (130.0 + 24.0 * cell[0] + rng.uniform(0, 6), 45.0 + 24.0 * cell[1] + rng.uniform(0, 6))
        L = g.loc(uv0=uv0, z=float(rng.uniform(7.0, 11.0)), level=int(rng.integers(1, 5)))
        seen = [kf for kf in range(n_kf) if rng.random() < 0.75]
        kps = {kf: g.kp(kf, L, mc.flip(L["base"], int(rng.integers(0, 13)), int(rng.integers(0, 200))), stereo=bool(rng.random() < 0.7)) for kf in seen}
        owner = {kf: int(rng.integers(0, 4)) for kf in seen}   # track 0 .. 2, 3: the keypoint holds no point
        for track in range(3):
            obs = [(kf, kps[kf]) for kf in seen if owner[kf] == track]
            if obs:
                g.pt(L, g.b[obs[0][0]].rows[obs[0][1]]["desc"], obs=obs, found=int(rng.integers(1, 9)), visible=int(rng.integers(9, 20)),
                     flags=MARKED if rng.random() < 0.03 else 0)
    others = list(range(1, n_kf))
    g.covis[0] = [int(k) for k in rng.permutation(others)[:int(rng.integers(3, 6))]]
    for kf in others:
        g.covis[kf] = [int(k) for k in rng.permutation(n_kf)[:int(rng.integers(0, 5))]]
    if n_kf > 9:
        g.kf_flags[n_kf - 1] = BAD
    case = g.finish("random_%s_%d" % (world, seed))
    n = [len(v["keys"]) for v in case["views"]]
    assert 8 <= n_kf <= 14 and 40 <= min(n) and max(n) <= 120 and 60 <= len(g.points) <= 300, (n_kf, min(n), max(n), len(g.points))
    ops = ops_of(case, env)
    assert any(o[0] == ref.ADD_OBSERVATION for o in ops), case["name"]
    assert any(o[0] == ref.REPLACE and o[4] == o[2] for o in ops) and any(o[0] == ref.REPLACE and o[4] == o[3] for o in ops), case["name"]
    return case


def hand_made(env):
    if "hand" not in _cache:
        cases = []
        for world in mc.WORLDS:
            cases += [order_case(env, world), direction_case(env, world), stage2_case(env, world), median_case(env, world), targets_case(env, world),
                      abort_case(env, world)]
        cases += [targets_wide_case(env, "identity")] + inertial_cases(env, "rotated")
        _cache["hand"] = cases
    return _cache["hand"]


def random_cases(env):
    if "random" not in _cache:
        _cache["random"] = [random_case(env, world, seed) for world in mc.WORLDS for seed in RANDOM_SEEDS]
    return _cache["random"]


def the_limit_case(env):
    if "limit" not in _cache:
        _cache["limit"] = limit_case(env)
    return _cache["limit"]


def the_many_candidates_case(env):
    if "many" not in _cache:
        _cache["many"] = many_candidates_case(env)
    return _cache["many"]


def the_stale_winner_case(env):
    if "stale" not in _cache:
        _cache["stale"] = stale_winner_case(env)
    return _cache["stale"]
