"""Cases for the tests of LocalMapping::ProcessNewKeyFrame in one call (tc2li_process_new_keyframe_batch and its host twin): small flat graphs,
each made for one rule of include/tc2li_hip.h and carrying the lists the rule gives written out by hand (`expect`), and seeded random graphs.
What the code under test should make of any case is process_new_keyframe_ref.process_new_keyframe (`want_of`, cached).

A keyframe here is a list of keypoints (descriptor, u_right) and a camera centre; nothing in ProcessNewKeyFrame projects a point, so the
keypoints' pixels are a lattice and the poses the identity.  Descriptors are a random base with chosen bits flipped (mapping_cases.flip), so
Hamming distances are known exactly.

A note on the threshold case.  KeyFrame::UpdateConnections never counts the current keyframe's own observations (KeyFrame.cc:418 skips
mnId == this->mnId), and AddObservation(current, i) is the only change the loop makes, so the votes taken on the observation rows on entry
and on the rows after the loop are the same numbers whatever the graph: no graph can tell the two apart through the votes.  What does tell a
wrong implementation apart is WHICH POINTS vote: every point of the slot row that is not bad, whether or not the current keyframe observed
it on entry.  The case gives one neighbour exactly 15 and another exactly 14 shared points, and for the first the 15th is a point that gains
its observation in this call; an implementation that takes the votes from the points the current keyframe observes on entry (the
covisibility as the entry state's observation rows alone define it) counts 14 and connects nobody by the threshold."""
import numpy as np

import mapping_cases as mc
import process_new_keyframe_ref as ref

IDENTITY7 = np.float32([0, 0, 0, 1, 0, 0, 0])
UNCHANGED, UPDATED = 0, 1
_cache = {}


class Graph:
    """rows of keyframes with their keypoints, points with their observations, the current keyframe's slots"""

    def __init__(self, n_kf, current=0, seed=0, slotless=()):
        self.n_kf, self.current, self.slotless = n_kf, current, set(slotless)
        self.rng = np.random.default_rng(seed)
        self.kps = [[] for _ in range(n_kf)]          # per keyframe: (descriptor, stereo)
        self.centres = self.rng.uniform(-1.0, 1.0, (n_kf, 3)).astype(np.float32)
        self.kf_flags = np.zeros(n_kf, np.uint8)
        self.conn = [dict() for _ in range(n_kf)]
        self.points, self.slots = [], {}

    def descriptor(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def kp(self, kf, desc=None, stereo=True):
        """a keypoint of keyframe kf -> its index"""
        self.kps[kf].append((self.descriptor() if desc is None else np.asarray(desc, np.uint8), stereo))
        return len(self.kps[kf]) - 1

    def pt(self, obs=(), bad=0, nobs=None, ref_kf=None, ref_scale=1.2, pos=None):
        """a map point observed at obs = [(kf, keypoint)]"""
        obs = sorted(obs)
        assert len({kf for kf, _ in obs}) == len(obs)
        if nobs is None:
            nobs = sum(2 if self.kps[kf][i][1] else 1 for kf, i in obs)
        pos = (self.rng.uniform(-4.0, 4.0, 3) + [0, 0, 12.0]) if pos is None else pos
        self.points.append(dict(obs=obs, bad=bad, nobs=nobs, ref_kf=(obs[0][0] if obs else self.current) if ref_kf is None else ref_kf, ref_scale=ref_scale,
                                pos=np.asarray(pos, np.float32)))
        return len(self.points) - 1

    def hold(self, i, p):
        """slot i of the current keyframe holds point p"""
        assert i not in self.slots and 0 <= i < len(self.kps[self.current])
        self.slots[i] = p

    def seen(self, desc=None, stereo=True, **kw):
        """a new keypoint of the current keyframe that holds a new point -> (slot, point)"""
        i = self.kp(self.current, desc, stereo)
        p = self.pt(**kw)
        self.hold(i, p)
        return i, p

    def finish(self, name, expect=None, **scalars):
        views = []
        for kf, rows in enumerate(self.kps):
            if kf in self.slotless:
                assert not rows
                views.append(None)
                continue
            b = mc.KfBuilder()
            for k, (d, stereo) in enumerate(rows):
                b.add((20.0 + 11.0 * (k % 64), 20.0 + 9.0 * (k // 64)), 0, d, **(dict(ur=5.0 + k, depth=4.0) if stereo else {}))
            views.append(b.finish(IDENTITY7, 0, shuffle=False) if rows else mc.empty_keyframe(IDENTITY7))
        slot, k = [], 0
        for kf in range(self.n_kf):
            slot.append(-1 if kf in self.slotless else k)
            k += kf not in self.slotless
        ns = len(self.kps[self.current])
        slot_point = np.full(ns, -1, np.int32)
        for i, p in self.slots.items():
            slot_point[i] = p
        P = self.points
        pr = dict(kf_slot=np.array(slot, np.int32), kf_flags=self.kf_flags.copy(), centres=self.centres.copy(),
                  conn_offsets=np.concatenate([[0], np.cumsum([len(c) for c in self.conn])]).astype(np.int32),
                  conn_kf=np.array([k for c in self.conn for k in sorted(c)], np.int32), conn_weight=np.array([c[k] for c in self.conn for k in sorted(c)], np.int32),
                  slot_point=slot_point, point_bad=np.array([p["bad"] for p in P], np.uint8),
                  positions=np.array([p["pos"] for p in P], np.float32).reshape(-1, 3), point_nobs=np.array([p["nobs"] for p in P], np.int32),
                  point_ref_kf=np.array([p["ref_kf"] for p in P], np.int32), point_ref_level_scale=np.array([p["ref_scale"] for p in P], np.float32),
                  obs_offsets=np.concatenate([[0], np.cumsum([len(p["obs"]) for p in P])]).astype(np.int32),
                  obs_kf=np.array([kf for p in P for kf, _ in p["obs"]], np.int32), obs_index=np.array([i for p in P for _, i in p["obs"]], np.int32),
                  current=self.current, last_level_scale=float(np.float32(1.2 ** 7)), first_connection=0, is_init_kf=0)
        pr.update(scalars)
        return dict(name=name, problem=pr, views=[v for v in views if v is not None], expect=dict(expect or {}))


def want_of(case):
    """the restatement's outputs for a case, computed once"""
    if "want" not in case:
        case["want"] = ref.process_new_keyframe(case["problem"], case["views"])
    return case["want"]


def rows_of(res, p):
    """the end-state observation row of point p as [(kf, index)]"""
    off = res["obs_offsets_out"]
    return [(int(k), int(i)) for k, i in zip(res["obs_kf_out"][off[p]:off[p + 1]], res["obs_index_out"][off[p]:off[p + 1]])]


def normal_f32(pos, centres):
    """MapPoint.cc:456-475, :501 in float32 for a point at pos seen from the centres, in that order"""
    f32 = np.float32
    n = [f32(0)] * 3
    for c in centres:
        v = [f32(pos[a]) - f32(c[a]) for a in range(3)]
        nr = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        n = [n[a] + v[a] / nr for a in range(3)]
    return np.array([n[a] / f32(len(centres)) for a in range(3)], f32)


# ---- hand-made cases ---------------------------------------------------------------------------------------------------------------------
def _with_keypoints(g, per_kf=10):
    for kf in range(g.n_kf):
        if kf not in g.slotless:
            for _ in range(per_kf):
                g.kp(kf, stereo=True)


def order_case(observed):
    """Rule 1: one point in slots 3 and 7.  Not yet observed: slot 3 associates it, slot 7 finds it in the keyframe and pushes it.  Observed
    (from slot 3): both slots push."""
    g = Graph(3, seed=21)
    _with_keypoints(g)
    p = g.pt(obs=[(1, 4), (2, 6)] + ([(0, 3)] if observed else []))
    g.hold(3, p); g.hold(7, p)
    if observed:
        expect = dict(associated_slot=[], associated_point=[], recent=[p, p], rows={p: [(0, 3), (1, 4), (2, 6)]}, nobs={p: 6}, refreshed=[])
    else:
        expect = dict(associated_slot=[3], associated_point=[p], recent=[p], rows={p: [(0, 3), (1, 4), (2, 6)]}, nobs={p: 6}, refreshed=[p])
    return g.finish("order_observed" if observed else "order", expect)


def in_case():
    """Rule 1: a point observed from the current keyframe at index 5 and held by slot 2 is "in": pushed, nothing changes."""
    g = Graph(2, seed=22)
    _with_keypoints(g)
    p = g.pt(obs=[(0, 5), (1, 1)])
    g.hold(2, p)
    return g.finish("in", dict(associated_slot=[], associated_point=[], recent=[p], rows={p: [(0, 5), (1, 1)]}, nobs={p: 4}, refreshed=[]))


def skips_case():
    """Rule 1: a NULL slot and a bad point are passed over (:329, :331); the point after them is associated."""
    g = Graph(2, seed=23)
    _with_keypoints(g)
    bad = g.pt(obs=[(1, 0)], bad=1)
    ok = g.pt(obs=[(1, 2)])
    g.hold(1, bad); g.hold(4, ok)     # slots 0, 2, 3 are NULL
    return g.finish("skips", dict(associated_slot=[4], associated_point=[ok], recent=[], rows={bad: [(1, 0)], ok: [(0, 4), (1, 2)]}, nobs={bad: 2, ok: 4},
                                  refreshed=[ok]))


def insert_case():
    """AddObservation puts the current keyframe's row (2) below, between and above the observers' rows."""
    g = Graph(5, current=2, seed=24)
    _with_keypoints(g)
    below = g.pt(obs=[(3, 1), (4, 1)])
    between = g.pt(obs=[(0, 2), (4, 2)])
    above = g.pt(obs=[(0, 3), (1, 3)])
    g.hold(6, below); g.hold(0, between); g.hold(9, above)
    return g.finish("insert", dict(associated_slot=[0, 6, 9], associated_point=[between, below, above], recent=[],
                                   rows={below: [(2, 6), (3, 1), (4, 1)], between: [(0, 2), (2, 0), (4, 2)], above: [(0, 3), (1, 3), (2, 9)]},
                                   nobs={below: 6, between: 6, above: 6}, refreshed=[below, between, above]))


def nobs_case():
    """MapPoint.cc:171-174: +2 for a slot with u_right >= 0, +1 for one without."""
    g = Graph(2, seed=25)
    for _ in range(4):
        g.kp(1)
    g.kp(0, stereo=True); g.kp(0, stereo=False)
    a = g.pt(obs=[(1, 0)], nobs=7)
    b = g.pt(obs=[(1, 1)], nobs=7)
    g.hold(0, a); g.hold(1, b)
    return g.finish("nobs", dict(associated_slot=[0, 1], associated_point=[a, b], recent=[], rows={a: [(0, 0), (1, 0)], b: [(0, 1), (1, 1)]}, nobs={a: 9, b: 8},
                                 refreshed=[a, b]))


def median_case(tie):
    """Rule 3 with N going from 2 to 3: the entry is index 1 of the sorted row.
    winner: rows C (current, row 0), A (row 1), B (row 2) with d(A, C) = 60, d(B, C) = 20, d(A, B) = 80: the medians are 20, 60, 20, so the
    new observation C wins as the first of the least -- with A and B alone both medians were 0 and A won.
    tie: current keyframe last (row 2), all three distances 40: every median is 40 and the first row, A, keeps it."""
    g = Graph(3, current=2 if tie else 0, seed=26)
    A = g.descriptor()
    if tie:
        B = mc.flip(A, 40, 0)
        Cd = mc.flip(mc.flip(A, 20, 0), 20, 100)
        ka, kb = g.kp(0, A), g.kp(1, B)
        rows = [(0, ka), (1, kb)]
    else:
        Cd = mc.flip(A, 60, 0)
        B = mc.flip(Cd, 20, 100)
        ka, kb = g.kp(1, A), g.kp(2, B)
        rows = [(1, ka), (2, kb)]
    p = g.pt(obs=rows)
    i = g.kp(g.current, Cd)
    g.hold(i, p)
    winner = (0, ka) if tie else (0, i)
    return g.finish("median_tie" if tie else "median_winner", dict(associated_slot=[i], associated_point=[p], recent=[], desc={p: winner}, refreshed=[p]))


def bad_observer_case():
    """Rules 2 and 3: a bad observer X (row 1) is left out of the descriptors and counted in the normal.  d(C, X) = 50, d(X, B) = 10,
    d(C, B) = 60: with X the medians would be 50, 10, 10 and X would win; without it N = 2, both medians are 0 and C (row 0) wins."""
    g = Graph(3, seed=27)
    Cd = g.descriptor()
    X = mc.flip(Cd, 50, 0)
    B = mc.flip(X, 10, 100)
    kx, kb = g.kp(1, X), g.kp(2, B)
    g.kf_flags[1] = 1
    p = g.pt(obs=[(1, kx), (2, kb)], ref_kf=2)
    i = g.kp(0, Cd)
    g.hold(i, p)
    normal = normal_f32(g.points[p]["pos"], g.centres[[0, 1, 2]])
    assert not np.array_equal(normal, normal_f32(g.points[p]["pos"], g.centres[[0, 2]]))
    return g.finish("bad_observer", dict(associated_slot=[i], associated_point=[p], recent=[], desc={p: (0, i)}, normal={p: normal}, refreshed=[p]))


def first_observation_case():
    """a point with no observation before the call: N = 1, its descriptor is the slot's, its normal the unit vector from the current centre"""
    g = Graph(2, seed=28)
    _with_keypoints(g, 3)
    p = g.pt(obs=[], ref_kf=0, nobs=0)
    g.hold(1, p)
    return g.finish("first_observation", dict(associated_slot=[1], associated_point=[p], recent=[], rows={p: [(0, 1)]}, nobs={p: 2}, desc={p: (0, 1)},
                                              normal={p: normal_f32(g.points[p]["pos"], g.centres[[0]])}, refreshed=[p]))


def threshold_case():
    """Rule 4 (see the module's note): keyframe 1 shares exactly 15 points with the current keyframe, keyframe 2 exactly 14.  Fourteen of the
    fifteen are observed from the current keyframe on entry, the fifteenth (and two of keyframe 2's) gain their observation in this call."""
    g = Graph(4, seed=29)
    k1 = [g.kp(1) for _ in range(15)]
    k2 = [g.kp(2) for _ in range(14)]
    assoc = []
    for j in range(15):
        i = g.kp(0)
        entry = j < 14
        p = g.pt(obs=[(1, k1[j])] + ([(2, k2[j])] if j < 14 else []) + ([(0, i)] if entry and j >= 2 else []))
        g.hold(i, p)
        if not (entry and j >= 2):
            assoc.append((i, p))
    g.conn[1] = {3: 20}
    g.conn[2] = {0: 9}
    return g.finish("threshold", dict(associated_slot=[i for i, _ in assoc], associated_point=[p for _, p in assoc],
                                      conn=dict(status=UPDATED, counter_kf=[1, 2], counter_weight=[15, 14], ordered_kf=[1], ordered_weight=[15], touched_kf=[1],
                                                touched_changed=[1], changed_kf=[3, 0], changed_weight=[20, 15], parent=1)), first_connection=1)


def nobody_reaches_15_case():
    """KeyFrame.cc:455-459: keyframes 1 and 2 share 3 points each, nobody reaches 15: the best alone, the lowest row among equals."""
    g = Graph(3, seed=30)
    _with_keypoints(g, 4)
    for j in range(3):
        g.hold(j, g.pt(obs=[(1, j), (2, j)]))
    return g.finish("nobody_reaches_15", dict(associated_slot=[0, 1, 2], associated_point=[0, 1, 2],
                                              conn=dict(status=UPDATED, counter_kf=[1, 2], counter_weight=[3, 3], ordered_kf=[1], ordered_weight=[3], touched_kf=[1],
                                                        touched_changed=[1], changed_kf=[0], changed_weight=[3], parent=-1)))


def only_nulls_case():
    """a slot row of NULLs: nothing associated, KFcounter empty (KeyFrame.cc:426-427)"""
    g = Graph(2, seed=31)
    _with_keypoints(g, 5)
    g.pt(obs=[(1, 0)])
    return g.finish("only_nulls", dict(associated_slot=[], associated_point=[], recent=[], refreshed=[], conn=dict(status=UNCHANGED, parent=-1)))


def hand_made():
    if "hand" not in _cache:
        _cache["hand"] = [order_case(False), order_case(True), in_case(), skips_case(), insert_case(), nobs_case(), median_case(False), median_case(True),
                          bad_observer_case(), first_observation_case(), threshold_case(), nobody_reaches_15_case(), only_nulls_case()]
    return _cache["hand"]


# ---- the limits ----------------------------------------------------------------------------------------------------------------------------
def the_limit_case(limit=112):
    """a point at `limit` observations that gains one: past what a wavefront's descriptor rows hold, the host twin finishes the problem.  A
    second point beside it stays small."""
    if "limit" not in _cache:
        g = Graph(limit + 1, seed=32)
        for kf in range(1, limit + 1):
            g.kp(kf)
        g.kp(0); g.kp(0)
        big = g.pt(obs=[(kf, 0) for kf in range(1, limit + 1)])
        small = g.pt(obs=[(3, 0)])
        g.hold(0, big); g.hold(1, small)
        _cache["limit"] = g.finish("limit", dict(associated_slot=[0, 1], associated_point=[big, small], recent=[]))
    return _cache["limit"]


def the_many_rows_case(lds_keyframes=2048, lds_points=16384):
    """one keyframe more than the connection kernel's LDS counters hold and one point more than the neighbours entry's LDS marks hold: the
    per-point marks of this entry are words in global memory, so the device computes the problem.  Most rows observe nothing and name no slot."""
    if "many" not in _cache:
        n_kf = lds_keyframes + 1
        live = (0, 1, 2, n_kf - 1)
        g = Graph(n_kf, seed=33, slotless=[k for k in range(n_kf) if k not in live])
        for kf in live:
            for _ in range(6):
                g.kp(kf)
        for j in range(5):
            g.hold(j, g.pt(obs=[(1, j), (n_kf - 1, j)] + ([(2, j)] if j % 2 else [])))
        rng = np.random.default_rng(34)
        for _ in range(lds_points + 1 - len(g.points)):           # the rest are in no slot of the current keyframe
            g.points.append(dict(obs=[(int(rng.integers(3, n_kf - 1)), 0)], bad=0, nobs=2, ref_kf=0, ref_scale=1.0, pos=np.float32([0, 0, 9])))
        last = len(g.points) - 1
        g.points[last]["obs"] = [(1, 5)]
        g.hold(5, last)                                           # the last point row is used
        g.conn[n_kf - 1] = {0: 3, 7: 2}
        _cache["many"] = g.finish("many_rows", dict(associated_slot=[0, 1, 2, 3, 4, 5], associated_point=[0, 1, 2, 3, 4, last], recent=[]))
    return _cache["many"]


# ---- random graphs ---------------------------------------------------------------------------------------------------------------------------
def random_case(seed):
    rng = np.random.default_rng(1000 + seed)
    n_kf = int(rng.integers(4, 24))
    cur = int(rng.integers(0, n_kf))
    g = Graph(n_kf, current=cur, seed=seed)
    n_keys = [int(rng.integers(20, 70)) for _ in range(n_kf)]
    n_keys[cur] = int(rng.integers(40, 300))      # more than one chunk of 256 slots at times
    bases = [g.descriptor() for _ in range(6)]    # descriptors near a few bases: medians tie often
    for kf in range(n_kf):
        for _ in range(n_keys[kf]):
            g.kp(kf, mc.flip(bases[int(rng.integers(6))], int(rng.integers(0, 12)), int(rng.integers(0, 200))), stereo=bool(rng.random() < 0.7))
    g.kf_flags[:] = (rng.random(n_kf) < 0.15) * 1 + (rng.random(n_kf) < 0.1) * 2
    g.kf_flags[cur] = 0
    free = list(rng.permutation(n_keys[cur]))
    others = [k for k in range(n_kf) if k != cur]
    for _ in range(int(0.6 * n_keys[cur])):
        seen_by = [int(k) for k in rng.choice(others, int(rng.integers(0, min(len(others), 9) + 1)), replace=False)]
        obs = [(k, int(rng.integers(n_keys[k]))) for k in seen_by]
        i = int(free.pop())
        kind = rng.random()
        if kind < 0.25:
            obs.append((cur, i))                                  # observed on entry from its own slot
        elif kind < 0.3:
            obs.append((cur, int(rng.integers(n_keys[cur]))))     # observed on entry from some index
        p = g.pt(obs=obs, bad=int(rng.random() < 0.1), ref_kf=int(rng.integers(n_kf)), ref_scale=float(np.float32(1.2 ** int(rng.integers(0, 8)))),
                 nobs=int(rng.integers(0, 30)))
        g.hold(i, p)
        if rng.random() < 0.12 and free:
            g.hold(int(free.pop()), p)                            # a second slot holds the same point
    for _ in range(5):                                            # points that no slot holds
        g.pt(obs=[(int(rng.integers(n_kf)), 0)])
    for k in others:                                              # weight rows: some hold the current keyframe already
        row = {int(j): int(rng.integers(1, 40)) for j in rng.choice(n_kf, int(rng.integers(0, min(n_kf, 6))), replace=False) if int(j) != k}
        g.conn[k] = row
    return g.finish("random_%d" % seed, first_connection=int(seed % 2), is_init_kf=int(seed % 5 == 0))


def random_cases(n=8):
    if "random" not in _cache:
        _cache["random"] = [random_case(s) for s in range(n)]
    return _cache["random"]


def all_cases():
    return hand_made() + random_cases() + [the_limit_case(), the_many_rows_case()]


def on_one_store(cases):
    """every case's keyframes side by side -> (views, problems with kf_slot moved to the case's first slot)"""
    views, problems = [], []
    for c in cases:
        pr = dict(c["problem"])
        slot = np.asarray(pr["kf_slot"])
        pr["kf_slot"] = np.where(slot >= 0, slot + len(views), -1).astype(np.int32)
        views += c["views"]
        problems.append(pr)
    return views, problems
