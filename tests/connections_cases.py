"""Problems for the covisibility tests: a generator of graphs around one keyframe, a builder for hand-made graphs of a few keyframes, and the
comparison (everything is an integer: equality)."""
import numpy as np

OUTPUTS = ("status", "parent", "counter_kf", "counter_weight", "ordered_kf", "ordered_weight", "touched_kf", "touched_changed", "changed_offsets",
           "changed_kf", "changed_weight")
ROW_LENS = (0, 1, 63, 64, 65, 255, 257, 1100)      # entries of a touched keyframe's row: around the widths of a wavefront and a workgroup


def make_problem(seed, n_kf, n_slots, n_seen, votes="mixed", row_lens=(3, 17, 40), weights=None, first=False, init=False, special=True):
    """One UpdateConnections call.  n_kf keyframes, one of them the current one; n_seen of the others observe its points: keyframe k sees a
    point with probability q_k (votes: "high" 0.3 for all, "low" 0.004, "mixed" drawn from {0.004, 0.02, 0.2, 0.6}), so that counts land on
    both sides of 15.  The current keyframe has n_slots slots: mostly distinct points, some NULL, some points twice, some bad points.
    special: a few bad keyframes and keyframes of another map among the observers.  Every observer has a weight row whose length cycles
    through row_lens (cut to the keyframes there are), with weights from `weights` (default 1..200); half of the rows hold the current
    keyframe, half of those with the weight this call will give it (AddConnection then changes nothing)."""
    rng = np.random.default_rng(seed)
    cur = int(rng.integers(0, n_kf))
    others = np.array([k for k in range(n_kf) if k != cur], np.int64)
    seen = np.sort(rng.choice(others, min(n_seen, len(others)), replace=False)) if len(others) else others
    flags = np.zeros(n_kf, np.uint8)
    if special and n_kf > 8:
        flags[rng.choice(n_kf, max(1, n_kf // 20), replace=False)] |= 1
        flags[rng.choice(n_kf, max(1, n_kf // 30), replace=False)] |= 2
        flags[cur] = 0
    n_points = max(1, n_slots)
    q = {"high": np.full(len(seen), 0.3), "low": np.full(len(seen), 0.004), "mixed": rng.choice([0.004, 0.02, 0.2, 0.6], len(seen))}[votes]
    sees = rng.random((n_points, len(seen))) < q[None, :]
    obs_offsets, obs_kf = [0], []
    for p in range(n_points):
        row = np.r_[seen[sees[p]], cur] if rng.random() < 0.9 else seen[sees[p]]     # the current keyframe observes its own points
        obs_kf.append(rng.permutation(row))                                          # GetObservations(): any order
        obs_offsets.append(obs_offsets[-1] + len(row))
    obs_kf = np.concatenate(obs_kf).astype(np.int32) if obs_kf else np.zeros(0, np.int32)
    point_bad = (rng.random(n_points) < 0.03).astype(np.uint8)
    slot_point = rng.permutation(n_points)[:n_slots].astype(np.int32) if n_slots else np.zeros(0, np.int32)
    if n_slots > 4:
        k = max(1, n_slots // 10)
        slot_point[rng.choice(n_slots, k, replace=False)] = -1                       # NULL slots
        slot_point[rng.choice(n_slots, k, replace=False)] = slot_point[rng.choice(n_slots, k, replace=False)]   # points held twice
    # the counts this call will find, to plant rows that hold them already
    count = np.zeros(n_kf, np.int64)
    for p in slot_point:
        if p >= 0 and not point_bad[p]:
            np.add.at(count, obs_kf[obs_offsets[p]:obs_offsets[p + 1]], 1)
    conn_offsets, conn_kf, conn_weight = [0], [], []
    lens = {int(k): min(row_lens[i % len(row_lens)], len(others) - 1) for i, k in enumerate(seen)}
    for k in range(n_kf):
        if k in lens:
            pool = others[others != k]
            row = rng.choice(pool, max(lens[k], 0), replace=False) if lens[k] > 0 else np.zeros(0, np.int64)
            mode = rng.integers(0, 4)                                                # 0, 1: without the current keyframe
            if mode >= 2 and lens[k] > 0:
                row[0] = cur
            row = np.sort(row)
            w = rng.choice(weights, len(row)) if weights is not None else rng.integers(1, 201, len(row))
            if mode == 3 and lens[k] > 0:
                w[row == cur] = count[k]
            conn_kf.append(row)
            conn_weight.append(w)
            conn_offsets.append(conn_offsets[-1] + len(row))
        else:
            conn_offsets.append(conn_offsets[-1])
    cat = lambda v: np.concatenate(v).astype(np.int32) if v else np.zeros(0, np.int32)
    return dict(kf_flags=flags, conn_offsets=np.array(conn_offsets, np.int32), conn_kf=cat(conn_kf), conn_weight=cat(conn_weight), current=cur,
                slot_point=slot_point, point_bad=point_bad, obs_offsets=np.array(obs_offsets, np.int32), obs_kf=obs_kf,
                first_connection=int(first), is_init_kf=int(init))


def family(lds_keyframes):
    """About 40 graphs at the smallest sizes where the kernels change path: n_keyframes from 1 to 3000 with both sides of lds_keyframes (the
    vote counters leave LDS), slot counts 0, 1, 63, 64, 65 and 2000, touched rows of ROW_LENS entries, weights with heavy ties, more than 256
    keyframes over the threshold, and lists of 63 / 64 / 65 / 255 / 257 entries for the current keyframe itself."""
    L = lds_keyframes
    spec = [  # n_kf, n_slots, n_seen, votes, row_lens, weights, first, init
        (1, 10, 0, "mixed", (3,), None, True, False), (2, 30, 1, "high", (1,), None, True, False), (2, 3, 1, "high", (0,), None, False, False),
        (5, 0, 4, "high", (2,), None, True, False), (5, 1, 4, "high", (3,), None, True, True), (12, 63, 8, "mixed", (0, 1, 5), None, False, True),
        (40, 64, 30, "mixed", (3, 17), None, True, False), (40, 65, 30, "mixed", (3, 17), (5, 15, 40), False, False),
        (40, 300, 30, "low", (3, 17), None, True, False), (90, 400, 60, "low", (5,), None, False, False),
        (200, 2000, 120, "mixed", (40, 63, 64, 65), (14, 15, 16), True, False), (200, 1000, 100, "mixed", (100,), None, False, False),
        (300, 500, 63, "high", (20,), None, True, False, False), (300, 500, 64, "high", (20,), (7, 8, 9), False, False, False),
        (300, 500, 65, "high", (20,), None, True, False, False), (600, 500, 255, "high", (10,), None, False, False, False),
        (600, 500, 257, "high", (10,), (1, 2, 3), True, False, False), (1300, 1000, 9, "high", ROW_LENS, None, True, False, False),
        (1300, 1000, 16, "high", ROW_LENS, (20, 30, 40), False, False, False), (1500, 300, 40, "mixed", (255, 257, 1100), None, True, False),
        (L - 1, 200, 50, "mixed", (30,), None, True, False), (L, 200, 50, "mixed", (30,), None, False, False),
        (L + 1, 200, 50, "mixed", (30,), None, True, False), (L + 1, 64, 400, "high", (4,), None, False, True),
        (3000, 2000, 120, "mixed", (50,), None, True, False), (3000, 400, 700, "high", (6,), (2, 4, 8), False, False),
        (L, 300, 600, "high", (5,), None, True, False), (3000, 0, 10, "high", (5,), None, True, False),
        (3000, 100, 40, "low", (5, 64), None, True, False), (L + 1, 100, 40, "low", (5, 64), (9, 10, 11), False, False),
        (64, 500, 63, "mixed", (62,), (3, 4, 5), True, False), (65, 500, 64, "mixed", (63,), None, False, False),
        (257, 700, 256, "mixed", (255,), (1, 2, 3), True, False), (100, 1000, 99, "mixed", (98,), None, True, True),
        (30, 65, 20, "low", (3,), None, True, True), (30, 64, 20, "low", (3,), None, False, True),
        (700, 1000, 300, "high", (0, 1), None, True, False), (50, 2000, 40, "high", (45,), (15,), False, False),
        (50, 500, 49, "mixed", (48,), None, True, False, False), (1000, 1000, 80, "mixed", (20, 90), None, True, False)]
    out = []
    for i, s in enumerate(spec):
        out.append(make_problem(100 + i, s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], special=s[8] if len(s) > 8 else True))
    return out


def workload(seed):
    """A problem of the workload's own shape: about 1 000 slots, 10-20 observations per point, 40-120 counted keyframes."""
    rng = np.random.default_rng(seed)
    n_seen = int(rng.integers(40, 121))
    pr = make_problem(seed, n_seen + 40, 1000, n_seen, "mixed", (30, 60, 90), None, first=bool(seed % 2))
    return pr


def hand(kfs, points, slots, current, **scalars):
    """A hand-made graph.  kfs: dicts with optionally flags and conn = {keyframe: weight}; points: dicts with obs = [keyframes] and
    optionally bad; slots: the points of the current keyframe's slots (-1 = NULL)."""
    co = np.cumsum([0] + [len(k.get("conn", {})) for k in kfs])
    oo = np.cumsum([0] + [len(p.get("obs", [])) for p in points])
    pr = dict(kf_flags=np.array([k.get("flags", 0) for k in kfs], np.uint8), conn_offsets=co.astype(np.int32),
              conn_kf=np.array([c for k in kfs for c in sorted(k.get("conn", {}))], np.int32),
              conn_weight=np.array([k["conn"][c] for k in kfs for c in sorted(k.get("conn", {}))], np.int32), current=current,
              slot_point=np.array(slots, np.int32), point_bad=np.array([p.get("bad", 0) for p in points], np.uint8), obs_offsets=oo.astype(np.int32),
              obs_kf=np.array([o for p in points for o in p.get("obs", [])], np.int32), first_connection=0, is_init_kf=0)
    pr.update(scalars)
    return pr


def votes(n_kf, current, counts):
    """kfs, points, slots of a graph in which keyframe k gets counts[k] votes: point i is seen by every keyframe with counts[k] > i"""
    n = max(list(counts.values()) + [0])
    points = [dict(obs=[current] + [k for k in sorted(counts) if counts[k] > i]) for i in range(n)]
    return [dict() for _ in range(n_kf)], points, list(range(n))


def random_rows(seed, n_rows, n_kf, long_rows=(63, 64, 65, 255, 257, 1100)):
    """Weight rows of mixed length for UpdateBestCovisibles: mostly 0-20 entries, a few long ones, weights with many ties, 10 % bad."""
    rng = np.random.default_rng(seed)
    lens = rng.integers(0, 21, n_rows)
    lens[rng.choice(n_rows, len(long_rows), replace=False)] = long_rows
    off = np.r_[0, np.cumsum(lens)].astype(np.int32)
    # strictly ascending rows: a random start and positive steps
    steps = rng.integers(1, max(2, n_kf // 1200), int(off[-1]))
    kf = np.zeros(int(off[-1]), np.int64)
    for r in np.flatnonzero(lens):
        s = slice(off[r], off[r + 1])
        c = np.cumsum(steps[s])
        kf[s] = c - c[0] + rng.integers(0, n_kf - (c[-1] - c[0]))
    return dict(offsets=off, kf=kf.astype(np.int32), weight=rng.integers(1, 30, len(kf)).astype(np.int32)), (rng.random(n_kf) < 0.1).astype(np.uint8)


def assert_equal(got, want, what=""):
    for k in OUTPUTS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, got[k], want[k])
