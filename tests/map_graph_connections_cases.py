"""Cases for the covisibility graph on the resident map graph: the problems of tests/connections_cases.py turned into graph tables plus
connection tables, the directed cases, and the restatements the device entries and the host twins are held against -- the result of
tests/connections_ref.py written into the tables, and KeyFrame::SetBadFlag's covisibility part (SF/src/KeyFrame.cc:600-603, :617-618,
:699-713).  Everything is an integer: the criterion is equality."""
import numpy as np

import connections_cases as C
import connections_ref as ref

ARRAYS = ("conn_offsets", "conn_kf", "conn_weight", "ord_offsets", "ord_kf", "ord_weight")
KF_ID0 = 100                               # kf_id of row 0; the ids ascend with the rows
POSE7 = np.array([0, 0, 0, 1, 0, 0, 0], np.float64)


def rows_of(c):
    """connection tables -> (weights: per row a dict keyframe -> weight, ordered: per row (keyframes, weights) as lists)"""
    co, oo = c["conn_offsets"], c["ord_offsets"]
    w = [dict(zip(c["conn_kf"][co[k]:co[k + 1]].tolist(), c["conn_weight"][co[k]:co[k + 1]].tolist())) for k in range(len(co) - 1)]
    o = [(c["ord_kf"][oo[k]:oo[k + 1]].tolist(), c["ord_weight"][oo[k]:oo[k + 1]].tolist()) for k in range(len(oo) - 1)]
    return w, o


def tables_of(weights, ordered):
    i32 = lambda v: np.array(v, np.int32).reshape(-1)
    return dict(conn_offsets=i32(np.cumsum([0] + [len(w) for w in weights])), conn_kf=i32([k for w in weights for k in sorted(w)]),
                conn_weight=i32([w[k] for w in weights for k in sorted(w)]), ord_offsets=i32(np.cumsum([0] + [len(o[0]) for o in ordered])),
                ord_kf=i32([k for o in ordered for k in o[0]]), ord_weight=i32([x for o in ordered for x in o[1]]))


def graph_of(pr, seed=0, kf_slot=0, stale=3, ordered=None):
    """A problem of connections_cases as (graph tables, connection tables, init_kf_id).  Only the current keyframe has slots; point_flags
    carry further bits beside bit 0, which alone means bad; the observation rows ascend by keyframe as the graph wants them (votes do not
    depend on their order).  The ordered rows are UpdateBestCovisibles of the weight rows, except every `stale`-th non-empty one, which
    is left reversed and short of its last entry -- the reference leaves such lists -- and those given in `ordered` {row: (kfs, weights)}."""
    rng = np.random.default_rng(seed)
    nk, npts, cur = len(pr["kf_flags"]), len(pr["point_bad"]), int(pr["current"])
    oo = np.asarray(pr["obs_offsets"])
    obs_kf = np.concatenate([np.sort(pr["obs_kf"][oo[p]:oo[p + 1]]) for p in range(npts)] + [np.zeros(0, np.int32)]).astype(np.int32)
    for p in range(npts):
        assert len(set(obs_kf[oo[p]:oo[p + 1]].tolist())) == oo[p + 1] - oo[p]
    slot_offsets = np.zeros(nk + 1, np.int32)
    slot_offsets[cur + 1:] = len(pr["slot_point"])
    flags = (np.asarray(pr["point_bad"], np.uint8) != 0).astype(np.uint8) | (rng.integers(0, 2, npts).astype(np.uint8) << 1)
    g = dict(kf_slot=np.full(nk, kf_slot, np.int32), kf_id=KF_ID0 + np.arange(nk, dtype=np.int64), kf_flags=np.asarray(pr["kf_flags"], np.uint8),
             poses7=np.tile(POSE7, (nk, 1)), slot_offsets=slot_offsets, slot_point=np.asarray(pr["slot_point"], np.int32), point_flags=flags,
             positions=np.zeros((npts, 3)), obs_offsets=oo.astype(np.int32), obs_kf=obs_kf, obs_index=np.full(len(obs_kf), -1, np.int32))
    bad = [int(f) & 1 for f in pr["kf_flags"]]
    co = pr["conn_offsets"]
    weights = [dict(zip(pr["conn_kf"][co[k]:co[k + 1]].tolist(), pr["conn_weight"][co[k]:co[k + 1]].tolist())) for k in range(nk)]
    lists, n = [], 0
    for k in range(nk):
        kfs, ws = ref.best_covisibles(weights[k], bad)
        if kfs:
            n += 1
            if stale and n % stale == 0:
                kfs, ws = kfs[::-1][:-1], ws[::-1][:-1]
        lists.append((kfs, ws))
    for k, v in (ordered or {}).items():
        lists[k] = (list(v[0]), list(v[1]))
    return g, tables_of(weights, lists), (KF_ID0 + cur if pr.get("is_init_kf", 0) else -1)


def problem_of(g, c, current, first_connection, init_kf_id):
    """The tc2li_connections_problem that a call on the graph stands for (the table of the header)."""
    so = g["slot_offsets"]
    return dict(kf_flags=g["kf_flags"], conn_offsets=c["conn_offsets"], conn_kf=c["conn_kf"], conn_weight=c["conn_weight"], current=int(current),
                slot_point=g["slot_point"][so[current]:so[current + 1]], point_bad=(g["point_flags"] & 1).astype(np.uint8),
                obs_offsets=g["obs_offsets"], obs_kf=g["obs_kf"], first_connection=int(first_connection),
                is_init_kf=int(int(g["kf_id"][current]) == int(init_kf_id)))


def with_rows(c, n_rows):
    """the tables with the empty rows of keyframes appended since"""
    add = n_rows - (len(c["conn_offsets"]) - 1)
    assert add >= 0
    return dict(c, conn_offsets=np.r_[c["conn_offsets"], np.full(add, c["conn_offsets"][-1])].astype(np.int32),
                ord_offsets=np.r_[c["ord_offsets"], np.full(add, c["ord_offsets"][-1])].astype(np.int32))


def counts_of(res):
    """the counts block of a result of connections_ref.update_connections"""
    if res["status"] == ref.UNCHANGED:
        return np.array([0, 0, 0, 0, 0, -1, 0, 0], np.int32)
    return np.array([1, len(res["counter_kf"]), len(res["ordered_kf"]), int(res["touched_changed"].sum()), len(res["changed_kf"]), res["parent"], 0, 0], np.int32)


def updated(c, pr, res):
    """The resident effect of an update: the result `res` of the call `pr` (in the shape of tc2li_update_connections_batch) written into
    the connection tables c, as the issue of the resident form states it."""
    if res["status"] == ref.UNCHANGED:
        return {k: np.array(c[k], np.int32) for k in ARRAYS}
    weights, lists = rows_of(c)
    cur = int(pr["current"])
    counter = dict(zip(np.asarray(res["counter_kf"]).tolist(), np.asarray(res["counter_weight"]).tolist()))
    weights[cur] = dict(counter)                                                     # :473
    lists[cur] = (np.asarray(res["ordered_kf"]).tolist(), np.asarray(res["ordered_weight"]).tolist())   # :474-475
    off, n = res["changed_offsets"], 0
    for k, changed in zip(np.asarray(res["touched_kf"]).tolist(), np.asarray(res["touched_changed"]).tolist()):
        weights[k][cur] = counter[k]                                                 # :207, :209
        if changed:                                                                  # :213
            lists[k] = (res["changed_kf"][off[n]:off[n + 1]].tolist(), res["changed_weight"][off[n]:off[n + 1]].tolist())
            n += 1
    return tables_of(weights, lists)


def update_ref(g, c, current, first_connection, init_kf_id):
    """-> (counts block, tables after) by tests/connections_ref.py"""
    c = with_rows(c, len(g["kf_flags"]))
    pr = problem_of(g, c, current, first_connection, init_kf_id)
    res = ref.update_connections(pr)
    return counts_of(res), updated(c, pr, res)


def erased(g, c, row):
    """KeyFrame::SetBadFlag on covisibility, restated: for every keyframe of the row's weights EraseConnection (:600-603 -> :699-713: the
    entry goes if it is there, and only then UpdateBestCovisibles with the flags as they are), then both rows of the keyframe are emptied
    (:617-618)."""
    c = with_rows(c, len(g["kf_flags"]))
    weights, lists = rows_of(c)
    bad = [int(f) & 1 for f in g["kf_flags"]]
    for k in sorted(weights[row]):
        if row in weights[k]:
            del weights[k][row]
            lists[k] = ref.best_covisibles(weights[k], bad)
    weights[row], lists[row] = {}, ([], [])
    return tables_of(weights, lists)


def assert_same(got, want, what=""):
    for k in ARRAYS:
        assert np.array_equal(np.asarray(got[k]), np.asarray(want[k])), (what, k, got[k], want[k])


def directed():
    """-> [(name, problem, ordered rows given, check of the reference's result)]: the cases the issue lists"""
    out = []

    def case(name, pr, ordered=None, check=None):
        out.append((name, pr, ordered, check))

    kfs, points, slots = C.votes(4, 0, {})
    case("an empty counter", C.hand(kfs, [dict(obs=[0]), dict(obs=[0, 1], bad=1)], [0, 1, -1], 0, first_connection=1),
         check=lambda r: r["status"] == ref.UNCHANGED)
    kfs, points, slots = C.votes(5, 2, {1: 7, 3: 7, 4: 5})
    case("nobody reaches 15: the lone best, the lowest row among equals", C.hand(kfs, points, slots, 2, first_connection=1),
         check=lambda r: r["by_max"] and r["ordered_kf"].tolist() == [1] and r["parent"] == 1 and r["counter_kf"].tolist() == [1, 3, 4])
    kfs, points, slots = C.votes(3, 0, {1: 8, 2: 7})
    case("a point in two slots votes twice", C.hand(kfs, points, slots + slots, 0),
         check=lambda r: not r["by_max"] and r["ordered_kf"].tolist() == [1] and r["counter_weight"].tolist() == [16, 14])
    kfs, points, slots = C.votes(5, 0, {1: 20, 2: 30, 3: 40, 4: 16})
    kfs[2]["flags"], kfs[3]["flags"] = 1, 2
    case("a bad voter and an other-map voter", C.hand(kfs, points, slots, 0), check=lambda r: r["counter_kf"].tolist() == [1, 4])
    kfs, points, slots = C.votes(5, 1, {0: 20, 2: 17, 3: 3})
    kfs[0]["conn"] = {1: 20, 3: 9, 4: 11}
    kfs[2]["conn"] = {1: 16, 4: 2}
    case("a neighbour holds (current, same weight) and keeps its stale list; another holds a different weight", C.hand(kfs, points, slots, 1),
         ordered={0: ([3, 1], [9, 2])}, check=lambda r: r["touched_kf"].tolist() == [0, 2] and r["touched_changed"].tolist() == [0, 1])
    kfs, points, slots = C.votes(6, 5, {0: 15, 1: 15})
    kfs[0]["conn"] = {2: 40, 3: 40, 4: 1}
    kfs[3]["flags"] = 1
    case("a bad keyframe inside a neighbour's weight row", C.hand(kfs, points, slots, 5),
         check=lambda r: r["changed_kf"][:r["changed_offsets"][1]].tolist() == [2, 5, 4])
    kfs, points, slots = C.votes(3, 1, {0: 15, 2: 16})
    for first in (1, 0):
        case("current is the init keyframe, first_connection %d" % first, C.hand(kfs, points, slots, 1, first_connection=first, is_init_kf=1),
             check=lambda r: r["parent"] == -1)
    case("first_connection, not the init keyframe", C.hand(kfs, points, slots, 1, first_connection=1), check=lambda r: r["parent"] == 2)
    # every other keyframe in the neighbour's row already: full up to one entry, then the insert
    n = 70
    kfs, points, slots = C.votes(n, 7, {3: 15})
    kfs[3]["conn"] = {k: 1 + k % 5 for k in range(n) if k not in (3, 7)}
    case("a neighbour's row full up to one entry, plus the insert", C.hand(kfs, points, slots, 7),
         check=lambda r: r["changed_offsets"].tolist() == [0, n - 1])
    return out


def erase_cases(lds_row):
    """-> [(name, problem whose weights are made symmetric where the case wants it, row to erase, ordered rows given)]"""
    out = []
    for n_nb in (0, 1, 65, lds_row + 1):
        n = n_nb + 6
        kfs = [dict(conn={}) for _ in range(n)]
        nbs = list(range(2, 2 + n_nb))
        for k in nbs:
            kfs[1]["conn"][k] = 10 + k % 7
            kfs[k]["conn"] = {1: 10 + k % 7, 0: 3 + k % 4, n - 1: 3 + k % 4}
        if n_nb >= 65:
            kfs[nbs[0]]["conn"] = {k: 5 + k % 3 for k in range(n) if k != nbs[0]}          # a long list, ties in it
            del kfs[nbs[1]]["conn"][1]                                                   # a neighbour that does not hold the entry
            kfs[n - 1]["flags"] = 1                                                      # another bad keyframe in the neighbours' lists
        pr = C.hand(kfs, [dict(obs=[0])], [0], 1)
        ordered = {nbs[1]: ([0], [77])} if n_nb >= 65 else None                          # ... and its deliberately odd list stays
        out.append(("%d neighbours" % n_nb, pr, 1, ordered))
    return out
