"""KeyFrame::UpdateConnections, AddConnection and UpdateBestCovisibles restated in Python from the reference's source, the checker of
tests/test_connections.py and tests/test_connections_gpu.py.  Line numbers are SF/src/KeyFrame.cc (:201-238, :391-486).  A problem is the
dict of arrays that tc2li_connections_problem describes (include/tc2li_hip.h "local mapping: covisibility graph").

The restatement keeps the objects' behaviour, not their layout: a keyframe's weights are a dict keyframe -> weight as
mConnectedKeyFrameWeights is a map, KFcounter a dict, vPairs a list of (weight, keyframe) tuples that sorted() orders as std::sort orders
pair<int, KeyFrame*>.  Row numbers stand for the addresses: iterating a map is iterating its keys in ascending order."""
import numpy as np

UNCHANGED, UPDATED = 0, 1
TH = 15                                   # :433


def best_covisibles(weights, bad):
    """UpdateBestCovisibles (:216-238) on a dict keyframe -> weight -> (keyframes, weights)"""
    pairs = sorted((w, kf) for kf, w in weights.items())                             # :221-224
    kfs, ws = [], []
    for w, kf in pairs:
        if not bad[kf]:                                                              # :229
            kfs.insert(0, kf)                                                        # :231-232 push_front
            ws.insert(0, w)
    return kfs, ws


def update_connections(pr):
    """-> the outputs of tc2li_update_connections_batch as a dict (status, parent, counter_kf, counter_weight, ordered_kf, ordered_weight,
    touched_kf, touched_changed, changed_offsets, changed_kf, changed_weight) and, for the tests' own bookkeeping, by_max (connected by the
    rule of :455-459) and n_unchanged (touched keyframes where AddConnection returned at :210)."""
    flags = [int(v) for v in pr["kf_flags"]]
    co, ck, cw = ([int(v) for v in pr[k]] for k in ("conn_offsets", "conn_kf", "conn_weight"))
    oo, ok = [int(v) for v in pr["obs_offsets"]], [int(v) for v in pr["obs_kf"]]
    point_bad = [int(v) for v in pr["point_bad"]]
    cur = int(pr["current"])
    bad = [f & 1 for f in flags]
    i32 = lambda v: np.array(v, np.int32)
    counter = {}
    for p in (int(v) for v in pr["slot_point"]):                                     # :404
        if p < 0:                                                                    # :408
            continue
        if point_bad[p]:                                                             # :411
            continue
        for kf in ok[oo[p]:oo[p + 1]]:                                               # :416
            if kf == cur or flags[kf] & 1 or flags[kf] & 2:                          # :418
                continue
            counter[kf] = counter.get(kf, 0) + 1                                     # :420
    empty = dict(status=UNCHANGED, parent=-1, changed_offsets=i32([0]), touched_changed=np.zeros(0, np.uint8), by_max=False, n_unchanged=0)
    if not counter:                                                                  # :426-427
        return dict(empty, **{k: i32([]) for k in ("counter_kf", "counter_weight", "ordered_kf", "ordered_weight", "touched_kf", "changed_kf", "changed_weight")})
    nmax, kf_max, pairs, touched = 0, None, [], []
    for kf in sorted(counter):                                                       # :439 in map order
        if counter[kf] > nmax:                                                       # :443
            nmax, kf_max = counter[kf], kf
        if counter[kf] >= TH:                                                        # :448
            pairs.append((counter[kf], kf))
            touched.append(kf)                                                       # :451
    by_max = not pairs
    if by_max:                                                                       # :455-459
        pairs.append((nmax, kf_max))
        touched.append(kf_max)
    pairs.sort()                                                                     # :461
    ordered_kf, ordered_weight = [], []
    for w, kf in pairs:                                                              # :464-468 push_front
        ordered_kf.insert(0, kf)
        ordered_weight.insert(0, w)
    parent = ordered_kf[0] if pr.get("first_connection", 0) and not pr.get("is_init_kf", 0) else -1    # :478-483
    changed, offsets, ch_kf, ch_w = [], [0], [], []
    for kf in touched:                                                               # AddConnection(this, weight) in kf (:201-214)
        weights = dict(zip(ck[co[kf]:co[kf + 1]], cw[co[kf]:co[kf + 1]]))
        if cur in weights and weights[cur] == counter[kf]:                           # :205-210
            changed.append(0)
            continue
        weights[cur] = counter[kf]
        changed.append(1)
        kfs, ws = best_covisibles(weights, bad)                                      # :213
        ch_kf += kfs
        ch_w += ws
        offsets.append(len(ch_kf))
    return dict(status=UPDATED, parent=parent, counter_kf=i32(sorted(counter)), counter_weight=i32([counter[k] for k in sorted(counter)]),   # :473
                ordered_kf=i32(ordered_kf), ordered_weight=i32(ordered_weight), touched_kf=i32(touched), touched_changed=np.array(changed, np.uint8),
                changed_offsets=i32(offsets), changed_kf=i32(ch_kf), changed_weight=i32(ch_w), by_max=by_max, n_unchanged=changed.count(0))


def update_best_covisibles(rows, bad):
    """tc2li_update_best_covisibles_batch: rows = dict(offsets, kf, weight) -> dict(offsets, kf, weight)"""
    off, kf, w = ([int(v) for v in rows[k]] for k in ("offsets", "kf", "weight"))
    bad = [int(v) for v in bad]
    out_off, out_kf, out_w = [0], [], []
    for r in range(len(off) - 1):
        kfs, ws = best_covisibles(dict(zip(kf[off[r]:off[r + 1]], w[off[r]:off[r + 1]])), bad)
        out_kf += kfs
        out_w += ws
        out_off.append(len(out_kf))
    return dict(offsets=np.array(out_off, np.int32), kf=np.array(out_kf, np.int32), weight=np.array(out_w, np.int32))
