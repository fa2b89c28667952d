"""A sequential restatement of the edit log of the resident map graph (include/tc2li_hip.h "the map graph resident on the device"),
independent of the library's host twin: plain Python lists and dicts, one edit after the other.  Reference lines: SF/src/Tracking.cc:3078
(new KeyFrame), SF/src/KeyFrame.cc:121 (SetPose), :585 (SetBadFlag), :309-340 (AddMapPoint / EraseMapPointMatch / ReplaceMapPointMatch),
SF/src/MapPoint.cc:150-175 (AddObservation), :177-210 (EraseObservation), :225 (SetBadFlag and its mObservations.clear())."""
import numpy as np

OPS = ("ADD_KEYFRAME", "SET_KEYFRAME_FLAGS", "SET_POSE", "ADD_POINT", "SET_POINT_FLAGS", "SET_POSITION", "SET_SLOT", "ADD_OBSERVATION",
       "ERASE_OBSERVATION", "CLEAR_OBSERVATIONS")
OP = {k: i for i, k in enumerate(OPS)}
INVALID, CAPACITY = -2, -5
TABLES = (("kf_slot", np.int32), ("kf_id", np.int64), ("kf_flags", np.uint8), ("poses7", np.float64), ("slot_offsets", np.int32),
          ("slot_point", np.int32), ("point_flags", np.uint8), ("positions", np.float64), ("obs_offsets", np.int32), ("obs_kf", np.int32),
          ("obs_index", np.int32))


class Refused(Exception):
    def __init__(self, code, what):
        Exception.__init__(self, what)
        self.code = code


def tables_of(problem):
    """The eleven tables of a window problem, typed and shaped as the library returns them."""
    t = {k: np.ascontiguousarray(problem[k], ty) for k, ty in TABLES}
    t["poses7"], t["positions"] = t["poses7"].reshape(-1, 7), t["positions"].reshape(-1, 3)
    return t


def apply(tables, edits, values, capacities, keypoints_of_slot=None):
    """tables: a dict of the eleven arrays; edits: rows (op, a, b, c); values: floats; capacities: keyframes, slots, points, observations.
    keypoints_of_slot: per store slot the keypoints it holds, None for an empty one -- or None altogether, as the host twin checks (a store
    slot >= 0, an index >= -1).  -> the tables after the log; raises Refused(code) and changes nothing otherwise.
    The first edit that fails decides; the observation bound (resident entries + ADD_OBSERVATION edits > capacity) comes after all edits."""
    t = tables_of(tables)
    values = [float(v) for v in np.asarray(values if values is not None else [], np.float64).reshape(-1)]
    cap_kf, cap_slot, cap_pt, cap_obs = [int(c) for c in capacities]
    kf_slot, kf_id, kf_flags = t["kf_slot"].tolist(), t["kf_id"].tolist(), t["kf_flags"].tolist()
    poses = [list(r) for r in t["poses7"].tolist()]
    so = t["slot_offsets"].tolist()
    slots = [t["slot_point"][so[k]:so[k + 1]].tolist() for k in range(len(kf_slot))]
    pflags, positions = t["point_flags"].tolist(), [list(r) for r in t["positions"].tolist()]
    oo = t["obs_offsets"].tolist()
    obs = [dict(zip(t["obs_kf"][oo[p]:oo[p + 1]].tolist(), t["obs_index"][oo[p]:oo[p + 1]].tolist())) for p in range(len(pflags))]   # mObservations
    resident, adds = oo[-1], 0

    def refuse(code, what):
        raise Refused(code, what)

    def vals(off, n):
        if off < 0 or off + n > len(values):
            refuse(INVALID, "values offset")
        return values[off:off + n]

    def kf_row(r):
        if not 0 <= r < len(kf_slot):
            refuse(INVALID, "keyframe row")

    def pt_row(r):
        if not 0 <= r < len(pflags):
            refuse(INVALID, "point row")

    def byte(v):
        if not 0 <= v <= 255:
            refuse(INVALID, "flags")

    for op, a, b, c in [tuple(int(x) for x in e) for e in np.asarray(edits).tolist()] if len(edits) else []:
        if op == OP["ADD_KEYFRAME"]:                                                   # Tracking.cc:3078
            if a < 0 or (keypoints_of_slot is not None and (a >= len(keypoints_of_slot) or keypoints_of_slot[a] is None)):
                refuse(INVALID, "store slot")
            if b < 0:
                refuse(INVALID, "slot count")
            v = vals(c, 9)
            if not np.isfinite(v[:2]).all() or v[0] != int(v[0]) or abs(v[0]) > 2.0 ** 53 or v[1] != int(v[1]):
                refuse(INVALID, "id or flags")
            byte(v[1])
            if len(kf_slot) + 1 > cap_kf or sum(len(s) for s in slots) + b > cap_slot:
                refuse(CAPACITY, "keyframes or slots")
            kf_slot.append(a); kf_id.append(int(v[0])); kf_flags.append(int(v[1])); poses.append(v[2:9]); slots.append([-1] * b)
        elif op == OP["SET_KEYFRAME_FLAGS"]:                                           # KeyFrame.cc:585
            kf_row(a); byte(b)
            kf_flags[a] = b
        elif op == OP["SET_POSE"]:                                                     # KeyFrame.cc:121
            kf_row(a)
            poses[a] = vals(b, 7)
        elif op == OP["ADD_POINT"]:
            byte(a)
            v = vals(b, 3)
            if len(pflags) + 1 > cap_pt:
                refuse(CAPACITY, "points")
            pflags.append(a); positions.append(v); obs.append({})
        elif op == OP["SET_POINT_FLAGS"]:                                              # MapPoint.cc:225
            pt_row(a); byte(b)
            pflags[a] = b
        elif op == OP["SET_POSITION"]:
            pt_row(a)
            positions[a] = vals(b, 3)
        elif op == OP["SET_SLOT"]:                                                     # KeyFrame.cc:309-340
            kf_row(a)
            if not 0 <= b < len(slots[a]) or not -1 <= c < len(pflags):
                refuse(INVALID, "slot or point")
            slots[a][b] = c
        elif op == OP["ADD_OBSERVATION"]:                                              # MapPoint.cc:150-175; a present keyframe: its index overwritten (:155-169)
            pt_row(a); kf_row(b)
            if c < -1 or (keypoints_of_slot is not None and c >= keypoints_of_slot[kf_slot[b]]):
                refuse(INVALID, "observation index")
            obs[a][b] = c
            adds += 1
        elif op == OP["ERASE_OBSERVATION"]:                                            # MapPoint.cc:177-210; absent: nothing (:182)
            pt_row(a); kf_row(b)
            obs[a].pop(b, None)
        elif op == OP["CLEAR_OBSERVATIONS"]:                                           # mObservations.clear()
            pt_row(a)
            obs[a].clear()
        else:
            refuse(INVALID, "op")
    if resident + adds > cap_obs:
        refuse(CAPACITY, "observations")
    rows = [sorted(o.items()) for o in obs]
    return dict(kf_slot=np.array(kf_slot, np.int32), kf_id=np.array(kf_id, np.int64), kf_flags=np.array(kf_flags, np.uint8),
                poses7=np.array(poses, np.float64).reshape(-1, 7), slot_offsets=np.cumsum([0] + [len(s) for s in slots]).astype(np.int32),
                slot_point=np.array([p for s in slots for p in s], np.int32), point_flags=np.array(pflags, np.uint8),
                positions=np.array(positions, np.float64).reshape(-1, 3), obs_offsets=np.cumsum([0] + [len(r) for r in rows]).astype(np.int32),
                obs_kf=np.array([k for r in rows for k, _ in r], np.int32), obs_index=np.array([i for r in rows for _, i in r], np.int32))


def assert_same_tables(got, want, what=""):
    for k, ty in TABLES:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.dtype == np.dtype(ty) and g.shape == w.shape and np.array_equal(g, w), (what, k, g, w)
