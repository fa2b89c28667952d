"""A restatement of the closing step of LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:455-485, "Recover optimized data") on the
flat tables of the map graph, independent of the library: commit() writes the tables directly, as the reference writes its objects;
commit_log() states the same step as the edit log that include/tc2li_hip.h defines.  A solved window is a dict with result, status,
pose_row, fixed, poses7, point_row, points3 and erase [n, 2] (pose index, point index), as ba_window_solve_batch returns it."""
import numpy as np

import map_graph_ref as ref

OP, INVALID, CAPACITY, Refused = ref.OP, ref.INVALID, ref.CAPACITY, ref.Refused
OK, ABORTED = 0, 1
POSITIONS_F32 = 1


def committed(solved):
    """the reference returns before this step for an aborted window (:126-130); a window the BA refused has no result to recover"""
    return int(solved["status"]) == OK and int(solved["result"]) >= 0


def _checked(tables, solved, flags):
    """-> per erase pair (keyframe row, point row, the index stored for the keyframe in the point's row); raises Refused"""
    if flags & ~POSITIONS_F32:
        raise Refused(INVALID, "flags")
    t = ref.tables_of(tables)
    n_kf, n_pt = len(t["kf_slot"]), len(t["point_flags"])
    pose_row, point_row = np.asarray(solved["pose_row"]).tolist(), np.asarray(solved["point_row"]).tolist()
    if any(not 0 <= r < n_kf for r in pose_row) or any(not 0 <= r < n_pt for r in point_row):
        raise Refused(INVALID, "a row outside the tables")
    erase = np.asarray(solved["erase"], np.int64).reshape(-1, 2).tolist()
    if int(solved.get("n_erase", len(erase))) > int(solved.get("erase_capacity", len(erase))):
        raise Refused(CAPACITY, "the erase lists are cut")
    oo = t["obs_offsets"].tolist()
    pairs = []
    for ep, et in erase:
        if not 0 <= ep < len(pose_row) or not 0 <= et < len(point_row):
            raise Refused(INVALID, "an erase index outside the counts")
        kf, pt = pose_row[ep], point_row[et]
        row = dict(zip(t["obs_kf"][oo[pt]:oo[pt + 1]].tolist(), t["obs_index"][oo[pt]:oo[pt + 1]].tolist()))   # mObservations
        if kf not in row:
            raise Refused(INVALID, "the keyframe is not in the point's row")
        pairs.append((kf, pt, row[kf]))                                                # GetIndexInKeyFrame, before any erase of this step
    return t, pairs


def _position(xyz, flags):
    xyz = np.asarray(xyz, np.float64)
    return xyz.astype(np.float32).astype(np.float64) if flags & POSITIONS_F32 else xyz   # vPoint->estimate().cast<float>() (:482)


def commit_log(tables, solved, flags=0):
    """-> (edit rows (op, a, b, c), values)"""
    if not committed(solved):
        if flags & ~POSITIONS_F32:
            raise Refused(INVALID, "flags")
        return [], []
    _, pairs = _checked(tables, solved, flags)
    edits, values = [], []
    n_slots = np.diff(ref.tables_of(tables)["slot_offsets"]).tolist()
    for kf, pt, index in pairs:                                                        # :457-463
        if 0 <= index < n_slots[kf]:                                                   # (a row whose matches are not resident has no such slot)
            edits.append((OP["SET_SLOT"], kf, index, -1))                              # pKFi->EraseMapPointMatch(pMPi) (:461)
        edits.append((OP["ERASE_OBSERVATION"], pt, kf, 0))                             # pMPi->EraseObservation(pKFi) (:462)
    for row, fixed, pose in zip(solved["pose_row"], solved["fixed"], np.asarray(solved["poses7"], np.float64).reshape(-1, 7)):
        if not fixed:                                                                  # lLocalKeyFrames (:468-475); the fixed cameras are not in it
            edits.append((OP["SET_POSE"], int(row), len(values), 0))
            values += pose.tolist()
    for row, xyz in zip(solved["point_row"], np.asarray(solved["points3"], np.float64).reshape(-1, 3)):   # lLocalMapPoints (:478-484)
        edits.append((OP["SET_POSITION"], int(row), len(values), 0))
        values += _position(xyz, flags).tolist()
    return edits, values


def commit(tables, solved, flags=0):
    """-> the tables after the step, written directly"""
    if not committed(solved):
        return ref.tables_of(tables)
    t, pairs = _checked(tables, solved, flags)
    t = {k: v.copy() for k, v in t.items()}
    so, oo = t["slot_offsets"].tolist(), t["obs_offsets"].tolist()
    obs = [dict(zip(t["obs_kf"][oo[p]:oo[p + 1]].tolist(), t["obs_index"][oo[p]:oo[p + 1]].tolist())) for p in range(len(oo) - 1)]
    for kf, pt, index in pairs:
        if 0 <= index < so[kf + 1] - so[kf]:
            t["slot_point"][so[kf] + index] = -1
        obs[pt].pop(kf, None)
    for row, fixed, pose in zip(solved["pose_row"], solved["fixed"], np.asarray(solved["poses7"], np.float64).reshape(-1, 7)):
        if not fixed:
            t["poses7"][int(row)] = pose
    for row, xyz in zip(solved["point_row"], np.asarray(solved["points3"], np.float64).reshape(-1, 3)):
        t["positions"][int(row)] = _position(xyz, flags)
    rows = [sorted(o.items()) for o in obs]
    t["obs_offsets"] = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    t["obs_kf"] = np.array([k for r in rows for k, _ in r], np.int32)
    t["obs_index"] = np.array([i for r in rows for _, i in r], np.int32)
    return t
