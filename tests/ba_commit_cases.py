"""Hand-made and random solved windows for the tests of the local BA's closing step on the map graph (tests/ba_commit_ref.py): a graph,
a window on it as ba_window_solve_batch would return it, and for the hand-made ones the LITERAL edit list the step must give."""
import numpy as np

import ba_window_cases as K
import map_graph_ref as ref

OP = ref.OP


def main_graph(without_slots=()):
    """4 keyframes with 8 slots each and 6 points; a keyframe holds a point in the slot the observation's index names.  without_slots: rows
    whose matches are not resident (an empty slot row, as the gather allows for a row that is neither current nor a neighbour)."""
    obs = [{0: 1, 2: 3}, {1: 0, 2: 1, 3: 2}, {0: 2}, {1: 4, 3: 5}, {0: 5, 1: 2, 3: 0}, {2: 6, 3: 7}]
    holds = [[-1] * 8 for _ in range(4)]
    for p, row in enumerate(obs):
        for k, i in row.items():
            holds[k][i] = p
    return K.hand([dict(slot=s, id=10 * (s + 1), holds=[] if s in without_slots else holds[s]) for s in range(4)], [dict(obs=o) for o in obs], 3, [0, 1, 2])


def main_window():
    """Keyframe row 0 is fixed.  Three erase pairs, not sorted by pose or point, two of them on point index 0 (point row 4); the pair
    (pose 2 = row 3, point 0 = row 4) erases the observation stored with index 0 at position 2 of the point's row."""
    poses7 = np.array([[0.1 * i + 0.01 * c for c in range(7)] for i in range(4)], np.float64)
    points3 = np.array([[0.1, 1.0 + j, 1.0 / 3.0] for j in range(6)], np.float64)
    return dict(result=5, status=0, pose_row=np.array([2, 0, 3, 1], np.int32), fixed=np.array([0, 1, 0, 0], np.uint8), poses7=poses7,
                point_row=np.array([4, 1, 5, 0, 2, 3], np.int32), points3=points3, erase=np.array([[2, 0], [0, 2], [3, 0]], np.int32))


MAIN_EDITS = [(OP["SET_SLOT"], 3, 0, -1), (OP["ERASE_OBSERVATION"], 4, 3, 0),          # pair (2, 0): keyframe row 3, point row 4, the index stored: 0
              (OP["SET_SLOT"], 2, 6, -1), (OP["ERASE_OBSERVATION"], 5, 2, 0),          # pair (0, 2): keyframe row 2, point row 5, index 6
              (OP["SET_SLOT"], 1, 2, -1), (OP["ERASE_OBSERVATION"], 4, 1, 0),          # pair (3, 0): keyframe row 1, point row 4, index 2
              (OP["SET_POSE"], 2, 0, 0), (OP["SET_POSE"], 3, 7, 0), (OP["SET_POSE"], 1, 14, 0),   # pose 1 (row 0) is fixed
              (OP["SET_POSITION"], 4, 21, 0), (OP["SET_POSITION"], 1, 24, 0), (OP["SET_POSITION"], 5, 27, 0), (OP["SET_POSITION"], 0, 30, 0),
              (OP["SET_POSITION"], 2, 33, 0), (OP["SET_POSITION"], 3, 36, 0)]


# keyframe row 1 without resident slots: its pair has no slot to clear and keeps its ERASE_OBSERVATION alone
EDITS_WITHOUT_SLOTS_OF_ROW_1 = [e for e in MAIN_EDITS if e != (OP["SET_SLOT"], 1, 2, -1)]


def main_values(window):
    return np.concatenate([window["poses7"][[0, 2, 3]].reshape(-1), window["points3"].reshape(-1)])


def refused():
    """(what, window, flags, capacities (edits, values) or None, code) on main_graph()"""
    w = main_window()
    R = lambda **kw: dict(w, **kw)
    return [("a pose_row beyond the tables", R(pose_row=np.array([2, 0, 4, 1], np.int32)), 0, None, ref.INVALID),
            ("a negative pose_row", R(pose_row=np.array([2, -1, 3, 1], np.int32)), 0, None, ref.INVALID),
            ("a point_row beyond the tables", R(point_row=np.array([4, 1, 5, 0, 2, 6], np.int32)), 0, None, ref.INVALID),
            ("a negative point_row", R(point_row=np.array([4, 1, 5, 0, -1, 3], np.int32)), 0, None, ref.INVALID),
            ("an erase pose beyond the counts", R(erase=np.array([[2, 0], [4, 2]], np.int32)), 0, None, ref.INVALID),
            ("a negative erase pose", R(erase=np.array([[-1, 0]], np.int32)), 0, None, ref.INVALID),
            ("an erase point beyond the counts", R(erase=np.array([[2, 6]], np.int32)), 0, None, ref.INVALID),
            ("a negative erase point", R(erase=np.array([[2, -1]], np.int32)), 0, None, ref.INVALID),
            ("a pair whose keyframe is not in the point's row", R(erase=np.array([[2, 0], [0, 0]], np.int32)), 0, None, ref.INVALID),   # row 2 does not see point row 4
            ("an unknown flag bit", w, 2, None, ref.INVALID),
            ("the erase lists cut at their capacity", R(n_erase=3, erase_capacity=2, erase=w["erase"][:2]), 0, None, ref.CAPACITY),
            ("room for one edit too few", w, 0, (len(MAIN_EDITS) - 1, 39), ref.CAPACITY),
            ("room for one value too few", w, 0, (len(MAIN_EDITS), 38), ref.CAPACITY)]


def random_windows(n=12):
    """(name, graph, window): random graphs of ba_window_cases.make_graph with a random window on each -- some rows as poses, a share of
    them fixed, some points, erase pairs drawn from the observations that join a listed pose and a listed point, whether the stored
    index names a slot of the keyframe row or not (make_graph gives slots to the current keyframe and its neighbours only)."""
    out = []
    for i in range(n):
        rng = np.random.default_rng(4100 + i)
        g = K.make_graph(4200 + i, int(rng.integers(3, 11)), int(rng.integers(10, 120)))
        n_kf, n_pt = len(g["kf_slot"]), len(g["point_flags"])
        pose_row = rng.permutation(n_kf)[:int(rng.integers(1, n_kf + 1))].astype(np.int32)
        point_row = rng.permutation(n_pt)[:int(rng.integers(1, n_pt + 1))].astype(np.int32)
        fixed = (rng.random(len(pose_row)) < 0.3).astype(np.uint8)
        pose_of, point_of = {int(r): k for k, r in enumerate(pose_row)}, {int(r): k for k, r in enumerate(point_row)}
        pairs = [(pose_of[int(k)], point_of[p]) for p in point_of for o in range(g["obs_offsets"][p], g["obs_offsets"][p + 1])
                 for k in [g["obs_kf"][o]] if int(k) in pose_of]
        pairs = [pairs[j] for j in rng.permutation(len(pairs))[:int(rng.integers(0, len(pairs) + 1)) if i % 4 else 0]]
        out.append(("random %d" % i, g, dict(result=int(rng.integers(0, 6)), status=0, pose_row=pose_row, fixed=fixed, poses7=rng.normal(0, 1, (len(pose_row), 7)),
                                             point_row=point_row, points3=rng.normal(0, 10, (len(point_row), 3)),
                                             erase=np.array(pairs, np.int32).reshape(-1, 2))))
    return out
