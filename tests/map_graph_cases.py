"""Graphs and edit logs for the tests of the resident map graph, built on ba_window_cases.make_graph / family / hand: random logs that
are valid by construction, and directed logs, one per rule of the log (tests/map_graph_ref.py says what each must give)."""
import numpy as np

import ba_window_cases as K
import map_graph_ref as ref

OP = ref.OP
N_KEYS = [None if v is None else len(v["keys"]) for v in K.WORLD]                       # keypoints per store slot
OCCUPIED = [s for s, v in enumerate(K.WORLD) if v is not None]
EDIT_DTYPE = np.dtype([("op", "<i4"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])


class Log:
    """An edit log under construction: the edits, their values, and the sizes they will meet (so that later edits may name new rows)."""

    def __init__(self, tables):
        self.edits, self.values = [], []
        self.kf_slot = [int(s) for s in tables["kf_slot"]]
        self.n_slots = np.diff(np.asarray(tables["slot_offsets"])).tolist()
        self.n_points = len(tables["point_flags"])

    def _put(self, vals):
        at = len(self.values)
        self.values += [float(v) for v in vals]
        return at

    def add_keyframe(self, slot, n_slots, kf_id, flags, pose7):
        self.edits.append((OP["ADD_KEYFRAME"], slot, n_slots, self._put([kf_id, flags] + list(pose7))))
        self.kf_slot.append(slot); self.n_slots.append(n_slots)
        return len(self.kf_slot) - 1

    def set_keyframe_flags(self, row, flags): self.edits.append((OP["SET_KEYFRAME_FLAGS"], row, flags, 0))
    def set_pose(self, row, pose7): self.edits.append((OP["SET_POSE"], row, self._put(pose7), 0))

    def add_point(self, flags, xyz):
        self.edits.append((OP["ADD_POINT"], flags, self._put(xyz), 0))
        self.n_points += 1
        return self.n_points - 1

    def set_point_flags(self, row, flags): self.edits.append((OP["SET_POINT_FLAGS"], row, flags, 0))
    def set_position(self, row, xyz): self.edits.append((OP["SET_POSITION"], row, self._put(xyz), 0))
    def set_slot(self, row, slot, point): self.edits.append((OP["SET_SLOT"], row, slot, point))
    def add_observation(self, point, row, index): self.edits.append((OP["ADD_OBSERVATION"], point, row, index))
    def erase_observation(self, point, row): self.edits.append((OP["ERASE_OBSERVATION"], point, row, 0))
    def clear_observations(self, point): self.edits.append((OP["CLEAR_OBSERVATIONS"], point, 0, 0))

    def done(self):
        return np.array(self.edits, np.int32).reshape(-1, 4).view(EDIT_DTYPE).reshape(-1), np.array(self.values, np.float64)


def random_log(seed, tables, n_edits, appends=True):
    """n_edits edits, every op drawn, valid against `tables` and the world's store; observation edits cluster on few points so that rows
    meet several edits, pairs are added, erased and added again, absent pairs erased."""
    rng = np.random.default_rng(seed)
    L = Log(tables)
    hot = rng.integers(0, max(L.n_points, 1), 6).tolist() if L.n_points else []
    while len(L.edits) < n_edits:
        op = int(rng.integers(0, 10))
        n_kf = len(L.kf_slot)
        point = int(hot[rng.integers(0, len(hot))]) if hot and rng.random() < 0.5 else (int(rng.integers(0, L.n_points)) if L.n_points else -1)
        row = int(rng.integers(0, n_kf)) if n_kf else -1
        if op == OP["ADD_KEYFRAME"]:
            if appends and rng.random() < 0.15:
                L.add_keyframe(int(rng.choice(OCCUPIED)), int(rng.integers(0, 12)), int(rng.integers(1, 1 << 40)), int(rng.integers(0, 8)), rng.normal(0, 1, 7))
        elif op == OP["ADD_POINT"]:
            if appends and rng.random() < 0.3:
                hot.append(L.add_point(int(rng.integers(0, 4)), rng.normal(0, 10, 3)))
        elif op == OP["SET_KEYFRAME_FLAGS"] and n_kf: L.set_keyframe_flags(row, int(rng.integers(0, 8)))
        elif op == OP["SET_POSE"] and n_kf: L.set_pose(row, rng.normal(0, 1, 7))
        elif op == OP["SET_POINT_FLAGS"] and point >= 0: L.set_point_flags(point, int(rng.integers(0, 4)))
        elif op == OP["SET_POSITION"] and point >= 0: L.set_position(point, rng.normal(0, 10, 3))
        elif op == OP["SET_SLOT"] and n_kf and L.n_slots[row]: L.set_slot(row, int(rng.integers(0, L.n_slots[row])), int(rng.integers(-1, L.n_points)))
        elif op == OP["ADD_OBSERVATION"] and n_kf and point >= 0: L.add_observation(point, row, int(rng.integers(-1, N_KEYS[L.kf_slot[row]])))
        elif op == OP["ERASE_OBSERVATION"] and n_kf and point >= 0: L.erase_observation(point, row)
        elif op == OP["CLEAR_OBSERVATIONS"] and point >= 0 and rng.random() < 0.2: L.clear_observations(point)
    return L.done()


def capacities_for(tables, edits, slack=0):
    """What the tables and the log need at most: keyframes, slots, points, observations."""
    e = np.asarray(edits)
    kf, pt = e["op"] == OP["ADD_KEYFRAME"], e["op"] == OP["ADD_POINT"]
    return np.array([max(1, len(tables["kf_slot"]) + kf.sum()), max(1, int(tables["slot_offsets"][-1]) + e["b"][kf].sum()),
                     max(1, len(tables["point_flags"]) + pt.sum()), max(1, int(tables["obs_offsets"][-1]) + (e["op"] == OP["ADD_OBSERVATION"]).sum())], np.int32) + slack


def random_graphs():
    """About 30 graphs of 3-12 keyframes and 20-300 points, each with a random log."""
    rng = np.random.default_rng(91)
    out = []
    for i in range(30):
        g = K.make_graph(700 + i, int(rng.integers(3, 13)), int(rng.integers(20, 301)))
        out.append(("random %d" % i, g, random_log(800 + i, g, int(rng.integers(1, 400)))))
    return out


def wide_graph(n_kf=300, n_points=12, long_rows=()):
    """n_kf keyframe rows with four slots each and n_points points; point p of long_rows = {p: n} is seen by the first n odd rows (so that
    even rows can be inserted in front, between and behind), the others by rows 2, 5 and 7."""
    kfs = [dict(slot=OCCUPIED[k % len(OCCUPIED)], id=1000 + 7 * ((k * 37) % n_kf), holds=[-1, k % n_points, -1, (k + 1) % n_points]) for k in range(n_kf)]
    points = [dict(obs={2 * j + 1: j % 8 for j in range(long_rows[p])} if p in long_rows else {2: 0, 5: 1, 7: 2}) for p in range(n_points)]
    points[1]["obs"] = {}
    points[2]["obs"] = {3: 1}
    return K.hand(kfs, points, 0, [1, 2, 3])


def directed(lds_row):
    """(name, graph, (edits, values)) per rule.  lds_row: tc2li_map_graph_limits' longest row merged in LDS."""
    out = []
    g = wide_graph()

    def case(name, build, graph=g):
        L = Log(graph)
        build(L)
        out.append((name, graph, L.done()))

    case("no edit", lambda L: None)
    case("insert at the front, the middle and the end", lambda L: (L.add_observation(0, 0, 3), L.add_observation(0, 4, -1), L.add_observation(0, 9, 5)))
    case("a row from 0 to 1 and from 1 to 0", lambda L: (L.add_observation(1, 6, 2), L.erase_observation(2, 3)))
    case("add, erase, add of one pair", lambda L: (L.add_observation(3, 4, 1), L.erase_observation(3, 4), L.add_observation(3, 4, 6)))
    case("add on a present pair overwrites the index", lambda L: L.add_observation(3, 5, 7))
    case("erase of an absent pair", lambda L: (L.erase_observation(3, 4), L.erase_observation(1, 0)))
    case("clear, then add", lambda L: (L.clear_observations(3), L.add_observation(3, 6, 0), L.clear_observations(4)))
    case("add, then clear", lambda L: (L.add_observation(3, 6, 0), L.clear_observations(3)))
    case("two writes of one slot, one pose, one flag, one position",
         lambda L: (L.set_slot(4, 1, 3), L.set_slot(4, 1, 7), L.set_pose(2, range(7)), L.set_pose(2, range(7, 14)), L.set_keyframe_flags(5, 1), L.set_keyframe_flags(5, 4),
                    L.set_point_flags(6, 1), L.set_point_flags(6, 2), L.set_position(6, (1, 2, 3)), L.set_position(6, (4, 5, 6))))

    def new_rows(L):
        k = L.add_keyframe(OCCUPIED[0], 5, (1 << 40) + 3, 4, (0, 0, 0, 1, 9, 8, 7))
        p = L.add_point(0, (1.5, 2.5, 3.5))
        L.set_slot(k, 2, p); L.set_slot(k, 4, 0); L.add_observation(p, k, 1); L.add_observation(p, 0, 2); L.add_observation(0, k, -1)
        L.set_pose(k, (0, 0, 1, 0, 1, 2, 3)); L.set_keyframe_flags(k, 5); L.set_position(p, (7, 8, 9)); L.set_point_flags(p, 1)
        k2 = L.add_keyframe(OCCUPIED[1], 0, 17, 0, (0, 0, 0, 1, 0, 0, 0))
        L.add_observation(p, k2, 0)
        p2 = L.add_point(3, (0, 0, 0))
        L.clear_observations(p2)
    case("new rows, then edits on them", new_rows)
    case("every point touched", lambda L: [L.add_observation(p, 10 + p, p % 8) for p in range(L.n_points)])
    case("no observation touched", lambda L: (L.set_pose(0, range(7)), L.set_slot(0, 0, 2)))

    long = wide_graph(n_kf=2 * lds_row + 30, long_rows={5: 60, 6: lds_row - 8, 7: lds_row - 7})
    case("a row growing across 64 entries", lambda L: [L.add_observation(5, 2 * j, j % 8) for j in range(10)], long)
    # old entries + the row's eight ADD edits: lds_row exactly (merged in LDS) and lds_row + 1 (merged in global memory); fronts, middles, an erase
    def at_the_limit(L):
        for p in (6, 7):
            for j in (0, 10, 40, 100, 120, 200, 260):
                L.add_observation(p, 2 * j, j % 8)
            L.erase_observation(p, 51); L.add_observation(p, 51, 3); L.erase_observation(p, 2)
    case("rows at and one beyond the LDS limit", at_the_limit, long)
    for n in (0, 1, 63, 64, 65, 256, 257):
        graph = K.make_graph(600 + n, 9, 120)
        out.append(("%d edits" % n, graph, random_log(900 + n, graph, n)))
    return out
