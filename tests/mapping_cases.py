"""Hand-made keyframes for the directed tests of local mapping's geometric front half (mapping_kernels.hip: k_tri_search, k_tri_points,
k_new_points_compact, k_fuse_search and their batch forms; mapping_host.hpp: set_pose, pair_constants, baseline).

This module builds inputs and never computes what the code under test should make of them.  A case is a small named group of keypoints
-- one in the current keyframe, candidates in one neighbour -- around a float64 world point, with the outcome it was built for
(`expect`) and the gate quantity it targets (`gates`: kind, value in float64, threshold).  test_mapping_cases.py shows on the CPU that
mapping_ref.py and the oracle produce that outcome; test_mapping_gates_gpu.py then runs the product on the same dicts.

Worlds.  Every scene is built for a world = the pose of the current keyframe and how the neighbours lie relative to it:
  identity  Rcw = I, the neighbours pure translations (what tests/test_mapping.py covers), except the one that looks backwards
  rotated   current keyframe yaw 25, pitch -12, roll 8 degrees with a translation in all three axes; neighbours rotated a further 5 to
            12 degrees about an oblique axis; two of them carry the quaternion with w < 0
  turned    the rotated world under a further 170 degree turn about an oblique axis, every quaternion negated (Fuse only)
Neighbour kinds (centre in the current camera's frame): SIDE (0.9, 0.15, 0.1), FWD (0.1, -0.05, 1.2) whose epipole lies inside the image,
SIDE2 (-0.8, 0.2, -0.3), BACK (0.6, 0.1, 0.4) turned by 170 degrees so that its rays leave the other way, FACING (0.3, 0.1, 6.0) turned by
172 degrees about the vertical: it looks back at the current keyframe, and a point between the two is in front of both.

Poses are made as float64 rotation matrices (rodrigues), rounded to pose7 once, and every keypoint is then placed against the pose that
the rounded pose7 stands for (pose_Rt), so the float32 inputs are exact to their own rounding.

Margins (margins_ok): a targeted quantity lies at least 1e-3 of the threshold from it ("rel": pixel, chi-square, distance and ratio
gates; image bounds use the image extent as the scale, their lower ends being 0), 2e-5 absolute for cosines ("cos", about 300 float32
ulps at 1.0).  One case is exempt by design: fuse chi2_mono_between_5.99_and_5.991 has to sit inside a band 1.7e-4 wide, 8e-5 of the
threshold from either end; at octave 7 the float32 evaluation of u is good to about 1e-4 px of 8.8 px, 2.3e-5 of the squared error.
Integer gates (Hamming, octaves) are exact."""
import numpy as np

W, H = 800, 300
BOUNDS0 = (0.0, 800.0, 0.0, 300.0)
BOUNDS1 = (-7.5, 805.25, -3.0, 303.5)
BOUNDS2 = (-7.5, 805.25, -5.25, 303.5)   # an origin of more than half a cell in y too (see fuse_scene, window origin)
GRID_COLS, GRID_ROWS = 64, 48
KP = np.dtype([("x", "<f4"), ("y", "<f4"), ("size", "<f4"), ("angle", "<f4"), ("response", "<f4"), ("octave", "<i4")])
MP = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"), ("max_distance_raw", "<f4"),
               ("descriptor", "u1", (32,))])
SIDE, FWD, SIDE2, BACK, FACING = 0, 1, 2, 3, 4
REL_MARGIN, COS_MARGIN = 1e-3, 2e-5

# Largest deviation of the oracle's triangulated points from mapping_ref.create_new_map_points, |delta| / max(1, |x3D|), over every
# triangulated record of the cnmp / far / first / baseline / compaction scenes of all worlds and the random scene with more than 2 degrees of
# parallax and less than 25 m from the current keyframe.  Measured 2026-10-20 on the CPU by test_mapping_cases.py::test_oracle_deviation_is_the_recorded_one,
# which fails if the figure drifts above it.  The product's bar is 4 x this and nothing more.
ORACLE_TRI_DEVIATION = 8.2e-7   # measured 8.145e-07 over 174 records
PRODUCT_TRI_BAR = 4 * ORACLE_TRI_DEVIATION


def tables(n_levels=8):
    sf = np.cumprod(np.concatenate([[np.float32(1)], np.full(n_levels - 1, np.float32(1.2))])).astype(np.float32)
    return sf, (sf * sf).astype(np.float32)


class Env:
    """camera, level tables: the float32 values the entries get, as Python floats"""

    def __init__(self, synthetic):
        self.cam4 = np.float32([synthetic.FX, synthetic.FY, synthetic.CX, synthetic.CY])
        self.fx, self.fy, self.cx, self.cy = [float(v) for v in self.cam4]
        bf = np.float32(synthetic.BF)
        self.bf, self.mb = float(bf), float(bf / np.float32(synthetic.FX))
        self.cam5 = np.float64([self.fx, self.fy, self.cx, self.cy, self.bf])
        self.sf, self.sg = tables()
        self.isg = (np.float32(1) / self.sg).astype(np.float32)
        self.logsf = float(np.log(np.float32(1.2)))

    def project(self, pose, X):
        x, y, z = pose[0] @ np.asarray(X, np.float64) + pose[1]
        return np.array([self.fx * x / z + self.cx, self.fy * y / z + self.cy]), z

    def ray(self, pose, uv):
        return pose[0].T @ np.array([(uv[0] - self.cx) / self.fx, (uv[1] - self.cy) / self.fy, 1.0])


# ---- poses ---------------------------------------------------------------------------------------------------------------------------------
def rodrigues(axis, deg):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * (Kx @ Kx)


def quat_of(R):
    """(x, y, z, w) with w >= 0"""
    w = 0.5 * np.sqrt(max(0.0, 1 + R[0, 0] + R[1, 1] + R[2, 2]))
    if w > 0.1:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:  # near a half turn: from the largest diagonal entry
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(1 + R[i, i] - R[j, j] - R[k, k])
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = 0.25 * s, (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s, (R[k, j] - R[j, k]) / s
        if q[3] < 0:
            q = -q
    return q / np.linalg.norm(q)


def pose7_of(R, t, negate=False):
    q = quat_of(R)
    return np.concatenate([-q if negate else q, t]).astype(np.float32)


def pose_Rt(pose7):
    """what a rounded pose7 stands for: (Rcw, tcw) float64, the textbook matrix of a unit quaternion"""
    x, y, z, w = np.asarray(pose7[:4], np.float64) / np.linalg.norm(np.asarray(pose7[:4], np.float64))
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, np.asarray(pose7[4:7], np.float64)


def centre(pose):
    return -pose[0].T @ pose[1]


OBLIQUE = (0.48, -0.62, 0.62)
NB_CENTRE = {SIDE: (0.9, 0.15, 0.1), FWD: (0.1, -0.05, 1.2), SIDE2: (-0.8, 0.2, -0.3), BACK: (0.6, 0.1, 0.4), FACING: (0.3, 0.1, 6.0)}
FACING_AXIS, FACING_TURN = (0.05, 1.0, 0.03), 172.0   # in front of the current keyframe, looking back at it
NB_TURN = {SIDE: 8.0, FWD: 5.0, SIDE2: 12.0}
WORLDS = ("identity", "rotated")
FUSE_WORLDS = ("identity", "rotated", "turned")


def current_pose7(world):
    if world == "identity":
        return pose7_of(np.eye(3), np.array([-0.4, 0.0, -1.1]))
    R = rodrigues((0, 1, 0), 25) @ rodrigues((1, 0, 0), -12) @ rodrigues((0, 0, 1), 8)
    t = np.array([0.7, -0.35, 1.9])
    if world == "turned":
        G = rodrigues(OBLIQUE, 170)
        return pose7_of(R @ G.T, t, negate=True)
    return pose7_of(R, t)


def neighbour_pose7(world, cur7, kind, c=None, turn=None):
    """the neighbour whose centre is c in the current camera's frame, its axes turned by `turn` degrees about OBLIQUE"""
    Rc, tc = pose_Rt(cur7)
    c = np.asarray(NB_CENTRE[kind] if c is None else c, np.float64)
    if turn is None:
        turn = 170.0 if kind == BACK else FACING_TURN if kind == FACING else (0.0 if world == "identity" else NB_TURN[kind])
    dR = rodrigues(FACING_AXIS if kind == FACING else OBLIQUE, turn)
    return pose7_of(dR.T @ Rc, dR.T @ (tc - c), negate=(world != "identity" and kind in (SIDE2, BACK)))


# ---- keyframes -----------------------------------------------------------------------------------------------------------------------------
def flip(desc, k, start=0):
    """the descriptor with bits start .. start + k - 1 inverted: Hamming distance k from desc, exactly"""
    bits = np.unpackbits(desc)
    bits[start:start + k] ^= 1
    return np.packbits(bits)


class KfBuilder:
    """Keypoints are added with a vocabulary node; the feature vector lists a node's keypoints in the order they were added, while the
    keypoint indices are a fixed shuffle of it, so that 'later in the feature vector' and 'larger index' are different things."""

    def __init__(self):
        self.rows = []

    def add(self, xy, node, desc, octave=0, ur=-1.0, depth=-1.0, hp=0, angle=0.0, case=None):
        self.rows.append(dict(x=np.float32(xy[0]), y=np.float32(xy[1]), node=int(node), desc=desc, octave=int(octave), ur=np.float32(ur),
                              depth=np.float32(depth), hp=int(hp), angle=np.float32(angle), case=case))
        return len(self.rows) - 1

    def xy(self, h):
        return np.array([float(self.rows[h]["x"]), float(self.rows[h]["y"])])

    def finish(self, pose7, seed, shuffle=True):
        n = len(self.rows)
        self.index = np.random.default_rng(seed).permutation(n) if shuffle else np.arange(n)   # handle -> keypoint index
        keys = np.zeros(n, KP)
        desc, ur, depth, hp = np.zeros((n, 32), np.uint8), np.zeros(n, np.float32), np.zeros(n, np.float32), np.zeros(n, np.uint8)
        for h, r in enumerate(self.rows):
            i = self.index[h]
            keys[i] = (r["x"], r["y"], 31.0, r["angle"], 1.0, r["octave"])
            desc[i], ur[i], depth[i], hp[i] = r["desc"], r["ur"], r["depth"], r["hp"]
        nodes = sorted({r["node"] for r in self.rows})
        members = [[self.index[h] for h, r in enumerate(self.rows) if r["node"] == nd] for nd in nodes]
        off = np.concatenate([[0], np.cumsum([len(m) for m in members])]).astype(np.int32)
        fvi = np.array([i for m in members for i in m], np.int32)
        return dict(keys=keys, descriptors=desc, u_right=ur, depth=depth, has_point=hp, fv_node=np.array(nodes, np.int32), fv_offset=off,
                    fv_index=fvi, pose7=np.asarray(pose7, np.float32))


class Scene:
    """current keyframe + neighbours + cases"""

    def __init__(self, env, world, kinds, seed, poses7=None):
        self.env, self.world, self.kinds = env, world, list(kinds)
        self.cur7 = current_pose7(world)
        self.nb7 = [neighbour_pose7(world, self.cur7, k) for k in kinds] if poses7 is None else list(poses7)
        self.cur_pose, self.nb_pose = pose_Rt(self.cur7), [pose_Rt(p) for p in self.nb7]
        self.cur_b, self.nb_b = KfBuilder(), [KfBuilder() for _ in self.nb7]
        self.rng = np.random.default_rng(seed)
        self.seed = seed
        self.cases = []
        self._node = 1

    def node(self):
        self._node += 1
        return 7 * self._node + 3

    def descriptor(self):
        return self.rng.integers(0, 256, 32, dtype=np.uint8)

    def from_cur(self, xc):
        """world point of a point given in the current camera's frame"""
        return self.cur_pose[0].T @ (np.asarray(xc, np.float64) - self.cur_pose[1])

    def stereo(self, pose, X):
        uv, z = self.env.project(pose, X)
        return dict(ur=uv[0] - self.env.bf / z, depth=z)

    def add(self, name, nb, X, cur, cands, expect, gates=(), node=None):
        """cur / cands: dicts with d (pixel offset from the exact projection of X, default none) or xy (absolute), octave, stereo, ur_off,
        depth, hp, flips, flip_start, angle, node.  expect: run name -> None or (candidate position, kind) with kind in
        'match' (search only), 'tri', 'cur', 'nb'."""
        e = self.env
        node = self.node() if node is None else node
        base = cur.get("desc", self.descriptor())

        def place(b, pose, spec):
            uv, z = e.project(pose, X)
            xy = np.asarray(spec["xy"], np.float64) if "xy" in spec else uv + np.asarray(spec.get("d", (0, 0)), np.float64)
            kw = {}
            if spec.get("stereo"):
                kw = dict(ur=uv[0] - e.bf / z + spec.get("ur_off", 0.0), depth=spec.get("depth", z))
            return b.add(xy, spec.get("node", node), flip(base, spec.get("flips", 0), spec.get("flip_start", 0)), octave=spec.get("octave", 0),
                         hp=spec.get("hp", 0), angle=spec.get("angle", 0.0), case=name, **kw)

        h1 = place(self.cur_b, self.cur_pose, cur)
        h2 = [place(self.nb_b[nb], self.nb_pose[nb], c) for c in cands]
        nodes = {node} | {c["node"] for c in cands if "node" in c}
        self.cases.append(dict(name=name, nb=nb, X=np.asarray(X, np.float64), cur=h1, cands=h2, expect=dict(expect), gates=list(gates), nodes=nodes))
        return self.cases[-1]

    def finish(self):
        self.current = self.cur_b.finish(self.cur7, 1000 + self.seed)
        self.neighbours = [b.finish(p, 2000 + self.seed + j) if b.rows else empty_keyframe(p) for j, (b, p) in enumerate(zip(self.nb_b, self.nb7))]
        for c in self.cases:
            c["idx1"] = int(self.cur_b.index[c["cur"]])
            c["idx2"] = [int(self.nb_b[c["nb"]].index[h]) for h in c["cands"]]
        return self


def empty_keyframe(pose7):
    return dict(keys=np.zeros(0, KP), descriptors=np.zeros((0, 32), np.uint8), u_right=np.zeros(0, np.float32), depth=np.zeros(0, np.float32),
                has_point=np.zeros(0, np.uint8), fv_node=np.zeros(0, np.int32), fv_offset=np.zeros(1, np.int32), fv_index=np.zeros(0, np.int32),
                pose7=np.asarray(pose7, np.float32))


def nodes_disjoint(scene):
    """no keypoint of another case lies in a node of this case, in the current keyframe or in any neighbour"""
    for c in scene.cases:
        for b in [scene.cur_b] + scene.nb_b:
            for r in b.rows:
                if r["node"] in c["nodes"] and r["case"] != c["name"]:
                    return False
    return len({c["name"] for c in scene.cases}) == len(scene.cases)


def margin_ok(gate):
    kind, value, threshold = gate[:3]
    if kind == "cos":
        return abs(value - threshold) >= COS_MARGIN
    if kind == "band":   # the one exempt case: inside (threshold[0], threshold[1]) by a quarter of its width
        lo, hi = threshold
        return lo + 0.25 * (hi - lo) <= value <= hi - 0.25 * (hi - lo)
    scale = gate[3] if len(gate) > 3 else abs(threshold)
    return abs(value - threshold) >= REL_MARGIN * scale


def margins_ok(case):
    return all(margin_ok(g) for g in case["gates"])


# ---- geometry used to place keypoints ------------------------------------------------------------------------------------------------------
def cos_rays(env, pose1, xy1, pose2, xy2):
    a, b = env.ray(pose1, xy1), env.ray(pose2, xy2)
    return a @ b / (np.linalg.norm(a) * np.linalg.norm(b))


def bisect(f, lo, hi, target):
    """s in (lo, hi) with f(s) = target, f monotonic on it"""
    flo = f(lo) - target
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if (f(mid) - target) * flo > 0:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


def epipolar_line(env, pose1, xy1, pose2):
    """the line in image 2 of the float32 keypoint xy1 of image 1: (a point on it, unit direction, unit normal), from two points of its ray"""
    O1, d = centre(pose1), env.ray(pose1, xy1)
    p, q = env.project(pose2, O1 + 5.0 * d)[0], env.project(pose2, O1 + 50.0 * d)[0]
    t = (q - p) / np.linalg.norm(q - p)
    return p, t, np.array([-t[1], t[0]])


def unproject(env, pose, row):
    """the world point of a stored stereo keypoint (KeyFrame::UnprojectStereo), float64"""
    z = float(row["depth"])
    return pose[0].T @ (np.array([(float(row["x"]) - env.cx) * z / env.fx, (float(row["y"]) - env.cy) * z / env.fy, z]) - pose[1])


def reprojection_e2(env, pose, X, row):
    """squared reprojection error of X against a stored keypoint, with the right-image term if it is a stereo one"""
    uv, z = env.project(pose, X)
    e2 = (uv[0] - float(row["x"])) ** 2 + (uv[1] - float(row["y"])) ** 2
    return e2 + (uv[0] - env.bf / z - float(row["ur"])) ** 2 if row["ur"] >= 0 else e2


def stereo_cos(env, z):
    return np.cos(2 * np.arctan2(env.mb / 2, z))


# ---- SearchForTriangulation ----------------------------------------------------------------------------------------------------------------
SFT_RUNS = {"default": {}, "coarse": dict(coarse=True), "only_stereo": dict(only_stereo=True)}
FIRST_NODE, LAST_NODE = 1, 10 ** 6


def sft_scene(env, world):
    s = Scene(env, world, (SIDE, FWD, SIDE2), seed=11)
    e = env
    hit = lambda k=0: (k, "match")
    every = lambda v: {r: v for r in SFT_RUNS}
    gx = lambda k: s.from_cur(((k % 7 - 3) * 0.8, (k % 5 - 2) * 0.4, 8 + (k % 4) * 1.5))
    s.add("plain_match", SIDE, gx(0), {}, [{}], every(hit()) | {"only_stereo": None})
    s.add("has_point_in_current", SIDE, gx(1), dict(hp=1), [{}], every(None))
    s.add("has_point_in_neighbour", SIDE2, gx(2), {}, [dict(hp=1)], every(None))
    s.add("only_stereo_mono_in_current", SIDE, gx(3), {}, [dict(stereo=True)], every(hit()) | {"only_stereo": None})
    s.add("only_stereo_mono_in_neighbour", SIDE2, gx(4), dict(stereo=True), [{}], every(hit()) | {"only_stereo": None})
    s.add("only_stereo_both_stereo", SIDE, gx(5), dict(stereo=True), [dict(stereo=True)], every(hit()))
    s.add("same_descriptor_other_node", SIDE, gx(6), {}, [dict(node=s.node())], every(None))
    # the first and the last node of the current keyframe hold one entry each; both are matched in FWD, while SIDE and SIDE2 lack them as
    # their first node and beyond their last node (every case of another neighbour is a missing middle node)
    s.add("first_node_single_entry_missing_as_first_node_of_the_others", FWD, gx(7), dict(stereo=True), [dict(stereo=True)], every(hit()), node=FIRST_NODE)
    s.add("last_node_single_entry_missing_beyond_last_node_of_the_others", FWD, gx(8), dict(stereo=True), [dict(stereo=True)], every(hit()), node=LAST_NODE)
    s.add("node_missing_in_the_middle_of_every_neighbour", SIDE, gx(24), dict(stereo=True), [], every(None))
    s.add("hamming_50_accepted", SIDE, gx(9), {}, [dict(flips=50)], every(hit()) | {"only_stereo": None})
    s.add("hamming_51_rejected", SIDE, gx(10), {}, [dict(flips=51)], every(None))
    s.add("equal_distance_later_wins", SIDE2, gx(11), dict(stereo=True), [dict(flips=7, stereo=True), dict(flips=7, flip_start=100, stereo=True)], every(hit(1)))
    far_off = 3.0 * np.sqrt(3.84)
    c = s.add("failing_candidate_keeps_best_dist", SIDE, gx(12), dict(stereo=True),
              [dict(flips=10, stereo=True), dict(flips=5, flip_start=60, stereo=True), dict(flips=8, flip_start=120, stereo=True)],
              every(hit(2)) | {"coarse": hit(1)})
    _, _, nrm = epipolar_line(e, s.cur_pose, s.cur_b.xy(c["cur"]), s.nb_pose[SIDE])     # push the d = 5 candidate off the line
    row = s.nb_b[SIDE].rows[c["cands"][1]]
    row["x"], row["y"] = np.float32(row["x"] + far_off * nrm[0]), np.float32(row["y"] + far_off * nrm[1])
    c["gates"].append(("rel", far_off ** 2, 3.84))

    # epipole proximity (FWD: the epipole lies inside the image); the candidate is placed first, the current keypoint is the projection of a
    # point of the candidate's ray, so the epipolar test is met exactly
    pose2 = s.nb_pose[FWD]
    ep = e.project(pose2, centre(s.cur_pose))[0]
    assert 0 < ep[0] < W and 0 < ep[1] < H

    def near_epipole(name, D, ang, octave, stereo1, stereo2, want):
        xy2 = ep + D * np.array([np.cos(ang), np.sin(ang)])
        X = centre(pose2) + 9.0 * e.ray(pose2, xy2)
        c = s.add(name, FWD, X, dict(stereo=stereo1, octave=octave), [dict(xy=xy2, octave=octave, stereo=stereo2)],
                  {"default": want, "coarse": want, "only_stereo": want if (stereo1 and stereo2) else None})
        c["gates"].append(("rel", float(np.sum((s.nb_b[FWD].xy(c["cands"][0]) - ep) ** 2)), 100.0 * float(e.sf[octave])))
    near_epipole("epipole_mono_mono_near_rejected", 0.9 * 10.0, 0.3, 0, False, False, None)
    near_epipole("epipole_near_accepted_current_stereo", 0.9 * 10.0, 1.4, 0, True, False, hit())
    near_epipole("epipole_near_accepted_neighbour_stereo", 0.9 * 10.0, 2.5, 0, False, True, hit())
    near_epipole("epipole_14px_octave0_accepted", 14.0, 3.6, 0, False, False, hit())
    near_epipole("epipole_14px_octave7_rejected", 14.0, 4.7, 7, False, False, None)

    # epipolar distance (SIDE): offsets perpendicular to the float64 epipolar line of the stored current keypoint
    def off_line(name, k, off, octave, want):
        c = s.add(name, SIDE, gx(k), dict(octave=octave), [dict(octave=octave)], {"default": want, "coarse": hit(), "only_stereo": None})
        on, _, nrm = epipolar_line(e, s.cur_pose, s.cur_b.xy(c["cur"]), s.nb_pose[SIDE])
        row = s.nb_b[SIDE].rows[c["cands"][0]]
        row["x"], row["y"] = np.float32(row["x"] + off * nrm[0]), np.float32(row["y"] + off * nrm[1])
        c["gates"].append(("rel", float((s.nb_b[SIDE].xy(c["cands"][0]) - on) @ nrm) ** 2, 3.84 * float(e.sg[octave])))
    for octave in (0, 7):
        lim = np.sqrt(3.84 * float(e.sg[octave]))
        off_line("epipolar_0.5_octave%d_accepted" % octave, 13 + octave, 0.5 * lim, octave, hit())
        off_line("epipolar_1.5_octave%d_rejected" % octave, 14 + octave, -1.5 * lim, octave, None)
    off_line("epipolar_4px_octave0_rejected", 22, 4.0, 0, None)
    off_line("epipolar_4px_octave7_accepted", 23, 4.0, 7, hit())
    return s.finish()


def same_pose_scene(env, world):
    """both keyframes at one pose: t12 = 0.  In the identity world F12 is exactly zero in every arithmetic (den == 0: no match unless coarse);
    under a rotated pose t12 is the rounding noise of T1 * T1^-1, which float64 does not reproduce, so only the coarse run is defined there."""
    cur7 = current_pose7(world)
    s = Scene(env, world, (SIDE,), seed=12, poses7=[cur7.copy()])
    for k in range(4):
        s.add("same_pose_%d" % k, 0, s.from_cur(((k - 1.5) * 0.9, 0.3 * (k % 2), 7.0 + k)), dict(stereo=True), [dict(stereo=True)],
              {"default": None, "coarse": (0, "match")})
    return s.finish()


def rotation_histogram_scene(env, world, majority=20):
    """check_orientation.  majority = 20: 20 matches in bin 0 (one of them 14.9 degrees, one through the rot < 0 wrap, one with rot = 900 that
    the bin == 30 fold sends to bin 0), 2 in bin 1 (15.1 and 44.9: exactly 10 % of the largest, kept), 1 in bin 2 (45.1) and 1 in bin 12 (350,
    through the wrap): removed.  majority = 21: 21, 3 in bin 1 (kept) and 2 in bin 2 (9.5 %, just under 10 %: removed), 1 in bin 12."""
    s = Scene(env, world, (SIDE,), seed=13)
    extra = majority - 20
    angles = [(40.0, 40.0)] * (17 + extra) + [(54.9, 40.0), (5.0, 355.0), (900.0, 0.0), (55.1, 40.0), (84.9, 40.0)] + [(60.0, 40.0)] * extra + \
             [(85.1, 40.0)] + [(100.0, 40.0)] * extra + [(10.0, 20.0)]
    keep = [True] * (majority + 2 + extra) + [False] * (2 + extra)
    assert len(angles) == len(keep)
    for k, ((a1, a2), kept) in enumerate(zip(angles, keep)):
        s.add("rot_%02d_%s" % (k, "kept" if kept else "removed"), 0, s.from_cur((((k * 5) % 9 - 4) * 0.6, (k % 4 - 1.5) * 0.3, 7.0 + (k % 5))),
              dict(stereo=True, angle=a1), [dict(stereo=True, angle=a2)], {"default": (0, "match"), "oriented": (0, "match") if kept else None})
    return s.finish()


# ---- CreateNewMapPoints --------------------------------------------------------------------------------------------------------------------
CNMP_RUNS = {"default": {}, "inertial": dict(inertial=True)}
TH_FAR = 10.0
FAR_RUNS = {"far": dict(far_points=True, th_far_points=TH_FAR), "default": {}}


def cnmp_scene(env, world):
    s = Scene(env, world, (SIDE, FWD, SIDE2, BACK, FACING), seed=21)
    e = env
    both = lambda v: {r: v for r in CNMP_RUNS}
    O1 = centre(s.cur_pose)
    fwd = s.cur_pose[0].T @ np.array([0.0, 0.0, 1.0])
    O2 = centre(s.nb_pose[SIDE])
    bhat = (O2 - O1) / np.linalg.norm(O2 - O1)

    # mono - mono parallax: the point on a ray of the current keyframe at which the rays to both centres meet at the wanted angle
    def at_parallax(name, uv, target, want):
        d = e.ray(s.cur_pose, uv)
        d /= np.linalg.norm(d)
        f = lambda z: ((O1 + z * d - O1) @ (O1 + z * d - O2)) / (z * np.linalg.norm(O1 + z * d - O2))
        X = O1 + bisect(f, 3.0, 500.0, target) * d
        c = s.add(name, SIDE, X, {}, [{}], want)
        cr = cos_rays(e, s.cur_pose, s.cur_b.xy(c["cur"]), s.nb_pose[SIDE], s.nb_b[SIDE].xy(c["cands"][0]))
        c["gates"] += [("cos", cr, 0.9996), ("cos", cr, 0.9998)]
    at_parallax("mono_mono_cos_0.9997_only_without_inertial", (300.0, 120.0), 0.9997, {"default": (0, "tri"), "inertial": None})
    at_parallax("mono_mono_cos_0.99985_dropped", (500.0, 200.0), 0.99985, both(None))
    at_parallax("mono_mono_cos_0.9990_created", (420.0, 90.0), 0.9990, both((0, "tri")))

    # rays more than 90 degrees apart: BACK looks the other way; the candidate sits on the epipolar line, far from the epipole
    xy1 = np.array([350.0, 140.0])
    Xb = O1 + 8.0 * e.ray(s.cur_pose, np.float32(xy1))
    p, t, _ = epipolar_line(e, s.cur_pose, np.float32(xy1), s.nb_pose[BACK])
    epb = e.project(s.nb_pose[BACK], O1)[0]
    xy2 = p + 40.0 * t if np.linalg.norm(p + 40.0 * t - epb) > np.linalg.norm(p - 40.0 * t - epb) else p - 40.0 * t
    c = s.add("mono_mono_rays_over_90_degrees_dropped", BACK, Xb, dict(xy=xy1), [dict(xy=xy2)], both(None))
    assert cos_rays(e, s.cur_pose, np.float32(xy1), s.nb_pose[BACK], np.float32(xy2)) < 0
    c["gates"] += [("cos", cos_rays(e, s.cur_pose, np.float32(xy1), s.nb_pose[BACK], np.float32(xy2)), 0.0),
                   ("rel", float(np.sum((xy2 - epb) ** 2)), 100.0)]

    # ... and the case in which nothing but cosRays > 0 stands in the way: a point between the current keyframe and FACING, in front of both,
    # exact projections on both sides (chi-square 0), equal octaves, distances 3.05 m and 3.02 m; the rays meet head-on
    Xf = s.from_cur((0.5, -0.2, 3.0))
    c = s.add("mono_mono_rays_head_on_only_the_cos_gate_drops_it", FACING, Xf, {}, [{}], both(None))
    crf = cos_rays(e, s.cur_pose, s.cur_b.xy(c["cur"]), s.nb_pose[FACING], s.nb_b[FACING].xy(c["cands"][0]))
    epf = e.project(s.nb_pose[FACING], O1)[0]
    assert crf < 0 and e.project(s.cur_pose, Xf)[1] > 1 and e.project(s.nb_pose[FACING], Xf)[1] > 1
    c["gates"] += [("cos", crf, 0.0), ("rel", float(np.sum((s.nb_b[FACING].xy(c["cands"][0]) - epf) ** 2)), 100.0)]

    # stereo parallax against ray parallax
    Xhi = s.from_cur((-1.0, 0.4, 8.0))
    c = s.add("stereo1_rays_wider_than_stereo_triangulated", SIDE, Xhi, dict(stereo=True), [{}], both((0, "tri")))
    c["gates"].append(("cos", cos_rays(e, s.cur_pose, s.cur_b.xy(c["cur"]), s.nb_pose[SIDE], s.nb_b[SIDE].xy(c["cands"][0])), stereo_cos(e, 8.0)))
    low = lambda k: s.from_cur((0.5 + 0.35 * (k % 5) - 0.7, 0.3 - 0.2 * (k % 3), 10.0 + 0.5 * (k % 4)))   # close to the axis: little parallax towards FWD

    def low_gate(c, z, side="cur"):
        cr = cos_rays(e, s.cur_pose, s.cur_b.xy(c["cur"]), s.nb_pose[FWD], s.nb_b[FWD].xy(c["cands"][0]))
        c["gates"].append(("cos", cr, stereo_cos(e, z)))
        assert cr > stereo_cos(e, z)
    c = s.add("stereo1_rays_narrower_unprojected_from_current", FWD, low(0), dict(stereo=True), [{}], both((0, "cur")))
    low_gate(c, e.project(s.cur_pose, low(0))[1])
    c = s.add("mono1_stereo2_unprojected_from_neighbour", FWD, low(1), {}, [dict(stereo=True)], both((0, "nb")))
    low_gate(c, e.project(s.nb_pose[FWD], low(1))[1])
    z2 = e.project(s.nb_pose[FWD], low(2))[1]
    c = s.add("both_stereo_neighbour_depth_smaller_still_from_current", FWD, low(2), dict(stereo=True), [dict(stereo=True, depth=0.8 * z2)], both((0, "cur")))
    low_gate(c, e.project(s.cur_pose, low(2))[1])
    s.add("u_right_without_depth_nothing_created", FWD, low(3), dict(stereo=True, depth=-1.0), [{}], both(None))

    # a wrong correspondence beyond the point at infinity of the current keypoint's ray: the triangulation falls behind the cameras
    xy1 = np.array([280.0, 210.0])
    Xi = O1 + 9.0 * e.ray(s.cur_pose, np.float32(xy1))
    d1 = e.ray(s.cur_pose, np.float32(xy1))
    v_inf = e.project(s.nb_pose[SIDE], O2 + d1)[0]
    p9 = e.project(s.nb_pose[SIDE], Xi)[0]
    xy2 = v_inf + 1.5 * (v_inf - p9)
    c = s.add("beyond_infinity_lands_behind_dropped", SIDE, Xi, dict(xy=xy1), [dict(xy=xy2)], both(None))
    c["gates"].append(("cos", cos_rays(e, s.cur_pose, np.float32(xy1), s.nb_pose[SIDE], np.float32(xy2)), 0.9996))

    # reprojection gates: the point is un-projected from one side, so the error of the other keypoint is what its offset says; offsets run
    # along the epipolar lines, which keeps the epipolar test met
    oct_r = 2
    sig = float(e.sg[oct_r])

    def along(pose_a, pose_b, X):  # unit direction in image a of the epipolar line through the projection of X (away from the epipole)
        pa, ea = e.project(pose_a, X)[0], e.project(pose_a, centre(pose_b))[0]
        return (pa - ea) / np.linalg.norm(pa - ea)
    def measured(c, source, side, limits):
        """the gates of a reprojection case: the error of the stored keypoint of `side` against the point un-projected from the stored keypoint of `source`"""
        rows = {"cur": (s.cur_pose, s.cur_b.rows[c["cur"]]), "nb": (s.nb_pose[FWD], s.nb_b[FWD].rows[c["cands"][0]])}
        X = unproject(e, *rows[source])
        e2 = reprojection_e2(e, rows[side][0], X, rows[side][1])
        c["gates"] += [("rel", e2, lim * sig) for lim in limits]
    k = 4
    for f, tag in ((0.5, "accepted"), (1.5, "rejected")):
        X = low(k); k += 1
        off = np.sqrt(f * 5.991 * sig)
        c = s.add("reproj_mono_current_%.1f_%s" % (f, tag), FWD, X, dict(octave=oct_r, d=off * along(s.cur_pose, s.nb_pose[FWD], X)), [dict(octave=oct_r, stereo=True)],
                  both((0, "nb") if f < 1 else None))
        measured(c, "nb", "cur", (5.991,))
        X = low(k); k += 1
        c = s.add("reproj_mono_neighbour_%.1f_%s" % (f, tag), FWD, X, dict(octave=oct_r, stereo=True), [dict(octave=oct_r, d=off * along(s.nb_pose[FWD], s.cur_pose, X))],
                  both((0, "cur") if f < 1 else None))
        measured(c, "cur", "nb", (5.991,))
        offs = np.sqrt(f * 7.8 * sig)
        X = low(k); k += 1
        c = s.add("reproj_stereo_current_u_right_%.1f_%s" % (f, tag), FWD, X, dict(octave=oct_r, stereo=True, ur_off=offs), [dict(octave=oct_r)],
                  both((0, "cur") if f < 1 else None))
        measured(c, "cur", "cur", (7.8,))
        X = low(k); k += 1
        c = s.add("reproj_stereo_neighbour_u_right_%.1f_%s" % (f, tag), FWD, X, dict(octave=oct_r, stereo=True), [dict(octave=oct_r, stereo=True, ur_off=-offs)],
                  both((0, "cur") if f < 1 else None))
        measured(c, "cur", "nb", (7.8,))
    offm = np.sqrt(6.9 * sig)
    for stereo2, want in ((False, None), (True, (0, "cur"))):
        X = low(k); k += 1
        c = s.add("reproj_6.9_sigma2_%s" % ("stereo_neighbour_accepted" if stereo2 else "mono_neighbour_rejected"), FWD, X, dict(octave=oct_r, stereo=True),
                  [dict(octave=oct_r, stereo=stereo2, d=offm * along(s.nb_pose[FWD], s.cur_pose, X))], both(want))
        measured(c, "cur", "nb", (5.991, 7.8))

    # scale consistency (ratioFactor = 1.5 * 1.2): equal distances with octave steps, equal octaves with distance ratios
    perp = fwd - (fwd @ bhat) * bhat
    perp /= np.linalg.norm(perp)
    for n, (o1, o2) in enumerate(((3, 0), (0, 3), (4, 0), (0, 4))):
        X = 0.5 * (O1 + O2) + (7.0 + n) * perp + 0.3 * n * np.cross(bhat, perp)
        s.add("scale_octaves_%d_%d_%s" % (o1, o2, "accepted" if abs(o1 - o2) == 3 else "rejected"), SIDE, X, dict(octave=o1), [dict(octave=o2)],
              both((0, "tri") if abs(o1 - o2) == 3 else None), gates=[("rel", 1.2 ** abs(o1 - o2), 1.8)])
    b = np.linalg.norm(O2 - O1)
    for ratio in (1.7, 1 / 1.7, 1.9, 1 / 1.9):
        # a point of the sphere of Apollonius dist_far = k dist_near, 60 degrees round it from the baseline towards the viewing direction
        k = max(ratio, 1 / ratio)
        along_b = b * (k * k / (k * k - 1) + k / (k * k - 1) * np.cos(np.deg2rad(60)))
        up = b * k / (k * k - 1) * np.sin(np.deg2rad(60)) * perp
        X = (O2 - along_b * bhat + up) if ratio > 1 else (O1 + along_b * bhat + up)
        assert abs(np.linalg.norm(X - O2) / np.linalg.norm(X - O1) - ratio) < 1e-9
        ok = max(ratio, 1 / ratio) < 1.8
        s.add("scale_distance_ratio_%.3f_%s" % (ratio, "accepted" if ok else "rejected"), SIDE, X, {}, [{}], both((0, "tri") if ok else None),
              gates=[("rel", max(ratio, 1 / ratio), 1.8)])
    return s.finish()


def far_scene(env, world):
    s = Scene(env, world, (SIDE,), seed=22)
    O1, O2 = centre(s.cur_pose), centre(s.nb_pose[0])
    fwd = s.cur_pose[0].T @ np.array([0.0, 0.0, 1.0])
    bhat = (O2 - O1) / np.linalg.norm(O2 - O1)
    unit = lambda v: v / np.linalg.norm(v)
    for name, X, far in (("far_within_current_beyond_neighbour", O1 + 9.8 * unit(fwd - 0.6 * bhat), None),
                         ("far_beyond_current_within_neighbour", O2 + 9.8 * unit(fwd + 0.6 * bhat), None),
                         ("far_both_within", O1 + 9.0 * unit(fwd + 0.1 * bhat), (0, "tri"))):
        s.add(name, 0, X, {}, [{}], {"far": far, "default": (0, "tri")},
              gates=[("rel", np.linalg.norm(X - O1), TH_FAR), ("rel", np.linalg.norm(X - O2), TH_FAR)])
    return s.finish()


def baseline_scene(env, world, factor):
    """one neighbour at factor x mb from the current keyframe (LocalMapping.cc:458-465), mono keypoints that triangulate when it is kept.  The
    offset runs along (I - dR) tcw of the rotated world, towards it for 1.1 and away from it for 0.9: there |tcw2 - tcw1| = |c - (I - dR) tcw|
    falls on the other side of mb than the distance of the centres, so the baseline has to come from Ow."""
    cur7 = current_pose7(world)
    Rr, tr = pose_Rt(current_pose7("rotated"))
    w = (np.eye(3) - rodrigues(OBLIQUE, NB_TURN[SIDE])) @ tr
    c = (1.0 if factor > 1 else -1.0) * factor * env.mb * w / np.linalg.norm(w)
    s = Scene(env, world, (SIDE,), seed=23, poses7=[neighbour_pose7(world, cur7, SIDE, c=c)])
    want = (0, "tri") if factor > 1 else None
    between = np.linalg.norm(centre(s.nb_pose[0]) - centre(s.cur_pose))
    gates = [("rel", between, env.mb)]
    if world == "rotated":
        dt = np.linalg.norm(s.nb_pose[0][1] - s.cur_pose[1])
        assert (dt - env.mb) * (between - env.mb) < 0
        gates.append(("rel", dt, env.mb))
    for k in range(3):
        s.add("baseline_%.1f_mb_%d" % (factor, k), 0, s.from_cur(((k - 1) * 0.7, 0.2 * k, 9.0 + k)), {}, [{}], {"default": want}, gates=gates)
    return s.finish()


def first_neighbour_scene(env, world):
    """neighbours FWD(0), SIDE(1), SIDE2(2): the first neighbour that yields a point keeps the keypoint"""
    s = Scene(env, world, (FWD, SIDE, SIDE2), seed=24)
    X = s.from_cur((-0.6, 0.3, 8.0))
    n = s.node()
    c = s.add("succeeds_with_1_and_2_reported_for_1", 1, X, {}, [{}], {"default": (0, "tri")}, node=n)
    uv2 = env.project(s.nb_pose[2], X)[0]
    s.nb_b[2].add(uv2, n, s.cur_b.rows[c["cur"]]["desc"], case=c["name"])
    X = s.from_cur((1.5, -0.4, 9.0))
    n = s.node()
    c = s.add("matched_but_dropped_with_0_succeeds_with_1", 1, X, {}, [{}], {"default": (0, "tri")}, node=n)
    uv0 = env.project(s.nb_pose[0], X)[0]
    s.nb_b[0].add(uv0, n, s.cur_b.rows[c["cur"]]["desc"], octave=5, case=c["name"])      # matched in neighbour 0: too little parallax, and five octaves apart
    for k in range(4):   # more records, so that the order (neighbour-major, keypoint-ascending) shows
        s.add("order_%d" % k, 2 - (k % 2) * 2 if k < 2 else 1, s.from_cur((0.4 * k - 1.0, 0.5 - 0.3 * k, 7.0 + k)), dict(stereo=True), [{}], {})
    return s.finish()


# ---- the compaction problem of the batch entry ---------------------------------------------------------------------------------------------
COMPACT_KEYS, COMPACT_NEIGHBOURS = 130, 70
COMPACT_OWNERS = (0, 3, 4, 63, 64, 69, 7, 12, 33, 68)
COMPACT_SKIPPED = (1, 40)          # neighbours nearer than the stereo baseline: they hold matches and yield nothing


def compaction_problem(env):
    """A current keyframe of 130 keypoints (64 + 64 + 2) and 70 neighbours for k_new_points_compact: the neighbour that shall own each
    keypoint is prescribed (`first`, -1 = none).  Neighbour 4 owns keypoints of all three 64-wide strides; 21 neighbours are empty or own
    nothing; an owned keypoint is also present in later neighbours, in an earlier neighbour behind has_point, and in a skipped neighbour."""
    world = "rotated"
    cur7 = current_pose7(world)
    poses = []
    for j in range(COMPACT_NEIGHBOURS):
        a = 2 * np.pi * j / COMPACT_NEIGHBOURS
        c = np.array([np.cos(a), 0.6 * np.sin(a), 0.15 * np.sin(2 * a)]) * (0.3 if j in COMPACT_SKIPPED else 1.0)
        poses.append(neighbour_pose7(world, cur7, SIDE, c=c, turn=3.0 + j % 5))
    s = Scene(env, world, [SIDE] * COMPACT_NEIGHBOURS, seed=31, poses7=poses)
    first = np.full(COMPACT_KEYS, -1, np.int64)
    for i in range(COMPACT_KEYS):
        X = s.from_cur(((i % 13 - 6) * 0.5, (i % 7 - 3) * 0.35, 7.0 + i % 5))
        node, desc = s.node(), s.descriptor()
        uv = env.project(s.cur_pose, X)[0]
        cur_hp = int(i % 17 == 3)
        s.cur_b.add(uv, node, desc, hp=cur_hp, case="k%d" % i)
        own = 4 if i in (5, 70, 129) else COMPACT_OWNERS[(i * 7) % len(COMPACT_OWNERS)]
        never = i % 13 == 0
        present = {} if never else {own: 0}
        if not never:
            for later in (own + 1, own + 5):
                if later < COMPACT_NEIGHBOURS:
                    present[later] = 0
        if i % 5 == 0 and own > 0:
            present[0] = 1                                 # an earlier neighbour holds the match behind has_point
        if never:
            present[2] = 1
        if i % 4 == 0:
            present[COMPACT_SKIPPED[(i // 4) % 2]] = 0
        for j, hp in present.items():
            s.nb_b[j].add(env.project(s.nb_pose[j], X)[0], node, desc, hp=hp, case="k%d" % i)
        if not never and not cur_hp:
            first[i] = min(j for j, hp in present.items() if not hp and j not in COMPACT_SKIPPED)
    s.finish()
    s.first = np.array([first[np.nonzero(s.cur_b.index == i)[0][0]] for i in range(COMPACT_KEYS)])   # by keypoint index
    return s


# ---- a random rotated scene with a known answer --------------------------------------------------------------------------------------------
def random_scene(env, n_points=150, seed=41):
    """150 world points seen from the rotated current keyframe and FWD, SIDE, SIDE2, exact projections rounded to float32; every third
    keypoint mono.  -> (scene, X [n, 3], index [1 + 3][n]: the keypoint of point p in each keyframe)"""
    s = Scene(env, "rotated", (FWD, SIDE, SIDE2), seed=seed)
    rng = np.random.default_rng(seed)
    Xc = np.stack([rng.uniform(-3, 3, n_points), rng.uniform(-1, 1, n_points), rng.uniform(4, 12, n_points)], 1)
    Xs, handles = [], []
    for p in range(n_points):
        X = s.from_cur(Xc[p])
        node, desc = (p % 10) * 7 + 3, s.descriptor()
        hs = []
        for b, pose in zip([s.cur_b] + s.nb_b, [s.cur_pose] + s.nb_pose):
            uv, z = env.project(pose, X)
            kw = dict(ur=uv[0] - env.bf / z, depth=z) if (p + len(hs)) % 3 else {}
            hs.append(b.add(uv, node, desc, octave=2, case="p%d" % p, **kw))
        Xs.append(X); handles.append(hs)
    s.finish()
    index = np.array([[int(b.index[h[k]]) for h in handles] for k, b in enumerate([s.cur_b] + s.nb_b)])
    return s, np.array(Xs), index


def random_fuse_points(env, s, X, index, k):
    """the world points as map points seen from keyframe k (0 = current)"""
    pose = ([s.cur_pose] + s.nb_pose)[k]
    kf = ([s.current] + s.neighbours)[k]
    pts = np.zeros(len(X), MP)
    pts["pos"] = X.astype(np.float32)
    PO = X - centre(s.cur_pose)
    dist = np.linalg.norm(PO, axis=1)
    pts["normal"] = (PO / dist[:, None]).astype(np.float32)
    pts["min_distance"], pts["max_distance"] = (0.5 * dist).astype(np.float32), (2.0 * dist).astype(np.float32)
    dk = np.linalg.norm(X - centre(pose), axis=1)
    pts["max_distance_raw"] = (dk * 1.2 ** 1.5).astype(np.float32)          # level 2 in the keyframe it is fused into
    pts["descriptor"] = kf["descriptors"][index[k]]
    return kf, pts


def true_point_tolerance(env, scene, X, j):
    """How far a created point may lie from the true one: each of the two rays is known to a few float32 roundings (the pixel, the
    normalisation, the rotation, the translation -- 8 units of 2^-24 each, 16 together) of the distance, and the intersection magnifies
    that by 1 / sin(parallax); a stereo un-projection carries the same roundings without the magnification."""
    O1, O2 = centre(scene.cur_pose), centre(scene.nb_pose[j])
    a, b = X - O1, X - O2
    sin_p = np.linalg.norm(np.cross(a, b)) / (np.linalg.norm(a) * np.linalg.norm(b))
    return 16 * 2.0 ** -24 * max(np.linalg.norm(a), np.linalg.norm(b)) * (1 + 1 / sin_p)


# ---- Fuse ----------------------------------------------------------------------------------------------------------------------------------
FUSE_RUNS = {"th3": 3.0, "th1.5": 1.5}


class FuseScene:
    """one keyframe (keypoint index = order of creation), map points, and per case the (best_idx, best_dist) it is made for"""

    def __init__(self, env, world, bounds, seed=51):
        self.env, self.world, self.bounds = env, world, tuple(float(np.float32(b)) for b in bounds)
        self.pose7 = current_pose7(world)
        self.pose = pose_Rt(self.pose7)
        self.b = KfBuilder()
        self.rng = np.random.default_rng(seed)
        self.points, self.valid, self.cases = [], [], []
        self.cell_w, self.cell_h = (self.bounds[1] - self.bounds[0]) / GRID_COLS, (self.bounds[3] - self.bounds[2]) / GRID_ROWS
        self._slot = 0

    def slot(self):
        """the next free place of a 17 x 6 lattice inside the image, 40 pixels or more between places"""
        k = self._slot
        self._slot += 1
        assert k < 17 * 6
        return np.array([self.bounds[0] + 60.0 + 44.0 * (k % 17), self.bounds[2] + 42.0 + 43.0 * (k // 17)])

    def point(self, uv0=None, z=9.0, level=3, normal_deg=20.0, min_f=0.5, max_f=2.0, level_pow=None, xc=None):
        """a map point that projects to uv0 at depth z (or lies at xc in the camera frame); -> (record, projection of the float32 position, depth, dist3D)"""
        e = self.env
        if xc is None:
            xc = np.array([(uv0[0] - e.cx) * z / e.fx, (uv0[1] - e.cy) * z / e.fy, z])
        R, t = self.pose
        rec = np.zeros((), MP)
        rec["pos"] = (R.T @ (np.asarray(xc, np.float64) - t)).astype(np.float32)
        X = rec["pos"].astype(np.float64)
        PO = X - centre(self.pose)
        dist = np.linalg.norm(PO)
        side = np.cross(PO, [0.3, 0.5, 0.8])
        a = np.deg2rad(normal_deg)
        rec["normal"] = (np.cos(a) * PO / dist + np.sin(a) * side / np.linalg.norm(side)).astype(np.float32)
        def clear(v):   # 0.999 x / 1.001 x of a float32 end lie 1e-3 from it up to its rounding: step the end until the margin holds
            while abs(dist / float(v) - 1) < REL_MARGIN:
                v = np.nextafter(v, np.float32(0 if dist > float(v) else np.inf))
            return v
        rec["min_distance"], rec["max_distance"] = clear(np.float32(dist * min_f)), clear(np.float32(dist * max_f))
        rec["max_distance_raw"] = np.float32(dist * 1.2 ** ((level - 0.5) if level_pow is None else level_pow))
        rec["descriptor"] = self.rng.integers(0, 256, 32, dtype=np.uint8)
        uv, zc = e.project(self.pose, X)
        return rec, uv, zc, dist

    def add(self, name, rec, uv, zc, keypoints, expect, th=3.0, gates=(), valid=1):
        """keypoints: dicts with d (offset from uv) or xy, octave, stereo, ur_off, flips; expect: (position in keypoints or -1, best_dist)"""
        e = self.env
        idx = []
        for kp in keypoints:
            xy = np.asarray(kp["xy"], np.float64) if "xy" in kp else uv + np.asarray(kp.get("d", (0, 0)), np.float64)
            kw = dict(ur=uv[0] - e.bf / zc + kp.get("ur_off", 0.0), depth=zc) if kp.get("stereo") else {}
            idx.append(self.b.add(xy, 0, flip(rec["descriptor"], kp.get("flips", 0), kp.get("flip_start", 0)), octave=kp.get("octave", 3), case=name, **kw))
        self.points.append(rec); self.valid.append(valid)
        gates = [(g[0], self.measure(rec, uv, zc, self.b.rows[idx[0]], g[1])) + tuple(g[2:]) if isinstance(g[1], str) else g for g in gates]
        self.cases.append(dict(name=name, point=len(self.points) - 1, uv=uv, keys=idx, th=th, gates=list(gates), valid=valid,
                               expect=(idx[expect[0]] if expect[0] >= 0 else -1, expect[1])))

    def measure(self, rec, uv, zc, row, what):
        """a gate quantity in float64 from the stored float32 point and keypoint"""
        e = self.env
        PO = rec["pos"].astype(np.float64) - centre(self.pose)
        dist = np.linalg.norm(PO)
        ex, ey = uv[0] - float(row["x"]), uv[1] - float(row["y"])
        if what == "chi2":
            er = (uv[0] - e.bf / zc - float(row["ur"])) if row["ur"] >= 0 else 0.0
            return (ex * ex + ey * ey + er * er) * float(e.isg[row["octave"]])
        return {"dx": abs(ex), "dy": abs(ey), "min_ratio": dist / float(rec["min_distance"]), "max_ratio": dist / float(rec["max_distance"]),
                "normal": PO @ rec["normal"].astype(np.float64) / dist}[what]

    def finish(self):
        self.kf = self.b.finish(self.pose7, 0, shuffle=False)
        self.points = np.array(self.points, MP)
        self.valid = np.array(self.valid, np.uint8)
        return self

    def valid_for(self, run):
        return np.array([c["valid"] and c["th"] == FUSE_RUNS[run] for c in self.cases], np.uint8)

    def expected(self, run):
        on = self.valid_for(run)
        return (np.array([c["expect"][0] if o else -1 for c, o in zip(self.cases, on)], np.int32),
                np.array([c["expect"][1] if o else 256 for c, o in zip(self.cases, on)], np.int32))


def fuse_isolated(scene):
    """no keypoint of another case within twice the largest search radius (th 3, level 7) of a case's projection"""
    reach = 2 * 3.0 * float(scene.env.sf[7])
    for c in scene.cases:
        if c["uv"] is None or not np.all(np.isfinite(c["uv"])):
            continue
        for r in scene.b.rows:
            if r["case"] != c["name"] and max(abs(float(r["x"]) - c["uv"][0]), abs(float(r["y"]) - c["uv"][1])) < reach:
                return False
    return len({c["name"] for c in scene.cases}) == len(scene.cases)


def fuse_scene(env, world, bounds=BOUNDS0):
    s = FuseScene(env, world, bounds)
    e = env
    min_x, max_x, min_y, max_y = s.bounds
    ext_x, ext_y = max_x - min_x, max_y - min_y
    sf, sg = [float(v) for v in e.sf], [float(v) for v in e.sg]
    HIT, MISS = (0, 0), (-1, 256)

    def simple(name, expect, kps=None, th=3.0, gates=(), valid=1, uv0=None, **pk):
        rec, uv, zc, dist = s.point(s.slot() if uv0 is None else uv0, **pk)
        s.add(name, rec, uv, zc, [dict()] if kps is None else kps, expect, th=th, gates=gates, valid=valid)
        return dist
    simple("plain_fused", HIT)
    simple("valid_0_returns_minus1_256", MISS, valid=0)
    # behind the camera, 5 m: a matching keypoint of the predicted level sits at the mirrored projection fx x / z + cx, fy y / z + cy of the
    # stored position, inside the image, and the distance and normal gates are met, so that nothing but z < 0 keeps it from being fused
    u0 = s.slot()
    rec, uv, zc, _ = s.point(xc=(-(u0[0] - e.cx) * 5.0 / e.fx, -(u0[1] - e.cy) * 5.0 / e.fy, -5.0))
    assert zc < -4 and np.abs(uv - u0).max() < 1e-3
    s.add("behind_the_camera_z_negative", rec, uv, zc, [dict()], MISS, gates=[("rel", "min_ratio", 1.0), ("rel", "max_ratio", 1.0), ("rel", "normal", 0.5)])
    # image bounds: a point 1 px (x) / 0.5 px (y) inside and outside each bound, a fusable octave 7 keypoint beside it (PosInGrid keeps no
    # keypoint in the last half cell before max_x / max_y, so the keypoint lies 0.55 cells inside those)
    mid_u, mid_v = min_x + 0.37 * ext_x, min_y + 0.41 * ext_y
    for name, axis, bound, sign, inward, ext in (("min_x", 0, min_x, 1, 1.5, ext_x), ("max_x", 0, max_x, -1, 0.55 * s.cell_w, ext_x),
                                                 ("min_y", 1, min_y, 1, 1.5, ext_y), ("max_y", 1, max_y, -1, 0.55 * s.cell_h, ext_y)):
        step = 1.0 if axis == 0 else 0.5
        for inside in (True, False):
            other = (mid_v if axis == 0 else mid_u) + (60.0 if sign < 0 else 0.0) + (0.0 if inside else 30.0)
            p, kxy = np.zeros(2), np.zeros(2)
            p[axis], p[1 - axis] = bound + sign * step * (1 if inside else -1), other
            kxy[axis], kxy[1 - axis] = bound + sign * inward, other
            rec, uv, zc, _ = s.point(p, level=7)
            s.add("bound_%s_%s" % (name, "inside_fused" if inside else "outside_dropped"), rec, uv, zc, [dict(xy=kxy, octave=7)], HIT if inside else MISS,
                  gates=[("rel", uv[axis], bound, ext)])
    # distance ends and the 60 degree normal gate
    for f, want in ((0.999, MISS), (1.001, HIT)):
        simple("dist_%.3f_of_min_distance" % f, want, min_f=1 / f, gates=[("rel", "min_ratio", 1.0)])
    for f, want in ((0.999, HIT), (1.001, MISS)):
        simple("dist_%.3f_of_max_distance" % f, want, max_f=1 / f, gates=[("rel", "max_ratio", 1.0)])
    simple("normal_59_degrees_fused", HIT, normal_deg=59.0, gates=[("rel", "normal", 0.5)])
    simple("normal_61_degrees_dropped", MISS, normal_deg=61.0, gates=[("rel", "normal", 0.5)])
    # predicted level: clamps and the level - 1 .. level window
    simple("level_negative_clamps_to_0_octave0_fused", HIT, [dict(octave=0)], level_pow=-2.5)
    simple("level_negative_clamps_to_0_octave1_dropped", MISS, [dict(octave=1)], level_pow=-2.5)
    simple("level_huge_clamps_to_7_octave7_fused", HIT, [dict(octave=7)], level_pow=12.5)
    simple("level_huge_clamps_to_7_octave6_fused", HIT, [dict(octave=6)], level_pow=12.5)
    simple("level_huge_clamps_to_7_octave5_dropped", MISS, [dict(octave=5)], level_pow=12.5)
    for octave, want in ((2, MISS), (3, HIT), (4, HIT), (5, MISS)):
        simple("level_4_octave_%d_%s" % (octave, "fused" if want is HIT else "dropped"), want, [dict(octave=octave)], level=4)
    # window gate, th = 1.5: it binds before chi-square ((1.07 * 1.5)^2 = 2.6 < 5.99)
    r = 1.5 * sf[3]
    for axis in (0, 1):
        for f, want in ((0.93, HIT), (1.07, MISS)):
            d = [0.0, 0.0]
            d[axis] = f * r * (1 if axis == 0 else -1)
            simple("window_d%s_%.2f_r" % ("xy"[axis], f), want, [dict(d=d)], th=1.5, gates=[("rel", "dxy"[:1] + "xy"[axis], r)])
    # chi-square, th = 3
    for f, want in ((0.9, HIT), (1.1, MISS)):
        off = np.sqrt(f * 5.99 * sg[3])
        simple("chi2_mono_%.1f_of_5.99" % f, want, [dict(d=(0.6 * off, -0.8 * off))], gates=[("rel", "chi2", 5.99)])
        offr = np.sqrt(f * 7.8 * sg[3])
        simple("chi2_stereo_u_right_%.1f_of_7.8" % f, want, [dict(stereo=True, ur_off=offr)], gates=[("rel", "chi2", 7.8)])
    simple("chi2_mono_between_5.99_and_5.991", MISS, [dict(octave=7, d=(np.sqrt(5.9905 * sg[7]), 0.0))], level=7,
           gates=[("band", "chi2", (5.99, 5.991))])
    # window origin: (u - min + r) * inv picks the window's last cell.  With an origin of more than half a cell the keypoint's PosInGrid cell
    # can be that last cell while ceil((u + r) * inv), the same without the origin, ends one cell short: th 1.5, level 0, the keypoint at
    # +0.9 r, and u + r a little (half of what the origin leaves) under a multiple of the cell size
    r0 = 1.5 * sf[0]
    for axis, lo, cell in ((0, min_x, s.cell_w), (1, min_y, s.cell_h)):
        room = -lo / cell - 0.5 - 0.1 * r0 / cell
        if room < 0.02:     # the origins 0 and -3.0 (0.47 of a row): dropping them from the window can lose no keypoint
            continue
        u0 = s.slot()
        p = u0.copy()
        p[axis] = (np.round((u0[axis] + r0) / cell) - 0.5 * room) * cell - r0
        rec, uv, zc, _ = s.point(p, level_pow=-0.5)
        d = [0.0, 0.0]
        d[axis] = 0.9 * r0
        s.add("window_origin_%s_keypoint_in_the_last_cell" % "xy"[axis], rec, uv, zc, [dict(d=d, octave=0)], HIT, th=1.5, gates=[("rel", "d" + "xy"[axis], r0)])
        kcell = np.floor((float(s.b.rows[-1]["xy"[axis]]) - lo) / cell + 0.5)
        with_origin, without = np.ceil((uv[axis] - lo + r0) / cell), np.ceil((uv[axis] + r0) / cell)
        assert kcell == with_origin == without + 1, (kcell, with_origin, without)
        for edge in ((float(s.b.rows[-1]["xy"[axis]]) - lo) / cell + 0.5, (uv[axis] + r0) / cell):   # neither decision closer than 0.25 px
            assert abs(edge - np.round(edge)) * cell > 0.25
    # equal Hamming distances, strict <: grid order decides (column, then row, then index)
    u0 = s.slot()
    ub = min_x + (np.floor((u0[0] - min_x) / s.cell_w) + 0.5) * s.cell_w          # a column boundary of PosInGrid's rounding
    vc = min_y + np.round((u0[1] - min_y) / s.cell_h) * s.cell_h                     # the middle of a row
    rec, uv, zc, _ = s.point((ub, vc))
    s.add("tie_columns_lower_column_wins", rec, uv, zc, [dict(xy=(ub + 2.0, vc), flips=9), dict(xy=(ub - 2.0, vc), flips=9, flip_start=90)], (1, 9))
    u0 = s.slot()
    uc = min_x + np.round((u0[0] - min_x) / s.cell_w) * s.cell_w
    vb = min_y + (np.floor((u0[1] - min_y) / s.cell_h) + 0.5) * s.cell_h
    rec, uv, zc, _ = s.point((uc, vb))
    s.add("tie_rows_lower_row_wins", rec, uv, zc, [dict(xy=(uc, vb + 2.0), flips=9), dict(xy=(uc, vb - 2.0), flips=9, flip_start=90)], (1, 9))
    u0 = s.slot()
    uc, vc = min_x + np.round((u0[0] - min_x) / s.cell_w) * s.cell_w, min_y + np.round((u0[1] - min_y) / s.cell_h) * s.cell_h
    rec, uv, zc, _ = s.point((uc, vc))
    s.add("tie_same_cell_lower_index_wins", rec, uv, zc, [dict(xy=(uc + 1.0, vc), flips=9), dict(xy=(uc - 1.0, vc), flips=9, flip_start=90)], (0, 9))
    simple("hamming_50_fused", (0, 50), [dict(flips=50)])
    simple("hamming_51_not_fused_best_dist_51", (-1, 51), [dict(flips=51)])
    # the corners: 0.25 px inside the far and the near bounds, the keypoint in the last / the first cell
    rec, uv, zc, _ = s.point((max_x - 0.25, max_y - 0.25), level=7)
    s.add("corner_max_keypoint_in_last_cell", rec, uv, zc, [dict(xy=(min_x + 63.45 * s.cell_w, min_y + 47.45 * s.cell_h), octave=7)], HIT)
    rec, uv, zc, _ = s.point((min_x + 0.25, min_y + 0.25), level=7)
    s.add("corner_min_keypoint_in_first_cell", rec, uv, zc, [dict(xy=(min_x + 4.0, min_y + 2.0), octave=7)], HIT)
    return s.finish()


# ---- what the tests of both files do with a scene ------------------------------------------------------------------------------------------
def pair_scenes(env, world):
    """name -> (scene, runs) for SearchForTriangulation; 'oriented' is the check_orientation run"""
    return {"sft": (sft_scene(env, world), SFT_RUNS),
            "same_pose": (same_pose_scene(env, world), {"default": {}, "coarse": dict(coarse=True)} if world == "identity" else {"coarse": dict(coarse=True)}),
            "rotation_histogram": (rotation_histogram_scene(env, world), {"default": {}, "oriented": dict(check_orientation=True)}),
            "rotation_histogram_21": (rotation_histogram_scene(env, world, 21), {"default": {}, "oriented": dict(check_orientation=True)})}


def point_scenes(env, world):
    """name -> (scene, runs) for CreateNewMapPoints"""
    return {"cnmp": (cnmp_scene(env, world), CNMP_RUNS), "far": (far_scene(env, world), FAR_RUNS),
            "baseline_0.9": (baseline_scene(env, world, 0.9), {"default": {}}), "baseline_1.1": (baseline_scene(env, world, 1.1), {"default": {}}),
            "first_neighbour": (first_neighbour_scene(env, world), {"default": {}})}


def check_matches(scene, run, j, match):
    """the matches of the current keyframe against neighbour j are what every case says for this run"""
    for c in scene.cases:
        if run not in c["expect"]:
            continue
        want = c["expect"][run]
        want = c["idx2"][want[0]] if (want is not None and c["nb"] == j) else -1
        assert match[c["idx1"]] == want, (scene.world, run, j, c["name"], int(match[c["idx1"]]), want)


def check_points(scene, run, idx):
    """the created records are what every case says for this run, in creation order"""
    for c in scene.cases:
        if run not in c["expect"]:
            continue
        rows = idx[idx[:, 0] == c["idx1"]]
        want = c["expect"][run]
        if want is None:
            assert len(rows) == 0, (scene.world, run, c["name"], rows)
        else:
            assert len(rows) == 1 and tuple(rows[0]) == (c["idx1"], c["nb"], c["idx2"][want[0]], 0 if want[1] == "tri" else 1), (scene.world, run, c["name"], rows)
    assert len(np.unique(idx[:, 0])) == len(idx) and np.all(np.diff(idx[:, 1]) >= 0)
    for j in np.unique(idx[:, 1]):
        assert np.all(np.diff(idx[idx[:, 1] == j, 0]) > 0)


def well_conditioned(scene, idx, x3D):
    """mask of the triangulated records with more than 2 degrees of parallax, less than 25 m from the current keyframe"""
    O1 = centre(scene.cur_pose)
    keep = np.zeros(len(idx), bool)
    for k, (row, X) in enumerate(zip(idx, np.asarray(x3D, np.float64))):
        if row[3] == 0:
            a, b = X - O1, X - centre(scene.nb_pose[row[1]])
            cosp = a @ b / (np.linalg.norm(a) * np.linalg.norm(b))
            keep[k] = cosp < np.cos(np.deg2rad(2.0)) and np.linalg.norm(a) < 25.0
    return keep


def deviation(got, want):
    """max |delta| / max(1, |x3D|) over records"""
    if len(want) == 0:
        return 0.0
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.linalg.norm(got - want, axis=1) / np.maximum(1.0, np.linalg.norm(want, axis=1))))
