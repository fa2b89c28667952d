"""Directed local map points for SearchLocalPoints (Frame::isInFrustum + MapPoint::PredictScale + the local-map overload of
ORBmatcher::SearchByProjection, SF/src/Frame.cc:542-603, MapPoint.cc:540-555, ORBmatcher.cc:52-149) on the features of one extracted
frame.  The camera sits at the identity, so mRcw is the unit matrix, mOw zero and a point's camera coordinates are its world coordinates
bit for bit.  Every point lies on (or at a chosen offset from) the ray of a chosen keypoint and carries that keypoint's descriptor with
chosen bits flipped.  Each group names the side of a comparison its points are built for; build() records it, test_projection_cases.py
checks it with projection_ref alone and test_projection_gates_gpu.py runs the points on the device.

frame = dict(keys, descriptors, u_right, cols, rows); cam = fx fy cx cy bf (floats)."""
import numpy as np

import projection_cases as PC

F32 = np.float32
MAP_POINT_DTYPE = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("min_distance", "<f4"), ("max_distance", "<f4"),
                            ("max_distance_raw", "<f4"), ("descriptor", "u1", (32,))])   # tc2li_map_point
LEVEL_STEPS = (-8, -1, 0, 1, 8)
COS_998 = F32(0.998)


def norm3(p):
    """Eigen's Vector3f::norm() as the library and the oracle restate it: sqrt((x * x + y * y) + z * z) in float."""
    p = [F32(x) for x in p]
    return F32(np.sqrt(F32(F32(F32(p[0] * p[0]) + F32(p[1] * p[1])) + F32(p[2] * p[2]))))


def project(p, cam):
    fx, fy, cx, cy = [F32(x) for x in cam[:4]]
    p = [F32(x) for x in p]
    return F32(F32(F32(fx * p[0]) / p[2]) + cx), F32(F32(F32(fy * p[1]) / p[2]) + cy)


def on_ray(u, v, z, cam):
    fx, fy, cx, cy = [F32(x) for x in cam[:4]]
    z = F32(z)
    return np.float32([F32(F32(F32(u) - cx) * z) / fx, F32(F32(F32(v) - cy) * z) / fy, z])


def view_cos_of(p, n):
    p, n = [F32(x) for x in p], [F32(x) for x in n]
    return F32(F32(F32(F32(p[0] * n[0]) + F32(p[1] * n[1])) + F32(p[2] * n[2])) / norm3(p))


def normal_for(p, target):
    """A normal (0, 0, c) whose viewing cosine with the point p, in the reference's float order, is exactly `target`: c near
    target * dist / z, a few units in the last place either way; None when the two roundings skip that value."""
    c0 = F32(F32(target) * norm3(p) / F32(p[2]))
    for sc in range(-16, 17):
        c = PC.ulp_neighbour(c0, sc)
        if view_cos_of(p, (0, 0, c)) == F32(target):
            return np.float32([0, 0, c])
    return None


def raw_for(dist, target):
    """max_distance_raw with float32(raw / dist) == target, or None when the division skips that value."""
    r0 = F32(F32(target) * F32(dist))
    for s in range(-6, 7):
        r = PC.ulp_neighbour(r0, s)
        if F32(r / F32(dist)) == F32(target):
            return r
    return None


class Spread:
    """Hands out keypoints that lie at least `gap` pixels (on either axis) from every keypoint handed out before."""

    def __init__(self, keys, gap=16.0):
        self.x, self.y, self.gap = keys["x"].astype(np.float32), keys["y"].astype(np.float32), gap
        self.free = np.ones(len(keys), bool)

    def take(self, i):
        self.free &= np.maximum(np.abs(self.x - self.x[i]), np.abs(self.y - self.y[i])) >= self.gap
        return int(i)

    def pick(self, mask):
        cand = np.flatnonzero(mask & self.free)
        assert len(cand), "the frame has no keypoint left for this case"
        return self.take(cand[0])


def build(frame, cam, scales):
    """-> dict(points = tc2li_map_point records, notes = one dict per point: group, key (the keypoint it was built on), and what the
    group states: `valid` (isInFrustum's answer), `level`, `radius_factor` (2.5 or 4.0), `ratio` ...; th_far = the far-points threshold
    that lies exactly on one point's depth)."""
    keys, desc, u_right = frame["keys"], frame["descriptors"], frame["u_right"]
    cols, rows = frame["cols"], frame["rows"]
    fx, fy, cx, cy, bf = [F32(x) for x in cam[:5]]
    inside = (keys["x"] > 30) & (keys["x"] < cols - 30) & (keys["y"] > 30) & (keys["y"] < rows - 30)
    depth_of = lambda i: F32(bf / F32(keys["x"][i] - u_right[i])) if u_right[i] > 0 else F32(5.0)   # the stereo depth: the u_right gate passes
    spread, pts, notes = Spread(keys), [], []

    def add(group, i, pos, d, level=None, normal=None, raw=None, lo=None, hi=None, **note):
        pos = np.float32(pos)
        dist = norm3(pos)
        rec = np.zeros(1, MAP_POINT_DTYPE)[0]
        rec["pos"] = pos
        rec["normal"] = np.float32(pos / dist) if normal is None else normal
        if raw is None:      # the middle of level `level`: no doubt about it
            raw = F32(dist * F32(1.2) ** F32(level - 0.5))
        rec["max_distance_raw"] = raw
        rec["min_distance"] = F32(0.0) if lo is None else lo
        rec["max_distance"] = F32(1e9) if hi is None else hi
        rec["descriptor"] = d
        pts.append(rec)
        notes.append(dict(group=group, key=int(i), level=level, **note))

    # ---- ratio pairs (first: close pairs are rare): two keypoints of one octave within 3.5 window units of each other; the point on the
    # first one's ray, seen under a cosine of 0.9 (window factor 4.0), with a descriptor at distance 40 or 41 (as the parity of their
    # mutual distance allows) from the first and 50 from the second
    pairs = []
    x, y = keys["x"].astype(np.float32), keys["y"].astype(np.float32)
    for i in range(len(keys)):
        if len(pairs) == 12:
            break
        if not (inside[i] and spread.free[i]):
            continue
        o = int(keys["octave"][i])
        near = (np.maximum(np.abs(x - x[i]), np.abs(y - y[i])) < 3.5 * scales[o]) & (keys["octave"] == o)
        near[i] = False
        for j in np.flatnonzero(near):
            diff = np.unpackbits(desc[i] ^ desc[j], bitorder="little")
            h = int(diff.sum())
            a = 40 if h % 2 == 0 else 41
            p, s = (a - 50 + h) // 2, (a + 50 - h) // 2
            if p < 0 or s < 0 or sum(1 for e in pairs if e[2] == a) >= 6:
                continue
            bits = np.unpackbits(desc[i], bitorder="little")
            bits[np.flatnonzero(diff)[:p]] ^= 1          # towards the second key: +1 / -1
            bits[np.flatnonzero(diff == 0)[:s]] ^= 1     # away from both: +1 / +1
            pairs.append((i, int(j), a, np.packbits(bits, bitorder="little")))
            spread.take(i)
            break
    for i, j, a, d in pairs:
        pos = on_ray(keys["x"][i], keys["y"][i], depth_of(i), cam)
        add("ratio", i, pos, d, level=int(keys["octave"][i]), normal=np.float32(F32(0.9) * pos / norm3(pos)), second=int(j), best=a, valid=True)

    # ---- levels: float32(max_distance_raw / dist) is 1.2^k or a neighbour; the keypoint's octave is reached from one of the two levels only
    for k in range(7):
        octave = 1 if k == 0 else k - 1            # k == 0: octave 1 is in the window of level 1 (0 .. 1), not of level 0 (-1 .. 0)
        for s in LEVEL_STEPS:
            target = PC.ulp_neighbour(PC.boundary_centre(k), s)
            for attempt in range(8):     # a division that skips the wanted float: the next keypoint
                i = spread.pick((keys["octave"] == octave) & inside)
                pos = on_ray(keys["x"][i], keys["y"][i], depth_of(i), cam)
                raw = raw_for(norm3(pos), target)
                if raw is not None:
                    add("level", i, pos, desc[i], raw=raw, k=k, step=s, ratio=target, octave=octave, valid=True)
                    break
            else:
                raise AssertionError("no keypoint on octave %d gives the ratio %r" % (octave, target))

    # ---- the distance gates at equality (kept) and one unit in the last place beyond (not in view)
    for name, side in (("min-at", 0), ("min-above", 1), ("max-at", 0), ("max-below", -1)):
        i = spread.pick(inside)
        pos = on_ray(keys["x"][i], keys["y"][i], depth_of(i), cam)
        bound = PC.ulp_neighbour(norm3(pos), side)
        add("distance-" + name, i, pos, desc[i], level=int(keys["octave"][i]), valid=side == 0, **({"lo": bound} if name.startswith("min") else {"hi": bound}))

    # ---- the viewing cosine at 0.5 (kept) and under it; around 0.998, where the window factor switches: a double comparison in the
    # reference (ORBmatcher.cc:226 `viewCos>0.998`), so float32(0.998) = 0.99800003 itself is already above it.  The point is moved
    # 3.25 windows' units to the right of its keypoint: the keypoint is inside the 4.0 window and outside the 2.5 one.
    for name, target, valid, factor in (("cos-half", F32(0.5), True, 4.0), ("cos-under-half", PC.ulp_neighbour(0.5, -1), False, 4.0),
                                        ("cos-under-998", PC.ulp_neighbour(COS_998, -1), True, 4.0), ("cos-998", COS_998, True, 2.5),
                                        ("cos-over-998", PC.ulp_neighbour(COS_998, 1), True, 2.5), ("cos-one", None, True, 2.5)):
        i = spread.pick(inside & (keys["octave"] <= 3))
        level = int(keys["octave"][i])
        u = F32(keys["x"][i] + F32(3.25) * F32(scales[level]))
        # the depth a little further each time, until the cosine can be met exactly; just under 0.5 the floats are twice as dense as the
        # products they come from unless dist lies just under a power of two: that point is not in view, so its depth is free
        ray = float(norm3(on_ray(u, keys["y"][i], 1.0, cam)))
        depths = [F32(depth_of(i) * F32(1 + 2.5e-5 * t)) for t in range(400)] if valid else [F32(4.0 * (1 - 1e-5 * t) / ray) for t in range(1, 400)]
        for z in depths:
            pos = on_ray(u, keys["y"][i], z, cam)
            normal = None if target is None else normal_for(pos, target)
            if target is None or normal is not None:
                break
        else:
            raise AssertionError("no normal gives the viewing cosine %r" % target)
        add(name, i, pos, desc[i], level=level, normal=normal, valid=valid, radius_factor=factor, view_cos=target, offset=F32(3.25) * F32(scales[level]))

    # ---- the image border: u == cols is in view, the next float is not
    for name, side in (("u-at-cols", 0), ("u-past-cols", 1)):
        want = PC.ulp_neighbour(F32(cols), side)
        pos = None
        for s in range(-200, 201):
            cand = np.float32([PC.ulp_neighbour(F32(F32(F32(cols) - cx) * F32(4.0)) / fx, s), 0.0, 4.0])
            if project(cand, cam)[0] == want:
                pos = cand
                break
        assert pos is not None, "no point projects onto u = %r" % want
        add(name, -1, pos, np.zeros(32, np.uint8), level=0, valid=side == 0)

    points = np.array(pts, MAP_POINT_DTYPE)
    # the far-points threshold: the depth of the point in view that about two thirds of the points do not exceed
    depth = np.array([norm3(p) for p in points["pos"]])
    in_view = [k for k, nt in enumerate(notes) if nt["valid"]]
    far_key = sorted(in_view, key=lambda k: depth[k])[2 * len(in_view) // 3]
    return dict(points=points, notes=notes, th_far=depth[far_key], far_point=far_key)


def runs(case):
    """(th, far_points, th_far) of the searches: th == 1.0 (no factor) and 3.0; far points with the threshold on point far_point's depth
    (`mTrackDepth > thFarPoints` is false: kept) and one unit in the last place under it (dropped)."""
    return [(1.0, False, 0.0), (3.0, False, 0.0), (1.0, True, float(case["th_far"])), (1.0, True, float(PC.ulp_neighbour(case["th_far"], -1)))]
