"""LocalMapping::SearchInNeighbors (SF/src/LocalMapping.cc:728-837) restated in Python from the reference's lines, on the flat graph that
tc2li_search_in_neighbors_batch takes (pinhole stereo rig: NLeft == -1, no second camera).  The search inside ORBmatcher::Fuse is
mapping_ref.fuse_search, one point at a time with the point's current descriptor; Replace / AddObservation / the descriptor median are
written here from SF/src/MapPoint.cc:150-175, :257-309, :338-412; UpdateNormalAndDepth (:435-503) is in float32, in the order
tc2li_map_points_refresh documents: a norm is sqrtf((x*x + y*y) + z*z), the normal is the sum of v / |v| over the observations in row
order divided by their number, max = dist * level scale, min = max / last level scale; a camera centre is -(R^T t) as Sophus / Eigen
evaluate the inverse of a pose (conjugate quaternion applied to -t).

A problem is a dict with the arrays of tc2li_neighbors_problem and `current`, `inertial`, `abort`, `last_level_scale`; `views[kf_slot[k]]` is
the keyframe of row k (keys, descriptors, u_right) and `bounds` its image bounds.  `on_search(T, p, point_record)` is called before every
search that runs, so that a case builder can look at the gates it evaluates."""
import numpy as np

import mapping_ref

ADD_OBSERVATION, REPLACE = 1, 2
f32 = np.float32


def centre_f32(pose7):
    """Tcw.inverse().translation() in float32: q^-1 applied to -t (Eigen's _transformVector)"""
    q = [f32(-pose7[0]), f32(-pose7[1]), f32(-pose7[2]), f32(pose7[3])]
    v = [f32(pose7[4]) * f32(-1), f32(pose7[5]) * f32(-1), f32(pose7[6]) * f32(-1)]
    uv = [q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]]
    uv = [uv[0] + uv[0], uv[1] + uv[1], uv[2] + uv[2]]
    return np.array([v[0] + q[3] * uv[0] + (q[1] * uv[2] - q[2] * uv[1]),
                     v[1] + q[3] * uv[1] + (q[2] * uv[0] - q[0] * uv[2]),
                     v[2] + q[3] * uv[2] + (q[0] * uv[1] - q[1] * uv[0])], f32)


def norm_f32(v):
    return np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])


def median_choice(descs):
    """row whose sorted Hamming row has the least entry (int)(0.5 (N - 1)); the first such row (MapPoint.cc:377-406)"""
    N = len(descs)
    bits = np.unpackbits(np.asarray(descs, np.uint8).reshape(N, 32), axis=1).astype(np.int32)
    D = (bits[:, None, :] != bits[None, :, :]).sum(2)
    best, best_median = 0, 2 ** 31 - 1
    for i in range(N):
        median = int(np.sort(D[i])[int(0.5 * (N - 1))])
        if median < best_median:
            best_median, best = median, i
    return best


def select_targets(pr):
    """vpTargetKFs (:731-777) -> (targets, keyframe marks)"""
    cur = int(pr["current"])
    bad = (np.asarray(pr["kf_flags"]) & 1).astype(bool)
    mark = (np.asarray(pr["kf_flags"]) & 2).astype(bool)
    co, cv, prev = pr["covis_offsets"], pr["covis"], pr["prev_kf"]
    targets = []
    for kf in cv[co[cur]:co[cur + 1]][:10]:                    # :734-743
        if bad[kf] or mark[kf]:
            continue
        targets.append(int(kf)); mark[kf] = True
    for i in range(len(targets)):                              # :747, imax fixed
        t = targets[i]
        for kf in cv[co[t]:co[t + 1]][:20]:                    # :749-757
            if bad[kf] or mark[kf] or kf == cur:
                continue
            targets.append(int(kf)); mark[kf] = True
        if pr.get("abort", False):                             # :758
            break
    if pr.get("inertial", False):                              # :763-777
        kf = int(prev[cur])
        while len(targets) < 20 and kf >= 0:
            if not (bad[kf] or mark[kf]):
                targets.append(kf); mark[kf] = True
            kf = int(prev[kf])
    return targets, mark


class State:
    def __init__(self, pr, views, bounds, env, on_search=None, search=None):
        self.pr, self.views, self.env, self.on_search, self.search = pr, views, env, on_search, search
        self.bounds = np.broadcast_to(np.asarray(bounds, np.float32).reshape(-1, 4), (len(views), 4))
        n = len(pr["points"])
        self.n = n
        self.points = np.array(pr["points"]).copy()
        self.bad = (np.asarray(pr["point_flags"], np.uint8) & 1).astype(bool)
        self.mark = (np.asarray(pr["point_flags"], np.uint8) & 2).astype(bool)
        self.kf_bad = (np.asarray(pr["kf_flags"], np.uint8) & 1).astype(bool)
        self.nobs = np.array(pr["point_nobs"], np.int32).copy()
        self.found, self.visible = np.array(pr["point_found"], np.int32).copy(), np.array(pr["point_visible"], np.int32).copy()
        oo = pr["obs_offsets"]
        self.obs = [dict((int(pr["obs_kf"][o]), int(pr["obs_index"][o])) for o in range(oo[p], oo[p + 1])) for p in range(n)]
        self.slot = np.array(pr["slot_point"], np.int32).copy()
        self.so = np.asarray(pr["slot_offsets"])
        self.replaced = np.full(n, -1, np.int32)
        self.desc_kf, self.desc_index = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
        self.ops = []

    def view(self, kf):
        return self.views[int(self.pr["kf_slot"][kf])]

    def add_observation(self, p, kf, idx):                     # MapPoint.cc:150-175
        self.obs[p][kf] = idx
        self.nobs[p] += 2 if self.view(kf)["u_right"][idx] >= 0 else 1

    def compute_distinctive_descriptors(self, p):              # MapPoint.cc:338-412
        if self.bad[p]:
            return
        rows = [(kf, idx) for kf, idx in sorted(self.obs[p].items()) if not self.kf_bad[kf]]
        if not rows:
            return
        b = median_choice([self.view(kf)["descriptors"][idx] for kf, idx in rows])
        self.points["descriptor"][p] = self.view(rows[b][0])["descriptors"][rows[b][1]]
        self.desc_kf[p], self.desc_index[p] = rows[b]

    def replace(self, x, w):                                   # x.Replace(w), MapPoint.cc:257-309
        if x == w:
            return
        obs, self.obs[x] = self.obs[x], {}
        self.bad[x] = True
        self.replaced[x] = w
        for kf, idx in sorted(obs.items()):
            if kf not in self.obs[w]:
                self.slot[self.so[kf] + idx] = w
                self.add_observation(w, kf, idx)
            else:
                self.slot[self.so[kf] + idx] = -1
        self.found[w] += self.found[x]
        self.visible[w] += self.visible[x]
        self.compute_distinctive_descriptors(w)

    def fuse(self, T, plist, ordinal):                         # ORBmatcher.cc:1186-1346, th = 3.0
        e, v = self.env, self.view(T)
        n_fused = 0
        for p in plist:
            p = int(p)
            if p < 0 or self.bad[p] or T in self.obs[p]:
                continue
            if self.on_search:
                self.on_search(T, p, self.points[p])
            if self.search:   # a test's own search results in place of the restatement's
                b = int(self.search(T, p))
            else:
                _, bi, _ = mapping_ref.fuse_search(v["keys"], v["descriptors"], v["u_right"], self.bounds[int(self.pr["kf_slot"][T])],
                                                   np.asarray(self.pr["poses7"]).reshape(-1, 7)[T], e.cam4, e.bf, e.sf, e.isg, e.logsf, self.points[p:p + 1], [1])
                b = int(bi[0])
            if b < 0:
                continue
            q = int(self.slot[self.so[T] + b])
            if q < 0:
                self.add_observation(p, T, b)
                self.slot[self.so[T] + b] = p
                self.ops.append((ADD_OBSERVATION, ordinal, p, -1, -1, T, b))
            elif not self.bad[q]:
                if q != p:
                    winner = q if self.nobs[q] > self.nobs[p] else p
                    self.replace(p if winner == q else q, winner)
                    self.ops.append((REPLACE, ordinal, p, q, winner, T, b))
            n_fused += 1
        return n_fused


def search_in_neighbors(pr, views, bounds, env, on_search=None, search=None):
    """-> dict with the outputs of tc2li_search_in_neighbors_batch (integers; normals / distances float32 where refreshed)"""
    s = State(pr, views, bounds, env, on_search, search)
    cur = int(pr["current"])
    targets, _ = select_targets(pr)
    plist = s.slot[s.so[cur]:s.so[cur + 1]].copy()                            # :781
    target_fused = [s.fuse(T, plist, i) for i, T in enumerate(targets)]       # :782-788
    n = s.n
    candidates, fused_current = [], 0
    refreshed = np.zeros(n, np.uint8)
    normals, mn, mx = np.zeros((n, 3), f32), np.zeros(n, f32), np.zeros(n, f32)
    if not pr.get("abort", False):                                            # :791
        for T in targets:                                                     # :798-814
            for p in s.slot[s.so[T]:s.so[T + 1]]:
                if p < 0 or s.bad[p] or s.mark[p]:
                    continue
                s.mark[p] = True
                candidates.append(int(p))
        fused_current = s.fuse(cur, candidates, len(targets))                 # :816
        poses = np.asarray(pr["poses7"], f32).reshape(-1, 7)
        last = f32(pr["last_level_scale"])
        for p in s.slot[s.so[cur]:s.so[cur + 1]]:                             # :821-833
            if p < 0 or s.bad[p]:
                continue
            s.compute_distinctive_descriptors(p)
            if not s.obs[p]:
                continue
            X = s.points["pos"][p].astype(f32)
            acc = np.zeros(3, f32)
            for kf in sorted(s.obs[p]):
                v = X - centre_f32(poses[kf])
                acc = acc + v / norm_f32(v)
            dist = norm_f32(X - centre_f32(poses[int(pr["point_ref_kf"][p])]))
            mx[p] = dist * f32(pr["point_ref_level_scale"][p])
            mn[p] = mx[p] / last
            normals[p] = acc / f32(len(s.obs[p]))
            refreshed[p] = 1
    obs_off = np.zeros(n + 1, np.int32)
    obs_kf, obs_index = [], []
    for p in range(n):
        for kf, idx in sorted(s.obs[p].items()):
            obs_kf.append(kf); obs_index.append(idx)
        obs_off[p + 1] = len(obs_kf)
    s.desc_kf[s.bad] = -1
    s.desc_index[s.bad] = -1
    return dict(targets=np.array(targets, np.int32), target_fused=np.array(target_fused, np.int32), candidates=np.array(candidates, np.int32),
                ops=np.array(s.ops, np.int32).reshape(-1, 7), fused_current=fused_current, slot_point_out=s.slot, point_bad_out=s.bad.astype(np.uint8),
                point_replaced=s.replaced, point_nobs_out=s.nobs, point_found_out=s.found, point_visible_out=s.visible, obs_offsets_out=obs_off,
                obs_kf_out=np.array(obs_kf, np.int32), obs_index_out=np.array(obs_index, np.int32), desc_kf=s.desc_kf, desc_index=s.desc_index,
                refreshed=refreshed, normals_out=normals, min_distance_out=mn, max_distance_out=mx)
