// tc2li_search_in_neighbors_batch / tc2li_host_search_in_neighbors_batch / tc2li_search_in_neighbors_limits (include/tc2li_hip.h):
// LocalMapping::SearchInNeighbors (SF/src/LocalMapping.cc:728-837) in the reference's order on the flat graph.  Here: the validation
// both entries share, the host twin (plain sequential C++ that follows the header's rules line by line, one problem per worker), the
// host's feature grids, and the device entry: one packed upload, one launch (neighbors_kernels.hip), one download, and the host twin for
// the problems that met a limit of the device path.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "common.hpp"
#include "fuse_search.hpp"
#include "mapping_host.hpp"
#include "neighbors_device.hpp"
#include "packed_batch.hpp"

static_assert(sizeof(tc2li_neighbors_op) == 32, "ABI layout");
static_assert(TC2LI_NEIGHBORS_COUNTS == tc2li::kNbCounts && TC2LI_NEIGHBORS_MAX_TARGETS == tc2li::kNbMaxTargets, "header and kernel agree");

namespace tc2li {
namespace {

typedef tc2li_neighbors_problem Problem;

// rule 1 (:731-777); false: the mPrevKF chain returns to itself within the walk
bool select_targets(const Problem& in, std::vector<uint8_t>& kflag, std::vector<int32_t>& targets) {
    const int cur = in.current;
    targets.clear();
    const int b0 = in.covis_offsets[cur], n0 = std::min(10, in.covis_offsets[cur + 1] - b0);
    for (int k = 0; k < n0; ++k) {
        const int kf = in.covis[b0 + k];
        if (kflag[kf] & 3) continue;                                         // :739
        targets.push_back(kf); kflag[kf] |= 2;                               // :741-742
    }
    const int imax = (int)targets.size();                                    // :747
    for (int i = 0; i < imax; ++i) {
        const int t = targets[i];
        const int b = in.covis_offsets[t], n = std::min(20, in.covis_offsets[t + 1] - b);
        for (int k = 0; k < n; ++k) {
            const int kf = in.covis[b + k];
            if ((kflag[kf] & 3) || kf == cur) continue;                      // :753
            targets.push_back(kf); kflag[kf] |= 2;                           // :755-756
        }
        if (in.abort) break;                                                 // :758
    }
    if (in.inertial) {
        int kf = in.prev_kf[cur], steps = 0;
        while ((int)targets.size() < 20 && kf >= 0) {                        // :766
            if (++steps > in.n_keyframes) return false;
            if (!(kflag[kf] & 3)) { targets.push_back(kf); kflag[kf] |= 2; }  // :768-774
            kf = in.prev_kf[kf];
        }
    }
    return true;
}

// "" or what is wrong with problem `in`; stored_n(k) = the keypoints stored for the slot of row k, -1: empty or out of range
template <class StoredN>
const char* what_is_wrong(const Problem& in, StoredN stored_n) {
    if (in.n_keyframes < 1 || in.n_points < 0 || in.current < 0 || in.current >= in.n_keyframes) return "sizes or current out of range";
    if (!in.kf_slot || !in.kf_flags || !in.prev_kf || !in.poses7 || !in.covis_offsets || !in.slot_offsets || !in.counts) return "null keyframe table or counts";
    if (in.n_points > 0 && (!in.points || !in.point_flags || !in.point_nobs || !in.point_found || !in.point_visible || !in.point_ref_kf ||
                            !in.point_ref_level_scale || !in.obs_offsets))
        return "null point table";
    if (in.target_capacity < 0 || in.candidate_capacity < 0 || in.op_capacity < 0 || in.obs_capacity < 0) return "negative capacity";
    if ((in.target_capacity > 0 && (!in.targets || !in.target_fused)) || (in.candidate_capacity > 0 && !in.candidates) || (in.op_capacity > 0 && !in.ops) ||
        (in.obs_capacity > 0 && (!in.obs_kf_out || !in.obs_index_out)))
        return "null list with a capacity";
    if (!(in.last_level_scale > 0)) return "last_level_scale must be positive";
    const int nk = in.n_keyframes, np = in.n_points;
    if (!ascending(in.covis_offsets, nk) || !ascending(in.slot_offsets, nk)) return "keyframe offsets do not ascend";
    if ((in.covis_offsets[nk] > 0 && !in.covis) || (in.slot_offsets[nk] > 0 && !in.slot_point)) return "null covis or slot_point";
    for (int k = 0; k < in.covis_offsets[nk]; ++k)
        if (in.covis[k] < 0 || in.covis[k] >= nk) return "covisible keyframe out of range";
    for (int k = 0; k < nk; ++k) {
        if (in.prev_kf[k] < -1 || in.prev_kf[k] >= nk) return "prev_kf out of range";
        const int n = stored_n(k);
        if (n < 0) return "a keyframe names a slot that is empty or out of range";
        if (in.slot_offsets[k + 1] - in.slot_offsets[k] != n) return "a slot row is not as long as the stored keypoint count";
    }
    for (int s = 0; s < in.slot_offsets[nk]; ++s)
        if (in.slot_point[s] < -1 || in.slot_point[s] >= np) return "slot_point out of range";
    if (np > 0) {
        if (!ascending(in.obs_offsets, np)) return "observation offsets do not ascend";
        if (in.obs_offsets[np] > 0 && (!in.obs_kf || !in.obs_index)) return "null observation table";
        for (int p = 0; p < np; ++p) {
            if (in.point_ref_kf[p] < 0 || in.point_ref_kf[p] >= nk) return "point_ref_kf out of range";
            for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) {
                const int kf = in.obs_kf[o];
                if (kf < 0 || kf >= nk) return "observing keyframe out of range";
                if (o > in.obs_offsets[p] && kf <= in.obs_kf[o - 1]) return "an observation row does not ascend strictly";
                if (in.obs_index[o] < 0 || in.obs_index[o] >= in.slot_offsets[kf + 1] - in.slot_offsets[kf]) return "observation index out of range";
            }
        }
    }
    try {
        std::vector<uint8_t> kflag(in.kf_flags, in.kf_flags + nk);
        std::vector<int32_t> targets;
        if (!select_targets(in, kflag, targets)) return "the prev_kf chain returns to itself";
    } catch (const std::bad_alloc&) {
        return "no memory for a table of n_keyframes entries";
    }
    return "";
}

int check_call(const char* entry, const Problem* problems, int n_problems, const float* cam4, const float* scale_factors, const float* inv_level_sigma2,
               int n_levels, float log_scale_factor) {
    if (n_problems < 0 || (n_problems > 0 && !problems) || !cam4 || !scale_factors || !inv_level_sigma2 || n_levels < 1 || !(log_scale_factor > 0)) {
        set_error("%s: invalid argument", entry);
        return TC2LI_ERR_INVALID;
    }
    return 0;
}

// ---- the host twin ---------------------------------------------------------------------------------------------------------------------
struct Result {
    int32_t counts[kNbCounts];
    std::vector<int32_t> targets, target_fused, candidates;
    std::vector<tc2li_neighbors_op> ops;
    std::vector<int32_t> slot, replaced, nobs, found, visible, obs_off, obs_kf, obs_idx, desc_kf, desc_idx;
    std::vector<uint8_t> bad, refreshed;
    std::vector<float> normals, mn, mx;
};

struct Twin {
    const Problem& in;
    const NbKf* kfs;   // per keyframe row, host memory
    const NbConsts& cc;
    Result& r;
    std::vector<std::vector<NbObs>> obs;
    std::vector<tc2li_map_point> pts;
    std::vector<uint8_t> kflag, pflag;   // bit 0 bad, bit 1 marked

    Twin(const Problem& in_, const NbKf* kfs_, const NbConsts& cc_, Result& r_) : in(in_), kfs(kfs_), cc(cc_), r(r_) {}

    bool in_kf(int p, int kf) const {
        for (const NbObs& o : obs[p]) if (o.kf == kf) return true;
        return false;
    }
    void add_obs(int w, int kf, int idx) {                                   // MapPoint.cc:150-175
        auto& v = obs[w];
        auto at = v.begin();
        while (at != v.end() && at->kf < kf) ++at;
        v.insert(at, NbObs{kf, idx});
        r.nobs[w] += kfs[kf].u_right[idx] >= 0 ? 2 : 1;                      // :171-174
    }
    void describe(int w) {                                                   // MapPoint.cc:338-412
        if (pflag[w] & 1) return;                                            // :347
        std::vector<uint32_t> d;
        std::vector<int> row_obs;
        for (size_t o = 0; o < obs[w].size(); ++o) {
            const NbObs& ob = obs[w][o];
            if (kflag[ob.kf] & 1) continue;                                  // :361
            const uint32_t* src = reinterpret_cast<const uint32_t*>(kfs[ob.kf].desc) + 8 * (size_t)ob.idx;
            d.insert(d.end(), src, src + 8);
            row_obs.push_back((int)o);
        }
        const int N = (int)row_obs.size();
        if (N == 0) return;                                                  // :352, :374
        int best_median = 0x7fffffff, best = 0;
        for (int i = 0; i < N; ++i) {
            const int m = row_median(d.data(), 8, N, i);                     // :397-399
            if (m < best_median) { best_median = m; best = i; }              // :401
        }
        memcpy(pts[w].descriptor, d.data() + 8 * (size_t)best, 32);          // :410
        r.desc_kf[w] = obs[w][row_obs[best]].kf; r.desc_idx[w] = obs[w][row_obs[best]].idx;
    }
    void replace(int x, int w) {                                             // MapPoint.cc:257-309, x != w
        std::vector<NbObs> mine;
        mine.swap(obs[x]);                                                   // :267-268
        pflag[x] |= 1; r.replaced[x] = w;                                    // :269, :272
        for (const NbObs& ob : mine) {                                       // :275
            int32_t& slot = r.slot[in.slot_offsets[ob.kf] + ob.idx];
            if (!in_kf(w, ob.kf)) { slot = w; add_obs(w, ob.kf, ob.idx); }   // :283-287
            else slot = -1;                                                  // :297
        }
        r.found[w] += r.found[x]; r.visible[w] += r.visible[x];              // :304-305
        describe(w);                                                         // :306
    }
    int fuse(int T, const std::vector<int32_t>& list, int ordinal) {         // ORBmatcher.cc:1186-1346
        FuseDev f{};
        const NbKf& k = kfs[T];
        f.keys = k.keys; f.desc = k.desc; f.u_right = k.u_right; f.cell_start = k.cell_start; f.items = k.items;
        f.n_keys = k.n; f.n_levels = cc.n_levels;
        memcpy(f.q, k.q, 16); memcpy(f.t, k.t, 12); memcpy(f.Ow, k.Ow, 12);
        f.fx = cc.fx; f.fy = cc.fy; f.cx = cc.cx; f.cy = cc.cy; f.bf = cc.bf; f.th = 3.0f; f.log_scale_factor = cc.log_scale_factor;
        f.min_x = k.bounds[0]; f.max_x = k.bounds[1]; f.min_y = k.bounds[2]; f.max_y = k.bounds[3];
        f.scale_factors = cc.scale_factors; f.inv_level_sigma2 = cc.inv_level_sigma2;
        int fused = 0;
        for (const int p : list) {
            if (p < 0 || (pflag[p] & 1) || in_kf(p, T)) continue;            // :1190, :1196, :1201
            int bi, bd;
            fuse_search_one(f, reinterpret_cast<const float*>(&pts[p]), &bi, &bd);
            if (bi < 0) continue;                                            // :1321
            const int q = r.slot[in.slot_offsets[T] + bi];                   // :1323
            if (q < 0) {
                add_obs(p, T, bi); r.slot[in.slot_offsets[T] + bi] = p;      // :1336-1337
                r.ops.push_back(tc2li_neighbors_op{TC2LI_NEIGHBORS_ADD_OBSERVATION, ordinal, p, -1, -1, T, bi, 0});
            } else if (!(pflag[q] & 1) && q != p) {                          // :1326; MapPoint.cc:259
                const bool q_wins = r.nobs[q] > r.nobs[p];                   // :1328
                if (q_wins) replace(p, q); else replace(q, p);
                r.ops.push_back(tc2li_neighbors_op{TC2LI_NEIGHBORS_REPLACE, ordinal, p, q, q_wins ? q : p, T, bi, 0});
            }
            ++fused;                                                         // :1339
        }
        return fused;
    }
    void run() {
        const int nk = in.n_keyframes, np = in.n_points, cur = in.current;
        kflag.assign(in.kf_flags, in.kf_flags + nk);
        pflag.resize(np); obs.resize(np);
        r.slot.assign(in.slot_point, in.slot_point + in.slot_offsets[nk]);
        if (np) { pts.assign(in.points, in.points + np); r.nobs.assign(in.point_nobs, in.point_nobs + np); r.found.assign(in.point_found, in.point_found + np);
                  r.visible.assign(in.point_visible, in.point_visible + np); }
        r.replaced.assign(np, -1); r.desc_kf.assign(np, -1); r.desc_idx.assign(np, -1);
        r.refreshed.assign(np, 0); r.normals.assign(3 * (size_t)np, 0.f); r.mn.assign(np, 0.f); r.mx.assign(np, 0.f);
        for (int p = 0; p < np; ++p) {
            pflag[p] = in.point_flags[p] & 3;
            for (int o = in.obs_offsets[p]; o < in.obs_offsets[p + 1]; ++o) obs[p].push_back(NbObs{in.obs_kf[o], in.obs_index[o]});
        }
        select_targets(in, kflag, r.targets);
        const std::vector<int32_t> list(r.slot.begin() + in.slot_offsets[cur], r.slot.begin() + in.slot_offsets[cur + 1]);   // :781
        int fused1 = 0, fused2 = 0, n_refreshed = 0;
        for (size_t ti = 0; ti < r.targets.size(); ++ti) {                   // :782-788
            r.target_fused.push_back(fuse(r.targets[ti], list, (int)ti));
            fused1 += r.target_fused.back();
        }
        if (!in.abort) {                                                     // :791
            for (const int T : r.targets)                                    // :798-814
                for (int s = in.slot_offsets[T]; s < in.slot_offsets[T + 1]; ++s) {
                    const int p = r.slot[s];
                    if (p < 0 || (pflag[p] & 3)) continue;
                    pflag[p] |= 2;
                    r.candidates.push_back(p);
                }
            fused2 = fuse(cur, r.candidates, (int)r.targets.size());         // :816
            for (int s = in.slot_offsets[cur]; s < in.slot_offsets[cur + 1]; ++s) {   // :821-833
                const int p = r.slot[s];
                if (p < 0 || (pflag[p] & 1) || r.refreshed[p]) continue;      // a point met twice gives the same values twice
                describe(p);
                const int N = (int)obs[p].size();
                if (N == 0) continue;                                        // MapPoint.cc:450
                const float px = pts[p].pos[0], py = pts[p].pos[1], pz = pts[p].pos[2];
                float nx = 0, ny = 0, nz = 0;
                for (const NbObs& ob : obs[p]) {                             // :456-468, the order of k_map_points_refresh
                    const float* C = kfs[ob.kf].Ow;
                    const float vx = px - C[0], vy = py - C[1], vz = pz - C[2];
                    const float nr = sqrtf(vx * vx + vy * vy + vz * vz);
                    nx = nx + vx / nr; ny = ny + vy / nr; nz = nz + vz / nr;
                }
                const float* R = kfs[in.point_ref_kf[p]].Ow;
                const float rx = px - R[0], ry = py - R[1], rz = pz - R[2];
                const float dist = sqrtf(rx * rx + ry * ry + rz * rz);
                r.mx[p] = dist * in.point_ref_level_scale[p];                // :499
                r.mn[p] = r.mx[p] / in.last_level_scale;                     // :500
                r.normals[3 * (size_t)p] = nx / (float)N; r.normals[3 * (size_t)p + 1] = ny / (float)N; r.normals[3 * (size_t)p + 2] = nz / (float)N;
                r.refreshed[p] = 1;
                ++n_refreshed;
            }
        }
        r.bad.resize(np);
        r.obs_off.assign(np + 1, 0);
        for (int p = 0; p < np; ++p) {
            r.bad[p] = pflag[p] & 1;
            if (r.bad[p]) { r.desc_kf[p] = -1; r.desc_idx[p] = -1; }
            for (const NbObs& ob : obs[p]) { r.obs_kf.push_back(ob.kf); r.obs_idx.push_back(ob.idx); }
            r.obs_off[p + 1] = (int32_t)r.obs_kf.size();
        }
        r.counts[kNbStatus] = TC2LI_NEIGHBORS_ON_HOST; r.counts[kNbTargets] = (int32_t)r.targets.size(); r.counts[kNbCandidates] = (int32_t)r.candidates.size();
        r.counts[kNbOps] = (int32_t)r.ops.size(); r.counts[kNbObs] = (int32_t)r.obs_kf.size(); r.counts[kNbRefreshed] = n_refreshed;
        r.counts[kNbFused1] = fused1; r.counts[kNbFused2] = fused2;
    }
};

bool fits(const Problem& in, const int32_t* counts) {
    return counts[kNbTargets] <= in.target_capacity && counts[kNbCandidates] <= in.candidate_capacity && counts[kNbOps] <= in.op_capacity &&
           counts[kNbObs] <= in.obs_capacity;
}
int capacity_error(const char* entry, const Problem* problems, int p) {
    const int32_t* c = problems[p].counts;
    set_error("%s: problem %d needs room for %d targets, %d candidates, %d ops, %d observations", entry, p, c[kNbTargets], c[kNbCandidates], c[kNbOps], c[kNbObs]);
    return TC2LI_ERR_CAPACITY;
}
template <class T> void give(T* dst, const std::vector<T>& v) { if (dst && !v.empty()) memcpy(dst, v.data(), v.size() * sizeof(T)); }
void write_result(const Problem& in, const Result& r) {
    give(in.targets, r.targets); give(in.target_fused, r.target_fused); give(in.candidates, r.candidates); give(in.ops, r.ops);
    give(in.slot_point_out, r.slot); give(in.point_bad_out, r.bad); give(in.point_replaced, r.replaced); give(in.point_nobs_out, r.nobs);
    give(in.point_found_out, r.found); give(in.point_visible_out, r.visible); give(in.obs_offsets_out, r.obs_off); give(in.obs_kf_out, r.obs_kf);
    give(in.obs_index_out, r.obs_idx); give(in.desc_kf, r.desc_kf); give(in.desc_index, r.desc_idx); give(in.refreshed, r.refreshed);
    give(in.normals_out, r.normals); give(in.min_distance_out, r.mn); give(in.max_distance_out, r.mx);
}

// KeyFrame::AssignFeaturesToGrid on the 64 x 48 grid of k_match_grid: cell starts and the keypoints of every cell, ascending
void host_grid(const tc2li_keypoint* keys, int n, const float* b, std::vector<int32_t>& cell_start, std::vector<uint16_t>& items) {
    const int cells = kFuseGridCols * kFuseGridRows;
    const float invW = (float)kFuseGridCols / (b[1] - b[0]), invH = (float)kFuseGridRows / (b[3] - b[2]);
    std::vector<int> cell_of(n);
    cell_start.assign(cells + 1, 0);
    for (int i = 0; i < n; ++i) {
        const int px = (int)roundf((keys[i].x - b[0]) * invW), py = (int)roundf((keys[i].y - b[2]) * invH);
        const bool in = !(px < 0 || px >= kFuseGridCols || py < 0 || py >= kFuseGridRows);
        cell_of[i] = in ? px * kFuseGridRows + py : -1;
        if (in) ++cell_start[cell_of[i] + 1];
    }
    for (int c = 0; c < cells; ++c) cell_start[c + 1] += cell_start[c];
    std::vector<int> cursor(cell_start.begin(), cell_start.end() - 1);
    items.assign(std::max(n, 1), 0);
    for (int i = 0; i < n; ++i)
        if (cell_of[i] >= 0) items[cursor[cell_of[i]]++] = (uint16_t)i;
}

void set_pose(NbKf& k, const float* pose7) {
    memcpy(k.q, pose7, 16); memcpy(k.t, pose7 + 4, 12);
    mapping_host::Q7 T; memcpy(T.q, k.q, 16); memcpy(T.t, k.t, 12);
    const mapping_host::Q7 Tw = mapping_host::inv7(T);
    memcpy(k.Ow, Tw.t, 12);
}

}  // namespace
}  // namespace tc2li

using namespace tc2li;

extern "C" int tc2li_search_in_neighbors_limits(int32_t* out, int capacity) {
    const int32_t v[5] = {kNbMaxObs, kNbMaxKeys, kNbMaxPoints, kNbMaxKeyframes, kNbThreads};
    if (!out || capacity < 0) { set_error("tc2li_search_in_neighbors_limits: invalid argument"); return TC2LI_ERR_INVALID; }
    for (int i = 0; i < std::min(capacity, 5); ++i) out[i] = v[i];
    return 5;
}

extern "C" int tc2li_host_search_in_neighbors_batch(const tc2li_keyframe_view* views, const float* bounds4, int n_views, const tc2li_neighbors_problem* problems,
                                                    int n_problems, const float cam4[4], float bf, const float* scale_factors, const float* inv_level_sigma2,
                                                    int n_levels, float log_scale_factor) {
    const char* entry = "tc2li_host_search_in_neighbors_batch";
    int rc = check_call(entry, problems, n_problems, cam4, scale_factors, inv_level_sigma2, n_levels, log_scale_factor);
    if (rc < 0) return rc;
    if (n_views < 0 || (n_views > 0 && (!views || !bounds4))) { set_error("%s: invalid argument", entry); return TC2LI_ERR_INVALID; }
    for (int v = 0; v < n_views; ++v) {
        const tc2li_keyframe_view& w = views[v];
        const float* b = bounds4 + 4 * (size_t)v;
        if (w.n < 0 || w.n > kNbMaxKeys || (w.n > 0 && (!w.keys || !w.descriptors || !w.u_right)) || !(b[1] > b[0]) || !(b[3] > b[2])) {
            set_error("%s: view %d: invalid keyframe view or empty image bounds", entry, v);
            return TC2LI_ERR_INVALID;
        }
        for (int i = 0; i < w.n; ++i)
            if (w.keys[i].octave < 0 || w.keys[i].octave >= n_levels) { set_error("%s: view %d: keypoint octave out of range", entry, v); return TC2LI_ERR_INVALID; }
    }
    rc = validate_each(entry, "problem", n_problems, invalid_if([&](int p) {
        return what_is_wrong(problems[p], [&](int k) { const int s = problems[p].kf_slot[k]; return s >= 0 && s < n_views ? views[s].n : -1; });
    }));
    if (rc < 0) return rc;
    if (n_problems == 0) return 0;
    // the grids of the views a problem names
    std::vector<uint8_t> used(n_views, 0);
    for (int p = 0; p < n_problems; ++p)
        for (int k = 0; k < problems[p].n_keyframes; ++k) used[problems[p].kf_slot[k]] = 1;
    std::vector<std::vector<int32_t>> cell_start(n_views);
    std::vector<std::vector<uint16_t>> items(n_views);
    tracking_pool().parallel_for(n_views, [&](int v) { if (used[v]) host_grid(views[v].keys, views[v].n, bounds4 + 4 * (size_t)v, cell_start[v], items[v]); });
    const NbConsts cc{cam4[0], cam4[1], cam4[2], cam4[3], bf, log_scale_factor, n_levels, 0, scale_factors, inv_level_sigma2};
    std::vector<Result> results(n_problems);
    tracking_pool().parallel_for(n_problems, [&](int p) {
        const Problem& in = problems[p];
        std::vector<NbKf> kfs(in.n_keyframes);
        for (int k = 0; k < in.n_keyframes; ++k) {
            const int v = in.kf_slot[k];
            NbKf& d = kfs[k];
            d.keys = reinterpret_cast<const float*>(views[v].keys); d.desc = views[v].descriptors; d.u_right = views[v].u_right;
            d.cell_start = cell_start[v].data(); d.items = items[v].data(); d.n = views[v].n;
            memcpy(d.bounds, bounds4 + 4 * (size_t)v, 16);
            set_pose(d, in.poses7 + 7 * (size_t)k);
        }
        Twin(in, kfs.data(), cc, results[p]).run();
        memcpy(in.counts, results[p].counts, sizeof(results[p].counts));
    });
    for (int p = 0; p < n_problems; ++p)
        if (!fits(problems[p], problems[p].counts)) return capacity_error(entry, problems, p);
    tracking_pool().parallel_for(n_problems, [&](int p) { write_result(problems[p], results[p]); });
    return n_problems;
}

namespace {

// the arrays of the store slots a problem names, copied to the host for the twin
struct HostSlot {
    std::vector<uint8_t> keys, desc;
    std::vector<float> u_right;
    std::vector<int32_t> cell_start;
    std::vector<uint16_t> items;
};

}  // namespace

extern "C" int tc2li_search_in_neighbors_batch(tc2li_keyframe_store* store, const tc2li_neighbors_problem* problems, int n_problems, const float cam4[4],
                                               float bf, const float* scale_factors, const float* inv_level_sigma2, int n_levels, float log_scale_factor,
                                               void* stream) {
    const char* entry = "tc2li_search_in_neighbors_batch";
    int rc = check_call(entry, problems, n_problems, cam4, scale_factors, inv_level_sigma2, n_levels, log_scale_factor);
    if (rc < 0) return rc;
    if (!store) { set_error("%s: invalid argument", entry); return TC2LI_ERR_INVALID; }
    // ---- every check before any allocation sized by the caller's counts: a row's slot is looked up in the store as it is now ----
    rc = validate_each(entry, "problem", n_problems, invalid_if([&](int p) {
        return what_is_wrong(problems[p], [&](int k) {
            NbKf d{};
            int32_t levels = 0;
            return keyframe_store_neighbors(store, problems[p].kf_slot[k], &d, &levels) ? d.n : -1;
        });
    }));
    if (rc < 0) return rc;
    std::vector<size_t> kf_first(n_problems + 1, 0);
    for (int p = 0; p < n_problems; ++p) kf_first[p + 1] = kf_first[p] + (size_t)problems[p].n_keyframes;
    std::vector<NbKf> kfs;
    try {
        kfs.resize(kf_first[n_problems]);
    } catch (const std::bad_alloc&) {
        set_error("%s: no memory for %zu keyframe rows", entry, kf_first[n_problems]);
        return TC2LI_ERR_INVALID;
    }
    for (int p = 0; p < n_problems; ++p)
        for (int k = 0; k < problems[p].n_keyframes; ++k) {
            NbKf& d = kfs[kf_first[p] + k];
            int32_t levels = 0;
            d = NbKf{};
            if (!keyframe_store_neighbors(store, problems[p].kf_slot[k], &d, &levels)) {   // erased since the check: another thread's doing
                set_error("%s: problem %d names slot %d, which is empty or out of range", entry, p, problems[p].kf_slot[k]);
                return TC2LI_ERR_INVALID;
            }
            if (levels > n_levels) { set_error("%s: slot %d holds octave %d, the tables have %d levels", entry, problems[p].kf_slot[k], levels - 1, n_levels); return TC2LI_ERR_INVALID; }
            set_pose(d, problems[p].poses7 + 7 * (size_t)k);
        }
    if (!device_ready()) return TC2LI_ERR_NO_DEVICE;
    if (n_problems == 0) return 0;
    hipStream_t st = stream ? (hipStream_t)stream : private_stream();

    // ---- which problems the kernel takes, and where their tables start ----
    std::vector<int> dev_of(n_problems, -1), on_dev;
    std::vector<NbProblemDev> dev;
    size_t n_kf = 0, n_covis = 0, n_slots = 0, n_points = 0, n_obs = 0, n_pool = 0, n_ops = 0, n_obs_out = 0, n_snap = 0;
    for (int p = 0; p < n_problems; ++p) {
        const Problem& in = problems[p];
        bool ok = in.n_points <= kNbMaxPoints && in.n_keyframes <= kNbMaxKeyframes;
        for (int q = 0; ok && q < in.n_points; ++q) ok = in.obs_offsets[q + 1] - in.obs_offsets[q] <= kNbMaxObs;
        if (!ok) continue;
        const size_t d = dev.size();
        NbProblemDev D{};
        D.n_kf = in.n_keyframes; D.n_points = in.n_points; D.current = in.current; D.flags = (in.inertial ? 1 : 0) | (in.abort ? 2 : 0);
        D.kf_off = (int32_t)n_kf; D.kf_row_off = (int32_t)(n_kf + d); D.covis_off = (int32_t)n_covis; D.slot_off = (int32_t)n_slots;
        D.point_off = (int32_t)n_points; D.point_row_off = (int32_t)(n_points + d); D.obs_off = (int32_t)n_obs;
        D.n_obs = in.n_points ? in.obs_offsets[in.n_points] : 0;
        // room for the lists that grow.  A list moves to a piece half as long again as the need, and for a Replace the need counts the
        // loser's observations before those in keyframes the winner is in already are dropped; the pieces of one point therefore add up
        // to less than three times its last ROOM, which may exceed its last length.  Three times the observations on entry, a first
        // piece for every point and twice the ops is a rule of thumb, not a bound: a problem that runs out (a sizing call with
        // op_capacity 0 may) is the host's and says so in counts[0]
        D.pool_off = (int32_t)n_pool; D.pool_size = 3 * D.n_obs + 8 * in.n_points + 2 * in.op_capacity + 256;
        D.op_off = (int32_t)n_ops; D.op_room = in.op_capacity; D.obs_out_off = (int32_t)n_obs_out; D.obs_out_room = in.obs_capacity;
        D.snap_off = (int32_t)n_snap; D.last_level_scale = in.last_level_scale;
        n_kf += in.n_keyframes; n_covis += in.covis_offsets[in.n_keyframes]; n_slots += in.slot_offsets[in.n_keyframes]; n_points += in.n_points;
        n_obs += D.n_obs; n_pool += D.pool_size; n_ops += in.op_capacity; n_obs_out += in.obs_capacity;
        n_snap += in.slot_offsets[in.current + 1] - in.slot_offsets[in.current];
        if (std::max(std::max(std::max(n_kf + d + 1, n_slots), std::max(n_points + d + 1, n_pool)), std::max(n_ops * 8, n_obs_out)) > kMaxRows || 68 * n_points > kMaxRows)
            return too_many_rows(entry, p);
        dev_of[p] = (int)d;
        on_dev.push_back(p);
        dev.push_back(D);
    }
    const size_t nd = dev.size();
    std::vector<Result> results(n_problems);   // of the problems the host twin computes
    std::vector<uint8_t> on_host(n_problems, 0);
    PackedTransfer T;
    Packer &io = T.io, &work = T.work;
    const auto t_prob = io.take<NbProblemDev>(nd); const auto t_kfs = io.take<NbKf>(n_kf); const auto t_kflag = io.take<uint8_t>(n_kf);
    const auto t_prev = io.take<int32_t>(n_kf); const auto t_coff = io.take<int32_t>(n_kf + nd); const auto t_covis = io.take<int32_t>(n_covis);
    const auto t_soff = io.take<int32_t>(n_kf + nd); const auto t_pflag = io.take<uint8_t>(n_points); const auto t_ref = io.take<int32_t>(n_points);
    const auto t_rscale = io.take<float>(n_points); const auto t_ooff = io.take<int32_t>(n_points + nd); const auto t_okf = io.take<int32_t>(n_obs);
    const auto t_oidx = io.take<int32_t>(n_obs); const auto t_sf = io.take<float>((size_t)n_levels); const auto t_sg = io.take<float>((size_t)n_levels);
    const auto t_pts = io.take<uint8_t>(68 * n_points);
    T.state_begins();
    const auto t_slot = io.take<int32_t>(n_slots); const auto t_nobs = io.take<int32_t>(n_points); const auto t_found = io.take<int32_t>(n_points);
    const auto t_vis = io.take<int32_t>(n_points);
    T.outputs_begin();
    const auto t_counts = io.take<int32_t>(nd * kNbCounts); const auto t_targets = io.take<int32_t>(nd * kNbMaxTargets);
    const auto t_tfused = io.take<int32_t>(nd * kNbMaxTargets); const auto t_cand = io.take<int32_t>(n_points); const auto t_ops = io.take<int32_t>(n_ops * 8);
    const auto t_bad = io.take<uint8_t>(n_points); const auto t_repl = io.take<int32_t>(n_points); const auto t_ooff_out = io.take<int32_t>(n_points + nd);
    const auto t_okf_out = io.take<int32_t>(n_obs_out); const auto t_oidx_out = io.take<int32_t>(n_obs_out); const auto t_dkf = io.take<int32_t>(n_points);
    const auto t_didx = io.take<int32_t>(n_points); const auto t_refreshed = io.take<uint8_t>(n_points); const auto t_normals = io.take<float>(3 * n_points);
    const auto t_mn = io.take<float>(n_points); const auto t_mx = io.take<float>(n_points);
    const auto w_pool = work.take<NbObs>(n_pool); const auto w_start = work.take<int32_t>(n_points); const auto w_len = work.take<int32_t>(n_points);
    const auto w_cap = work.take<int32_t>(n_points); const auto w_snap = work.take<int32_t>(n_snap);
    // the lock is held to the end: the results are read from the space's pinned block
    PackedSpace& S = shutdown_owned<PackedSpace, kSpaceNeighbors>();
    std::lock_guard<std::mutex> lk(S.mu);
    if (nd > 0) {
        TC2LI_HIP_CHECK(T.ensure(S));
        io.put(t_prob, 0, dev.data(), nd);
        io.put(t_sf, 0, scale_factors, (size_t)n_levels); io.put(t_sg, 0, inv_level_sigma2, (size_t)n_levels);
        tracking_pool().parallel_for((int)nd, [&](int d) {
            const Problem& in = problems[on_dev[d]];
            const NbProblemDev& D = dev[d];
            const size_t nk = (size_t)in.n_keyframes, np = (size_t)in.n_points;
            io.put(t_kfs, D.kf_off, kfs.data() + kf_first[on_dev[d]], nk); io.put(t_kflag, D.kf_off, in.kf_flags, nk); io.put(t_prev, D.kf_off, in.prev_kf, nk);
            io.put(t_coff, D.kf_row_off, in.covis_offsets, nk + 1); io.put(t_covis, D.covis_off, in.covis, (size_t)in.covis_offsets[nk]);
            io.put(t_soff, D.kf_row_off, in.slot_offsets, nk + 1); io.put(t_slot, D.slot_off, in.slot_point, (size_t)in.slot_offsets[nk]);
            if (np == 0) { const int32_t zero = 0; io.put(t_ooff, D.point_row_off, &zero, 1); return; }
            io.put(t_pflag, D.point_off, in.point_flags, np); io.put(t_ref, D.point_off, in.point_ref_kf, np); io.put(t_rscale, D.point_off, in.point_ref_level_scale, np);
            io.put(t_ooff, D.point_row_off, in.obs_offsets, np + 1); io.put(t_okf, D.obs_off, in.obs_kf, (size_t)D.n_obs); io.put(t_oidx, D.obs_off, in.obs_index, (size_t)D.n_obs);
            io.put(t_pts, 68 * (size_t)D.point_off, in.points, 68 * np);
            io.put(t_nobs, D.point_off, in.point_nobs, np); io.put(t_found, D.point_off, in.point_found, np); io.put(t_vis, D.point_off, in.point_visible, np);
        });
        // with tc2li_profile_enable(1) the two copies are bracketed by events like the launches: the report lists them by these names
        hipEvent_t up_a = nullptr, up_b = nullptr, down_a = nullptr, down_b = nullptr;
        const bool timed = prof::g_enabled.load(std::memory_order_relaxed) && prof::acquire("upload(search_in_neighbors)", &up_a, &up_b) &&
                           prof::acquire("download(search_in_neighbors)", &down_a, &down_b);
        if (timed) TC2LI_HIP_CHECK(hipEventRecord(up_a, st));
        TC2LI_HIP_CHECK(T.upload(st));
        if (timed) TC2LI_HIP_CHECK(hipEventRecord(up_b, st));
        // the state tables go up with the block: everything before outputs_begin()
        NbBatch B{};
        B.problems = T.dev(t_prob); B.kfs = T.dev(t_kfs); B.kf_flags = T.dev(t_kflag); B.prev_kf = T.dev(t_prev); B.covis_offsets = T.dev(t_coff);
        B.covis = T.dev(t_covis); B.slot_offsets = T.dev(t_soff); B.point_flags = T.dev(t_pflag); B.ref_kf = T.dev(t_ref); B.ref_scale = T.dev(t_rscale);
        B.obs_offsets = T.dev(t_ooff); B.obs_kf = T.dev(t_okf); B.obs_index = T.dev(t_oidx);
        B.c = NbConsts{cam4[0], cam4[1], cam4[2], cam4[3], bf, log_scale_factor, n_levels, 0, T.dev(t_sf), T.dev(t_sg)};
        B.slot_point = T.dev(t_slot); B.points = T.dev(t_pts); B.nobs = T.dev(t_nobs); B.found = T.dev(t_found); B.visible = T.dev(t_vis);
        B.pool = T.dev_work(w_pool); B.p_start = T.dev_work(w_start); B.p_len = T.dev_work(w_len); B.p_cap = T.dev_work(w_cap); B.snap = T.dev_work(w_snap);
        B.counts = T.dev(t_counts); B.targets = T.dev(t_targets); B.target_fused = T.dev(t_tfused); B.candidates = T.dev(t_cand); B.ops = T.dev(t_ops);
        B.bad = T.dev(t_bad); B.replaced = T.dev(t_repl); B.obs_offsets_out = T.dev(t_ooff_out); B.obs_kf_out = T.dev(t_okf_out); B.obs_index_out = T.dev(t_oidx_out);
        B.desc_kf = T.dev(t_dkf); B.desc_index = T.dev(t_didx); B.refreshed = T.dev(t_refreshed); B.normals = T.dev(t_normals); B.min_dist = T.dev(t_mn);
        B.max_dist = T.dev(t_mx);
        launch_search_in_neighbors(B, (int)nd, st);
        TC2LI_HIP_CHECK(hipGetLastError());
        if (timed) TC2LI_HIP_CHECK(hipEventRecord(down_a, st));
        TC2LI_HIP_CHECK(T.download(T.down_from, io.off, st));
        if (timed) TC2LI_HIP_CHECK(hipEventRecord(down_b, st));
        TC2LI_HIP_CHECK(stream_wait_blocking(st));
        for (size_t d = 0; d < nd; ++d) {
            const int32_t* c = T.host(t_counts) + kNbCounts * d;
            if (c[kNbStatus] == TC2LI_NEIGHBORS_ON_DEVICE) memcpy(problems[on_dev[d]].counts, c, kNbCounts * 4);
            else on_host[on_dev[d]] = 1;
        }
    }
    for (int p = 0; p < n_problems; ++p) if (dev_of[p] < 0) on_host[p] = 1;
    // ---- the host twin for what met a limit: the arrays of the slots those problems name come down once ----
    std::vector<int> host_list;
    for (int p = 0; p < n_problems; ++p) if (on_host[p]) host_list.push_back(p);
    if (!host_list.empty()) {
        std::map<int, HostSlot> slots;
        for (const int p : host_list)
            for (int k = 0; k < problems[p].n_keyframes; ++k) {
                const int s = problems[p].kf_slot[k];
                if (slots.count(s)) continue;
                const NbKf& d = kfs[kf_first[p] + k];
                HostSlot& h = slots[s];
                const size_t n = (size_t)d.n;
                h.keys.resize(std::max<size_t>(24 * n, 4)); h.desc.resize(std::max<size_t>(32 * n, 4)); h.u_right.resize(std::max<size_t>(n, 1));
                h.cell_start.resize(kCellsPlus1); h.items.resize(std::max<size_t>(n, 1));
                if (n) {
                    TC2LI_HIP_CHECK(hipMemcpyAsync(h.keys.data(), d.keys, 24 * n, hipMemcpyDeviceToHost, st));
                    TC2LI_HIP_CHECK(hipMemcpyAsync(h.desc.data(), d.desc, 32 * n, hipMemcpyDeviceToHost, st));
                    TC2LI_HIP_CHECK(hipMemcpyAsync(h.u_right.data(), d.u_right, 4 * n, hipMemcpyDeviceToHost, st));
                    TC2LI_HIP_CHECK(hipMemcpyAsync(h.items.data(), d.items, 2 * n, hipMemcpyDeviceToHost, st));
                }
                TC2LI_HIP_CHECK(hipMemcpyAsync(h.cell_start.data(), d.cell_start, 4 * (size_t)kCellsPlus1, hipMemcpyDeviceToHost, st));
            }
        TC2LI_HIP_CHECK(stream_wait_blocking(st));
        const NbConsts cc{cam4[0], cam4[1], cam4[2], cam4[3], bf, log_scale_factor, n_levels, 0, scale_factors, inv_level_sigma2};
        tracking_pool().parallel_for((int)host_list.size(), [&](int i) {
            const int p = host_list[i];
            const Problem& in = problems[p];
            std::vector<NbKf> hk(kfs.begin() + kf_first[p], kfs.begin() + kf_first[p + 1]);
            for (int k = 0; k < in.n_keyframes; ++k) {
                const HostSlot& h = slots.find(in.kf_slot[k])->second;
                hk[k].keys = reinterpret_cast<const float*>(h.keys.data()); hk[k].desc = h.desc.data(); hk[k].u_right = h.u_right.data();
                hk[k].cell_start = h.cell_start.data(); hk[k].items = h.items.data();
            }
            Twin(in, hk.data(), cc, results[p]).run();
            memcpy(in.counts, results[p].counts, sizeof(results[p].counts));
        });
    }
    for (int p = 0; p < n_problems; ++p)
        if (!fits(problems[p], problems[p].counts)) return capacity_error(entry, problems, p);
    // ---- every list fits: the results into the problems' arrays ----
    for (int p = 0; p < n_problems; ++p) {
        const Problem& in = problems[p];
        if (on_host[p]) { write_result(in, results[p]); continue; }
        const NbProblemDev& D = dev[dev_of[p]];
        const size_t d = (size_t)dev_of[p], np = (size_t)in.n_points;
        const int32_t* c = in.counts;
        if (in.targets) io.get(in.targets, t_targets, kNbMaxTargets * d, (size_t)c[kNbTargets]);
        if (in.target_fused) io.get(in.target_fused, t_tfused, kNbMaxTargets * d, (size_t)c[kNbTargets]);
        if (in.candidates) io.get(in.candidates, t_cand, D.point_off, (size_t)c[kNbCandidates]);
        if (in.ops) io.get(in.ops, t_ops, 8 * (size_t)D.op_off, 8 * (size_t)c[kNbOps]);
        if (in.slot_point_out) io.get(in.slot_point_out, t_slot, D.slot_off, (size_t)in.slot_offsets[in.n_keyframes]);
        if (in.point_bad_out) io.get(in.point_bad_out, t_bad, D.point_off, np);
        if (in.point_replaced) io.get(in.point_replaced, t_repl, D.point_off, np);
        if (in.point_nobs_out) io.get(in.point_nobs_out, t_nobs, D.point_off, np);
        if (in.point_found_out) io.get(in.point_found_out, t_found, D.point_off, np);
        if (in.point_visible_out) io.get(in.point_visible_out, t_vis, D.point_off, np);
        if (in.obs_offsets_out) io.get(in.obs_offsets_out, t_ooff_out, D.point_row_off, np + 1);
        if (in.obs_kf_out) io.get(in.obs_kf_out, t_okf_out, D.obs_out_off, (size_t)c[kNbObs]);
        if (in.obs_index_out) io.get(in.obs_index_out, t_oidx_out, D.obs_out_off, (size_t)c[kNbObs]);
        if (in.desc_kf) io.get(in.desc_kf, t_dkf, D.point_off, np);
        if (in.desc_index) io.get(in.desc_index, t_didx, D.point_off, np);
        if (in.refreshed) io.get(in.refreshed, t_refreshed, D.point_off, np);
        if (in.normals_out) io.get(in.normals_out, t_normals, 3 * (size_t)D.point_off, 3 * np);
        if (in.min_distance_out) io.get(in.min_distance_out, t_mn, D.point_off, np);
        if (in.max_distance_out) io.get(in.max_distance_out, t_mx, D.point_off, np);
    }
    return n_problems;
}
