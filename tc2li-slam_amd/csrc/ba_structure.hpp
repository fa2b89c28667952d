// The index structure of the projection-edge part of a local BA as a function of its own: what VisualProblem::setup (ba_internal.hpp)
// builds from (fixed, edges) before it touches the device -- free-pose numbering, the edges by landmark and by free pose, the slots of the W
// blocks, the slices of the Schur product, duplicates, the 256-slot blocks of the pose role, the groups of the linearisation and the sizes
// that follow from them -- and the layout of the window's input block as a function of those sizes alone.  Host only, no device call:
// tc2li_host_ba_structure (include/tc2li_hip.h) returns the record, and ba_structure_kernels.hip builds the same arrays on the device.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#include "ba_device.hpp"
#include "common.hpp"

namespace tc2li {
namespace ba_detail {

// What sizes the input block and the workspace of a window: a function of the structure, small enough to travel on its own.
struct BaStructureSizes {
    int32_t n_poses = 0, n_points = 0, n_edges = 0;
    int32_t n_free = 0;
    int32_t n_free_edges = 0;        // the SLOTS: edges with a free pose, duplicates of a (point, pose) pair not counted
    int32_t n_free_pose_edges = 0;   // edges with a free pose, duplicates counted (the room of the fl_* arrays and of pv_edges)
    int32_t n_dups = 0, n_blocks = 0, n_groups = 0, max_group_landmarks = 0;
    int32_t np = 0, np_pad = 0, n_schur_slices = 0, n_slices = 1, k_per_slice = 4, schur_group = 1, sparse = 0, schur_rd = 1, schur_ro = 1;
    bool lean_wide() const { return n_free > kSchurBlocksMaxFree && n_free <= kSchurLeanMaxFree; }
};

struct BaStructure : BaStructureSizes {
    std::vector<int> pose_var, pt_off, pt_edges, pv_off, pv_edges, fl_off, fl_pose, fl_lm, fl_place, fl_edge, w_slot, slice_off, dup_off, dup_edge,
        dup_slot, blk_off, grp_k0, grp_l0;
    std::vector<uint8_t> blk_rows;
    std::vector<uint32_t> chunk_mask;
};

// Whether a window of n_free free keyframes runs the lean block-by-block Schur product (the sparse path); sets the np_pad, slice and range
// fields of `s` from n_free and n_schur_slices.
inline void ba_structure_schur_sizes(BaStructureSizes& s) {
    const int n_free = s.n_free;
    const bool lean_wide = s.lean_wide();
    const bool sparse = (6 * n_free + 1 + 15) / 16 <= 8 || lean_wide;
    s.sparse = sparse ? 1 : 0;
    s.np = 6 * n_free;
    // sparse path: one spare row for W D^-1 b_l (row np of the product); dense path: the operands' width
    s.np_pad = sparse ? (s.np + 1 + 15) / 16 * 16 : std::max(16, (s.np + 15) / 16 * 16);
    s.schur_group = 1;
    if (sparse) {
        s.schur_group = kSchurGroupLean;  // slices per part
        s.n_slices = ba_schur_parts(s.n_schur_slices, s.schur_group);  // partial sums in S_part
        s.k_per_slice = 0;
    } else {
        // dense windows (round 5: d_ba_schur_units): the chunks (slices of slice_off: 16 landmarks each) in at most 8 ranges = partial sums
        const int want_slices = 8;  // (full-width form, 32 windows per launch beside two other groups: 2 / 4 / 8 slices 0.263 / 0.154 / 0.099 ms)
        s.k_per_slice = std::min(64, std::max(1, (s.n_schur_slices + want_slices - 1) / want_slices));   // chunks per partial sum (at most kUnitMaxChunks: ba_kernels.hip)
        s.n_slices = std::max(1, (s.n_schur_slices + s.k_per_slice - 1) / s.k_per_slice);
    }
    s.schur_rd = s.schur_ro = 1;
    if (sparse) {
        int rd = 1, ro = 1;
        if (lean_wide) schur_ranges_wide(n_free, rd, ro); else schur_ranges(n_free, rd, ro);
        s.schur_rd = rd; s.schur_ro = ro;
    }
}

// fixed [n_poses], edges [n_edges], extra_used [n_poses] or NULL (poses that count as used without an edge: the LiDAR / inertial terms')
// -> s.  TC2LI_OK, or TC2LI_ERR_INVALID with the error text set (an edge out of range, a point without an edge, a point with more than 256
// edges, more than 256 landmarks in a group, more than 85 free keyframes).
inline int ba_build_structure(const uint8_t* fixed, int n_poses, int n_points, const tc2li_ba_edge* edges, int n_edges, const uint8_t* extra_used,
                              BaStructure& s) {
    s.n_poses = n_poses; s.n_points = n_points; s.n_edges = n_edges;
    std::vector<int>& pose_var = s.pose_var;
    // ---- structure: free-pose numbering, CSR by landmark and by free pose ----
    pose_var.assign(n_poses, -1);
    int n_free = 0;
    std::vector<uint8_t> used(n_poses, 0);
    for (int e = 0; e < n_edges; ++e) {
        if (edges[e].pose < 0 || edges[e].pose >= n_poses || edges[e].point < 0 || edges[e].point >= n_points) {
            set_error("edge %d references pose %d / point %d out of range", e, edges[e].pose, edges[e].point);
            return TC2LI_ERR_INVALID;
        }
        used[edges[e].pose] = 1;
    }
    for (int k = 0; k < n_poses; ++k) if (extra_used && extra_used[k]) used[k] = 1;
    for (int k = 0; k < n_poses; ++k) if (!fixed[k] && used[k]) pose_var[k] = n_free++;
    s.n_free = n_free;
    std::vector<int>&pt_off = s.pt_off, &pt_edges = s.pt_edges, &pv_off = s.pv_off;
    pt_off.assign(n_points + 1, 0); pt_edges.assign(n_edges, 0); pv_off.assign(n_free + 1, 0);
    for (int e = 0; e < n_edges; ++e) { pt_off[edges[e].point + 1]++; if (pose_var[edges[e].pose] >= 0) pv_off[pose_var[edges[e].pose] + 1]++; }
    for (int l = 0; l < n_points; ++l) {
        if (pt_off[l + 1] == 0) { set_error("point %d has no edge", l); return TC2LI_ERR_INVALID; }
        pt_off[l + 1] += pt_off[l];
    }
    for (int i = 0; i < n_free; ++i) pv_off[i + 1] += pv_off[i];
    int n_free_edges = pv_off[n_free];  // edges with a free pose; after the slots are made: the SLOTS (duplicates of a (point, pose) pair have none)
    s.n_free_pose_edges = n_free_edges;
    std::vector<int>& pv_edges = s.pv_edges;
    pv_edges.assign(std::max(n_free_edges, 1), 0);
    {
        std::vector<int> fl(pt_off.begin(), pt_off.end() - 1), fp(pv_off.begin(), pv_off.end() - 1);
        for (int e = 0; e < n_edges; ++e) {
            pt_edges[fl[edges[e].point]++] = e;
            const int i = pose_var[edges[e].pose];
            if (i >= 0) pv_edges[fp[i]++] = e;
        }
    }
    // the edges with a free pose in landmark-major order: where the W blocks live (the Schur product and the back substitution walk
    // them by landmark)
    // fl_off: per landmark [begin, end) of its slots, the landmarks in index order.  (Tried: slots in the order of the poses a landmark
    // is seen from, so that a chunk of the Schur kernel spans a narrow band of poses and the product's empty tiles can be skipped -- the
    // windows' covisibility is not banded enough for that, and the linearisation lost its locality: 64 -> 98 us.)
    // Every window of at most kSchurLeanMaxFree (24) free keyframes runs the lean block-by-block Schur product (ba_device.hpp) -- up to
    // kSchurBlocksMaxFree (21) with one workgroup per part, above with two (schur_ranges_wide); wider windows the block-sparse MFMA kernels.
    const bool lean_wide = n_free > kSchurBlocksMaxFree && n_free <= kSchurLeanMaxFree;
    struct DupEdge { int pose, edge, slot; };
    std::vector<DupEdge> dups;
    std::vector<int>&fl_off = s.fl_off, &fl_pose = s.fl_pose, &fl_lm = s.fl_lm, &fl_place = s.fl_place, &fl_edge = s.fl_edge, &w_slot = s.w_slot,
        &slice_off = s.slice_off;
    fl_off.assign(2 * (size_t)n_points, 0); fl_pose.assign(std::max(n_free_edges, 1), 0); fl_lm.assign(std::max(n_free_edges, 1), 0);
    fl_place.assign(std::max(n_free_edges, 1), 0); fl_edge.assign(std::max(n_free_edges, 1), 0); w_slot.assign(n_edges, -1); slice_off.assign(1, 0);
    {
        // slices of the sparse Schur kernel: whole landmarks, at most 256 edges (one per thread) of at most 64 landmarks; a function of
        // the window alone, so that a window gives the same bits alone and in a batch
        // (the lean form of the block-by-block product stages half as many slots at a time: kSchurLeanSlots)
        // Dense windows (more than 21 free keyframes -- the temporal window of LocalInertialBA's bLarge case; round 5, d_ba_schur_units): the
        // slots follow the landmarks sorted by the first and the last free pose that sees them, and a slice is a CHUNK of 16 landmarks -- a
        // landmark of a temporal window is seen from a run of consecutive keyframes, so a chunk touches a band of the reduced system and the
        // product skips the rest.  (The covisibility windows of the sparse path are not banded: see above.)
        const bool dense_window = (6 * n_free + 1 + 15) / 16 > 8 && !lean_wide;
        const int kSliceEdges = dense_window ? std::numeric_limits<int>::max() : kSchurLeanSlots;
        const int kSliceLandmarks = dense_window ? kUnitChunkHost : 64;
        std::vector<int> order(n_points);
        for (int l = 0; l < n_points; ++l) order[l] = l;
        if (dense_window) {
            std::vector<int> first(n_points, std::numeric_limits<int>::max()), last(n_points, -1);
            for (int e = 0; e < n_edges; ++e) {
                const int i = pose_var[edges[e].pose], l = edges[e].point;
                if (i >= 0) { first[l] = std::min(first[l], i); last[l] = std::max(last[l], i); }
            }
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return first[a] != first[b] ? first[a] < first[b] : last[a] < last[b]; });
        }
        std::vector<int> seen(std::max(n_free, 1), -1), seen_slot(std::max(n_free, 1), -1);
        int at = 0, slice_lms = 0;
        for (int lo = 0; lo < n_points; ++lo) {
            const int l = order[lo];
            const int begin = at;
            for (int k = pt_off[l]; k < pt_off[l + 1]; ++k) {
                const int e = pt_edges[k], i = pose_var[edges[e].pose];
                if (i < 0) continue;
                // A second edge between the same point and the same free pose: g2o adds the two edges' blocks (BaseBinaryEdge::
                // constructQuadraticForm on the same Hpl / Hpp blocks, base_binary_edge.hpp:55-137).  The slot arrays hold one W block per
                // (landmark, pose): the later edge gets no slot -- k_ba_dups adds its W block to the first edge's slot and its pose block to
                // the pose's sums after the linearisation (round 5; rounds 2-4 refused such a window).  The reference's gather cannot produce
                // one for a pinhole rig, a two-camera shim can.
                if (seen[i] == l) { dups.push_back(DupEdge{i, e, seen_slot[i]}); continue; }
                seen[i] = l; seen_slot[i] = at;
                w_slot[e] = at; fl_pose[at] = i; fl_lm[at] = l; fl_edge[at] = e; ++at;
            }
            fl_off[2 * (size_t)l] = begin; fl_off[2 * (size_t)l + 1] = at;
            if (at == begin) continue;
            if (slice_lms == kSliceLandmarks || at - slice_off.back() > kSliceEdges) { slice_off.push_back(begin); slice_lms = 0; }
            for (int k = begin; k < at; ++k) fl_place[k] = slice_lms;
            ++slice_lms;
        }
        if (at > slice_off.back()) slice_off.push_back(at);
        n_free_edges = at;
    }
    s.n_free_edges = n_free_edges;
    s.n_dups = (int32_t)dups.size();
    // duplicates (k_ba_dups): by pose, in edge order; the per-pose edge lists of the dense windows' coefficient sums hold the slots' edges only
    std::vector<int>&dup_off = s.dup_off, &dup_edge = s.dup_edge, &dup_slot = s.dup_slot;
    dup_off.assign(n_free + 1, 0); dup_edge.assign(std::max(dups.size(), (size_t)1), 0); dup_slot.assign(std::max(dups.size(), (size_t)1), 0);
    if (!dups.empty()) {
        std::stable_sort(dups.begin(), dups.end(), [](const DupEdge& a, const DupEdge& b) { return a.pose != b.pose ? a.pose < b.pose : a.edge < b.edge; });
        for (size_t k = 0; k < dups.size(); ++k) { dup_off[dups[k].pose + 1]++; dup_edge[k] = dups[k].edge; dup_slot[k] = dups[k].slot; }
        for (int i = 0; i < n_free; ++i) dup_off[i + 1] += dup_off[i];
        std::fill(pv_off.begin(), pv_off.end(), 0);
        for (int e = 0; e < n_edges; ++e) if (w_slot[e] >= 0) pv_off[pose_var[edges[e].pose] + 1]++;
        for (int i = 0; i < n_free; ++i) pv_off[i + 1] += pv_off[i];
        std::vector<int> fp(pv_off.begin(), pv_off.end() - 1);
        for (int e = 0; e < n_edges; ++e) if (w_slot[e] >= 0) pv_edges[fp[pose_var[edges[e].pose]]++] = e;
    }
    // blocks of 256 free-pose edges (the pose role of the linearisation): the block's rows sorted by pose, for the per-pose sums
    const int n_blocks = (n_free_edges + 255) / 256;
    s.n_blocks = n_blocks;
    std::vector<int>& blk_off = s.blk_off;
    std::vector<uint8_t>& blk_rows = s.blk_rows;
    blk_off.assign((size_t)std::max(n_blocks, 1) * (n_free + 1), 0);
    blk_rows.assign((size_t)std::max(n_blocks, 1) * 256, 0);
    for (int b = 0; b < n_blocks; ++b) {
        int* off = blk_off.data() + (size_t)b * (n_free + 1);
        const int s0 = 256 * b, s1 = std::min(n_free_edges, s0 + 256);
        for (int sl = s0; sl < s1; ++sl) off[fl_pose[sl] + 1]++;
        for (int i = 0; i < n_free; ++i) off[i + 1] += off[i];
        std::vector<int> fill(off, off + n_free);
        for (int sl = s0; sl < s1; ++sl) blk_rows[(size_t)b * 256 + fill[fl_pose[sl]]++] = (uint8_t)(sl - s0);
    }
    // groups of the linearisation: whole landmarks, at most 256 edges (one per thread)
    std::vector<int>&grp_k0 = s.grp_k0, &grp_l0 = s.grp_l0;
    grp_k0.assign(1, 0); grp_l0.assign(1, 0);
    for (int l = 0; l < n_points; ++l) {
        if (pt_off[l + 1] - pt_off[l] > 256) { set_error("point %d has more than 256 edges", l); return TC2LI_ERR_INVALID; }
        if (pt_off[l + 1] - grp_k0.back() > 256) { grp_k0.push_back(pt_off[l]); grp_l0.push_back(l); }
    }
    grp_k0.push_back(n_edges); grp_l0.push_back(n_points);
    const int n_groups = (int)grp_k0.size() - 1;
    s.n_groups = n_groups;
    s.max_group_landmarks = 0;
    for (int g = 0; g < n_groups; ++g) s.max_group_landmarks = std::max(s.max_group_landmarks, grp_l0[g + 1] - grp_l0[g]);
    if (s.max_group_landmarks > 256) { set_error("more than 256 landmarks without edges in a row"); return TC2LI_ERR_INVALID; }  // (a landmark-role workgroup has a thread per landmark)
    s.n_schur_slices = (int)slice_off.size() - 1;
    ba_structure_schur_sizes(s);
    // which 16-column tiles of the reduced system a chunk of landmarks touches (bit t: a pose with columns in tile t sees one of them)
    std::vector<uint32_t>& chunk_mask = s.chunk_mask;
    chunk_mask.clear();
    if (!s.sparse) {
        if (s.np_pad / 16 > 32) { set_error("more than 85 free keyframes"); return TC2LI_ERR_INVALID; }
        chunk_mask.assign((size_t)std::max(s.n_schur_slices, 1), 0u);
        for (int c = 0; c < s.n_schur_slices; ++c)
            for (int sl = slice_off[c]; sl < slice_off[c + 1]; ++sl) {
                const int c0 = 6 * fl_pose[sl];
                chunk_mask[c] |= (1u << (c0 / 16)) | (1u << ((c0 + 5) / 16));
            }
    }
    return TC2LI_OK;
}

// ---- the input block: [poses | points | edges | pose_var | pt_off | pt_edges | pv_off | pv_edges | fl_off | fl_pose | chunk_mask | fl_lm |
// fl_place | slice_off | fl_edge | grp_k0 | grp_l0 | blk_off | blk_rows | ticket words | dup_off | dup_edge | dup_slot], every part 16-byte
// aligned; a function of the sizes alone ----
struct BaInputLayout {
    size_t o_poses, o_points, o_edges, o_pose_var, o_pt_off, o_pt_edges, o_pv_off, o_pv_edges, o_fl_off, o_fl_pose, o_w_slot, o_fl_lm, o_fl_place,
        o_slice_off, o_fl_edge, o_grp_k0, o_grp_l0, o_blk_off, o_blk_rows, o_ticket, o_dup_off, o_dup_edge, o_dup_slot, in_bytes;
    // how many entries the block holds of the arrays whose room is not their count
    size_t n_fl, n_pv_edges, n_chunk_mask, n_slice_off, n_grp, n_blk_off, n_blk_rows;
};
inline BaInputLayout ba_input_layout(const BaStructureSizes& s) {
    auto align16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
    const size_t E = s.n_edges, P = s.n_points, n_poses = s.n_poses, n_free = s.n_free, n_dups = s.n_dups;
    const bool sparse = s.sparse != 0;
    BaInputLayout L{};
    L.n_fl = (size_t)std::max(s.n_free_pose_edges, 1);
    L.n_pv_edges = sparse ? 0 : L.n_fl;
    L.n_chunk_mask = sparse ? 0 : (size_t)std::max(s.n_schur_slices, 1);
    L.n_slice_off = (size_t)s.n_schur_slices + 1;
    L.n_grp = (size_t)s.n_groups + 1;
    L.n_blk_off = (size_t)std::max(s.n_blocks, 1) * (n_free + 1);
    L.n_blk_rows = (size_t)std::max(s.n_blocks, 1) * 256;
    L.o_poses = 0; L.o_points = align16(L.o_poses + n_poses * sizeof(Se3)); L.o_edges = align16(L.o_points + 3 * P * sizeof(double));
    L.o_pose_var = align16(L.o_edges + E * sizeof(BaEdge)); L.o_pt_off = align16(L.o_pose_var + n_poses * sizeof(int));
    L.o_pt_edges = align16(L.o_pt_off + (P + 1) * sizeof(int)); L.o_pv_off = align16(L.o_pt_edges + E * sizeof(int));
    L.o_pv_edges = align16(L.o_pv_off + (n_free + 1) * sizeof(int)); L.o_fl_off = align16(L.o_pv_edges + L.n_pv_edges * sizeof(int));
    L.o_fl_pose = align16(L.o_fl_off + 2 * P * sizeof(int)); L.o_w_slot = align16(L.o_fl_pose + L.n_fl * sizeof(int));
    L.o_fl_lm = align16(L.o_w_slot + L.n_chunk_mask * sizeof(uint32_t)); L.o_fl_place = align16(L.o_fl_lm + L.n_fl * sizeof(int));
    L.o_slice_off = align16(L.o_fl_place + L.n_fl * sizeof(int)); L.o_fl_edge = align16(L.o_slice_off + L.n_slice_off * sizeof(int));
    L.o_grp_k0 = align16(L.o_fl_edge + L.n_fl * sizeof(int)); L.o_grp_l0 = align16(L.o_grp_k0 + L.n_grp * sizeof(int));
    L.o_blk_off = align16(L.o_grp_l0 + L.n_grp * sizeof(int)); L.o_blk_rows = align16(L.o_blk_off + L.n_blk_off * sizeof(int));
    L.o_ticket = align16(L.o_blk_rows + L.n_blk_rows); L.o_dup_off = align16(L.o_ticket + 4 * sizeof(int32_t));
    L.o_dup_edge = align16(L.o_dup_off + (n_dups ? n_free + 1 : 0) * sizeof(int));
    L.o_dup_slot = align16(L.o_dup_edge + n_dups * sizeof(int));
    L.in_bytes = align16(L.o_dup_slot + n_dups * sizeof(int));
    return L;
}

}  // namespace ba_detail
}  // namespace tc2li
