// tc2li_host_ba_structure (include/tc2li_hip.h "the optimiser's index structure of a window"): the record of ba_build_structure
// (ba_structure.hpp) in the header's flat form.  tc2li_ba_window_structure_batch and tc2li_ba_window_solve_batch: the gather of
// ba_window_host.cpp followed by the structure kernels (ba_structure_kernels.hip) and, for the second, by the lock-step batch that adopts the
// windows where they are (ba_lockstep.cpp, VisualProblem::adopt).
#include <algorithm>
#include <cstring>
#include <mutex>

#include "lockstep_host.hpp"
#include "map_graph_host.hpp"

namespace tc2li {
namespace ba_detail {

void ba_structure_scalars(const BaStructureSizes& s, int32_t* sc) {
    sc[TC2LI_BA_STRUCTURE_N_FREE] = s.n_free; sc[TC2LI_BA_STRUCTURE_N_SLOTS] = s.n_free_edges;
    sc[TC2LI_BA_STRUCTURE_N_FREE_POSE_EDGES] = s.n_free_pose_edges; sc[TC2LI_BA_STRUCTURE_N_DUPS] = s.n_dups;
    sc[TC2LI_BA_STRUCTURE_N_BLOCKS] = s.n_blocks; sc[TC2LI_BA_STRUCTURE_N_GROUPS] = s.n_groups;
    sc[TC2LI_BA_STRUCTURE_MAX_GROUP_LANDMARKS] = s.max_group_landmarks; sc[TC2LI_BA_STRUCTURE_NP] = s.np; sc[TC2LI_BA_STRUCTURE_NP_PAD] = s.np_pad;
    sc[TC2LI_BA_STRUCTURE_N_SCHUR_SLICES] = s.n_schur_slices; sc[TC2LI_BA_STRUCTURE_N_SLICES] = s.n_slices;
    sc[TC2LI_BA_STRUCTURE_K_PER_SLICE] = s.k_per_slice; sc[TC2LI_BA_STRUCTURE_SCHUR_GROUP] = s.schur_group; sc[TC2LI_BA_STRUCTURE_SPARSE] = s.sparse;
    sc[TC2LI_BA_STRUCTURE_SCHUR_RD] = s.schur_rd; sc[TC2LI_BA_STRUCTURE_SCHUR_RO] = s.schur_ro;
}

// the counts of the flat form's fields, in the enum's order
void ba_structure_counts(const BaStructureSizes& s, bool with_host_only, int32_t* count) {
    const int blocks = std::max(s.n_blocks, 1);
    count[TC2LI_BA_STRUCTURE_SCALARS] = TC2LI_BA_STRUCTURE_SCALAR_COUNT;
    count[TC2LI_BA_STRUCTURE_POSE_VAR] = s.n_poses; count[TC2LI_BA_STRUCTURE_PT_OFF] = s.n_points + 1; count[TC2LI_BA_STRUCTURE_PT_EDGES] = s.n_edges;
    count[TC2LI_BA_STRUCTURE_PV_OFF] = s.n_free + 1;
    count[TC2LI_BA_STRUCTURE_PV_EDGES] = with_host_only || !s.sparse ? s.n_free_edges : 0;
    count[TC2LI_BA_STRUCTURE_FL_OFF] = 2 * s.n_points;
    count[TC2LI_BA_STRUCTURE_FL_POSE] = count[TC2LI_BA_STRUCTURE_FL_LM] = count[TC2LI_BA_STRUCTURE_FL_PLACE] = count[TC2LI_BA_STRUCTURE_FL_EDGE] = s.n_free_edges;
    count[TC2LI_BA_STRUCTURE_W_SLOT] = with_host_only ? s.n_edges : 0;
    count[TC2LI_BA_STRUCTURE_SLICE_OFF] = s.n_schur_slices + 1;
    count[TC2LI_BA_STRUCTURE_DUP_OFF] = with_host_only || s.n_dups ? s.n_free + 1 : 0;
    count[TC2LI_BA_STRUCTURE_DUP_EDGE] = count[TC2LI_BA_STRUCTURE_DUP_SLOT] = s.n_dups;
    count[TC2LI_BA_STRUCTURE_BLK_OFF] = blocks * (s.n_free + 1); count[TC2LI_BA_STRUCTURE_BLK_ROWS] = blocks * 256;
    count[TC2LI_BA_STRUCTURE_GRP_K0] = count[TC2LI_BA_STRUCTURE_GRP_L0] = s.n_groups + 1;
    count[TC2LI_BA_STRUCTURE_CHUNK_MASK] = s.sparse ? 0 : std::max(s.n_schur_slices, 1);
}

// table from the counts; returns the total
int64_t ba_structure_table(const int32_t* count, int32_t* table) {
    int64_t at = 0;
    for (int f = 0; f < TC2LI_BA_STRUCTURE_FIELDS; ++f) {
        table[2 * f] = (int32_t)std::min<int64_t>(at, 0x7fffffff); table[2 * f + 1] = count[f];
        at += count[f];
    }
    return at;
}

}  // namespace ba_detail
}  // namespace tc2li

using namespace tc2li;
using namespace tc2li::ba_detail;

extern "C" int tc2li_host_ba_structure(const uint8_t* fixed, int n_poses, int n_points, const tc2li_ba_edge* edges, int n_edges,
                                       const uint8_t* extra_used, int32_t* table, int32_t* out, int capacity) {
    const char* entry = "tc2li_host_ba_structure";
    if (n_poses < 0 || n_points < 0 || n_edges < 0 || capacity < 0 || (n_poses && !fixed) || (n_edges && !edges) || !table || (capacity && !out)) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    BaStructure s;
    const int rc = ba_build_structure(fixed, n_poses, n_points, edges, n_edges, extra_used, s);
    if (rc != TC2LI_OK) return rc;
    int32_t count[TC2LI_BA_STRUCTURE_FIELDS];
    ba_structure_counts(s, true, count);
    const int64_t total = ba_structure_table(count, table);
    if (total > 0x7fffffff) {
        set_error("%s: the structure takes more than 2^31 entries", entry);
        return TC2LI_ERR_INVALID;
    }
    if (!out) return (int)total;
    if (total > capacity) {
        set_error("%s: %lld entries, room for %d", entry, (long long)total, capacity);
        return TC2LI_ERR_CAPACITY;
    }
    ba_structure_scalars(s, out + table[2 * TC2LI_BA_STRUCTURE_SCALARS]);
    auto put = [&](int f, const int* src) { if (count[f]) memcpy(out + table[2 * f], src, (size_t)count[f] * sizeof(int32_t)); };
    put(TC2LI_BA_STRUCTURE_POSE_VAR, s.pose_var.data()); put(TC2LI_BA_STRUCTURE_PT_OFF, s.pt_off.data()); put(TC2LI_BA_STRUCTURE_PT_EDGES, s.pt_edges.data());
    put(TC2LI_BA_STRUCTURE_PV_OFF, s.pv_off.data()); put(TC2LI_BA_STRUCTURE_PV_EDGES, s.pv_edges.data()); put(TC2LI_BA_STRUCTURE_FL_OFF, s.fl_off.data());
    put(TC2LI_BA_STRUCTURE_FL_POSE, s.fl_pose.data()); put(TC2LI_BA_STRUCTURE_FL_LM, s.fl_lm.data()); put(TC2LI_BA_STRUCTURE_FL_PLACE, s.fl_place.data());
    put(TC2LI_BA_STRUCTURE_FL_EDGE, s.fl_edge.data()); put(TC2LI_BA_STRUCTURE_W_SLOT, s.w_slot.data()); put(TC2LI_BA_STRUCTURE_SLICE_OFF, s.slice_off.data());
    put(TC2LI_BA_STRUCTURE_DUP_OFF, s.dup_off.data()); put(TC2LI_BA_STRUCTURE_DUP_EDGE, s.dup_edge.data()); put(TC2LI_BA_STRUCTURE_DUP_SLOT, s.dup_slot.data());
    put(TC2LI_BA_STRUCTURE_BLK_OFF, s.blk_off.data()); put(TC2LI_BA_STRUCTURE_GRP_K0, s.grp_k0.data()); put(TC2LI_BA_STRUCTURE_GRP_L0, s.grp_l0.data());
    for (int k = 0; k < count[TC2LI_BA_STRUCTURE_BLK_ROWS]; ++k) out[table[2 * TC2LI_BA_STRUCTURE_BLK_ROWS] + k] = s.blk_rows[k];
    for (int k = 0; k < count[TC2LI_BA_STRUCTURE_CHUNK_MASK]; ++k) out[table[2 * TC2LI_BA_STRUCTURE_CHUNK_MASK] + k] = (int32_t)s.chunk_mask[k];
    return (int)total;
}

// ---- the structure built on the device from the gather's output: what the two device entries share -------------------------------------
namespace tc2li {
namespace {

struct BasSpace {
    std::mutex mu;
    DevBuf<uint8_t> scratch, blocks;
    DevBuf<BasWindowDev> d_windows;
    DevBuf<BasSizes> d_sizes;
    PinnedBuf<BasWindowDev> h_windows;
    PinnedBuf<BasSizes> h_sizes;
    PinnedBuf<int32_t> h_pose_var;   // the windows' pose_var back to back (window p at win[p].pose_var)
    PinnedBuf<CopyTask> h_tasks;
    PinnedBuf<uint8_t> h_blocks;
    PinnedBuf<int32_t> h_erase;      // per window [n_erase | pad | erase_pose cap | erase_point cap]
    DevBuf<int32_t> d_erase;         // the same blocks in device memory: what a commit reads (tc2li_ba_window_solve_graph_commit_batch)
};
// [0]: tc2li_ba_window_structure_batch's; [1 + group]: tc2li_ba_window_solve_batch's on the lock-step context `group`
struct BasSpaces { BasSpace s[1 + kMaxLockstepGroups]; };

// The sizes of a window's structure from the record its kernels left (a gathered window has no duplicate pair).
ba_detail::BaStructureSizes sizes_of(const BasSizes& r, const int32_t* counts) {
    ba_detail::BaStructureSizes s;
    s.n_poses = counts[TC2LI_BA_WINDOW_N_POSES]; s.n_points = counts[TC2LI_BA_WINDOW_N_POINTS]; s.n_edges = counts[TC2LI_BA_WINDOW_N_EDGES];
    s.n_free = r.n_free; s.n_free_edges = s.n_free_pose_edges = r.n_free_edges; s.n_dups = 0;
    s.n_blocks = r.n_blocks; s.n_groups = r.n_groups; s.max_group_landmarks = r.max_group_landmarks; s.n_schur_slices = r.n_schur_slices;
    ba_detail::ba_structure_schur_sizes(s);
    return s;
}

// Queues the structure kernels behind the gather and the download of what the host needs of them: the size records and pose_var.
struct StructureBase : BawFollow {
    const tc2li_ba_window_problem* problems = nullptr;
    int n = 0;
    std::vector<uint8_t> use_lidar;   // per window: the keyframes of lidar_pose_index count as used
    BasSpace& S;
    std::vector<BasWindowDev> win;
    explicit StructureBase(BasSpace& space) : S(space) {}

    int after_gather(const BawBatch& B, const BawProblemDev* dev, hipStream_t st) override {
        win.assign(n, BasWindowDev{});
        int64_t at = 0;   // in ints; every piece starts at a multiple of 16 bytes
        auto take = [&at](int64_t ints) { const int64_t o = at; at = (at + ints + 3) & ~(int64_t)3; return o; };
        int max_blocks = 1;
        for (int p = 0; p < n; ++p) win[p].pose_var = take(dev[p].pose_cap);   // first, back to back: they come down in one copy
        const int64_t pose_var_ints = at;
        for (int p = 0; p < n; ++p) {
            const int64_t P = dev[p].point_cap, E = dev[p].edge_cap;
            BasWindowDev& w = win[p];
            w.max_blocks = (int32_t)std::max<int64_t>(1, (E + 255) / 256);
            w.use_lidar = use_lidar[p];
            w.pt_off = take(P + 1); w.pt_edges = take(E); w.pv_off = take(kBasMaxFree + 2); w.fl_off = take(2 * P);
            w.fl_pose = take(E); w.fl_lm = take(E); w.fl_place = take(E); w.fl_edge = take(E); w.slice_off = take(P + 2);
            w.grp_k0 = take(P + 2); w.grp_l0 = take(P + 2); w.blk_off = take((int64_t)w.max_blocks * (kBasMaxFree + 1));
            w.blk_rows = 4 * take((int64_t)w.max_blocks * 64);
            max_blocks = std::max(max_blocks, (int)w.max_blocks);
        }
        TC2LI_HIP_CHECK(S.scratch.ensure((size_t)std::max<int64_t>(at, 4) * 4));
        TC2LI_HIP_CHECK(S.d_windows.ensure(n)); TC2LI_HIP_CHECK(S.h_windows.ensure(n));
        TC2LI_HIP_CHECK(S.d_sizes.ensure(n)); TC2LI_HIP_CHECK(S.h_sizes.ensure(n));
        TC2LI_HIP_CHECK(S.h_pose_var.ensure((size_t)std::max<int64_t>(pose_var_ints, 4)));
        memcpy(S.h_windows.p, win.data(), (size_t)n * sizeof(BasWindowDev));
        TC2LI_HIP_CHECK(hipMemcpyAsync(S.d_windows.p, S.h_windows.p, (size_t)n * sizeof(BasWindowDev), hipMemcpyHostToDevice, st));
        BasBatch A{};
        A.n_windows = n; A.max_blocks = max_blocks; A.problems = static_cast<const BawProblemDev*>(B.problems); A.counts = B.counts; A.lidar_pose_index = B.lidar_pose_index;
        A.fixed = B.fixed; A.edge_start = B.edge_start; A.edges = B.edges; A.windows = S.d_windows.p;
        A.scratch = reinterpret_cast<int32_t*>(S.scratch.p); A.scratch_rows = S.scratch.p; A.sizes = S.d_sizes.p;
        launch_ba_structure(A, st);
        TC2LI_HIP_CHECK(hipGetLastError());
        TC2LI_HIP_CHECK(hipMemcpyAsync(S.h_sizes.p, S.d_sizes.p, (size_t)n * sizeof(BasSizes), hipMemcpyDeviceToHost, st));
        if (pose_var_ints) TC2LI_HIP_CHECK(hipMemcpyAsync(S.h_pose_var.p, S.scratch.p, (size_t)pose_var_ints * 4, hipMemcpyDeviceToHost, st));
        return 0;
    }

    // where the pieces of window p's input block lie in device memory (the block's poses, points and edges are copies of the gather's output)
    void pieces_of(const BawBatch& B, const BawProblemDev* dev, int p, ba_detail::BaPrepared& pr) const {
        const int32_t* scratch = reinterpret_cast<const int32_t*>(S.scratch.p);
        const BasWindowDev& w = win[p];
        pr.pose_var_host = S.h_pose_var.p + w.pose_var;
        pr.poses = B.poses7_out + (size_t)dev[p].pose_off * 7; pr.points = B.points3_out + (size_t)dev[p].pointo_off * 3; pr.edges = B.edges + dev[p].edge_off;
        pr.pose_var = scratch + w.pose_var; pr.pt_off = scratch + w.pt_off; pr.pt_edges = scratch + w.pt_edges; pr.pv_off = scratch + w.pv_off;
        pr.fl_off = scratch + w.fl_off; pr.fl_pose = scratch + w.fl_pose; pr.fl_lm = scratch + w.fl_lm; pr.fl_place = scratch + w.fl_place;
        pr.slice_off = scratch + w.slice_off; pr.fl_edge = scratch + w.fl_edge; pr.grp_k0 = scratch + w.grp_k0; pr.grp_l0 = scratch + w.grp_l0;
        pr.blk_off = scratch + w.blk_off; pr.blk_rows = S.scratch.p + w.blk_rows;
    }
};

// tc2li_ba_window_structure_batch: the input blocks are laid out and filled as the BA would have them, then downloaded and taken apart
struct StructureFollow : StructureBase {
    int32_t *tables = nullptr, *out = nullptr, *results = nullptr;
    int out_stride = 0;
    using StructureBase::StructureBase;

    int after_download(const BawBatch& B, const BawProblemDev* dev, hipStream_t st) override {
        using namespace ba_detail;
        std::vector<BaStructureSizes> sizes(n);
        std::vector<BaInputLayout> lay(n);
        std::vector<size_t> block_at(n, 0);
        std::vector<int32_t> count((size_t)n * TC2LI_BA_STRUCTURE_FIELDS, 0);
        size_t bytes = 0;
        bool short_of_room = false;
        for (int p = 0; p < n; ++p) {
            const BasSizes& r = S.h_sizes.p[p];
            int32_t* table = tables + (size_t)p * 2 * TC2LI_BA_STRUCTURE_FIELDS;
            std::fill(table, table + 2 * TC2LI_BA_STRUCTURE_FIELDS, 0);
            results[p] = r.status == kBasInvalid ? TC2LI_ERR_INVALID : r.status == kBasDeclined ? TC2LI_BA_STRUCTURE_DECLINED : 0;
            if (r.status != kBasBuilt) continue;
            sizes[p] = sizes_of(r, problems[p].counts);
            if (!sizes[p].sparse) { set_error("tc2li_ba_window_structure_batch: problem %d: the device built a window outside the sparse path", p); return TC2LI_ERR_HIP; }
            lay[p] = ba_input_layout(sizes[p]);
            block_at[p] = bytes;
            bytes += (lay[p].in_bytes + 255) & ~(size_t)255;
            int32_t* c = count.data() + (size_t)p * TC2LI_BA_STRUCTURE_FIELDS;
            ba_structure_counts(sizes[p], false, c);
            const int64_t total = ba_structure_table(c, table);
            results[p] = (int32_t)std::min<int64_t>(total, 0x7fffffff);
            if (total > out_stride) short_of_room = true;
        }
        if (short_of_room) {
            set_error("tc2li_ba_window_structure_batch: a window's structure does not fit out_stride = %d", out_stride);
            return TC2LI_ERR_CAPACITY;
        }
        if (!bytes) return 0;
        TC2LI_HIP_CHECK(S.blocks.ensure(bytes)); TC2LI_HIP_CHECK(S.h_blocks.ensure(bytes));
        TC2LI_HIP_CHECK(S.h_tasks.ensure((size_t)n * 20));
        int n_tasks = 0;
        size_t max_bytes = 0;
        for (int p = 0; p < n; ++p) {
            if (S.h_sizes.p[p].status != kBasBuilt) continue;
            const BaStructureSizes& s = sizes[p];
            const BaInputLayout& L = lay[p];
            BaPrepared pr;
            pieces_of(B, dev, p, pr);
            uint8_t* blk = S.blocks.p + block_at[p];
            auto add = [&](size_t o, const void* src, size_t b) {
                if (!b) return;
                S.h_tasks.p[n_tasks++] = CopyTask{blk + o, src, b};
                max_bytes = std::max(max_bytes, b);
            };
            const size_t K = s.n_poses, P = s.n_points, E = s.n_edges, F = s.n_free_edges;
            add(L.o_poses, pr.poses, K * sizeof(Se3)); add(L.o_points, pr.points, 3 * P * sizeof(double)); add(L.o_edges, pr.edges, E * sizeof(BaEdge));
            add(L.o_pose_var, pr.pose_var, K * 4); add(L.o_pt_off, pr.pt_off, (P + 1) * 4); add(L.o_pt_edges, pr.pt_edges, E * 4);
            add(L.o_pv_off, pr.pv_off, ((size_t)s.n_free + 1) * 4); add(L.o_fl_off, pr.fl_off, 2 * P * 4);
            add(L.o_fl_pose, pr.fl_pose, F * 4); add(L.o_fl_lm, pr.fl_lm, F * 4); add(L.o_fl_place, pr.fl_place, F * 4);
            add(L.o_slice_off, pr.slice_off, L.n_slice_off * 4); add(L.o_fl_edge, pr.fl_edge, F * 4);
            add(L.o_grp_k0, pr.grp_k0, L.n_grp * 4); add(L.o_grp_l0, pr.grp_l0, L.n_grp * 4);
            add(L.o_blk_off, pr.blk_off, L.n_blk_off * 4); add(L.o_blk_rows, pr.blk_rows, L.n_blk_rows);
            add(L.o_ticket, nullptr, 4 * sizeof(int32_t));
        }
        launch_copy_tasks(S.h_tasks.p, n_tasks, max_bytes, st);
        TC2LI_HIP_CHECK(hipGetLastError());
        TC2LI_HIP_CHECK(hipMemcpyAsync(S.h_blocks.p, S.blocks.p, bytes, hipMemcpyDeviceToHost, st));
        TC2LI_HIP_CHECK(stream_wait_blocking(st));
        std::atomic<bool> numbering_differs{false};
        tracking_pool().parallel_for(n, [&](int p) {
            if (S.h_sizes.p[p].status != kBasBuilt) return;
            const uint8_t* blk = S.h_blocks.p + block_at[p];
            const BaInputLayout& L = lay[p];
            const int32_t* table = tables + (size_t)p * 2 * TC2LI_BA_STRUCTURE_FIELDS;
            int32_t* o = out + (size_t)p * out_stride;
            ba_structure_scalars(sizes[p], o + table[2 * TC2LI_BA_STRUCTURE_SCALARS]);
            auto get = [&](int f, size_t from) { if (table[2 * f + 1]) memcpy(o + table[2 * f], blk + from, (size_t)table[2 * f + 1] * 4); };
            get(TC2LI_BA_STRUCTURE_POSE_VAR, L.o_pose_var); get(TC2LI_BA_STRUCTURE_PT_OFF, L.o_pt_off); get(TC2LI_BA_STRUCTURE_PT_EDGES, L.o_pt_edges);
            get(TC2LI_BA_STRUCTURE_PV_OFF, L.o_pv_off); get(TC2LI_BA_STRUCTURE_FL_OFF, L.o_fl_off); get(TC2LI_BA_STRUCTURE_FL_POSE, L.o_fl_pose);
            get(TC2LI_BA_STRUCTURE_FL_LM, L.o_fl_lm); get(TC2LI_BA_STRUCTURE_FL_PLACE, L.o_fl_place); get(TC2LI_BA_STRUCTURE_FL_EDGE, L.o_fl_edge);
            get(TC2LI_BA_STRUCTURE_SLICE_OFF, L.o_slice_off); get(TC2LI_BA_STRUCTURE_BLK_OFF, L.o_blk_off); get(TC2LI_BA_STRUCTURE_GRP_K0, L.o_grp_k0);
            get(TC2LI_BA_STRUCTURE_GRP_L0, L.o_grp_l0);
            for (int k = 0; k < table[2 * TC2LI_BA_STRUCTURE_BLK_ROWS + 1]; ++k) o[table[2 * TC2LI_BA_STRUCTURE_BLK_ROWS] + k] = blk[L.o_blk_rows + k];
            if (memcmp(S.h_pose_var.p + win[p].pose_var, blk + L.o_pose_var, (size_t)sizes[p].n_poses * 4) != 0) numbering_differs = true;
        });
        if (numbering_differs) {   // (what the solve entry hands the LiDAR term's host steps is the copy that came down beside the size records)
            set_error("tc2li_ba_window_structure_batch: the downloaded pose numbering is not the block's");
            return TC2LI_ERR_HIP;
        }
        return 0;
    }
};

// tc2li_ba_window_solve_batch: the BA of the windows the device prepared, the rest through the one-window path
struct SolveFollow : StructureBase {
    const tc2li_ba_window_solve_problem* solve = nullptr;
    const tc2li_camera* cam = nullptr;
    int group = 0;
    int32_t* results = nullptr;
    // tc2li_ba_window_solve_graph_commit_batch: the lease of the gather, under whose lock the solved windows are written into their sequences
    MgLease* commit = nullptr;
    uint32_t commit_flags = 0;
    const char* entry = "tc2li_ba_window_solve_batch";
    using StructureBase::StructureBase;

    int after_counts() override {
        for (int p = 0; p < n; ++p) {
            const tc2li_ba_window_solve_problem& q = solve[p];
            if ((q.edge_chi2 || q.edge_depth_positive) && q.window.counts[TC2LI_BA_WINDOW_N_EDGES] > q.edge_out_capacity) {
                set_error("tc2li_ba_window_solve_batch: problem %d has %d edges and room for %d chi2 / depth flags", p, q.window.counts[TC2LI_BA_WINDOW_N_EDGES],
                          q.edge_out_capacity);
                return TC2LI_ERR_CAPACITY;
            }
        }
        return 0;
    }

    int after_download(const BawBatch& B, const BawProblemDev* dev, hipStream_t st) override {
        using namespace ba_detail;
        const BaOptions opt = BaOptions::read();
        std::vector<tc2li_ba_problem> prob(n);
        std::vector<tc2li_lidar_window> lidar(n);
        std::vector<std::vector<float>> cloud(n);
        std::vector<std::vector<int32_t>> cloud_off(n);
        std::vector<int> alive, built;   // not ABORTED; of those, the ones the device prepared
        for (int p = 0; p < n; ++p) {
            const tc2li_ba_window_solve_problem& q = solve[p];
            const int32_t* c = q.window.counts;
            results[p] = 0;
            if (q.n_erase) *q.n_erase = 0;
            if (c[TC2LI_BA_WINDOW_STATUS] != TC2LI_BA_WINDOW_OK) continue;
            alive.push_back(p);
            tc2li_ba_problem& b = prob[p];
            b = tc2li_ba_problem{};
            b.poses7 = q.window.poses7_out; b.fixed = q.window.fixed; b.points3 = q.window.points3_out; b.edges = q.window.edges;
            b.n_poses = c[TC2LI_BA_WINDOW_N_POSES]; b.n_points = c[TC2LI_BA_WINDOW_N_POINTS]; b.n_edges = c[TC2LI_BA_WINDOW_N_EDGES];
            b.iterations = q.iterations; b.lambda_init = q.lambda_init; b.stop_flag = q.stop_flag; b.edge_chi2 = q.edge_chi2;
            b.edge_depth_positive = q.edge_depth_positive; b.stats = q.stats; b.lidar_stats = q.lidar_stats;
            const int n_lidar = c[TC2LI_BA_WINDOW_N_LIDAR];
            if (q.cloud_xyz && n_lidar > 0) {   // the window of :226-253 from the keyframe rows' clouds
                tc2li_lidar_window& L = lidar[p];
                L = tc2li_lidar_window{};
                cloud_off[p].assign(1, 0);
                for (int k = 0; k < n_lidar; ++k) {
                    const int row = q.window.pose_row[q.window.lidar_pose_index[k]];
                    const int32_t a = q.cloud_offsets[row], e = q.cloud_offsets[row + 1];
                    if (e > a) cloud[p].insert(cloud[p].end(), q.cloud_xyz + 3 * (size_t)a, q.cloud_xyz + 3 * (size_t)e);
                    cloud_off[p].push_back(cloud_off[p].back() + std::max(e - a, 0));
                }
                L.n_keyframes = n_lidar; L.pose_index = q.window.lidar_pose_index; L.cloud_xyz = cloud[p].data(); L.cloud_offsets = cloud_off[p].data();
                memcpy(L.Tcl, q.Tcl, sizeof(L.Tcl)); L.weight = q.weight;
                b.lidar = &L;
            }
            if (S.h_sizes.p[p].status == kBasBuilt) built.push_back(p);
        }
        // a batch of one and TC2LI_BA_NO_LOCKSTEP take the one-window path in the two-step form too
        const bool lockstep = opt.lockstep && alive.size() > 1;
        std::vector<uint8_t> done(n, 0);
        // per prepared window [n_erase | pad | erase_pose | erase_point], pinned: the outlier kernel writes there
        std::vector<size_t> erase_at(n, 0);
        size_t erase_ints = 0;
        for (int p : built) { erase_at[p] = erase_ints; erase_ints += 4 + 2 * (size_t)std::max(std::min(solve[p].erase_capacity, prob[p].n_edges), 0); }
        if (lockstep && !built.empty()) {
            TC2LI_HIP_CHECK(S.h_erase.ensure(std::max<size_t>(erase_ints, 4)));
            if (commit) TC2LI_HIP_CHECK(S.d_erase.ensure(std::max<size_t>(erase_ints, 4)));
            std::vector<tc2li_ba_problem> bp(built.size());
            std::vector<BaPrepared> prep(built.size());
            std::vector<int32_t> rc(built.size(), 0);
            for (size_t k = 0; k < built.size(); ++k) {
                const int p = built[k];
                bp[k] = prob[p];
                prep[k].sizes = sizes_of(S.h_sizes.p[p], solve[p].window.counts);
                pieces_of(B, dev, p, prep[k]);
                if (solve[p].n_erase) {
                    const int cap = std::max(std::min(solve[p].erase_capacity, prob[p].n_edges), 0);
                    int32_t* e = S.h_erase.p + erase_at[p];
                    e[0] = 0;
                    prep[k].n_erase = e; prep[k].erase_pose = e + 4; prep[k].erase_point = e + 4 + cap; prep[k].erase_capacity = cap;
                    if (commit) { prep[k].write_back = true; prep[k].erase_dev = S.d_erase.p + erase_at[p]; }
                }
            }
            if (ba_batch_lockstep(bp.data(), (int)bp.size(), cam, named_pool(kPoolBaGroup0 + group), rc.data(), group, prep.data())) {
                for (size_t k = 0; k < built.size(); ++k) {
                    const int p = built[k];
                    results[p] = rc[k];
                    done[p] = 1;
                    if (rc[k] < 0 || !solve[p].n_erase) continue;
                    const int32_t* e = S.h_erase.p + erase_at[p];
                    const int m = std::min(e[0], prep[k].erase_capacity);
                    *solve[p].n_erase = e[0];
                    if (m > 0) { memcpy(solve[p].erase_pose, e + 4, (size_t)m * 4); memcpy(solve[p].erase_point, e + 4 + prep[k].erase_capacity, (size_t)m * 4); }
                }
            }
        }
        // what is left: declined by the device or by the lock-step group, a batch of one, an INVALID window -- the existing path, edges on the host
        for (int p : alive) {
            if (done[p]) continue;
            const tc2li_ba_window_solve_problem& q = solve[p];
            tc2li_ba_problem& b = prob[p];
            std::vector<tc2li_ba_edge> edges_here;
            if (!b.edges && b.n_edges > 0) {
                edges_here.resize(b.n_edges);
                TC2LI_HIP_CHECK(hipMemcpyAsync(edges_here.data(), B.edges + dev[p].edge_off, (size_t)b.n_edges * sizeof(tc2li_ba_edge), hipMemcpyDeviceToHost, st));
                TC2LI_HIP_CHECK(stream_wait_blocking(st));
                b.edges = edges_here.data();
            }
            std::vector<double> chi2_here;
            std::vector<uint8_t> depth_here;
            if (q.n_erase) {   // the outlier rule needs both, whether the caller asked for them or not
                if (!b.edge_chi2) { chi2_here.resize(std::max(b.n_edges, 1)); b.edge_chi2 = chi2_here.data(); }
                if (!b.edge_depth_positive) { depth_here.resize(std::max(b.n_edges, 1)); b.edge_depth_positive = depth_here.data(); }
            }
            results[p] = tc2li_local_lv_bundle_adjustment(b.poses7, b.fixed, b.n_poses, b.points3, b.n_points, b.edges, b.n_edges, cam, b.iterations, b.lambda_init,
                                                          b.stop_flag, b.edge_chi2, b.edge_depth_positive, b.stats, b.lidar, b.lidar_stats, private_stream());
            if (results[p] < 0 || !q.n_erase) continue;
            std::vector<uint8_t> nobody_bad(std::max(b.n_points, 1), 0);
            const int cap = std::max(q.erase_capacity, 0);
            std::vector<int32_t> ep(std::max(b.n_edges, 1)), et(std::max(b.n_edges, 1));
            const int m = tc2li_ba_window_outliers(b.edges, b.edge_chi2, b.edge_depth_positive, b.n_edges, nobody_bad.data(), b.n_points, ep.data(), et.data(), b.n_edges);
            if (m < 0) return m;
            *q.n_erase = m;
            if (std::min(m, cap) > 0) { memcpy(q.erase_pose, ep.data(), (size_t)std::min(m, cap) * 4); memcpy(q.erase_point, et.data(), (size_t)std::min(m, cap) * 4); }
        }
        for (int p : alive)
            if (solve[p].n_erase && *solve[p].n_erase > std::max(solve[p].erase_capacity, 0)) {
                set_error("tc2li_ba_window_solve_batch: problem %d has %d outlier pairs and room for %d", p, *solve[p].n_erase, solve[p].erase_capacity);
                return TC2LI_ERR_CAPACITY;
            }
        if (!commit) return 0;
        // ---- "Recover optimized data" (OptimizerWithLidar.cc:455-485) into the resident tables: no error can follow that would have to undo it ----
        std::vector<MgCommitWindow> on_device;
        std::vector<int> on_host;
        for (int p : alive) {
            if (results[p] < 0) continue;
            if (!done[p]) { on_host.push_back(p); continue; }
            const int32_t* c = solve[p].window.counts;
            MgCommitWindow w{};
            w.sequence = commit->sequences[p];
            w.pose_off = dev[p].pose_off; w.point_off = dev[p].pointo_off; w.n_poses = c[TC2LI_BA_WINDOW_N_POSES]; w.n_points = c[TC2LI_BA_WINDOW_N_POINTS];
            w.n_erase = *solve[p].n_erase; w.erase_at = (int32_t)erase_at[p] + 4; w.erase_cap = std::max(std::min(solve[p].erase_capacity, prob[p].n_edges), 0);
            w.erase_point = solve[p].erase_point;
            on_device.push_back(w);
        }
        // a window finished on the host path: its log from the sequence's tables and its host arrays (tc2li_host_ba_window_commit_log)
        std::vector<MgHostTables> tables(on_host.size());
        std::vector<std::vector<tc2li_map_graph_edit>> log_edits(on_host.size());
        std::vector<std::vector<double>> log_values(on_host.size());
        std::vector<tc2li_map_graph_delta> logs(on_host.size());
        for (size_t k = 0; k < on_host.size(); ++k) {
            const int p = on_host[k];
            const int32_t* c = solve[p].window.counts;
            const int rrc = map_graph_read(entry, *commit, commit->sequences[p], &tables[k]);
            if (rrc < 0) return rrc;
            log_edits[k].resize(2 * (size_t)std::max(*solve[p].n_erase, 0) + c[TC2LI_BA_WINDOW_N_POSES] + c[TC2LI_BA_WINDOW_N_POINTS] + 1);
            log_values[k].resize(7 * (size_t)c[TC2LI_BA_WINDOW_N_POSES] + 3 * (size_t)c[TC2LI_BA_WINDOW_N_POINTS] + 1);
            int32_t n_values = 0;
            const int n_edits = tc2li_host_ba_window_commit_log(&tables[k].tables, &solve[p], results[p], commit_flags, log_edits[k].data(), (int)log_edits[k].size(),
                                                                log_values[k].data(), (int)log_values[k].size(), nullptr, &n_values);
            if (n_edits < 0) return n_edits;
            logs[k] = tc2li_map_graph_delta{log_edits[k].data(), log_values[k].data(), commit->sequences[p], n_edits, n_values, 0};
        }
        const MgCommitSource src{B.pose_row, B.fixed, B.poses7_out, B.point_row, B.points3_out, S.d_erase.p};
        return map_graph_commit(entry, *commit, src, on_device, logs.data(), (int)logs.size(), commit_flags, st);
    }
};

}  // namespace
}  // namespace tc2li

extern "C" int tc2li_ba_window_solve_limits(int32_t* out, int capacity) {
    if (!out || capacity < 4) {
        set_error("tc2li_ba_window_solve_limits: room for 4 values is needed");
        return TC2LI_ERR_INVALID;
    }
    out[0] = kBasMaxFree; out[1] = kBasMaxPoses; out[2] = kBasMaxPoints; out[3] = kBasThreads;
    return 4;
}

extern "C" int tc2li_ba_window_structure_batch(tc2li_keyframe_store* store, const tc2li_ba_window_problem* problems, int n_problems,
                                               const float* inv_level_sigma2, int n_levels, const uint8_t* with_lidar, int32_t* tables, int32_t* out,
                                               int out_stride, int32_t* results, void* stream) {
    const char* entry = "tc2li_ba_window_structure_batch";
    if (out_stride < 0 || (n_problems > 0 && (!tables || !results || (out_stride && !out)))) {
        set_error("%s: null or negative argument", entry);
        return TC2LI_ERR_INVALID;
    }
    BasSpace& S = shutdown_owned<BasSpaces>().s[0];
    std::lock_guard<std::mutex> lk(S.mu);
    StructureFollow F(S);
    F.problems = problems; F.n = n_problems; F.tables = tables; F.out = out; F.results = results; F.out_stride = out_stride;
    F.use_lidar.assign(std::max(n_problems, 0), 1);
    for (int p = 0; p < n_problems && with_lidar; ++p) F.use_lidar[p] = with_lidar[p] ? 1 : 0;
    return ba_window_batch_run(entry, store, problems, n_problems, inv_level_sigma2, n_levels, stream, &F, 0, false);
}

namespace {
// tc2li_ba_window_solve_batch, or with a graph tc2li_ba_window_solve_graph_batch: the windows' tables from the sequences of the map graph
// commit: the solved windows are then written into their sequences (tc2li_ba_window_solve_graph_commit_batch)
int solve_batch(const char* entry, tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                const tc2li_ba_window_solve_problem* problems, int n_problems, const float* inv_level_sigma2, int n_levels, const tc2li_camera* cam,
                int group, int32_t* results, bool commit = false, uint32_t flags = 0, bool cov = false) {
    if (n_problems < 0 || (n_problems > 0 && (!problems || !results)) || !cam || group < 0 || group >= kMaxLockstepGroups) {
        set_error("%s: invalid argument (group 0 .. %d)", entry, kMaxLockstepGroups - 1);
        return TC2LI_ERR_INVALID;
    }
    std::vector<tc2li_ba_window_problem> windows(std::max(n_problems, 0));
    for (int p = 0; p < n_problems; ++p) {
        const tc2li_ba_window_solve_problem& q = problems[p];
        if (q.iterations < 0 || q.edge_out_capacity < 0 || q.erase_capacity < 0 || (q.cloud_xyz && !q.cloud_offsets) ||
            (q.n_erase && q.erase_capacity > 0 && (!q.erase_pose || !q.erase_point))) {
            set_error("%s: problem %d: negative iterations or capacity, clouds without offsets, or null erase arrays", entry, p);
            return TC2LI_ERR_INVALID;
        }
        if (commit && !q.n_erase) { set_error("%s: problem %d: n_erase is NULL: the commit is defined by the outlier rule", entry, p); return TC2LI_ERR_INVALID; }
        windows[p] = q.window;
    }
    if (commit) {
        if (flags & ~(uint32_t)TC2LI_BA_COMMIT_POSITIONS_F32) { set_error("%s: unknown flag bits", entry); return TC2LI_ERR_INVALID; }
        if (n_problems > 0 && !sequences) { set_error("%s: null sequences", entry); return TC2LI_ERR_INVALID; }
        std::vector<int32_t> named(sequences, sequences + n_problems);   // the local mapping of a map is one thread
        std::sort(named.begin(), named.end());
        if (std::adjacent_find(named.begin(), named.end()) != named.end()) { set_error("%s: a sequence is named by two problems", entry); return TC2LI_ERR_INVALID; }
    }
    MgLease lease;
    if (graph) {
        const int lrc = resident_windows(entry, &lease, store, graph, sequences, n_problems, &windows);
        if (lrc < 0) return lrc;
        if (cov) {
            const int crc = resident_cov(entry, &lease, windows.data(), n_problems);
            if (crc < 0) return crc;
        }
    }
    BasSpace& S = shutdown_owned<BasSpaces>().s[1 + group];
    std::lock_guard<std::mutex> lk(S.mu);
    SolveFollow F(S);
    F.problems = windows.data(); F.n = n_problems; F.solve = problems; F.cam = cam; F.group = group; F.results = results;
    F.entry = entry; F.commit = commit ? &lease : nullptr; F.commit_flags = flags;
    F.use_lidar.assign(std::max(n_problems, 0), 0);
    for (int p = 0; p < n_problems; ++p) F.use_lidar[p] = problems[p].cloud_xyz ? 1 : 0;
    return ba_window_batch_run(entry, store, windows.data(), n_problems, inv_level_sigma2, n_levels, nullptr, &F, 1 + group, true, graph ? &lease : nullptr);
}
}  // namespace

extern "C" int tc2li_ba_window_solve_batch(tc2li_keyframe_store* store, const tc2li_ba_window_solve_problem* problems, int n_problems,
                                           const float* inv_level_sigma2, int n_levels, const tc2li_camera* cam, int group, int32_t* results) {
    return solve_batch("tc2li_ba_window_solve_batch", store, nullptr, nullptr, problems, n_problems, inv_level_sigma2, n_levels, cam, group, results);
}

extern "C" int tc2li_ba_window_solve_graph_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                                                 const tc2li_ba_window_solve_problem* problems, int n_problems, const float* inv_level_sigma2, int n_levels,
                                                 const tc2li_camera* cam, int group, int32_t* results) {
    if (!graph) { set_error("tc2li_ba_window_solve_graph_batch: null graph"); return TC2LI_ERR_INVALID; }
    return solve_batch("tc2li_ba_window_solve_graph_batch", store, graph, sequences, problems, n_problems, inv_level_sigma2, n_levels, cam, group, results);
}

extern "C" int tc2li_ba_window_solve_graph_commit_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                                                        const tc2li_ba_window_solve_problem* problems, int n_problems, const float* inv_level_sigma2,
                                                        int n_levels, const tc2li_camera* cam, int group, uint32_t flags, int32_t* results) {
    const char* entry = "tc2li_ba_window_solve_graph_commit_batch";
    if (!graph) { set_error("%s: null graph", entry); return TC2LI_ERR_INVALID; }
    return solve_batch(entry, store, graph, sequences, problems, n_problems, inv_level_sigma2, n_levels, cam, group, results, true, flags);
}

extern "C" int tc2li_ba_window_solve_graph_commit_cov_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                                                            const tc2li_ba_window_solve_problem* problems, int n_problems, const float* inv_level_sigma2,
                                                            int n_levels, const tc2li_camera* cam, int group, uint32_t flags, int32_t* results) {
    const char* entry = "tc2li_ba_window_solve_graph_commit_cov_batch";
    if (!graph) { set_error("%s: null graph", entry); return TC2LI_ERR_INVALID; }
    return solve_batch(entry, store, graph, sequences, problems, n_problems, inv_level_sigma2, n_levels, cam, group, results, true, flags, true);
}
