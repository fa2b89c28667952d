// The closing step of LocalLVBundleAdjustment on the resident map graph for gfx950 (include/tc2li_hip.h "the closing step of
// LocalLVBundleAdjustment"; SF/src/OptimizerWithLidar.cc:455-485): what a solved window writes into its sequence's tables, from where the
// BA left it on the device.  The host sends one MgApplyDev record per committed window (map_graph_device.hpp) and no value.
//   k_mgc_erase_log   one wavefront per window with erase pairs, the lanes over the pairs (:457-463).  A lane reads its pair from the
//                     device copy of the erase lists, turns it into (keyframe row, point row) through pose_row / point_row, finds the
//                     keyframe row in the point's CURRENT observation row by bisection (the rows ascend strictly) and takes the obs_index
//                     stored there -- GetIndexInKeyFrame of KeyFrame::EraseMapPointMatch(MapPoint*) -- then writes its two edits,
//                     SET_SLOT(kf row, index, -1) and ERASE_OBSERVATION(point row, kf row), at 2 i and 2 i + 1 of the window's log.  The
//                     log stays in device memory; k_mg_apply / k_mg_write (map_graph_kernels.hip) apply it.  Those kernels trust their
//                     edits, so every index is checked here.  An index that is no slot of the keyframe row (the row's matches are not
//                     resident: the gather reads the slots of the current keyframe and its neighbours only) leaves an edit of no op in
//                     place of the SET_SLOT, as the host's log leaves it out.  A pair that is out of range or not in the point's row
//                     gets two edits of no op and raises the window's status word, on which the host drops the whole commit.
//   k_mgc_scatter     one lane per (window, pose) and (window, point) of the whole batch (:468-484): a free pose goes to poses7 of its
//                     keyframe row, a point to positions of its point row, under TC2LI_BA_COMMIT_POSITIONS_F32 rounded through float
//                     (:482).  A window lists a row once, so no write meets another.
// Every loop runs to a bound in the host's record; no workgroup waits for another.
#include <algorithm>

#include "launch.hpp"
#include "map_graph_device.hpp"

namespace tc2li {
namespace {

__global__ __launch_bounds__(64) void k_mgc_erase_log(MgCommitBatch B) {
    const MgApplyDev& D = B.records[blockIdx.x];
    const MgTables& T = B.T;
    const size_t seq = (size_t)D.sequence, gen = seq * 2 + (size_t)D.generation;
    const int32_t* obs_off = T.obs_offsets + gen * ((size_t)T.cap_pt + 1);
    const int32_t* obs_kf = T.obs_kf + gen * T.cap_obs;
    const int32_t* obs_index = T.obs_index + gen * T.cap_obs;
    const int32_t* slot_offsets = T.slot_offsets + seq * ((size_t)T.cap_kf + 1);
    const int32_t* pose_row = B.pose_row + D.pad_[kMgcPoseOff];
    const int32_t* point_row = B.point_row + D.pad_[kMgcPointOff];
    const int32_t* erase_pose = B.erase + D.pad_[kMgcEraseAt];
    const int32_t* erase_point = erase_pose + D.pad_[kMgcEraseCap];
    tc2li_map_graph_edit* log = B.edits + D.edit_off;
    const int n_pairs = D.n_edits / 2;
    bool bad = false;
    for (int i = threadIdx.x; i < n_pairs; i += 64) {
        const int ep = erase_pose[i], et = erase_point[i];
        int kf = -1, pt = -1, index = -1;
        bool found = false;
        if (ep >= 0 && ep < D.pad_[kMgcPoses] && et >= 0 && et < D.pad_[kMgcPoints]) { kf = pose_row[ep]; pt = point_row[et]; }
        if (kf >= 0 && kf < D.n_kf && pt >= 0 && pt < D.n_points) {
            int lo = obs_off[pt], hi = obs_off[pt + 1];                                  // the first entry that is not below kf: at most 31 steps
            const int end = hi;
            for (int step = 0; step < 32 && lo < hi; ++step) {
                const int mid = lo + (hi - lo) / 2;
                if (obs_kf[mid] < kf) lo = mid + 1; else hi = mid;
            }
            if (lo < end && obs_kf[lo] == kf) {
                found = true;
                const int idx = obs_index[lo];
                if (idx >= 0 && idx < slot_offsets[kf + 1] - slot_offsets[kf]) index = idx;      // else: a row whose matches are not resident holds no such slot
            }
        }
        const tc2li_map_graph_edit none{kMgcNoEdit, 0, 0, 0};
        log[2 * i] = index >= 0 ? tc2li_map_graph_edit{TC2LI_MAP_GRAPH_SET_SLOT, kf, index, -1} : none;               // KeyFrame::EraseMapPointMatch (:461)
        log[2 * i + 1] = found ? tc2li_map_graph_edit{TC2LI_MAP_GRAPH_ERASE_OBSERVATION, pt, kf, 0} : none;           // MapPoint::EraseObservation (:462)
        bad |= !found;
    }
    const bool any_bad = __any(bad ? 1 : 0) != 0;
    if (threadIdx.x == 0) B.status[blockIdx.x] = any_bad ? 1 : 0;
}

__global__ __launch_bounds__(kMgcThreads) void k_mgc_scatter(MgCommitBatch B) {
    const MgApplyDev& D = B.records[blockIdx.y];
    const MgTables& T = B.T;
    const int n_poses = D.pad_[kMgcPoses], n_points = D.pad_[kMgcPoints];
    const int i = blockIdx.x * kMgcThreads + threadIdx.x;
    if (i >= n_poses + n_points) return;
    const size_t seq = (size_t)D.sequence;
    if (i < n_poses) {                                                                   // KeyFrame::SetPose of lLocalKeyFrames (:468-475)
        const size_t r = (size_t)D.pad_[kMgcPoseOff] + i;
        const int row = B.pose_row[r];
        if (B.fixed[r] || row < 0 || row >= D.n_kf) return;
        const double* src = B.poses7 + r * 7;
        double* dst = T.poses7 + (seq * T.cap_kf + row) * 7;
#pragma unroll
        for (int c = 0; c < 7; ++c) dst[c] = src[c];
    } else {                                                                             // MapPoint::SetWorldPos of lLocalMapPoints (:478-484)
        const size_t r = (size_t)D.pad_[kMgcPointOff] + (i - n_poses);
        const int row = B.point_row[r];
        if (row < 0 || row >= D.n_points) return;
        const double* src = B.points3 + r * 3;
        double* dst = T.positions + (seq * T.cap_pt + row) * 3;
        const bool as_float = (B.flags & TC2LI_BA_COMMIT_POSITIONS_F32) != 0;
#pragma unroll
        for (int c = 0; c < 3; ++c) dst[c] = as_float ? (double)(float)src[c] : src[c];  // vPoint->estimate().cast<float>() (:482)
    }
}

}  // namespace

void launch_map_graph_commit_erase_log(const MgCommitBatch& B, hipStream_t st) {
    if (B.n_erasing <= 0) return;
    TC2LI_LAUNCH(k_mgc_erase_log, dim3(B.n_erasing), dim3(64), 0, st, B);
}

void launch_map_graph_commit_scatter(const MgCommitBatch& B, hipStream_t st) {
    if (B.n <= 0 || B.max_rows <= 0) return;
    for (int first = 0; first < B.n; first += 65535) {                                   // (the grid's second extent ends at 65535)
        MgCommitBatch part = B;
        part.records = B.records + first; part.n = std::min(B.n - first, 65535);
        TC2LI_LAUNCH(k_mgc_scatter, dim3((B.max_rows + kMgcThreads - 1) / kMgcThreads, part.n), dim3(kMgcThreads), 0, st, part);
    }
}

}  // namespace tc2li
