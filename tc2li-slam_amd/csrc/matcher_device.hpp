// Shared between the host orchestration and the projection-matching kernel.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "global_ptr.hpp"
#include "orb_device.hpp"  // MatchKey

namespace tc2li {

constexpr int kMaxMatchKeys = 3072;  // keypoints of one frame that fit the LDS working set
constexpr int kCellsPlus1 = 64 * 48 + 1;  // cell_start entries of one frame: the feature grid of matcher_kernels.hip (kCells) + 1

struct MatchQuery {  // tc2li_proj_query, 64 bytes
    float u, v, radius, u_right;
    int32_t min_level, max_level;
    float angle;
    int16_t valid, has_observations;
    uint8_t desc[32];
};
static_assert(sizeof(MatchQuery) == 64, "layout");

struct MatchFrameDev {
    const MatchKey* keys;
    const uint8_t* desc;      // 32 bytes per key, 16-byte aligned (read as two 16-byte loads)
    const float* u_right;
    const uint8_t* occupied;
    const MatchQuery* queries;
    int32_t n_keys, n_queries, query_off, pad_;
    float min_x, max_x, min_y, max_y;
};

#if defined(__HIPCC__)
__device__ __forceinline__ MatchFrameDev global_record(MatchFrameDev f) {  // global_ptr.hpp
    TC2LI_GLOBAL_FIELD(f, keys); TC2LI_GLOBAL_FIELD(f, desc); TC2LI_GLOBAL_FIELD(f, u_right); TC2LI_GLOBAL_FIELD(f, occupied); TC2LI_GLOBAL_FIELD(f, queries);
    return f;
}
#endif

// the three-launch form (grid, candidate lists, rounds over the lists); the tables live in the caller's workspace.  When
// pool_top[1] comes back non-zero the candidate pool was too small and launch_match_by_projection has to be used instead.
struct MatchLists {
    int32_t* cell_start;   // [nframes][kCellsPlus1]
    uint16_t* items;       // [total keys], frame f at key_base[f]
    const int32_t* key_base;  // [nframes]
    int32_t* cand_off;     // [total queries]
    int32_t* cand_cnt;     // [total queries], bit 30 = has_observations
    uint32_t* pool;
    int32_t* pool_top;     // [0] = entries used, [1] = overflow flag
    int32_t pool_cap;
    int32_t grid_ready;    // launch_match_lists: cell_start / items hold the frames' grids already (frame_grids of projection_search.hpp)
    const int32_t* cell_row;  // frame f's row of cell_start is cell_row[f]; NULL = row f (the keyframe store: row = slot; a pass over some
                              // of a handle's frames: row = frame)
};
// only the feature grids (cell_start, items) of the frames: used by the fuse search as well
void launch_match_grid(const MatchFrameDev* frames, int nframes, const MatchLists& L, hipStream_t st);
// max_dist: the best distance a match may have -- TH_HIGH of the frame and map-point overloads, ORBdist of the keyframe overload
constexpr int kMatchThHigh = 100;
void launch_match_lists(const MatchFrameDev* frames, int nframes, const int32_t* query_frame, int total_q, const MatchLists& L, int mode,
                        float nn_ratio, int32_t* match_of_query, int32_t* prev_claim, int32_t* rounds_out, hipStream_t st,
                        int max_dist = kMatchThHigh);
void launch_match_by_projection(const MatchFrameDev* frames, int nframes, int mode, float nn_ratio, int32_t* match_of_query,
                                int32_t* prev_claim, int32_t* rounds_out, hipStream_t st, int max_dist = kMatchThHigh);

}  // namespace tc2li
