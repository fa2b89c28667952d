// Device side of relocalisation (include/tc2li_hip.h "Relocalisation"): TemplatedVocabulary::score,
// KeyFrameDatabase::DetectRelocalizationCandidates and the bookkeeping of the refinement ladder on gfx950 (reloc_kernels.hip);
// reloc_host.cpp owns the database handle and sequences the calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tracking_device.hpp"

namespace tc2li {

constexpr int kRelocMaxWords = 4096;       // words per BowVector
constexpr int kRelocMaxLive = 4096;        // live keyframes per database: the size of the per-query sort
constexpr int kRelocMaxNeighbours = 10;    // GetBestCovisibilityKeyFrames(10)

// One keyframe row of a database's pool: words pool[off .. off + n), ascending.
struct RelocRowDev {
    int32_t off, n;
    int32_t live;
    int32_t map_id, kf_id;
    int32_t n_cov;
    int32_t cov[kRelocMaxNeighbours];      // pool row of every neighbour, -1 for an id that is no live entry
};

// One query: its database's device arrays, the frame's BowVector in the staged arrays, and where its scratch and outputs start.
struct RelocQueryDev {
    const int32_t* kf_word;                // the database's pool
    const double* kf_value;
    const RelocRowDev* rows;
    float* score;                          // [n_rows] the score state (mRelocScore)
    int32_t n_rows;
    int32_t f_off, f_n;                    // the frame's words in f_word / f_value
    int32_t map_id;
    int32_t row_off;                       // first slot of the query's per-row scratch
    int32_t pad_;
};

// a pair of tc2li_vocabulary_score_batch in the staged arrays
struct RelocPairDev {
    int32_t off1, n1, off2, n2;
};

struct RelocArgs {
    const RelocQueryDev* queries;
    int n_queries, max_rows, scoring;
    const int32_t* f_word;
    const double* f_value;
    // per (query, row) scratch, [total rows]
    int32_t* common;                       // mnRelocWords
    int32_t* first_word;                   // the smallest shared word
    float* si;                             // (float)score(F, KF)
    // per query outputs; list arrays [n_queries][list_cap]
    int capacity, list_cap;
    int32_t* n_candidates;
    int32_t* candidates;                   // [n_queries][capacity], preset to -1
    int32_t* n_scored;
    int32_t* sc_row;                       // the entry's pool row
    int32_t* sc_kf;
    int32_t* sc_words;
    float* sc_si;
    float* sc_acc;
    int32_t* sc_best_row;
    int32_t* sc_best;
};

// ---- the refinement ladder of Tracking::Relocalization (SF/src/Tracking.cc:3562-3631), hypothesis h ----
enum RelocStatus {
    kRelocOpt1 = 1,        // the first PoseOptimization ran (always)
    kRelocRejected = 2,    // nGood < 10 after it: `continue`
    kRelocSearch1 = 4,     // SearchByProjection(.., 10, 100) ran
    kRelocOpt2 = 8,        // nadditional + nGood >= 50: the second PoseOptimization ran
    kRelocSearch2 = 16,    // 30 < nGood < 50: SearchByProjection(.., 3, 64) ran
    kRelocOpt3 = 32,       // nGood + nadditional >= 50: the third PoseOptimization ran
    kRelocSuccess = 64     // nGood >= 50 at the end
};

struct RelocLadder {
    int n_hyps, capacity;
    TrackFrameDev* frames;         // [n_hyps] pose7 = the frame's current pose, th / slot of the search pass; key_off / n_keys the frame's keypoints
    const int32_t* frame_of_hyp;   // [n_hyps] frame_index (u_right rows)
    const MatchKey* keys;          // the extractor's device arrays
    const float* u_right;          // [n_frames][capacity]
    float inv_sigma2[kMaxLevels];
    const float* kf_Xw;            // query-indexed
    const int32_t* in_match;       // [n_hyps][capacity] vvpMapPointMatches as keyframe keypoints
    const uint8_t* in_inlier;      // [n_hyps][capacity] vbInliers
    uint8_t* found;                // query-indexed: sFound
    uint8_t* occupied;             // [n_hyps][capacity]
    int32_t* assign;               // [n_hyps][capacity] mvpMapPoints as keyframe keypoints
    uint8_t* outlier_of_key;       // [n_hyps][capacity] mvbOutlier of the last PoseOptimization
    int32_t* n_matches;            // [n_hyps] the search's result
    int32_t* active;               // [n_hyps] part of the stage in progress
    int32_t* status;
    int32_t* n_good;
    int32_t* n_additional;         // [n_hyps][2]
    double* stage_poses;           // [n_hyps][3][7]
    // PoseOptimization
    PoseProblem* probs;
    BaEdge* edges;
    double* Xw;
    int32_t* edge_kp;
    double* poses;
    const uint8_t* outlier;
    const int32_t* inliers;
};
void launch_reloc_ladder_init(const RelocLadder& L, hipStream_t st);
// before PoseOptimization number `stage` (0, 1, 2): the gate on the preceding search's result, then the edges of the hypotheses that pass
void launch_reloc_ladder_edges(const RelocLadder& L, int stage, hipStream_t st);
// after it: nGood, the pose, the discard (stages 0 and 2), the outlier flags, and who takes part in the search that follows
void launch_reloc_ladder_after(const RelocLadder& L, int stage, hipStream_t st);

void launch_bow_score(const RelocPairDev* pairs, int n_pairs, const int32_t* word, const double* value, int scoring, double* out, hipStream_t st);
void launch_reloc_candidates(const RelocArgs& A, hipStream_t st);

}  // namespace tc2li
