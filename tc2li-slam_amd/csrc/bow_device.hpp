// Device side of the ORB vocabulary (include/tc2li_hip.h "ORB vocabulary"): DBoW2's TemplatedVocabulary::transform and
// ORBmatcher::SearchByBoW(KeyFrame*, Frame&) on gfx950 (bow_kernels.hip); bow_host.cpp owns the handle and sequences the calls.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orb_device.hpp"
#include "pose_opt_device.hpp"

namespace tc2li {

// One node of the device tree.  Nodes are renumbered breadth first so that the children of every internal node are one contiguous
// block of rows in child order: children are rows first .. first + cnt - 1.
struct BowNodeDev {
    int32_t first;   // device index of the first child (0 for a leaf)
    int32_t cnt;     // number of children (0: a leaf, i.e. a word)
    int32_t ref;     // the reference's node id (what mFeatVec records)
    int32_t word;    // word id of a leaf, -1 for an internal node
};

struct BowVocDev {
    const uint4* rows;          // [n_nodes][2]: the 32 descriptor bytes of every node, device order
    const BowNodeDev* nodes;    // [n_nodes]
    const double* weight;       // [n_nodes] node weight (idf / 1 as trained)
    int32_t n_nodes, n_words;
};

// Where frame f's descriptors are read (src_row, in rows of 32 bytes) and its outputs are written (out_off: the per-descriptor
// arrays, the BowVector and FeatureVector slices; fv_offset at out_off + f), and how many descriptors it has.
struct BowFrameDev {
    int32_t src_row, out_off, n, pad_;
};

struct BowOutDev {
    int32_t* word;        // [..] per descriptor, -1 when stopped
    int32_t* node;
    int32_t* n_words;     // [n_frames]
    int32_t* bow_word;
    double* bow_value;
    int32_t* n_nodes;     // [n_frames]
    int32_t* fv_node;
    int32_t* fv_offset;
    int32_t* fv_index;
    int32_t* n_valid;     // [n_frames] features that were not stopped
    uint32_t* rank;       // [..] scratch: rank of the feature in (node, index) order, flags and word count
    int32_t* flags;       // [..] scratch: bit 0 first of its node, bit 1 first of its word, bits 2.. features with the same word
};

// One common node of a (keyframe, frame) pair of SearchByBoW: the keyframe's features kf_idx[0 .. kf_n) and the frame's
// f_idx[0 .. f_n) (indices into the pair's arrays), in FeatureVector order.
struct BowTaskDev {
    int32_t pair, kf_pos, kf_n, f_pos, f_n, pad_[3];
};

struct BowPairDev {
    int32_t kf_key, f_key;     // first row of the pair's keyframe / frame keypoints in the staged descriptor and angle arrays
    int32_t f_n;               // F.N
    int32_t out_off;           // pair * capacity
    float nn_ratio;
    int32_t check_orientation;
};

// TrackReferenceKeyFrame: frame f is pair f (kf_key: the reference keyframe's first row in the staged arrays, f_key: the frame's first
// keypoint in the extractor's device arrays, out_off = f * capacity)
struct BowRefConst {
    float inv_sigma2[kMaxLevels];  // mvInvLevelSigma2
};

struct BowRefArgs {
    int n_frames, n_tasks;
    const BowTaskDev* tasks;       // one per node of every reference keyframe: pair = frame, kf_pos / kf_n its features
    const int32_t* kf_node;        // [n_tasks] the node id of the task
    const BowPairDev* pairs;       // [n_frames]
    const uint8_t* kf_desc;        // staged keyframe arrays, rows from pairs[f].kf_key
    const uint8_t* kf_has_point;
    const uint8_t* kf_observed;    // pMP->Observations() > 0
    const float* kf_angle;
    const float* kf_Xw;            // [..][3]
    const int32_t* kf_fv_index;
    const float* last_pose7;       // [n_frames][7]
    const uint8_t* f_desc;         // the extractor's device-resident features
    const float* f_angle;
    const MatchKey* keys;
    const float* u_right;          // [n_frames][capacity]
    BowOutDev O;                   // the frames' transform
    BowRefConst C;
    int32_t* match;                // [n_frames][capacity] kf_keypoint_of_keypoint
    int32_t* n_matches;
    PoseProblem* probs;
    BaEdge* edges;
    double* Xw;
    int32_t* edge_kp;
    double* poses;
    uint8_t* outlier;
    int32_t* inliers;
    int32_t* n_inliers;
    int32_t* n_matches_map;
};

void launch_bow_descend(const BowVocDev& V, const uint8_t* desc, const BowFrameDev* frames, int n_frames, int max_n, int nid_level,
                        const BowOutDev& O, hipStream_t st);
void launch_bow_assemble(const BowVocDev& V, const double* word_weight, const BowFrameDev* frames, int n_frames, int scoring, int weighting,
                         const BowOutDev& O, hipStream_t st);
void launch_bow_search(const BowTaskDev* tasks, int n_tasks, const BowPairDev* pairs, int n_pairs, const uint8_t* desc, const float* angle,
                       const uint8_t* has_point, const int32_t* fv_index, int32_t* match, int32_t* n_matches, hipStream_t st);
// search, rotation filter and PoseOptimization edges of TrackReferenceKeyFrame; then launch_pose_optimization; then the finish
void launch_bow_reference(const BowRefArgs& A, hipStream_t st);
void launch_bow_reference_finish(const BowRefArgs& A, hipStream_t st);

}  // namespace tc2li
