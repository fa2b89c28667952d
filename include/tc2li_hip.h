/*
 * tc2li_hip.h -- C ABI of the MI355X (gfx950) implementation of TC2LI-SLAM's per-frame front end and
 * local bundle adjustment.  Plain pointers and sizes only; every entry point names the reference call
 * site it replaces (paths relative to the reference tree, SF/ = slam_framework/).
 *
 * Conventions
 *   - return value: >= 0 success (often a count), < 0 a tc2li_status error.  tc2li_last_error() gives text.
 *   - "host" pointers are ordinary process memory, "dev" pointers are HIP device memory on the current device.
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).
 *   - there is no CPU fallback: every compute entry point fails with TC2LI_ERR_NO_DEVICE without a GPU.
 */
#ifndef TC2LI_HIP_H
#define TC2LI_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum tc2li_status {
    TC2LI_OK = 0,
    TC2LI_ERR_INVALID = -2,    /* bad argument */
    TC2LI_ERR_NO_DEVICE = -3,  /* no HIP device / HIP runtime failure at init */
    TC2LI_ERR_HIP = -4,        /* a HIP call failed; see tc2li_last_error() */
    TC2LI_ERR_CAPACITY = -5,   /* caller-provided buffer too small */
    TC2LI_ERR_COMM = -6,       /* the all-reduce of a sharded window failed (or librccl could not be loaded) */
    TC2LI_ERR_EMPTY = -1       /* empty image: the reference returns -1 (SF/src/ORBextractor.cc:1063-1064) */
} tc2li_status;

const char* tc2li_last_error(void);
/* ABI version, bumped on any signature change. */
int tc2li_abi_version(void);
/* Number of visible HIP devices (0 without a GPU; never fails). */
int tc2li_device_count(void);
/* Hardware queues the HIP runtime maps this process's streams onto (the runtime's GPU_MAX_HW_QUEUES, 4 by default).  A process that runs
 * ONE sequence -- the reference's own configuration: tracking, LiDAR and local-mapping threads with a stream each, every kernel tiny --
 * should ask for 8 (streams that share a queue wait for each other: 479 against 761 frames/s) -- 16 to 24 when it also
 * runs streams of its own, e.g. the uploads of the next frame's images and scan (557 against 810-827 frames/s host-fed); batched callers keep
 * the default.  Returns TC2LI_ERR_INVALID for n < 1 or n > 32.  No reference counterpart.
 * It only takes effect before the process's first HIP call: once this library has called into HIP (any entry that needs the device,
 * tc2li_device_count included) it returns TC2LI_ERR_INVALID instead of silently doing nothing.  It sets an environment variable (setenv):
 * call it before the process starts other threads. */
int tc2li_set_hardware_queues(int n);
/* CPUs this process may really keep busy (a launcher passes min(affinity, cgroup quota) / ranks on the node): the library sizes its worker
 * pools from it -- TC2LI_HOST_THREADS_PER_CPU (default 8: measured on a 16-CPU grant) threads per CPU in all, of
 * which the extractor pool takes a quarter, the tracking pool, the LiDAR pool and every lock-step BA group an eighth after the caller's own
 * stage threads; caps 32 / 16 / 16 / 16, the sizes the pools were tuned at on a one-GPU box.  Default: the environment variable
 * TC2LI_HOST_THREAD_BUDGET, else the cores the process may run on (sched_getaffinity).  Returns
 * TC2LI_ERR_INVALID for threads < 1 or when a pool exists already (call it first, or after tc2li_shutdown).  No reference counterpart (the
 * reference's four threads are fixed, SF/src/System.cc:184-224). */
int tc2li_set_host_thread_budget(int threads);
/* counts[0] = the budget in force, [1] extractor pool, [2] tracking pool, [3] LiDAR pool, [4] threads per lock-step BA group,
 * [5] largest number of lock-step groups; capacity >= 6.  Returns 6. */
int tc2li_host_threads(int32_t* counts, int capacity);
/* Orderly end (or pause) of the library's own threads: joins every worker pool -- each worker's thread-local work spaces (device and pinned
 * buffers, streams) are released by its exit -- releases the process-wide work spaces (lock-step BA contexts, mapping work spaces) and
 * synchronises the device, all while the HIP runtime is alive.  The caller guarantees that no other thread is inside the library; its own
 * threads that called the library should have ended (their thread-local work spaces go with them).  Handles stay valid and every entry
 * keeps working afterwards (pools and work spaces are made again on demand).  Call it before main() returns: a process that leaves with
 * library threads alive runs their teardown concurrently with the HIP runtime's (the reference's System::Shutdown, SF/src/System.cc:325-377,
 * joins its threads for the same reason). */
int tc2li_shutdown(void);

/* ------------------------------------------------------------------------------------------------
 * ORB extractor -- replaces TC2LI_SLAM::ORBextractor (SF/include/ORBextractor.h:46-121,
 * SF/src/ORBextractor.cc:383-443 ctor, :1060-1141 operator()).  One handle per extractor object; the
 * reference runs the left and right extractor concurrently from two threads (SF/src/Frame.cc:139-142),
 * so handles are independent and re-entrant per handle.
 * ---------------------------------------------------------------------------------------------- */

/* Subset of cv::KeyPoint the reference reads (pt, size, angle, response, octave). */
typedef struct tc2li_keypoint {
    float x, y;      /* level-0 pixel coordinates (SF/src/ORBextractor.cc:1122-1124) */
    float size;      /* 31 * scale[octave], truncated (:851,:861) */
    float angle;     /* degrees, cv::fastAtan2 of the intensity centroid (:50-77) */
    float response;  /* FAST score */
    int32_t octave;
} tc2li_keypoint;

/* ORBextractor ctor arguments (SF/src/ORBextractor.cc:383-384; values from config/.../KITTI00-02.yaml:60-73). */
typedef struct tc2li_orb_params {
    int32_t nfeatures;
    float scale_factor;
    int32_t nlevels;
    int32_t ini_th_fast;
    int32_t min_th_fast;
} tc2li_orb_params;

typedef struct tc2li_orb tc2li_orb;

/* Creates an extractor able to process up to `max_images` images of at most max_width x max_height per call.
 * The FAST thresholds are differences of 8-bit pixels: 0 <= ini_th_fast, min_th_fast <= 255, anything else is TC2LI_ERR_INVALID. */
int tc2li_orb_create(const tc2li_orb_params* params, int max_width, int max_height, int max_images, tc2li_orb** out);
void tc2li_orb_destroy(tc2li_orb* orb);

/* ORBextractor::operator()(image, mask, keypoints, descriptors, vLappingArea)  (SF/src/ORBextractor.cc:1060).
 * One host image in; keypoints and N x 32 descriptor bytes out in the reference's order (level-major, mono
 * indices ascending from the front, lapping-area keys descending from the back).  *n_keypoints receives N.
 * Returns monoIndex like the reference, TC2LI_ERR_EMPTY (-1) for an empty image. */
int tc2li_orb_extract(tc2li_orb* orb, const uint8_t* image, int width, int height, int stride,
                      const int32_t lapping_area[2], tc2li_keypoint* keypoints, uint8_t* descriptors, int capacity,
                      int32_t* n_keypoints);

/* Batched form for images already resident in device memory: image i starts at dev_images + i*image_pitch_bytes,
 * rows are `stride` bytes apart.  Results go to host arrays laid out [n_images][capacity].  mono_index may be NULL.
 * The device images must stay valid until the handle's pyramids are no longer needed (level 0 is read in place). */
int tc2li_orb_extract_batch(tc2li_orb* orb, const uint8_t* dev_images, int n_images, int width, int height, int stride,
                            size_t image_pitch_bytes, const int32_t lapping_area[2], tc2li_keypoint* keypoints,
                            uint8_t* descriptors, int capacity, int32_t* n_keypoints, int32_t* mono_index, void* stream);

/* Host-only: the per-pixel forms of the FAST kernel (csrc/fast_forms.hpp, the source k_fast_cells runs), exposed so that their exactness
 * can be checked without a GPU.  Item i is a centre v[i] and its 16 circle pixels p[16 i .. 16 i + 15] (cv::FAST's order); th in 0 .. 255.
 * pretest[i]: the compass pre-test (items go through it four at a time, item i in byte i & 3); mask_bright / mask_dark[i]: bit j = circle
 * pixel j is brighter than v + th / darker than v - th; polarity[i]: bit 0 a darker arc of nine, bit 1 a brighter one; score_dark /
 * score_bright[i]: the largest arc contrast of either sign (a corner at th <=> the larger one exceeds th).  Outputs may be NULL. */
int tc2li_host_fast_forms(const uint8_t* v, const uint8_t* p, int n, int th, uint8_t* pretest, uint16_t* mask_bright, uint16_t* mask_dark,
                          uint8_t* polarity, int16_t* score_dark, int16_t* score_bright);

/* Accessors the reference reads off the extractor: GetLevels/GetScaleFactors/... (SF/include/ORBextractor.h:70-90)
 * and mvImagePyramid (:92; used by Frame::ComputeStereoMatches, SF/src/Frame.cc:848,938,953). */
int tc2li_orb_levels(const tc2li_orb* orb);
int tc2li_orb_scale_factors(const tc2li_orb* orb, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2);
int tc2li_orb_features_per_level(const tc2li_orb* orb, int32_t* per_level);
int tc2li_orb_level_size(const tc2li_orb* orb, int level, int* width, int* height);
/* Copies pyramid level `level` of image `image_index` of the last call to host, tightly packed width*height. */
int tc2li_orb_download_level(tc2li_orb* orb, int image_index, int level, uint8_t* dst);
/* Same for the 7x7 Gaussian-blurred level the descriptors were sampled from (SF/src/ORBextractor.cc:1105-1106). */
int tc2li_orb_download_blurred(tc2li_orb* orb, int image_index, int level, uint8_t* dst);
/* FAST candidates of the last call before the quadtree (diagnostic; x, y in level pixels, response): returns count. */
int tc2li_orb_download_candidates(tc2li_orb* orb, int image_index, int level, float* xyr, int capacity);

/* Times of the last batch call in milliseconds.  Device stages are measured with HIP events on the stream each
 * kernel is launched on: [0] pyramid (nlevels-1 resize launches), [1] FAST cells kernel, [2] candidate compaction
 * kernel, [3] blur (nlevels launches), [4] orientation+descriptor kernel, [5] keypoint distribution (quadtree + gather kernels);
 * host wall clock: [6] call entry until everything is queued, [7] whole call.
 * With profiling enabled every kernel is issued on the caller's stream (no overlap of blur with FAST), so that
 * [0]..[4] are clean per-stage durations. */
int tc2li_orb_set_profiling(tc2li_orb* orb, int enabled);
int tc2li_orb_last_timings(const tc2li_orb* orb, float ms[8]);
/* A batch call is queued in chunks of images (the blur of one chunk runs on a second stream beside the keypoint distribution of the
 * chunk before): every device stage is launched once per chunk, and [0]..[5] above are the sums over the chunks.  Returns the chunk
 * count of the last call. */
int tc2li_orb_last_chunks(const tc2li_orb* orb);
/* The projection searches on the features of the last tc2li_orb_extract_batch call (tc2li_track_motion_model_batch and its retry pass,
 * tc2li_track_local_map_batch, tc2li_search_local_points_batch, the refinement ladder of relocalisation) share one feature grid per left
 * image, as Frame's constructor builds mGrid once: the first search after an extraction builds the grids of all frames, on its stream,
 * and an extraction drops them.  Returns how many such builds the handle has done.  TC2LI_MATCH_GRID_CACHE=0 (read per call) makes every
 * search build its own grids and leaves the count alone. */
int tc2li_orb_match_grid_builds(tc2li_orb* orb);

/* ------------------------------------------------------------------------------------------------
 * Stereo matching -- replaces Frame::ComputeStereoMatches (SF/src/Frame.cc:841-1011; called from the stereo
 * Frame constructor, :160).  bf = mbf, b = mb (= mbf / fx, :197).  Outputs are mvuRight / mvDepth: -1 where a left
 * keypoint has no accepted match.  best_sad (may be NULL) receives the SAD of the sub-pixel stage before the
 * final 1.5*1.4*median cut (-1 = none).
 * ---------------------------------------------------------------------------------------------- */

/* Single frame, reference-style: the two extractor handles hold the pyramids of the left / right image of their
 * last tc2li_orb_extract call (mvImagePyramid), keypoints and descriptors come back from the caller. */
int tc2li_stereo_match(tc2li_orb* left, tc2li_orb* right, const tc2li_keypoint* keys_left, const uint8_t* desc_left,
                       int n_left, const tc2li_keypoint* keys_right, const uint8_t* desc_right, int n_right, float bf, float b,
                       float* u_right, float* depth, int32_t* best_sad);

/* Batched: frame f = images 2f (left) and 2f+1 (right) of the handle's last tc2li_orb_extract_batch call (lapping
 * area {0,0}); features are taken from device memory where that call left them.  Outputs are [n_frames][capacity]. */
int tc2li_stereo_match_batch(tc2li_orb* orb, int n_frames, float bf, float b, float* u_right, float* depth,
                             int32_t* best_sad, int capacity, void* stream);

/* ------------------------------------------------------------------------------------------------
 * LiDAR front end, camera-LiDAR branch -- replaces the internals of
 *   Preprocess::process / velodyne_handler      SF/include/lidar_front_end/preprocess.cpp:63-167 (both branches: feature_enabled
 *                                                through tc2li_lidar_set_preprocess_features, give_feature :169-623)
 *   pcl::VoxelGrid<PointXYZINormal>::filter      call sites LidarFrontEnd.cpp:712-714, 913-915
 *   ikdtree.Build / Add_Points / Nearest_Search  SF/include/ikd-Tree/ikd_Tree.cpp:409-461 (a hash grid here, same 5-NN)
 *   feature_extraction / EstiPlane               LidarFrontEnd.cpp:964-1073, with pointBodyToWorld :130-139
 * Point layouts are PCL's: velodyne_ros::Point (32 B, preprocess.h:62-70) and pcl::PointXYZINormal (48 B).
 * ---------------------------------------------------------------------------------------------- */
typedef struct tc2li_velodyne_point {
    float x, y, z, pad0;
    float intensity, time;
    uint16_t ring, pad1;
    float pad2;
} tc2li_velodyne_point;

typedef struct tc2li_point { /* pcl::PointXYZINormal */
    float x, y, z, pad0;
    float normal_x, normal_y, normal_z, pad1;
    float intensity, curvature, pad2, pad3;
} tc2li_point;

/* The parts of state_ikfom that pointBodyToWorld reads (LidarFrontEnd.cpp:130-139); matrices row-major. */
typedef struct tc2li_lidar_state {
    double rot[9], pos[3], offset_R_L_I[9], offset_T_L_I[3];
} tc2li_lidar_state;

typedef struct tc2li_lidar tc2li_lidar;         /* stage workspace for up to max_scans scans per call */
typedef struct tc2li_lidar_map tc2li_lidar_map; /* the incremental map (the reference's global `ikdtree`) */

int tc2li_lidar_create(int max_points_per_scan, int max_scans, tc2li_lidar** out);
void tc2li_lidar_destroy(tc2li_lidar* lidar);

/* Preprocess::process for a Velodyne cloud with feature_enabled = false: keeps point i when i % point_filter_num == 0
 * and |p|^2 > blind^2; curvature = time * time_unit_scale (ms).  Returns the number of points written.  With the handle's
 * tc2li_lidar_set_preprocess_features switch on: the feature branch instead (see there). */
int tc2li_lidar_preprocess(tc2li_lidar* lidar, const tc2li_velodyne_point* raw, int n, int point_filter_num, double blind,
                           float time_unit_scale, tc2li_point* out, int capacity);

/* Preprocess::feature_enabled (LidarFrontEnd.cpp:639, :823): f != NULL switches every preprocess of the handle (tc2li_lidar_preprocess,
 * tc2li_lidar_frontend_batch, tc2li_lidar_inertial_prepare_batch, tc2li_lidar_inertial_frontend_batch) to velodyne_handler's feature
 * branch (preprocess.cpp:100-143): points whose ring >= n_lines are dropped, the others bucketed into their ring's line in input order,
 * give_feature (:169-482) labels every line, and the output is pl_surf -- surface points, every point_filter_num-th of a run of them,
 * an unfinished group averaged, line by line.  blind is compared with the 2-D range sqrt(x^2 + y^2) there.  f == NULL: off (the default).
 * point_filter_num, blind and time_unit_scale keep coming from the preprocess calls. */
typedef struct tc2li_preprocess_features {
    int32_t n_lines;   /* N_SCANS ("preprocess/scan_line"), 1..128 */
    int32_t reserved;  /* 0 */
    double  dis_b;     /* Preprocess::disB: the ctor assigns disA twice (preprocess.cpp:40-41) and disB never; 0.0 = zeroed memory */
} tc2li_preprocess_features;
int tc2li_lidar_set_preprocess_features(tc2li_lidar* lidar, const tc2li_preprocess_features* f);
/* pl_corn of scan slot `scan` of the last preprocess with the switch on: the points labelled Edge_Jump or Edge_Plane, line by line.
 * Returns the number of points written. */
int tc2li_lidar_corner_points(tc2li_lidar* lidar, int scan, tc2li_point* out, int capacity);
/* Tests / diagnostics: the Feature label (preprocess.h:40: Nor 0, Poss_Plane 1, Real_Plane 2, Edge_Jump 3, Edge_Plane 4, Wire 5) of every
 * bucketed point of scan slot `scan` of the last preprocess with the switch on, in line order, and the n_lines + 1 line offsets.  A line
 * of fewer than 2 points is labelled Nor.  Returns the number of labels written. */
int tc2li_lidar_point_labels(tc2li_lidar* lidar, int scan, uint8_t* ftype, int32_t* ring_offsets, int capacity);

/* downSizeFilterSurf.setInputCloud(in); downSizeFilterSurf.filter(out) with leaf size `leaf` on all three axes:
 * one centroid (of every field) per occupied voxel, in ascending voxel-index order. */
int tc2li_lidar_voxel_filter(tc2li_lidar* lidar, const tc2li_point* in, int n, float leaf, tc2li_point* out, int capacity);

/* LiDAR map handle -- thread contract.  In the reference the global `ikdtree` is touched from two threads: the LiDAR thread
 * (feature_extraction / h_share_model, LidarFrontEnd.cpp:942,749) and the tracking thread (UpdateMap -> map_incremental,
 * Tracking.cc:1602-1603, under `finishMutex`).  A tc2li_lidar_map may be used from any number of host threads: every entry
 * point that reads or changes a map (build / add / size / download / feature_extraction / frontend_batch / eskf_update /
 * map_incremental / delete_boxes) holds the handle's internal lock from its first access until its device work on the map
 * has completed (each of them synchronises its stream before it returns), so calls on one handle serialise inside the
 * library; a batch call locks the distinct maps of its batch in address order.  What the lock cannot give is the reference's
 * sequencing: tc2li_lidar_map_incremental replays the neighbours found by the handle's LAST feature extraction against the
 * same map, so the caller must not let another thread change that map in between (the reference's finishMutex does this).
 * A tc2li_lidar workspace itself is NOT shareable between threads (one per calling thread, like the ORB extractor handle).
 * tc2li_lidar_map_destroy must not race with any other call on the handle.
 * Entry points without a `stream` argument run on a private non-blocking stream of the calling thread (never the NULL stream). */
int tc2li_lidar_map_create(tc2li_lidar_map** out);
void tc2li_lidar_map_destroy(tc2li_lidar_map* map);
/* ikdtree.Build(points) (LidarFrontEnd.cpp:918-931): replaces the map content.  Returns the map size. */
int tc2li_lidar_map_build(tc2li_lidar_map* map, const tc2li_point* world_points, int n);
/* ikdtree.Add_Points(points, false): appends without down-sampling.  Returns the map size. */
int tc2li_lidar_map_add(tc2li_lidar_map* map, const tc2li_point* world_points, int n);
int tc2li_lidar_map_size(const tc2li_lidar_map* map);
/* Measurement / test hooks of the map's spatial index (no reference counterpart: ikd-Tree keeps its own counters, ikd_Tree.h:117-123).
 * tc2li_lidar_map_stats: out[0] points, [1] places of the grid (entries + the rows' room), [2] grid builds so far, [3] in-place grid updates
 * so far (map_incremental calls that merged their points into the existing rows, KD_TREE::Add_Points' own way, ikd_Tree.cpp:478-584),
 * [4] tombstones (upper bound), [5] cells; capacity >= 6, returns 6.
 * tc2li_lidar_map_grid_download: walks the grid on the host, checks it (every live entry stands in the cell its coordinates name and names
 * an existing point, rows stay inside their room, unused room holds no live entry: TC2LI_ERR_INVALID with the finding otherwise) and
 * returns the number of live entries, the first `capacity` of them as (cell, point index) in grid order. */
int tc2li_lidar_map_stats(const tc2li_lidar_map* map, int32_t* out, int capacity);
int tc2li_lidar_map_grid_download(const tc2li_lidar_map* map, int32_t* cells, int32_t* indices, int capacity);

/* feature_extraction() (LidarFrontEnd.cpp:999-1073) for one down-sampled scan.  Per input point i (arrays of n, any
 * may be NULL): feats_down_world[i], point_selected[i], normvec[i] (plane normal, intensity = pd2), the up-to-5
 * Nearest_Points[i] ([n][5], ascending distance) with their squared distances and count.  laser_cloud_ori /
 * corr_normvect receive the compacted selection; the return value is effct_feat_num. */
int tc2li_lidar_feature_extraction(tc2li_lidar* lidar, tc2li_lidar_map* map, const tc2li_point* feats_down_body, int n,
                                   const tc2li_lidar_state* state, tc2li_point* feats_down_world, uint8_t* point_selected,
                                   tc2li_point* normvec, tc2li_point* nearest_points, float* nearest_sqdist, int32_t* n_nearest,
                                   tc2li_point* laser_cloud_ori, tc2li_point* corr_normvect, int capacity);

/* Whole front end for a batch of raw scans resident in device memory (scan s = dev_raw[raw_offsets[s] .. raw_offsets[s+1])):
 * preprocess -> voxel filter -> feature extraction against maps[s] with states[s]; stages chain on the device.
 * Per-scan counts come back in the three int arrays; the compacted selections in [n_scans][capacity] host arrays
 * (either may be NULL). */
int tc2li_lidar_frontend_batch(tc2li_lidar* lidar, int n_scans, const tc2li_velodyne_point* dev_raw, const int32_t* raw_offsets,
                               int point_filter_num, double blind, float time_unit_scale, float leaf,
                               tc2li_lidar_map* const* maps, const tc2li_lidar_state* states, int32_t* n_preprocessed,
                               int32_t* n_downsampled, int32_t* n_selected, tc2li_point* laser_cloud_ori,
                               tc2li_point* corr_normvect, int capacity, void* stream);
/* ---- persistent map maintenance on the device (the map never returns to the host) ----
 * map_incremental (SF/include/lidar_front_end/LidarFrontEnd.cpp:387-435) for scan slot `scan` of the handle's last
 * feature extraction (tc2li_lidar_feature_extraction: slot 0; tc2li_lidar_frontend_batch: the scan's index) against the
 * SAME map, unchanged since: world coordinates at `state` (UpdateLidarPose may have moved it), the insertion rule
 * (one point per filter_size_map_min voxel, the one nearest the voxel centre), then
 * ikdtree.Add_Points(PointToAdd, true) / Add_Points(PointNoNeedDownsample, false) (ikd_Tree.cpp:478-584).
 * ekf_inited = flg_EKF_inited.  Returns the new map size; the list sizes go to n_to_add / n_no_need (may be NULL). */
int tc2li_lidar_map_incremental(tc2li_lidar* lidar, int scan, tc2li_lidar_map* map, const tc2li_lidar_state* state, int ekf_inited,
                                double filter_size_map_min, int32_t* n_to_add, int32_t* n_no_need, void* stream);
/* The same for n (scan slot, map) pairs of the handle's last tc2li_lidar_frontend_batch in one call -- what the tracking threads of n
 * sequences do at SyncWithLidar (Tracking.cc:1602-1603), with one kernel launch per phase for all maps instead of a dozen per map.
 * scans[i] = scan slot, maps[i] = its map (every map at most once), states[i] = the state map_incremental reads.  The list sizes and
 * the new map sizes go to the three int arrays (any may be NULL).  Returns n.  On TC2LI_ERR_CAPACITY no map has been changed. */
int tc2li_lidar_map_incremental_batch(tc2li_lidar* lidar, int n, const int32_t* scans, tc2li_lidar_map* const* maps,
                                      const tc2li_lidar_state* states, int ekf_inited, double filter_size_map_min, int32_t* n_to_add,
                                      int32_t* n_no_need, int32_t* map_sizes, void* stream);
/* ---- pose plumbing between the camera thread and the LiDAR front end ----
 * Poses are Sophus::SE3f as qx qy qz qw tx ty tz; the arithmetic is float, in Sophus' / Eigen's order.
 * tc2li_lidar_update_pose = UpdateLidarPose (SF/include/lidar_front_end/LidarFrontEnd.cpp:786-800): Twc = Tcw_last^-1 * exp(t * log(velocity^-1)),
 * the LiDAR pose in the front end's world frame (Rw2_w1 * Twc * Tcl) into state->rot / state->pos, pos_lid = pos + rot * offset_T_L_I (may be NULL).
 * tc2li_se3_interpolate = InterpolateSE3 (SF/src/Tracking.cc:1552-1563): quaternion slerp + linear translation.
 * tc2li_lidar_sync_transform = the transform Tracking::SyncWithLidar applies to a scan's feature cloud (:1600-1626):
 *   Tlc * Tcw_frame * InterpolateSE3(Tcw_last^-1, Tcw_cur^-1, ratio) * Tcl, Tcw_frame = the frame the scan pairs with (current or last).
 * tc2li_lidar_keyframe_transform = the one of Tracking::BuildLidarFeat4KeyFrame (:1537-1547): Tlc * Tcw_cur * (rel * Tcw_refkf)^-1 * Tcl.
 * tc2li_transform_point_cloud = LidarFrontEndTools::transformPointCloud (SF/src/LidarTypes.cc:42-65) on host arrays; returns n.
 * tc2li_lidar_transform_features_batch: the same for the selected feature clouds (laserCloudOri = mCurrFeatPoints) of scan slots `scans` of the
 * handle's last tc2li_lidar_frontend_batch, read on the device where the front end left them, one launch for all scans:
 * out [n][capacity] (host), n_points[i] = points written for scans[i] (may be NULL). */
int tc2li_lidar_update_pose(const float Tcw_last7[7], const float velocity7[7], double time_from_last_frame, const float Tcl7[7],
                            tc2li_lidar_state* state, double pos_lid[3]);
int tc2li_se3_interpolate(const float a7[7], const float b7[7], float t, float out7[7]);
int tc2li_lidar_sync_transform(const float Tcw_frame7[7], const float Tcw_last7[7], const float Tcw_cur7[7], float ratio, const float Tlc7[7],
                               const float Tcl7[7], float out7[7]);
int tc2li_lidar_keyframe_transform(const float Tcw_cur7[7], const float rel7[7], const float Tcw_refkf7[7], const float Tlc7[7],
                                   const float Tcl7[7], float out7[7]);
int tc2li_transform_point_cloud(const tc2li_point* in, int n, const float T7[7], tc2li_point* out, void* stream);
int tc2li_lidar_transform_features_batch(tc2li_lidar* lidar, int n, const int32_t* scans, const float* T7, tc2li_point* out, int capacity,
                                         int32_t* n_points, void* stream);
/* ikdtree.Delete_Point_Boxes (ikd_Tree.cpp:643): removes the points inside the boxes [min, max) given as
 * min x y z, max x y z per box; returns how many were removed. */
int tc2li_lidar_map_delete_boxes(tc2li_lidar_map* map, const float* boxes6, int n_boxes, void* stream);
/* The same for n_maps different maps in one go (one launch per phase; the per-sequence lasermap_fov_segment calls of a batch of
 * sequences): map i gets the boxes box_offsets[i] .. box_offsets[i+1] of boxes6 (box_offsets[0] = 0).  n_removed [n_maps] (may be
 * NULL) receives the per-map counts; returns their sum. */
int tc2li_lidar_map_delete_boxes_batch(int n_maps, tc2li_lidar_map* const* maps, const float* boxes6, const int32_t* box_offsets,
                                       int32_t* n_removed, void* stream);
/* Copies the map points to the host (diagnostics / tests); returns the map size. */
int tc2li_lidar_map_download(const tc2li_lidar_map* map, tc2li_point* out, int capacity);
/* lasermap_fov_segment (LidarFrontEnd.cpp:183-231), host logic: keeps the local-map cube around the sensor and returns
 * the number of boxes (<= 3, written to boxes6) whose points must be deleted. */
typedef struct tc2li_local_map_box { float vertex_min[3], vertex_max[3]; int32_t initialized; } tc2li_local_map_box;
int tc2li_lidar_fov_segment(tc2li_local_map_box* local_map, const double pos_lid[3], double cube_len, double det_range, float boxes6[18]);
/* The same for n sensors in one call (the per-sequence calls of a batch driver): local_maps [n], pos_lid3 [n][3]; boxes6 [n][18] and n_boxes [n]
 * receive every sequence's boxes and their number; returns the total. */
int tc2li_lidar_fov_segment_batch(tc2li_local_map_box* local_maps, const double* pos_lid3, int n, double cube_len, double det_range, float* boxes6,
                                  int32_t* n_boxes);

/* ---- camera-LiDAR-inertial branch: motion compensation of the scan (ImuProcess::UndistortPcl,
 * SF/include/lidar_front_end/IMU_Processing.cpp:160-277) ---- */
typedef struct tc2li_imu_pose6d {   /* Pose6D saved at every IMU sample during the forward propagation */
    double offset_time;             /* seconds since the scan start */
    double acc[3], gyr[3];          /* world-frame acceleration / bias-free angular velocity of the interval ending here */
    double vel[3], pos[3], rot[9];  /* IMU state at the sample */
} tc2li_imu_pose6d;
typedef struct tc2li_imu_state {    /* the parts of state_ikfom the propagation reads / writes (rotations row-major) */
    double pos[3], rot[9], vel[3], bg[3], ba[3], grav[3], offset_R_L_I[9], offset_T_L_I[3];
} tc2li_imu_state;
typedef struct tc2li_imu_meas { double t, acc[3], gyr[3]; } tc2li_imu_meas;   /* sensor_msgs::Imu fields used */

/* Forward propagation of UndistortPcl (:176-233), state part of esekf::predict (covariance: see the ESKF entry):
 * v_imu = last scan's tail sample followed by this scan's samples; acc_scale = G_m_s2 / mean_acc.norm();
 * acc_s_last / angvel_last from the previous call.  Writes the poses (capacity >= n_imu) and the scan-end state into
 * *state; returns the number of poses.  Host-only. */
int tc2li_lidar_imu_propagate(tc2li_imu_state* state, const tc2li_imu_meas* v_imu, int n_imu, double pcl_beg_time,
                              double pcl_end_time, double last_lidar_end_time, double acc_scale, double acc_s_last[3],
                              double angvel_last[3], tc2li_imu_pose6d* poses, int capacity);

/* The same forward propagation with the covariance (esekf::predict, SF/include/IKFoM_toolkit/esekfom/esekfom.hpp:281-392 with
 * get_f / df_dx / df_dw of SF/src/use-ikfom.cpp:45-91): P is the 23 x 23 row-major error-state covariance in the order pos, rot,
 * offset_R_L_I, offset_T_L_I, vel, bg, ba, grav (2); cov12 = cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc, the diagonal of Q
 * (IMU_Processing.cpp:215-218).  Host-only: 23 x 23 products per IMU sample. */
int tc2li_lidar_imu_propagate_cov(tc2li_imu_state* state, double* P, const double cov12[12], const tc2li_imu_meas* v_imu, int n_imu,
                                  double pcl_beg_time, double pcl_end_time, double last_lidar_end_time, double acc_scale,
                                  double acc_s_last[3], double angvel_last[3], tc2li_imu_pose6d* poses, int capacity);
/* One esekf::predict step with a full 12 x 12 process noise Q (ng, na, nbg, nba). */
int tc2li_eskf_predict(tc2li_imu_state* state, double* P, const double* Q, const double acc[3], const double gyr[3], double dt);

/* esekf::update_iterated_dyn_share_modified (esekfom.hpp:1621-1932) with h_share_model (LidarFrontEnd.cpp:485-602) as the
 * measurement model, as called at LidarFrontEnd.cpp:749: R = LASER_POINT_COV, maximum_iter = NUM_MAX_ITERATIONS, limit23 = epsi.
 * Every iteration evaluates the point-to-plane residuals of feats_down_body against `map` at the current state (the neighbour
 * search only when the previous iteration converged, as the reference does), reduces the 12 active columns of H to H^T H and
 * H^T h on the device, and solves the 23-dof update on the host.  State and P (23 x 23) are updated in place.  Afterwards the
 * handle holds Nearest_Points / the selection of the last evaluation for tc2li_lidar_map_incremental.  Returns effct_feat_num
 * of the last evaluation. */
typedef struct tc2li_eskf_stats {
    int32_t calls;            /* h_share_model evaluations */
    int32_t effct_feat_num;   /* selected points of the last one */
    int32_t searches;         /* evaluations that ran the neighbour search */
    int32_t converged;        /* iterations whose step stayed below limit23 */
    int32_t finished;         /* the covariance update ran (:1823-1928) */
    int32_t pad_;
    double res_mean_last;
} tc2li_eskf_stats;
int tc2li_lidar_eskf_update(tc2li_lidar* lidar, tc2li_lidar_map* map, const tc2li_point* feats_down_body, int n, tc2li_imu_state* state,
                            double* P, double R, int maximum_iter, const double* limit23, int extrinsic_est_en, tc2li_eskf_stats* stats);

/* The point part (:170-172, 236-276): sorts the scan by time offset (curvature, ms) in the order std::sort(time_list)
 * produces and moves every point into the scan-end frame; in place on the host array.  end_state = imu_state after the
 * last predict (rot, pos, offset_R_L_I, offset_T_L_I are read). */
int tc2li_lidar_undistort(tc2li_lidar* lidar, tc2li_point* points, int n, const tc2li_imu_pose6d* imu_poses, int n_poses,
                          const tc2li_lidar_state* end_state);

/* ---- the LiDAR thread of the camera-LiDAR-inertial configuration for a batch of sequences ----
 * LidarInertialProcess (SF/include/lidar_front_end/LidarFrontEnd.cpp:615-785) for n_scans scans of n_scans sequences in one call:
 * Preprocess::process of the raw scans (resident in device memory like tc2li_lidar_frontend_batch's), ImuProcess::Process = forward
 * propagation with the covariance on the host (tc2li_lidar_imu_propagate_cov) + UndistortPcl on the device -- the time sort included: the
 * permutation std::sort leaves is replayed on the device --, downSizeFilterSurf.filter, and kf.update_iterated_dyn_share_modified with
 * h_share_model (:749) for all scans in lock step: per iteration one launch per phase over the scans still iterating, then every
 * scan's 23-dof algebra on host threads.  Every scan's result is the one of the one-scan entry points called in that order
 * (tc2li_lidar_preprocess, tc2li_lidar_imu_propagate_cov, tc2li_lidar_undistort, tc2li_lidar_voxel_filter, tc2li_lidar_eskf_update).
 * Afterwards the handle holds every scan's down-sampled points and Nearest_Points for tc2li_lidar_map_incremental_batch (scan slot s). */
typedef struct tc2li_lidar_inertial_scan {
    const tc2li_imu_meas* imu;          /* v_imu: the last scan's tail sample followed by this scan's samples */
    int32_t n_imu, pad_;
    double pcl_beg_time, pcl_end_time, last_lidar_end_time, acc_scale;
    double acc_s_last[3], angvel_last[3];   /* in / out, as tc2li_lidar_imu_propagate */
    tc2li_imu_state state;              /* in: the filter state at the last scan end; out: after the iterated update */
    double* P;                          /* [23 * 23] in / out */
    tc2li_eskf_stats stats;             /* out */
    int32_t n_preprocessed, n_downsampled;  /* out */
} tc2li_lidar_inertial_scan;
int tc2li_lidar_inertial_frontend_batch(tc2li_lidar* lidar, int n_scans, const tc2li_velodyne_point* dev_raw, const int32_t* raw_offsets,
                                        int point_filter_num, double blind, float time_unit_scale, float leaf, tc2li_lidar_map* const* maps,
                                        tc2li_lidar_inertial_scan* scans, const double cov12[12], double R, int maximum_iter,
                                        const double* limit23, int extrinsic_est_en, void* stream);
/* The part of LidarInertialProcess that depends on the scans alone, as a call of its own: Preprocess::process of every raw scan (the reference
 * runs it in the scan callback, LidarFrontEnd.cpp:253, ahead of the thread that consumes lidar_buffer) and the order UndistortPcl's
 * std::sort(time_list) will leave the points in.  The handle then holds n_scans prepared scans; the next
 * tc2li_lidar_inertial_frontend_batch on it with dev_raw = NULL (raw_offsets, point_filter_num, blind, time_unit_scale are not read then) and
 * the same n_scans consumes them and gives exactly the results of the one-call form.  Two handles let a caller prepare the scans of step k + 1
 * (own stream, own thread) while step k's iterated update runs.  Returns n_scans. */
int tc2li_lidar_inertial_prepare_batch(tc2li_lidar* lidar, int n_scans, const tc2li_velodyne_point* dev_raw, const int32_t* raw_offsets,
                                       int point_filter_num, double blind, float time_unit_scale, void* stream);
/* The time sort of UndistortPcl alone (tests / diagnostics): perm[i] = index of the point std::sort(points, time_list) leaves at place i,
 * computed by the device kernel of the batch entry (one scan; depth_limit < 0: std::sort's own 2 floor(log2 n)).  Returns 1 when the
 * recursion reached the depth limit (perm is then unspecified: the batch entry sorts such a scan on the host), else 0. */
int tc2li_device_time_sort(tc2li_lidar* lidar, const tc2li_point* points, int n, int depth_limit, int32_t* perm);

/* Device time of the stages of the last tc2li_lidar_frontend_batch call, from HIP events on its stream: ms[0]
 * preprocess, [1] voxel hashing/sorting, [2] voxel centroids, [3] 5-NN + plane fit, [4] selection, [5] total, [6] / [7] the two
 * kernels of stage [3] (k_knn_plane, k_knn_hard). */
int tc2li_lidar_last_timings(tc2li_lidar* lidar, float ms[8]);

/* ------------------------------------------------------------------------------------------------
 * Projection-guided matching of the tracking thread -- replaces the two overloads of ORBmatcher::SearchByProjection
 * that Tracking uses: (Frame&, const Frame& LastFrame, th, bMono) SF/src/ORBmatcher.cc:1685 (TrackWithMotionModel,
 * Tracking.cc:2771,2780) and (Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints) :52 (SearchLocalPoints,
 * Tracking.cc:3282).  Map-point pointers stay on the host: each source point becomes one query.
 * ---------------------------------------------------------------------------------------------- */
typedef struct tc2li_proj_query {
    float u, v;                 /* projection in the current frame */
    float radius;               /* window half size handed to Frame::GetFeaturesInArea */
    float u_right;              /* predicted right coordinate (stereo consistency check) */
    int32_t min_level, max_level; /* GetFeaturesInArea level arguments */
    float angle;                /* keypoint angle in the source frame (rotation histogram) */
    int16_t valid;              /* 0: the source point produces no search */
    int16_t has_observations;   /* pMP->Observations() > 0: a match blocks the keypoint for later points */
    uint8_t descriptor[32];     /* pMP->GetDescriptor() */
} tc2li_proj_query;

typedef struct tc2li_frame_view {  /* the parts of the current Frame the matcher reads */
    const tc2li_keypoint* keys;    /* mvKeysUn */
    const uint8_t* descriptors;    /* mDescriptors, n x 32 */
    const float* u_right;          /* mvuRight */
    const uint8_t* occupied;       /* mvpMapPoints[i] && Observations() > 0 before the call (may be NULL) */
    int32_t n;
    float min_x, max_x, min_y, max_y; /* mnMinX .. mnMaxY */
} tc2li_frame_view;

typedef struct tc2li_map_point {  /* what Frame::isInFrustum / PredictScale read off a MapPoint */
    float pos[3], normal[3];
    float min_distance, max_distance; /* Get{Min,Max}DistanceInvariance() */
    float max_distance_raw;           /* mfMaxDistance */
    uint8_t descriptor[32];
} tc2li_map_point;

/* The matching loops.  mode 0: best Hamming distance <= TH_HIGH (last-frame overload); mode 1: best / second best with
 * nn_ratio when both lie on one level (local-map overload).  check_orientation applies the 30-bin rotation histogram.
 * match_of_query[q] = matched keypoint or -1; query_of_keypoint[i] (may be NULL) = the query now held by keypoint i.
 * Returns nmatches like the reference.
 * The histogram filter works on KEYPOINTS, as the reference's does (rotHist[bin].push_back(bestIdx2), ORBmatcher.cc:1800; the loop of
 * :1882-1891 clears CurrentFrame.mvpMapPoints[keypoint] and counts down once per rejected entry).  Two queries share a keypoint when the
 * earlier one has has_observations == 0 (:1756-1758 does not skip such a keypoint); if either of the two entries falls outside the
 * three dominant bins the keypoint is cleared: query_of_keypoint[i] = -1, match_of_query = -1 for every query that pointed at it, and
 * nmatches drops by the number of rejected entries, not of queries. */
int tc2li_search_by_projection(const tc2li_frame_view* frame, const tc2li_proj_query* queries, int n_queries, int mode,
                               float nn_ratio, int check_orientation, int32_t* match_of_query, int32_t* query_of_keypoint);

/* Query construction of the last-frame overload (ORBmatcher.cc:1696-1739).  Poses are Sophus::SE3f as 7 floats
 * (qx, qy, qz, qw, tx, ty, tz); cam4 = fx, fy, cx, cy; b = mb, bf = mbf.  One query per last-frame keypoint i
 * (has_point[i] = LastFrame.mvpMapPoints[i] != NULL, outlier[i] = mvbOutlier[i], Xw = world positions).  Returns the
 * number of valid queries. */
int tc2li_project_last_frame(const float pose_cur7[7], const float pose_last7[7], const float cam4[4], float b, float bf,
                             const float* scale_factors, int n_levels, int cols, int rows, int n, const uint8_t* has_point,
                             const uint8_t* outlier, const float* Xw, const tc2li_keypoint* last_keys, const uint8_t* mp_descriptors,
                             float th, int mono, tc2li_proj_query* queries);

/* Frame::isInFrustum(pMP, viewing_cos_limit) (SF/src/Frame.cc:542-603) + MapPoint::PredictScale + the window of the
 * local-map overload (ORBmatcher.cc:62-81) for n local map points. */
int tc2li_project_local_map(const float pose7[7], const float cam4[4], float bf, const float* scale_factors, int n_levels,
                            float log_scale_factor, int cols, int rows, int n, const tc2li_map_point* points, float th,
                            int far_points, float th_far_points, float viewing_cos_limit, tc2li_proj_query* queries);

/* ------------------------------------------------------------------------------------------------
 * Optimisation back end.  Poses are Tcw as 7 doubles (qx, qy, qz, qw, tx, ty, tz) -- g2o::SE3Quat of
 * VertexSE3Expmap (Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:60-77); map points 3 doubles.
 * ---------------------------------------------------------------------------------------------- */
typedef struct tc2li_camera { double fx, fy, cx, cy, bf; } tc2li_camera;

/* One projection edge: EdgeStereoSE3ProjectXYZ[OnlyPose] when u_right >= 0, else the monocular
 * EdgeSE3ProjectXYZ[OnlyPose]; information = inv_sigma2 * I (mvInvLevelSigma2[octave]). */
typedef struct tc2li_ba_edge {
    int32_t point, pose; /* indices into the point / pose arrays of the call */
    double u, v, u_right, inv_sigma2;
} tc2li_ba_edge;

/* Optimizer::PoseOptimization(Frame*) (SF/src/Optimizer.cc:816; callers Tracking.cc:2628,2796,2858): motion-only
 * optimisation of one frame pose against its n map-point correspondences (Xw[3*edges[i].point], edges[i].pose
 * ignored), 4 rounds x optimize(10) with Huber sqrt(5.991)/sqrt(7.815) and chi2 gates 5.991/7.815.  pose7 is updated
 * (rounded through float like Frame::SetPose), outlier[i] = mvbOutlier; returns nInitialCorrespondences - nBad. */
int tc2li_pose_optimization(double pose7[7], const double* Xw, const tc2li_ba_edge* edges, int n, const tc2li_camera* cam,
                            uint8_t* outlier);
/* Many frames in one launch (one workgroup per frame): frame f owns edges/Xw/outlier [edge_offsets[f], edge_offsets[f+1]),
 * its edges' `point` index is relative to that range. */
int tc2li_pose_optimization_batch(int n_frames, double* poses7, const int32_t* edge_offsets, const double* Xw,
                                  const tc2li_ba_edge* edges, const tc2li_camera* cam, uint8_t* outlier, int32_t* n_inliers,
                                  void* stream);
/* The sizes at which the pose optimisation (every caller: the two entries above, the tracking, BoW and relocalisation batches) changes
 * kernel, and which kernel ran last (for tests): out[0] = the largest number of correspondences of a batch's largest frame at which the
 * frames are staged in LDS (beyond: every frame of the batch works in global memory), out[1] = the step in correspondences by which the
 * LDS block grows, out[2] = threads per frame, out[3] = what the most recent pose optimisation of this process launched: 0 nothing yet,
 * 1 the LDS kernel (61 bytes per correspondence), 2 the global-memory kernel, 3 the LDS kernel in its compact form (33 bytes per
 * correspondence: map points and observations held as floats; launched only when every one of them is a float's value, so the results are
 * the same bits; reported by the two entries above, which have the device check the staged values.  The tracking batches make their
 * values from floats and take the compact layout without a check; their launches report 1, "staged in LDS", in either layout).
 * TC2LI_PO_COMPACT=0, read per call, keeps the 61-byte layout everywhere.  Returns 4.  Needs no device.  No reference counterpart. */
int tc2li_pose_optimization_limits(int32_t* out, int capacity);

/* Statistics of one bundle adjustment (all optional). */
typedef struct tc2li_ba_stats {
    int32_t iterations, trials, n_free_poses, pad_;
    double initial_chi2, final_chi2, final_lambda;
} tc2li_ba_stats;

/* The optimisation of Optimizer::LocalBundleAdjustment / OptimizerWithLidar::LocalLVBundleAdjustment (visual edges;
 * SF/src/Optimizer.cc:1118, SF/src/OptimizerWithLidar.cc:60; callers LocalMapping.cc:170,173).  In: the window as the reference
 * gathers it (OptimizerWithLidar.cc:63-130), flattened -- poses in vertex-id order with their fixed flags, points, one edge
 * per observation: the arrays tc2li_ba_window_batch ("the window of the local BA" below) fills from the flat graph.  Runs
 * optimizer.optimize(iterations) with Huber sqrt(5.991) / sqrt(7.815); lambda_init <= 0 selects tau * max diagonal,
 * the inertial-map branch passes 100 (OptimizerWithLidar.cc:141-142).  stop_flag is *pbStopFlag, polled between
 * Levenberg trials like g2o's forceStopFlag.  Outputs: poses and points updated in place (double; the shim casts to
 * float, :468-484), per-edge chi2 as the optimiser left it and isDepthPositive() for the outlier rules (:402-449).
 * Returns the number of iterations performed.  Limits of the graph: every point has an edge and at most 256 edges in all.  Several edges
 * between a point and the same optimisable keyframe are added into the same Hessian blocks, as g2o does
 * (Thirdparty/g2o/g2o/core/base_binary_edge.hpp:55-137; since round 5 -- rounds 2-4 returned TC2LI_ERR_INVALID for such a pair). */
int tc2li_local_bundle_adjustment(double* poses7, const uint8_t* fixed, int n_poses, double* points3, int n_points,
                                  const tc2li_ba_edge* edges, int n_edges, const tc2li_camera* cam, int iterations,
                                  double lambda_init, const volatile uint8_t* stop_flag, double* edge_chi2,
                                  uint8_t* edge_depth_positive, tc2li_ba_stats* stats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * IMU pre-integration (camera-LiDAR-inertial configuration) -- replaces IMU::Preintegrated (SF/src/ImuTypes.cc:152-316),
 * the sample interpolation of Tracking::PreintegrateIMU (SF/src/Tracking.cc:1710-1822) and Tracking::PredictStateIMU
 * (:1825-1875).  Host-only (about ten float samples per frame); the result feeds the inertial edges of the local BA.
 * Matrices are row-major floats.
 * ---------------------------------------------------------------------------------------------- */
typedef struct tc2li_imu_sample { double t; float a[3], w[3]; } tc2li_imu_sample;              /* IMU::Point */
typedef struct tc2li_imu_bias { float bax, bay, baz, bwx, bwy, bwz; } tc2li_imu_bias;          /* IMU::Bias */
typedef struct tc2li_preintegrated {                                                           /* IMU::Preintegrated */
    float dT;
    int32_t n_measurements;
    float dR[9], dV[3], dP[3], JRg[9], JVg[9], JVa[9], JPg[9], JPa[9], avgA[3], avgW[3];
    float C[225];                  /* 15 x 15 covariance: rotation, velocity, position, gyro walk, acc walk */
    float noise[6], noise_walk[6]; /* diagonals of Nga / NgaWalk (IMU::Calib::Set, ImuTypes.cc:403-416) */
    tc2li_imu_bias bias;           /* the bias the integration was made with */
} tc2li_preintegrated;

/* Preintegrated(bias, calib): ng, na, ngw, naw as passed to IMU::Calib::Set. */
int tc2li_imu_preintegrated_init(tc2li_preintegrated* p, const tc2li_imu_bias* bias, float ng, float na, float ngw, float naw);
/* Preintegrated::IntegrateNewMeasurement */
int tc2li_imu_integrate(tc2li_preintegrated* p, const float acc[3], const float ang_vel[3], float dt);
/* The loop of Tracking::PreintegrateIMU over mvImuFromLastFrame (samples between the two frame stamps, one before and
 * one after included); returns the number of integration steps. */
int tc2li_imu_preintegrate(tc2li_preintegrated* p, const tc2li_imu_sample* samples, int n_samples, double t_prev, double t_cur);
/* The same for one frame of each of n_frames sequences (a batch of tracking threads): pre[f] is initialised at bias[f] with the calibration's
 * noise values and integrates samples[sample_offsets[f] .. sample_offsets[f + 1]) between t_prev[f] and t_cur[f].  Returns n_frames. */
int tc2li_imu_preintegrate_frames(int n_frames, tc2li_preintegrated* pre, const tc2li_imu_bias* bias, float ng, float na, float ngw, float naw,
                                  const tc2li_imu_sample* samples, const int32_t* sample_offsets, const double* t_prev, const double* t_cur);
/* GetDeltaRotation / GetDeltaVelocity / GetDeltaPosition at another bias (outputs may be NULL) */
int tc2li_imu_delta(const tc2li_preintegrated* p, const tc2li_imu_bias* bias, float dR[9], float dV[3], float dP[3]);
/* Tracking::PredictStateIMU: (Rwb1, twb1, Vwb1) of the last keyframe / frame -> the current frame's IMU state */
int tc2li_imu_predict_state(const tc2li_preintegrated* p, const tc2li_imu_bias* bias, const float Rwb1[9], const float twb1[3],
                            const float Vwb1[3], float Rwb2[9], float twb2[3], float Vwb2[3]);

/* IMU initialisation (one problem on the host: tens of keyframes, one 9-d edge per consecutive pair.  Many
 * maps at once, on the device or on the host's pool: "IMU initialisation: the inertial optimisation, batched" below).
 * tc2li_imu_init_gravity = the first estimate of LocalMapping::InitializeIMU (SF/src/LocalMapping.cc:1241-1270): keyframes in temporal
 * order (Rwb [n][9] row-major, twb [n][3], float), pre[i] = keyframe i's pre-integration from keyframe i - 1 (pre[0] ignored, NULL
 * entries skipped) -> the finite-difference velocities vel3 [n][3] and Rwg (gravity direction of the IMU world).  Returns the links used.
 * tc2li_inertial_optimization = Optimizer::InertialOptimization(pMap, Rwg, scale, bg, ba, bMono, covInertial, bFixedVel, bGauss, priorG,
 * priorA) (SF/src/Optimizer.cc:2169-2356): Levenberg-Marquardt (lambda 1e3 when prior_g != 0, `iterations` = 200 in the reference,
 * g2o's stop rules) over the keyframe velocities (in / out, double), one gyro and one accelerometer bias (in: the first keyframe's; out:
 * the estimate), the gravity direction Rwg (in / out) and, when mono, the scale (in / out); fixed_vel freezes velocities and biases.
 * The pre-integrations are evaluated at the estimated biases through their bias Jacobians (SetNewBias + GetDelta*(b)).  What the
 * reference does with the result on its objects (SetVelocity / SetNewBias / Reintegrate) stays with the caller; Map::ApplyScaledRotation
 * on the flat map is tc2li_apply_scaled_rotation_batch ("IMU initialisation: the map update" below).
 * Returns the iterations run. */
typedef struct tc2li_inertial_init_stats { int32_t iterations, trials; double initial_chi2, final_chi2, final_lambda; } tc2li_inertial_init_stats;
int tc2li_imu_init_gravity(int n_kfs, const float* Rwb9, const float* twb3, const tc2li_preintegrated* const* pre, float* vel3, float Rwg9[9]);
/* Optimizer::InertialOptimization(pMap, Rwg, scale), the second overload (SF/src/Optimizer.cc:2359-2466; LocalMapping::ScaleRefinement):
 * Gauss-Newton, `iterations` = 10 in the reference, gravity direction and scale only; the keyframes' velocities and biases ([n][3] each,
 * edge i takes keyframe i - 1's biases) are fixed, every edge carries Huber(1).  chi2 (may be NULL) = activeRobustChi2 before / after.
 * Returns the iterations run. */
int tc2li_inertial_scale_refinement(int n_kfs, const double* Rwb9, const double* twb3, const double* vel3, const double* bg3, const double* ba3,
                                    const tc2li_preintegrated* const* pre, double Rwg9[9], double* scale, int iterations, double chi2[2]);
int tc2li_inertial_optimization(int n_kfs, const double* Rwb9, const double* twb3, double* vel3, const tc2li_preintegrated* const* pre,
                                double Rwg9[9], double* scale, double bg[3], double ba[3], int mono, int fixed_vel, float prior_g, float prior_a,
                                int iterations, tc2li_inertial_init_stats* stats);


/* ------------------------------------------------------------------------------------------------
 * Tracking::TrackWithMotionModel (SF/src/Tracking.cc:2737-2834), data path only, for a batch of independent frames
 * whose features are device-resident: SearchByProjection(cur, last, th) with ORBmatcher(0.9, true), the 2*th retry
 * when fewer than 20 matches, Optimizer::PoseOptimization, outlier bookkeeping.  Frame f is images 2f / 2f+1 of the
 * handle's last tc2li_orb_extract_batch call; keypoints ([2*n_frames][capacity]) and u_right ([n_frames][capacity])
 * are the host arrays that call and tc2li_stereo_match_batch returned.
 * ---------------------------------------------------------------------------------------------- */
typedef struct tc2li_last_frame {      /* what the matcher reads of mLastFrame */
    int32_t n;
    int32_t pad_;
    const uint8_t* has_point;          /* mvpMapPoints[i] != NULL */
    const uint8_t* outlier;            /* mvbOutlier[i] */
    const float* Xw;                   /* pMP->GetWorldPos(), 3 per keypoint */
    const tc2li_keypoint* keys;        /* mvKeysUn (octave, angle are read) */
    const uint8_t* descriptors;        /* pMP->GetDescriptor(), 32 B per keypoint */
    float pose7[7];                    /* LastFrame.GetPose() */
    float pad2_;
} tc2li_last_frame;

/* pose_pred7 [n_frames][7] = mVelocity * mLastFrame.GetPose() (Sophus::SE3f).  Outputs: poses7 [n_frames][7] (double:
 * the optimised pose rounded through float as Frame::SetPose does, or the prediction when tracking failed),
 * map_point_of_keypoint [n_frames][capacity] = index of the last-frame point now held by keypoint i (mvpMapPoints[i])
 * or -1, outliers already discarded; n_matches[f] = matches after the search stage; n_inliers[f] = the value
 * PoseOptimization returned, -1 when fewer than 20 matches were found (Tracking.cc:2785-2793).
 * The batched tracking entries (this one, tc2li_track_local_map_batch, tc2li_search_local_points_batch and the keyframe overload of
 * relocalisation) assume that every source point has observations (Observations() > 0): a match always blocks its keypoint, so no two
 * points of one search share a keypoint and the histogram filter's removal by keypoint equals a removal by point. */
int tc2li_track_motion_model_batch(tc2li_orb* orb, int n_frames, const tc2li_keypoint* keypoints, const float* u_right,
                                   int capacity, const tc2li_last_frame* last, const float* pose_pred7,
                                   const tc2li_camera* cam, float b, float th, double* poses7,
                                   int32_t* map_point_of_keypoint, int32_t* n_matches, int32_t* n_inliers, void* stream);

/* The data path of Tracking::TrackLocalMap (SF/src/Tracking.cc:3119-3230) after TrackWithMotionModel, for the same batch of
 * frames: SearchLocalPoints (:3232-3294: Frame::isInFrustum(pMP, 0.5) + ORBmatcher(0.8).SearchByProjection(F, mvpLocalMapPoints,
 * th, mbFarPoints, mThFarPoints)), Optimizer::PoseOptimization over every map point the frame holds, mnMatchesInliers.
 * poses7 [n_frames][7] (float) = the frames' current poses; held [n_frames][capacity]: 0 = keypoint i holds no map point, 1 = holds
 * one with Observations() > 0 (it blocks the search), 2 = holds one without observations; held_Xw [n_frames][capacity][3] its
 * world position.  local_points + local_offsets [n_frames + 1]: per frame the local map points still to be matched (not bad,
 * mnLastFrameSeen != this frame).  th as chosen at :3262-3281.  Out: poses7_out (double), local_of_keypoint [n_frames][capacity] =
 * index (within the frame's list) of the local point now held by keypoint i or -1, outlier [n_frames][capacity] = mvbOutlier
 * of every held point, n_matches[f] = SearchByProjection's result, n_inliers[f] = mnMatchesInliers.  The caller applies the
 * sensor-specific clean-up (:3198-3199) and the thresholds of :3205-3229. */
int tc2li_track_local_map_batch(tc2li_orb* orb, int n_frames, const tc2li_keypoint* keypoints, const float* u_right, int capacity,
                                const float* poses7, const uint8_t* held, const float* held_Xw, const tc2li_map_point* local_points,
                                const int32_t* local_offsets, const tc2li_camera* cam, float th, int far_points, float th_far_points,
                                double* poses7_out, int32_t* local_of_keypoint, uint8_t* outlier, int32_t* n_matches,
                                int32_t* n_inliers, void* stream);
/* Tracking::SearchLocalPoints alone (SF/src/Tracking.cc:3232-3294), same arguments: with the IMU initialised TrackLocalMap does not call
 * PoseOptimization but PoseInertialOptimizationLastFrame / LastKeyFrame on the frame's map points (Tracking.cc:2857-2878;
 * tc2li_pose_inertial_optimization_batch), and TrackWithMotionModel is PredictStateIMU alone (:2746-2752).  local_of_keypoint and
 * n_matches as above. */
int tc2li_search_local_points_batch(tc2li_orb* orb, int n_frames, const tc2li_keypoint* keypoints, const float* u_right, int capacity,
                                    const float* poses7, const uint8_t* held, const float* held_Xw, const tc2li_map_point* local_points,
                                    const int32_t* local_offsets, const tc2li_camera* cam, float th, int far_points, float th_far_points,
                                    int32_t* local_of_keypoint, int32_t* n_matches, void* stream);

/* The LiDAR co-visibility window of LocalLVBundleAdjustment (SF/src/OptimizerWithLidar.cc:226-260): the first
 * min(6, .) local keyframes with a non-empty surface cloud, in list order.  Replaces LidarCovisRes::AddFromKeyFrame /
 * BuildVoxHess (SF/src/LidarRes.cc:32-80) and the EdgeLidarSE3 they feed (SF/include/G2oTypesWithLidar.h:88-236). */
typedef struct tc2li_lidar_window {
    int32_t n_keyframes;          /* win_size_, 1 .. 20 */
    int32_t pad_;
    const int32_t* pose_index;    /* [n_keyframes] rows of poses7, the order of eBalm->setVertex(i, .) */
    const float* cloud_xyz;       /* GetSurfacePcl() of the keyframes back to back, x y z per point, LiDAR frame */
    const int32_t* cloud_offsets; /* [n_keyframes + 1], in points; every keyframe must have points */
    float Tcl[7];                 /* mLidarParam->mTcl as qx qy qz qw tx ty tz */
    float pad2_;
    double weight;                /* mLidarParam->mWeightLocalBA (the edge's information) */
} tc2li_lidar_window;

typedef struct tc2li_lidar_ba_stats {
    int32_t n_planes, hessian_evaluations;
    double residual, chi2;        /* the edge's last error and chi2 */
} tc2li_lidar_ba_stats;

/* OptimizerWithLidar::LocalLVBundleAdjustment with the LiDAR edge (SF/src/OptimizerWithLidar.cc:60-487): the arguments of
 * tc2li_local_bundle_adjustment plus the window.  The planes are extracted at the input poses; the optimiser then
 * minimises the visual cost + weight * (sum over planes of N * lambda_min)^2 as the reference's edge does, including
 * its bookkeeping (the Hessian is kept while the LiDAR cost grows, 6x6 blocks read at element offsets).  lidar == NULL
 * is the visual-only optimisation.  Returns the number of iterations performed. */
int tc2li_local_lv_bundle_adjustment(double* poses7, const uint8_t* fixed, int n_poses, double* points3, int n_points,
                                     const tc2li_ba_edge* edges, int n_edges, const tc2li_camera* cam, int iterations,
                                     double lambda_init, const volatile uint8_t* stop_flag, double* edge_chi2,
                                     uint8_t* edge_depth_positive, tc2li_ba_stats* stats, const tc2li_lidar_window* lidar,
                                     tc2li_lidar_ba_stats* lidar_stats, void* stream);

/* Many independent windows (multi-sequence operation, BASELINE configs[4]): every problem is what one
 * tc2li_local_lv_bundle_adjustment call takes; up to max_concurrency of them are in flight at a time, each on its own
 * HIP stream with its own device workspace, so that the small kernels of different windows overlap on the GPU.
 * results[i] receives the return value of problem i.  Returns the number of problems that succeeded. */
typedef struct tc2li_ba_problem {
    double* poses7; const uint8_t* fixed; double* points3; const tc2li_ba_edge* edges;
    int32_t n_poses, n_points, n_edges, iterations;
    double lambda_init;
    const volatile uint8_t* stop_flag;
    double* edge_chi2; uint8_t* edge_depth_positive;
    tc2li_ba_stats* stats;
    const tc2li_lidar_window* lidar; tc2li_lidar_ba_stats* lidar_stats;
} tc2li_ba_problem;
int tc2li_local_bundle_adjustment_batch(const tc2li_ba_problem* problems, int n_problems, const tc2li_camera* cam,
                                        int max_concurrency, int32_t* results);
/* The same for callers that run several local-mapping workers of their own (one LocalMapping thread per sequence in the reference,
 * SF/src/LocalMapping.cc:66-160; a multi-sequence system has a pool of them): the windows of this call form ONE lock-step group on the
 * context `group` (0 .. 7: its stream, device work spaces and host pool).  Calls on different groups run side by side and return
 * independently -- no worker waits for the slowest group of a common call --, calls on the same group serialise.  Every window's result is
 * the one tc2li_local_bundle_adjustment_batch / tc2li_local_lv_bundle_adjustment give for it. */
int tc2li_local_bundle_adjustment_batch_group(const tc2li_ba_problem* problems, int n_problems, const tc2li_camera* cam, int group,
                                              int32_t* results);

/* The same windows through a running ENGINE instead of a call per batch: the local-mapping threads of many sequences (one
 * LocalMapping::Run loop per sequence, SF/src/LocalMapping.cc:66-160, each reaching Optimizer::LocalBundleAdjustment /
 * OptimizerWithLidar::LocalLVBundleAdjustment at its own time) submit their windows as they come and collect them one ticket at a time.
 * The engine keeps up to max_windows windows in flight in ONE lock-step Levenberg-Marquardt queue on a stream of its own: a window joins
 * the queue at the next round after its setup, leaves it at the round its optimisation ends, and its slot is handed to the next waiting
 * window -- no window waits for the slowest one of a batch, and the host work of setting a window up and of writing its results back
 * runs beside the rounds of the others.  Every window's result is bit for bit the one tc2li_local_bundle_adjustment_batch /
 * tc2li_local_lv_bundle_adjustment give for it (a window's arithmetic never depends on its neighbours in the queue).
 *   submit: the windows of `problems` (arrays that stay valid and untouched until the ticket has been waited for) -> ticket > 0, or an
 *           error code < 0; results[i] receives window i's return value.  May be called from any thread, also while tickets are open.
 *   poll:   1 when every window of the ticket has finished (wait will not block), 0 while one is still in the queue.
 *   wait:   blocks until every window of the ticket has finished -> number of windows that succeeded; a ticket is collected once.
 *   destroy: finishes the windows already submitted, then stops the engine's thread. */
typedef struct tc2li_ba_engine tc2li_ba_engine;
int tc2li_ba_engine_create(const tc2li_camera* cam, int max_windows, tc2li_ba_engine** out);
void tc2li_ba_engine_destroy(tc2li_ba_engine* engine);
int64_t tc2li_ba_engine_submit(tc2li_ba_engine* engine, const tc2li_ba_problem* problems, int n_problems, int32_t* results);
int tc2li_ba_engine_poll(tc2li_ba_engine* engine, int64_t ticket);
int tc2li_ba_engine_wait(tc2li_ba_engine* engine, int64_t ticket);

/* One window split over the GPUs of a node (BASELINE configs[4]): the landmarks -- and with them the stereo / mono
 * edges, W, Hll and the back-substitution -- are partitioned over the ranks (landmark l belongs to rank l % world); every rank
 * keeps all keyframe poses.  What the ranks exchange are the shared-pose blocks only: per LM trial ONE sum of
 * [S | b_schur | b_p] (the rank's part of the reduced camera system: its Hpp, minus its landmarks' W Hll^-1 W^T), and one sum
 * of [scale, chi2] after the trial update; once per call the max / sum that g2o's initial lambda needs, and at the end one
 * sum that hands every rank all points, per-edge chi2 and depth flags.  The LM control flow, the LDL^T of the reduced system
 * and the LiDAR edge are replicated (they are deterministic, so every rank takes the same decisions).
 * The reference has no counterpart: its g2o solver is single-threaded (SF/Thirdparty/g2o/config.h:4); this entry is the
 * "RCCL all-reduce of the shared-pose Hessian" BASELINE.json names.  EVERY rank passes the SAME arguments (the whole window)
 * and every rank receives the whole result.  The sums run in rank order inside the collective, so the result agrees with the
 * single-GPU entry to rounding, not bit for bit.
 *
 * allreduce(ctx, device_buf, count, op, stream): in-place all-reduce of `count` doubles in device memory, enqueued on (or
 * ordered after the work already on) `stream`; returns 0 on success.  tc2li_rccl_allreduce below is such a function over an
 * RCCL communicator; a host may pass its own (torch.distributed, MPI). */
enum { TC2LI_REDUCE_SUM = 0, TC2LI_REDUCE_MAX = 1 };
typedef int (*tc2li_allreduce_fn)(void* ctx, double* device_buf, size_t count, int op, void* stream);
typedef struct tc2li_ba_shard {
    int32_t rank, world;
    tc2li_allreduce_fn allreduce;
    void* ctx;
} tc2li_ba_shard;
int tc2li_local_lv_bundle_adjustment_sharded(double* poses7, const uint8_t* fixed, int n_poses, double* points3, int n_points,
                                             const tc2li_ba_edge* edges, int n_edges, const tc2li_camera* cam, int iterations,
                                             double lambda_init, const volatile uint8_t* stop_flag, double* edge_chi2,
                                             uint8_t* edge_depth_positive, tc2li_ba_stats* stats, const tc2li_lidar_window* lidar,
                                             tc2li_lidar_ba_stats* lidar_stats, const tc2li_ba_shard* shard, void* stream);
/* The rank's share of a window: landmark_owned[l] = 1 where l % world == rank, edge_owned[e] likewise for the edge's landmark.
 * Host logic only (no device needed).  Returns the number of owned edges. */
int tc2li_ba_shard_select(const tc2li_ba_edge* edges, int n_edges, int n_points, int rank, int world, uint8_t* landmark_owned,
                          uint8_t* edge_owned);

/* RCCL glue for the sharded window (one process per GPU; librccl is loaded on first use, the library has no link-time
 * dependency on it).  unique_id: 128 bytes made by rank 0 with tc2li_rccl_unique_id and handed to the other ranks by the
 * launcher (bench.py broadcasts it over torch.distributed).  tc2li_rccl_allreduce has the tc2li_allreduce_fn signature with
 * ctx = the communicator. */
int tc2li_rccl_unique_id(void* unique_id_128);
int tc2li_rccl_comm_create(const void* unique_id_128, int rank, int world, void** comm);
int tc2li_rccl_comm_destroy(void* comm);
int tc2li_rccl_allreduce(void* comm, double* device_buf, size_t count, int op, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Visual-inertial local bundle adjustment -- the optimisation of Optimizer::LocalInertialBA (SF/src/Optimizer.cc:1512-2085;
 * caller LocalMapping.cc:158,161): vertices VertexPose (ImuCamPose, body-frame update), VertexVelocity, VertexGyroBias,
 * VertexAccBias per keyframe and marginalised points; edges EdgeMono / EdgeStereo (Huber), EdgeInertial (+ Huber
 * sqrt(16.92) where `robust`), EdgeGyroRW, EdgeAccRW (SF/include/G2oTypes.h, SF/src/G2oTypes.cc).  The host shim gathers
 * the temporal window, the fixed keyframes and the points exactly as :1520-1640 does and passes them flattened, keyframes in
 * vertex-id order.  Projection edges run on the GPU, the few inertial edges on the host (row c6); the reduced system
 * (6 + 9 unknowns per optimisable keyframe; g2o's sparse LinearSolverEigen, :1635-1638) is solved on the GPU inside the envelope of
 * the velocity / bias band (windows of at most 25 optimisable keyframes whose inertial edges join keyframes at most two places apart
 * in the numbering; other windows, and every window with TC2LI_LVI_DEVICE_SOLVE=0, on the host by the same elimination).
 * ---------------------------------------------------------------------------------------------- */
typedef struct tc2li_inertial_keyframe {  /* ImuCamPose(KeyFrame*) + velocity + biases, widened from the map's floats */
    double Rcw[9], tcw[3];                /* GetRotation(), GetTranslation() */
    double Rwb[9], twb[3];                /* GetImuRotation(), GetImuPosition() */
    double velocity[3], gyro_bias[3], acc_bias[3];
} tc2li_inertial_keyframe;
typedef struct tc2li_imu_calib { double Rcb[9], tcb[3], Rbc[9], tbc[3]; } tc2li_imu_calib;  /* mImuCalib.mTcb / mTbc */
typedef struct tc2li_inertial_link {      /* EdgeInertial + EdgeGyroRW + EdgeAccRW between keyframe kf1 (= kf2->mPrevKF) and kf2 */
    int32_t kf1, kf2;
    int32_t robust;                       /* i == N-1 || bRecInit (Optimizer.cc:1757-1766) */
    int32_t pad_;
    double info_scale;                    /* 1e-2 for the link to the keyframe before the window, else 1 */
    const tc2li_preintegrated* preintegrated; /* kf2->mpImuPreintegrated after SetNewBias(kf1->GetImuBias()) */
} tc2li_inertial_link;

/* fixed[k]: the keyframe's pose, velocity and biases are constants; has_imu[k] = pKFi->bImu.  iterations / lambda_init:
 * 10 and 1e0, or 4 and 1e-2 for bLarge (:1516-1523, 1637-1650).  stats->initial_chi2 / final_chi2 are activeRobustChi2()
 * before and after optimize() (err / err_end of :1968-1971).  Keyframes and points are updated in place; edge_chi2 /
 * edge_depth_positive as in tc2li_local_bundle_adjustment.  Returns the number of iterations performed. */
int tc2li_local_inertial_bundle_adjustment(tc2li_inertial_keyframe* keyframes, const uint8_t* fixed, const uint8_t* has_imu,
                                           int n_keyframes, const tc2li_imu_calib* calib, double* points3, int n_points,
                                           const tc2li_ba_edge* edges, int n_edges, const tc2li_inertial_link* links,
                                           int n_links, const tc2li_camera* cam, int iterations, double lambda_init,
                                           const volatile uint8_t* stop_flag, double* edge_chi2,
                                           uint8_t* edge_depth_positive, tc2li_ba_stats* stats, void* stream);

/* OptimizerWithLidar::LocalLVIBA (SF/src/OptimizerWithLidar.cc:489-1100): the visual-inertial local BA plus the LiDAR edge
 * on the body-frame pose vertices (EdgeLidar, SF/src/G2oTypesWithLidar.cc:33-140; LidarCovisRes::ComputeJandH,
 * SF/src/LidarRes.cc:89-128).  lidar->pose_index are rows of `keyframes` -- the reference takes the first min(N, 6) optimisable
 * keyframes when N > 5 (:704-724); Tbl = mLidarParam->mTbl as qx qy qz qw tx ty tz.  The edge's error is sqrt(sum over planes of
 * N * lambda_min), its information lidar->weight.  lidar == NULL is tc2li_local_inertial_bundle_adjustment. */
int tc2li_local_lvi_bundle_adjustment(tc2li_inertial_keyframe* keyframes, const uint8_t* fixed, const uint8_t* has_imu,
                                      int n_keyframes, const tc2li_imu_calib* calib, double* points3, int n_points,
                                      const tc2li_ba_edge* edges, int n_edges, const tc2li_inertial_link* links, int n_links,
                                      const tc2li_camera* cam, int iterations, double lambda_init,
                                      const volatile uint8_t* stop_flag, double* edge_chi2, uint8_t* edge_depth_positive,
                                      tc2li_ba_stats* stats, const tc2li_lidar_window* lidar, const float* Tbl,
                                      tc2li_lidar_ba_stats* lidar_stats, void* stream);

/* Many independent LocalLVIBA windows (the local-mapping threads of many sequences in the camera-LiDAR-inertial configuration): every
 * problem is what one tc2li_local_lvi_bundle_adjustment call takes (same IMU calibration and camera for all).  With max_concurrency > 1
 * the windows advance through the Levenberg-Marquardt phases in lock step like tc2li_local_bundle_adjustment_batch's -- one launch per
 * kernel and one synchronisation per phase for all windows (Schur product, solve of the reduced system and trial estimate are one
 * queue with one synchronisation per Levenberg trial), the inertial edges on host threads between the phases -- and every window's
 * result is the one of the one-window call.  (A window's reduced system is solved on the device or by the host's envelope LDL^T according
 * to the window's own shape -- at most 25 optimisable keyframes with IMU state, inertial edges at most two keyframes apart --; the two
 * solvers agree to 1e-9 relative, not bit for bit.  A lock-step group runs one of them: windows that differ from their group's majority
 * go through the one-window call inside the batch call.)  results[i] = iterations of window i or its error code;
 * returns the number of windows that succeeded. */
typedef struct tc2li_lvi_problem {
    tc2li_inertial_keyframe* keyframes; const uint8_t* fixed; const uint8_t* has_imu;
    double* points3; const tc2li_ba_edge* edges; const tc2li_inertial_link* links;
    int32_t n_keyframes, n_points, n_edges, n_links, iterations, pad_;
    double lambda_init;
    const volatile uint8_t* stop_flag;
    double* edge_chi2; uint8_t* edge_depth_positive;
    tc2li_ba_stats* stats;
    const tc2li_lidar_window* lidar; const float* Tbl; tc2li_lidar_ba_stats* lidar_stats;
} tc2li_lvi_problem;
int tc2li_local_lvi_bundle_adjustment_batch(const tc2li_lvi_problem* problems, int n_problems, const tc2li_imu_calib* calib,
                                            const tc2li_camera* cam, int max_concurrency, int32_t* results);
/* The same as ONE lock-step group on the context `group` (0 .. 7), for callers with several local-mapping workers: as
 * tc2li_local_bundle_adjustment_batch_group.  Every window's result is the one tc2li_local_lvi_bundle_adjustment gives for it. */
int tc2li_local_lvi_bundle_adjustment_batch_group(const tc2li_lvi_problem* problems, int n_problems, const tc2li_imu_calib* calib,
                                                  const tc2li_camera* cam, int group, int32_t* results);

/* ---- local mapping: new map points ----
 * What ORBmatcher::SearchForTriangulation (SF/src/ORBmatcher.cc:916) and the pair loop of LocalMapping::CreateNewMapPoints
 * (SF/src/LocalMapping.cc:402-726) read of a keyframe (pinhole camera, no second camera model). */
typedef struct tc2li_keyframe_view {
    int32_t n, n_nodes;            /* keypoints; entries of mFeatVec */
    const tc2li_keypoint* keys;    /* mvKeysUn */
    const uint8_t* descriptors;    /* mDescriptors, [n][32] */
    const float* u_right;          /* mvuRight */
    const float* depth;            /* mvDepth */
    const uint8_t* has_point;      /* GetMapPoint(i) != NULL */
    const int32_t* fv_node;        /* mFeatVec: node ids, ascending */
    const int32_t* fv_offset;      /* [n_nodes + 1] */
    const int32_t* fv_index;       /* the feature indices of every node, in insertion order */
    float pose7[7];                /* GetPose(): qx qy qz qw tx ty tz of Tcw */
    float pad_;
} tc2li_keyframe_view;

/* ORBmatcher::SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse): match12[i] = matched keypoint of kf2 or
 * -1 for every keypoint of kf1 (vMatchedPairs = the pairs with match12[i] >= 0, i ascending).  level_sigma2 = mvLevelSigma2,
 * scale_factors = mvScaleFactors.  Returns nmatches. */
int tc2li_search_for_triangulation(const tc2li_keyframe_view* kf1, const tc2li_keyframe_view* kf2, const tc2li_camera* cam,
                                   const float* scale_factors, const float* level_sigma2, int n_levels, int only_stereo,
                                   int coarse, int check_orientation, int32_t* match12, void* stream);

typedef struct tc2li_new_map_point {
    int32_t idx1, neighbour, idx2; /* keypoint of the current keyframe, index into `neighbours`, keypoint there */
    int32_t stereo;                /* the point came from UnprojectStereo (bPointStereo) */
    float x3D[3];
    float pad_;
} tc2li_new_map_point;

/* The geometric loop of LocalMapping::CreateNewMapPoints over the neighbours the caller chose (vpNeighKFs, in order): search,
 * parallax gates, triangulation or stereo un-projection, depth / reprojection / scale gates; a keypoint that received a point
 * from an earlier neighbour is skipped for the later ones.  mb = pKF->mb, cam->bf = mbf, scale_factor = mfScaleFactor, inertial =
 * mbInertial, far_points / th_far_points = mbFarPoints / mThFarPoints, coarse = bCoarse.  The points come in creation order;
 * the caller creates the MapPoint objects, adds the observations and refreshes them (tc2li_map_points_refresh).  Triangulated
 * coordinates agree with the reference to float rounding (Eigen's JacobiSVD is not reproduced bit for bit).  Returns the count. */
int tc2li_create_new_map_points(const tc2li_keyframe_view* current, const tc2li_keyframe_view* neighbours, int n_neighbours,
                                const tc2li_camera* cam, float mb, const float* scale_factors, const float* level_sigma2,
                                int n_levels, float scale_factor, int inertial, int far_points, float th_far_points, int coarse,
                                tc2li_new_map_point* points, int capacity, void* stream);

/* ORBmatcher::Fuse(pKF, vpMapPoints, th, bRight = false), the search (SF/src/ORBmatcher.cc:1157-1330; called from
 * LocalMapping::SearchInNeighbors :728-837): for every map point the keypoint of the keyframe it is fused with -- projection and
 * gates (depth, image, distance range, viewing direction), MapPoint::PredictScale, the keypoints inside th * scale on the
 * keyframe's feature grid, level and reprojection gates (7.8 / 5.99 on mvInvLevelSigma2), least descriptor distance <= TH_LOW --
 * or -1.  valid[i] = pMP && !pMP->isBad() && !pMP->IsInKeyFrame(pKF).  A point's result depends on no other point; the caller
 * walks the results in list order and does Replace / AddObservation on its objects (re-checking isBad / IsInKeyFrame there).
 * best_dist may be NULL.  Returns how many points found a keypoint. */
int tc2li_fuse_search(const tc2li_frame_view* keyframe, const float pose7[7], const float cam4[4], float bf, const float* scale_factors,
                      const float* inv_level_sigma2, int n_levels, float log_scale_factor, const tc2li_map_point* points,
                      const uint8_t* valid, int n_points, float th, int32_t* best_idx, int32_t* best_dist, void* stream);

/* ---- local mapping for many keyframes: keyframe store, CreateNewMapPoints and Fuse search in batches ----
 * The store keeps on the device what a KeyFrame never changes after its constructor (SF/src/KeyFrame.cc:56-104: mvKeysUn,
 * mDescriptors, mvuRight, mvDepth, mFeatVec, mnMinX .. mnMaxY, and the feature grid mGrid that GetFeaturesInArea :716-760 walks),
 * so that the batch entries below upload only what changes between calls: the poses (GetPose() after a BA) and has_point
 * (GetMapPoint(i) != NULL after every created or fused point).
 * One slab is allocated at create; a slot has a fixed size derived from max_keypoints, so a put never moves another slot, and puts
 * into other slots are safe while searches run.  Slots are numbered 0 .. max_keyframes - 1; the caller keeps the keyframe -> slot
 * map: put at Tracking::CreateNewKeyFrame, erase at KeyFrame::SetBadFlag (:585). */
typedef struct tc2li_keyframe_store tc2li_keyframe_store;
int tc2li_keyframe_store_create(int max_keyframes, int max_keypoints, tc2li_keyframe_store** out);
int tc2li_keyframe_store_destroy(tc2li_keyframe_store* store);
/* Stores n keyframes: views[k] goes to slots[k] (an occupied slot is replaced), bounds4[k] = mnMinX, mnMaxX, mnMinY, mnMaxY.  The
 * has_point and pose7 fields of the views are IGNORED: they are inputs of every search.  All views are packed into one pinned
 * staging block, copied once, and the feature grids of the n keyframes are built by one launch; the call returns when the data is
 * resident, so a search on any stream may follow.  Every check comes before any device work, and a refused call leaves the store
 * unchanged: the checks of tc2li_create_new_map_points on a view plus octaves in [0, n_levels); TC2LI_ERR_CAPACITY for a keyframe
 * with more keypoints (or feature-vector entries) than max_keypoints or than the feature grid's 3072; TC2LI_ERR_INVALID for a slot
 * out of range or named twice in the call. */
int tc2li_keyframe_store_put_batch(tc2li_keyframe_store* store, int n, const int32_t* slots, const tc2li_keyframe_view* views,
                                   const float* bounds4, int n_levels, void* stream);
int tc2li_keyframe_store_erase(tc2li_keyframe_store* store, int slot);
/* n_keypoints / n_nodes of the keyframe in the slot; -1 / -1 for an empty slot */
int tc2li_keyframe_store_info(tc2li_keyframe_store* store, int slot, int32_t* n_keypoints, int32_t* n_nodes);

/* One LocalMapping::CreateNewMapPoints (SF/src/LocalMapping.cc:402-726): mpCurrentKeyFrame and vpNeighKFs as store slots, with the
 * poses and has_point they have at the time of the call.  The same slot may appear in many problems with different poses and
 * has_point. */
typedef struct tc2li_new_points_problem {
    int32_t current;                 /* store slot of mpCurrentKeyFrame */
    int32_t n_neighbours;
    const int32_t* neighbours;       /* store slots, vpNeighKFs in order */
    const float* poses7;             /* [1 + n_neighbours][7]: GetPose() of current, then of each neighbour */
    const uint8_t* const* has_point; /* [1 + n_neighbours] arrays, each of that keyframe's n */
    uint8_t inertial, far_points, coarse, pad_; /* mbInertial, mbFarPoints, bCoarse */
    float th_far_points;             /* mThFarPoints */
} tc2li_new_points_problem;

/* tc2li_create_new_map_points for n_problems keyframes in one call: problem p yields exactly the records of the single call for
 * the same keyframe, neighbours, poses, has_point and flags -- same creation order (neighbour-major, keypoint-ascending, a
 * keypoint served by an earlier neighbour skipped for the later ones), same x3D bits -- at points[point_offsets[p] ...], and
 * n_points[p] of them (at most one per keypoint of the current keyframe).  One packed upload, three kernel launches whatever the
 * batch, one download, one wait; the stream is the caller's or, when NULL, the calling thread's own, and concurrent callers share no
 * work space.  Room point_offsets[p + 1] - point_offsets[p] smaller than a problem's count: TC2LI_ERR_CAPACITY, with n_points
 * filled for all problems (and the records that fit written).  An empty or out-of-range slot: TC2LI_ERR_INVALID before any launch.
 * Returns the number of points written. */
int tc2li_create_new_map_points_batch(tc2li_keyframe_store* store, const tc2li_new_points_problem* problems, int n_problems,
                                      const tc2li_camera* cam, float mb, const float* scale_factors, const float* level_sigma2,
                                      int n_levels, float scale_factor, tc2li_new_map_point* points, const int32_t* point_offsets,
                                      int32_t* n_points, void* stream);

/* One ORBmatcher::Fuse(pKF, vpMapPoints, th) search (SF/src/ORBmatcher.cc:1157-1330) of LocalMapping::SearchInNeighbors (:728-837). */
typedef struct tc2li_fuse_item {
    int32_t keyframe;          /* store slot of the keyframe the points are fused into */
    int32_t first_point;       /* into points[] */
    int32_t first_valid;       /* into valid[]: valid differs per target (IsInKeyFrame), the point list often does not */
    int32_t n_points;
    float pose7[7];            /* GetPose() of that keyframe */
    float th;
} tc2li_fuse_item;

/* tc2li_fuse_search for n_items (keyframe, point list) items in one call, on the grids the store built at put: the results of item k
 * lie at best_idx / best_dist [first_valid, first_valid + n_points) -- the output is indexed like valid -- and equal those of the
 * single call for that keyframe, pose, points, valid and th; n_fused[k] counts them.  Several items may name one point range.
 * SearchInNeighbors has two stages and the second reads what the first changed, so the caller issues stage 1 (the current
 * keyframe's points into every target keyframe, :778-788) for all sequences in one call, applies the results (Replace /
 * AddObservation on its objects, as for the single call), then issues stage 2 (the targets' points into the current keyframe,
 * :795-817: one item per sequence) in a second call.  One upload, one launch over all (item, point) pairs, one download.  An empty or
 * out-of-range slot, a range outside n_points_total / n_valid_total or log_scale_factor <= 0: TC2LI_ERR_INVALID before any
 * launch.  best_dist may be NULL.  Returns the sum of n_fused. */
int tc2li_fuse_search_batch(tc2li_keyframe_store* store, const tc2li_fuse_item* items, int n_items, const float cam4[4], float bf,
                            const float* scale_factors, const float* inv_level_sigma2, int n_levels, float log_scale_factor,
                            const tc2li_map_point* points, int n_points_total, const uint8_t* valid, int n_valid_total,
                            int32_t* best_idx, int32_t* best_dist, int32_t* n_fused, void* stream);

/* ---- LocalMapping::SearchInNeighbors (SF/src/LocalMapping.cc:728-837) in the reference's order, for many sequences in one call ----
 * The reference fuses target by target: after target k a point that absorbed another (MapPoint::Replace, SF/src/MapPoint.cc:257-309)
 * carries a new descriptor (ComputeDistinctiveDescriptors at :306), more observations and is "in" more keyframes, the loser is bad, and
 * target k + 1 is searched with that state (ORBmatcher.cc:1311, :1323, :1328 read it).  One tc2li_fuse_search_batch call over all
 * targets searches every target with the entry state and departs from the reference wherever a point absorbs another before a later
 * target.  Here the whole function runs on the flat graph with the side effects simulated, as tc2li_keyframe_culling_batch simulates
 * SetBadFlag.  Rig: pinhole stereo, NLeft == -1, mpCamera2 == nullptr, mbMonocular == false (nn = 10 at :731); the bRight calls of
 * :787 and :817 are not covered.  One problem is one mpCurrentKeyFrame; all pointers are host memory and the call copies the arrays;
 * indices are rows of the problem's own tables; row order stands in for the address order of the reference's
 * std::map<KeyFrame*, tuple<int,int>> mObservations (as in tc2li_ba_window_problem).  The problems of a batch are independent and one
 * store slot may appear in several problems.
 *
 * Keyframes (n_keyframes rows): the current keyframe, everything its covisibility lists and mPrevKF chain can reach within rule 1, and
 * every observer of every point listed.
 *   kf_slot        the keyframe's store slot; in the host entry an index into views
 *   kf_flags       bit 0 isBad(); bit 1 mnFuseTargetForKF == mpCurrentKeyFrame->mnId on entry (:739)
 *   prev_kf        mPrevKF (:765), -1 = NULL
 *   poses7         [n][7] GetPose()
 *   covis_offsets / covis   CSR of mvpOrderedConnectedKeyFrames (GetBestCovisibilityKeyFrames, :734, :749); only the rows of the current
 *                  keyframe and of its first-ring targets are read
 *   slot_offsets / slot_point   CSR of GetMapPointMatches() (:781, :802, :821), -1 = NULL; every row has the keyframe's stored keypoint count
 * Points (n_points rows):
 *   points         position, normal, the two invariance distances, max_distance_raw, mDescriptor: what tc2li_fuse_search_batch takes
 *   point_flags    bit 0 isBad(); bit 1 mnFuseCandidateForKF == mpCurrentKeyFrame->mnId on entry (:809)
 *   point_nobs     nObs (MapPoint.cc:171-174);  point_found / point_visible  mnFound / mnVisible (:304-305)
 *   point_ref_kf   mpRefKF (:477);  point_ref_level_scale  as in tc2li_map_points_refresh (:494)
 *   obs_offsets / obs_kf / obs_index   CSR of mObservations; a row ascends strictly by keyframe row; obs_index is the left index
 * Scalars: current = row of mpCurrentKeyFrame; inertial = mbInertial (:763); abort = mbAbortBA AS IT IS WHEN THE CALL IS MADE -- the
 * reference reads it live at :758 and :791; the snapshot is a stated deviation, as abort_ba is in tc2li_culling_problem;
 * last_level_scale = mvScaleFactors[nLevels - 1] (MapPoint.cc:500).  The search radius factor is Fuse's default th = 3.0.
 *
 * Rule 1, targets (:731-777).  The first 10 entries of the current keyframe's covisibility row (:734), skipping a keyframe that is bad
 *   or marked (:739); each keyframe taken is marked (:742).  For i over the targets gathered by that first loop (imax is fixed before
 *   the loop, :747) the first 20 of target i's row (:749), skipping a keyframe that is bad, marked or the current one (:753), marking
 *   what is taken (:756).  With abort the loop breaks after i = 0 has been processed (:758).  With inertial, mPrevKF is walked from the
 *   current keyframe while the targets number fewer than 20 (:765-776): bad or marked keyframes are passed over, the others taken and
 *   marked.  At most 10 + 10 * 20 = 210 targets.
 * Rule 2, stage 1 (:781-788).  vpMapPointMatches is the current keyframe's slot row as it is BEFORE stage 1 (:781 copies it): later
 *   replacements in that row do not change the list.  For every target in order: Fuse(target, list) (:786).
 * Rule 3, Fuse (ORBmatcher.cc:1186-1344) walks the list in order.  An entry is skipped when it is NULL (:1190), bad NOW (:1196), or in
 *   the target keyframe NOW -- its observation list holds the target's row (:1201).  Otherwise the search runs (:1207-1318): exactly
 *   the arithmetic of tc2li_fuse_search with the point's CURRENT descriptor (:1265).  With bestDist <= 50 (:1321) let q be the live
 *   occupant of slot bestIdx of the target (:1323).  No occupant: AddObservation(target, bestIdx) (:1336; MapPoint.cc:150-175: nObs += 2
 *   if u_right[bestIdx] >= 0, else += 1) and AddMapPoint (:1337).  Occupant not bad (:1326): nObs(q) > nObs(p) ? p.Replace(q) :
 *   q.Replace(p) (:1328-1331).  Occupant bad: nothing happens.  nFused counts all three outcomes (:1339).
 * Rule 4, x.Replace(w) (MapPoint.cc:257-309).  x == w: nothing (:259).  Otherwise, for x's observations in row order (:275): w not in that
 *   keyframe (:283) -- the keyframe's slot takes w (:286) and w gains the observation with its nObs weight (:287); w already in that
 *   keyframe -- the slot becomes NULL (:297).  x is bad, holds no observations and replaced[x] = w (:267-272); w.found += x.found,
 *   w.visible += x.visible (:304-305); w.ComputeDistinctiveDescriptors() (:306; :338-412): the descriptors of w's observations in
 *   keyframes that are not bad (:361), in row order, the Hamming matrix (:381-390), per row the sorted row's entry (int)(0.5 * (N - 1))
 *   (:399), the first row with the least such median becomes mDescriptor (:401-410).  mpRefKF, position, normal and the distances do
 *   not change here.
 * Rule 5, abort (:791).  With abort the call returns after stage 1: no stage 2, no refresh, no candidate marks.
 * Rule 6, stage 2 (:795-817).  The targets in order and their slot rows AS THEY ARE AFTER STAGE 1 (:802), slots ascending: a point is
 *   taken if it is not NULL (:807), not bad and not marked (:809), and is then marked (:811).  This is vpFuseCandidates (:812).  Then
 *   Fuse(current keyframe, candidates) (:816) by rule 3.
 * Rule 7, refresh (:821-833).  For every slot of the current keyframe's row as it is now (:821) that holds a point that is not bad
 *   (:825-827): ComputeDistinctiveDescriptors (:829) and UpdateNormalAndDepth (:830; MapPoint.cc:435-503), the arithmetic of
 *   tc2li_map_points_refresh with the camera centres of poses7; a point without observations is left alone (:352, :450).
 * UpdateConnections (:836) stays tc2li_update_connections_batch; the end state below is what it needs.
 *
 * Why a target's list entries may be searched side by side (the device path), for a graph in which every slot's point has the matching
 * observation: (a) an entry that is skipped when the target starts stays skipped, because NULL and bad are final and a point leaves a
 * keyframe only by becoming bad (rule 4); (b) an earlier entry of the same target changes another point only through Replace, whose
 * loser is bad and whose winner afterwards holds the target's row -- an occupant with the matching observation held it already, the
 * list point gains it at :286-287 from such an occupant -- so every point whose descriptor or observations changed during the target
 * is skipped by rule 3 when its turn comes; (c) hence the search of an entry that is not skipped at its turn reads exactly the state
 * the point had when the target started, and only the occupant of the slot and the nObs comparison are read live.
 * The entries do NOT require that consistency: the rules above are applied as written to a slot that holds a point without the
 * matching observation.  There (b) can fail -- the winner may stay outside the target and still have an entry ahead in the list, which
 * the reference then searches with the winner's new descriptor -- so the device path checks every Replace for exactly that (winner
 * not in the target, winner ahead in the list) and hands such a problem to the host twin (TC2LI_NEIGHBORS_ON_HOST).
 *
 * Outputs; the capacities are the caller's and an array of capacity 0 may be NULL.
 *   counts [TC2LI_NEIGHBORS_COUNTS], always written: status (TC2LI_NEIGHBORS_ON_DEVICE / _ON_HOST), targets, candidates, ops, entries
 *                  of the observation CSR out, points refreshed, nFused summed over stage 1, nFused of stage 2 (fused_current, :816)
 *   targets, target_fused [target_capacity]   vpTargetKFs in order and Fuse's return value per target (:786)
 *   candidates [candidate_capacity]           vpFuseCandidates in order (:812)
 *   ops [op_capacity]   every state change in execution order: kind ADD_OBSERVATION (:1336) or REPLACE (:1329, :1331), stage_target =
 *                  the target's ordinal (n_targets for stage 2), point = the list's point, occupant (or -1), winner (REPLACE: the
 *                  survivor; else -1), kf, idx = the keyframe row and keypoint searched.  x == w and a bad occupant change nothing and
 *                  give no op.  A shim replays these on its objects.
 *   slot_point_out (the shape of slot_point), point_bad_out, point_replaced (-1 or mpReplaced, :272), point_nobs_out, point_found_out,
 *   point_visible_out, obs_offsets_out [n_points + 1], obs_kf_out, obs_index_out [obs_capacity]: the end state
 *   desc_kf, desc_index [n_points]   the observation whose descriptor is mDescriptor at the end (:410) of a point that is not bad then;
 *                  -1 where ComputeDistinctiveDescriptors did not run or returned early (:347, :352, :374) and for points that are bad
 *   refreshed [n_points] and, where it is set, normals_out [n][3], min_distance_out, max_distance_out (MapPoint.cc:499-501)
 * Errors.  TC2LI_ERR_INVALID before any device work and with nothing written: sizes, NULLs, offsets that do not ascend, indices out of
 *   range, observation rows that do not ascend strictly, a slot that is empty or out of range, a slot-row length that is not the stored
 *   keypoint count, a prev_kf chain that returns to itself within the walk of rule 1.  TC2LI_ERR_CAPACITY: counts is written for every
 *   problem with the sizes needed and no list of any problem; the call repeated with those capacities succeeds (the contract of
 *   tc2li_local_map_update_batch).
 * The device entry: one workgroup owns one problem from the targets to the refresh; one upload, one launch whatever n_problems, one
 * download.  A problem beyond a limit of tc2li_search_in_neighbors_limits -- the observations of a point are only known while running --
 * or one that the check of the paragraph above catches, is finished inside the call by the host twin, reports TC2LI_NEIGHBORS_ON_HOST
 * in counts[0] (so a caller sees how often that happens) and has the same outputs.  Both entries
 * return n_problems. */
#define TC2LI_NEIGHBORS_COUNTS 8
#define TC2LI_NEIGHBORS_ON_DEVICE 0
#define TC2LI_NEIGHBORS_ON_HOST 1
#define TC2LI_NEIGHBORS_ADD_OBSERVATION 1
#define TC2LI_NEIGHBORS_REPLACE 2
#define TC2LI_NEIGHBORS_MAX_TARGETS 210
typedef struct tc2li_neighbors_op {
    int32_t kind, stage_target, point, occupant, winner, kf, idx, pad_;
} tc2li_neighbors_op;
typedef struct tc2li_neighbors_problem {
    const int32_t* kf_slot; const uint8_t* kf_flags; const int32_t* prev_kf; const float* poses7;
    const int32_t *covis_offsets, *covis, *slot_offsets, *slot_point;
    const tc2li_map_point* points; const uint8_t* point_flags;
    const int32_t *point_nobs, *point_found, *point_visible, *point_ref_kf; const float* point_ref_level_scale;
    const int32_t *obs_offsets, *obs_kf, *obs_index;
    int32_t* counts; int32_t *targets, *target_fused, *candidates; tc2li_neighbors_op* ops;
    int32_t* slot_point_out; uint8_t* point_bad_out;
    int32_t *point_replaced, *point_nobs_out, *point_found_out, *point_visible_out;
    int32_t *obs_offsets_out, *obs_kf_out, *obs_index_out, *desc_kf, *desc_index;
    uint8_t* refreshed; float *normals_out, *min_distance_out, *max_distance_out;
    int32_t n_keyframes, n_points, current;
    int32_t target_capacity, candidate_capacity, op_capacity, obs_capacity;
    float last_level_scale;
    uint8_t inertial, abort, pad_[6];
} tc2li_neighbors_problem;
int tc2li_search_in_neighbors_batch(tc2li_keyframe_store* store, const tc2li_neighbors_problem* problems, int n_problems,
                                    const float cam4[4], float bf, const float* scale_factors, const float* inv_level_sigma2,
                                    int n_levels, float log_scale_factor, void* stream);
/* The host twin: plain sequential C++, one problem per worker thread under the host thread budget; kf_slot indexes views (keys,
 * descriptors, u_right are read; bounds4[k] = mnMinX, mnMaxX, mnMinY, mnMaxY of view k), whose feature grids (KeyFrame.cc:716-760) are
 * built on the host.  counts[0] is TC2LI_NEIGHBORS_ON_HOST.  Needs no device. */
int tc2li_host_search_in_neighbors_batch(const tc2li_keyframe_view* views, const float* bounds4, int n_views,
                                         const tc2li_neighbors_problem* problems, int n_problems, const float cam4[4], float bf,
                                         const float* scale_factors, const float* inv_level_sigma2, int n_levels,
                                         float log_scale_factor);
/* The limits of the device path: out[0] the most observations a point may reach (those of tc2li_map_points_refresh's descriptor step),
 * out[1] the most keypoints of a keyframe, out[2] / out[3] the most points / keyframes of a problem whose marks live in LDS, out[4]
 * threads per problem.  Returns how many values there are; needs no device. */
int tc2li_search_in_neighbors_limits(int32_t* out, int capacity);

/* Per-map-point refresh of local mapping after a local BA / after creating or fusing points (LocalMapping.cc, Optimizer.cc:1506,
 * OptimizerWithLidar.cc:484 `pMP->UpdateNormalAndDepth()`; `ComputeDistinctiveDescriptors` in CreateNewMapPoints / Fuse):
 * MapPoint::ComputeDistinctiveDescriptors (SF/src/MapPoint.cc:338-412) and MapPoint::UpdateNormalAndDepth (:444-503) for a flat
 * list of points.  Observations of point p are [obs_offsets[p], obs_offsets[p + 1]) in the iteration order of mObservations
 * (left, then right index of every keyframe that is not bad): obs_descriptors [total][32], obs_centres [total][3] = the
 * observing camera's centre.  positions / ref_centres (mpRefKF->GetCameraCenter()) [n][3], ref_level_scale[p] =
 * mvScaleFactors[octave of the reference observation], last_level_scale = mvScaleFactors[nLevels - 1].
 * Out: best_obs[p] = the observation whose descriptor becomes mDescriptor (-1: no observations, outputs untouched),
 * normals [n][3] = mNormalVector, min_distance / max_distance = mfMinDistance / mfMaxDistance.  At most 112 observations
 * per point (TC2LI_ERR_CAPACITY beyond).  Returns n_points. */
int tc2li_map_points_refresh(int n_points, const int32_t* obs_offsets, const uint8_t* obs_descriptors, const float* obs_centres,
                             const float* positions, const float* ref_centres, const float* ref_level_scale, float last_level_scale,
                             int32_t* best_obs, float* normals, float* min_distance, float* max_distance, void* stream);

/* Local-map bookkeeping that feeds SearchLocalPoints: Tracking::UpdateLocalKeyFrames + Tracking::UpdateLocalPoints
 * (SF/src/Tracking.cc:3326-3476, :3296-3323; caller Tracking::UpdateLocalMap :3286) on a device-resident mirror of the graph
 * pieces they read.  Keyframes and map points are indices into the mirror.  The reference keys its containers by object
 * address (std::map<KeyFrame*, int> keyframeCounter, std::set<KeyFrame*> children, std::map<KeyFrame*, ...> observations), so
 * its iteration order is the allocator's; here index order stands in for address order and the caller lists children /
 * observations in the order its containers iterate.
 *   covis        mvpOrderedConnectedKeyFrames per keyframe (GetBestCovisibilityKeyFrames(10) takes the first 10)
 *   children     GetChilds();  parent / prev_kf: GetParent() / mPrevKF, -1 = none
 *   matches      GetMapPointMatches(): the map point of every keypoint slot, -1 = none
 *   obs_kf       the keyframes of GetObservations() per map point */
typedef struct tc2li_map_graph {
    int32_t n_keyframes, n_points;
    const uint8_t* kf_bad;                               /* [n_keyframes] KeyFrame::isBad() */
    const int32_t *covis_offsets, *covis;                /* CSR over keyframes */
    const int32_t *child_offsets, *children;
    const int32_t *parent, *prev_kf;                     /* [n_keyframes] */
    const int32_t *match_offsets, *matches;
    const uint8_t* point_bad;                            /* [n_points] MapPoint::isBad() */
    const int32_t *obs_offsets, *obs_kf;                 /* CSR over map points */
} tc2li_map_graph;
typedef struct tc2li_local_map tc2li_local_map;
int tc2li_local_map_create(tc2li_local_map** out);
void tc2li_local_map_destroy(tc2li_local_map* map);
/* Uploads (replaces) the mirror; call when keyframes / points / observations changed.  The arrays are copied. */
int tc2li_local_map_set_graph(tc2li_local_map* map, const tc2li_map_graph* graph, void* stream);
/* One UpdateLocalMap.  frame_points = mCurrentFrame.mvpMapPoints (mLastFrame's once the IMU is initialised, :3350), -1 = none;
 * temporal_last_kf = mCurrentFrame.mpLastKeyFrame for IMU_STEREO_LIDAR (the temporal block :3453-3469), -1 otherwise.
 * Out: mvpLocalKeyFrames in the reference's order (voted keyframes by index, then the neighbour / child / parent extensions with
 * the reference's early exits, then up to 20 temporal keyframes), reference_kf = pKFmax (-1: none), mvpLocalMapPoints in the
 * reference's order (local keyframes walked backwards, slots forwards, first occurrence kept, bad points skipped), and
 * frame_point_cleared[i] = 1 where the reference sets the frame's point to NULL because it is bad.  The local point list also
 * stays on the device (tc2li_local_map_device_points).  Returns the number of local points; TC2LI_ERR_CAPACITY when a list does not fit. */
int tc2li_local_map_update(tc2li_local_map* map, const int32_t* frame_points, int n_frame_points, int temporal_last_kf,
                           int32_t* local_keyframes, int keyframe_capacity, int32_t* n_local_keyframes, int32_t* reference_kf,
                           int32_t* local_points, int point_capacity, int32_t* n_local_points, uint8_t* frame_point_cleared,
                           void* stream);
const int32_t* tc2li_local_map_device_points(const tc2li_local_map* map);

/* UpdateLocalMap for many sequences in one call: one problem per sequence, each with the semantics of tc2li_local_map_update, line for
 * line against Tracking.cc:3296-3476.  Problems are independent: a problem's result does not depend on the batch's size or order.
 * counts [TC2LI_LOCAL_MAP_COUNTS] is always written on success and on TC2LI_ERR_CAPACITY; local_keyframes / local_points /
 * frame_point_cleared get their first N_KEYFRAMES / N_POINTS / n_frame_points entries, what lies beyond stays untouched.
 * Refused before any work with TC2LI_ERR_INVALID and the problem's number in the message, nothing written: NULL map (device entry) /
 * graph (host entry) / counts, NULL frame_points or frame_point_cleared with n_frame_points > 0, a NULL list with a capacity > 0,
 * negative sizes or capacities, a map without a graph, a frame point outside [-1, n_points), temporal_last_kf outside
 * [-1, n_keyframes), and (device entry) the same map named by two problems of one call.
 * TC2LI_ERR_CAPACITY when a list of some problem does not fit: counts holds the sizes needed for EVERY problem, no list of any
 * problem is written, and the call repeated with those capacities succeeds.  Returns n_problems (0 for an empty batch).
 * The device entry issues a number of launches, memsets, copies and stream waits that does not depend on n_problems: one upload, five
 * kernels, one download of the counts, one of the lists at the sizes found (never at capacity).  The host entry walks problem.graph in
 * plain C++ on the tracking pool, one problem per thread, validates the graph as tc2li_local_map_set_graph does, and needs no device.
 * After a batch call tc2li_local_map_device_points(map) is unspecified: the batch keeps its lists in its own buffers. */
enum tc2li_local_map_count {
    TC2LI_LOCAL_MAP_N_KEYFRAMES = 0,   /* entries of local_keyframes (mvpLocalKeyFrames) */
    TC2LI_LOCAL_MAP_N_VOTED = 1,       /* how many of them came from the vote (:3383-3398) */
    TC2LI_LOCAL_MAP_REFERENCE_KF = 2,  /* pKFmax, -1: mpReferenceKF stays */
    TC2LI_LOCAL_MAP_N_POINTS = 3,      /* entries of local_points (mvpLocalMapPoints) */
    TC2LI_LOCAL_MAP_N_CLEARED = 4,     /* frame points set to NULL because they are bad (:3345, :3369) */
    TC2LI_LOCAL_MAP_COUNTS = 8         /* ints in the block, the rest 0 */
};
typedef struct tc2li_local_map_update_problem {
    tc2li_local_map* map;              /* device entry: the sequence's mirror; the host entry does not read it */
    const tc2li_map_graph* graph;      /* host entry: the graph itself; the device entry does not read it */
    const int32_t* frame_points;       /* as tc2li_local_map_update */
    int32_t n_frame_points, temporal_last_kf;
    int32_t* counts;                   /* [TC2LI_LOCAL_MAP_COUNTS], always written */
    int32_t* local_keyframes; int32_t* local_points; uint8_t* frame_point_cleared;
    int32_t keyframe_capacity, point_capacity;
} tc2li_local_map_update_problem;
int tc2li_local_map_update_batch(const tc2li_local_map_update_problem* problems, int n_problems, void* stream);
int tc2li_host_local_map_update_batch(const tc2li_local_map_update_problem* problems, int n_problems);  /* needs no device */
/* tc2li_local_map_set_graph for n_maps mirrors: every graph is validated first (one invalid graph, or a map named twice: TC2LI_ERR_INVALID
 * with the map's number and no mirror changes), then all copies go on the stream and one wait ends the call.  Returns n_maps. */
int tc2li_local_map_set_graph_batch(tc2li_local_map* const* maps, const tc2li_map_graph* graphs, int n_maps, void* stream);
/* The sizes at which the kernels of tc2li_local_map_update_batch change path, for tests: out[0] keyframes up to which the vote counters
 * live in LDS, out[1] workgroups per problem of the point phase, out[2] threads per workgroup.  Returns 3.  Needs no device. */
int tc2li_local_map_limits(int32_t* out, int capacity);

/* The LiDAR term alone at the poses poses7 (Tcw of the window keyframes are rows lidar->pose_index): planes from the
 * window, then *residual = LidarCovisRes::ComputeError() and JacT [6W] / Hessian [(6W)^2, row-major] =
 * LidarCovisRes::ComputeJandHSE3 (SF/src/LidarRes.cc:136-186, with respect to the camera se3 increments).  JacT and
 * Hessian may be NULL.  Returns the number of planes. */
int tc2li_lidar_window_evaluate(const double* poses7, int n_poses, const tc2li_lidar_window* lidar, double* residual,
                                double* JacT, double* Hessian, void* stream);

/* Host-only: the envelope LDL^T of the inertial windows' reduced system (csrc/reduced_solve.hpp -- what tc2li_local_lvi_bundle_adjustment uses
 * with TC2LI_LVI_DEVICE_SOLVE=0 and for windows the device solve does not take), exposed so that it can be checked without a GPU.
 * Hi [n][n]: the inertial + LiDAR part in the caller's numbering (np pose unknowns first, lower triangle read); S [np][np]: the visual Schur
 * complement with its damping (lower triangle read); lambda is added to the diagonal of the other n - np unknowns.  Solves for x [n] from rhs [n];
 * returns 1, or 0 when a pivot is zero or not finite. */
int tc2li_host_reduced_solve(const double* Hi, const double* S, int n, int np, double lambda, const double* rhs, double* x);
/* The same system through the device solve (k_lvi_solve: what the inertial windows use by default), for tests of the kernel alone: returns 1,
 * 0 for a failed pivot, TC2LI_ERR_INVALID when the kernel does not take the system (more than 150 pose unknowns, no velocity / bias
 * unknowns, a velocity / bias row wider than 28). */
int tc2li_device_reduced_solve(const double* Hi, const double* S, int n, int np, double lambda, const double* rhs, double* x, void* stream);

/* Host-only stage of the LiDAR term, exposed so that it can be checked without a GPU: the planes of the window
 * (cut_voxel + recut + tras_opt, SF/src/bavoxel.cc:42-91, SF/include/bavoxel.h:492-602,723-740).  clusters receives, per
 * plane and window keyframe, 10 doubles: P00 P01 P02 P11 P12 P22 (sum x x^T), v (sum x), N in the keyframe's LiDAR
 * frame; coe the plane weights.  Returns the number of planes (which may exceed `capacity`; only that many are written). */
int tc2li_host_lidar_planes(const double* poses7, int n_poses, const tc2li_lidar_window* lidar, double* clusters, double* coe,
                            int capacity);

/* The same planes from the kernels that extract them for the windows of the batched local BA entry points (round 4: cut_voxel / recut as
 * three stable sorts of the window's points and a plane test per cell, balm_cut_kernels.hip): same layout, and the same bits as
 * tc2li_host_lidar_planes.  info (may be NULL) receives [planes, declined, root voxels, planes found].  A window outside the kernels'
 * range (more than 7 keyframes, 65535 points or 2048 planes, coordinates beyond +-1e6 voxels) is TC2LI_ERR_INVALID here; the BA entry
 * points take the host extraction for such a window. */
int tc2li_device_lidar_planes(const double* poses7, int n_poses, const tc2li_lidar_window* lidar, double* clusters, double* coe,
                              int capacity, int32_t* info);

/* Host-only stage of the extractor, exposed so that it can be checked without a GPU: keypoint distribution of
 * ORBextractor::DistributeOctTree (SF/src/ORBextractor.cc:529-753).  Candidates are (x, y, response) triples with
 * integer-valued x, y in the border-free level frame, in cv::FAST emission order; writes the retained triples in
 * the reference's output order and returns their number. */
int tc2li_host_distribute_quadtree(const float* xyr, int n, int min_x, int max_x, int min_y, int max_y, int n_target,
                                   float* out_xyr, int capacity);
/* The same distribution as one job of the device kernels the extractor runs: `threads` = 0 is the extractor's choice (k_quadtree_sorted:
 * the keys sorted once by their path through the tree, everything in LDS; a job too large for LDS falls to k_quadtree; `threads` = -1 - c starts with LDS class c), `threads` =
 * 256 / 512 / 1024 forces k_quadtree (work arrays in global memory) with that many lanes.  Same arguments, same result.  The extractor itself calls the kernel on the device-resident
 * candidates of a whole batch; this entry exists to check the kernel on arbitrary candidate sets. */
int tc2li_device_distribute_quadtree(const float* xyr, int n, int min_x, int max_x, int min_y, int max_y, int n_target, float* out_xyr,
                                     int capacity, int threads);

/* ------------------------------------------------------------------------------------------------
 * Optimizer::PoseInertialOptimizationLastKeyFrame (SF/src/Optimizer.cc:2469-2852) and PoseInertialOptimizationLastFrame
 * (:2854-3270) -- the per-frame optimiser of Tracking::TrackLocalMap once the IMU is initialised (Tracking.cc:2872 / 2877) -- for a
 * batch of independent frames: pose, velocity and biases of the frame (and, in the last-frame form, of the previous frame) against the
 * map points the frame holds (EdgeMonoOnlyPose / EdgeStereoOnlyPose, Huber sqrt(5.991) / sqrt(7.815)), EdgeInertial + EdgeGyroRW +
 * EdgeAccRW to the other state and, in the last-frame form, EdgePriorPoseImu (Huber 5) on the previous frame's mpcpi; Gauss-Newton with
 * a dense LDL^T, 4 rounds x 10 iterations, the inlier tests {12, 7.5, 5.991, 5.991} (keyframe form) or 5.991 (last-frame form) for
 * monocular edges (x 1.5 for points with mTrackDepth < 10) and {15.6, 9.8, 7.815, 7.815} for stereo edges, the recovery pass when fewer
 * than 30 inliers remain and !bRecInit; then the frame's new prior: state + Hessian (the last-frame form marginalises the previous
 * frame out of the 30 x 30 system, Optimizer::Marginalize :2087-2166; eigenvalues below 1e-12 cleared as ConstraintPoseImu does).
 * The whole optimisation of every frame runs inside one kernel launch (one workgroup per frame).
 * ---------------------------------------------------------------------------------------------- */
typedef struct tc2li_pose_imu_prior {      /* ConstraintPoseImu (SF/include/G2oTypes.h:716-740): pFrame->mpcpi */
    double Rwb[9], twb[3], vwb[3], bg[3], ba[3];
    double H[225];                         /* 15 x 15: rotation, translation, velocity, gyro bias, accelerometer bias */
} tc2li_pose_imu_prior;
typedef struct tc2li_pose_inertial_problem {
    tc2li_inertial_keyframe frame;         /* in / out: VertexPose(pFrame), VertexVelocity, VertexGyroBias, VertexAccBias */
    tc2li_inertial_keyframe other;         /* mpLastKeyFrame (constant) or, with last_frame, mpPrevFrame (in / out) */
    const tc2li_pose_imu_prior* prior;     /* pFp->mpcpi; last_frame only */
    const tc2li_preintegrated* preintegrated;     /* EdgeInertial: mpImuPreintegrated (keyframe form) / mpImuPreintegratedFrame */
    const tc2li_preintegrated* preintegrated_rw;  /* the bias-walk covariance of InfoG / InfoA: always pFrame->mpImuPreintegrated (:2645, :3049) */
    const double* Xw;                      /* [n_edges][3]: pMP->GetWorldPos() widened */
    const tc2li_ba_edge* edges;            /* u, v, u_right (< 0: monocular), inv_sigma2; point / pose are not read */
    const uint8_t* close_point;            /* [n_edges]: mTrackDepth < 10 */
    uint8_t* outlier;                      /* out [n_edges]: mvbOutlier */
    tc2li_pose_imu_prior* prior_out;       /* out (may be NULL): the frame's new mpcpi */
    int32_t n_edges, last_frame, rec_init;
    int32_t n_initial, n_bad, n_inliers, solver_failed;  /* out */
    int32_t pad_;
} tc2li_pose_inertial_problem;
/* results[f] (may be NULL) = nInitialCorrespondences - nBad, the value the reference returns.  Returns n_frames. */
int tc2li_pose_inertial_optimization_batch(tc2li_pose_inertial_problem* problems, int n_frames, const tc2li_imu_calib* calib,
                                           const tc2li_camera* cam, int32_t* results, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Measurement (bench.py; not on the hot path).
 * tc2li_profile_enable(1): every kernel launch of the library is bracketed by two HIP events on the stream it is launched on.
 * tc2li_profile_report: call when the streams are idle; writes "name<TAB>launches<TAB>total_ms<NL>" per kernel (sorted by total
 * time) into text, forgets the recorded launches and returns the bytes the whole report needs.
 * tc2li_diag_peaks: what this GPU reaches on back-to-back v_mfma_f64_16x16x4_f64 (TFLOP/s), on f64 vector FMAs (TFLOP/s) and on a
 * 1 GiB float4 copy (GB/s, read + write) -- the peaks the roofline of bench.py is priced against next to the datasheet's 8 TB/s.
 * Any pointer may be NULL.
 * ---------------------------------------------------------------------------------------------- */
int tc2li_profile_enable(int on);
int tc2li_profile_report(char* text, int capacity);
/* The environment switches the bundle-adjustment entry points would run under if called now, as one line of JSON (what a benchmark logs beside
 * its numbers): {"device_lm": 1, "device_solve": 0, "fuse_linearize": 0, "fuse_trial": 0, "lvi_device_solve": 1, "lockstep": 1, "groups": 3}.
 * Returns the number of bytes the text needs (including the terminator); writes at most `capacity`.  No reference counterpart. */
int tc2li_ba_options(char* text, int capacity);
int tc2li_diag_peaks(double* mfma_f64_tflops, double* fma_f64_tflops, double* hbm_copy_gbps);
/* The shader clock (GHz) the chip holds inside the two arithmetic loops of tc2li_diag_peaks, from s_memtime against the constant 100 MHz
 * counter: the data sheet's 78.6 TFLOP/s of f64 matrix / vector arithmetic assume 2.4 GHz. */
int tc2li_diag_clocks(double* mfma_loop_ghz, double* fma_loop_ghz);

/* ------------------------------------------------------------------------------------------------
 * ORB vocabulary -- DBoW2's TemplatedVocabulary<FORB::TDescriptor, FORB> (ORBVocabulary, SF/Thirdparty/DBoW2/DBoW2/
 * TemplatedVocabulary.h), the transform behind Frame::ComputeBoW / KeyFrame::ComputeBoW (SF/src/Frame.cc:768-775,
 * SF/src/KeyFrame.cc:110-119) and ORBmatcher::SearchByBoW(KeyFrame*, Frame&) (SF/src/ORBmatcher.cc:232-434).
 * Loading and readback are host logic and work without a GPU; the device copy of a vocabulary is made on the first call that
 * computes with it (once per handle, thread-safe: tracking and local mapping share one vocabulary), on the device current then.
 * ---------------------------------------------------------------------------------------------- */
typedef struct tc2li_vocabulary tc2li_vocabulary;

/* TemplatedVocabulary::loadFromTextFile (TemplatedVocabulary.h:1350-1436; System.cc:126, 148 load ORBvoc.txt at start-up).  The first
 * line is "k L scoring weighting" (0 <= k <= 20, 1 <= L <= 10, 0 <= scoring <= 5, 0 <= weighting <= 3), every further line one node in
 * id order from 1 (the root, node 0, has no line): "parent isLeaf d0 .. d31 weight", separated by any whitespace ('\r' included);
 * descriptor bytes are read as int and cast to unsigned char (FORB::fromString), the weight as a double (strtod: the value operator>>
 * gives).  Children are appended to their parent in line order, word ids numbered in the order of the lines with isLeaf > 0.
 * Blank lines are skipped.  The reference turns the empty line after saveToTextFile's final endl into one more node built from
 * uninitialised pid / nIsLeaf (undefined behaviour), and spins forever on a missing file; here both are defined.  Rejected with
 * TC2LI_ERR_INVALID, the file's line named in tc2li_last_error(): an unreadable file, a bad header, a line with fewer than 35 fields or
 * a field that is not a number, a parent that is not an earlier node, a node flagged as a word that receives children, a childless
 * node not flagged as a word (the descent's leaf test is children.empty(), :340, so every leaf is a word). */
int tc2li_vocabulary_load_text(const char* path, tc2li_vocabulary** out);
/* The same content from arrays in file order: node i + 1 of n_nodes has parent[i], is_leaf[i], descriptors[i][32], weights[i].
 * Same checks (the message names the node). */
int tc2li_vocabulary_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent, const int32_t* is_leaf,
                            const uint8_t* descriptors, const double* weights, tc2li_vocabulary** out);
/* info[6] = k, L, scoring, weighting, nodes (the root included), words.  Returns 6. */
int tc2li_vocabulary_info(const tc2li_vocabulary* voc, int32_t* info);
/* Host readback per node in reference numbering (root first; arrays [nodes], NULL skips one): parent (-1 for the root), word id
 * (-1 for a node that is not a word; the reference's default is 0), descriptor [32], weight (the root's 0).  Returns the node count. */
int tc2li_vocabulary_nodes(const tc2li_vocabulary* voc, int32_t* parent, int32_t* word_id, uint8_t* descriptors, double* weights);
void tc2li_vocabulary_destroy(tc2li_vocabulary* voc);

/* Output of the transform of a batch (caller arrays).  Frame f owns the slot range [base_f, base_f + n_f) of every per-descriptor
 * array, base_f = desc_offsets[f] (tc2li_vocabulary_transform_batch) or f * capacity (tc2li_orb_compute_bow_batch):
 *   word / node       per descriptor i: word id and the node recorded for the FeatureVector, -1 for a stopped feature (weight <= 0);
 *   n_words[f]        entries of frame f's mBowVec: bow_word[base_f ..] word ids ascending, bow_value[base_f ..] their values;
 *   n_nodes[f]        entries of frame f's mFeatVec: fv_node[base_f ..] node ids ascending, fv_offset[base_f + f ..] (n_nodes[f] + 1
 *                     entries, from 0) and fv_index[base_f ..] the feature indices of every node in feature order.
 * fv_offset holds (total slots + n_frames) entries.  A tc2li_keyframe_view with n_nodes = n_nodes[f], fv_node = fv_node + base_f,
 * fv_offset = fv_offset + base_f + f and fv_index = fv_index + base_f is frame f's FeatureVector, without copying.  Slots beyond the
 * counts read -1 (bow_value 0). */
typedef struct tc2li_bow_out {
    int32_t* word;
    int32_t* node;
    int32_t* n_words;
    int32_t* bow_word;
    double* bow_value;
    int32_t* n_nodes;
    int32_t* fv_node;
    int32_t* fv_offset;
    int32_t* fv_index;
} tc2li_bow_out;

/* TemplatedVocabulary::transform(features, BowVector&, FeatureVector&, levelsup) (TemplatedVocabulary.h:1139-1206, per feature
 * :1230-1271) for n_frames frames of host descriptors: frame f's are rows desc_offsets[f] .. desc_offsets[f + 1] of
 * descriptors [..][32] (desc_offsets [n_frames + 1], desc_offsets[0] = 0).  ComputeBoW passes levelsup = 4.  Bit for bit the
 * reference: the descent takes at every level the first child of least FORB::distance and stops at a node without children; the
 * node recorded is the one chosen at level L - levelsup (L the header's), the root (0) when L - levelsup <= 0 -- and the leaf itself
 * when the leaf lies above that level, where the reference leaves nid uninitialised (undefined behaviour).  A word's value is its weight
 * added once per feature in feature order (TF, TF_IDF) or its weight (IDF, BINARY); L1 (L1_NORM, CHI_SQUARE, KL, BHATTACHARYYA) or L2
 * (L2_NORM) normalisation in one pass in ascending word order, applied when the norm is > 0; DOT_PRODUCT with TF / TF_IDF divides by
 * the number of words instead.  Returns n_frames. */
int tc2li_vocabulary_transform_batch(tc2li_vocabulary* voc, int n_frames, const uint8_t* descriptors, const int32_t* desc_offsets,
                                     int levelsup, const tc2li_bow_out* out, void* stream);
/* The same for the device-resident features of frames: frame f is image 2f of the handle's last tc2li_orb_extract_batch call (lapping
 * area {0,0}, as the tracking batches), feature i its keypoint i; its slots start at f * capacity.  The descriptors never leave the
 * device.  Returns n_frames. */
int tc2li_orb_compute_bow_batch(tc2li_orb* orb, tc2li_vocabulary* voc, int n_frames, int levelsup, int capacity, const tc2li_bow_out* out,
                                void* stream);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vpMapPointMatches) (SF/src/ORBmatcher.cc:232-434; ORBmatcher(0.7, true) in
 * Tracking::TrackReferenceKeyFrame, SF/src/Tracking.cc:2603-2662, (0.75, true) in relocalisation :3517) for a batch of pairs.
 * keyframe: n, keys (angle), descriptors, has_point (= pMP && !pMP->isBad()) and its FeatureVector (n_nodes, fv_*); frame: n, keys,
 * descriptors and its FeatureVector (has_point, u_right, depth, pose7 are not read).  Common nodes in ascending order; within a node the
 * keyframe's features in order, the frame's features not yet matched; best and second-best distance (both from 256, strict <);
 * accepted when best <= TH_LOW (50) and best < nn_ratio * second (float); with check_orientation the rotation histogram (30 bins,
 * bin = roundf(rot / 30), so only 0..12 occur) and ComputeThreeMaxima (:2021-2062).  The right-camera branch (F.Nleft != -1) is not
 * built (pinhole stereo).  At most 4096 frame features per node (TC2LI_ERR_CAPACITY).  Out: kf_keypoint_of_keypoint [n_pairs][capacity]
 * = the keyframe keypoint whose map point frame keypoint i now holds (vpMapPointMatches[i]) or -1, n_matches[p].  Returns n_pairs. */
typedef struct tc2li_bow_pair {
    tc2li_keyframe_view keyframe;
    tc2li_keyframe_view frame;
    float nn_ratio;                /* mfNNratio */
    int32_t check_orientation;     /* mbCheckOrientation */
} tc2li_bow_pair;
int tc2li_search_by_bow_batch(const tc2li_bow_pair* pairs, int n_pairs, int capacity, int32_t* kf_keypoint_of_keypoint, int32_t* n_matches,
                              void* stream);

/* Tracking::TrackReferenceKeyFrame (SF/src/Tracking.cc:2603-2662), data path only, for a batch of independent frames whose features are
 * device-resident -- the fallback of TrackWithMotionModel (Tracking.cc:2032, 2042, 2147) and the first frames after initialisation.
 * Frame f is image 2f of the handle's last tc2li_orb_extract_batch call (lapping area {0,0}); keypoints ([2*n_frames][capacity], the
 * host copy of that call's output: the device-resident copy is what is read) and u_right ([n_frames][capacity]) as for
 * tc2li_track_motion_model_batch.  One stream, one staging upload: the frame's ComputeBoW (levelsup 4), ORBmatcher(0.7, true).SearchByBoW
 * against refs[f] (as tc2li_search_by_bow_batch), and with at least 15 matches -- decided on the device -- SetPose(mLastFrame.GetPose()),
 * Optimizer::PoseOptimization over every keypoint that now holds a point (keypoint order, stereo when uRight >= 0, invSigma2[octave]; the
 * kernel of tc2li_track_motion_model_batch), outliers discarded, nmatchesMap = inliers whose point has Observations() > 0.
 * At most 4096 keypoints per frame.  Out: poses7 [n_frames][7] (double: the optimised pose rounded through float, the last pose when
 * failed), kf_keypoint_of_keypoint [n_frames][capacity] = the reference keyframe keypoint whose map point keypoint i holds after the
 * discard, or -1 (every entry -1 when failed), n_matches[f] = SearchByBoW's result, n_inliers[f] = PoseOptimization's result or -1 with
 * fewer than 15 matches, n_matches_map[f].  bow (may be NULL) receives the frames' BowVector / FeatureVector as
 * tc2li_orb_compute_bow_batch gives them (the Frame keeps them; a new KeyFrame copies them).  The sensor rule (:2658-2661) and the
 * MapPoint flags stay with the caller.  Returns n_frames. */
typedef struct tc2li_reference_keyframe {
    tc2li_keyframe_view kf;        /* mpReferenceKF: n, keys (angle), descriptors, has_point (pMP && !pMP->isBad()), n_nodes / fv_* */
    const float* Xw;               /* [n][3] GetWorldPos() of the point of every keypoint slot that has one */
    const uint8_t* observed;       /* [n] pMP->Observations() > 0 */
    float last_pose7[7];           /* mLastFrame.GetPose() */
    float pad_;
} tc2li_reference_keyframe;
int tc2li_track_reference_keyframe_batch(tc2li_orb* orb, tc2li_vocabulary* voc, int n_frames, const tc2li_keypoint* keypoints,
                                         const float* u_right, int capacity, const tc2li_reference_keyframe* refs, const tc2li_camera* cam,
                                         double* poses7, int32_t* kf_keypoint_of_keypoint, int32_t* n_matches, int32_t* n_inliers,
                                         int32_t* n_matches_map, const tc2li_bow_out* bow, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Relocalisation -- the keyframe database and DetectRelocalizationCandidates, the stage of Tracking::Relocalization
 * (SF/src/Tracking.cc:3478-3646) between the frame's ComputeBoW (tc2li_orb_compute_bow_batch) and SearchByBoW
 * (tc2li_search_by_bow_batch with nn_ratio 0.75).  MLPnPsolver stays the reference's host code.
 * ---------------------------------------------------------------------------------------------- */

/* One BowVector: n entries, word ids strictly ascending (std::map order), their values. */
typedef struct tc2li_bow_vector {
    const int32_t* word;
    const double* value;
    int32_t n;
    int32_t pad_;
} tc2li_bow_vector;

/* TemplatedVocabulary::score(v1, v2) (TemplatedVocabulary.h:1274-1280 -> SF/Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-311) for n_pairs
 * pairs, scores[p] = score(v1[p], v2[p]) in double, with the scoring type of the vocabulary (tc2li_vocabulary_info).  Bit for bit the
 * reference for L1_NORM, L2_NORM, CHI_SQUARE, BHATTACHARYYA and DOT_PRODUCT: the terms of the common words are added one at a time in
 * ascending word order into a double that starts at 0 (vi is v1's value, wi is v2's), then the closing step of the type (-score / 2;
 * score >= 1 ? 1 : 1 - sqrt(1 - score); 2 * score; none; none).  CHI_SQUARE skips a word with vi + wi == 0.  Two vectors without a common
 * word score what the closing step makes of 0 (L1_NORM: -0.0).  KL is rejected with TC2LI_ERR_INVALID: it calls log(), whose device
 * result is not the host library's to the last bit.  Word ids not strictly ascending or outside the vocabulary: TC2LI_ERR_INVALID; more
 * than 4096 words in a vector: TC2LI_ERR_CAPACITY.  Returns n_pairs. */
int tc2li_vocabulary_score_batch(tc2li_vocabulary* voc, int n_pairs, const tc2li_bow_vector* v1, const tc2li_bow_vector* v2, double* scores,
                                 void* stream);

/* KeyFrameDatabase (SF/src/KeyFrameDatabase.cc:40-107), bound to one vocabulary (the constructor's argument, :41-45), which must outlive
 * it.  Host logic that works without a GPU; the device copy is brought up to date by the first query after a change.  Instead of the
 * reference's inverted file (a std::list<KeyFrame*> per word) the handle keeps the keyframes' BowVectors as rows of one pool, with a
 * sequence number per tc2li_keyframe_db_add call: every word's list is in the order of the add calls, so the order in which a query
 * meets the keyframes (lKFsSharingWords) is the order by (smallest word shared with the frame, sequence number).  Calls on one handle
 * are serialised by a mutex (mMutex).  At most 4096 live keyframes and 4096 words per keyframe (TC2LI_ERR_CAPACITY). */
typedef struct tc2li_keyframe_db tc2li_keyframe_db;
int tc2li_keyframe_db_create(const tc2li_vocabulary* voc, tc2li_keyframe_db** out);
void tc2li_keyframe_db_destroy(tc2li_keyframe_db* db);
/* KeyFrameDatabase::add (:48-54): kf_id is the keyframe's mnId (>= 0, unique among the live entries: a live duplicate is TC2LI_ERR_INVALID,
 * as are word ids not strictly ascending or outside the vocabulary), map_id its GetMap(), the BowVector its mBowVec.  The entry takes the
 * handle's next sequence number, has no covisibility list and the score state 0.0f (the reference leaves KeyFrame::mRelocScore
 * uninitialised, KeyFrame.h:349).  Returns the sequence number. */
int tc2li_keyframe_db_add(tc2li_keyframe_db* db, int32_t kf_id, int32_t map_id, int n_words, const int32_t* bow_word, const double* bow_value);
/* KeyFrameDatabase::erase (:56-75; KeyFrame::SetBadFlag calls it).  An unknown id is a no-op like the reference's loop.  Returns 1 when an
 * entry was erased, 0 otherwise.  The dead rows leave the pool when they pass half of it. */
int tc2li_keyframe_db_erase(tc2li_keyframe_db* db, int32_t kf_id);
/* KeyFrameDatabase::clear (:77-81) and clearMap (:83-107): every entry / every entry of map_id.  Returns the number of entries erased. */
int tc2li_keyframe_db_clear(tc2li_keyframe_db* db);
int tc2li_keyframe_db_clear_map(tc2li_keyframe_db* db, int32_t map_id);
/* Live entries. */
int tc2li_keyframe_db_size(const tc2li_keyframe_db* db);
/* pKF->GetBestCovisibilityKeyFrames(10) of entry kf_id as the caller's graph has it now (KeyFrameDatabase.cc:808): n <= 10 ids in the
 * reference's order, replacing the entry's list.  Ids that are not live entries when a query runs are skipped by it, as a neighbour that
 * shares no word with the frame is (:816).  TC2LI_ERR_INVALID for n > 10 or an unknown kf_id.  Returns n. */
int tc2li_keyframe_db_set_covisibility(tc2li_keyframe_db* db, int32_t kf_id, int n, const int32_t* neighbour_ids);
/* Host readback of the live entries in sequence order (arrays [capacity], NULL skips one): kf_id, map_id, sequence number and the score
 * state (mRelocScore: what the last query that scored the entry left).  Returns the number of live entries; TC2LI_ERR_CAPACITY when
 * capacity is smaller. */
int tc2li_keyframe_db_entries(const tc2li_keyframe_db* db, int capacity, int32_t* kf_id, int32_t* map_id, int32_t* sequence, float* score);

/* One query of DetectRelocalizationCandidates: the database, pMap as its map_id, and F->mBowVec as tc2li_bow_out gives it. */
typedef struct tc2li_reloc_query {
    tc2li_keyframe_db* db;
    int32_t map_id;
    int32_t n_words;
    const int32_t* bow_word;
    const double* bow_value;
} tc2li_reloc_query;
/* Optional output: the scored list of every query in lScoreAndMatch order (KeyFrameDatabase.cc:780-830), arrays [n_queries][capacity]:
 * the keyframe, mnRelocWords, si, accScore and pBestKF of every entry; n_scored [n_queries]. */
typedef struct tc2li_reloc_scored {
    int32_t capacity;
    int32_t pad_;
    int32_t* n_scored;
    int32_t* kf_id;
    int32_t* words;
    float* si;
    float* acc_score;
    int32_t* best_kf_id;
} tc2li_reloc_scored;
/* KeyFrameDatabase::DetectRelocalizationCandidates(F, pMap) (:742-854) for n_queries <= 512 queries, each against its own database (the
 * queries of one database depend on each other through the score state: the same handle twice is TC2LI_ERR_INVALID).  Line for line:
 * mnRelocWords = words the keyframe shares with the frame, keyframes without one take no part (:750-768); minCommonWords =
 * (int)(maxCommonWords * 0.8f) (:778); for the keyframes with more words than that, in lKFsSharingWords order, si = (float)score(F, KF),
 * stored as the keyframe's score state (:785-796); accScore in float over the keyframe's covisibility list in its order, a neighbour
 * counting iff it is a live entry that shares a word with this frame, with its STORED score -- this query's si if it passed the word
 * gate, otherwise what an earlier query left, 0.0f on a fresh entry (:805-830); kept are the entries with accScore > 0.75f * bestAccScore
 * whose best keyframe has the query's map_id, first occurrence of each best keyframe, in list order (:833-851).
 * Out: n_candidates [n_queries], candidates [n_queries][capacity] kf_ids, -1 beyond the count.  TC2LI_ERR_CAPACITY when a list (or a
 * scored list) does not fit (the score states have been updated then), for a frame with more than 4096 words or more than 512 queries.
 * The databases of one call share the scoring type of their vocabularies (TC2LI_ERR_INVALID otherwise); KL vocabularies are rejected as in
 * tc2li_vocabulary_score_batch.  Returns n_queries. */
int tc2li_detect_relocalization_candidates_batch(const tc2li_reloc_query* queries, int n_queries, int capacity, int32_t* n_candidates,
                                                 int32_t* candidates, const tc2li_reloc_scored* scored, void* stream);

/* One item of ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, th, ORBdist)
 * (SF/src/ORBmatcher.cc:1898-2019; Tracking::Relocalization calls it with (10, 100) and (3, 64), SF/src/Tracking.cc:3578, 3594): the frame
 * and the candidate keyframe's points in keypoint order (vpMPs = pKF->GetMapPointMatches()). */
typedef struct tc2li_projection_keyframe_item {
    int32_t n;                         /* CurrentFrame.N (at most 3072, the matcher's limit) */
    int32_t n_points;                  /* vpMPs.size() */
    const tc2li_keypoint* keys;        /* CurrentFrame.mvKeysUn */
    const uint8_t* descriptors;        /* CurrentFrame.mDescriptors, [n][32] */
    const uint8_t* held;               /* [n] CurrentFrame.mvpMapPoints[i] != NULL: any held point blocks the keypoint (:1961) */
    float pose7[7];                    /* CurrentFrame.GetPose(): qx qy qz qw tx ty tz of Tcw */
    float bounds[4];                   /* mnMinX, mnMaxX, mnMinY, mnMaxY */
    float pad_;
    const uint8_t* has_point;          /* [n_points] pMP && !pMP->isBad() */
    const uint8_t* found;              /* [n_points] sAlreadyFound.count(pMP) */
    const float* Xw;                   /* [n_points][3] pMP->GetWorldPos() */
    const uint8_t* point_descriptors;  /* [n_points][32] pMP->GetDescriptor() -- the map point's, not the keyframe keypoint's */
    const float* min_distance;         /* [n_points] GetMinDistanceInvariance() */
    const float* max_distance;         /* [n_points] GetMaxDistanceInvariance() */
    const float* max_distance_raw;     /* [n_points] mfMaxDistance (MapPoint::PredictScale) */
    const float* angle;                /* [n_points] pKF->mvKeysUn[i].angle */
} tc2li_projection_keyframe_item;
/* The overload for a batch of items with one (th, ORBdist, mbCheckOrientation).  Per keyframe keypoint in order, for a point that is
 * there, not bad and not in sAlreadyFound: projection with the frame's pose (no depth-sign and no viewing-cosine test), the image
 * bounds, dist3D = |Xw - Ow| with Ow = Tcw.inverse().translation() inside [min_distance, max_distance], PredictScale(dist3D,
 * &CurrentFrame) with log_scale_factor = mfLogScaleFactor and n_levels, the window th * scale_factors[level] over the levels level - 1 ..
 * level + 1 (handed to GetFeaturesInArea unclamped), among the keypoints that hold no point the one of least descriptor distance (from
 * 256, strict <, first wins), accepted when bestDist <= orb_dist; a matched keypoint blocks later points.  With check_orientation the
 * rotation histogram (bin = round(rot * (1.0f / 30)), 30 -> 0) and ComputeThreeMaxima remove the matches outside the three maxima.
 * Out: kf_keypoint_of_keypoint [n_items][capacity] = the keyframe keypoint whose point the frame keypoint received, -1 elsewhere (held
 * keypoints included), n_matches [n_items] after the removals.  Returns n_items. */
int tc2li_search_by_projection_keyframe_batch(const tc2li_projection_keyframe_item* items, int n_items, const float* cam4,
                                              const float* scale_factors, int n_levels, float log_scale_factor, float th, int orb_dist,
                                              int check_orientation, int capacity, int32_t* kf_keypoint_of_keypoint, int32_t* n_matches,
                                              void* stream);

/* One hypothesis of the refinement ladder: a frame, a candidate keyframe, the pose MLPnPsolver::iterate returned for the pair and its
 * inliers among SearchByBoW's matches. */
typedef struct tc2li_reloc_hypothesis {
    int32_t frame_index;               /* the frame is image 2 * frame_index of the handle's last tc2li_orb_extract_batch call */
    int32_t n_points;                  /* keypoints of the candidate keyframe (vpCandidateKFs[i]) */
    const uint8_t* has_point;          /* the candidate as in tc2li_projection_keyframe_item */
    const float* Xw;
    const uint8_t* point_descriptors;
    const float* min_distance;
    const float* max_distance;
    const float* max_distance_raw;
    const float* angle;
    const int32_t* match;              /* [keypoints of the frame] the keyframe keypoint vvpMapPointMatches[i][j] names, or -1 */
    const uint8_t* inlier;             /* [keypoints of the frame] vbInliers[j] */
    float pose7[7];                    /* Tcw of the PnP solution: qx qy qz qw tx ty tz */
    float pad_;
} tc2li_reloc_hypothesis;
enum tc2li_reloc_status {
    TC2LI_RELOC_OPT1 = 1,              /* the first PoseOptimization ran (always) */
    TC2LI_RELOC_REJECTED = 2,          /* nGood < 10 after it: the reference's `continue` */
    TC2LI_RELOC_SEARCH1 = 4,           /* nGood < 50: SearchByProjection(.., 10, 100) ran */
    TC2LI_RELOC_OPT2 = 8,              /* nadditional + nGood >= 50: the second PoseOptimization ran */
    TC2LI_RELOC_SEARCH2 = 16,          /* 30 < nGood < 50: SearchByProjection(.., 3, 64) ran */
    TC2LI_RELOC_OPT3 = 32,             /* nGood + nadditional >= 50: the third PoseOptimization ran */
    TC2LI_RELOC_SUCCESS = 64           /* nGood >= 50 at the end */
};
/* What Tracking::Relocalization does with a PnP pose (SF/src/Tracking.cc:3562-3631), for n_hyps independent hypotheses on the device-resident
 * features of the last tc2li_orb_extract_batch call (lapping area {0,0}; n_frames frames, u_right [n_frames][capacity] as for
 * tc2li_track_motion_model_batch); several hypotheses may name one frame, each works on its own copy of the frame's map points.  One stream,
 * one staging upload, every branch decided on the device:
 *   mvpMapPoints = match where inlier, sFound = those points; PoseOptimization (the kernel of tc2li_track_motion_model_batch: one edge per
 *   keypoint that holds a point, keypoint order, stereo when uRight >= 0); nGood < 10: rejected, the frame stays as PoseOptimization left it;
 *   outliers discarded; if nGood < 50: ORBmatcher(0.9, true).SearchByProjection(F, pKF, sFound, 10, 100)
 *   (tc2li_search_by_projection_keyframe_batch); if nadditional + nGood >= 50: PoseOptimization -- no discard after this one --; if then
 *   30 < nGood < 50: sFound = every point the frame holds (flagged outliers included), SearchByProjection(.., 3, 64); if nGood +
 *   nadditional >= 50: PoseOptimization and discard.  Success iff nGood >= 50.
 * Out per hypothesis: status (tc2li_reloc_status bits), n_good, n_additional [2] (0 for a search that did not run), poses7 [3][7] the pose
 * after each PoseOptimization that ran (double, rounded through float as Frame::SetPose stores it; zeros otherwise),
 * kf_keypoint_of_keypoint [capacity] the frame's map points at the end as keyframe keypoints, outlier [capacity] mvbOutlier of the last
 * PoseOptimization that ran.  The MapPoint flags and mnLastRelocFrameId stay with the caller.  Returns n_hyps. */
int tc2li_relocalization_refine_batch(tc2li_orb* orb, const tc2li_reloc_hypothesis* hyps, int n_hyps, int n_frames, const float* u_right,
                                      int capacity, const tc2li_camera* cam, int32_t* status, int32_t* n_good, int32_t* n_additional,
                                      double* poses7, int32_t* kf_keypoint_of_keypoint, uint8_t* outlier, void* stream);

/* ---- MLPnP RANSAC: the PnP stage of Tracking::Relocalization (SF/src/MLPnPsolver.cpp, SF/include/MLPnPsolver.h) -------------------------
 * The solver is a function of its inputs once the caller hands in the rand() values it would have drawn: DUtils::Random::RandomInt
 * (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) is a pure function of rand()'s return value. */
/* SetRansacParameters' arguments (MLPnPsolver.cpp:205; (0.99, 10, 300, 6, 0.5, 5.991) at SF/src/Tracking.cc:3526).  min_set must be 6. */
typedef struct tc2li_mlpnp_params {
    double probability;
    int32_t min_inliers, max_iterations, min_set;
    float epsilon, th2;
    int32_t pad_;
} tc2li_mlpnp_params;
/* What a solver carries from one iterate() call to the next, besides the best flags: mnIterations, mnBestInliers, mBestTcw (rows 0-2,
 * row-major 3 x 4).  All zero = a fresh solver. */
typedef struct tc2li_mlpnp_state {
    int32_t iterations, best_inliers;
    float best_Tcw[12];
} tc2li_mlpnp_state;
/* One solver and one iterate() call on it.  The constructor (MLPnPsolver.cpp:35-77) takes keypoint i when match[i] >= 0: mvP2D = (x, y),
 * mvSigma2 = level_sigma2[octave], bearing = ((x - cx) / fx, (y - cy) / fy, 1) in float (not of unit length), mvP3Dw = Xw[match[i]]
 * widened, mvKeyPointIndices = i.  All pointers are host memory. */
typedef struct tc2li_mlpnp_problem {
    const tc2li_keypoint* keys;        /* mvKeysUn of the frame */
    const int32_t* match;              /* [n_keypoints] index into Xw or -1: vpMapPointMatches with bad points already removed */
    const float* Xw;                   /* [n_points][3] */
    const uint32_t* draws;             /* rand() return values, 6 per iteration (:110), consumed in order */
    tc2li_mlpnp_state* state;          /* in / out */
    uint8_t* best_inlier;              /* in / out [n_keypoints]: mvbBestInliers per frame keypoint; zeros for a fresh solver */
    int32_t n_keypoints, n_points, n_draws;
    int32_t n_iterations;              /* iterate()'s argument: 5 at Tracking.cc:3552 */
} tc2li_mlpnp_problem;
/* SetRansacParameters (:205-240) for N correspondences: min_inliers = max(int(N * epsilon), min_inliers, min_set), epsilon raised to
 * (float)min_inliers / N, max_iterations = clamp(ceil(log(1 - p) / log(1 - pow(epsilon, 3))), 1, max_iterations), 1 when min_inliers == N.
 * Host arithmetic (libm).  Returns 0. */
int tc2li_mlpnp_iterations(int n_correspondences, const tc2li_mlpnp_params* params, int32_t* min_inliers, int32_t* max_iterations);
/* One MLPnPsolver::iterate(n_iterations, ..) call (:80-203) per problem, all problems at once on the device.  Kept as written:
 *   N < min_inliers: no_more, not found (:86-90).  The loop runs while state.iterations < max_iterations OR fewer than n_iterations
 *   passes were made (:95), so a fresh solver runs up to max(max_iterations, n_iterations) iterations in its first call.  Each draws six
 *   correspondences without replacement (:108-120), computePose (:336-638: null spaces, planar test on the uncentred second moment,
 *   the eigenvector of A^T A, nearest rotation, direction test, rot2rodrigues, at most 5 Gauss-Newton steps), CheckInliers (:242-273,
 *   mixed float / double).  A count >= min_inliers that beats the best replaces it (:149-167).  Refine() (:275-333) throws its N-point
 *   solve away and re-tests the iteration's own pose, so an iteration whose count is > min_inliers returns with its own pose and flags.
 *   When the loop ends with state.iterations >= max_iterations: no_more, and the best is returned if it reaches min_inliers (:185-200).
 * A call that may run K = max(max_iterations - state.iterations, n_iterations) iterations needs 6 K draws; unused draws are not consumed
 * (an early return after j iterations has used the first 6 j: the caller keeps the rest for the next call to stay on the reference's
 * sequence).  TC2LI_ERR_INVALID before any launch for min_set != 6, too few draws, a draw above RAND_MAX = 2^31 - 1, a match outside
 * [-1, n_points), an octave outside [0, n_levels); TC2LI_ERR_CAPACITY for n_keypoints > capacity.
 * Out per problem: found (the return value), no_more (bNoMore), n_inliers, inlier [capacity] per frame keypoint (vbInliers, zeros
 * beyond), pose7 = Tcw as qx qy qz qw tx ty tz in float -- what tc2li_reloc_hypothesis.pose7 takes --, identity when not found (:81);
 * Rt12 (may be NULL) the double [R | t] row-major 3 x 4 the pose was rounded from (the widened mBestTcw when the best of an earlier
 * call is returned).  state and best_inlier are updated.  found, no_more, n_inliers may be NULL.  Returns n_problems. */
int tc2li_mlpnp_ransac_batch(const tc2li_mlpnp_problem* problems, int n_problems, const tc2li_mlpnp_params* params,
                             const float* level_sigma2, int n_levels, const tc2li_camera* cam, int32_t* found, int32_t* no_more,
                             int32_t* n_inliers, float* pose7, double* Rt12, uint8_t* inlier, int capacity, void* stream);
/* The same arithmetic on the CPU (the kernels and this entry share mlpnp_math.hpp); needs no device. */
int tc2li_host_mlpnp_ransac_batch(const tc2li_mlpnp_problem* problems, int n_problems, const tc2li_mlpnp_params* params,
                                  const float* level_sigma2, int n_levels, const tc2li_camera* cam, int32_t* found, int32_t* no_more,
                                  int32_t* n_inliers, float* pose7, double* Rt12, uint8_t* inlier, int capacity);

/* ---- local mapping: culling (SF/src/LocalMapping.cc:360-399 MapPointCulling, :913-1065 KeyFrameCulling) -----------------------------------
 * The two culling stages of LocalMapping::Run on the flat graph (matches per keyframe, observations per point).  The library returns the
 * decisions; the caller applies them to its own objects in list order (INTEGRATION.md "KeyFrameCulling / MapPointCulling").  Rig: pinhole
 * stereo, NLeft == -1, mpCamera2 == nullptr; the NLeft != -1 branches of :979-1003 are not covered.  mbMonocular is false, so the
 * redundancy threshold is 0.9f without IMU and 0.5f with (:923-929). */
enum tc2li_cull_verdict {
    TC2LI_CULL_SKIPPED = -1,           /* the init keyframe or a bad one (:955) */
    TC2LI_CULL_NOT_VISITED = -2,       /* after the break of :1060 */
    TC2LI_CULL_REDUNDANT = 1,          /* otherwise a mask: nRedundantObservations > redundant_th * nMPs (:1021) */
    TC2LI_CULL_SET_BAD = 2,            /* SetBadFlag() was called (:1042, :1051, :1057) */
    TC2LI_CULL_MERGED = 4,             /* MergePrevious and the relink of mPrevKF / mNextKF before it (:1037-1041, :1046-1050) */
    TC2LI_CULL_DEFERRED = 8            /* mbNotErase: SetBadFlag only set mbToBeErased (SF/src/KeyFrame.cc:593-597), nothing was erased */
};
/* One call of LocalMapping::KeyFrameCulling.  All pointers are host memory, the arrays are copied by the call; indices are rows of the
 * problem's own tables.
 *   keyframes (n_keyframes rows, every keyframe that appears anywhere in the problem):
 *     kf_flags  bit 0 isBad(), bit 1 mnId == GetMap()->GetInitKFid(), bit 2 mbNotErase;  kf_id mnId;  kf_prev / kf_next mPrevKF / mNextKF
 *     (-1 = none);  kf_time mTimeStamp;  kf_imu_pos [n][3] GetImuPosition();  kf_th_depth mThDepth
 *   slots: CSR slot_offsets [n_keyframes + 1] (keyframes outside `local` may have empty rows); slot_point mvpMapPoints[i] (-1 = NULL),
 *     slot_depth mvDepth[i], slot_octave mvKeysUn[i].octave
 *   local [n_local]: GetVectorCovisibleKeyFrames() after UpdateBestCovisibles() (:920-921), in that order
 *   points (n_points rows): point_bad isBad(); point_nobs Observations() = nObs, which counts a stereo observation twice; CSR obs_offsets
 *     [n_points + 1]; obs_kf the observing keyframe, obs_octave mvKeysUn[leftIndex].octave there, obs_weight 2 if mvuRight[leftIndex] >= 0
 *     else 1: what MapPoint::EraseObservation subtracts (SF/src/MapPoint.cc:187-192).  THE ORDER OF A POINT'S OBSERVATIONS MATTERS TO NO
 *     RESULT (the early break of :1008 only ends a count that has already passed the threshold).  A keyframe appears at most once in a
 *     row (mObservations is a map); if it appears more often, every such entry is erased with it.  A bad point holds no observations
 *     (MapPoint.cc:233): the row of a point that is bad on entry is ignored.
 *   scalars: inertial mbInertial; imu_initialized mpAtlas->isImuInitialized(); inertial_ba2 GetIniertialBA2(); abort_ba mbAbortBA AS IT
 *     IS WHEN THE CALL IS MADE -- the reference reads it live at :1060, where it only bounds the work after 20 keyframes; this snapshot is a
 *     deviation --; keyframes_in_map mpAtlas->KeyFramesInMap(); current_id mpCurrentKeyFrame->mnId; last_id the last_ID of :935-946 (at
 *     most 21 hops along mPrevKF from the current keyframe; read only when inertial).
 * Out: verdict [n_local] (tc2li_cull_verdict), n_mps / n_redundant [n_local] nMPs and nRedundantObservations as they were when the
 * keyframe was decided (untouched where verdict < 0), n_visited [1] the entries of local the loop reached, and optionally (may be NULL)
 * point_bad_after / point_nobs_after [n_points]: the simulated end state of isBad() and nObs. */
typedef struct tc2li_culling_problem {
    const uint8_t* kf_flags;
    const int64_t* kf_id;
    const int32_t* kf_prev;
    const int32_t* kf_next;
    const double* kf_time;
    const float* kf_imu_pos;
    const float* kf_th_depth;
    const int32_t* slot_offsets;
    const int32_t* slot_point;
    const float* slot_depth;
    const int8_t* slot_octave;
    const int32_t* local;
    const uint8_t* point_bad;
    const int32_t* point_nobs;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int8_t* obs_octave;
    const uint8_t* obs_weight;
    int32_t* verdict;
    int32_t* n_mps;
    int32_t* n_redundant;
    int32_t* n_visited;
    uint8_t* point_bad_after;
    int32_t* point_nobs_after;
    int64_t current_id, last_id;
    int32_t n_keyframes, n_local, n_points, keyframes_in_map;
    uint8_t inertial, imu_initialized, inertial_ba2, abort_ba;
    int32_t pad_;
} tc2li_culling_problem;
/* LocalMapping::KeyFrameCulling (:913-1065) for n_problems independent calls (one per sequence) at once on the device, with the side
 * effects of every cull simulated so that the later verdicts of the same call are the reference's:
 *   walk local in order, count incremented first (:952); the init keyframe and bad keyframes are skipped (:955) -- this continue and the
 *   inertial ones below jump over the closing test (count > 20 && abort_ba) || count > 100 (:1060), which is reached only at the end of an
 *   iteration that did not continue.  Per slot with a non-NULL, non-bad point: dropped if depth > th_depth || depth < 0 (:972), otherwise
 *   nMPs++; if Observations() > 3 (:977) the point's live observations in OTHER keyframes with octave <= own octave + 1 are counted
 *   (:984-1011) and the slot is redundant iff there are more than 3.  Redundant keyframe iff (float)nRedundant > th * (float)nMPs in float
 *   (:1021; 0 > 0 is false).  Without IMU: SetBadFlag() (:1057).  With (:1023-1054): continue if keyframes_in_map <= 21 (:1025); continue
 *   if kf_id > current_id - 2 in unsigned 64-bit arithmetic (:1028); only if prev and next both exist: t = (float)(time[next] -
 *   time[prev]) (:1033); merge and cull if (imu_initialized && kf_id < last_id && t < 3.) || t < 0.5 (:1035), else if !inertial_ba2 &&
 *   |imu_pos - imu_pos[prev]| < 0.02 && t < 3 (:1044).  The norm is float, sqrtf(x*x + (y*y + z*z)) without contraction: Eigen leaves the
 *   order of that sum to its build, THIS CHOICE DEFINES PARITY.  A merge sets next.prev = prev, prev.next = next, clears the keyframe's own
 *   links (:1038-1041) and then calls SetBadFlag(); later keyframes see the new links.
 *   SetBadFlag() (SF/src/KeyFrame.cc:585-691): with mbNotErase nothing is erased (the relink before it has still happened).  Otherwise the
 *   point of every non-NULL slot drops its observation of this keyframe if it holds one (:605-611): nObs -= weight, and at nObs <= 2 the
 *   point turns bad and loses all its observations (MapPoint.cc:177-248); a point held by two slots of the keyframe loses its observation
 *   once.  Then the keyframe is bad and keyframes_in_map is one less (Map::EraseKeyFrame).  KeyFrame::UpdateConnections and the
 *   spanning-tree repair of SetBadFlag stay with the caller's objects.
 * Two kernel launches, one upload and one download for the whole batch; the results are in host memory when the call returns (stream:
 * NULL = the calling thread's private stream).  TC2LI_ERR_INVALID before any launch for negative sizes, NULL required pointers, offsets
 * that do not ascend from 0 and indices out of range.  Returns n_problems. */
int tc2li_keyframe_culling_batch(const tc2li_culling_problem* problems, int n_problems, void* stream);
/* The same contract as plain sequential C++ (one problem per worker thread); needs no device. */
int tc2li_host_keyframe_culling_batch(const tc2li_culling_problem* problems, int n_problems);
enum tc2li_mp_cull_action {
    TC2LI_MP_CULL_KEEP = 0,            /* stays in mlpRecentAddedMapPoints (:393-397) */
    TC2LI_MP_CULL_DROP_BAD = 1,        /* already bad: erased from the list (:379-380) */
    TC2LI_MP_CULL_BAD_RATIO = 2,       /* GetFoundRatio() < 0.25f: SetBadFlag and erased (:381-385) */
    TC2LI_MP_CULL_BAD_OBS = 3,         /* two keyframes old with Observations() <= th_obs: SetBadFlag and erased (:386-390) */
    TC2LI_MP_CULL_DROP_AGE = 4         /* three keyframes old: erased from the list (:391-392) */
};
/* LocalMapping::MapPointCulling (:360-399) for n_points entries of mlpRecentAddedMapPoints, of any number of sequences (current_kf_id is
 * per point): the first rule that holds, in the order above.  The found ratio is (float)n_found / (float)n_visible < 0.25f as IEEE float
 * (SF/src/MapPoint.cc GetFoundRatio; a zero denominator gives inf or NaN, which are not below 0.25); the ages are (int)current_kf_id -
 * (int)first_kf_id, through int as :386 and :391 cast.  th_obs: 3 for stereo, 2 for monocular (:366-371).  A point's action depends on no
 * other point.  One launch, one upload, one download.  Returns n_points. */
int tc2li_map_point_culling_batch(const uint8_t* bad, const int32_t* n_found, const int32_t* n_visible, const int64_t* first_kf_id,
                                  const int32_t* n_obs, const int64_t* current_kf_id, int n_points, int th_obs, uint8_t* action, void* stream);
/* The same on the CPU; needs no device. */
int tc2li_host_map_point_culling_batch(const uint8_t* bad, const int32_t* n_found, const int32_t* n_visible, const int64_t* first_kf_id,
                                       const int32_t* n_obs, const int64_t* current_kf_id, int n_points, int th_obs, uint8_t* action);

/* ---- local mapping: covisibility graph (SF/src/KeyFrame.cc:391-486 UpdateConnections, :201-214 AddConnection, :216-238
 * UpdateBestCovisibles) ---------------------------------------------------------------------------------------------------------------------
 * The covisibility update that LocalMapping makes for every new keyframe (SF/src/LocalMapping.cc:348 in ProcessNewKeyFrame, :836 at the
 * end of SearchInNeighbors) on the flat graph: slots of the keyframe, observations per point, weight rows per keyframe.  The library
 * returns the new weight map and ordered lists of the keyframe and of every neighbour whose lists change; the caller writes them into its
 * objects (INTEGRATION.md "UpdateConnections / UpdateBestCovisibles").  Row order stands in for the address order of the reference's
 * std::map<KeyFrame*, ...> containers, and where the reference compares mnId (:418) row equality is used: one row per keyframe. */
enum tc2li_connections_status {
    TC2LI_CONNECTIONS_UNCHANGED = 0,   /* KFcounter was empty: the reference returns at :426-427, nothing is to be applied */
    TC2LI_CONNECTIONS_UPDATED = 1
};
/* the entries of tc2li_connections_problem.counts */
enum tc2li_connections_count {
    TC2LI_CONNECTIONS_STATUS = 0,      /* tc2li_connections_status */
    TC2LI_CONNECTIONS_N_COUNTER = 1,   /* entries of counter_kf / counter_weight */
    TC2LI_CONNECTIONS_N_ORDERED = 2,   /* entries of ordered_kf / ordered_weight, and of touched_kf / touched_changed */
    TC2LI_CONNECTIONS_N_CHANGED = 3,   /* touched keyframes with changed = 1: rows of changed_offsets */
    TC2LI_CONNECTIONS_N_CHANGED_ENTRIES = 4,   /* entries of changed_kf / changed_weight = changed_offsets[n_changed] */
    TC2LI_CONNECTIONS_PARENT = 5,      /* the new mpParent, or -1: mpParent stays */
    TC2LI_CONNECTIONS_COUNTS = 8       /* ints in the block (the last two are 0) */
};
#define TC2LI_CONNECTIONS_TH 15        /* th of :433 */
/* One call of KeyFrame::UpdateConnections.  All pointers are host memory, the arrays are copied by the call; indices are rows of the
 * problem's own tables.  Problems of one batch are independent: two problems over the same graph both see the input state.
 *   keyframes (n_keyframes rows: the current keyframe, every keyframe that observes one of its points, and whatever their rows name):
 *     kf_flags  bit 0 isBad(), bit 1 GetMap() != mpMap of the current keyframe
 *     conn_offsets [n_keyframes + 1], conn_kf, conn_weight: mConnectedKeyFrameWeights per keyframe as a CSR.  A row ascends strictly by
 *     keyframe row (map order; at most one entry per keyframe).  The row of a keyframe that the call cannot touch may be left empty;
 *     every keyframe that observes a point of the current keyframe needs its row.  The current keyframe's own row is not read.
 *   current: the row of the keyframe the call is made on;  slot_point [n_slots]: its mvpMapPoints, -1 = NULL
 *   points (n_points rows): point_bad isBad(); CSR obs_offsets [n_points + 1], obs_kf: the keyframes of GetObservations(), in any order
 *   scalars: first_connection mbFirstConnection; is_init_kf mnId == mpMap->GetInitKFid()
 * Out (capacities are the caller's; an array whose capacity is 0 may be NULL):
 *   counts [TC2LI_CONNECTIONS_COUNTS]: always written.
 *   counter_kf / counter_weight [counter_capacity]: KFcounter, ascending by row = the new mConnectedKeyFrameWeights (:473)
 *   ordered_kf / ordered_weight [ordered_capacity]: the new mvpOrderedConnectedKeyFrames / mvOrderedWeights (:474-475)
 *   touched_kf [ordered_capacity]: the keyframes that got AddConnection(current, weight) (:451, :458), ascending by row -- the same set as
 *     ordered_kf;  touched_changed [ordered_capacity]: 1 if AddConnection went on to UpdateBestCovisibles, 0 if it returned at :210
 *   changed_offsets [ordered_capacity + 1], changed_kf / changed_weight [changed_capacity]: a CSR over the touched keyframes with
 *     changed = 1, in touched order: their new mvpOrderedConnectedKeyFrames / mvOrderedWeights.  Their map entry is (current, weight). */
typedef struct tc2li_connections_problem {
    const uint8_t* kf_flags;
    const int32_t* conn_offsets;
    const int32_t* conn_kf;
    const int32_t* conn_weight;
    const int32_t* slot_point;
    const uint8_t* point_bad;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    int32_t* counts;
    int32_t* counter_kf;
    int32_t* counter_weight;
    int32_t* ordered_kf;
    int32_t* ordered_weight;
    int32_t* touched_kf;
    uint8_t* touched_changed;
    int32_t* changed_offsets;
    int32_t* changed_kf;
    int32_t* changed_weight;
    int32_t n_keyframes, n_slots, n_points, current;
    int32_t counter_capacity, ordered_capacity, changed_capacity;
    uint8_t first_connection, is_init_kf;
    uint8_t pad_[2];
} tc2li_connections_problem;
/* KeyFrame::UpdateConnections (:391-486) for n_problems independent calls at once on the device, with the AddConnection (:201-214) and
 * UpdateBestCovisibles (:216-238) it triggers in the connected keyframes.  Line for line:
 *   votes (:404-423): for every slot whose point is not NULL (:408) and not bad (:411), every observation of the point adds one to its
 *   keyframe's counter unless that keyframe is the current one (row equality for :418's mnId), is bad or belongs to another map (:418).
 *   The loop runs over slots: a point held by two slots votes twice.
 *   empty counter (:426-427): status TC2LI_CONNECTIONS_UNCHANGED, all sizes 0, parent -1; NO OTHER OUTPUT IS WRITTEN.
 *   threshold (:431-459): every counted keyframe with at least th = 15 votes enters vPairs and gets AddConnection(current, votes); if none
 *   does, the one with the most votes, the lowest row among equals (`>` at :443 in map order), enters alone (:455-459).
 *   own lists (:461-475): vPairs sorted ascending as (weight, keyframe) and pushed to the front: weight descending, equal weights by row
 *   DESCENDING.  No isBad() test here beyond the one of the vote.  The weight map becomes the WHOLE counter, entries below 15 included
 *   (:473).
 *   spanning tree (:478-483): parent = ordered_kf[0] if first_connection && !is_init_kf, else -1 = unchanged.  The caller then does
 *   mpParent->AddChild(this) and clears mbFirstConnection.
 *   every touched keyframe k (:201-214): if k's row holds (current, the same weight), AddConnection returns before UpdateBestCovisibles
 *   (:209-210): changed = 0 and no list is given -- k's stored lists may be stale and the reference does not refresh them here.  Otherwise
 *   the entry is inserted or overwritten and k's new lists are UpdateBestCovisibles of its updated row (:216-238): every entry, THOSE
 *   BELOW 15 INCLUDED, except bad keyframes (:229; bit 0 of kf_flags, the current keyframe's too), weight descending, equal weights by row
 *   descending.
 * Two kernel launches, one upload and one download for the whole batch; the results are in host memory when the call returns (stream:
 * NULL = the calling thread's private stream).  TC2LI_ERR_INVALID before any launch for negative sizes or capacities, NULL required
 * pointers, offsets that do not ascend from 0, indices out of range (current, conn_kf, slot_point below -1, obs_kf) and conn rows that
 * do not ascend strictly.  TC2LI_ERR_CAPACITY when a list of some problem does not fit: then counts is written for every problem and no
 * list for any; N_COUNTER and N_ORDERED are the sizes needed, N_CHANGED and N_CHANGED_ENTRIES too once those two fit (they are 0 until
 * then).  Returns n_problems. */
int tc2li_update_connections_batch(const tc2li_connections_problem* problems, int n_problems, void* stream);
/* The same contract as plain sequential C++ (one problem per worker thread); needs no device. */
int tc2li_host_update_connections_batch(const tc2li_connections_problem* problems, int n_problems);
/* KeyFrame::UpdateBestCovisibles (:216-238) alone for n_rows keyframes of any number of sequences: what LocalMapping::KeyFrameCulling
 * calls first (SF/src/LocalMapping.cc:920) and what KeyFrame::EraseConnection (SF/src/KeyFrame.cc:699-713) calls in every neighbour of a
 * culled keyframe.  In: the CSR row_offsets [n_rows + 1], row_kf, row_weight of the keyframes' mConnectedKeyFrameWeights -- a row ascends
 * strictly by keyframe (map order); row_kf are rows of bad [n_keyframes], isBad() of every keyframe the rows name (non-zero = bad).
 * Out: out_offsets [n_rows + 1], out_kf / out_weight [row_offsets[n_rows]]: per keyframe its entries without the bad ones (:229), weight
 * descending, equal weights by row descending (the sort of :224 on (weight, keyframe) read from the back, :231-232) -- the device function
 * that orders the neighbours' lists of tc2li_update_connections_batch.  An empty row gives an empty list.  One launch, one upload, one
 * download.  TC2LI_ERR_INVALID before any launch as above.  Returns n_rows. */
int tc2li_update_best_covisibles_batch(const int32_t* row_offsets, const int32_t* row_kf, const int32_t* row_weight, int n_rows,
                                       const uint8_t* bad, int n_keyframes, int32_t* out_offsets, int32_t* out_kf, int32_t* out_weight,
                                       void* stream);
/* The same on the CPU; needs no device. */
int tc2li_host_update_best_covisibles_batch(const int32_t* row_offsets, const int32_t* row_kf, const int32_t* row_weight, int n_rows,
                                            const uint8_t* bad, int n_keyframes, int32_t* out_offsets, int32_t* out_kf,
                                            int32_t* out_weight);
/* The sizes at which tc2li_update_connections_batch changes path (for tests): out[0] = the largest n_keyframes whose vote counters are
 * kept in LDS (beyond: in global memory), out[1] = lanes per ranking group (a wavefront), out[2] = threads per problem in the vote
 * kernel.  Returns 3.  No reference counterpart. */
int tc2li_connections_limits(int32_t* out, int capacity);

/* ---- LocalMapping::ProcessNewKeyFrame (SF/src/LocalMapping.cc:312-352) for many sequences in one call ----
 * The first stage of LocalMapping::Run: the new keyframe's tracked points gain their observation (:326-345), mlpRecentAddedMapPoints is
 * filled (:341) and the first KeyFrame::UpdateConnections is made (:348), on the flat graph.  ComputeBoW (:321) is
 * tc2li_orb_compute_bow_batch; the queue (:314-318), mpAtlas->AddKeyFrame (:351) and mbFirstConnection stay the caller's.  Rig: that of
 * tc2li_search_in_neighbors_batch (pinhole stereo, NLeft == -1, mpCamera2 == nullptr, every observation index is a left index >= 0).
 * One problem is one mpCurrentKeyFrame; all pointers are host memory and the call copies the arrays; indices are rows of the problem's own
 * tables; row order stands in for the address order of std::map<KeyFrame*, ...> (as in tc2li_neighbors_problem).  Problems of a batch are
 * independent: two problems over one graph both see the input state, and one store slot may appear in several problems.
 *
 * Inputs.  `conn` is a tc2li_connections_problem and is read as that entry reads it -- kf_flags, conn_offsets / conn_kf / conn_weight,
 * current, slot_point [n_slots] (GetMapPointMatches() at :324, -1 = NULL; n_slots must equal the stored keypoint count of the current
 * keyframe's slot), point_bad, first_connection, is_init_kf, the capacities and the outputs -- except that its obs_offsets / obs_kf are the
 * observation rows ON ENTRY (a row ascends strictly by keyframe row) while the votes of rule 4 are taken on the END state.  Beside it:
 *   keyframes (conn.n_keyframes rows: the current keyframe, every observer of every point in its slot row, whatever the connection rows name):
 *     kf_slot   the store slot (host entry: an index into views); -1 is allowed only for a row that observes no point of the slot row
 *     centres   [n][3] GetCameraCenter()
 *   points (conn.n_points rows): positions [n][3]; point_nobs nObs; point_ref_kf the row of mpRefKF and point_ref_level_scale as in
 *     tc2li_map_points_refresh; obs_index, parallel to conn.obs_kf: the left index
 *   last_level_scale = mvScaleFactors[nLevels - 1] (MapPoint.cc:500)
 *
 * Rule 1, association (:326-345).  Slots ascend.  A NULL slot (:329) and a bad point (:331) are skipped.  If the current keyframe's row is
 *   not in the point's observation row NOW (IsInKeyFrame, MapPoint.cc:429-433): AddObservation(current, i) (MapPoint.cc:150-175) inserts
 *   the pair at its place in row order and adds 2 to nObs if u_right[i] >= 0, else 1; UpdateNormalAndDepth (:336) and
 *   ComputeDistinctiveDescriptors (:337) then run on the new state.  Otherwise the point is pushed to the recent list (:341), which is in
 *   slot order; a point held by two observed slots is pushed twice.  A point held by two slots and not yet observed is associated by the
 *   lower slot and pushed by the higher one.  A point observed from the current keyframe at an index other than its slot is simply "in":
 *   recent list, nothing changes.
 * Rule 2, UpdateNormalAndDepth (MapPoint.cc:435-503).  The normal is the float sum of (pos - centre) / |pos - centre| over every observation
 *   in row order, BAD KEYFRAMES INCLUDED (:456-475 has no isBad() test), divided by their number; max_distance = |pos - centres[point_ref_kf]|
 *   * point_ref_level_scale (:499), min_distance = max_distance / last_level_scale (:500).  The arithmetic and evaluation order of
 *   tc2li_map_points_refresh, bit for bit.
 * Rule 3, ComputeDistinctiveDescriptors (MapPoint.cc:338-412): rule 4 of tc2li_search_in_neighbors_batch -- the descriptors of the
 *   observations in keyframes that are NOT bad (:361), in row order, read from the store; per row the sorted row's entry
 *   (int)(0.5 * (N - 1)); the first row with the least such median wins.
 * Rule 4, UpdateConnections (:348): every output of `conn` equals what tc2li_update_connections_batch returns for the same kf_flags,
 *   connection rows, slot_point and point_bad with the observation CSR AFTER rule 1.
 *
 * Why the device may work on a slot row side by side: a point is associated at most once per call, and nothing else in the loop changes
 * any point's observations, any position or any centre; so the refresh of an associated point reads the same state whether it runs at
 * its slot's turn or after the loop.  The only sequential fact is which of several slots holding one unobserved point comes first: a
 * first-occurrence minimum over slot indices, taken with an integer atomicMin.
 *
 * Outputs (capacities are the caller's; an array of capacity 0 may be NULL):
 *   counts [TC2LI_PROCESS_KEYFRAME_COUNTS], always written: status (TC2LI_PROCESS_KEYFRAME_ON_DEVICE / _ON_HOST), associated, recent
 *                  pushes, entries of the observation CSR out
 *   associated_slot / associated_point [associated_capacity]   in slot order: the shim replays AddObservation from these
 *   recent [recent_capacity]                                   the pushes of :341 in order
 *   point_nobs_out [n_points]; obs_offsets_out [n_points + 1], obs_kf_out / obs_index_out [obs_capacity]: the end state
 *   desc_kf / desc_index [n_points]   the observation whose descriptor is mDescriptor afterwards, -1 where the step did not run or left early
 *   refreshed [n_points] and, where it is set, normals_out [n][3], min_distance_out, max_distance_out
 *   conn.counts and the lists of conn, exactly as tc2li_connections_problem defines them
 * Errors.  TC2LI_ERR_INVALID before any device work and with nothing written: sizes and NULLs, offsets that do not ascend from 0, indices
 *   out of range, observation or connection rows that do not ascend strictly, an empty or out-of-range slot where one is needed (the
 *   current keyframe and the observers of the slot row's points), n_slots different from the stored keypoint count, an observation index
 *   beyond the observer's keypoints, a point_ref_kf out of range for a point that can be associated (in the slot row, not bad, not yet
 *   observed from the current keyframe).  TC2LI_ERR_CAPACITY as tc2li_search_in_neighbors_batch: counts and conn.counts are written for
 *   every problem with the sizes needed and no list for any; the call repeated with those capacities succeeds.  conn.counts keeps its own
 *   rule: N_CHANGED and N_CHANGED_ENTRIES are the sizes needed once counter_capacity and ordered_capacity suffice, and 0 until then.
 * The device entry: one upload, four launches whatever the batch (classification and the end-state CSR, one workgroup per problem; the
 * refresh, one wavefront per associated point over the whole batch; the two connection kernels on the CSR the first launch wrote), one
 * download, no host wait between launches.  A problem in which a point would pass the observation limit of
 * tc2li_process_new_keyframe_limits is finished inside the call by the host twin, reports TC2LI_PROCESS_KEYFRAME_ON_HOST and has the same
 * outputs.  Both entries return n_problems. */
#define TC2LI_PROCESS_KEYFRAME_COUNTS 4
#define TC2LI_PROCESS_KEYFRAME_ON_DEVICE 0
#define TC2LI_PROCESS_KEYFRAME_ON_HOST 1
typedef struct tc2li_process_keyframe_problem {
    tc2li_connections_problem conn;
    const int32_t* kf_slot; const float* centres;
    const float* positions; const int32_t *point_nobs, *point_ref_kf; const float* point_ref_level_scale; const int32_t* obs_index;
    int32_t* counts; int32_t *associated_slot, *associated_point, *recent;
    int32_t *point_nobs_out, *obs_offsets_out, *obs_kf_out, *obs_index_out, *desc_kf, *desc_index;
    uint8_t* refreshed; float *normals_out, *min_distance_out, *max_distance_out;
    int32_t associated_capacity, recent_capacity, obs_capacity;
    float last_level_scale;
} tc2li_process_keyframe_problem;
int tc2li_process_new_keyframe_batch(tc2li_keyframe_store* store, const tc2li_process_keyframe_problem* problems, int n_problems,
                                     void* stream);
/* The host twin: plain sequential C++ in the reference's order, the refresh at the slot's turn; one problem per worker thread under the
 * host thread budget; kf_slot indexes views (n, descriptors and u_right are read; n < 0 = an empty slot).  No observation limit; needs
 * no device.  counts[0] is TC2LI_PROCESS_KEYFRAME_ON_HOST. */
int tc2li_host_process_new_keyframe_batch(const tc2li_keyframe_view* views, int n_views, const tc2li_process_keyframe_problem* problems,
                                          int n_problems);
/* The limits of the device path: out[0] the most observations a point may reach (tc2li_map_points_refresh's), out[1] the most keypoints
 * of a keyframe, out[2] threads per problem of the classification kernel, out[3] wavefronts per workgroup of the refresh kernel.  The
 * per-point and per-keyframe marks live in global memory, so there is no limit on the points or keyframes of a problem.  Returns how
 * many values there are; needs no device. */
int tc2li_process_new_keyframe_limits(int32_t* out, int capacity);

/* ---- local mapping: the window of the local BA (SF/src/OptimizerWithLidar.cc:63-130 the gather, :157-187 the pose vertices, :226-253 the
 * keyframes of the BALM edge, :263-384 the point vertices and edges; the identical gather of Optimizer::LocalBundleAdjustment,
 * SF/src/Optimizer.cc:1124-1190) -----------------------------------------------------------------------------------------------------------
 * The graph walk that turns "the current keyframe" into the arrays of tc2li_local_bundle_adjustment / tc2li_ba_problem /
 * tc2li_lidar_window, on the flat graph of tc2li_connections_problem, for many sequences at once.  The pixel, the right coordinate and the
 * octave of every observation are read from the keyframe store's slots; floats are widened to double, so every output is exact.
 * Not covered: the two-camera branch (:347-381). */
enum tc2li_ba_window_status {
    TC2LI_BA_WINDOW_OK = 0,
    TC2LI_BA_WINDOW_ABORTED = 1        /* num_fixedKF == 0 (:126-130): the reference returns without a BA */
};
enum tc2li_ba_window_count {
    TC2LI_BA_WINDOW_STATUS = 0,        /* tc2li_ba_window_status */
    TC2LI_BA_WINDOW_NUM_FIXED_KF = 1,  /* num_fixedKF of :123: the fixed cameras, plus the 1 of :85-88 when a local keyframe is the initial one */
    TC2LI_BA_WINDOW_NUM_OPT_KF = 2,    /* num_OptKF of :171: lLocalKeyFrames.size() */
    TC2LI_BA_WINDOW_N_POSES = 3,       /* entries of pose_row / poses7_out / fixed: local keyframes + fixed cameras */
    TC2LI_BA_WINDOW_N_POINTS = 4,      /* entries of point_row / points3_out: lLocalMapPoints.size() */
    TC2LI_BA_WINDOW_N_EDGES = 5,       /* entries of edges (num_edges of :385) */
    TC2LI_BA_WINDOW_N_LIDAR = 6,       /* entries of lidar_pose_index: 0, or 3 .. 6 */
    TC2LI_BA_WINDOW_N_POINTS_WITHOUT_EDGE = 7,   /* listed points that got no edge (tc2li_local_bundle_adjustment refuses such a point) */
    TC2LI_BA_WINDOW_COUNTS = 8
};
#define TC2LI_BA_WINDOW_MAX_LIDAR 6    /* win_size_ of :245 */
/* One call of the gather for one current keyframe.  All pointers are host memory, the arrays are copied by the call; indices are rows of the
 * problem's own tables; problems of one batch are independent.  The row order of the keyframes stands in for the address order of the
 * reference's std::map<KeyFrame*, ...>, as in tc2li_connections_problem.
 *   keyframes (n_keyframes rows: the current keyframe, cov_kf, every observer of their points):
 *     kf_slot   the slot of the keyframe in the store (the host entry: the index into views)
 *     kf_id     mnId
 *     kf_flags  bit 0 isBad(), bit 1 GetMap() != pCurrentMap, bit 2 mLidarProps->GetSurfacePcl()->size() > 0
 *     poses7    [n_keyframes][7] GetPose() as tc2li_ba_problem takes it (qx qy qz qw tx ty tz, widened)
 *     slot_offsets [n_keyframes + 1], slot_point: GetMapPointMatches() per keyframe as a CSR, -1 = NULL.  Only the rows of the current
 *     keyframe and of cov_kf are read; others may be empty.
 *   current: the row of pKF;  cov_kf [n_cov]: GetVectorCovisibleKeyFrames() in its order (no row twice, not the current one);
 *   init_kf_id: pMap->GetInitKFid()
 *   points (n_points rows): point_flags bit 0 isBad(), bit 1 GetMap() != pCurrentMap; positions [n_points][3] GetWorldPos() widened; CSR
 *     obs_offsets [n_points + 1], obs_kf, obs_index: GetObservations(), a row ascending strictly by keyframe row, obs_index = get<0> of
 *     the tuple (the left keypoint, or -1)
 * Out (capacities are the caller's; an array whose capacity is 0 may be NULL):
 *   counts [TC2LI_BA_WINDOW_COUNTS]: always written.  ABORTED: every count after NUM_FIXED_KF is 0 and NO OTHER OUTPUT IS WRITTEN.
 *   pose_row [pose_capacity], poses7_out [pose_capacity][7], fixed [pose_capacity]: the local keyframes and the fixed cameras ascending by
 *     kf_id (by row among equal ids) -- the vertex-id order tc2li_local_bundle_adjustment asks for; fixed = 1 for a fixed camera (:181) and
 *     for a local keyframe whose id is init_kf_id (:164)
 *   point_row [point_capacity], points3_out [point_capacity][3]: lLocalMapPoints in the reference's order
 *   edges [edge_capacity]: one per observation in the creation order of :263-384; point / pose index the two lists above
 *   lidar_pose_index [TC2LI_BA_WINDOW_MAX_LIDAR]: the entries of pose_row of vOptKeyFrames[0 .. n_lidar), -1 beyond; the clouds stay with
 *     the caller (tc2li_lidar_window::win_pose) */
typedef struct tc2li_ba_window_problem {
    const int32_t* kf_slot;
    const int64_t* kf_id;
    const uint8_t* kf_flags;
    const double* poses7;
    const int32_t* slot_offsets;
    const int32_t* slot_point;
    const int32_t* cov_kf;
    const uint8_t* point_flags;
    const double* positions;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int32_t* obs_index;
    int32_t* counts;
    int32_t* pose_row;
    double* poses7_out;
    uint8_t* fixed;
    int32_t* point_row;
    double* points3_out;
    tc2li_ba_edge* edges;
    int32_t* lidar_pose_index;
    int64_t init_kf_id;
    int32_t n_keyframes, n_points, n_cov, current;
    int32_t pose_capacity, point_capacity, edge_capacity;
    int32_t pad_;
} tc2li_ba_window_problem;
/* The gather for n_problems current keyframes at once on the device.  Line for line:
 *   local keyframes (:63-76): the current keyframe whatever its flags (:65), then every keyframe of cov_kf in order that is neither bad nor
 *   of another map (:74).  EVERY keyframe of cov_kf is marked local (:73 comes before the test of :74): a bad or other-map neighbour is
 *   neither local nor ever fixed (:115).
 *   local points (:78-104): the local keyframes in list order, their slots ascending; a point that is not NULL (:93), not bad and of this
 *   map (:94) is listed at its first occurrence (:97-101), whether two slots or two keyframes hold it.
 *   fixed cameras (:107-122): every observer of a listed point that is not marked local and is neither bad nor of another map (:115-119),
 *   WHATEVER ITS obs_index: a fixed pose may end up with no edge.
 *   num_fixedKF (:123) = the fixed cameras + 1 if a local keyframe has init_kf_id (:85-88); 0: ABORTED (:126-130).
 *   poses (:157-187): setId(mnId) is what orders them.
 *   BALM keyframes (:226-253): the local keyframes in list order with bit 2 set; n_lidar = min(their number, 6) if there are more than 2,
 *   else 0.
 *   edges (:263-384): the listed points in order, the observations of a point ascending by row; an observer that is bad or of another map
 *   is skipped (:281), so is obs_index -1 (:286, :313).  u, v = mvKeysUn[obs_index].pt, u_right = mvuRight[obs_index] when >= 0 (:313),
 *   else -1 (:286), inv_sigma2 = inv_level_sigma2[octave] (mvInvLevelSigma2, :297, :325).
 * Two kernel launches, one upload and one download for the whole batch; the results are in host memory when the call returns (stream:
 * NULL = the calling thread's private stream).  TC2LI_ERR_INVALID before any launch for negative sizes or capacities, NULL required
 * pointers, offsets that do not ascend from 0, indices out of range (current, cov_kf, slot_point below -1, obs_kf, obs_index below -1 or
 * beyond the keypoints of the observer's slot), a row of cov_kf named twice or equal to current, observation rows that do not ascend
 * strictly, a kf_slot that is empty or out of range, and a slot that holds an octave outside [0, n_levels).  TC2LI_ERR_CAPACITY when a
 * list of some problem does not fit: then counts is written for every problem, with the sizes needed, and no list for any.  Returns
 * n_problems. */
int tc2li_ba_window_batch(tc2li_keyframe_store* store, const tc2li_ba_window_problem* problems, int n_problems,
                          const float* inv_level_sigma2, int n_levels, void* stream);
/* The same contract as plain sequential C++ (one problem per worker thread): the walk the host shim made until now.  kf_slot indexes
 * views [n_views], of which n, keys and u_right are read (n < 0: an empty slot).  Needs no device. */
int tc2li_host_ba_window_batch(const tc2li_keyframe_view* views, int n_views, const tc2li_ba_window_problem* problems, int n_problems,
                               const float* inv_level_sigma2, int n_levels);
/* The sizes at which tc2li_ba_window_batch changes path (for tests): out[0] = the largest n_keyframes whose local / fixed marks are kept
 * in LDS (beyond: in global memory), out[1] = the largest n_points whose first-occurrence keys are kept in LDS (beyond: in global
 * memory), out[2] = threads per problem.  Returns 3.  Needs no device.  No reference counterpart. */
int tc2li_ba_window_limits(int32_t* out, int capacity);
/* The outlier rule after the BA (:402-449), host only: vToErase as (pose index, point index) pairs in the reference's order -- the
 * monocular edges (u_right < 0) with chi2 > 5.991 || !depthPositive (:406-419) in creation order, then the stereo edges with 7.815
 * (:436-449); edges of a point with point_bad_now (pMP->isBad() after the BA, :411, :441) are skipped.  edges, edge_chi2 and
 * edge_depth_positive are those of the finished tc2li_local_bundle_adjustment; erase_pose / erase_point [capacity].  Returns the count;
 * TC2LI_ERR_CAPACITY (nothing written) when it exceeds capacity, TC2LI_ERR_INVALID for an edge whose point is outside [0, n_points). */
int tc2li_ba_window_outliers(const tc2li_ba_edge* edges, const double* edge_chi2, const uint8_t* edge_depth_positive, int n_edges,
                             const uint8_t* point_bad_now, int n_points, int32_t* erase_pose, int32_t* erase_point, int capacity);

/* ---- local mapping: the optimiser's index structure of a window (no reference counterpart: g2o builds its own containers) ----------------
 * What tc2li_local_bundle_adjustment builds from (fixed, edges) before its first kernel: the numbering of the free poses, the edges by
 * landmark and by free pose, one slot per (landmark, free pose) pair in landmark-major order, the slices of the Schur product, duplicate
 * pairs, the blocks of 256 slots sorted by pose, the groups of the linearisation, and the sizes that follow
 * (tc2li-slam_amd/csrc/ba_structure.hpp:69-229 ba_build_structure, :39-65 the sizes of the Schur product, :231-264 the layout of the
 * window's input block from the sizes alone; VisualProblem::setup, csrc/ba_internal.hpp:230-285, calls them).  The arrays come back in one
 * int32 buffer; table [TC2LI_BA_STRUCTURE_FIELDS][2] holds (offset, count) of every field in it. */
enum tc2li_ba_structure_field {
    TC2LI_BA_STRUCTURE_SCALARS = 0,   /* [TC2LI_BA_STRUCTURE_SCALAR_COUNT], see tc2li_ba_structure_scalar */
    TC2LI_BA_STRUCTURE_POSE_VAR,      /* [n_poses] the number of a free pose that is used by an edge (or extra_used), -1 otherwise */
    TC2LI_BA_STRUCTURE_PT_OFF,        /* [n_points + 1] CSR of the edges by point */
    TC2LI_BA_STRUCTURE_PT_EDGES,      /* [n_edges] */
    TC2LI_BA_STRUCTURE_PV_OFF,        /* [n_free + 1] CSR of the edges with a slot by free pose */
    TC2LI_BA_STRUCTURE_PV_EDGES,      /* [pv_off[n_free]] */
    TC2LI_BA_STRUCTURE_FL_OFF,        /* [2 * n_points] begin, end of a point's slots */
    TC2LI_BA_STRUCTURE_FL_POSE,       /* [n_slots] the slot's free pose */
    TC2LI_BA_STRUCTURE_FL_LM,         /* [n_slots] its point */
    TC2LI_BA_STRUCTURE_FL_PLACE,      /* [n_slots] the point's number within its slice */
    TC2LI_BA_STRUCTURE_FL_EDGE,       /* [n_slots] its edge */
    TC2LI_BA_STRUCTURE_W_SLOT,        /* [n_edges] the edge's slot, -1: a fixed pose or a duplicate */
    TC2LI_BA_STRUCTURE_SLICE_OFF,     /* [n_schur_slices + 1] first slot of every slice */
    TC2LI_BA_STRUCTURE_DUP_OFF,       /* [n_free + 1] CSR of the duplicates by free pose (all 0 without duplicates) */
    TC2LI_BA_STRUCTURE_DUP_EDGE,      /* [n_dups] */
    TC2LI_BA_STRUCTURE_DUP_SLOT,      /* [n_dups] the slot of the pair's first edge */
    TC2LI_BA_STRUCTURE_BLK_OFF,       /* [max(n_blocks, 1)][n_free + 1] per block of 256 slots: CSR of its rows by pose */
    TC2LI_BA_STRUCTURE_BLK_ROWS,      /* [max(n_blocks, 1)][256] the block's slots (0 .. 255) sorted by pose, stable; bytes widened to int32 */
    TC2LI_BA_STRUCTURE_GRP_K0,        /* [n_groups + 1] first edge (in pt_edges order) of every group */
    TC2LI_BA_STRUCTURE_GRP_L0,        /* [n_groups + 1] first point of every group */
    TC2LI_BA_STRUCTURE_CHUNK_MASK,    /* dense windows only: [max(n_schur_slices, 1)] the 16-column tiles a chunk touches */
    TC2LI_BA_STRUCTURE_FIELDS
};
enum tc2li_ba_structure_scalar {
    TC2LI_BA_STRUCTURE_N_FREE = 0,
    TC2LI_BA_STRUCTURE_N_SLOTS,              /* n_free_edges after the slots are made */
    TC2LI_BA_STRUCTURE_N_FREE_POSE_EDGES,    /* edges with a free pose, duplicates counted */
    TC2LI_BA_STRUCTURE_N_DUPS,
    TC2LI_BA_STRUCTURE_N_BLOCKS,
    TC2LI_BA_STRUCTURE_N_GROUPS,
    TC2LI_BA_STRUCTURE_MAX_GROUP_LANDMARKS,
    TC2LI_BA_STRUCTURE_NP,                   /* 6 * n_free */
    TC2LI_BA_STRUCTURE_NP_PAD,
    TC2LI_BA_STRUCTURE_N_SCHUR_SLICES,
    TC2LI_BA_STRUCTURE_N_SLICES,             /* partial sums of the Schur product */
    TC2LI_BA_STRUCTURE_K_PER_SLICE,
    TC2LI_BA_STRUCTURE_SCHUR_GROUP,
    TC2LI_BA_STRUCTURE_SPARSE,               /* 1: the lean block-by-block product (at most 24 free poses) */
    TC2LI_BA_STRUCTURE_SCHUR_RD,
    TC2LI_BA_STRUCTURE_SCHUR_RO,
    TC2LI_BA_STRUCTURE_SCALAR_COUNT
};
/* Host only, needs no device.  fixed [n_poses], edges [n_edges] (point, pose and nothing else is read), extra_used [n_poses] or NULL: poses
 * that count as used without an edge (the keyframes of the LiDAR edge).  table [TC2LI_BA_STRUCTURE_FIELDS][2] and out [capacity] are
 * written; out == NULL with capacity 0 is a sizing call that writes the table alone.  Returns the number of int32 the fields take;
 * TC2LI_ERR_CAPACITY when that exceeds a non-zero capacity (the table is written); TC2LI_ERR_INVALID, as tc2li_local_bundle_adjustment
 * would, for an edge whose pose or point is out of range, a point without an edge, a point with more than 256 edges, more than 256 points
 * in a group, more than 85 free poses. */
int tc2li_host_ba_structure(const uint8_t* fixed, int n_poses, int n_points, const tc2li_ba_edge* edges, int n_edges, const uint8_t* extra_used,
                            int32_t* table, int32_t* out, int capacity);
/* The gather of tc2li_ba_window_batch followed by the structure of every window, built ON THE DEVICE from the gather's device output: the
 * front half of the hand-over of a window to the BA without a trip over the bus.  Per window the kernels write the arrays and a size
 * record; the host reads the records, lays out the window's input block -- [poses | points | edges | pose_var | pt_off | pt_edges | pv_off
 * | fl_off | fl_pose | fl_lm | fl_place | slice_off | fl_edge | grp_k0 | grp_l0 | blk_off | blk_rows | ticket words], what the BA's kernels
 * read -- and the pieces are moved there device to device.  This entry then downloads the blocks and returns them in the flat form of
 * tc2li_host_ba_structure, for tests and tools: tables [n_problems][TC2LI_BA_STRUCTURE_FIELDS][2], out [n_problems][out_stride].  The fields
 * a sparse window's block does not hold (pv_edges, w_slot, dup_*, chunk_mask) have count 0; every other field equals
 * tc2li_host_ba_structure of the gathered window, integer for integer.  with_lidar [n_problems] or NULL (= all 1): whether the window's
 * keyframes of lidar_pose_index count as used (extra_used), as they do when the window gets the LiDAR edge.
 * The problems are those of tc2li_ba_window_batch, and their outputs are written as it writes them (so is its TC2LI_ERR_CAPACITY).
 * results [n_problems]: the int32 written to the window's row of out; 0 for an ABORTED window; TC2LI_ERR_INVALID for what
 * tc2li_local_bundle_adjustment refuses (a listed point without an edge, a point with more than 256 edges, more than 256 points in a
 * group), decided on the device; TC2LI_BA_STRUCTURE_DECLINED for a window outside the device range (tc2li_ba_window_solve_limits).  Returns
 * n_problems; TC2LI_ERR_CAPACITY when out_stride is too small for some window (results then holds the sizes needed). */
#define TC2LI_BA_STRUCTURE_DECLINED (-1000)
int tc2li_ba_window_structure_batch(tc2li_keyframe_store* store, const tc2li_ba_window_problem* problems, int n_problems,
                                    const float* inv_level_sigma2, int n_levels, const uint8_t* with_lidar, int32_t* tables, int32_t* out,
                                    int out_stride, int32_t* results, void* stream);
/* The range in which a window's structure is built on the device: out[0] = the most free poses (the lean sparse path of the BA), out[1] =
 * the most poses, out[2] = the most points (both live in LDS), out[3] = threads per window.  Returns 4.  Needs no device. */
int tc2li_ba_window_solve_limits(int32_t* out, int capacity);

/* ---- local mapping: gather, local BA and outlier rule of LocalBundleAdjustment / LocalLVBundleAdjustment in one call
 * (SF/src/OptimizerWithLidar.cc:63-130 the gather, :157-384 the graph, :386-400 the optimisation, :402-449 the outlier rule) ---------------
 * What tc2li_ba_window_batch, tc2li_local_bundle_adjustment_batch_group and tc2li_ba_window_outliers do one after the other, without the
 * window's points, edges and index structure crossing the bus in between: the gather's output stays on the device, the structure is built
 * there (tc2li_ba_window_structure_batch above; csrc/ba_structure_kernels.hip), the lock-step batch adopts the windows' input blocks device
 * to device (VisualProblem::adopt, csrc/ba_internal.hpp:290-320, in place of setup's host structure and upload), and the outlier rule
 * runs on the device after the last iteration.  Downloaded: the counts, the lists of poses and points, the optimised poses and points, the
 * outlier pairs (and the edges, chi2 and depth flags a problem asks for).  Uploaded: the flat graph.
 *   window: a problem of tc2li_ba_window_batch.  Its inputs as there; edges may be NULL (with any edge_capacity): the window's edges are then
 *     never downloaded.  counts, pose_row, fixed, point_row and lidar_pose_index are written as the gather writes them; poses7_out and
 *     points3_out receive the OPTIMISED values.
 *   iterations, lambda_init, stop_flag, stats, edge_chi2, edge_depth_positive [edge_out_capacity]: the arguments of
 *     tc2li_local_bundle_adjustment; the two arrays may be NULL.
 *   The LiDAR edge: cloud_xyz == NULL means none.  Otherwise cloud_offsets [n_keyframes + 1] (in points) and cloud_xyz give GetSurfacePcl() of
 *     every keyframe ROW of the window's tables, back to back (rows without bit 2 of kf_flags may be empty), Tcl and weight as in
 *     tc2li_lidar_window; the window of n_lidar keyframes is put together from lidar_pose_index (n_lidar == 0: no LiDAR edge) and goes
 *     through the plane extraction with the gathered poses.  lidar_stats as in tc2li_local_lv_bundle_adjustment (may be NULL).
 *   erase_pose, erase_point [erase_capacity], n_erase: vToErase of :402-449 as (pose index, point index) pairs in the reference's order,
 *     what tc2li_ba_window_outliers gives with no point bad (the caller applies pMP->isBad(): the test skips single pairs, so the order of
 *     the others stands).  n_erase may be NULL: the rule is then not evaluated. */
typedef struct tc2li_ba_window_solve_problem {
    tc2li_ba_window_problem window;
    const volatile uint8_t* stop_flag;
    tc2li_ba_stats* stats;
    double* edge_chi2;
    uint8_t* edge_depth_positive;
    const int32_t* cloud_offsets;
    const float* cloud_xyz;
    tc2li_lidar_ba_stats* lidar_stats;
    int32_t* erase_pose;
    int32_t* erase_point;
    int32_t* n_erase;
    double lambda_init, weight;
    float Tcl[7];
    int32_t iterations, edge_out_capacity, erase_capacity;
} tc2li_ba_window_solve_problem;
/* One lock-step group on context `group` (0 .. 7), like tc2li_local_bundle_adjustment_batch_group.  results [n_problems]:
 *   a window that was optimised: the iterations done, as the two-step path returns them, every output written;
 *   an ABORTED window (:126-130): 0, counts alone written;
 *   a window the BA refuses (a listed point without an edge, a point with more than 256 edges, more than 256 points in a group -- decided
 *   on the device): TC2LI_ERR_INVALID, the lists as the gather leaves them, stats zeroed, n_erase 0.
 * Every window's outputs are bit for bit those of tc2li_ba_window_batch followed by tc2li_local_bundle_adjustment_batch_group over the
 * windows that are not ABORTED and by tc2li_ba_window_outliers: the device builds the same structure, and the structure fixes the order of
 * every sum.  A window outside the device range (tc2li_ba_window_solve_limits: more than 24 free keyframes, 1024 poses or 6144 points), every
 * window of a call in which at most one is not ABORTED, of a call with TC2LI_BA_NO_LOCKSTEP set, or of a call whose lock-step group declines
 * (a LiDAR window with more than 2048 planes) is finished inside the call through tc2li_local_lv_bundle_adjustment and
 * tc2li_ba_window_outliers: its edges are copied down for that, and the caller sees the same contract.
 * TC2LI_ERR_CAPACITY for the whole call, with every counts written, nothing else written and no BA run, when a pose or point capacity, a
 * non-NULL edges' edge_capacity, or the edge_out_capacity of a non-NULL edge_chi2 / edge_depth_positive is too small in any problem.  An
 * erase_capacity that turns out too small is only known after the BA: the call then returns TC2LI_ERR_CAPACITY as well, every other output
 * is written, n_erase holds the number of pairs and the first erase_capacity of them are in the arrays.  TC2LI_ERR_INVALID before any
 * launch as tc2li_ba_window_batch, and for NULL cloud_offsets when cloud_xyz is given (a LiDAR keyframe with an empty cloud is refused
 * for its window, as tc2li_local_lv_bundle_adjustment refuses it).  Returns n_problems. */
int tc2li_ba_window_solve_batch(tc2li_keyframe_store* store, const tc2li_ba_window_solve_problem* problems, int n_problems,
                                const float* inv_level_sigma2, int n_levels, const tc2li_camera* cam, int group, int32_t* results);

/* ---- local mapping: the map graph resident on the device, and the local-BA gather reading from it (no reference counterpart as a
 * whole: the reference keeps the graph in KeyFrame / MapPoint objects; every edit below names the call it stands for) --------------------
 * The input half of tc2li_ba_window_problem -- kf_slot, kf_id, kf_flags, poses7, slot_offsets / slot_point, point_flags, positions,
 * obs_offsets / obs_kf / obs_index -- of n_sequences sequences in one slab allocated at create, in the dense CSR layout the gather kernels
 * read.  After tc2li_map_graph_set_batch only edit logs cross the bus (tc2li_map_graph_apply_batch), and tc2li_ba_window_graph_batch /
 * tc2li_ba_window_solve_graph_batch gather from the resident tables.  One lock per handle: calls on one graph run one after the other.
 * The graph is bound to one keyframe store for life: kf_slot names that store's slots, and an observation's index is checked against the
 * keypoints the slot holds when the edit arrives.  (tc2li_map_graph, without a suffix, is the host-array graph of tc2li_local_map.) */
typedef struct tc2li_map_graph_handle tc2li_map_graph_handle;
enum tc2li_map_graph_capacity {       /* per sequence */
    TC2LI_MAP_GRAPH_KEYFRAMES = 0,    /* keyframe rows */
    TC2LI_MAP_GRAPH_SLOTS = 1,        /* entries of slot_point */
    TC2LI_MAP_GRAPH_POINTS = 2,       /* point rows */
    TC2LI_MAP_GRAPH_OBSERVATIONS = 3, /* entries of obs_kf / obs_index */
    TC2LI_MAP_GRAPH_CAPACITIES = 4
};
/* The tables of one sequence as host arrays, the members named as in tc2li_ba_window_problem.  Read by set_batch and the host twin,
 * written by download and the host twin. */
typedef struct tc2li_map_graph_tables {
    int32_t* kf_slot;
    int64_t* kf_id;
    uint8_t* kf_flags;
    double* poses7;
    int32_t* slot_offsets;
    int32_t* slot_point;
    uint8_t* point_flags;
    double* positions;
    int32_t* obs_offsets;
    int32_t* obs_kf;
    int32_t* obs_index;
    int32_t n_keyframes, n_points;
} tc2li_map_graph_tables;
/* One edit: 16 bytes.  Operands that carry doubles name an offset into the log's `values`.
 *   op                  a          b          c            reference                                         effect
 *   ADD_KEYFRAME        store slot n_slots    values off   new KeyFrame, SF/src/Tracking.cc:3078             appends a keyframe row whose n_slots slots are -1;
 *                                                                                                            values: id, flags, pose7 (9 doubles; id and flags
 *                                                                                                            integral).  Its row is n_keyframes + the appends
 *                                                                                                            before it in this log
 *   SET_KEYFRAME_FLAGS  row        flags      -            KeyFrame::SetBadFlag SF/src/KeyFrame.cc:585,      overwrites
 *                                                          the LiDAR cloud bit
 *   SET_POSE            row        values off -            KeyFrame::SetPose SF/src/KeyFrame.cc:121          overwrites poses7 (7 doubles)
 *   ADD_POINT           flags      values off -            new MapPoint                                      appends a point row (3 doubles) with an empty
 *                                                                                                            observation row
 *   SET_POINT_FLAGS     row        flags      -            MapPoint::SetBadFlag SF/src/MapPoint.cc:225       overwrites
 *   SET_POSITION        row        values off -            MapPoint::SetWorldPos                             overwrites (3 doubles)
 *   SET_SLOT            kf row     slot       point or -1  KeyFrame::AddMapPoint / EraseMapPointMatch /      overwrites one slot
 *                                                          ReplaceMapPointMatch SF/src/KeyFrame.cc:309-340
 *   ADD_OBSERVATION     point      kf row     index        MapPoint::AddObservation SF/src/MapPoint.cc:150-175  inserts the pair at its place in row order; a
 *                                                                                                            keyframe already in the row gets its index
 *                                                                                                            OVERWRITTEN (mObservations[pKF] = indexes, :155-169)
 *   ERASE_OBSERVATION   point      kf row     -            MapPoint::EraseObservation SF/src/MapPoint.cc:177-210  removes the pair; a no-op if absent (:182)
 *   CLEAR_OBSERVATIONS  point      -          -            mObservations.clear() in MapPoint::SetBadFlag     empties the row
 * The graph stores literal edits: what the reference chains onto one (EraseObservation turning a point bad at nObs <= 2, SetBadFlag
 * erasing the slots of every observer, Replace) the caller spells out as further edits.  The result is what applying the log one edit
 * after the other gives; an edit may name a row the same log appended earlier. */
enum tc2li_map_graph_op {
    TC2LI_MAP_GRAPH_ADD_KEYFRAME = 0,
    TC2LI_MAP_GRAPH_SET_KEYFRAME_FLAGS = 1,
    TC2LI_MAP_GRAPH_SET_POSE = 2,
    TC2LI_MAP_GRAPH_ADD_POINT = 3,
    TC2LI_MAP_GRAPH_SET_POINT_FLAGS = 4,
    TC2LI_MAP_GRAPH_SET_POSITION = 5,
    TC2LI_MAP_GRAPH_SET_SLOT = 6,
    TC2LI_MAP_GRAPH_ADD_OBSERVATION = 7,
    TC2LI_MAP_GRAPH_ERASE_OBSERVATION = 8,
    TC2LI_MAP_GRAPH_CLEAR_OBSERVATIONS = 9,
    TC2LI_MAP_GRAPH_OPS = 10
};
typedef struct tc2li_map_graph_edit {
    int32_t op, a, b, c;
} tc2li_map_graph_edit;
/* The ordered edit log of one sequence. */
typedef struct tc2li_map_graph_delta {
    const tc2li_map_graph_edit* edits;
    const double* values;
    int32_t sequence, n_edits, n_values, pad_;
} tc2li_map_graph_delta;
enum tc2li_map_graph_info_field {
    TC2LI_MAP_GRAPH_INFO_KEYFRAMES = 0,
    TC2LI_MAP_GRAPH_INFO_POINTS = 1,
    TC2LI_MAP_GRAPH_INFO_SLOTS = 2,          /* entries of slot_point */
    TC2LI_MAP_GRAPH_INFO_OBSERVATIONS = 3,   /* entries of obs_kf */
    TC2LI_MAP_GRAPH_INFO_APPLIES = 4,        /* applies since the last set; -1: the sequence was never set */
    TC2LI_MAP_GRAPH_INFO_APPLY_BYTES = 5,    /* host-to-device bytes of the last apply that named the sequence, the sequence's share: its
                                              * record, its edits, the values they use */
    TC2LI_MAP_GRAPH_INFO_GATHER_BYTES = 6,   /* host-to-device bytes of the last graph-reading gather that named the sequence, the whole call's:
                                              * problem records, level table, cov_kf.  NOT counted: what the BA after the gather of
                                              * tc2li_ba_window_solve_graph_batch uploads of its own -- the clouds of LiDAR windows, and the
                                              * whole window where one is finished on the host path -- exactly as in tc2li_ba_window_solve_batch */
    TC2LI_MAP_GRAPH_INFO_FIELDS = 7
};
/* capacities [TC2LI_MAP_GRAPH_CAPACITIES], per sequence, fixed for life.  TC2LI_ERR_INVALID for a capacity below 1 or a table of all
 * sequences beyond 2^31 rows; TC2LI_ERR_NO_DEVICE without one. */
int tc2li_map_graph_create(tc2li_keyframe_store* store, int n_sequences, const int32_t* capacities, tc2li_map_graph_handle** out);
int tc2li_map_graph_destroy(tc2li_map_graph_handle* graph);
/* The full state of n sequences (no sequence twice).  The validation is tc2li_ba_window_batch's of the same tables: offsets ascending
 * from 0, slot_point, obs_kf and obs_index in range, observation rows ascending strictly by keyframe row, every kf_slot occupied in the
 * store; kf_flags and point_flags are bytes and kept as given.  TC2LI_ERR_CAPACITY for tables beyond a capacity.  A refused call leaves the
 * graph unchanged.  One upload per call; resident when the call returns. */
int tc2li_map_graph_set_batch(tc2li_map_graph_handle* graph, const int32_t* sequences, const tc2li_map_graph_tables* tables, int n, void* stream);
/* One edit log per named sequence (none twice: TC2LI_ERR_INVALID).  Every edit is checked on the host before any device work, against the
 * row counts, the slot count and store slot of every keyframe row and the observation total -- the host mirrors no table.
 * TC2LI_ERR_INVALID, graph unchanged: an unknown op; a row, slot or values offset out of range; a row named before its append; a point
 * below -1; flags outside a byte; an observation index below -1 or at or beyond the keypoints of the observer's store slot; a store slot
 * that is empty or out of range; a sequence that was never set.  TC2LI_ERR_CAPACITY, graph unchanged: appends beyond a row capacity, slot
 * entries beyond theirs, or observation entries resident now + ADD_OBSERVATION edits in the log > the observation capacity (the host
 * cannot know whether an ADD grows a row; the resident total is exact, each apply downloads 4 bytes per sequence); or a log whose
 * observation edits are too scattered: a touched row finds its edits by walking the log from its first to its last edit, and the sum of
 * those stretches over the points of one log may not exceed tc2li_map_graph_limits' out[5] (one keyframe's worth of edits, one per point,
 * sums to their number; keep a point's edits together, or split the log).
 * Crossing the bus: one 64-byte record per sequence, the edits, the values.  Two kernel launches whatever the number of edits and
 * sequences.  Returns n. */
int tc2li_map_graph_apply_batch(tc2li_map_graph_handle* graph, const tc2li_map_graph_delta* deltas, int n, void* stream);
/* The resident tables of one sequence as host arrays (for tests and tools).  capacities [4] are the caller's arrays' (keyframe rows, slot
 * entries, point rows, observation entries; the offset arrays hold one more than their rows), counts [4] is always written;
 * TC2LI_ERR_CAPACITY when an array is too small. */
int tc2li_map_graph_download(tc2li_map_graph_handle* graph, int sequence, tc2li_map_graph_tables* tables_out, const int32_t* capacities, int32_t* counts);
/* out [TC2LI_MAP_GRAPH_INFO_FIELDS] of one sequence; returns the number written. */
int tc2li_map_graph_info(tc2li_map_graph_handle* graph, int sequence, int64_t* out, int capacity);
/* The sizes at which the apply kernel changes path (for tests): out[0] = the longest observation row (old entries + the row's edits) that
 * is merged in LDS (beyond: in global memory), out[1] = edits per step of the workgroup, out[2] = threads per sequence, out[3] = bytes of
 * the per-sequence record of an apply, out[4] = bytes of the per-problem record of a graph-reading gather, out[5] = the most edit reads
 * the walks of one log's touched rows may sum to.  Returns 6.  Needs no device. */
int tc2li_map_graph_limits(int32_t* out, int capacity);
/* The host twin: the same log applied by plain sequential C++ to host arrays; it defines the result.  tables_out's arrays have
 * capacities [4]; counts [4] receives the sizes.  The checks of tc2li_map_graph_apply_batch except those that need the store (a store
 * slot is only required to be >= 0, an observation index to be >= -1); on an error nothing is written.  Needs no device. */
int tc2li_host_map_graph_apply(const tc2li_map_graph_tables* tables_in, const tc2li_map_graph_edit* edits, int n_edits, const double* values,
                               int n_values, tc2li_map_graph_tables* tables_out, const int32_t* capacities, int32_t* counts);
/* ---- the covisibility graph on the resident map graph (SF/src/KeyFrame.cc:391-486 UpdateConnections, :201-238 AddConnection and
 * UpdateBestCovisibles, :600-603 and :617-618 the covisibility part of SetBadFlag, :699-713 EraseConnection) ------------------------------
 * mConnectedKeyFrameWeights and mvpOrderedConnectedKeyFrames / mvOrderedWeights of every keyframe row as two CSRs per sequence, resident
 * beside the tables above and updated on the device from them:
 *   weights  conn_offsets [n_keyframes + 1], conn_kf, conn_weight: a row ascends strictly by keyframe row, the map order of
 *            tc2li_connections_problem;
 *   ordered  ord_offsets [n_keyframes + 1], ord_kf, ord_weight: the lists as the reference last wrote them.  They are stored, not derived:
 *            the reference leaves a list stale when AddConnection returns at :209-210, and leaves bad keyframes out of it at :229.
 * The spanning tree (mpParent, mspChildrens, mbFirstConnection) stays with the caller, as for tc2li_update_connections_batch.
 * Keyframe rows that ADD_KEYFRAME appends after the connections were set have empty rows in both CSRs, with no further call;
 * tc2li_map_graph_set_batch on a sequence empties its connections.  Until tc2li_map_graph_connections_reserve has been called every entry
 * of this section returns TC2LI_ERR_INVALID and the graph behaves as without it. */
typedef struct tc2li_map_graph_connections {
    int32_t* conn_offsets;
    int32_t* conn_kf;
    int32_t* conn_weight;
    int32_t* ord_offsets;
    int32_t* ord_kf;
    int32_t* ord_weight;
    int32_t n_keyframes, pad_;
} tc2li_map_graph_connections;
enum tc2li_map_graph_connections_info_field {
    TC2LI_MAP_GRAPH_CONNECTIONS_WEIGHT_ENTRIES = 0,   /* entries of conn_kf */
    TC2LI_MAP_GRAPH_CONNECTIONS_ORDERED_ENTRIES = 1,  /* entries of ord_kf */
    TC2LI_MAP_GRAPH_CONNECTIONS_UPDATES = 2,          /* update and erase calls that named the sequence and succeeded, since its last set */
    TC2LI_MAP_GRAPH_CONNECTIONS_UPDATE_BYTES = 3,     /* host-to-device bytes of the last update or erase that named the sequence, its share */
    TC2LI_MAP_GRAPH_CONNECTIONS_INFO_FIELDS = 4
};
/* Once per graph: allocates both CSRs (two generations each, see tc2li_map_graph_update_connections_batch) with room for
 * entries_per_sequence entries per sequence and CSR.  TC2LI_ERR_INVALID for a second call, a capacity below 1 or tables of all sequences
 * beyond 2^31 entries. */
int tc2li_map_graph_connections_reserve(tc2li_map_graph_handle* graph, int entries_per_sequence);
/* The full connection state of n sequences (none twice; each must have been set by tc2li_map_graph_set_batch).  TC2LI_ERR_INVALID, the
 * graph unchanged: n_keyframes negative or beyond the sequence's resident keyframe rows (rows beyond n_keyframes are empty); offsets that
 * do not ascend from 0; a keyframe out of [0, n_keyframes); a weight row that does not ascend strictly; an ordered row that names a
 * keyframe twice; a row of either CSR that names its own keyframe.  TC2LI_ERR_CAPACITY, the graph unchanged: a CSR beyond the reserve.
 * One upload per call; resident when the call returns.  Returns n. */
int tc2li_map_graph_set_connections_batch(tc2li_map_graph_handle* graph, const int32_t* sequences, const tc2li_map_graph_connections* tables, int n,
                                          void* stream);
/* The resident connections of one sequence as host arrays (for tests and tools), n_keyframes = the sequence's resident keyframe rows.
 * capacities [2]: weight entries, ordered entries of the caller's arrays (the offset arrays hold the keyframe rows + 1); counts [2] is
 * always written; TC2LI_ERR_CAPACITY when an array is too small. */
int tc2li_map_graph_download_connections(tc2li_map_graph_handle* graph, int sequence, tc2li_map_graph_connections* out, const int32_t* capacities,
                                         int32_t* counts);
/* out [TC2LI_MAP_GRAPH_CONNECTIONS_INFO_FIELDS] of one sequence; returns the number written. */
int tc2li_map_graph_connections_info(tc2li_map_graph_handle* graph, int sequence, int64_t* out, int capacity);
/* out[0] = bytes of the per-sequence record that an update or an erase sends to the device -- all it sends; out[1] = bytes per sequence
 * that come back beside the counts block (the status words).  Returns 2.  Needs no device. */
int tc2li_map_graph_connections_limits(int32_t* out, int capacity);
/* One KeyFrame::UpdateConnections (:391-486) per named sequence (none twice: TC2LI_ERR_INVALID), on the resident tables and into them.
 * The inputs of tc2li_connections_problem come from the graph: kf_flags are the graph's (bits 0 and 1 mean the same), slot_point is the
 * slot row of current_rows[i], point_bad is bit 0 of point_flags, the observation rows are the resident ones, the weight rows the resident
 * weights, is_init_kf is kf_id[current] == init_kf_id[i]; first_connection [n] is mbFirstConnection.  The rules are those written under
 * tc2li_update_connections_batch, line for line -- votes per slot, the empty-counter return, th = 15 with the lone best keyframe
 * otherwise (the lowest row among equals), the whole counter as the weight row, equal weights ordered by row descending, AddConnection's
 * early return leaving a neighbour's ordered list as it is -- and the same device functions compute them.
 *   counts_out [n][TC2LI_CONNECTIONS_COUNTS]: that entry's counts block, PARENT included; the caller still does AddChild and clears
 *   mbFirstConnection.
 *   Status UPDATED: current's weight row := the counter; current's ordered row := the new list; every touched keyframe's weight row gets
 *   (current, weight) inserted at its place or overwritten; every touched keyframe with changed = 1 gets its ordered row replaced by the
 *   UpdateBestCovisibles result.  Status UNCHANGED: nothing is written.
 *   TC2LI_ERR_CAPACITY when a CSR of some sequence would pass the reserve: NO sequence is changed, and of every sequence's counts block
 *   entries 6 and 7 (0 otherwise) hold the weight and the ordered entries its CSRs would hold.  Both CSRs have two generations per
 *   sequence: the kernels read the current one and write the other whole, and the host makes the written one current only after every
 *   sequence of the call has reported that it fitted.
 *   TC2LI_ERR_INVALID before any launch: no reserve, a sequence out of range, never set or named twice, a current row out of range, more
 *   than 65535 sequences.
 * Crossing the bus: host to device one record per sequence (tc2li_map_graph_connections_limits' out[0] bytes) and nothing else; device to
 * host the counts blocks and out[1] bytes of status per sequence.  No table, list or weight row crosses in either direction.  Three
 * kernel launches whatever n.  The results are resident and counts_out is written when the call returns.  Returns n. */
int tc2li_map_graph_update_connections_batch(tc2li_map_graph_handle* graph, const int32_t* sequences, const int32_t* current_rows,
                                             const uint8_t* first_connection, const int64_t* init_kf_id, int n, int32_t* counts_out, void* stream);
/* What KeyFrame::SetBadFlag does to covisibility (:600-603, :617-618) for keyframe rows[i] of sequence sequences[i] (none twice): for
 * every keyframe k of the row's weight row, the row's entry is removed from k's weight row if it is there (EraseConnection, :699-713), and
 * where it was, k's ordered row is replaced by UpdateBestCovisibles (:216-238) under the resident kf_flags as they are at the call -- the
 * reference sets mbBad afterwards, at :685; a neighbour that did not hold the entry keeps its ordered row.  Then both rows of the keyframe
 * itself are emptied.  Flags, observations, slots and the repair of the spanning tree are not part of it: the caller sends those as
 * edits.  Bus contract and atomicity as tc2li_map_graph_update_connections_batch.  Returns n. */
int tc2li_map_graph_erase_connections_batch(tc2li_map_graph_handle* graph, const int32_t* sequences, const int32_t* rows, int n, void* stream);
/* The host twins: plain sequential C++ over host copies of the graph tables and the connection tables; they define the result and need
 * no device.  in->n_keyframes may be below tables->n_keyframes (the rows beyond are empty); out has tables->n_keyframes rows, arrays with
 * room for capacities [2] (weight entries, ordered entries) and tables->n_keyframes + 1 offsets.  sizes [2] receives the entries of both
 * CSRs after the call, also with TC2LI_ERR_CAPACITY, when nothing else is written.  The update writes counts [TC2LI_CONNECTIONS_COUNTS]
 * and returns its status; with UNCHANGED out is a copy of in.  TC2LI_ERR_INVALID for tables or connections that
 * tc2li_map_graph_set_batch (the store apart) or tc2li_map_graph_set_connections_batch would refuse, and a row out of range. */
int tc2li_host_map_graph_update_connections(const tc2li_map_graph_tables* tables, const tc2li_map_graph_connections* in, int32_t current,
                                            int first_connection, int64_t init_kf_id, tc2li_map_graph_connections* out, const int32_t* capacities,
                                            int32_t* sizes, int32_t* counts);
int tc2li_host_map_graph_erase_connections(const tc2li_map_graph_tables* tables, const tc2li_map_graph_connections* in, int32_t row,
                                           tc2li_map_graph_connections* out, const int32_t* capacities, int32_t* sizes);

/* tc2li_ba_window_batch with the tables of problem p taken from sequence sequences[p] of the graph.
 * NOTE: of a problem only current, cov_kf / n_cov, init_kf_id, the outputs and the capacities are read.  ITS TABLE POINTERS, n_keyframes
 * AND n_points ARE IGNORED WITHOUT AN ERROR: a caller who also passes tables gets the graph's, never its own, however stale they are.
 * Pass NULL and 0 there.  Every output, count,
 * status and error is bit for bit that of tc2li_ba_window_batch given the tables tc2li_map_graph_download returns -- the same kernels read
 * the same layout.  Several problems may name one sequence.  Uploaded: the problem records, cov_kf and the level table; no table.  Per
 * call the host checks in O(n_keyframes) that the store slots of the sequence's keyframe rows are occupied and hold no octave beyond
 * n_levels and hold no fewer keypoints than when the rows' observation indices were checked (a slot put again with fewer is refused:
 * TC2LI_ERR_INVALID), and current and cov_kf. */
int tc2li_ba_window_graph_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences, const tc2li_ba_window_problem* problems,
                                int n_problems, const float* inv_level_sigma2, int n_levels, void* stream);
/* The same step for tc2li_ba_window_solve_batch: stop flag, stats, clouds, erase lists as there. */
int tc2li_ba_window_solve_graph_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                                      const tc2li_ba_window_solve_problem* problems, int n_problems, const float* inv_level_sigma2, int n_levels,
                                      const tc2li_camera* cam, int group, int32_t* results);

/* tc2li_ba_window_graph_batch with the neighbour list of every problem taken from the graph as well: GetVectorCovisibleKeyFrames()
 * (SF/src/OptimizerWithLidar.cc:69, SF/src/Optimizer.cc:1127) is the resident ordered row of `current` (tc2li_map_graph_connections), in
 * its order -- a keyframe of it that is bad or of another map is marked local and not optimised (:73-74), as one of an uploaded list is.
 * cov_kf / n_cov of every problem must be NULL / 0, and the connections must have been reserved: TC2LI_ERR_INVALID otherwise.  Every
 * output, count, status and error is bit for bit that of tc2li_ba_window_graph_batch given cov_kf = that row as
 * tc2li_map_graph_download_connections returns it: the same kernels, which read the list through the sequence's ordered CSR in place of an
 * uploaded array.  GATHER_BYTES is smaller by exactly the 4 * n_cov bytes no longer sent: the problem records and the level table are all
 * that goes up. */
int tc2li_ba_window_graph_cov_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                                    const tc2li_ba_window_problem* problems, int n_problems, const float* inv_level_sigma2, int n_levels, void* stream);

/* ---- local mapping: the closing step of LocalLVBundleAdjustment, "Recover optimized data" (SF/src/OptimizerWithLidar.cc:455-485), on the
 * resident graph -----------------------------------------------------------------------------------------------------------------------
 * The reference ends its local BA by writing into the map: EraseMapPointMatch / EraseObservation for every pair of vToErase (:458-465),
 * SetPose for every local keyframe (:468-475), SetWorldPos for every local point (:478-484).  tc2li_host_ba_window_commit_log states that
 * step as an edit log of the map graph and so defines it; tc2li_ba_window_solve_graph_commit_batch is tc2li_ba_window_solve_graph_batch
 * followed by that log on the resident tables, the optimised values never leaving the device for it.
 *
 * The log of one solved window, applied by tc2li_host_map_graph_apply to the sequence's tables as they were before the solve:
 *   1. for every erase pair i in the order of erase_pose / erase_point: SET_SLOT(kf row, index, -1), then ERASE_OBSERVATION(point row,
 *      kf row), with kf row = pose_row[erase_pose[i]], point row = point_row[erase_point[i]] and index the obs_index stored for that
 *      keyframe row in the point's observation row (KeyFrame::EraseMapPointMatch(MapPoint*) goes through GetIndexInKeyFrame, :461-462).
 *      Where the keyframe row holds no slot of that index -- a row whose matches are not resident: the gather reads the slots of the
 *      current keyframe and of cov_kf only, and a graph may leave the others empty -- there is nothing to clear and the SET_SLOT is left out;
 *   2. SET_POSE(pose_row[i], poses7_out[i]) for every pose with fixed[i] == 0, in pose order (:468-475);
 *   3. SET_POSITION(point_row[j], points3_out[j]) for every listed point, in order (:478-484).
 * The values are those of the arrays bit for bit, except under TC2LI_BA_COMMIT_POSITIONS_F32, where every position component is
 * (double)(float)x, the cast<float>() of :482.  Poses are never rounded: Sophus::SE3f's constructor renormalises, which stays with the
 * caller, who may send a SET_POSE of its own.
 * A window is committed when its status is TC2LI_BA_WINDOW_OK and its result is >= 0 -- also with result 0 because iterations == 0 or
 * the stop flag was raised: the reference recovers the data then too.  An ABORTED window and a window with a negative result give no
 * edit.
 * NOT part of the step (the graph stores literal edits, as its contract says): what the reference chains onto an erase -- nObs <= 2
 * turning the point bad (MapPoint.cc:203-209), a changed mpRefKF, UpdateNormalAndDepth, IncreaseChangeIndex.  The caller spells these out
 * in its next log from the erase lists, which are returned as before.  The inertial windows and the other readers of the graph have no
 * such entry yet. */
#define TC2LI_BA_COMMIT_POSITIONS_F32 1u
/* Host only, needs no device.  tables: the sequence's tables before the solve; problem: a problem of tc2li_ba_window_solve_batch after
 * the call, of which window.counts, pose_row, fixed, poses7_out, point_row, points3_out, erase_pose, erase_point, n_erase and
 * erase_capacity are read; result: the call's results[] entry of the problem.  edits [edit_capacity], values [value_capacity].
 * n_edits and n_values receive the sizes of the log (n_edits may be NULL); returns the number of edits.  TC2LI_ERR_CAPACITY, the sizes
 * written and nothing else, when an array is too small or *n_erase exceeds erase_capacity (the lists are then cut).  TC2LI_ERR_INVALID,
 * nothing written: unknown flag bits, NULL n_erase, a pose_row / point_row outside the tables, an erase index outside the counts, an
 * erase pair whose keyframe row is not in the point's observation row. */
int tc2li_host_ba_window_commit_log(const tc2li_map_graph_tables* tables, const tc2li_ba_window_solve_problem* problem, int32_t result,
                                    uint32_t flags, tc2li_map_graph_edit* edits, int edit_capacity, double* values, int value_capacity,
                                    int32_t* n_edits, int32_t* n_values);
/* tc2li_ba_window_solve_graph_batch -- every output, count, result and error as there, bit for bit; poses, points and erase lists are
 * downloaded as there -- and then, for every committed window p, the log above on sequence sequences[p].
 *   n_erase must be non-NULL in every problem (the commit is defined by the outlier rule) and no sequence may be named twice (the local
 *   mapping of a map is one thread): TC2LI_ERR_INVALID.  So are unknown bits of flags.
 *   On any error of the whole call no sequence is changed, the late TC2LI_ERR_CAPACITY of an erase_capacity that turns out too small
 *   included.  The graph's lock is held for the whole call.
 *   Windows the lock-step group solved on the device: a scatter kernel writes poses and positions from the device copy of the final
 *   estimate, a second kernel turns the device copy of the erase pairs into an edit log in device memory (one wavefront per window, the
 *   index by bisection of the point's observation row) and the kernels of tc2li_map_graph_apply_batch apply it.  Host to device: one
 *   64-byte record per sequence, no value, no table, no edit.  A window without erase pairs gets no rebuild of the observation CSR.
 *   Should the erase pairs of one window name single points so far apart that tc2li_map_graph_apply_batch would refuse the log
 *   (tc2li_map_graph_limits' out[5]), the call returns TC2LI_ERR_CAPACITY with no sequence changed; the outputs are written.
 *   Windows finished on the host path (see tc2li_ba_window_solve_batch): their sequence's tables are downloaded, the log is built by
 *   tc2li_host_ba_window_commit_log and goes through the apply.
 *   tc2li_map_graph_info: APPLIES goes up by one per committed sequence; APPLY_BYTES is what the commit moved host to device for the
 *   sequence (64, or the record and the log of a host-path window); GATHER_BYTES as tc2li_ba_window_solve_graph_batch counts it. */
int tc2li_ba_window_solve_graph_commit_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                                             const tc2li_ba_window_solve_problem* problems, int n_problems, const float* inv_level_sigma2,
                                             int n_levels, const tc2li_camera* cam, int group, uint32_t flags, int32_t* results);

/* tc2li_ba_window_solve_graph_commit_batch with the neighbour lists taken from the graph as tc2li_ba_window_graph_cov_batch takes them
 * (cov_kf / n_cov of every window NULL / 0).  Results, outputs and the graph afterwards are bit for bit those of
 * tc2li_ba_window_solve_graph_commit_batch given cov_kf = the resident ordered row of every window's current keyframe.  The commit writes
 * poses, positions, slots and observations; the connections are not touched by it. */
int tc2li_ba_window_solve_graph_commit_cov_batch(tc2li_keyframe_store* store, tc2li_map_graph_handle* graph, const int32_t* sequences,
                                                 const tc2li_ba_window_solve_problem* problems, int n_problems, const float* inv_level_sigma2,
                                                 int n_levels, const tc2li_camera* cam, int group, uint32_t flags, int32_t* results);

/* ---- local mapping: the window of the inertial local BA (OptimizerWithLidar::LocalLVIBA, SF/src/OptimizerWithLidar.cc:489-607 the gather,
 * :632-727 the vertices and the keyframes of the LiDAR edge, :729-800 the inertial links, :832-969 the point vertices and edges, :985-1045
 * the outlier rule; the twin Optimizer::LocalInertialBA, SF/src/Optimizer.cc:1512-1631 and on) -------------------------------------------
 * The graph walk that turns "the current keyframe" into the arrays of tc2li_local_inertial_bundle_adjustment /
 * tc2li_local_lvi_bundle_adjustment / tc2li_lvi_problem, on the flat graph of tc2li_ba_window_problem, for many sequences at once.  Line
 * numbers below are OptimizerWithLidar.cc's.  The two reference functions were compared line by line: gather, vertices, links, edges and
 * outlier rule are the same text; they differ in the LiDAR edge alone (:697-727), which `with_lidar` selects.  It is NOT the visual gather
 * with another list: it follows mPrevKF, tests points with isBad() only, may turn its oldest keyframe into the fixed one, picks fixed
 * observers greedily up to 200, and takes the LiDAR keyframes by position.  maxCovKF is 0 and the loop of :557-584 breaks on entry
 * (size() >= 0), so GetVectorCovisibleKeyFrames() is never read and the problem has no cov_kf.  Not covered: the two-camera branch
 * (:934-966). */
enum tc2li_inertial_window_status {
    TC2LI_INERTIAL_WINDOW_OK = 0,
    TC2LI_INERTIAL_WINDOW_EMPTY = 1      /* the window was one keyframe without predecessor: :553 popped it and nothing is left to optimise */
};
enum tc2li_inertial_window_count {
    TC2LI_INERTIAL_WINDOW_STATUS = 0,        /* tc2li_inertial_window_status */
    TC2LI_INERTIAL_WINDOW_N_FIXED_KF = 1,    /* lFixedKeyFrames.size(): the keyframe of :542-554 and the picks of :586-607 */
    TC2LI_INERTIAL_WINDOW_N_OPT_KF = 2,      /* vpOptimizableKFs.size() after :553 (N of :633) */
    TC2LI_INERTIAL_WINDOW_N_VERTICES = 3,    /* entries of kf_row / keyframes_out / fixed / has_imu: the two above added */
    TC2LI_INERTIAL_WINDOW_N_POINTS = 4,      /* entries of point_row / points3_out: lLocalMapPoints.size() */
    TC2LI_INERTIAL_WINDOW_N_EDGES = 5,       /* entries of edges */
    TC2LI_INERTIAL_WINDOW_N_LINKS = 6,       /* entries of links / link_kf2_row */
    TC2LI_INERTIAL_WINDOW_N_LIDAR = 7,       /* entries of lidar_pose_index: 0 or 6 */
    TC2LI_INERTIAL_WINDOW_N_POINTS_WITHOUT_EDGE = 8,   /* listed points that got no edge */
    TC2LI_INERTIAL_WINDOW_N_VERTICES_UNDER_3_EDGES = 9,   /* vertices with mVisEdges < 3: the assert of :972-975, reported and not enforced */
    TC2LI_INERTIAL_WINDOW_COUNTS = 10
};
#define TC2LI_INERTIAL_WINDOW_MAX_LIDAR 6    /* N1 of :712 */
#define TC2LI_INERTIAL_WINDOW_MAX_OPT 25     /* maxOpt of :497 */
#define TC2LI_INERTIAL_WINDOW_MAX_FIXED 200  /* maxFixKF of :586 */
/* One call of the gather for one current keyframe.  All pointers are host memory, the arrays are copied by the call; indices are rows of the
 * problem's own tables; problems of one batch are independent.  The row order of the keyframes stands in for the address order of the
 * reference's std::map<KeyFrame*, ...>, as in tc2li_ba_window_problem.
 *   keyframes (n_keyframes rows: the current keyframe, its chain of predecessors, every observer of their points):
 *     kf_slot   the slot of the keyframe in the store (the host entry: the index into views)
 *     kf_id     mnId
 *     kf_flags  bit 0 isBad(), bit 1 GetMap() != pCurrentMap, bit 2 bImu, bit 3 mpImuPreintegrated != NULL
 *     prev_kf   the row of mPrevKF, -1 = NULL
 *     states    [n_keyframes] what the optimiser takes of a keyframe; read only for the rows that get a vertex
 *     slot_offsets [n_keyframes + 1], slot_point: GetMapPointMatches() per keyframe as a CSR, -1 = NULL.  Only the rows of the window
 *     keyframes are read; others may be empty.
 *   points (n_points rows): point_flags bit 0 isBad() (no other bit is read: :532 has no map test); positions [n_points][3] GetWorldPos()
 *     widened; CSR obs_offsets [n_points + 1], obs_kf, obs_index: GetObservations(), a row ascending strictly by keyframe row, obs_index =
 *     get<0> of the tuple (the left keypoint, or -1)
 *   current: the row of pKF;  keyframes_in_map: pCurrentMap->KeyFramesInMap();  large, rec_init: bLarge, bRecInit;  with_lidar: non-zero =
 *     LocalLVIBA, 0 = LocalInertialBA
 * Out (capacities are the caller's; an array whose capacity is 0 may be NULL):
 *   counts [TC2LI_INERTIAL_WINDOW_COUNTS]: always written.  EMPTY: N_FIXED_KF is 1, every later count is 0 and NO OTHER OUTPUT IS WRITTEN.
 *   kf_row, keyframes_out, fixed, has_imu [kf_capacity]: the optimisable keyframes and the fixed ones ascending by kf_id (by row among equal
 *     ids) -- the vertex-id order tc2li_local_inertial_bundle_adjustment asks for; has_imu = bit 2 of kf_flags
 *   point_row [point_capacity], points3_out [point_capacity][3]: lLocalMapPoints in the reference's order
 *   edges [edge_capacity]: one per observation in creation order; point / pose index the two lists above
 *   links, link_kf2_row [link_capacity]: the inertial links in the order of :734 (the current keyframe's first); kf1 / kf2 index the vertex
 *     list, preintegrated is NULL: the caller sets it to the mpImuPreintegrated of row link_kf2_row[i], after
 *     SetNewBias(mPrevKF->GetImuBias()) (:745)
 *   lidar_pose_index [TC2LI_INERTIAL_WINDOW_MAX_LIDAR]: the vertices of vpOptimizableKFs[0 .. n_lidar), -1 beyond */
typedef struct tc2li_inertial_window_problem {
    const int32_t* kf_slot;
    const int64_t* kf_id;
    const uint8_t* kf_flags;
    const int32_t* prev_kf;
    const tc2li_inertial_keyframe* states;
    const int32_t* slot_offsets;
    const int32_t* slot_point;
    const uint8_t* point_flags;
    const double* positions;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int32_t* obs_index;
    int32_t* counts;
    int32_t* kf_row;
    tc2li_inertial_keyframe* keyframes_out;
    uint8_t* fixed;
    uint8_t* has_imu;
    int32_t* point_row;
    double* points3_out;
    tc2li_ba_edge* edges;
    tc2li_inertial_link* links;
    int32_t* link_kf2_row;
    int32_t* lidar_pose_index;
    int32_t n_keyframes, n_points, current, keyframes_in_map;
    int32_t large, rec_init, with_lidar;
    int32_t kf_capacity, point_capacity, edge_capacity, link_capacity;
    int32_t pad_;
} tc2li_inertial_window_problem;
/* The gather for n_problems current keyframes at once on the device.  Line for line:
 *   temporal window (:493-519): Nd = min(keyframes_in_map - 2, large ? 25 : 10).  The current keyframe is taken whatever Nd is (:508), then
 *   mPrevKF is followed while i < Nd and a predecessor exists.  No flag of any keyframe is tested.
 *   points (:524-539): the window keyframes in list order, their slots ascending; a point that is not NULL and not bad is listed at its
 *   first occurrence.  A point of another map IS listed.
 *   fixed keyframe (:542-554): the predecessor of the last window keyframe, whatever its flags; without one, the last window keyframe
 *   itself leaves the window (its points stay listed) and is the first fixed keyframe.  A window of one such keyframe is EMPTY.
 *   fixed observers (:586-607), a sequential rule: for the listed points in order, the observers ascending by row; the first observer that
 *   carries neither the local nor the fixed mark gets the fixed mark WHETHER IT IS BAD OR NOT; if it is not bad it joins the fixed keyframes
 *   and the point is done, if it is bad the point's next observer is looked at.  No map test.  After every point the walk stops if the
 *   fixed keyframes are 200 or more, the one of :542-554 included.  A bad keyframe with the mark passes :862 and is dropped by :865: no
 *   vertex, no edge.
 *   vertices (:632-696): the window keyframes (free) and the fixed keyframes (fixed); setId(mnId) is what orders them.
 *   LiDAR keyframes (:699-727, with_lidar only): N > 5: vpOptimizableKFs[0 .. 6) BY POSITION; vLiDAROptKeyFrames (those with a surface
 *   cloud) is computed and never used, so no cloud bit is read.  Otherwise none.
 *   links (:734-800): for window keyframe i with a predecessor, bit 2 of both and bit 3 of its own: kf1 = the predecessor's vertex, kf2 =
 *   its own, robust = (i == N-1) || rec_init, info_scale = 1e-2 for i == N-1, else 1.  The lookups of :746-759 cannot fail: the predecessor
 *   of window keyframe i < N-1 is window keyframe i+1, and the predecessor of the last one is the fixed keyframe of :542-554 in either arm;
 *   both have a vertex, and the velocity / bias vertices exist where bit 2 is set (:643, :681), which the link already requires.
 *   edges (:845-969): the listed points in order, the observers ascending by row; an observer needs one of the two marks (:862) and must be
 *   neither bad nor of another map (:865); obs_index -1 makes no edge; u_right < 0 a monocular edge, else stereo; inv_sigma2 =
 *   inv_level_sigma2[octave] (Pinhole::uncertainty2 is 1.0f).  mVisEdges is kept per row, not per mnId.
 * Marks and first-occurrence keys live in LDS up to the sizes tc2li_inertial_window_limits reports, in global memory beyond.  Two kernel
 * launches, one upload and one download for the whole batch; the results are in host memory when the call returns (stream: NULL = the
 * calling thread's private stream).  TC2LI_ERR_INVALID before any launch for negative sizes or capacities, NULL required pointers,
 * offsets that do not ascend from 0, indices out of range (current, prev_kf below -1 or >= n_keyframes, slot_point below -1, obs_kf,
 * obs_index below -1 or beyond the keypoints of the observer's slot), observation rows that do not ascend strictly, a kf_slot that is
 * empty or out of range, a slot that holds an octave outside [0, n_levels), and a prev_kf chain that, within the window and the one
 * predecessor behind it, returns to a keyframe already in the window.  TC2LI_ERR_CAPACITY when a list of some problem does not fit: then
 * counts is written for every problem, with the sizes needed, and no list for any.  Returns n_problems; 0 for an empty batch. */
int tc2li_inertial_window_batch(tc2li_keyframe_store* store, const tc2li_inertial_window_problem* problems, int n_problems,
                                const float* inv_level_sigma2, int n_levels, void* stream);
/* The same contract as plain sequential C++ with the reference's mark fields (one problem per worker thread).  kf_slot indexes views
 * [n_views], of which n, keys and u_right are read (n < 0: an empty slot).  Needs no device. */
int tc2li_host_inertial_window_batch(const tc2li_keyframe_view* views, int n_views, const tc2li_inertial_window_problem* problems,
                                     int n_problems, const float* inv_level_sigma2, int n_levels);
/* The sizes at which tc2li_inertial_window_batch changes path (for tests): out[0] = the largest n_keyframes whose marks are kept in LDS
 * (beyond: in global memory), out[1] = the largest n_points whose first-occurrence keys are kept in LDS (beyond: in global memory),
 * out[2] = threads per problem.  Returns 3.  Needs no device.  No reference counterpart. */
int tc2li_inertial_window_limits(int32_t* out, int capacity);
/* The outlier rule after the BA (:985-1045), host only: vToErase as (pose index, point index) pairs in the reference's order.  The
 * rejection of :1028 comes first: *rejected = (2 * err < err_end || isnan(err) || isnan(err_end)) && !large with err / err_end =
 * (float)initial_chi2 / (float)final_chi2; a rejected window returns 0 pairs (the reference returns before any erasure and any write-back).
 * Otherwise the monocular edges (u_right < 0) in creation order, erased if (chi2 > chi2Mono2 && !close) || (chi2 > 1.5f * chi2Mono2 &&
 * close) || !depthPositive with close = track_depth[point] < 10.f (:994-999), then the stereo edges, erased if chi2 > chi2Stereo2 alone --
 * no depth test (:1016).  The thresholds are the reference's float variables widened: (double)5.991f, (double)(1.5f * 5.991f),
 * (double)7.815f.  Edges of a point with point_bad_now are skipped.  track_depth [n_points] = pMP->mTrackDepth.  Returns the count;
 * TC2LI_ERR_CAPACITY (nothing written but *rejected) when it exceeds capacity, TC2LI_ERR_INVALID for an edge whose point is outside
 * [0, n_points). */
int tc2li_inertial_window_outliers(const tc2li_ba_edge* edges, const double* edge_chi2, const uint8_t* edge_depth_positive, int n_edges,
                                   const uint8_t* point_bad_now, const float* track_depth, int n_points, double initial_chi2,
                                   double final_chi2, int large, int32_t* rejected, int32_t* erase_pose, int32_t* erase_point, int capacity);

/* ---- local mapping: the inertial term of local-BA windows ----------------------------------------------------------------------------
 * The inertial edges of a window -- EdgeInertial, EdgeGyroRW and EdgeAccRW per link (SF/src/G2oTypes.cc:499-601, SF/include/G2oTypes.h:645-714)
 * -- evaluated at given states for many windows at once: the robust cost and, with linearize, the normal equations.  The values per link
 * are those the inertial local BA uses (tc2li_local_inertial_bundle_adjustment): information = inverse of C(0:9, 0:9), symmetrised,
 * eigenvalues below 1e-12 cleared, times info_scale; random-walk informations = the inverses of the two 3 x 3 bias-walk blocks of C; Huber
 * with sqrtf(16.92f) on the inertial edge where `robust`, never on the random-walk edges.  A building block: the LM loop of the inertial
 * windows does not call it yet.
 * Unknowns of a keyframe (15): pose 6 (the body-frame update of VertexPose) | velocity 3 | gyro bias 3 | acc bias 3.
 *   chi2 [1]: the sum over the links, in link order, of rho(e' Omega e) + the two random-walk costs
 *   H_diag [n_keyframes][15][15] row-major: per keyframe the sum, in link order, of the diagonal contributions of every link that touches
 *     it, the random-walk informations on the bias diagonals included.  For kf2 the inertial edge has pose and velocity columns only.
 *   H_link [n_links][15][15]: link l's off-diagonal block, rows = kf1's unknowns, columns = kf2's; the transpose is implied
 *   b [n_keyframes][15] = -J' (rho' Omega) e
 * Rows and columns of a fixed keyframe are zero (so is H_link of a link with a fixed end), and the whole block of a keyframe no link
 * touches.  With linearize == 0 only chi2 is written and H_diag, H_link, b may be NULL. */
typedef struct tc2li_inertial_term_problem {
    const tc2li_inertial_keyframe* keyframes;   /* [n_keyframes] the state the term is evaluated at */
    const uint8_t* fixed;                       /* [n_keyframes] as tc2li_local_inertial_bundle_adjustment */
    const uint8_t* has_imu;                     /* [n_keyframes] */
    const tc2li_inertial_link* links;           /* [n_links] */
    int32_t n_keyframes, n_links;
    double* chi2;
    double* H_diag;
    double* H_link;
    double* b;
} tc2li_inertial_term_problem;
/* On the device: one upload, the launches, one download; the results are in host memory when the call returns (stream: NULL = the calling
 * thread's private stream).  The information matrices are prepared on the host, once per link and call.  A window's results are the same
 * bits alone and anywhere in any batch, and from call to call.  TC2LI_ERR_INVALID before any launch, naming the window and the link, and
 * with no output written: a link's keyframe index out of range, kf1 == kf2, a link to a keyframe with has_imu == 0, a NULL
 * pre-integration, a covariance that is not positive definite, NULL arrays, sizes that are negative or beyond
 * tc2li_inertial_term_limits.  Returns n_problems. */
int tc2li_inertial_term_batch(const tc2li_inertial_term_problem* problems, int n_problems, int linearize, void* stream);
/* The same contract on host threads: the same per-link arithmetic and the same sums in the same order (the two differ by the compilers'
 * contraction and the math libraries only).  Needs no device. */
int tc2li_host_inertial_term_batch(const tc2li_inertial_term_problem* problems, int n_problems, int linearize);
/* out[0] = the most keyframes, out[1] = the most links a window may have.  Returns 2.  Needs no device.  No reference counterpart. */
int tc2li_inertial_term_limits(int32_t* out, int capacity);

/* ---- tracking: stereo map points and the keyframe decision (SF/src/Tracking.cc:2942-3076 NeedNewKeyFrame, :3078-3212 CreateNewKeyFrame,
 * :2676-2734 UpdateLastFrame, :2477-2495 StereoInitialization) ----------------------------------------------------------------------------
 * The step between TrackLocalMap and local mapping: whether the frame becomes a keyframe, and which of its stereo keypoints become new map
 * points, with their world positions.  The library returns the decision, the keypoints in creation order and their positions; the caller
 * makes the objects (INTEGRATION.md "NeedNewKeyFrame / CreateNewKeyFrame / UpdateLastFrame / StereoInitialization").  Rig: pinhole stereo,
 * Nleft == -1, mpCamera2 == nullptr; the fisheye / two-camera branches (:2496-2517, :3171-3184, :3019) are not covered. */
enum tc2li_stereo_points_mode {
    TC2LI_STEREO_POINTS_CLOSEST = 0,   /* CreateNewKeyFrame (:3132-3203) and UpdateLastFrame (:2676-2734): the depth-sorted walk */
    TC2LI_STEREO_POINTS_ALL = 1        /* StereoInitialization (:2477-2495): every keypoint with depth, if the frame has more than 500 */
};
#define TC2LI_STEREO_POINTS_MAX_KEYPOINTS 4096
/* One frame.  All pointers are host memory, the arrays are copied by the call.
 *   n keypoints (Frame::N; more than 4096: TC2LI_ERR_CAPACITY);  depth [n] mvDepth;  keys [n] mvKeysUn (only x, y are read);
 *   held [n] as in tc2li_track_local_map_batch: 0 = mvpMapPoints[i] is NULL, 1 = a point with Observations() > 0, 2 = a point without
 *   observations;  outlier [n] mvbOutlier (read only by the counts of tc2li_new_keyframe_batch; may be NULL for tc2li_stereo_points_batch);
 *   Rwc [9] mRwc row-major and Ow [3] mOw as Frame::UpdatePoseMatrices left them (SF/src/Frame.cc:505-506);  th_depth mThDepth;
 *   max_point 100 at both sites (:2731, :3128);  mode tc2li_stereo_points_mode.
 * Out: created_keypoint [n] and x3D [n][3] (room for n; the first n_created entries are written, in creation order), counts [3] =
 * n_created, n_visited (nPoints when the walk ended; in mode ALL = n_created), n_with_depth (keypoints with depth > 0). */
typedef struct tc2li_stereo_points_frame {
    const float* depth;
    const tc2li_keypoint* keys;
    const uint8_t* held;
    const uint8_t* outlier;
    int32_t* created_keypoint;
    float* x3D;
    int32_t* counts;
    float Rwc[9];
    float Ow[3];
    float th_depth;
    int32_t n, max_point, mode;
} tc2li_stereo_points_frame;
/* The stereo map points of n_frames frames (one per sequence) at once on the device.  unproject4 = {cx, cy, invfx, invfy} as floats, as
 * Frame holds them (invfx = 1.0f / fx, SF/src/Frame.cc:188).
 *   CLOSEST: the pairs (depth[i], i) with depth[i] > 0 (NaN fails the test, +inf passes) in the order of std::sort on pair<float, int>:
 *   by depth, ties by index -- a total order, the result is unique.  The walk visits them in that order, nPoints counts every entry, an
 *   entry with held != 1 is created (:3156-3162, :2704-2707), and the walk ends AFTER an entry with depth > th_depth && nPoints >
 *   max_point (:3199, :2731).  So with c entries of depth <= th_depth out of M it takes min(M, max(c, max_point) + 1) entries: one more
 *   than max_point, or all close ones and one far one.  That is the reference's behaviour.
 *   ALL: every i with depth[i] > 0 in index order, held is ignored; nothing when n <= 500 (:2433).
 *   Position of keypoint i (Frame::UnprojectStereo, SF/src/Frame.cc:1037-1050), float, every product and sum rounded (no contraction):
 *     x = ((u - cx) * z) * invfx;  y = ((v - cy) * z) * invfy;  x3D[r] = ((R[r][0] * x + R[r][1] * y) + R[r][2] * z) + Ow[r]
 *   Eigen leaves the order of the three-term sum to its build: THIS CHOICE DEFINES PARITY.
 * One workgroup per frame: the keys (depth bits << 32 | index; positive floats order as their bit patterns) are compacted into the LDS,
 * sorted there and walked.  One upload, one launch, one download; the results are in host memory when the call returns (stream: NULL =
 * the calling thread's private stream).  Before any device work: TC2LI_ERR_CAPACITY for n > 4096; TC2LI_ERR_INVALID for negative sizes,
 * NULL required arrays, held outside {0, 1, 2}, an unknown mode, max_point < 0.  A refused call writes nothing.  Returns n_frames. */
int tc2li_stereo_points_batch(const tc2li_stereo_points_frame* frames, int n_frames, const float unproject4[4], void* stream);
/* The same contract as plain sequential C++ (the reference's loops with std::sort, one frame per worker thread); needs no device. */
int tc2li_host_stereo_points_batch(const tc2li_stereo_points_frame* frames, int n_frames, const float unproject4[4]);

enum tc2li_new_keyframe_condition {    /* tc2li_keyframe_verdict.conditions */
    TC2LI_NEWKF_C1A = 1, TC2LI_NEWKF_C1B = 2, TC2LI_NEWKF_C1C = 4, TC2LI_NEWKF_C2 = 8, TC2LI_NEWKF_C3 = 16
};
enum tc2li_new_keyframe_exit {         /* tc2li_keyframe_verdict.exit_rule: the rule that answered */
    TC2LI_NEWKF_EXIT_IMU_NOT_INITIALIZED = 1,   /* :2944-2950 */
    TC2LI_NEWKF_EXIT_ONLY_TRACKING = 2,         /* :2952 */
    TC2LI_NEWKF_EXIT_MAPPER_STOPPED = 3,        /* :2956 */
    TC2LI_NEWKF_EXIT_AFTER_RELOC = 4,           /* :2967 */
    TC2LI_NEWKF_EXIT_CONDITIONS = 5,            /* :3049 was false */
    TC2LI_NEWKF_EXIT_MAPPER_ACCEPTS = 6,        /* :3053 */
    TC2LI_NEWKF_EXIT_MAPPER_BUSY = 7            /* :3059-3065: InterruptBA, then the queue length decides */
};
/* What Tracking::NeedNewKeyFrame reads besides the frame (:2942-3076).
 *   inertial mSensor == IMU_STEREO_LIDAR;  imu_initialized GetCurrentMap()->isImuInitialized();  only_tracking mbOnlyTracking;
 *   mapper_stopped isStopped() || stopRequested();  mapper_idle AcceptKeyFrames();  mapper_initializing IsInitializing();
 *   keyframes_in_queue KeyframesInQueue();  has_last_kf mpLastKeyFrame != NULL (0 with inertial && !imu_initialized is refused: the
 *   reference would dereference NULL at :2946);  time_frame / time_last_kf the two mTimeStamp;
 *   create_blocked: the gates of CreateNewKeyFrame (:3080-3084), IsInitializing() && !isImuInitialized() or SetNotStop(true) failing
 *     because local mapping has stopped, AS THEY ARE WHEN THE CALL IS MADE -- the reference evaluates SetNotStop(true) live, after the
 *     decision; this snapshot is a deviation (the caller still makes the SetNotStop calls on its own objects);
 *   frame_id mCurrentFrame.mnId (unsigned long);  last_reloc_frame_id mnLastRelocFrameId, last_keyframe_id mnLastKeyFrameId: unsigned int
 *     in the reference (SF/include/Tracking.h:335-336), so last + max_frames / + min_frames at :2967, :3023, :3025 is an unsigned 32-bit
 *     sum that is then compared with the 64-bit frame_id; the library does the same, and a value above 2^32 - 1 is refused;
 *   max_frames, min_frames mMaxFrames, mMinFrames;  n_kfs KeyFramesInMap();  matches_inliers mnMatchesInliers;
 *   n_ref_matches mpReferenceKF->TrackedMapPoints(n_kfs <= 2 ? 2 : 3) -- or ref_nobs [n_ref] != NULL: Observations() of every non-NULL,
 *     non-bad map point of the reference keyframe and -1 for the other slots, and the library counts the entries >= that minimum itself
 *     (SF/src/KeyFrame.cc:352-377, Tracking.cc:2973-2976; n_ref_matches is then not read). */
typedef struct tc2li_keyframe_decision {
    const int32_t* ref_nobs;
    uint64_t frame_id, last_reloc_frame_id, last_keyframe_id;
    double time_frame, time_last_kf;
    int32_t n_ref, max_frames, min_frames, n_kfs, matches_inliers, n_ref_matches, keyframes_in_queue;
    uint8_t inertial, imu_initialized, only_tracking, mapper_stopped, mapper_idle, mapper_initializing, create_blocked, has_last_kf;
    int32_t pad_;
} tc2li_keyframe_decision;
typedef struct tc2li_keyframe_verdict {
    int32_t need;                      /* NeedNewKeyFrame()'s return value */
    int32_t interrupt_ba;              /* 1: the caller calls mpLocalMapper->InterruptBA() (:3059) */
    int32_t conditions;                /* tc2li_new_keyframe_condition mask; 0 where exit_rule < 5 */
    int32_t exit_rule;                 /* tc2li_new_keyframe_exit */
    int32_t n_tracked_close, n_non_tracked_close;   /* :2982-2998; computed whichever rule answered */
    int32_t n_ref_matches;             /* the value the rules used */
    int32_t pad_;
} tc2li_keyframe_verdict;
/* Tracking::NeedNewKeyFrame for n_frames frames at once and, where it says yes and create_blocked is 0, the CLOSEST creation of
 * tc2li_stereo_points_batch for the new keyframe (frames[f].mode must be TC2LI_STEREO_POINTS_CLOSEST, outlier must not be NULL); elsewhere
 * counts = {0, 0, n_with_depth}.  The rules in the reference's order:
 *   1. inertial && !imu_initialized: need = time_frame - time_last_kf >= 0.25 and nothing else is evaluated (:2944-2950)
 *   2. only_tracking: no (:2952)      3. mapper_stopped: no (:2956)
 *   4. frame_id < last_reloc_frame_id + max_frames && n_kfs > max_frames: no (:2967)
 *   5. over the keypoints with depth > 0 && depth < th_depth (:2990; depth == th_depth is not close here, though the walk above treats it
 *      as close): tracked iff held != 0 && !outlier.  close = nTrackedClose < 100 && nNonTrackedClose > 70;  thRefRatio = n_kfs < 2 ? 0.4f
 *      : 0.75f;  c1a = frame_id >= last_keyframe_id + max_frames;  c1b = frame_id >= last_keyframe_id + min_frames && mapper_idle;
 *      c1c = !inertial && ((double)inliers < (double)ref * 0.25 || close);  c2 = ((float)inliers < (float)ref * thRefRatio || close) &&
 *      inliers > 15 -- the int-by-double and int-by-float products of :3027, :3029 as C++ evaluates them;  c3 = has_last_kf && inertial &&
 *      time_frame - time_last_kf >= 0.5;  c4 is false (:3044)
 *   6. if ((c1a || c1b || c1c) && c2) || c3: yes if mapper_idle || mapper_initializing; otherwise interrupt_ba = 1 and the answer is
 *      keyframes_in_queue < 3.  Else no.
 * The counts, the decision, the sort and the walk of a frame are one workgroup's work in one launch; with the upload, the download and the
 * wait that is the whole step of a batch of sequences.  Refusals as tc2li_stereo_points_batch, and TC2LI_ERR_INVALID for outlier == NULL,
 * a mode other than CLOSEST, n_ref < 0, has_last_kf == 0 with inertial && !imu_initialized, last ids above 2^32 - 1.  A refused call
 * writes nothing.  Returns n_frames. */
int tc2li_new_keyframe_batch(const tc2li_stereo_points_frame* frames, const tc2li_keyframe_decision* decisions, tc2li_keyframe_verdict* verdicts,
                             int n_frames, const float unproject4[4], void* stream);
/* The same contract as plain sequential C++; needs no device. */
int tc2li_host_new_keyframe_batch(const tc2li_stereo_points_frame* frames, const tc2li_keyframe_decision* decisions,
                                  tc2li_keyframe_verdict* verdicts, int n_frames, const float unproject4[4]);

/* ---- image ingest: what a camera image passes before ORBextractor::operator() sees it -------------------------------------------------
 * System::TrackStereoLidar (SF/src/System.cc:240-257): with settings_->needToRectify() cv::remap(im, out, M1, M2, INTER_LINEAR) with the
 * CV_32F maps of SF/src/Settings.cc:523-526 (:241-248), else with needToResize() cv::resize(im, out, newImSize) (:250-252), else a clone
 * (:254-255).  Tracking::GrabImageStereoLidar (SF/src/Tracking.cc:1646-1671): a 3-channel image through cvtColor RGB2GRAY / BGR2GRAY, a
 * 4-channel one through RGBA2GRAY / BGRA2GRAY, chosen by mbRGB.  Both steps in one pass: remap or resize first, on the image as delivered,
 * every channel on its own and rounded to 8 bits; gray is formed from that result (gray first and remap second gives other bytes).
 * Semantics (a recollection of OpenCV 4.2, parity unpinned: SURVEY.md Appendix B; tests/image_prep_ref.py restates them in numpy):
 *   gray     (R * 9798 + G * 19235 + B * 3735 + 16384) >> 15;  rgb != 0: channel 0 is R, else B;  a fourth channel is not read.
 *   remap    INTER_LINEAR, BORDER_CONSTANT 0, maps of the destination's size: sx = cvRound(map_x * 32) (float product, ties to even),
 *            ix = saturate_cast<short>(sx >> 5), fx = sx & 31, the same in y; taps (iy, ix), (iy, ix + 1), (iy + 1, ix), (iy + 1, ix + 1)
 *            with weights (32 - fx)(32 - fy) 32, fx (32 - fy) 32, (32 - fx) fy 32, fx fy 32; a tap outside the source reads 0;
 *            out = (sum + 16384) >> 15.
 *   resize   INTER_LINEAR as the extractor's pyramid (SF/src/ORBextractor.cc:1156): source coordinate (dx + 0.5) * scale - 0.5, floor and
 *            clamp, 11-bit weights, (((b0 * (S0 >> 4)) >> 16) + ((b1 * (S1 >> 4)) >> 16) + 2) >> 2; any source and destination size.
 * Computing the maps (stereoRectify / initUndistortRectifyMap) stays with the caller, and so do 16-bit and float images. */
enum tc2li_image_prep_mode {
    TC2LI_IMAGE_PREP_COPY = 0,      /* System.cc:254-255 */
    TC2LI_IMAGE_PREP_RECTIFY = 1,   /* System.cc:241-248 */
    TC2LI_IMAGE_PREP_RESIZE = 2     /* System.cc:250-252 */
};
typedef struct tc2li_image_prep_params {
    int32_t src_width, src_height;  /* the image as delivered, 1 .. 16384 */
    int32_t channels;               /* 1, 3 or 4 interleaved bytes per pixel (Tracking.cc:1646, :1660) */
    int32_t rgb;                    /* mbRGB (Tracking.cc:1648, :1662) */
    int32_t mode;                   /* tc2li_image_prep_mode */
    int32_t dst_width, dst_height;  /* RECTIFY: the maps' size; RESIZE: newImSize; COPY: the source's size.  1 .. 16384 */
} tc2li_image_prep_params;
typedef struct tc2li_image_prep tc2li_image_prep;
/* A handle for calls of up to max_images (1 .. 65535) images.  TC2LI_ERR_INVALID for a channel count other than 1, 3 or 4, a dimension
 * outside 1 .. 16384, an unknown mode, COPY with a destination size other than the source's; checked before the device is looked for. */
int tc2li_image_prep_create(const tc2li_image_prep_params* params, int max_images, tc2li_image_prep** out);
void tc2li_image_prep_destroy(tc2li_image_prep* prep);
/* The maps of camera 0 (left: M1l, M2l) or 1 (right: M1r, M2r): host memory, dst_height rows of dst_width floats.  They are checked once,
 * here -- a value that is not finite or has |v| >= 2^24 is TC2LI_ERR_INVALID, cvRound is undefined for it -- and converted once, on the
 * device, to the fixed-point form above, which stays with the handle; no call converts them again.  The maps are no longer read when
 * the call returns (stream: NULL = the calling thread's private stream).  The call is ordered behind every tc2li_image_prep_batch queued
 * on the handle before it: kernels in flight read the maps they were queued with.  TC2LI_ERR_INVALID for a handle whose mode is not
 * RECTIFY.  A refused call changes nothing: a camera that had no map still has none, one that had an accepted map keeps it. */
int tc2li_image_prep_set_maps(tc2li_image_prep* prep, int camera, const float* map_x, const float* map_y, void* stream);
/* n_images images in one launch: image i starts at images + i * image_pitch_bytes, its rows are `stride` bytes apart, and it belongs to
 * camera i & 1 (the frame convention of tc2li_stereo_match_batch).  images_on_device == 0: host memory, staged and uploaded inside the
 * call, which then returns when the gray images are complete; != 0: device memory, the call only queues work on `stream` (NULL = the
 * null stream, as for tc2li_orb_extract_batch).
 * dev_gray is CALLER-OWNED device memory in exactly the layout tc2li_orb_extract_batch reads (gray image i at dev_gray + i *
 * gray_pitch_bytes, rows gray_stride bytes apart): pass it on with width = dst_width, height = dst_height, stride = gray_stride,
 * image_pitch_bytes = gray_pitch_bytes on the same stream.  That call reads level 0 in place, so the buffer must outlive the handle's
 * pyramids (the stereo matcher and the tracking searches read them), not only the ingest.
 * TC2LI_ERR_INVALID before any launch for stride < src_width * channels, gray_stride < dst_width, gray images that would overlap, a
 * RECTIFY call before the maps of both cameras are set; TC2LI_ERR_CAPACITY for n_images > max_images.  Returns n_images. */
int tc2li_image_prep_batch(tc2li_image_prep* prep, const uint8_t* images, int images_on_device, int n_images, int stride,
                           size_t image_pitch_bytes, uint8_t* dev_gray, int gray_stride, size_t gray_pitch_bytes, void* stream);
/* The same contract as plain C++ on the worker pool, every pointer host memory; needs no device.  maps = {x left, y left, x right,
 * y right} (NULL, or NULL entries, unless the mode is RECTIFY); they are checked as tc2li_image_prep_set_maps checks them, on every call. */
int tc2li_host_image_prep_batch(const tc2li_image_prep_params* params, const float* const maps[4], const uint8_t* images, int n_images,
                                int stride, size_t image_pitch_bytes, uint8_t* gray, int gray_stride, size_t gray_pitch_bytes);

/* ---- IMU initialisation: the map update (SF/src/Map.cc:256-287 Map::ApplyScaledRotation, called at SF/src/LocalMapping.cc:1299 and :1494;
 * SF/src/LocalMapping.cc:1346-1425, the update of the map after FullInertialBA, which is the reference's update after any global BA) ------
 * The two steps of LocalMapping::InitializeIMU (:1184-1445) and ScaleRefinement (:1447-1512) that rewrite every keyframe and every map
 * point, on a flat copy of the map, one problem per sequence.  The library returns the new poses, velocities, biases and positions; the
 * caller writes them into its objects (INTEGRATION.md "InitializeIMU / ScaleRefinement").  Rig: pinhole stereo, NLeft == -1, no
 * mpCamera2: an observation contributes its left camera centre only.  All pointers are host memory, the arrays are copied by the call,
 * indices are rows of the problem's own tables, outputs must not overlap inputs.  A pose is seven floats, the unit quaternion x, y, z, w
 * and the translation, as Sophus::SE3f holds it.
 * Arithmetic: float, every product and sum rounded (no contraction), the Sophus operations in the order Sophus writes them
 * (csrc/se3f_math.hpp):
 *   unit(q)      len = sqrt(x*x + y*y + z*z + w*w) summed left to right, then four divisions (SO3::normalize)
 *   spin(q, p)   uv = q.vec x p; uv += uv; p + w * uv + q.vec x uv, summed left to right (so3.hpp:358-367)
 *   inverse(T)   q' = unit(conj(q)) -- the conjugate passes the SO3(Quaternion) constructor --, t' = spin(q', t * -1) (se3.hpp:208-211)
 *   compose(A,B) q = unit(a * b) with the product of so3.hpp:325-339, t = t_a + spin(q_a, t_b) (se3.hpp:304-308)
 *   rotation_of  Eigen's toRotationMatrix
 * Where Eigen leaves a summation order to its build, THESE CHOICES DEFINE PARITY: a 3-term row sum is ((a*x + b*y) + c*z), a translation
 * is added after it; a vector norm is sqrtf((x*x + y*y) + z*z), the order of tc2li_map_points_refresh.
 *
 * One call of Map::ApplyScaledRotation(T, s, bScaledVel):
 *   T7 Tyw as the caller's Sophus::SE3f holds it;  s;  scaled_vel bScaledVel;  has_tcb mImuCalib.mbIsSet and tcb3 mImuCalib.mTcb.translation();
 *   keyframes (n_keyframes rows): kf_pose7 mTcw;  kf_vel [n][3] mVw
 *   points (n_points rows): point_pos [n][3];  point_bad isBad();  CSR obs_offsets [n_points + 1];  obs_kf the observing keyframe, IN THE
 *     ITERATION ORDER OF mObservations -- the normal is a float sum in that order --;  point_ref_kf mpRefKF (-1 only where the point is bad
 *     or has no observations);  point_ref_level_scale mvScaleFactors[octave of the reference observation];  last_level_scale
 *     mvScaleFactors[nLevels - 1]
 * Per keyframe (Map.cc:268-277, KeyFrame::SetPose SF/src/KeyFrame.cc:121-134): Twc = inverse(Tcw); Twc.t *= s componentwise; Tyc =
 *   compose(Tyw, Twc); Tcw' = inverse(Tyc); Twc' = inverse(Tcw'); with has_tcb Owb' = rotation_of(Twc'.q) * tcb + Twc'.t; V' = Ryw * V,
 *   then * s with scaled_vel, Ryw = rotation_of(Tyw.q).
 * Per point (Map.cc:283-284): M = s * Ryw with every entry rounded; pos' = ((M[r][0]*x + M[r][1]*y) + M[r][2]*z) + tyw[r] -- a bad point
 *   is moved too, SetWorldPos does not look at the flag --; then MapPoint::UpdateNormalAndDepth (SF/src/MapPoint.cc:444-503) against the
 *   new camera centres Twc'.t, which does nothing for a bad point or one without observations: normal = the sum over the observations, in
 *   order, of (pos' - Ow) / |pos' - Ow|, divided by their number; max_distance = |pos' - Ow_ref| * point_ref_level_scale; min_distance =
 *   max_distance / last_level_scale.  The arithmetic of tc2li_map_points_refresh, without its cap on the observations of a point.
 * Out: kf_pose7_out mTcw;  kf_inv_pose7_out mTwc (its translation is the camera centre);  kf_imu_pos_out [n][3] mOwb (may be NULL;
 * written when has_tcb);  kf_vel_out;  point_pos_out;  point_normal [n][3], point_min_distance, point_max_distance: left untouched where
 * the reference returns early. */
typedef struct tc2li_scaled_rotation_problem {
    const float* kf_pose7;
    const float* kf_vel;
    const float* point_pos;
    const uint8_t* point_bad;
    const int32_t* obs_offsets;
    const int32_t* obs_kf;
    const int32_t* point_ref_kf;
    const float* point_ref_level_scale;
    float* kf_pose7_out;
    float* kf_inv_pose7_out;
    float* kf_imu_pos_out;
    float* kf_vel_out;
    float* point_pos_out;
    float* point_normal;
    float* point_min_distance;
    float* point_max_distance;
    float T7[7];
    float s;
    float tcb3[3];
    float last_level_scale;
    int32_t n_keyframes, n_points;
    uint8_t scaled_vel, has_tcb;
    uint8_t pad_[6];
} tc2li_scaled_rotation_problem;
/* Map::ApplyScaledRotation for n_problems maps at once on the device: one lane per keyframe, then one lane per point with the point's
 * observations walked in order.  One upload, two launches, one download; the results are in host memory when the call returns (stream:
 * NULL = the calling thread's private stream).  Before any device work: TC2LI_ERR_INVALID for negative sizes, NULL required arrays,
 * offsets that do not ascend from 0, obs_kf or point_ref_kf out of range.  A refused call writes nothing.  Returns n_problems. */
int tc2li_apply_scaled_rotation_batch(const tc2li_scaled_rotation_problem* problems, int n_problems, void* stream);
/* The same contract as plain sequential C++ with the same arithmetic (one problem per worker thread); needs no device. */
int tc2li_host_apply_scaled_rotation_batch(const tc2li_scaled_rotation_problem* problems, int n_problems);

/* One map update after a global BA with nLoopId != 0 (LocalMapping.cc:1346-1425), on what Optimizer.cc:734-810 left on the objects.
 *   keyframes (n_keyframes rows, at most 4096): kf_parent mpParent (-1 = none);  kf_origin member of mvpKeyFrameOrigins (an origin has no
 *     parent);  kf_bad isBad();  kf_in_gba mnBAGlobalForKF == GBAid on entry;  kf_imu bImu;  kf_vel_set isVelocitySet();  kf_pose7 mTcw;
 *     kf_gba_pose7 mTcwGBA as stored;  kf_bef_gba_pose7 mTcwBefGBA as stored (read only for keyframes the walk does not reach);  kf_vel /
 *     kf_gba_vel [n][3] mVw / mVwbGBA;  kf_bias / kf_gba_bias [n][6] GetImuBias() / mBiasGBA
 *   points (n_points rows): point_bad;  point_in_gba mnBAGlobalForKF == GBAid;  point_pos;  point_gba_pos mPosGBA;  point_ref_kf (-1 only
 *     where the point is bad or in the GBA)
 * The walk (:1347-1394) starts at the origins and goes down the children.  A bad child is skipped with everything below it; an origin is
 * not asked.  A visited child with !kf_in_gba gets TcwGBA = compose(compose(Tcw_child, Twc_parent), TcwGBA_parent), where Twc_parent is
 * the parent's mTwc when the parent is popped, inverse() of its pose before its own SetPose; VwbGBA = spin(compose_q(inverse_q(TcwGBA.q),
 * Tcw_child.q), V) when kf_vel_set (inverse_q = unit(conj), SO3::inverse), else its stored kf_gba_vel; BiasGBA = its bias; and the flag.
 * Every visited keyframe then gets TcwBefGBA = Tcw, Tcw = TcwGBA and, with kf_imu, V = VwbGBA and bias = BiasGBA.  EVERY KEYFRAME HAS ONE
 * PARENT, SO THE ORDER AMONG SIBLINGS REACHES NO RESULT.
 * Points (:1399-1425): a bad point is untouched; point_in_gba: pos = gba_pos; otherwise, only if the reference keyframe's flag is set
 * after the walk: Xc = spin(TcwBef.q, pos) + TcwBef.t, pos = spin(Twc'.q, Xc) + Twc'.t with Twc' = inverse() of that keyframe's pose
 * after the walk.  UpdateNormalAndDepth is not called here in the reference.
 * Out: kf_visited;  kf_in_gba_out;  kf_pose7_out;  kf_bef_gba_pose7_out;  kf_vel_out;  kf_bias_out (all rows are written: a keyframe the
 * walk did not reach gets its inputs back);  point_pos_out;  point_moved: 0 untouched, 1 took the GBA position, 2 followed its reference
 * keyframe. */
typedef struct tc2li_gba_correction_problem {
    const int32_t* kf_parent;
    const uint8_t* kf_origin;
    const uint8_t* kf_bad;
    const uint8_t* kf_in_gba;
    const uint8_t* kf_imu;
    const uint8_t* kf_vel_set;
    const float* kf_pose7;
    const float* kf_gba_pose7;
    const float* kf_bef_gba_pose7;
    const float* kf_vel;
    const float* kf_gba_vel;
    const float* kf_bias;
    const float* kf_gba_bias;
    const uint8_t* point_bad;
    const uint8_t* point_in_gba;
    const float* point_pos;
    const float* point_gba_pos;
    const int32_t* point_ref_kf;
    uint8_t* kf_visited;
    uint8_t* kf_in_gba_out;
    float* kf_pose7_out;
    float* kf_bef_gba_pose7_out;
    float* kf_vel_out;
    float* kf_bias_out;
    float* point_pos_out;
    uint8_t* point_moved;
    int32_t n_keyframes, n_points;
} tc2li_gba_correction_problem;
/* The map update of n_problems maps at once on the device: one workgroup per problem walks the tree in rounds (a round resolves every
 * keyframe whose parent is resolved; a chain of depth d takes d rounds), then one lane per point.  One upload, two launches, one
 * download; the results are in host memory when the call returns (stream: NULL = the calling thread's private stream).  Before any device
 * work: TC2LI_ERR_INVALID for negative sizes, NULL arrays, kf_parent or point_ref_kf out of range, an origin with a parent, a parent
 * chain that does not end (a cycle); TC2LI_ERR_CAPACITY for more than 4096 keyframes in a problem.  A refused call writes nothing.
 * Returns n_problems. */
int tc2li_gba_map_correction_batch(const tc2li_gba_correction_problem* problems, int n_problems, void* stream);
/* The same contract as plain sequential C++ (the list of :1347 as a queue, one problem per worker thread); needs no device. */
int tc2li_host_gba_map_correction_batch(const tc2li_gba_correction_problem* problems, int n_problems);
/* out[0] = the most keyframes of a tc2li_gba_correction_problem (the walk's state bytes live in LDS), out[1] = threads per problem in the
 * walk, out[2] = keyframes and out[3] = points per workgroup of the per-row kernels.  Returns 4.  Needs no device.  No reference
 * counterpart. */
int tc2li_map_update_limits(int32_t* out, int capacity);

/* ---- IMU initialisation: the inertial optimisation, batched (SF/src/Optimizer.cc:2169-2356 Optimizer::InertialOptimization(pMap, Rwg,
 * scale, bg, ba, bMono, covInertial, bFixedVel, bGauss, priorG, priorA), called at SF/src/LocalMapping.cc:1283; SF/src/Optimizer.cc:2359-2466
 * Optimizer::InertialOptimization(pMap, Rwg, scale), called at SF/src/LocalMapping.cc:1491) --------------------------------------------------
 * tc2li_inertial_optimization and tc2li_inertial_scale_refinement ("IMU initialisation" above) for many maps at once: when many sequences
 * start together they reach the 1 s, 5 s and 15 s initialisations (SF/src/LocalMapping.cc:204-240) and every 10 s scale refinement (:253)
 * in the same step.  One problem per map; it carries exactly the arguments of the two single-problem entries, with their meaning:
 *   n_keyframes;  Rwb9 [n][9], twb3 [n][3] the keyframes in temporal order;  vel3 [n][3] the velocities: in / out in the first form, read
 *   only in the refinement form;  pre [n]: pre[i] = keyframe i's pre-integration from keyframe i - 1, pre[0] is ignored and a NULL entry
 *   is a link that is skipped;  Rwg9 [9], scale: in / out;  bg [3], ba [3]: in / out, first form;  bg3, ba3 [n][3]: the keyframes' fixed
 *   biases, refinement form -- edge i takes keyframe i - 1's;  mono, fixed_vel, prior_g, prior_a: first form;  iterations: 200 / 10 in the
 *   reference;  refine: 0 = the first overload, otherwise the second.
 *   Out: stats (may be NULL): the first form's iterations, trials, chi2 before and after and the last lambda;  chi2 [2] (may be NULL): the
 *   refinement form's activeRobustChi2 before and after;  iterations_run (may be NULL): the iterations either form ran.
 * ONE STRUCT, TWO ENTRIES: tc2li_inertial_optimization_batch takes each problem in the form its `refine` says, so one call serves a step
 * in which some maps initialise and others refine; tc2li_inertial_scale_refinement_batch takes every problem in the refinement form
 * whatever `refine` says -- LocalMapping::ScaleRefinement's call needs no flag.  All pointers are host memory. */
typedef struct tc2li_inertial_init_problem {
    const double* Rwb9;
    const double* twb3;
    double* vel3;
    const tc2li_preintegrated* const* pre;
    double* Rwg9;
    double* scale;
    double* bg;
    double* ba;
    const double* bg3;
    const double* ba3;
    tc2li_inertial_init_stats* stats;
    double* chi2;
    int32_t* iterations_run;
    int32_t n_keyframes, mono, fixed_vel, iterations, refine;
    float prior_g, prior_a;
    int32_t pad_;
} tc2li_inertial_init_problem;
/* On the device, one workgroup per map with the whole optimisation inside the launch: Levenberg-Marquardt with g2o's control, trials,
 * backup and restore and stop rules (first form, SF/src/Optimizer.cc:2169-2356), Gauss-Newton with Huber(1) (refinement form, :2359-2466).
 * The links' informations are prepared on the host as the single-problem entries prepare them; the 15 x 15 covariances are not uploaded.
 * One upload, one launch per form present, one download; the results are in host memory when the call returns (stream: NULL = the
 * calling thread's private stream).  A map's results are the same bits alone, anywhere in any batch, and from call to call.  They differ
 * from the host entries' by rounding: the sums over links are formed in another (fixed) order and the pre-integration at the new bias
 * normalises its rotation as tc2li_pose_inertial_optimization_batch does.  Before any device work: TC2LI_ERR_INVALID, naming the problem,
 * for n_keyframes < 2, NULL required arrays, negative iterations, a link covariance that is not positive definite, sizes or iterations
 * beyond tc2li_inertial_init_limits.  A refused call writes nothing.  Returns n_problems. */
int tc2li_inertial_optimization_batch(const tc2li_inertial_init_problem* problems, int n_problems, void* stream);
int tc2li_inertial_scale_refinement_batch(const tc2li_inertial_init_problem* problems, int n_problems, void* stream);
/* The same contract through tc2li_inertial_optimization / tc2li_inertial_scale_refinement, one problem per worker thread under the host
 * thread budget: their results, bit for bit; no limits on sizes or iterations; needs no device. */
int tc2li_host_inertial_optimization_batch(const tc2li_inertial_init_problem* problems, int n_problems);
int tc2li_host_inertial_scale_refinement_batch(const tc2li_inertial_init_problem* problems, int n_problems);
/* out[0] = the most keyframes of a first-form problem in a device call (its solver state is per keyframe), out[1] = of a refinement-form
 * problem, out[2] = the most iterations of either (so that no launch is unbounded).  Returns 3.  Needs no device.  No reference
 * counterpart. */
int tc2li_inertial_init_limits(int32_t* out, int capacity);
/* One step of the block factorisation of the first form's velocity part, the function the kernel's chain runs (csrc/imu_init_device.hpp):
 * S = D + lambda I - L Sinv_prev L' (Sinv_prev NULL: the first block, L is not read), Sinv = S^-1.  Returns 1, or 0 when S is singular or
 * not finite -- the trial then fails and Sinv is not written.  Needs no device.  No reference counterpart (g2o hands the system to a sparse
 * Cholesky). */
int tc2li_inertial_init_arrow_pivot(const double D[9], const double L[9], const double Sinv_prev[9], double lambda, double Sinv[9]);

#ifdef __cplusplus
}
#endif
#endif /* TC2LI_HIP_H */
