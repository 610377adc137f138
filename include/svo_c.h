/*
 * svo_c.h — C ABI of the MI355X-native direct-alignment hot path (libsvo_hip.so).
 *
 * This is the drop-in boundary for amin-abouee/semi-direct-visual-odometry's sparse image alignment,
 * feature alignment and image pyramid.  The reference has no plugin registry or FFI: its boundary is
 * the C++ class surface.  Each entry point below names the reference interface it
 * replaces (paths relative to the reference root).  The C++ host mirror of that class surface
 * (semi-direct-visual-odometry_amd/host/svo.hpp) and the Python mirror (svo_amd) sit on top of it.
 *
 * Conventions
 *   - every function returns int: 0 = SVO_OK, < 0 = error (svo_last_error() has the message);
 *     no C++ exception crosses the ABI;
 *   - host buffers are caller-owned and only read/written during the call (or until the documented
 *     synchronisation point for *_run);
 *   - device memory is owned by the context; one context per (host thread, GPU); not reentrant;
 *   - poses are world->camera SE(3) in Sophus params() order: qx, qy, qz, qw, tx, ty, tz
 *     (Frame::m_absPose, include/frame.hpp:198);
 *   - images are 8-bit grey, row-major, tightly packed (cv::Mat CV_8UC1, continuous).
 */
#ifndef SVO_C_H
#define SVO_C_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVO_ABI_VERSION 2

enum {
    SVO_OK = 0,
    SVO_ERR_ARG = -1,    /* bad argument (null pointer, size out of range, bad index) */
    SVO_ERR_HIP = -2,    /* HIP runtime error */
    SVO_ERR_NODEV = -3,  /* no usable gfx950 device */
    SVO_ERR_STATE = -4   /* object used in the wrong state (e.g. results before run) */
};

/* Optimizer::Status values (include/optimizer.hpp:21-33) reported per alignment. */
enum {
    SVO_STATUS_SUCCESS = 0,
    SVO_STATUS_MAX_COFF_DX = 1,
    SVO_STATUS_NON_IN_DX = 2,
    SVO_STATUS_SMALL_STEP_SIZE = 3,
    SVO_STATUS_LAMBDA_VALUE = 4,
    SVO_STATUS_NORM_INF_DIFF = 5,
    SVO_STATUS_NON_SUFF_POINTS = 6,
    SVO_STATUS_INCREASE_CHI_SQUARED_ERROR = 7,
    SVO_STATUS_SMALL_CHI_SQUARED_ERROR = 8,
    SVO_STATUS_FAILED = 9
};

typedef struct svo_ctx svo_ctx;
typedef struct svo_pyramid_set svo_pyramid_set;
typedef struct svo_align_batch svo_align_batch;

/* PinholeCamera's ideal pinhole model (src/pinhole_camera.cpp:50-101; KITTI d = 0, resource/kitti.yaml).  Every entry
 * point that takes a camera works on UNDISTORTED pixels: a lens with distortion is handled once per frame, ahead of the
 * pyramid (svo_undistort_*, svo_pyramid_set_upload_undistort below), after which the image is this camera's. */
typedef struct {
    double fx, fy, cx, cy;
    int32_t width, height;
} svo_camera;

/* Robust-scale semantics of the Tukey weights (Optimizer::tukeyWeighting, src/optimizer.cpp:485-514, with
 * algorithm::computeMedian / computeMAD, src/algorithm.cpp:834-865).
 *   SVO_MEDIAN_REFERENCE: the reference's own values: std::nth_element on the full residual vector and,
 *     for an even length, vec[n/2 - 1] as libstdc++'s introselect leaves it (not always the (n/2 - 1)-th
 *     order statistic): the device re-runs the introselect -- K2V (csrc/align_refv.hip, the vector in one
 *     CU's registers) whenever every pair of a launch holds at most svo_robust_scale_capacity(SVO_SCALE_K2V)
 *     slots, K2R (csrc/align_ref.hip, segments in LDS / global scratch) otherwise; the same bits either way;
 *   SVO_MEDIAN_EXACT: true order statistics ((n/2 - 1)-th and n/2-th), the robust statistic the
 *     reference means; faster (K2). */
enum { SVO_MEDIAN_EXACT = 0, SVO_MEDIAN_REFERENCE = 1 };
/* SVO_MEDIAN_REFERENCE: largest residual vector per pair (max_features * patch_size^2) */
#define SVO_REF_MAX_SLOTS 524288

/* ImageAlignment(patchSize, minLevel, maxLevel, numParameters=6) (include/image_alignment.hpp:18).
 * median_mode: SVO_MEDIAN_EXACT or SVO_MEDIAN_REFERENCE (above). */
typedef struct {
    int32_t patch_size;
    int32_t min_level;
    int32_t max_level;
    int32_t median_mode;
} svo_align_params;

/* Per pair, per pyramid level record of the single LM step (mirrors Optimizer state after
 * optimizeLM, src/optimizer.cpp:162-370).  H is the damped 6x6 (row-major), g the gradient. */
typedef struct {
    int32_t level, n_ref_vis, n_vis, status;
    double median, mad, sigma, chi2, lambda, err;
    double H[36], g[6], dx[6];
    int32_t scale_kernel; /* the device kernel that computed median / MAD at this level: SVO_SCALE_K2R,
                             SVO_SCALE_K2V or SVO_SCALE_K2 (exact mode); 0 if the level did not run */
    int32_t reserved;
} svo_level_trace;

/* ---------------------------------------------------------------- context */
int svo_device_count(int32_t* count);
int svo_ctx_create(int32_t device, svo_ctx** out);
int svo_ctx_destroy(svo_ctx* ctx);
int svo_ctx_synchronize(svo_ctx* ctx);
/* hipStream_t of the context, for event timing.  The handle is joined with the side chains a batch run may have left
 * pending only at the moment of this call: work the caller queues on a handle it kept across a later
 * svo_align_batch_run does not wait for that run's chains.  Call svo_ctx_stream() (or svo_ctx_event_record) again
 * after each run, or set SVO_DEFER_JOIN=0 when the stream has been handed out. */
void* svo_ctx_stream(svo_ctx* ctx);
const char* svo_last_error(void);
int svo_abi_version(void);
/* hipEvent timing on the context stream: record event `slot` (0..15) now; elapsed ms between two
 * recorded slots (waits for the later one). */
int svo_ctx_event_record(svo_ctx* ctx, int32_t slot);
int svo_ctx_event_elapsed(svo_ctx* ctx, int32_t slot_begin, int32_t slot_end, float* ms);

/* ---------------------------------------------------------------- ImagePyramid
 * Replaces ImagePyramid::createImagePyramid (src/image_pyramid.cpp:36-52), called from the Frame
 * constructor (src/frame.cpp:26): per frame an intensity stack (level 0 = input, level l = pyrDown
 * of level l-1) and a gradient stack (level 0 = Simd::AbsGradientSaturatedSum, level l = pyrDown of
 * gradient l-1).  A set holds n_frames device-resident stacks of equal geometry, packed level after
 * level; level sizes are ((w+1)/2, (h+1)/2) per step (cv::pyrDown default). */
int svo_pyramid_set_create(svo_ctx* ctx, int32_t n_frames, int32_t width, int32_t height, int32_t levels,
                           svo_pyramid_set** out);
int svo_pyramid_set_destroy(svo_pyramid_set* set);
/* Copy `count` base images (count*width*height bytes) into frames [first, first+count). Async. */
int svo_pyramid_set_upload(svo_pyramid_set* set, int32_t first, int32_t count, const uint8_t* host_images);
/* Same, from device memory (e.g. a decoder's output), stream-ordered. */
int svo_pyramid_set_upload_device(svo_pyramid_set* set, int32_t first, int32_t count, const uint8_t* dev_images);
/* Build both stacks for frames [first, first+count) on the device.  Async (context stream). */
int svo_pyramid_set_build(svo_pyramid_set* set, int32_t first, int32_t count);
/* The same build on the context's prep stream, after everything queued on the context stream so far, so that it
 * overlaps work queued later (the next batch's pyramids building while the current batch aligns:
 * src/frame.cpp:26 -> src/image_pyramid.cpp:36-52 for the frames of the next call).  Every later use of the set's
 * planes through this ABI (upload, build, download, svo_align_batch_set_pair / set_pairs) waits for it. */
int svo_pyramid_set_build_async(svo_pyramid_set* set, int32_t first, int32_t count);
/* ImagePyramid::getImageAtLevel / getGradientAtLevel (src/image_pyramid.cpp:54-124): copy one level
 * to the host (synchronous).  gradient = 0 for the intensity stack, 1 for the gradient stack. */
int svo_pyramid_set_download(const svo_pyramid_set* set, int32_t frame, int32_t level, int32_t gradient, uint8_t* out);
/* ImagePyramid::getImageSizeAtLevel (src/image_pyramid.cpp:110-116). */
int svo_pyramid_level_size(const svo_pyramid_set* set, int32_t level, int32_t* width, int32_t* height);

/* ---------------------------------------------------------------- ImageAlignment
 * Replaces ImageAlignment::align(refFrame, curFrame) (src/image_alignment.cpp:25-67, declared
 * include/image_alignment.hpp:25; called src/system.cpp:313).  A batch holds n_pairs independent
 * (ref, ref->lastKeyframe, cur) problems; each is the reference's whole coarse-to-fine call:
 * for level = max..min: Jacobian of the ref patches, one Tukey-weighted Nielsen-damped LM step,
 * pose <- pose * exp(-dx).  Features are the ref frame's, then the last keyframe's, in vector order
 * (slots exist for features without a point, src/image_alignment.cpp:81-121). */
int svo_align_batch_create(svo_ctx* ctx, const svo_camera* cam, const svo_align_params* params, int32_t n_pairs,
                           int32_t max_features, svo_align_batch** out);
int svo_align_batch_destroy(svo_align_batch* batch);
/* Describe pair `pair`: each frame is (pyramid set, frame index); the sets must outlive the batch's runs.
 *   px       (n_ref+n_kf) x 2   Feature::m_pixelPosition at level 0 (include/feature.hpp:31)
 *   bearing  (n_ref+n_kf) x 3   Feature::m_bearingVec (include/feature.hpp:33-34)
 *   point    (n_ref+n_kf) x 3   Point::m_position in world coordinates (include/point.hpp:28)
 *   has_point(n_ref+n_kf)       Feature::m_point != nullptr
 * The host arrays are consumed on return (copied into the context's pinned staging ring, or read
 * directly for pairs too large for it); the device copies are stream-ordered before any later work on
 * the context stream and are not waited for.  A copy that fails after this call returned is reported
 * by a later call on the context (the next run, results or pinned-memory user). */
int svo_align_batch_set_pair(svo_align_batch* batch, int32_t pair, const svo_pyramid_set* ref_set, int32_t ref_frame,
                             const svo_pyramid_set* kf_set, int32_t kf_frame, const svo_pyramid_set* cur_set,
                             int32_t cur_frame, const double* ref_pose, const double* kf_pose,
                             const double* cur_pose, int32_t n_ref, int32_t n_kf, const double* px,
                             const double* bearing, const double* point, const uint8_t* has_point);
/* Describe pairs [first, first + count) in one call (the bulk form of svo_align_batch_set_pair): one copy
 * per array for all of them, then a device scatter into the pairs' feature slots.
 *   frames   count x 3   frame indices (ref, kf, cur) in ref_set / kf_set / cur_set
 *   poses    count x 21  ref, kf, cur poses (7 each, as set_pair)
 *   n_feat   count x 2   n_ref, n_kf
 *   px, bearing, point, has_point: the pairs' feature rows packed pair after pair (pair i's rows start at
 *   the sum of the earlier pairs' n_ref + n_kf), layouts as set_pair.  With features_on_device != 0 they
 *   are device pointers on the context's device (e.g. FeatureSelection output), else host memory.
 * Every host array is consumed on return; the upload runs on a copy stream of the context (overlapping
 * earlier work queued there, e.g. a pyramid build) and the scatter is queued on the context stream,
 * ordered before any later work on it.  With features_on_device the call also waits for the scatter, so
 * the device arrays may be reused on return. */
int svo_align_batch_set_pairs(svo_align_batch* batch, int32_t first, int32_t count, const svo_pyramid_set* ref_set,
                              const svo_pyramid_set* kf_set, const svo_pyramid_set* cur_set, const int32_t* frames,
                              const double* poses, const int32_t* n_feat, const double* px, const double* bearing,
                              const double* point, const uint8_t* has_point, int32_t features_on_device);
/* Replace the initial cur poses of all pairs (n_pairs x 7).  Synchronous H2D. */
int svo_align_batch_set_initial_poses(svo_align_batch* batch, const double* poses);
/* Run every pair.  Asynchronous on the context stream; inputs stay untouched, so repeated runs are
 * identical (the result pose is written to a separate device buffer).  A large reference-mode batch runs as
 * sub-batch chains on the context's side streams; back-to-back runs of the same batch are ordered per chain (each
 * chain touches only its own pairs), and every other call that uses the context (results, traces, set_pair(s),
 * pyramid uploads / builds, FeatureAlignment, events, synchronize, destroy) first waits for all of them. */
int svo_align_batch_run(svo_align_batch* batch);
/* One run with a hipEvent between consecutive kernel launches (diagnostics; synchronous).  stage_ms[5]
 * receives the device time per stage summed over the levels: [0] world points + state, [1] residuals,
 * [2] robust scale, [3] weights + normal equations, [4] LM step.  No reference counterpart. */
int svo_align_batch_profile(svo_align_batch* batch, float* stage_ms);
/* Wait for the last run and copy results: poses n_pairs x 7 (the aligned cur->m_absPose), err
 * n_pairs (the RMSE of the finest level, as align() returns), status n_pairs (Optimizer::Status of
 * the finest level).  Any pointer may be NULL. */
int svo_align_batch_results(svo_align_batch* batch, double* poses, double* err, int32_t* status);
/* Per-level records of one pair (max_level+1 entries, indexed by level). */
int svo_align_batch_traces(svo_align_batch* batch, int32_t pair, svo_level_trace* out);

/* Device forms of the reference robust scale (SVO_MEDIAN_REFERENCE): K2V keeps the residual vector in
 * registers (vectors of <= 60 416 slots, 2416 features at patch 5; the faster of its two register layouts up
 * to 50 176 slots, config 2's 2000 features x 25), K2R runs its large rounds through global scratch (any size).
 * Both give the same bits. */
enum { SVO_SCALE_AUTO = 0, SVO_SCALE_K2R = 1, SVO_SCALE_K2V = 2, SVO_SCALE_K2 = 3 /* exact mode (trace only) */ };

/* Diagnostics (no reference counterpart): the SVO_MEDIAN_REFERENCE robust scale of an arbitrary residual
 * vector, i.e. algorithm::computeMAD(values, n_valid) (src/algorithm.cpp:855-865) and the median it uses, on
 * the device, with the kernel `impl` (SVO_SCALE_*; AUTO picks K2V where the vector fits).  values: n_slots
 * doubles, none NaN (an invisible slot is DBL_MAX).  out[0] = median, out[1] = MAD, then as many diagnostics
 * as out_len allows (out_len >= 2):
 *   K2V: [2 + 5p ..] per pass p: cycles, block rounds, one-wave rounds, heap select, chunked exchanges;
 *   K2R: with the environment variable SVO_DEBUG_STAMPS set, [2..9] cycles / block rounds / one-wave rounds
 *        / heap select per pass, [10..189] the block rounds, [190..205] cycles per round phase
 *        (tools/k2r_probe.py).
 * K2V with out_len > 206: out[206..] receives a round trace (development): per round 8 header doubles (pass + 10
 * kind, f, l, pivot, Ks, #GE, #LE, cut) and the vector's n_slots values after the round.
 * K2V with out_len == 2: no diagnostics; the vector runs through the product kernel's own code path (its layouts
 * and one-wave size), whereas the diagnostics kernel hands segments of <= 1024 positions to wave 0.
 * Synchronous.  SVO_ERR_ARG if impl is K2V and the vector does not fit it. */
int svo_debug_robust_scale(svo_ctx* ctx, const double* values, int64_t n_slots, int64_t n_valid, int32_t impl,
                           double* out, int64_t out_len);
/* The largest residual vector (slots = features x patch^2) the robust-scale kernel `impl` (SVO_SCALE_K2V or
 * SVO_SCALE_K2R) takes.  A reference-mode launch runs K2V when every pair's vector fits it, K2R otherwise. */
int svo_robust_scale_capacity(int32_t impl, int64_t* slots);

/* ---------------------------------------------------------------- FeatureAlignment
 * Replaces FeatureAlignment::align(refFeature, curFrame, pixelPos) (src/feature_alignment.cpp:25-62,
 * declared include/feature_alignment.hpp:25; called src/map.cpp:538,608) for n candidates at once:
 * 2-D translation + intensity bias on the level-0 GRADIENT images of the ref and cur frames, one
 * LM step, pixelPos <- flow.xy.  Candidate i's reference feature lives in frame ref_frames[i]
 * (refFeature->m_frame; NULL = every candidate in ref_frame) at ref_px[i] (its m_pixelPosition).
 * px_inout: n x 2 (initial pixel positions in, aligned out); err: the returned RMSE (NaN when the
 * patch left the frame); status: Optimizer::Status.  patch_size: footprint (2 (patch_size / 2) + 1)^2 <= 128 px
 * (patch_size <= 11); with patch_size 1 (one observation, three unknowns) nothing moves: status Non_Suff_Points,
 * err -1 (src/optimizer.cpp:53-54).  Synchronous. */
int svo_feature_align(svo_ctx* ctx, const svo_camera* cam, int32_t patch_size, const svo_pyramid_set* ref_set,
                      const int32_t* ref_frames, int32_t ref_frame, const svo_pyramid_set* cur_set, int32_t cur_frame,
                      int32_t n, const double* ref_px, double* px_inout, double* err, int32_t* status);

/* As svo_feature_align, with each candidate's reference frame in a pyramid set of its own:
 * candidate i reads ref_sets[i] frame ref_frames[i] (the batched call Map::reprojectCell and
 * Map::addCandidateToFrame make: their candidates come from different keyframes). */
int svo_feature_align_multi(svo_ctx* ctx, const svo_camera* cam, int32_t patch_size, const svo_pyramid_set* const* ref_sets,
                            const int32_t* ref_frames, const svo_pyramid_set* cur_set, int32_t cur_frame, int32_t n,
                            const double* ref_px, double* px_inout, double* err, int32_t* status);

/* ---------------------------------------------------------------- map reprojection (host side)
 * Frame::world2image (src/frame.cpp:83-92): px[i] = project2d(pose * points[i]) for n points (n x 3). */
int svo_world2image(const svo_camera* cam, const double* pose, int32_t n, const double* points, double* px);

/* The decisions of Map::reprojectMap (src/map.cpp:260-267, 436-478) with reprojectPoint (:481-492) and
 * reprojectCell (:495-570), before any FeatureAlignment: the reference accepts the aligned position of
 * the first non-deleted candidate of a cell whatever its error, so which candidates are aligned is fixed
 * by the geometry alone and the alignments can run as one batch (svo_feature_align_multi).
 * Grid: cell_size-pixel cells, n_cells = ceil(W / c) * ceil(H / c), visited in cell_order (the
 * reference shuffles it with an unseeded std::random_device; callers pass a seeded permutation).
 * Keyframes k < n_kf (ref frame, then its last keyframe) own features kf_feat_off[k] .. kf_feat_off[k+1]-1;
 * feat_point[f] is the feature's point (-1: none).  Points: position (n_points x 3), type
 * (Point::PointType: 0 GOOD, 1 DELETED, 2 CANDIDATE, 3 UNKNOWN), point_last = m_lastProjectedKFId
 * (updated: set to cur_id for every point projected).  Out: overlap[k] points of keyframe k in the
 * frame; the selected candidates in acceptance order (sel_feat, sel_cell, sel_px = the initial
 * pixel for the alignment; capacity n_cells); matches (m_matches) and trials (m_trials).  The caller
 * applies the per-candidate effects (:558-569): succeededProjection += 1, UNKNOWN -> GOOD past 10, a new
 * feature at the aligned pixel, and marks sel_cell visited. */
int svo_map_reproject_plan(const svo_camera* cam, int32_t cell_size, int32_t n_cells, const int32_t* cell_order,
                           const double* cur_pose, uint64_t cur_id, int32_t n_kf, const int32_t* kf_feat_off,
                           const int32_t* feat_point, int32_t n_points, const double* point_pos,
                           const uint32_t* point_type, uint64_t* point_last, int32_t* overlap, int32_t* n_sel,
                           int32_t* sel_feat, int32_t* sel_cell, double* sel_px, int32_t* matches, int32_t* trials);

/* ---------------------------------------------------------------- depth filter
 * One depth-filter seed: MixedGaussianFilter (include/mixed_gaussian_filter.hpp:28-38) and the feature
 * it refines (m_feature: pixel position and bearing in its keyframe). */
typedef struct {
    double a, b, mu, sigma, var, max_depth; /* Beta(a, b) inlier ratio; inverse-depth N(mu, var); 1 / depthMin */
    double px[2];                           /* m_feature->m_pixelPosition (keyframe, level 0) */
    double bearing[3];                      /* m_feature->m_bearingVec */
    int32_t kf;                             /* keyframe of m_feature->m_frame: index into the call's keyframe table */
    int32_t valid;                          /* m_validity */
} svo_depth_seed;

/* Outcome of one seed in svo_depth_update (no reference counterpart; the reference only logs it). */
enum {
    SVO_DEPTH_REJECTED = 0,  /* point behind / outside the current image: seed invalid (src/depth_estimator.cpp:229-237) */
    SVO_DEPTH_NO_MATCH = 1,  /* epipolar search failed: b += 1 (:252-258) */
    SVO_DEPTH_UPDATED = 2,   /* Gaussian x Beta update (:261-266) */
    SVO_DEPTH_CONVERGED = 3, /* sqrt(var) * 10 < max_depth: candidate point emitted, seed invalid (:281-291) */
    SVO_DEPTH_NAN = 4        /* inverse depth NaN: seed invalid (:292-297) */
};

/* MixedGaussianFilter(feature, depthMean, depthMin) (src/mixed_gaussian_filter.cpp:7-24): initial state
 * of a seed (px, bearing, kf are the caller's; valid = 1).  Host only. */
int svo_depth_seed_init(double depth_mean, double depth_min, svo_depth_seed* seed);

/* Replaces DepthEstimator::updateFilters(frame) (src/depth_estimator.cpp:192-309, with
 * algorithm::matchEpipolarConstraint src/algorithm.cpp:412-551, computeTau :342-357, updateFilter
 * :311-340): every seed against the current frame, then the reference's stable remove_if of invalid
 * seeds.  Keyframe k of the table is frame kf_frames[k] of kf_sets[k] (its level-0 intensity image) with
 * pose kf_poses[7k..7k+6]; the current frame is cur_frame of cur_set with pose cur_pose (Sophus params).
 *   seeds_inout   n_seeds in; the n_seeds_out survivors out (order kept)
 *   outcome       n_seeds (per input seed, SVO_DEPTH_*), may be NULL
 *   cand_points   n_seeds x 3 capacity: world points of the converged seeds (m_map->addNewCandidate),
 *   cand_seed     n_seeds capacity: their input seed index; both in the reference's loop order
 *                 (seeds visited from the last to the first); *n_cand entries.
 * Synchronous. */
int svo_depth_update(svo_ctx* ctx, const svo_camera* cam, int32_t n_kf, const svo_pyramid_set* const* kf_sets,
                     const int32_t* kf_frames, const double* kf_poses, const svo_pyramid_set* cur_set,
                     int32_t cur_frame, const double* cur_pose, int32_t n_seeds, svo_depth_seed* seeds_inout,
                     int32_t* n_seeds_out, int32_t* outcome, double* cand_points, int32_t* cand_seed,
                     int32_t* n_cand);

/* ---------------------------------------------------------------- FeatureSelection
 * Replaces FeatureSelection (src/feature_selection.cpp:19-287; constructed src/system.cpp:28 with the
 * image size and cell_pixel_size, called :81, :252-254, :428-430).  Its bool occupancy grid of
 * (height / cell_size + 1) rows x (width / cell_size + 1) columns (:19-25) is caller-owned bytes here
 * (`occupancy`, row-major, 1 = occupied): setExistingFeatures / setCellInGridOccupancy (:268-282) mark
 * it, the bucketing branches clear it on return (resetGridOccupancy, :75, :141).  The gradient magnitude
 * is the frame's level-0 gradient plane (computeImageGradient :250-266 is the same
 * Simd::AbsGradientSaturatedSum as the pyramid's); the orientation is 0 everywhere (:261).  Output
 * features are in Frame::addFeature order: pixel (x, y) and response = gradient magnitude. */
int svo_feature_grid_size(int32_t width, int32_t height, int32_t cell_size, int32_t* rows, int32_t* cols);
/* Device step of gradientMagnitudeWithSSC (:38-50): the level-0 gradient pixels of `frame` above
 * `threshold` in row-major order, as keys (response << 24 | y * width + x; width * height <= 2^24).
 * keys: capacity entries.  Synchronous. */
int svo_feature_detect(svo_ctx* ctx, const svo_pyramid_set* set, int32_t frame, int32_t threshold, int32_t capacity,
                       uint32_t* keys, int32_t* n_keys);
/* gradientMagnitudeWithSSC(frame, detectionThreshold, numberCandidate, useBucketing) (:27-89): device
 * detection, then std::sort by response (reference comparator) and SSC (:166-248, tolerance 0.1) on the
 * host.  n_keypoints (may be NULL): keypoints above the threshold.  Synchronous. */
int svo_feature_select_ssc(svo_ctx* ctx, const svo_pyramid_set* set, int32_t frame, int32_t threshold,
                           int32_t number_candidate, int32_t use_bucketing, int32_t cell_size, uint8_t* occupancy,
                           int32_t capacity, double* px_out, double* response_out, int32_t* n_out, int32_t* n_keypoints);
/* gradientMagnitudeByValue(frame, detectionThreshold, useBucketing = true) (:91-143): per free cell the
 * first maximum in row-major order, kept if above the threshold; cells in row-major order.  The
 * reference's useBucketing = false branch reads the 8-bit magnitude as float (:150) and is rejected.
 * Synchronous. */
int svo_feature_select_by_value(svo_ctx* ctx, const svo_pyramid_set* set, int32_t frame, int32_t threshold,
                                int32_t cell_size, uint8_t* occupancy, int32_t capacity, double* px_out,
                                double* response_out, int32_t* n_out);

/* ---------------------------------------------------------------- trajectory output (host only)
 * System::writeInFile (src/system.cpp:635-640, called per image from src/main.cpp:114-121): the ref
 * frame's camera->world pose m_absPose.inverse().matrix3x4() (Sophus) as one KITTI trajectory line.
 * out12: that 3x4 matrix, row-major. */
int svo_pose_matrix3x4_inverse(const double* pose, double* out12);
/* The same line as text: the 12 numbers row-major, single spaces, each as an std::ostream with
 * precision 6 prints a double ("%.6g"; Eigen IOFormat utils::eigenFormatIO, src/utils.cpp:10-13), NUL
 * terminated, no newline.  cap: bytes of buf (>= 12 * 14 is always enough). */
int svo_format_kitti_pose(const double* pose, char* buf, int32_t cap);

/* ---------------------------------------------------------------- pose-only bundle adjustment
 * Replaces BundleAdjustment::optimizePose(frame) (src/bundle_adjustment.cpp:35-69; BundleAdjustment(camera,
 * 0, 6) constructed src/system.cpp:31, the call itself is commented out at :388) for n_frames independent
 * frames: one LM step of Optimizer::optimizeLM<SE3d> on |bearing - normalise(T * P)| (three rows per
 * feature, only the third visible), pose <- exp(dx) * pose.  Frame f owns features feat_off[f] ..
 * feat_off[f+1]-1: bearing (x3), point (x3, the feature's m_point->m_position), has_point (m_point != null).
 * vis_inout is m_refVisibility of the BundleAdjustment object that optimises the frame, resized to the
 * frame's feature count (new entries 0): the residual step reads the flags the PREVIOUS call left (the
 * reference calls the residual functor before the Jacobian functor, src/optimizer.cpp:199 vs :242), so a
 * fresh object returns NaN and leaves the pose as exp(0) * pose; on return the flags are has_point.
 * poses_inout n_frames x 7; err: the returned RMSE (0 when the frame has no features, -1 on
 * Non_Suff_Points); status: Optimizer::Status, -1 when nothing ran (no features).  A stale flag on a
 * feature without a point (the reference dereferences null) is SVO_ERR_ARG.  Synchronous. */
int svo_pose_optimize(svo_ctx* ctx, int32_t n_frames, const int32_t* feat_off, const double* bearing,
                      const double* point, const uint8_t* has_point, uint8_t* vis_inout, double* poses_inout,
                      double* err, int32_t* status);

/* ---------------------------------------------------------------- two-view map initialisation
 * Replaces algorithm::triangulate3DWorldPoints(refFrame, curFrame, pointsWorld) (src/algorithm.cpp:553-566 with
 * triangulatePointDLT :655-680) for n_pairs independent frame pairs: pair p owns matches feat_off[p] ..
 * feat_off[p+1]-1 (feat_off[0] = 0, ascending); match k is ref_px[2k..] in the frame posed ref_poses[7p..] and
 * cur_px[2k..] in the frame posed cur_poses[7p..].  Per match the 4x3 system of both projection matrices
 * K * pose.matrix3x4(), its normal equations and Eigen's LDLT on the 3x3.  points_world: n x 3.  Synchronous. */
int svo_triangulate_dlt(svo_ctx* ctx, const svo_camera* cam, int32_t n_pairs, const int32_t* feat_off,
                        const double* ref_poses, const double* cur_poses, const double* ref_px, const double* cur_px,
                        double* points_world);

/* Replaces the map initialisation of System::processSecondFrame from the essential matrix on
 * (src/system.cpp:144-223) for n_pairs independent frame pairs, matches laid out as for svo_triangulate_dlt:
 * F = invK^T E invK (:144), algorithm::sampsonCorrection (src/algorithm.cpp:173-237), recoverPose with
 * decomposeEssentialMatrix (:241-333), the triangulation against the recovered pose, computeMedian (:813-832) of
 * the current-camera norms, the rescaling to map_scale (m_initMapScaleFactor, :179-190) and the validity test with
 * halfPatchSize = ceil(cell_size / 2) (:196-202).  It ends where twoViewBA would be called (:229).
 *   E            n_pairs x 9, row-major (the caller's findEssentialMat result)
 *   ref_poses    n_pairs x 7
 *   ref_px, cur_px  in: the matched pixels; out: Sampson-corrected (also for a pair that fails afterwards)
 *   F            n_pairs x 9, row-major
 *   counts       n_pairs x 4: matches with z > 0 in both cameras under (R1,t) (R1,-t) (R2,t) (R2,-t), each
 *                hypothesis posed as poses[i] * ref_pose (:297).  Which of the two rotations an SVD calls R1 and
 *                which sign it gives t is a convention of the SVD; the set of four is not.
 *   winner       n_pairs: the first hypothesis with the strictly largest count (:318); -1 when every count is 0:
 *                recoverPose fails, the rest of that pair's outputs are median_depth NaN, n_valid 0, valid 0,
 *                survivor -1, points and depths 0, and its cur_poses row is left as the caller had it
 *   cur_poses    n_pairs x 7: poses[winner] alone, without the reference frame's pose (:329), its translation
 *                rewritten as -R_cur (C_ref + s (C_cur - C_ref)) with s = map_scale / median_depth (:184-186)
 *   median_depth n_pairs: the median before scaling; for an even count (vec[mid-1] + vec[mid]) / 2 with vec[mid-1]
 *                as libstdc++'s std::nth_element leaves it
 *   n_valid      n_pairs: matches with isInFrame(ref px, h) && isInFrame(cur px, h) && z_cur > 0
 *   points_world n x 3: the rescaled points (of every match, valid or not)
 *   valid        n: that test per match
 *   survivor     n: per pair, at feat_off[p], the indices within the pair of its valid matches in match order
 *                (the features remove_if keeps, :217-223), then -1
 *   depth        n, may be NULL: the current-camera norms median_depth was taken from
 * Synchronous. */
int svo_two_view_init(svo_ctx* ctx, const svo_camera* cam, int32_t n_pairs, const int32_t* feat_off, const double* E,
                      const double* ref_poses, double map_scale, int32_t cell_size, double* ref_px, double* cur_px,
                      double* F, int32_t* counts, int32_t* winner, double* cur_poses, double* median_depth,
                      int32_t* n_valid, double* points_world, uint8_t* valid, int32_t* survivor, double* depth);

/* ---------------------------------------------------------------- windowed bundle adjustment
 * Replaces the optimisation inside BundleAdjustment::twoViewBA and ::localBA (src/bundle_adjustment.cpp:397-478,
 * :480-625) for n_problems independent problems.  The reference hands these to g2o, which is not part of its tree;
 * the cost and the schedule below are THIS PROJECT'S CONTRACT, modelled on g2o's OptimizationAlgorithmLevenberg
 * with EdgeProjectXYZ2UV edges, and NOT pinned to g2o's bits.
 *   problem    p owns frames frame_off[p] .. frame_off[p+1]-1 (each free or fixed; at most SVO_BA_MAX_FRAMES free
 *              ones, any number of fixed ones: localBA holds every observing frame outside the keyframe list, and a
 *              point keeps the observers of every frame that ever saw it),
 *              points point_off[p] .. (all free) and observations obs_off[p] .. (frame i, point j, pixel u; i and j
 *              local to the problem).  Observations are grouped by point, points ascending, every point with at
 *              least two and no (frame, point) twice.
 *   residual   e = u - proj(T_i X_j), proj(c) = (f c.x / c.z + cx, f c.y / c.z + cy), f = cam->fx on BOTH axes
 *              (setupG2o passes g2o::CameraParameters(fx, principalPoint, 0), :333: fy is never used); no
 *              cheirality test
 *   cost       Huber of width huber_delta on e2 = e.e: rho = e2 while sqrt(e2) <= delta, else
 *              2 delta sqrt(e2) - delta^2; weight w = 1 or delta / sqrt(e2); information identity; chi = sum rho
 *   step       pose <- exp(dp) * pose, dp = (upsilon; omega); X <- X + dx; with c = T_i X_j and A = d proj / d c:
 *              J_p = A [I | -hat(c)], J_x = A R_i, H = sum w J^T J, b = sum w J^T e, (H + lambda I) dx = b, the
 *              points eliminated first (Schur complement), Cholesky on the reduced system
 *   schedule   lambda = 1e-5 * max diag(H) at the first linearisation, nu = 2.  Per iteration: cur = chi, build
 *              H and b, then trials: solve, apply to a copy, tmp = chi(copy),
 *              r = (cur - tmp) / (dx.(lambda dx + b) + 1e-3).  r > 0 and tmp finite: accept,
 *              lambda *= max(1/3, min(1 - (2r-1)^3, 2/3)), nu = 2, next iteration.  Otherwise (also a non-positive
 *              Cholesky pivot, recorded with r = 0 and chi = cur) lambda *= nu, nu *= 2; after 5 failed trials the
 *              problem terminates.  At most max_iterations iterations (the reference passes 10).
 *   structure  when structure_iterations > 0 every point is first adjusted on its own with all poses held
 *              (StructureOnlySolver<3>::calc, :556-564): the same cost and schedule on its 3x3 system with its own
 *              lambda and nu, a point that fails 5 trials stops
 *   poses_inout  n_frames x 7, only free frames are written        frame_fixed  n_frames (uint8)
 *   points_inout n_points x 3                                      obs_px       n_obs x 2
 *   obs_chi2   n_obs: the non-robust e2 at the final estimate (edge->chi2(), :466, :603)
 *   init_chi, final_chi  the robust sums before and after the joint run
 *   iterations accepted iterations          status  0: ran max_iterations, 1: 5 failed trials, -1: no points
 *              (a problem without points or frames leaves everything as given)
 *   trace      NULL, or n_problems x SVO_BA_TRACE_CAP x 6: per trial (iteration, trial, accepted, lambda, r, chi) in
 *              order; unused records have iteration -1, trials past the capacity are dropped
 * A problem whose frames are all fixed is a structure-only problem (its reduced system is empty).  Every sum runs
 * in an order fixed by the layout and no floating-point atomics are used: equal inputs give equal bytes.
 * SVO_ERR_ARG: more than SVO_BA_MAX_FRAMES free frames in a problem, observations not grouped by ascending point, a
 * duplicate (frame, point), an index out of range, a point with fewer than two observations.  Synchronous. */
#define SVO_BA_MAX_FRAMES 16
#define SVO_BA_TRACE_CAP 64
int svo_bundle_adjust(svo_ctx* ctx, const svo_camera* cam, int32_t n_problems, const int32_t* frame_off,
                      const int32_t* point_off, const int32_t* obs_off, double* poses_inout,
                      const uint8_t* frame_fixed, double* points_inout, const int32_t* obs_frame,
                      const int32_t* obs_point, const double* obs_px, double huber_delta, int32_t max_iterations,
                      int32_t structure_iterations, double* obs_chi2, double* init_chi, double* final_chi,
                      int32_t* iterations, int32_t* status, double* trace);

/* ---------------------------------------------------------------- sparse optical flow (pyramidal Lucas-Kanade)
 * Replaces the tracking inside algorithm::computeOpticalFlowSparse (src/algorithm.cpp:29-107, called
 * src/system.cpp:128-129), which hands the two base images to cv::calcOpticalFlowPyrLK (window patchSize^2, maxLevel 3,
 * 30 iterations, eps 1e-4, OPTFLOW_USE_INITIAL_FLOW), for n_pairs independent frame pairs.  OpenCV is not part of the
 * reference tree; the arithmetic below is THIS PROJECT'S CONTRACT, modelled on calcOpticalFlowPyrLK and NOT pinned to
 * OpenCV's bits.  The pyramid is the intensity stack of svo_pyramid_set_build (level l = pyrDown of level l-1).
 *   ref_set, cur_set  two pyramid sets of equal geometry; frames: n_pairs x 2 frame indices (ref in ref_set, cur in
 *                     cur_set)
 *   feat_off   n_pairs + 1, laid out as for svo_triangulate_dlt: pair p owns points feat_off[p] .. feat_off[p+1]-1
 *   ref_px     n x 2
 *   cur_px     n x 2, in: the initial flow (the reference passes the ref positions); out: the tracked positions
 *   status     n (uint8): 1 tracked, 0 lost
 *   trace      NULL, or n x (max_level+1) x 2 int32: per level l (index l) the iterations run (steps computed) and an
 *              exit code: 0 level skipped (above L, below), 1 eps, 2 oscillation, 3 iteration limit, 4 left the
 *              image, 5 template out of range, 6 min-eigenvalue / determinant reject
 *   median_disparity  NULL, or n_pairs: algorithm::computeMedian (src/algorithm.cpp:813-832, a real std::nth_element)
 *              of the pair's disparities (:74): per tracked point the double norm of the float32 differences
 *              ref.x - cur.x, ref.y - cur.y of the float32 positions; NaN for a pair without tracked points
 * Per point, with h = (win - 1) / 2, W_l x H_l the size of level l and I / J the ref / cur intensity planes:
 *   1 ref_px and the initial cur_px are rounded to float32 (the reference's static_cast<float>); all later state is
 *     double.
 *   2 L is the largest l <= max_level with W_l > win and H_l > win (0 if there is none).  Levels L .. 0 are processed;
 *     the flow starts as cur / 2^L and is doubled between levels.
 *   3 template: p = ref / 2^l - h, ip = floor(p), (a, b) = p - ip.  Unless -win <= ip.x < W_l and -win <= ip.y < H_l:
 *     exit 5; at level 0 status = 0, at another level the level is skipped and the flow carries on.
 *     iw00 = rint((1-a)(1-b) 2^14), iw01 = rint(a (1-b) 2^14), iw10 = rint((1-a) b 2^14) (ties to even),
 *     iw11 = 2^14 - iw00 - iw01 - iw10; descale(v, k) = (v + 2^(k-1)) >> k (arithmetic shift).
 *     For the win^2 pixels (x, y), 0 <= x, y < win, at X = ip.x + x, Y = ip.y + y:
 *       S(F) = iw00 F(X, Y) + iw01 F(X+1, Y) + iw10 F(X, Y+1) + iw11 F(X+1, Y+1)
 *       T = descale(S(I), 9) (5 extra bits); I outside the image is BORDER_REFLECT_101 (one reflection, then clamped)
 *       Ix(X, Y) = 3 (I(X+1,Y-1) - I(X-1,Y-1)) + 10 (I(X+1,Y) - I(X-1,Y)) + 3 (I(X+1,Y+1) - I(X-1,Y+1)) (Scharr), Iy
 *       likewise with the axes exchanged, REFLECT_101 inside the 3x3; Ix = Iy = 0 where (X, Y) is outside the image
 *       gx = descale(S(Ix), 14), gy = descale(S(Iy), 14)
 *   4 A11 = sum gx^2, A12 = sum gx gy, A22 = sum gy^2: exact 64-bit integer sums, then converted to double and
 *     multiplied by 2^-20.  D = A11 A22 - A12 A12,
 *     minEig = (A22 + A11 - sqrt((A11 - A22)(A11 - A22) + 4 A12 A12)) / (2 win^2).
 *     minEig < min_eig_threshold or D < FLT_EPSILON: exit 6, status as in step 3.
 *   5 q = flow - h, prev = (0, 0); for j < max_iterations: iq = floor(q); the range test of step 3 on iq, failing:
 *     exit 4, status = 0 at level 0.  With the weights of q - iq: d = descale(S(J), 9) - T per pixel;
 *     b1 = sum d gx, b2 = sum d gy (exact 64-bit integer sums) times 2^-20;
 *     delta = ((A12 b2 - A22 b1) (1 / D), (A12 b1 - A11 b2) (1 / D)); q += delta.
 *     delta.delta <= epsilon^2: exit 1.  j > 0 and |delta.x + prev.x| < 0.01 and |delta.y + prev.y| < 0.01:
 *     q -= delta / 2, exit 2.  Otherwise prev = delta.  j reaching max_iterations: exit 3.
 *     The flow becomes q + h (also after exit 4).
 *   6 cur_px = the level-0 flow rounded to float32 and widened (what a cv::Point2f holds), written for every point;
 *     status = 1 unless cleared above.
 * Every sum is over integers and the double tail uses IEEE add, multiply, divide and sqrt only (no contraction), so
 * equal inputs give equal bytes, equal to a CPU restatement.
 * SVO_ERR_ARG: win even, < 3 or > SVO_KLT_MAX_WIN, max_level < 0 (these before anything else is looked at),
 * max_level >= the sets' level count, sets of different geometry, a frame index out of range.  Waits for a pending
 * svo_pyramid_set_build_async of either set and for pending alignment chains.  Synchronous. */
#define SVO_KLT_MAX_WIN 21
int svo_klt_track(svo_ctx* ctx, const svo_pyramid_set* ref_set, const svo_pyramid_set* cur_set, int32_t n_pairs,
                  const int32_t* frames, const int32_t* feat_off, const double* ref_px, double* cur_px, int32_t win,
                  int32_t max_level, int32_t max_iterations, double epsilon, double min_eig_threshold, uint8_t* status,
                  int32_t* trace, double* median_disparity);

/* ---------------------------------------------------------------- essential-matrix RANSAC
 * Replaces algorithm::computeEssentialMatrix's cv::findEssentialMat(ref, cur, K, RANSAC, 0.999, 1.0, status)
 * (src/algorithm.cpp:109-171, called src/system.cpp:137) for n_pairs independent frame pairs.  OpenCV is not part of
 * the reference tree; the arithmetic below is THIS PROJECT'S CONTRACT, modelled on findEssentialMat (five-point minimal
 * solver, Sampson distance on normalised coordinates, threshold over the mean focal length, confidence-driven sample
 * count, the best minimal model returned without refinement) and NOT pinned to OpenCV's samples or bits.
 * The convention is the one svo_two_view_init consumes: cur^T E ref = 0, E = [t]x R for X_cur = R X_ref + t.
 * Matches are laid out by feat_off as for svo_triangulate_dlt: pair p owns matches feat_off[p] .. feat_off[p+1]-1.
 *
 * svo_essential_score: the inliers of given models.
 *   hyp_off   n_pairs + 1: pair p owns models hyp_off[p] .. hyp_off[p+1]-1 of E_hyp (m x 9, row-major)
 *   counts    m: the inliers of each model among its pair's matches
 *   mask      NULL, or n (uint8): per pair the inlier mask of its first model with the strictly largest count (a count
 *             of 0 never wins: the mask is then 0)
 * Per match: both pixels are rounded to float32 and widened (the reference's static_cast<float>), x = (u - cx) / fx,
 * y = (v - cy) / fy.  With x1 = ref, x2 = cur and every product and sum one rounded IEEE operation in the written order
 *   a_i = (E_i0 x1.x + E_i1 x1.y) + E_i2                 (i = 0, 1, 2)
 *   b_j = (E_0j x2.x + E_1j x2.y) + E_2j                 (j = 0, 1)
 *   num = (x2.x a_0 + x2.y a_1) + a_2
 *   den = ((a_0 a_0 + a_1 a_1) + b_0 b_0) + b_1 b_1
 *   err = (num num) / den
 * and the match is an inlier iff err <= thr2, thr = threshold / ((fx + fy) / 2), thr2 = thr thr (a NaN never is).
 *
 * svo_essential_ransac:
 *   ref_px, cur_px  n x 2, not modified;  threshold in pixels (the reference passes 1.0), confidence (0.999),
 *   max_iterations (1000; 1 .. SVO_ESSENTIAL_MAX_ITERATIONS), seed
 *   E           n_pairs x 9 row-major, Frobenius norm 1 (its sign is unspecified)
 *   mask        n (uint8): the winner's inliers;  n_inliers  n_pairs: their number
 *   iterations  n_pairs: samples consumed;  best  n_pairs x 2: the winner's sample h and its solution index k
 *   status      n_pairs: 0 ok; -1 fewer than 5 matches or no sample produced a model with an inlier: E and mask are 0,
 *               best is -1
 *   hyp_E, hyp_count  both NULL, or the trace: n_pairs x max_iterations x 10 x 9 models and n_pairs x max_iterations
 *               x 10 counts (-1: the sample has no such solution; -2: a sample past `iterations`, its models 0)
 * Per pair p with n_p matches:
 *   1 sampling, integer only.  mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31 (64-bit, the splitmix64 finaliser).  Draw c = 0 .. 255 of
 *     sample h is r = mix(seed ^ (p << 44) ^ (h << 8) ^ c), index ((r >> 32) * n_p) >> 32; a draw equal to an index
 *     already held is skipped; the first five distinct indices are the sample; a sample without five by c = 255 has no
 *     models.
 *   2 five-point solver.  The models of a sample are the real solutions of Nister's system: E in the four-dimensional
 *     null space of the five epipolar equations x2^T E x1 = 0 on the normalised points, E = x X + y Y + z Z + W,
 *     with det E = 0 and E E^T E - tr(E E^T) E / 2 = 0 (ten cubics in x, y, z).  How the null space and the starting
 *     roots are found is not part of the contract (here: Householder QR, Gauss-Jordan of the 10 x 20 system, the roots
 *     of det B(z) by simultaneous Ehrlich-Aberth iteration).  Every starting root is polished by Gauss-Newton on the
 *     ten cubics in (x, y, z), for as long as the scaled residual |c| / |E|_F^3 decreases and at most 10 steps; a root
 *     whose polished scaled residual exceeds 1e-9 is discarded, as is one whose unit model lies within 1e-6 (largest
 *     entry difference, up to sign) of one already kept.  The models are scaled to Frobenius norm 1; their order
 *     within a sample is unspecified.
 *   3 every model is scored with the arithmetic of svo_essential_score.
 *   4 stopping rule, sequential in definition: best = 0, niters = max_iterations; for h = 0, 1, .. while h < niters:
 *     a model of sample h with a strictly larger count than best becomes the winner (k ascending); after sample h, if
 *     best rose, niters = update(confidence, (n_p - best) / n_p, max_iterations), evaluated in double with std::log
 *     and std::pow: num = max(1 - confidence, DBL_MIN), den = 1 - (1 - ep)^5; den < DBL_MIN: 0; log den >= 0 or
 *     -log num >= max_iterations (-log den): max_iterations; otherwise rint(log num / log den).
 *     `iterations` is the h at which the loop ends.  Samples are computed in rounds; the result does not depend on
 *     the rounds.
 *   5 mask = the winner's inliers, n_inliers their count, E the winner.
 * Every count is an integer sum; there are no floating-point atomics: equal inputs give equal bytes.
 * SVO_ERR_ARG: threshold <= 0, confidence outside (0, 1), max_iterations outside 1 .. 65536, feat_off not ascending
 * (all of these before the context is looked at), more than 65535 pairs in one svo_essential_ransac call, a null
 * argument, one of hyp_E / hyp_count without the other.
 * Synchronous; waits for pending alignment chains. */
#define SVO_ESSENTIAL_MAX_ITERATIONS 65536
int svo_essential_score(svo_ctx* ctx, const svo_camera* cam, int32_t n_pairs, const int32_t* feat_off,
                        const int32_t* hyp_off, const double* E_hyp, const double* ref_px, const double* cur_px,
                        double threshold, int32_t* counts, uint8_t* mask);
int svo_essential_ransac(svo_ctx* ctx, const svo_camera* cam, int32_t n_pairs, const int32_t* feat_off,
                         const double* ref_px, const double* cur_px, double threshold, double confidence,
                         int32_t max_iterations, uint64_t seed, double* E, uint8_t* mask, int32_t* n_inliers,
                         int32_t* iterations, int32_t* best, int32_t* status, double* hyp_E, int32_t* hyp_count);

/* ---------------------------------------------------------------- lens undistortion ahead of the pyramid
 * Replaces PinholeCamera's undistortion: the map its constructor builds with cv::initUndistortRectifyMap(K, d, I, K,
 * size, CV_16SC2, ..) (src/pinhole_camera.cpp:7-48) and PinholeCamera::undistortImage = cv::remap(.., INTER_LINEAR)
 * over it (:178-184; pinned by tests/test_camera.cpp:105-130 against a recorded image).  The reference's System never
 * calls undistortImage; here the step runs on the device between the upload and the pyramid build, so that everything
 * behind a Frame sees the ideal pinhole svo_camera.  OpenCV is not part of the reference tree; the arithmetic below is
 * THIS PROJECT'S CONTRACT, modelled on OpenCV's fixed-point remap.  On the one recorded OpenCV result the reference
 * ships (1280 x 960, green channel) it differs in 47 of 1 228 800 bytes, by at most 3 grey levels, each at a pixel
 * whose u * 32 or v * 32 lies within 0.002 of a rounding tie (tests/test_undistort.py).
 *
 * Inputs: the camera (fx, fy, cx, cy, width, height) and d = (k1, k2, p1, p2, k3) in OpenCV's order; the output camera
 * matrix equals the input one.  Map, per output pixel (j, i), in IEEE double, every operation rounded once, in exactly
 * this order (left to right, no contraction):
 *   x = (j - cx) / fx            y = (i - cy) / fy
 *   x2 = x*x   y2 = y*y   r2 = x2 + y2   xy2 = 2*x*y
 *   kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2
 *   xd = x*kr + p1*xy2 + p2*(r2 + 2*x2)
 *   yd = y*kr + p1*(r2 + 2*y2) + p2*xy2
 *   u  = fx*xd + cx              v  = fy*yd + cy
 *   iu = rint(u*32)   iv = rint(v*32)        (ties to even; as int32 after saturation)
 *   X = iu >> 5   Y = iv >> 5   ax = iu & 31   ay = iv & 31      (arithmetic shift)
 * Remap, in integers: the taps are (Y,X), (Y,X+1), (Y+1,X), (Y+1,X+1); a tap outside the image contributes 0
 * (BORDER_CONSTANT with value 0, cv::remap's default);
 *   out = ((32-ax)*(32-ay)*p00 + ax*(32-ay)*p01 + (32-ax)*ay*p10 + ax*ay*p11 + 512) >> 10
 * (the fractions are multiples of 1/32, so OpenCV's 15-bit weight table is exactly a*b*32 and its sum correction never
 * fires).  Stored map: X clamped to [-2, width], Y to [-2, height] (every position beyond gives 0 either way), which
 * fits int16 up to 32767 x 32767; a larger camera is SVO_ERR_ARG.
 * When to apply (the mirrors' rule): when any of the five coefficients is non-zero (the reference tests |k1| > 1e-5
 * alone and would skip a purely tangential lens).  With all five zero nothing of this section runs.
 *
 * Two host helpers of the mirrors (PinholeCamera::raw_pixel / undistorted_pixel) carry points between the raw and the
 * undistorted image in the same double arithmetic: raw_pixel(p) is the unrounded (u, v) above; undistorted_pixel(raw)
 * inverts it by x <- (xd - tangential(x)) / kr(x), y likewise, SVO_UNDISTORT_POINT_ITERATIONS times from the distorted
 * normalised point (xd, yd) = ((u - cx) / fx, (v - cy) / fy), with tangential = (p1*xy2 + p2*(r2 + 2*x2),
 * p1*(r2 + 2*y2) + p2*xy2) and kr as above at the current (x, y); the result is (fx*x + cx, fy*y + cy). */
typedef struct svo_undistort_map svo_undistort_map;
typedef struct {
    double k1, k2, p1, p2, k3;
} svo_distortion;
#define SVO_UNDISTORT_POINT_ITERATIONS 40
/* Build the device-resident map of one camera (queued on the context stream; every later use is ordered after it). */
int svo_undistort_map_create(svo_ctx* ctx, const svo_camera* cam, const svo_distortion* d, svo_undistort_map** out);
int svo_undistort_map_destroy(svo_undistort_map* map);
/* The map as OpenCV's CV_16SC2 + CV_16UC1 pair: xy height*width*2 (X, Y per pixel), frac height*width
 * ((ay << 5) | ax).  Synchronous. */
int svo_undistort_map_download(const svo_undistort_map* map, int16_t* xy, uint16_t* frac);
/* PinholeCamera::undistortImage for `count` images (count*width*height bytes in, as many out).  Synchronous. */
int svo_undistort_images(svo_ctx* ctx, const svo_undistort_map* map, const uint8_t* host_in, uint8_t* host_out,
                         int32_t count);
/* svo_pyramid_set_upload / _upload_device of RAW images: they are remapped into level 0 of frames
 * [first, first+count) (the host form stages them in the context's per-call device block first).  Stream-ordered like
 * the plain uploads, with the same waits with respect to svo_pyramid_set_build_async.  SVO_ERR_ARG when the map's size
 * differs from the set's or the map belongs to another context. */
int svo_pyramid_set_upload_undistort(svo_pyramid_set* set, int32_t first, int32_t count, const uint8_t* host_images,
                                     const svo_undistort_map* map);
int svo_pyramid_set_upload_undistort_device(svo_pyramid_set* set, int32_t first, int32_t count,
                                            const uint8_t* dev_images, const svo_undistort_map* map);

/* ---------------------------------------------------------------- pixel formats: colour and 16-bit frames to grey
 * Replaces the cv::imread(.., IMREAD_GRAYSCALE) the reference reads every frame with (src/main.cpp:105): the step from
 * what a camera, a decoder or a file holds to the 8-bit grey plane that is level 0 of a pyramid.  It runs on the device
 * on the frame's way into the set, ahead of the undistortion (convert first, then remap).  The arithmetic below is THIS
 * PROJECT'S CONTRACT, in integers:
 *   colour (BGR8, RGB8, BGRA8, RGBA8; one byte per channel in the named order; alpha is ignored):
 *       Y = (4899*R + 9617*G + 1868*B + 8192) >> 14
 *     The weights sum to 16384, so R = G = B = v gives v and nothing saturates.  This is the rule OpenCV documents for
 *     its 8-bit COLOR_BGR2GRAY / COLOR_RGB2GRAY and the rule tests/golden/make_golden_refimages.py built refimages.npz
 *     with.  OpenCV is not part of the reference tree or of this project's build, so there is NO recorded OpenCV result
 *     that anchors it; and it is not claimed to equal imread(IMREAD_GRAYSCALE), which converts inside libpng / libjpeg.
 *   GRAY16 (native-endian uint16):
 *       Y = min(255, v >> shift)        shift in 0..8
 *     shift = 8 keeps the high byte, which is what an 8-bit imread keeps of a 16-bit PNG; shift = 4 serves 12-bit
 *     sensors.
 *   GRAY8: a copy that honours the strides (a decoder's pitched luma plane).
 * Layout: `count` images of width x height pixels; row y of image k starts at byte k*image_stride + y*row_stride.  A
 * stride of 0 means packed: row_stride = width*bytes_per_pixel, image_stride = row_stride*height.  The bytes a call
 * reads are exactly [0, image_stride*(count-1) + row_stride*(height-1) + width*bytes_per_pixel): no byte before the
 * pointer and none past that end is touched, whatever the pointer's alignment.  A GRAY16 pointer and GRAY16 strides are
 * even; nothing else is required of the pointer's or the strides' alignment. */
enum { SVO_PIXEL_GRAY8 = 0, SVO_PIXEL_BGR8, SVO_PIXEL_RGB8, SVO_PIXEL_BGRA8, SVO_PIXEL_RGBA8, SVO_PIXEL_GRAY16 };
typedef struct {
    int32_t format;        /* SVO_PIXEL_* */
    int32_t shift;         /* GRAY16 only: 0..8; ignored otherwise */
    int64_t row_stride;    /* bytes between rows;   0 = width * bytes_per_pixel */
    int64_t image_stride;  /* bytes between images; 0 = row_stride * height */
} svo_image_layout;
/* Host only: the number of bytes a call with this layout reads (0 for count = 0).  SVO_ERR_ARG with a text for an
 * unknown format, a GRAY16 shift outside 0..8, a row stride below width*bytes_per_pixel, an image stride below
 * row_stride*(height-1) + width*bytes_per_pixel, an odd GRAY16 stride, width or height < 1, count < 0.  Every entry
 * point below validates its layout through this function. */
int svo_image_layout_bytes(const svo_image_layout* layout, int32_t width, int32_t height, int32_t count,
                           int64_t* bytes);
/* `count` images to grey, host to host (count*width*height bytes out, packed).  Synchronous; the counterpart of
 * svo_undistort_images. */
int svo_convert_images(svo_ctx* ctx, const svo_image_layout* layout, int32_t width, int32_t height, int32_t count,
                       const void* host_in, uint8_t* host_out);
/* svo_pyramid_set_upload / _upload_device of images in `layout` (width and height are the set's): they are converted
 * into level 0 of frames [first, first+count).  `map` may be NULL; with a map the result is, bit for bit, the grey
 * image of the contract above remapped by the undistortion contract.  Stream order and waits are those of the plain
 * uploads; the host form stages the raw bytes in the context's per-call device block first.  SVO_ERR_ARG for a NULL
 * layout, an odd GRAY16 pointer, a map of another size or of another context. */
int svo_pyramid_set_upload_format(svo_pyramid_set* set, int32_t first, int32_t count, const void* host_images,
                                  const svo_image_layout* layout, const svo_undistort_map* map);
int svo_pyramid_set_upload_format_device(svo_pyramid_set* set, int32_t first, int32_t count, const void* dev_images,
                                         const svo_image_layout* layout, const svo_undistort_map* map);

#ifdef __cplusplus
}
#endif

#endif /* SVO_C_H */
