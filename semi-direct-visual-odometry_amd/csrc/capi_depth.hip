// capi_depth.hip — C ABI: the depth filter's seed update (kernel: depth_filter.hip).
#include <cmath>

#include "capi_ctx.h"
using namespace svo::shim;

extern "C" {
int svo_depth_seed_init(double depth_mean, double depth_min, svo_depth_seed* seed) {
    if (!seed) return fail(SVO_ERR_ARG, "null seed");
    seed->a = 10;                          // src/mixed_gaussian_filter.cpp:10-11
    seed->b = 10;
    seed->mu = 1.0 / depth_mean;           // :13
    seed->max_depth = 1.0 / depth_min;     // :14
    seed->sigma = seed->max_depth / 6;     // :18
    seed->var = seed->sigma * seed->sigma; // :20
    seed->valid = 1;                       // :21
    return SVO_OK;
}

int svo_depth_update(svo_ctx* c, const svo_camera* cam, int32_t n_kf, const svo_pyramid_set* const* kf_sets,
                     const int32_t* kf_frames, const double* kf_poses, const svo_pyramid_set* cur_set,
                     int32_t cur_frame, const double* cur_pose, int32_t n, svo_depth_seed* seeds,
                     int32_t* n_out, int32_t* outcome, double* cand_points, int32_t* cand_seed, int32_t* n_cand) {
    if (!c || !cam || !cur_set || !cur_pose || !n_out || !n_cand || (n_kf > 0 && (!kf_sets || !kf_frames || !kf_poses)))
        return fail(SVO_ERR_ARG, "null argument");
    if (n < 0 || n_kf < 0) return fail(SVO_ERR_ARG, "negative count");
    if (n > 0 && (!seeds || !cand_points || !cand_seed)) return fail(SVO_ERR_ARG, "null seed / candidate array");
    if (int r = check_set(c, cur_set, cam)) return r;
    if (cur_frame < 0 || cur_frame >= cur_set->n_frames) return fail(SVO_ERR_ARG, "frame %d out of range", cur_frame);
    SVO_HIP(set_join(cur_set));
    std::vector<const uint8_t*> kimg(n_kf > 0 ? n_kf : 1);
    for (int32_t k = 0; k < n_kf; ++k) {
        if (int r = check_set(c, kf_sets[k], cam)) return r;
        if (kf_frames[k] < 0 || kf_frames[k] >= kf_sets[k]->n_frames)
            return fail(SVO_ERR_ARG, "frame %d out of range", kf_frames[k]);
        SVO_HIP(set_join(kf_sets[k]));
        kimg[k] = kf_sets[k]->d_base + (size_t)kf_frames[k] * kf_sets[k]->stride;  // intensity stack, level 0
    }
    for (int32_t i = 0; i < n; ++i)
        if (seeds[i].kf < 0 || seeds[i].kf >= n_kf) return fail(SVO_ERR_ARG, "seed %d: keyframe %d out of range", i, seeds[i].kf);
    *n_out = 0;
    *n_cand = 0;
    if (n == 0) return SVO_OK;
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    // one block, same layout on both sides: inputs, outputs, device-only scratch (updated seeds | points); one H2D and
    // one D2H copy through the context's pinned staging
    const size_t N = (size_t)n, K = (size_t)n_kf;
    int32_t counts[2];
    svo::DepthArgs a{};
    Block blk(c, s);
    blk.in(&a.seeds, seeds, N);
    blk.in(&a.kf_poses, kf_poses, K * 7);
    blk.in(&a.kf_imgs, kimg.data(), K);
    blk.in(&a.cur_pose, cur_pose, 7);
    blk.out(&a.counts, counts, 2);
    const auto d_out = blk.out(&a.seeds_out, nullptr, N);  // (survivors and candidates: only the counted rows go to
    blk.out(&a.outcome, outcome, N);                       //  the caller, below)
    const auto d_cpts = blk.out(&a.cand_points, nullptr, N * 3);
    const auto d_cseed = blk.out(&a.cand_seed, nullptr, N);
    blk.dev(&a.seeds_new, N);
    blk.dev(&a.points, N * 3);
    a.cur_img = cur_set->d_base + (size_t)cur_frame * cur_set->stride;
    a.n = n; a.width = cam->width; a.height = cam->height;
    fill_camera(a, cam);
    a.err_angle = std::atan(1.0 / (2.0 * cam->fx)) * 2.0;  // src/depth_estimator.cpp:202-206 (pixel noise 1)
    if (blk.alloc(Block::kPageable) == hipSuccess) blk.run([&] { svo::launch_depth_update(a, s); });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_depth_update: %s", hipGetErrorString(blk.err));
    std::memcpy(seeds, blk.host(d_out), (size_t)counts[0] * sizeof(svo_depth_seed));
    std::memcpy(cand_points, blk.host(d_cpts), (size_t)counts[1] * 24);
    std::memcpy(cand_seed, blk.host(d_cseed), (size_t)counts[1] * 4);
    *n_out = counts[0];
    *n_cand = counts[1];
    return SVO_OK;
}
}  // extern "C"
