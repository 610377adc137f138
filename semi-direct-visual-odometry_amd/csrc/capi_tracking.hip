// capi_tracking.hip — C ABI: FeatureAlignment over candidates (feature_align.hip), pyramidal Lucas-Kanade (klt.hip).
#include <cmath>

#include "capi_ctx.h"
using namespace svo::shim;

// One FeatureAlignment launch over n candidates whose reference gradient planes are rg[i].
static int feature_align_impl(svo_ctx* c, const svo_camera* cam, int32_t patch_size, const std::vector<const uint8_t*>& rg,
                              const svo_pyramid_set* cur_set, int32_t cur_frame, int32_t n, const double* ref_px,
                              double* px_inout, double* err, int32_t* status) {
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    // one block, same layout both sides; one H2D copy (planes .. px), one D2H (px .. status, with room for n doubles)
    const size_t nn = (size_t)n;
    svo::FeatureAlignArgs a;
    Block blk(c, s);
    blk.in(&a.ref_grad, rg.data(), nn);
    blk.in(&a.ref_px, ref_px, 2 * nn);
    blk.inout(&a.px, px_inout, 2 * nn);
    blk.out(&a.err, err, nn);
    blk.out(&a.status, status, nn, 2 * nn);
    a.cur_grad = cur_set->d_base + (size_t)cur_frame * cur_set->stride + cur_set->grad_off;
    a.n = n; a.width = cam->width; a.height = cam->height;
    a.half = patch_size / 2;
    a.area = (2 * a.half + 1) * (2 * a.half + 1);
    if (blk.alloc(Block::kPageable) == hipSuccess) blk.run([&] { svo::launch_feature_align(a, s); });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_feature_align: %s", hipGetErrorString(blk.err));
    return SVO_OK;
}

static int feature_align_check(svo_ctx* c, const svo_camera* cam, int32_t patch_size, const svo_pyramid_set* cur_set,
                               int32_t cur_frame, int32_t n, const double* ref_px, const double* px_inout) {
    if (!c || !cam || !cur_set || (n > 0 && (!ref_px || !px_inout))) return fail(SVO_ERR_ARG, "null argument");
    if (n < 0) return fail(SVO_ERR_ARG, "n < 0");
    if (patch_size < 1 || (2 * (patch_size / 2) + 1) * (2 * (patch_size / 2) + 1) > 128)
        return fail(SVO_ERR_ARG, "patch_size %d unsupported (footprint must be <= 128 px)", patch_size);
    if (int r = check_set(c, cur_set, cam)) return r;
    if (cur_frame < 0 || cur_frame >= cur_set->n_frames) return fail(SVO_ERR_ARG, "cur_frame out of range");
    return SVO_OK;
}

// src/algorithm.cpp:64-79 (float32 differences, double norm, computeMedian); kept out of svo_klt_track: DESIGN 26
static void klt_median_disparity(int32_t n_pairs, const int32_t* feat_off, const double* ref_px, const double* cur_px,
                                 const uint8_t* status, double* median_disparity) {
    std::vector<double> disp;
    for (int32_t p = 0; p < n_pairs; ++p) {
        disp.clear();
        for (int64_t k = feat_off[p]; k < feat_off[p + 1]; ++k) {
            if (!status[k]) continue;
            const double dx = (double)((float)ref_px[2 * k] - (float)cur_px[2 * k]);
            const double dy = (double)((float)ref_px[2 * k + 1] - (float)cur_px[2 * k + 1]);
            disp.push_back(std::sqrt(dx * dx + dy * dy));
        }
        median_disparity[p] = svo::two_view_median(disp.data(), (int64_t)disp.size());
    }
}

extern "C" {
int svo_feature_align(svo_ctx* c, const svo_camera* cam, int32_t patch_size, const svo_pyramid_set* ref_set,
                      const int32_t* ref_frames, int32_t ref_frame, const svo_pyramid_set* cur_set, int32_t cur_frame,
                      int32_t n, const double* ref_px, double* px_inout, double* err, int32_t* status) {
    if (int r = feature_align_check(c, cam, patch_size, cur_set, cur_frame, n, ref_px, px_inout)) return r;
    if (!ref_set) return fail(SVO_ERR_ARG, "null argument");
    if (int r = check_set(c, ref_set, cam)) return r;
    if (n == 0) return SVO_OK;
    SVO_HIP(set_join(ref_set));
    SVO_HIP(set_join(cur_set));
    std::vector<const uint8_t*> rg(n);
    for (int32_t i = 0; i < n; ++i) {
        const int32_t f = ref_frames ? ref_frames[i] : ref_frame;
        if (f < 0 || f >= ref_set->n_frames) return fail(SVO_ERR_ARG, "ref frame %d out of range", f);
        rg[i] = ref_set->d_base + (size_t)f * ref_set->stride + ref_set->grad_off;
    }
    return feature_align_impl(c, cam, patch_size, rg, cur_set, cur_frame, n, ref_px, px_inout, err, status);
}

int svo_feature_align_multi(svo_ctx* c, const svo_camera* cam, int32_t patch_size, const svo_pyramid_set* const* ref_sets,
                            const int32_t* ref_frames, const svo_pyramid_set* cur_set, int32_t cur_frame, int32_t n,
                            const double* ref_px, double* px_inout, double* err, int32_t* status) {
    if (int r = feature_align_check(c, cam, patch_size, cur_set, cur_frame, n, ref_px, px_inout)) return r;
    if (n > 0 && (!ref_sets || !ref_frames)) return fail(SVO_ERR_ARG, "null argument");
    if (n == 0) return SVO_OK;
    std::vector<const uint8_t*> rg(n);
    for (int32_t i = 0; i < n; ++i) {
        const svo_pyramid_set* p = ref_sets[i];
        if (int r = check_set(c, p, cam, "candidate", i)) return r;
        if (ref_frames[i] < 0 || ref_frames[i] >= p->n_frames)
            return fail(SVO_ERR_ARG, "ref frame %d out of range", ref_frames[i]);
        rg[i] = p->d_base + (size_t)ref_frames[i] * p->stride + p->grad_off;
        SVO_HIP(set_join(p));
    }
    SVO_HIP(set_join(cur_set));
    return feature_align_impl(c, cam, patch_size, rg, cur_set, cur_frame, n, ref_px, px_inout, err, status);
}

int svo_klt_track(svo_ctx* c, const svo_pyramid_set* ref_set, const svo_pyramid_set* cur_set, int32_t n_pairs,
                  const int32_t* frames, const int32_t* feat_off, const double* ref_px, double* cur_px, int32_t win,
                  int32_t max_level, int32_t max_iterations, double epsilon, double min_eig_threshold, uint8_t* status,
                  int32_t* trace, double* median_disparity) {
    // the scalar parameters first: these need neither a context nor a set
    if (win < 3 || win > SVO_KLT_MAX_WIN || win % 2 == 0)
        return fail(SVO_ERR_ARG, "svo_klt_track: win %d must be odd and within 3..%d", win, SVO_KLT_MAX_WIN);
    if (max_level < 0) return fail(SVO_ERR_ARG, "svo_klt_track: max_level < 0");
    if (max_iterations < 0) return fail(SVO_ERR_ARG, "svo_klt_track: max_iterations < 0");
    int64_t n = 0;
    if (int r = check_pair_offsets("svo_klt_track", n_pairs, feat_off, &n)) return r;
    if (!c || !ref_set || !cur_set || (n_pairs > 0 && !frames) || (n > 0 && (!ref_px || !cur_px || !status)))
        return fail(SVO_ERR_ARG, "svo_klt_track: null argument");
    if (int r = check_set(c, ref_set, nullptr, "svo_klt_track: ")) return r;
    if (int r = check_set(c, cur_set, nullptr, "svo_klt_track: ")) return r;
    if (ref_set->width != cur_set->width || ref_set->height != cur_set->height || ref_set->levels != cur_set->levels)
        return fail(SVO_ERR_ARG, "svo_klt_track: the sets differ in geometry (%dx%d, %d levels vs %dx%d, %d levels)",
                    ref_set->width, ref_set->height, ref_set->levels, cur_set->width, cur_set->height, cur_set->levels);
    if (max_level >= ref_set->levels)
        return fail(SVO_ERR_ARG, "svo_klt_track: max_level %d, the sets hold %d levels", max_level, ref_set->levels);
    for (int32_t p = 0; p < n_pairs; ++p)
        if (frames[2 * p] < 0 || frames[2 * p] >= ref_set->n_frames || frames[2 * p + 1] < 0 ||
            frames[2 * p + 1] >= cur_set->n_frames)
            return fail(SVO_ERR_ARG, "svo_klt_track: pair %d: frame index out of range", p);
    if (median_disparity)
        for (int32_t p = 0; p < n_pairs; ++p) median_disparity[p] = std::nan("");
    if (n_pairs == 0 || n == 0) return SVO_OK;
    SVO_HIP(hipSetDevice(c->device));
    SVO_HIP(set_join(ref_set));
    SVO_HIP(set_join(cur_set));
    hipStream_t s = ctx_stream(c);
    const size_t P = (size_t)n_pairs, N = (size_t)n;
    svo::KltArgs a{};
    Block blk(c, s);
    blk.in(&a.feat_off, feat_off, P + 1);
    blk.in(&a.frames, frames, P * 2);
    blk.in(&a.ref_px, ref_px, N * 2);
    blk.inout(&a.cur_px, cur_px, N * 2);
    blk.out(&a.status, status, N);
    blk.out(&a.trace, trace, trace ? N * (size_t)(max_level + 1) * 2 : 0);
    if (blk.alloc() != hipSuccess) return fail(SVO_ERR_HIP, "svo_klt_track scratch: %s", hipGetErrorString(blk.err));
    if (!trace) a.trace = nullptr;
    a.ref_base = ref_set->d_base; a.ref_stride = ref_set->stride;
    a.cur_base = cur_set->d_base; a.cur_stride = cur_set->stride;
    a.n = (int32_t)n; a.n_pairs = n_pairs; a.win = win; a.max_level = max_level; a.max_iterations = max_iterations;
    a.epsilon = epsilon; a.min_eig = min_eig_threshold;
    a.geom = ref_set->geom;
    blk.run([&] { svo::launch_klt(a, s); });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_klt_track: %s", hipGetErrorString(blk.err));
    if (median_disparity) klt_median_disparity(n_pairs, feat_off, ref_px, cur_px, status, median_disparity);
    return SVO_OK;
}
}  // extern "C"
