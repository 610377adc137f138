// capi_two_view.hip — C ABI: two-view geometry on matches: map init, DLT (two_view.hip), RANSAC (essential.hip).
#include <algorithm>
#include <cmath>
#include <limits>

#include "capi_ctx.h"
using namespace svo::shim;

static int essential_scalars(const char* fn, double threshold) {
    if (!(threshold > 0.0) || !std::isfinite(threshold)) return fail(SVO_ERR_ARG, "%s: threshold must be positive and finite", fn);
    return SVO_OK;
}
static void essential_camera(svo::EssentialArgs& a, const svo_camera* cam, double threshold) {
    fill_camera(a, cam);
    // thr^2 on normalised coordinates: the pixel threshold over the mean focal length, squared
    const double thr = threshold / ((cam->fx + cam->fy) / 2.0);
    a.thr2 = thr * thr;
}

extern "C" {
int svo_triangulate_dlt(svo_ctx* c, const svo_camera* cam, int32_t n_pairs, const int32_t* feat_off,
                        const double* ref_poses, const double* cur_poses, const double* ref_px, const double* cur_px,
                        double* points_world) {
    int64_t n = 0;
    if (int r = check_pair_offsets("svo_triangulate_dlt", n_pairs, feat_off, &n)) return r;
    if (!c || !cam || (n_pairs > 0 && (!ref_poses || !cur_poses)) || (n > 0 && (!ref_px || !cur_px || !points_world)))
        return fail(SVO_ERR_ARG, "svo_triangulate_dlt: null argument");
    if (n_pairs == 0 || n == 0) return SVO_OK;
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    const size_t P = (size_t)n_pairs, N = (size_t)n;
    svo::TwoViewArgs a{};
    Block blk(c, s);
    blk.in(&a.feat_off, feat_off, P + 1);
    blk.in(&a.ref_poses, ref_poses, P * 7);
    blk.in(&a.cur_pose, cur_poses, P * 7);
    blk.in(&a.ref_px, ref_px, N * 2);
    blk.in(&a.cur_px, cur_px, N * 2);
    blk.out(&a.points_world, points_world, N * 3);
    fill_camera(a, cam);
    a.width = cam->width; a.height = cam->height; a.n_pairs = n_pairs;
    if (blk.alloc() != hipSuccess) return fail(SVO_ERR_HIP, "two-view scratch: %s", hipGetErrorString(blk.err));
    blk.run([&] { svo::launch_triangulate_dlt(a, s); });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_triangulate_dlt: %s", hipGetErrorString(blk.err));
    return SVO_OK;
}

int svo_two_view_init(svo_ctx* c, const svo_camera* cam, int32_t n_pairs, const int32_t* feat_off, const double* E,
                      const double* ref_poses, double map_scale, int32_t cell_size, double* ref_px, double* cur_px,
                      double* F, int32_t* counts, int32_t* winner, double* cur_poses, double* median_depth,
                      int32_t* n_valid, double* points_world, uint8_t* valid, int32_t* survivor, double* depth) {
    int64_t n = 0;
    if (int r = check_pair_offsets("svo_two_view_init", n_pairs, feat_off, &n)) return r;
    if (cell_size < 1) return fail(SVO_ERR_ARG, "svo_two_view_init: cell_size < 1");
    if (!(map_scale > 0.0) || !std::isfinite(map_scale))
        return fail(SVO_ERR_ARG, "svo_two_view_init: map_scale must be positive and finite");
    if (!c || !cam ||
        (n_pairs > 0 && (!E || !ref_poses || !F || !counts || !winner || !cur_poses || !median_depth || !n_valid)) ||
        (n > 0 && (!ref_px || !cur_px || !points_world || !valid || !survivor)))
        return fail(SVO_ERR_ARG, "svo_two_view_init: null argument");
    if (n_pairs == 0) return SVO_OK;
    const size_t P = (size_t)n_pairs, N = (size_t)n;
    // host: F and the four poses of every pair (these vectors outlive their copies: a sync() or finish() follows each)
    std::vector<double> hyp(28 * P), scale(P, 0.0), dep(N), pose(7 * P);
    for (size_t p = 0; p < P; ++p) {
        svo::two_view_fundamental(*cam, E + 9 * p, F + 9 * p);
        svo::two_view_hypotheses(E + 9 * p, hyp.data() + 28 * p);
    }
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    svo::TwoViewArgs a{};
    Block blk(c, s);
    blk.in(&a.feat_off, feat_off, P + 1);
    blk.in(&a.F, F, P * 9);
    blk.in(&a.ref_poses, ref_poses, P * 7);
    blk.in(&a.hyp, hyp.data(), P * 28);
    blk.inout(&a.ref_px, ref_px, N * 2);
    blk.inout(&a.cur_px, cur_px, N * 2);
    const auto d_cnt = blk.dev(&a.counts, P * 4);  // counts, winner, pose and depth come back after the vote (below)
    const auto d_win = blk.dev(&a.winner, P);
    const auto d_cp = blk.dev(&a.cur_pose, P * 7);
    blk.out(&a.points_world, points_world, N * 3);
    blk.dev(&a.points_cur, N * 3);
    const auto d_dep = blk.dev(&a.depth, N);
    const auto d_sc = blk.dev(&a.scale, P);
    blk.out(&a.valid, valid, N);
    blk.out(&a.survivor, survivor, N);
    blk.out(&a.n_valid, n_valid, P);
    fill_camera(a, cam);
    a.half_patch = std::ceil(static_cast<double>(cell_size) / 2.0);  // halfPatchSize (src/system.cpp:196)
    a.width = cam->width; a.height = cam->height; a.n_pairs = n_pairs;
    if (blk.alloc() != hipSuccess) return fail(SVO_ERR_HIP, "two-view scratch: %s", hipGetErrorString(blk.err));
    blk.upload();
    blk.launch([&] { svo::launch_two_view_vote(a, s); });
    blk.get(counts, d_cnt);
    blk.get(winner, d_win);
    blk.get(pose.data(), d_cp);
    blk.get(dep.data(), d_dep);
    blk.sync();
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_two_view_init: %s", hipGetErrorString(blk.err));
    // host: median depth, scale = map_scale / median and the rescaled pose of every pair that has a winner
    // (src/system.cpp:172-186); a failed pair keeps the caller's cur_poses row
    for (size_t p = 0; p < P; ++p) {
        median_depth[p] = std::numeric_limits<double>::quiet_NaN();
        if (winner[p] < 0) continue;
        median_depth[p] = svo::two_view_median(dep.data() + feat_off[p], feat_off[p + 1] - feat_off[p]);
        scale[p] = map_scale / median_depth[p];
        svo::two_view_rescale_pose(ref_poses + 7 * p, scale[p], pose.data() + 7 * p);
        std::memcpy(cur_poses + 7 * p, pose.data() + 7 * p, 56);
    }
    blk.put(d_sc, scale.data());
    blk.put(d_cp, pose.data());
    blk.launch([&] { svo::launch_two_view_finish(a, s); });
    blk.finish();
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_two_view_init: %s", hipGetErrorString(blk.err));
    if (depth)
        for (size_t p = 0; p < P; ++p)  // a failed pair has no depths
            for (int64_t k = feat_off[p]; k < feat_off[p + 1]; ++k) depth[k] = winner[p] < 0 ? 0.0 : dep[k];
    return SVO_OK;
}

int svo_essential_score(svo_ctx* c, const svo_camera* cam, int32_t n_pairs, const int32_t* feat_off,
                        const int32_t* hyp_off, const double* E_hyp, const double* ref_px, const double* cur_px,
                        double threshold, int32_t* counts, uint8_t* mask) {
    if (int r = essential_scalars("svo_essential_score", threshold)) return r;
    int64_t n = 0, m = 0;
    if (int r = check_pair_offsets("svo_essential_score", n_pairs, feat_off, &n)) return r;
    if (int r = check_pair_offsets("svo_essential_score (hyp_off)", n_pairs, hyp_off, &m)) return r;
    if (!c || !cam || (n > 0 && (!ref_px || !cur_px)) || (m > 0 && (!E_hyp || !counts)))
        return fail(SVO_ERR_ARG, "svo_essential_score: null argument");
    if (mask && n > 0) std::memset(mask, 0, (size_t)n);
    if (n_pairs == 0 || m == 0) return SVO_OK;
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    const size_t P = (size_t)n_pairs, N = (size_t)n, M = (size_t)m;
    svo::EssentialArgs a{};
    Block blk(c, s);
    blk.in(&a.feat_off, feat_off, P + 1);
    blk.in(&a.hyp_off, hyp_off, P + 1);
    blk.in(&a.ref_px, ref_px, N * 2);
    blk.in(&a.cur_px, cur_px, N * 2);
    blk.dev(&a.xn, N * 4);
    blk.in(&a.hyp_E, E_hyp, M * 9);
    const auto d_cnt = blk.dev(&a.counts, M);  // counts .. mask travel one by one (below)
    const auto d_best = blk.dev(&a.best_E, P * 9);
    const auto d_has = blk.dev(&a.has_best, P);
    const auto d_mask = blk.dev(&a.mask, N);
    essential_camera(a, cam, threshold);
    a.n = (int32_t)n; a.n_pairs = n_pairs; a.n_models = (int32_t)m;
    if (blk.alloc() != hipSuccess) return fail(SVO_ERR_HIP, "svo_essential_score scratch: %s", hipGetErrorString(blk.err));
    blk.upload();
    blk.launch([&] {
        svo::launch_essential_normalise(a, s);
        svo::launch_essential_score_models(a, s);
    });
    blk.get(counts, d_cnt);
    blk.sync();
    if (blk.ok() && mask && n > 0) {  // per pair: its first model with the strictly largest count
        std::vector<double> best(P * 9, 0.0);
        std::vector<int32_t> has(P, 0);
        for (int32_t p = 0; p < n_pairs; ++p) {
            int32_t top = 0;
            for (int32_t k = hyp_off[p]; k < hyp_off[p + 1]; ++k)
                if (counts[k] > top) {
                    top = counts[k];
                    has[p] = 1;
                    std::memcpy(&best[(size_t)p * 9], E_hyp + (size_t)k * 9, 72);
                }
        }
        blk.put(d_best, best.data());
        blk.put(d_has, has.data());
        blk.launch([&] { svo::launch_essential_mask(a, s); });
        blk.get(mask, d_mask);
        blk.sync();  // (also keeps `best` and `has` alive for the copies)
    }
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_essential_score: %s", hipGetErrorString(blk.err));
    return SVO_OK;
}

int svo_essential_ransac(svo_ctx* c, const svo_camera* cam, int32_t n_pairs, const int32_t* feat_off,
                         const double* ref_px, const double* cur_px, double threshold, double confidence,
                         int32_t max_iterations, uint64_t seed, double* E, uint8_t* mask, int32_t* n_inliers,
                         int32_t* iterations, int32_t* best, int32_t* status, double* hyp_E, int32_t* hyp_count) {
    // the scalar parameters and the layout first: these need no context
    if (int r = essential_scalars("svo_essential_ransac", threshold)) return r;
    if (!(confidence > 0.0 && confidence < 1.0)) return fail(SVO_ERR_ARG, "svo_essential_ransac: confidence must lie in (0, 1)");
    if (max_iterations < 1 || max_iterations > SVO_ESSENTIAL_MAX_ITERATIONS)
        return fail(SVO_ERR_ARG, "svo_essential_ransac: max_iterations %d outside 1..%d", max_iterations, SVO_ESSENTIAL_MAX_ITERATIONS);
    int64_t n = 0;
    if (int r = check_pair_offsets("svo_essential_ransac", n_pairs, feat_off, &n)) return r;
    if (n_pairs > 65535) return fail(SVO_ERR_ARG, "svo_essential_ransac: more than 65535 pairs in one call");
    if (!c || !cam || (n_pairs > 0 && (!E || !n_inliers || !iterations || !best || !status)) ||
        (n > 0 && (!ref_px || !cur_px || !mask)) || ((hyp_E != nullptr) != (hyp_count != nullptr)))
        return fail(SVO_ERR_ARG, "svo_essential_ransac: null argument");
    if (n_pairs == 0) return SVO_OK;
    const size_t P = (size_t)n_pairs, N = (size_t)n, MI = (size_t)max_iterations;
    const bool trace = hyp_E != nullptr;
    std::fill(E, E + P * 9, 0.0);
    if (n > 0) std::memset(mask, 0, N);
    std::fill(best, best + 2 * P, -1);
    if (trace) {
        std::fill(hyp_E, hyp_E + P * MI * 90, 0.0);
        std::fill(hyp_count, hyp_count + P * MI * 10, -2);
    }
    std::vector<int32_t> active(P), niters(P, max_iterations), top(P, 0), select(P), has(P, 0);
    bool any = false;
    for (size_t p = 0; p < P; ++p) {
        const int32_t np = feat_off[p + 1] - feat_off[p];
        active[p] = np >= 5;
        any = any || active[p];
        n_inliers[p] = 0;
        iterations[p] = 0;
        status[p] = -1;
    }
    if (!any) return SVO_OK;
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    // samples per round: the rounds only bound the work past the stop, the result does not depend on them
    const int32_t chunk = std::min<int32_t>((max_iterations + 63) / 64 * 64, n_pairs >= 64 ? 64 : 256);
    const size_t CH = (size_t)chunk;
    svo::EssentialArgs a{};
    Block blk(c, s);
    blk.in(&a.feat_off, feat_off, P + 1);
    blk.in(&a.ref_px, ref_px, N * 2);
    blk.in(&a.cur_px, cur_px, N * 2);
    blk.dev(&a.xn, N * 4);
    const auto d_act = blk.dev(&a.active, P);  // active .. mask travel one by one, round by round (below)
    blk.dev(&a.nsol, P * CH);
    const auto d_E = blk.dev(&a.hyp_E, P * CH * 90);
    const auto d_cnt = blk.dev(&a.counts, P * CH * 10);
    const auto d_sel = blk.dev(&a.select, P);
    const auto d_best = blk.dev(&a.best_E, P * 9);
    const auto d_has = blk.dev(&a.has_best, P);
    const auto d_mask = blk.dev(&a.mask, N);
    essential_camera(a, cam, threshold);
    a.seed = seed;
    a.n = (int32_t)n; a.n_pairs = n_pairs; a.chunk = chunk; a.max_iterations = max_iterations;
    if (blk.alloc() != hipSuccess) return fail(SVO_ERR_HIP, "svo_essential_ransac scratch: %s", hipGetErrorString(blk.err));
    blk.upload();
    blk.zero(d_best);
    blk.launch([&] { svo::launch_essential_normalise(a, s); });
    std::vector<int32_t> cnt(P * CH * 10);
    std::vector<double> round_E(trace ? P * CH * 90 : 0);
    for (int32_t h0 = 0; any && blk.ok(); h0 += chunk) {
        a.h0 = h0;
        blk.put(d_act, active.data());
        blk.launch([&] {
            svo::launch_essential_solve(a, s);
            svo::launch_essential_score_samples(a, s);
        });
        blk.get(cnt.data(), d_cnt);
        if (trace) blk.get(round_E.data(), d_E);
        blk.sync();
        if (!blk.ok()) break;
        // the sequential stopping rule on this round's counts
        any = false;
        bool rose_any = false;
        for (size_t p = 0; p < P; ++p) {
            select[p] = -1;
            if (!active[p]) continue;
            const int32_t np = feat_off[p + 1] - feat_off[p];
            int32_t h = h0;
            for (; h < h0 + chunk && h < niters[p]; ++h) {
                const size_t slot = p * CH + (size_t)(h - h0);
                bool rose = false;
                for (int k = 0; k < 10; ++k) {
                    const int32_t v = cnt[slot * 10 + k];
                    if (trace) hyp_count[(p * MI + (size_t)h) * 10 + k] = v;
                    if (v > top[p]) {
                        top[p] = v;
                        best[2 * p] = h;
                        best[2 * p + 1] = k;
                        select[p] = (int32_t)(slot * 10 + k);
                        rose = true;
                    }
                }
                if (trace) std::memcpy(hyp_E + (p * MI + (size_t)h) * 90, &round_E[slot * 90], 720);
                if (rose)
                    niters[p] = svo::essential_update_iterations(confidence, (double)(np - top[p]) / (double)np, max_iterations);
            }
            if (h >= niters[p]) {
                active[p] = 0;
                iterations[p] = h;
            } else {
                any = true;
            }
            rose_any = rose_any || select[p] >= 0;
        }
        if (rose_any) {
            blk.put(d_sel, select.data());
            blk.launch([&] { svo::launch_essential_gather(a, s); });
            blk.sync();  // `select` is rewritten by the next round
        }
    }
    for (size_t p = 0; p < P; ++p) {
        has[p] = top[p] > 0;
        status[p] = has[p] ? 0 : -1;
        n_inliers[p] = top[p];
    }
    blk.put(d_has, has.data());
    if (n > 0) blk.launch([&] { svo::launch_essential_mask(a, s); });
    blk.get(E, d_best);
    blk.get(mask, d_mask);
    blk.sync();
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_essential_ransac: %s", hipGetErrorString(blk.err));
    return SVO_OK;
}
}  // extern "C"
