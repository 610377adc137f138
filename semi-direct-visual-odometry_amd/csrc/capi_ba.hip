// capi_ba.hip — C ABI: bundle adjustment, pose-only per frame (pose_ba.hip) and windowed (bundle_adjust.hip).
#include <algorithm>
#include <cmath>

#include "capi_ctx.h"
using namespace svo::shim;

extern "C" {
int svo_pose_optimize(svo_ctx* c, int32_t n_frames, const int32_t* feat_off, const double* bearing, const double* point,
                      const uint8_t* has_point, uint8_t* vis_inout, double* poses_inout, double* err, int32_t* status) {
    if (!c || (n_frames > 0 && (!feat_off || !poses_inout || !err || !status))) return fail(SVO_ERR_ARG, "null argument");
    if (n_frames < 0) return fail(SVO_ERR_ARG, "n_frames < 0");
    if (n_frames == 0) return SVO_OK;
    if (int r = check_offsets(nullptr, "feat_off", "frame", n_frames, feat_off, 0, nullptr)) return r;
    const int64_t nf = feat_off[n_frames];
    if (nf > 0 && (!bearing || !point || !has_point || !vis_inout)) return fail(SVO_ERR_ARG, "null argument");
    if (nf >= ((int64_t)1 << 28)) return fail(SVO_ERR_ARG, "too many features");
    for (int64_t k = 0; k < nf; ++k)
        if (vis_inout[k] && !has_point[k])
            return fail(SVO_ERR_ARG, "feature %lld: visible from the previous call but without a point "
                                     "(the reference dereferences a null m_point)", (long long)k);
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    // one block, same layout on both sides: inputs, then outputs, then device-only scratch; one H2D copy of the inputs
    // and one D2H copy of the outputs through the context's pinned staging (past its size: one copy per piece)
    const size_t F = (size_t)n_frames, N = (size_t)nf;
    svo::PoseBAArgs a{};
    Block blk(c, s);
    blk.in(&a.feat_off, feat_off, F + 1);
    blk.in(&a.poses, poses_inout, F * 7);
    blk.in(&a.bearing, bearing, N * 3);
    blk.in(&a.point, point, N * 3);
    blk.in(&a.has_point, has_point, N);
    blk.in(&a.vis_in, vis_inout, N);
    blk.out(&a.poses_out, poses_inout, F * 7);
    blk.out(&a.err, err, F);
    blk.out(&a.status, status, F);
    blk.out(&a.vis_out, vis_inout, N);
    blk.dev(&a.rows, N * 3);
    blk.dev(&a.wts, N);
    a.n_frames = n_frames;
    if (blk.alloc(Block::kDirect) == hipSuccess) blk.run([&] { svo::launch_pose_ba(a, s); });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_pose_optimize: %s", hipGetErrorString(blk.err));
    return SVO_OK;
}

int svo_bundle_adjust(svo_ctx* c, const svo_camera* cam, int32_t n_problems, const int32_t* frame_off,
                      const int32_t* point_off, const int32_t* obs_off, double* poses_inout,
                      const uint8_t* frame_fixed, double* points_inout, const int32_t* obs_frame,
                      const int32_t* obs_point, const double* obs_px, double huber_delta, int32_t max_iterations,
                      int32_t structure_iterations, double* obs_chi2, double* init_chi, double* final_chi,
                      int32_t* iterations, int32_t* status, double* trace) {
    if (n_problems < 0) return fail(SVO_ERR_ARG, "svo_bundle_adjust: n_problems < 0");
    // (cap 2^24: the structure kernel's grid spans max points / 256 in y, at most 65535)
    auto table = [&](const char* name, const int32_t* off) {
        return check_offsets("svo_bundle_adjust", name, "problem", n_problems, off, 24, nullptr);
    };
    if (int r = table("frame_off", frame_off)) return r;
    if (int r = table("point_off", point_off)) return r;
    if (int r = table("obs_off", obs_off)) return r;
    if (max_iterations < 0 || structure_iterations < 0)
        return fail(SVO_ERR_ARG, "svo_bundle_adjust: negative iteration count");
    if (!(huber_delta > 0.0) || !std::isfinite(huber_delta))
        return fail(SVO_ERR_ARG, "svo_bundle_adjust: huber_delta must be positive and finite");
    const size_t NP = (size_t)n_problems, NF = (size_t)frame_off[n_problems], NX = (size_t)point_off[n_problems],
                 NO = (size_t)obs_off[n_problems];
    if ((NP > 0 && (!init_chi || !final_chi || !iterations || !status)) ||
        (NF > 0 && (!poses_inout || !frame_fixed)) || (NX > 0 && !points_inout) ||
        (NO > 0 && (!obs_frame || !obs_point || !obs_px || !obs_chi2)))
        return fail(SVO_ERR_ARG, "svo_bundle_adjust: null argument");
    // layout: every point's observation block, checked before anything reaches the device
    std::vector<int32_t> pobs(NX + 1, 0);
    std::vector<int64_t> tab_off(NP + 1, 0);
    std::vector<int32_t> ridx(NF, -1), seen;
    int32_t max_points = 0;
    for (size_t p = 0; p < NP; ++p) {
        const int32_t F = frame_off[p + 1] - frame_off[p], P = point_off[p + 1] - point_off[p];
        int32_t nfree = 0;  // only the free frames enter the reduced system, which lives in LDS
        for (int32_t i = 0; i < F; ++i)
            if (!frame_fixed[frame_off[p] + i]) ridx[(size_t)frame_off[p] + i] = nfree++;
        if (nfree > SVO_BA_MAX_FRAMES)
            return fail(SVO_ERR_ARG, "svo_bundle_adjust: problem %zu has %d frames free to move (at most %d; fixed "
                                     "frames do not count)", p, nfree, SVO_BA_MAX_FRAMES);
        seen.assign((size_t)F, -1);  // the last point seen in each frame
        tab_off[p + 1] = tab_off[p] + (int64_t)F * P;
        max_points = std::max(max_points, P);
        int32_t o = obs_off[p];
        for (int32_t j = 0; j < P; ++j) {
            pobs[(size_t)point_off[p] + j] = o;
            while (o < obs_off[p + 1] && obs_point[o] == j) {
                const int32_t i = obs_frame[o];
                if (i < 0 || i >= F) return fail(SVO_ERR_ARG, "svo_bundle_adjust: observation %d: frame index out of range", o);
                if (seen[(size_t)i] == j)
                    return fail(SVO_ERR_ARG, "svo_bundle_adjust: observation %d: duplicate (frame, point)", o);
                seen[(size_t)i] = j;
                ++o;
            }
            if (o - pobs[(size_t)point_off[p] + j] < 2)
                return fail(SVO_ERR_ARG, "svo_bundle_adjust: problem %zu point %d has fewer than two observations "
                                         "(observations must be grouped by ascending point)", p, j);
        }
        if (o != obs_off[p + 1])
            return fail(SVO_ERR_ARG, "svo_bundle_adjust: observation %d: point index out of range or observations not "
                                     "grouped by ascending point", o);
    }
    pobs[NX] = (int32_t)NO;
    if (!c || !cam) return fail(SVO_ERR_ARG, "svo_bundle_adjust: null argument (ctx / cam)");
    if (NP == 0) return SVO_OK;
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    // (pobs, tab_off and ridx outlive their copies: run() below waits for the stream)
    svo::BundleAdjustArgs a{};
    Block blk(c, s);
    blk.in(&a.frame_off, frame_off, NP + 1);
    blk.in(&a.point_off, point_off, NP + 1);
    blk.in(&a.obs_off, obs_off, NP + 1);
    blk.in(&a.pobs_off, pobs.data(), NX + 1);
    blk.in(&a.tab_off, tab_off.data(), NP + 1);
    blk.inout(&a.poses, poses_inout, NF * 7);
    blk.in(&a.ridx, ridx.data(), NF);
    blk.inout(&a.points, points_inout, NX * 3);
    blk.in(&a.obs_frame, obs_frame, NO);
    blk.in(&a.obs_px, obs_px, NO * 2);
    blk.dev(&a.tab, (size_t)tab_off[NP]);
    blk.dev(&a.edge, NO * 15);
    blk.dev(&a.W, NO * 18);
    blk.dev(&a.Vg, NX * 9);
    blk.dev(&a.Vi, NX * 6);
    blk.dev(&a.dx, NX * 3);
    blk.dev(&a.Xt, NX * 3);
    blk.out(&a.obs_chi2, obs_chi2, NO);
    blk.out(&a.init_chi, init_chi, NP);
    blk.out(&a.final_chi, final_chi, NP);
    blk.out(&a.iterations, iterations, NP);
    blk.out(&a.status, status, NP);
    blk.out(&a.trace, trace, trace ? NP * SVO_BA_TRACE_CAP * 6 : 0);
    if (blk.alloc() != hipSuccess) return fail(SVO_ERR_HIP, "bundle-adjust scratch: %s", hipGetErrorString(blk.err));
    if (!trace) a.trace = nullptr;
    a.f = cam->fx; a.cx = cam->cx; a.cy = cam->cy;  // fx on both axes (src/bundle_adjustment.cpp:333)
    a.delta = huber_delta; a.max_iterations = max_iterations; a.structure_iterations = structure_iterations;
    a.n_problems = n_problems; a.max_points = max_points;
    blk.run([&] {
        svo::launch_ba_structure(a, s);
        svo::launch_ba_joint(a, s);
    });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_bundle_adjust: %s", hipGetErrorString(blk.err));
    return SVO_OK;
}
}  // extern "C"
