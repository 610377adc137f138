// essential.hip — essential-matrix RANSAC over a batch of frame pairs (svo_essential_ransac, svo_essential_score; the
// contract is stated in include/svo_c.h and modelled on cv::findEssentialMat as algorithm::computeEssentialMatrix
// calls it, src/algorithm.cpp:124-125).  The arithmetic is in essential_math.h.
//
// solve   one lane per minimal sample, one wave64 per block.  The 10 x 20 elimination, the polynomial work and the root
//         iteration index their arrays by run-time values; those arrays live in LDS, element e of lane l at
//         lds[64 e + l] (a lane's accesses never meet another lane's bank), 240 doubles per lane = 120 KB per block.
//         What is left in registers is indexed by unrolled loop counters: no private segment.
// score   one wave64 per model, four per block: the lanes stride over the pair's normalised matches (computed once by
//         the normalise kernel and read through L2), inliers are counted by ballot + popcount, so a count is an
//         integer sum that no order can change.
// gather / mask   the winner of every pair is kept on the device; the mask is the Sampson test of that model.
#include "svo_internal.h"
#include "essential_math.h"
#include <algorithm>
#include <cfloat>
#include <cmath>

namespace svo {

namespace {

constexpr int kScoreWaves = 4;

struct LdsStore {  // element i of this lane's slice
    double* base;
    __device__ __forceinline__ double& operator()(int i) const { return base[64 * i]; }
};

// the pair that owns item i of a prefix array: off[p] <= i < off[p + 1]
__device__ __forceinline__ int owner(const int32_t* off, int n_pairs, int i) {
    int lo = 0, hi = n_pairs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= i) lo = mid; else hi = mid;
    }
    return lo;
}

__global__ void __launch_bounds__(256) essential_normalise_kernel(EssentialArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    a.xn[4 * i] = ess_normalise(a.ref_px[2 * i], a.cx, a.fx);
    a.xn[4 * i + 1] = ess_normalise(a.ref_px[2 * i + 1], a.cy, a.fy);
    a.xn[4 * i + 2] = ess_normalise(a.cur_px[2 * i], a.cx, a.fx);
    a.xn[4 * i + 3] = ess_normalise(a.cur_px[2 * i + 1], a.cy, a.fy);
}

__global__ void __launch_bounds__(64) essential_solve_kernel(EssentialArgs a) {
    __shared__ double lds[kEssStore * 64];
    const int p = blockIdx.y, hl = blockIdx.x * 64 + threadIdx.x;
    if (hl >= a.chunk || (a.active && !a.active[p])) return;  // no barrier below: lanes may leave
    const int h = a.h0 + hl;
    const int64_t slot = (int64_t)p * a.chunk + hl;
    double* out = a.hyp_E + slot * (kEssMaxModels * 9);
    const int first = a.feat_off[p], n = a.feat_off[p + 1] - first;
    int idx[5];
    if (h >= a.max_iterations || n < 5 || !ess_sample(a.seed, (uint32_t)p, (uint32_t)h, (uint32_t)n, idx)) {
        for (int i = 0; i < kEssMaxModels * 9; ++i) out[i] = 0.0;
        a.nsol[slot] = -1;
        return;
    }
    double x1[5][2], x2[5][2];
#pragma unroll
    for (int k = 0; k < 5; ++k) {
        const double* m = a.xn + 4 * (int64_t)(first + idx[k]);
        x1[k][0] = m[0];
        x1[k][1] = m[1];
        x2[k][0] = m[2];
        x2[k][1] = m[3];
    }
    const LdsStore s{lds + threadIdx.x};
    a.nsol[slot] = ess_five_point(x1, x2, s, out);
}

// the inliers of model E among the matches first .. first + n - 1, counted by the whole wave
__device__ __forceinline__ int wave_count(const double* E, const double* xn, int first, int n, double thr2, int lane) {
    double e[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) e[i] = E[i];
    int count = 0;
    for (int base = 0; base < n; base += 64) {
        const int i = base + lane;
        bool in = false;
        if (i < n) {
            const double* m = xn + 4 * (int64_t)(first + i);
            in = ess_inlier(e, m[0], m[1], m[2], m[3], thr2);
        }
        count += __popcll(__ballot(in));
    }
    return count;
}

__global__ void __launch_bounds__(64 * kScoreWaves) essential_score_samples_kernel(EssentialArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t m = (int64_t)blockIdx.x * kScoreWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t per_pair = (int64_t)a.chunk * kEssMaxModels;
    if (m >= per_pair * a.n_pairs) return;  // whole waves leave
    const int p = (int)(m / per_pair);
    if (a.active && !a.active[p]) return;
    const int64_t slot = m / kEssMaxModels;
    const int k = (int)(m - slot * kEssMaxModels);
    int count = -1;
    if (k < a.nsol[slot]) {
        const int first = a.feat_off[p];
        count = wave_count(a.hyp_E + m * 9, a.xn, first, a.feat_off[p + 1] - first, a.thr2, lane);
    }
    if (lane == 0) a.counts[m] = count;
}

__global__ void __launch_bounds__(64 * kScoreWaves) essential_score_models_kernel(EssentialArgs a) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * kScoreWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (m >= a.n_models) return;
    const int p = owner(a.hyp_off, a.n_pairs, m);
    const int first = a.feat_off[p];
    const int count = wave_count(a.hyp_E + (int64_t)m * 9, a.xn, first, a.feat_off[p + 1] - first, a.thr2, lane);
    if (lane == 0) a.counts[m] = count;
}

__global__ void __launch_bounds__(256) essential_gather_kernel(EssentialArgs a) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= a.n_pairs * 9) return;
    const int p = t / 9, j = t - 9 * p;
    const int src = a.select[p];
    if (src >= 0) a.best_E[t] = a.hyp_E[(int64_t)src * 9 + j];
}

__global__ void __launch_bounds__(256) essential_mask_kernel(EssentialArgs a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const int p = owner(a.feat_off, a.n_pairs, i);
    bool in = false;
    if (a.has_best[p]) {
        const double* m = a.xn + 4 * (int64_t)i;
        in = ess_inlier(a.best_E + 9 * p, m[0], m[1], m[2], m[3], a.thr2);
    }
    a.mask[i] = in ? 1 : 0;
}

}  // namespace

void launch_essential_normalise(const EssentialArgs& a, hipStream_t s) {
    if (a.n > 0) hipLaunchKernelGGL(essential_normalise_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}
void launch_essential_solve(const EssentialArgs& a, hipStream_t s) {
    if (a.n_pairs > 0 && a.chunk > 0)
        hipLaunchKernelGGL(essential_solve_kernel, dim3((a.chunk + 63) / 64, a.n_pairs), dim3(64), 0, s, a);
}
void launch_essential_score_samples(const EssentialArgs& a, hipStream_t s) {
    const int64_t models = (int64_t)a.n_pairs * a.chunk * kEssMaxModels;
    if (models > 0)
        hipLaunchKernelGGL(essential_score_samples_kernel, dim3((uint32_t)((models + kScoreWaves - 1) / kScoreWaves)),
                           dim3(64 * kScoreWaves), 0, s, a);
}
void launch_essential_score_models(const EssentialArgs& a, hipStream_t s) {
    if (a.n_models > 0)
        hipLaunchKernelGGL(essential_score_models_kernel, dim3((a.n_models + kScoreWaves - 1) / kScoreWaves),
                           dim3(64 * kScoreWaves), 0, s, a);
}
void launch_essential_gather(const EssentialArgs& a, hipStream_t s) {
    if (a.n_pairs > 0) hipLaunchKernelGGL(essential_gather_kernel, dim3((a.n_pairs * 9 + 255) / 256), dim3(256), 0, s, a);
}
void launch_essential_mask(const EssentialArgs& a, hipStream_t s) {
    if (a.n > 0) hipLaunchKernelGGL(essential_mask_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
}

int essential_update_iterations(double confidence, double ep, int max_iterations) {
    const double num = std::max(1.0 - confidence, DBL_MIN);
    const double den = 1.0 - std::pow(1.0 - ep, 5);
    if (den < DBL_MIN) return 0;
    const double ln = std::log(num), ld = std::log(den);
    if (ld >= 0.0 || -ln >= (double)max_iterations * (-ld)) return max_iterations;
    return (int)std::rint(ln / ld);
}

}  // namespace svo
