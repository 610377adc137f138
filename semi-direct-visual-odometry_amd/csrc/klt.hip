// klt.hip — pyramidal Lucas-Kanade tracking of a batch of points (svo_klt_track; the contract is stated in
// include/svo_c.h and modelled on cv::calcOpticalFlowPyrLK as algorithm::computeOpticalFlowSparse calls it,
// src/algorithm.cpp:60-62).
//
// One 64-lane wave per point, four waves per block, no LDS and no barriers.  The win^2 window maps onto the lanes,
// pixel k = lane + 64 r for r < NREG = ceil(win^2 / 64) (7 at win 21): the template T and both gradients gx, gy of
// a level stay in 3 NREG registers per lane, and in every iteration each lane samples its own pixels of the current
// image.  The Scharr derivatives are formed on the fly from the 4x4 u8 neighbourhood of a pixel (once per level and
// pixel).  All sums are 64-bit integer sums (DPP reduction over the wave: every lane ends up with the total), so their
// order does not matter; the fp64 step that follows is computed by every lane from the same totals, which keeps the
// level / iteration control flow wave-uniform (the point index is an SGPR: scalar branches).
#include "svo_internal.h"
#include "svo_wave.h"

namespace svo {

namespace {

constexpr int kWavesPerBlock = 4;
constexpr double kScale20 = 9.5367431640625e-07;     // 2^-20
constexpr double kFltEpsilon = 1.1920928955078125e-07;  // FLT_EPSILON

template <int kCtrl>
__device__ __forceinline__ int64_t dpp_mov64(int64_t v) {
    const uint2 u = __builtin_bit_cast(uint2, v);
    return __builtin_bit_cast(int64_t, make_uint2(dpp_mov<kCtrl>(u.x), dpp_mov<kCtrl>(u.y)));
}
__device__ __forceinline__ int64_t lane_read64(int64_t v, int l) {
    const uint2 u = __builtin_bit_cast(uint2, v);
    return __builtin_bit_cast(int64_t, make_uint2(lane_read(u.x, l), lane_read(u.y, l)));
}
// sum over the wave's 64 lanes (all active), the same total in every lane
__device__ __forceinline__ int64_t wave_sum_i64(int64_t v) {
    v += dpp_mov64<0xB1>(v);   // quad_perm [1,0,3,2]
    v += dpp_mov64<0x4E>(v);   // quad_perm [2,3,0,1]
    v += dpp_mov64<0x141>(v);  // row_half_mirror
    v += dpp_mov64<0x140>(v);  // row_mirror
    return (lane_read64(v, 0) + lane_read64(v, 16)) + (lane_read64(v, 32) + lane_read64(v, 48));
}

// BORDER_REFLECT_101, one reflection per side, then clamped (always a valid index)
__device__ __forceinline__ int refl101(int i, int n) {
    i = i < 0 ? -i : i;
    i = i >= n ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

__device__ __forceinline__ int descale(int v, int k) { return (v + (1 << (k - 1))) >> k; }

struct Weights {
    int w00, w01, w10, w11;
};
__device__ __forceinline__ Weights make_weights(double a, double b) {
    Weights w;
    w.w00 = (int)rint((1.0 - a) * (1.0 - b) * 16384.0);
    w.w01 = (int)rint(a * (1.0 - b) * 16384.0);
    w.w10 = (int)rint((1.0 - a) * b * 16384.0);
    w.w11 = 16384 - w.w00 - w.w01 - w.w10;
    return w;
}

// the window's corner floor(p) is in range: -win <= ip.x < W and -win <= ip.y < H (false for a NaN)
__device__ __forceinline__ bool corner_in_range(double fx, double fy, int win, int W, int H) {
    return fx >= (double)-win && fx < (double)W && fy >= (double)-win && fy < (double)H;
}

}  // namespace

template <int NREG>
__global__ void __launch_bounds__(64 * kWavesPerBlock) klt_kernel(KltArgs a) {
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (i >= a.n) return;  // whole waves leave; nothing below synchronises across waves

    // the pair that owns point i: feat_off[lo] <= i < feat_off[hi]
    int lo = 0, hi = a.n_pairs;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (a.feat_off[mid] <= i) lo = mid; else hi = mid;
    }
    const uint8_t* ref_pyr = a.ref_base + (int64_t)a.frames[2 * lo] * a.ref_stride;
    const uint8_t* cur_pyr = a.cur_base + (int64_t)a.frames[2 * lo + 1] * a.cur_stride;

    const int win = a.win, h = (win - 1) / 2, area = win * win;
    const double hd = (double)h;
    int kx[NREG], ky[NREG];
    bool kin[NREG];
#pragma unroll
    for (int r = 0; r < NREG; ++r) {
        const int k = lane + 64 * r;
        kin[r] = k < area;
        const int kk = kin[r] ? k : 0;
        ky[r] = kk / win;
        kx[r] = kk - ky[r] * win;
    }

    // step 1: float32 rounding of both positions
    const double rx = (double)(float)a.ref_px[2 * i], ry = (double)(float)a.ref_px[2 * i + 1];
    double fx = (double)(float)a.cur_px[2 * i], fy = (double)(float)a.cur_px[2 * i + 1];

    // step 2: the coarsest level larger than the window
    int L = a.max_level;
    while (L > 0 && !(a.geom.w[L] > win && a.geom.h[L] > win)) --L;
    int32_t* tr = a.trace ? a.trace + (int64_t)i * (a.max_level + 1) * 2 : nullptr;
    if (tr && lane == 0)
        for (int l = a.max_level; l > L; --l) { tr[2 * l] = 0; tr[2 * l + 1] = 0; }
    const double inv0 = 1.0 / (double)(1 << L);
    fx *= inv0;
    fy *= inv0;
    int st = 1;

    for (int l = L; l >= 0; --l) {
        if (l != L) { fx *= 2.0; fy *= 2.0; }
        const int W = a.geom.w[l], H = a.geom.h[l];
        const uint8_t* I = ref_pyr + a.geom.off[l];
        const uint8_t* J = cur_pyr + a.geom.off[l];
        const double inv = 1.0 / (double)(1 << l);
        int iters = 0, code = 0;

        // step 3: template and gradients
        const double px = rx * inv - hd, py = ry * inv - hd;
        const double fpx = floor(px), fpy = floor(py);
        int T[NREG], gx[NREG], gy[NREG];
        double A11 = 0.0, A12 = 0.0, A22 = 0.0, D = 0.0;
        if (!corner_in_range(fpx, fpy, win, W, H)) {
            code = 5;
        } else {
            const int ipx = (int)fpx, ipy = (int)fpy;
            const Weights w = make_weights(px - fpx, py - fpy);
            int64_t s11 = 0, s12 = 0, s22 = 0;
#pragma unroll
            for (int r = 0; r < NREG; ++r) {
                const int X = ipx + kx[r], Y = ipy + ky[r];
                int V[4][4];
                int cx[4], ro[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    cx[t] = refl101(X - 1 + t, W);
                    ro[t] = refl101(Y - 1 + t, H) * W;
                }
#pragma unroll
                for (int v = 0; v < 4; ++v)
#pragma unroll
                    for (int u = 0; u < 4; ++u) V[v][u] = I[ro[v] + cx[u]];
                T[r] = descale(w.w00 * V[1][1] + w.w01 * V[1][2] + w.w10 * V[2][1] + w.w11 * V[2][2], 9);
                int dx[2][2], dy[2][2];
#pragma unroll
                for (int v = 0; v < 2; ++v)
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int cy = 1 + v, cc = 1 + u;
                        const bool in = X + u >= 0 && X + u < W && Y + v >= 0 && Y + v < H;
                        const int sx = 3 * (V[cy - 1][cc + 1] - V[cy - 1][cc - 1]) + 10 * (V[cy][cc + 1] - V[cy][cc - 1]) +
                                       3 * (V[cy + 1][cc + 1] - V[cy + 1][cc - 1]);
                        const int sy = 3 * (V[cy + 1][cc - 1] - V[cy - 1][cc - 1]) + 10 * (V[cy + 1][cc] - V[cy - 1][cc]) +
                                       3 * (V[cy + 1][cc + 1] - V[cy - 1][cc + 1]);
                        dx[v][u] = in ? sx : 0;
                        dy[v][u] = in ? sy : 0;
                    }
                const int g1 = descale(w.w00 * dx[0][0] + w.w01 * dx[0][1] + w.w10 * dx[1][0] + w.w11 * dx[1][1], 14);
                const int g2 = descale(w.w00 * dy[0][0] + w.w01 * dy[0][1] + w.w10 * dy[1][0] + w.w11 * dy[1][1], 14);
                gx[r] = kin[r] ? g1 : 0;
                gy[r] = kin[r] ? g2 : 0;
                s11 += (int64_t)gx[r] * gx[r];
                s12 += (int64_t)gx[r] * gy[r];
                s22 += (int64_t)gy[r] * gy[r];
            }
            // step 4
            A11 = (double)wave_sum_i64(s11) * kScale20;
            A12 = (double)wave_sum_i64(s12) * kScale20;
            A22 = (double)wave_sum_i64(s22) * kScale20;
            D = A11 * A22 - A12 * A12;
            const double df = A11 - A22;
            const double min_eig = (A22 + A11 - sqrt(df * df + 4.0 * A12 * A12)) / (double)(2 * win * win);
            if (min_eig < a.min_eig || D < kFltEpsilon) code = 6;
        }

        if (code == 0) {
            // step 5
            const double invD = 1.0 / D;
            double qx = fx - hd, qy = fy - hd, pdx = 0.0, pdy = 0.0;
            code = 3;
            for (int j = 0; j < a.max_iterations; ++j) {
                const double fqx = floor(qx), fqy = floor(qy);
                if (!corner_in_range(fqx, fqy, win, W, H)) {
                    code = 4;
                    break;
                }
                const int iqx = (int)fqx, iqy = (int)fqy;
                const Weights w = make_weights(qx - fqx, qy - fqy);
                int64_t s1 = 0, s2 = 0;
#pragma unroll
                for (int r = 0; r < NREG; ++r) {
                    const int X = iqx + kx[r], Y = iqy + ky[r];
                    const int c0 = refl101(X, W), c1 = refl101(X + 1, W);
                    const int r0 = refl101(Y, H) * W, r1 = refl101(Y + 1, H) * W;
                    const int d = descale(w.w00 * J[r0 + c0] + w.w01 * J[r0 + c1] + w.w10 * J[r1 + c0] + w.w11 * J[r1 + c1], 9) - T[r];
                    s1 += (int64_t)d * gx[r];
                    s2 += (int64_t)d * gy[r];
                }
                const double b1 = (double)wave_sum_i64(s1) * kScale20, b2 = (double)wave_sum_i64(s2) * kScale20;
                const double ddx = (A12 * b2 - A22 * b1) * invD, ddy = (A12 * b1 - A11 * b2) * invD;
                qx += ddx;
                qy += ddy;
                iters = j + 1;
                if (ddx * ddx + ddy * ddy <= a.epsilon * a.epsilon) {
                    code = 1;
                    break;
                }
                if (j > 0 && fabs(ddx + pdx) < 0.01 && fabs(ddy + pdy) < 0.01) {
                    qx -= ddx * 0.5;
                    qy -= ddy * 0.5;
                    code = 2;
                    break;
                }
                pdx = ddx;
                pdy = ddy;
            }
            fx = qx + hd;
            fy = qy + hd;
            if (code == 4 && l == 0) st = 0;
        } else if (l == 0) {
            st = 0;
        }
        if (tr && lane == 0) { tr[2 * l] = iters; tr[2 * l + 1] = code; }
    }

    // step 6
    if (lane == 0) {
        a.cur_px[2 * i] = (double)(float)fx;
        a.cur_px[2 * i + 1] = (double)(float)fy;
        a.status[i] = (uint8_t)st;
    }
}

void launch_klt(const KltArgs& a, hipStream_t s) {
    const int blocks = (a.n + kWavesPerBlock - 1) / kWavesPerBlock;
    if (blocks <= 0) return;
    const dim3 g(blocks), b(64 * kWavesPerBlock);
    switch ((a.win * a.win + 63) / 64) {  // win <= SVO_KLT_MAX_WIN = 21: at most 7
        case 1: hipLaunchKernelGGL(klt_kernel<1>, g, b, 0, s, a); break;
        case 2: hipLaunchKernelGGL(klt_kernel<2>, g, b, 0, s, a); break;
        case 3: hipLaunchKernelGGL(klt_kernel<3>, g, b, 0, s, a); break;
        case 4: hipLaunchKernelGGL(klt_kernel<4>, g, b, 0, s, a); break;
        case 5: hipLaunchKernelGGL(klt_kernel<5>, g, b, 0, s, a); break;
        case 6: hipLaunchKernelGGL(klt_kernel<6>, g, b, 0, s, a); break;
        default: hipLaunchKernelGGL(klt_kernel<7>, g, b, 0, s, a); break;
    }
}

}  // namespace svo
