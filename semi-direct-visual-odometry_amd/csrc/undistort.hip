// undistort.hip — lens undistortion ahead of the pyramid (contract: include/svo_c.h, svo_undistort_*).
//   map kernel    one thread per output pixel: the contract's fp64 arithmetic (this file is compiled with
//                 -ffp-contract=off like every other), the fixed-point source position as OpenCV's CV_16SC2 + CV_16UC1
//                 pair: xy[p] = X | Y << 16 (int16 each, clamped), frac[p] = ay << 5 | ax.  Built once per camera.
//   remap kernel  the hot path: a thread owns four adjacent output pixels of the (tightly packed) plane, reads their
//                 map entries as one 16-B and one 8-B load, turns them into two byte-pair offsets and four integer
//                 weights per pixel (a tap outside the image: weight 0, offset clamped into the plane, so no load is
//                 conditional and none leaves the image), and then walks the images of its slice of the batch: eight
//                 16-bit gathers and one dword store per image.  The map entry is read once per thread however many
//                 images share it.  No LDS.
#include "svo_internal.h"

namespace svo {
namespace {

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads)
undistort_map_kernel(UndistortMapArgs a) {
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= a.n_padded) return;
    if (p >= a.n) {  // the padding that lets the remap kernel read whole vectors: every tap outside
        a.xy[p] = 0xFFFEFFFEu;
        a.frac[p] = 0;
        return;
    }
    const int32_t i = (int32_t)(p / a.width), j = (int32_t)(p - (int64_t)i * a.width);
    const double x = ((double)j - a.cx) / a.fx, y = ((double)i - a.cy) / a.fy;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, xy2 = 2.0 * x * y;
    const double kr = 1.0 + ((a.k3 * r2 + a.k2) * r2 + a.k1) * r2;
    const double xd = x * kr + a.p1 * xy2 + a.p2 * (r2 + 2.0 * x2);
    const double yd = y * kr + a.p1 * (r2 + 2.0 * y2) + a.p2 * xy2;
    const double u = a.fx * xd + a.cx, v = a.fy * yd + a.cy;
    // rint: ties to even; saturated to int32 before the conversion
    const int32_t iu = (int32_t)fmin(fmax(rint(u * 32.0), -2147483648.0), 2147483647.0);
    const int32_t iv = (int32_t)fmin(fmax(rint(v * 32.0), -2147483648.0), 2147483647.0);
    const int32_t X = min(max(iu >> 5, -2), a.width), Y = min(max(iv >> 5, -2), a.height);
    a.xy[p] = ((uint32_t)X & 0xFFFFu) | ((uint32_t)Y << 16);
    a.frac[p] = (uint16_t)(((iv & 31) << 5) | (iu & 31));
}

// The taps of one output pixel as two byte pairs, one per source row: (Y, X), (Y, X+1) are adjacent bytes, and so are
// (Y+1, X), (Y+1, X+1).  A pair starts at column clamp(X, 0, w-2), so it never leaves its row; lo / hi are the weights of
// its two bytes: (w00, w01) in the interior, (w01, 0) at X = -1 (only column 0 counts), (0, w00) at X = w-1 (only column
// w-1), 0 for a row or a column outside.  Every offset lies inside the plane whatever the map holds.
struct Taps {
    int32_t o0, o1;              // byte offset of the pair in rows Y and Y+1 (clamped into the plane)
    uint32_t lo0, hi0, lo1, hi1; // weights of the pair's bytes in row Y, in row Y+1
};

template <bool kPairs>
__device__ __forceinline__ Taps make_taps(uint32_t xy, uint32_t fr, int32_t w, int32_t h) {
    const int32_t X = (int32_t)(int16_t)(xy & 0xFFFFu), Y = (int32_t)(int16_t)(xy >> 16);
    const uint32_t ax = fr & 31u, ay = (fr >> 5) & 31u;
    const bool x0 = X >= 0 && X < w, x1 = X + 1 >= 0 && X + 1 < w, y0 = Y >= 0 && Y < h, y1 = Y + 1 >= 0 && Y + 1 < h;
    const uint32_t wx0 = x0 ? 32u - ax : 0u, wx1 = x1 ? ax : 0u;        // column weights, 0 outside
    const uint32_t wy0 = y0 ? 32u - ay : 0u, wy1 = y1 ? ay : 0u;        // row weights, 0 outside
    // the pair's first column, and which of its bytes columns X and X+1 are
    const int32_t c = kPairs ? min(max(X, 0), w - 2) : min(max(X, 0), w - 1);
    uint32_t lo, hi;
    if (kPairs) {
        lo = X == c ? wx0 : (X + 1 == c ? wx1 : 0u);
        hi = X == c ? wx1 : (X == c + 1 ? wx0 : 0u);
    } else {  // one-column images: a single byte per row, column 0
        lo = X == 0 ? wx0 : (X == -1 ? wx1 : 0u);
        hi = 0u;
    }
    Taps t;
    t.o0 = min(max(Y, 0), h - 1) * w + c;
    t.o1 = min(max(Y + 1, 0), h - 1) * w + c;
    t.lo0 = lo * wy0; t.hi0 = hi * wy0; t.lo1 = lo * wy1; t.hi1 = hi * wy1;
    return t;
}

template <bool kPairs>
__device__ __forceinline__ uint32_t tap_sum(const Taps& t, const uint8_t* __restrict__ in) {
    uint32_t a, b;
    if (kPairs) {  // two adjacent bytes in one (possibly odd-addressed) 16-bit load
        uint16_t p0, p1;
        __builtin_memcpy(&p0, in + t.o0, 2);
        __builtin_memcpy(&p1, in + t.o1, 2);
        a = t.lo0 * (p0 & 0xFFu) + t.hi0 * (uint32_t)(p0 >> 8);
        b = t.lo1 * (p1 & 0xFFu) + t.hi1 * (uint32_t)(p1 >> 8);
    } else {
        a = t.lo0 * in[t.o0];
        b = t.lo1 * in[t.o1];
    }
    return (a + b + 512u) >> 10;
}

template <bool kPairs>
__global__ void __launch_bounds__(kThreads)
undistort_remap_kernel(UndistortArgs a) {
    const int64_t p = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * 4;
    if (p >= a.n) return;
    // the map planes are padded to a multiple of four entries, so the vector reads are always whole
    const uint4 xy = *reinterpret_cast<const uint4*>(a.xy + p);
    const uint2 fr = *reinterpret_cast<const uint2*>(a.frac + p);
    const Taps t0 = make_taps<kPairs>(xy.x, fr.x & 0xFFFFu, a.width, a.height);
    const Taps t1 = make_taps<kPairs>(xy.y, fr.x >> 16, a.width, a.height);
    const Taps t2 = make_taps<kPairs>(xy.z, fr.y & 0xFFFFu, a.width, a.height);
    const Taps t3 = make_taps<kPairs>(xy.w, fr.y >> 16, a.width, a.height);
    const int32_t live = (int32_t)min((int64_t)4, a.n - p);  // < 4: the plane's tail
    const int32_t k0 = (int32_t)blockIdx.y * a.per_thread, k1 = min(k0 + a.per_thread, a.count);
    for (int32_t k = k0; k < k1; ++k) {
        const uint8_t* __restrict__ in = a.src + (int64_t)k * a.src_stride;
        uint8_t* out = a.dst + (int64_t)k * a.dst_stride + p;
        const uint32_t v0 = tap_sum<kPairs>(t0, in), v1 = tap_sum<kPairs>(t1, in);
        const uint32_t v2 = tap_sum<kPairs>(t2, in), v3 = tap_sum<kPairs>(t3, in);
        if (live == 4 && (reinterpret_cast<uintptr_t>(out) & 3u) == 0) {
            *reinterpret_cast<uint32_t*>(out) = v0 | v1 << 8 | v2 << 16 | v3 << 24;
        } else {  // a plane that starts off a dword boundary, or the tail: bytewise
            out[0] = (uint8_t)v0;
            if (live > 1) out[1] = (uint8_t)v1;
            if (live > 2) out[2] = (uint8_t)v2;
            if (live > 3) out[3] = (uint8_t)v3;
        }
    }
}

}  // namespace

void launch_undistort_map(const UndistortMapArgs& a, hipStream_t s) {
    const uint32_t blocks = (uint32_t)((a.n_padded + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(undistort_map_kernel, dim3(blocks), dim3(kThreads), 0, s, a);
}

void launch_undistort_remap(const UndistortArgs& a, hipStream_t s) {
    if (a.count <= 0 || a.n <= 0) return;
    const uint32_t bx = (uint32_t)(((a.n + 3) / 4 + kThreads - 1) / kThreads);
    const uint32_t by = (uint32_t)((a.count + a.per_thread - 1) / a.per_thread);
    if (a.width >= 2) hipLaunchKernelGGL(undistort_remap_kernel<true>, dim3(bx, by), dim3(kThreads), 0, s, a);
    else hipLaunchKernelGGL(undistort_remap_kernel<false>, dim3(bx, by), dim3(kThreads), 0, s, a);
}

}  // namespace svo
