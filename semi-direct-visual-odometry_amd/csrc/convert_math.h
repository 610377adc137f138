// convert_math.h — the per-thread body of the pixel-format conversion (convert.hip), host and device: the address
// arithmetic, the loads of a thread's input bytes and the packing of its four grey values.  The contract is stated in
// include/svo_c.h ("pixel formats"); tests/convert_ref.py restates it in numpy, and tests/cpp/convert_model.cpp runs
// this body for every thread index of a launch on the CPU, over an exactly sized heap buffer.
//
// Memory is reached only through the `Mem` argument (ld32 / ld8 / st32 / st8): plain loads and stores on the device,
// range-checked ones in the model.  No HIP header is needed, so a plain C++ compiler builds this file.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define SVO_CONVERT_HD __host__ __device__ __forceinline__
#else
#define SVO_CONVERT_HD inline
#endif

namespace svo {

// the values of SVO_PIXEL_* (include/svo_c.h)
enum : int32_t { kPixGray8 = 0, kPixBgr8, kPixRgb8, kPixBgra8, kPixRgba8, kPixGray16, kPixFormats };

SVO_CONVERT_HD constexpr int32_t convert_bpp(int32_t fmt) {
    return fmt == kPixGray8 ? 1 : fmt == kPixGray16 ? 2 : (fmt == kPixBgr8 || fmt == kPixRgb8) ? 3 : 4;
}

// Y = (4899 R + 9617 G + 1868 B + 8192) >> 14: the weights sum to 2^14, so the result is at most 255
SVO_CONVERT_HD constexpr uint32_t convert_luma(uint32_t r, uint32_t g, uint32_t b) {
    return (4899u * r + 9617u * g + 1868u * b + 8192u) >> 14;
}

struct ConvertArgs {
    const uint8_t* src;    // the first byte of the layout
    int64_t src_bytes;     // what svo_image_layout_bytes reports: no load leaves [src, src + src_bytes)
    uint8_t* dst;          // grey plane k at dst + k * dst_stride, rows packed (width bytes)
    int64_t row_stride, image_stride, dst_stride;  // resolved: never 0
    int32_t width, height, count;
    int32_t shift;         // GRAY16
    int32_t groups;        // threads per row: convert_groups(width)
    int32_t per_thread;    // images one thread walks (grid y = count / per_thread, rounded up)
};

// A row is cut at the dword boundaries of its OUTPUT: with phase = (address of the row's first output byte) & 3, group g
// owns the pixels [4g - phase, 4g - phase + 4) that exist.  Every whole group then stores one aligned dword, and only
// the first and the last group of a row can be partial (byte stores).  (width + 3) / 4 + 1 groups cover any phase.
SVO_CONVERT_HD constexpr int32_t convert_groups(int32_t width) { return (width + 3) / 4 + 1; }

// The `nbytes` (<= 4 * kWords) input bytes from offset `off` of the layout, as little-endian words from w[0]; what
// follows byte nbytes in w is unspecified (a partial group stores only its own pixels).  The span is covered with ALIGNED dword loads; a dword that is not wholly inside the layout's
// bytes [0, src_bytes) -- it would reach before an unaligned start or past the end -- is put together from byte loads
// of the span's own bytes instead.  So no load leaves the layout's bytes and none is misaligned.
template <int kWords, class Mem>
SVO_CONVERT_HD void convert_load_span(const ConvertArgs& a, int64_t off, int32_t nbytes, uint32_t (&w)[kWords], Mem& mem) {
    const int32_t mis = (int32_t)((reinterpret_cast<uintptr_t>(a.src) + (uintptr_t)off) & 3u);
    const int64_t first = off - mis, end = off + nbytes;  // first: the aligned dword that holds byte `off` (may be < 0)
    uint32_t d[kWords + 1];
#pragma unroll
    for (int i = 0; i <= kWords; ++i) {
        const int64_t o = first + 4 * i;
        uint32_t v = 0;
        if (o < end) {
            if (o >= 0 && o + 4 <= a.src_bytes) {
                v = mem.ld32(a.src + o);
            } else {
#pragma unroll
                for (int b = 0; b < 4; ++b)
                    if (o + b >= off && o + b < end) v |= (uint32_t)mem.ld8(a.src + (o + b)) << (8 * b);
            }
        }
        d[i] = v;
    }
    const uint32_t sh = 8u * (uint32_t)mis;
#pragma unroll
    for (int i = 0; i < kWords; ++i) w[i] = (uint32_t)(((uint64_t)d[i + 1] << 32 | d[i]) >> sh);
}

SVO_CONVERT_HD uint32_t convert_byte(const uint32_t* w, int j) { return (w[j >> 2] >> (8 * (j & 3))) & 0xFFu; }

// four pixels' input words to four grey bytes, pixel 0 in the low byte
template <int kFmt>
SVO_CONVERT_HD uint32_t convert_pack(const uint32_t* w, int32_t shift) {
    if (kFmt == kPixGray8) return w[0];
    uint32_t out = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t y;
        if (kFmt == kPixGray16) {
            const uint32_t v = (w[i >> 1] >> (16 * (i & 1))) & 0xFFFFu;
            y = v >> shift;
            y = y < 255u ? y : 255u;
        } else {
            constexpr int bpp = convert_bpp(kFmt);
            constexpr bool blue_first = kFmt == kPixBgr8 || kFmt == kPixBgra8;
            const uint32_t c0 = convert_byte(w, bpp * i), g = convert_byte(w, bpp * i + 1), c2 = convert_byte(w, bpp * i + 2);
            y = blue_first ? convert_luma(c2, g, c0) : convert_luma(c0, g, c2);
        }
        out |= y << (8 * i);
    }
    return out;
}

// Thread `idx` of grid row `slice`: group idx % groups of row idx / groups, in images [slice * per_thread, ..).
template <int kFmt, class Mem>
SVO_CONVERT_HD void convert_thread(const ConvertArgs& a, int64_t idx, int32_t slice, Mem& mem) {
    constexpr int32_t bpp = convert_bpp(kFmt);
    constexpr int kWords = bpp;  // 4 pixels * bpp bytes / 4
    if (idx >= (int64_t)a.groups * a.height) return;
    const int32_t y = (int32_t)(idx / a.groups), g = (int32_t)(idx - (int64_t)y * a.groups);
    const int32_t k0 = slice * a.per_thread, k1 = k0 + a.per_thread < a.count ? k0 + a.per_thread : a.count;
    for (int32_t k = k0; k < k1; ++k) {
        const int64_t orow = (int64_t)k * a.dst_stride + (int64_t)y * a.width;
        const int32_t phase = (int32_t)((reinterpret_cast<uintptr_t>(a.dst) + (uintptr_t)orow) & 3u);
        const int32_t xa = 4 * g - phase > 0 ? 4 * g - phase : 0;
        const int32_t xb = 4 * g - phase + 4 < a.width ? 4 * g - phase + 4 : a.width;
        const int32_t npx = xb - xa;
        if (npx <= 0) continue;
        uint32_t w[kWords];
        convert_load_span<kWords>(a, (int64_t)k * a.image_stride + (int64_t)y * a.row_stride + (int64_t)xa * bpp,
                                  npx * bpp, w, mem);
        const uint32_t v = convert_pack<kFmt>(w, a.shift);
        uint8_t* out = a.dst + orow + xa;
        if (npx == 4) {  // a whole group starts on a dword boundary by construction
            mem.st32(out, v);
        } else {
            mem.st8(out, (uint8_t)v);
            if (npx > 1) mem.st8(out + 1, (uint8_t)(v >> 8));
            if (npx > 2) mem.st8(out + 2, (uint8_t)(v >> 16));
        }
    }
}

}  // namespace svo
