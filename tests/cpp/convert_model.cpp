// CPU model of a launch of the pixel-format conversion kernel (csrc/convert.hip): the per-thread body of
// csrc/convert_math.h run for every thread index of the grid, over input and output buffers of exactly the contract's
// sizes.  Every load must lie inside the bytes svo_image_layout_bytes reports, every dword access must be aligned,
// every output byte must be written exactly once, and the result must equal the scalar loop below.
//   convert_model            the shapes of tests/test_convert_gpu.py's edge list; prints "ok <cases>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../semi-direct-visual-odometry_amd/csrc/convert_math.h"

using namespace svo;

struct CheckedMem {
    const uint8_t *src_lo, *src_hi;
    uint8_t *dst_lo, *dst_hi;
    std::vector<uint8_t> written;  // per output byte of [dst_lo, dst_hi)
    bool ok = true;
    void bad(const char* what, const void* p) {
        if (ok) std::fprintf(stderr, "%s at src%+lld / dst%+lld\n", what, (long long)((const uint8_t*)p - src_lo),
                             (long long)((const uint8_t*)p - dst_lo));
        ok = false;
    }
    uint32_t ld32(const uint8_t* p) {
        if (p < src_lo || p + 4 > src_hi) return bad("dword load outside the layout", p), 0;
        if (reinterpret_cast<uintptr_t>(p) & 3) return bad("misaligned dword load", p), 0;
        uint32_t v;
        std::memcpy(&v, p, 4);
        return v;
    }
    uint32_t ld8(const uint8_t* p) {
        if (p < src_lo || p >= src_hi) return bad("byte load outside the layout", p), 0;
        return *p;
    }
    void st8(uint8_t* p, uint8_t v) {
        if (p < dst_lo || p >= dst_hi) return bad("store outside the planes", p);
        if (written[p - dst_lo]++) return bad("output byte written twice", p);
        *p = v;
    }
    void st32(uint8_t* p, uint32_t v) {
        if (reinterpret_cast<uintptr_t>(p) & 3) return bad("misaligned dword store", p);
        for (int b = 0; b < 4; ++b) st8(p + b, (uint8_t)(v >> (8 * b)));
    }
};

static uint8_t scalar_pixel(int fmt, const uint8_t* p, int shift) {
    switch (fmt) {
        case kPixGray8: return p[0];
        case kPixGray16: {
            uint16_t v;
            std::memcpy(&v, p, 2);
            const uint32_t y = (uint32_t)v >> shift;
            return (uint8_t)(y < 255 ? y : 255);
        }
        case kPixBgr8: case kPixBgra8: return (uint8_t)((4899u * p[2] + 9617u * p[1] + 1868u * p[0] + 8192u) >> 14);
        default: return (uint8_t)((4899u * p[0] + 9617u * p[1] + 1868u * p[2] + 8192u) >> 14);
    }
}

template <int kFmt>
static void run_grid(const ConvertArgs& a, CheckedMem& mem) {
    const int64_t threads = ((int64_t)a.groups * a.height + 255) / 256 * 256;  // whole blocks, as the launch has them
    const int32_t slices = (a.count + a.per_thread - 1) / a.per_thread;
    for (int32_t s = 0; s < slices; ++s)
        for (int64_t idx = 0; idx < threads; ++idx) convert_thread<kFmt>(a, idx, s, mem);
}

static uint32_t rng_state = 12345;
static uint8_t rnd() {
    rng_state = rng_state * 1664525u + 1013904223u;
    return (uint8_t)(rng_state >> 24);
}

static bool one_case(int fmt, int width, int height, int count, int row_pad, int pad_rows, int src_off, int dst_off,
                     int per_thread, int shift) {
    const int bpp = convert_bpp(fmt);
    ConvertArgs a{};
    a.width = width; a.height = height; a.count = count; a.shift = shift;
    a.groups = convert_groups(width); a.per_thread = per_thread;
    a.row_stride = (int64_t)width * bpp + row_pad;
    a.image_stride = a.row_stride * (height + pad_rows);
    a.src_bytes = a.image_stride * (count - 1) + a.row_stride * (height - 1) + (int64_t)width * bpp;
    a.dst_stride = (int64_t)width * height;
    const int64_t dst_bytes = a.dst_stride * count;
    // exactly sized heap blocks (the offsets shift the alignment; the bytes ahead of them are outside the layout too)
    uint8_t* sbuf = (uint8_t*)std::malloc((size_t)(a.src_bytes + src_off));
    uint8_t* dbuf = (uint8_t*)std::malloc((size_t)(dst_bytes + dst_off));
    for (int64_t i = 0; i < a.src_bytes + src_off; ++i) sbuf[i] = rnd();
    std::memset(dbuf, 0xA5, (size_t)(dst_bytes + dst_off));
    a.src = sbuf + src_off;
    a.dst = dbuf + dst_off;
    CheckedMem mem{a.src, a.src + a.src_bytes, a.dst, a.dst + dst_bytes, std::vector<uint8_t>((size_t)dst_bytes, 0)};
    switch (fmt) {
        case kPixGray8: run_grid<kPixGray8>(a, mem); break;
        case kPixBgr8: run_grid<kPixBgr8>(a, mem); break;
        case kPixRgb8: run_grid<kPixRgb8>(a, mem); break;
        case kPixBgra8: run_grid<kPixBgra8>(a, mem); break;
        case kPixRgba8: run_grid<kPixRgba8>(a, mem); break;
        default: run_grid<kPixGray16>(a, mem); break;
    }
    bool ok = mem.ok;
    for (int k = 0; k < count && ok; ++k)
        for (int y = 0; y < height && ok; ++y)
            for (int x = 0; x < width; ++x) {
                const int64_t o = k * a.dst_stride + (int64_t)y * width + x;
                const uint8_t want = scalar_pixel(fmt, a.src + k * a.image_stride + y * a.row_stride + (int64_t)x * bpp, shift);
                if (mem.written[o] != 1 || a.dst[o] != want) {
                    std::fprintf(stderr, "pixel (%d, %d, %d): written %d times, %d, expected %d\n", k, y, x,
                                 mem.written[o], a.dst[o], want);
                    ok = false;
                    break;
                }
            }
    for (int i = 0; i < dst_off; ++i) ok = ok && dbuf[i] == 0xA5;
    if (!ok)
        std::fprintf(stderr, "FAILED: format %d, %dx%d x %d, row pad %d, image pad %d rows, src +%d, dst +%d, per thread %d\n",
                     fmt, width, height, count, row_pad, pad_rows, src_off, dst_off, per_thread);
    std::free(sbuf);
    std::free(dbuf);
    return ok;
}

int main() {
    const int widths[] = {1, 2, 3, 4, 5, 7, 8, 9, 61, 64, 67}, heights[] = {1, 2, 5};
    const int pads8[] = {0, 1, 3, 13}, pads16[] = {0, 2, 6};
    long cases = 0;
    for (int fmt = 0; fmt < kPixFormats; ++fmt) {
        const bool g16 = fmt == kPixGray16;
        for (int w : widths)
            for (int h : heights)
                for (int pi = 0; pi < (g16 ? 3 : 4); ++pi)
                    for (int count : {1, 3})
                        for (int so = 0; so < 4; so += g16 ? 2 : 1)
                            for (int dof = 0; dof < 4; ++dof) {
                                const int per_thread = 1 + (int)(cases % 4);
                                const int shift = g16 ? (int)(cases % 9) : 0;
                                if (!one_case(fmt, w, h, count, g16 ? pads16[pi] : pads8[pi], count > 1 ? 5 : 0, so, dof,
                                              per_thread, shift))
                                    return 1;
                                ++cases;
                            }
    }
    std::printf("ok %ld\n", cases);
    return 0;
}
