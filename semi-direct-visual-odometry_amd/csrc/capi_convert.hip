// capi_convert.hip — C ABI: frames of a pixel format into grey planes and into level 0 of a pyramid set (kernel:
// convert.hip; contract: include/svo_c.h, "pixel formats").
#include <cstdlib>

#include "capi_ctx.h"
#include "convert_math.h"
using namespace svo::shim;

static_assert(SVO_PIXEL_GRAY8 == svo::kPixGray8 && SVO_PIXEL_BGR8 == svo::kPixBgr8 && SVO_PIXEL_RGB8 == svo::kPixRgb8 &&
              SVO_PIXEL_BGRA8 == svo::kPixBgra8 && SVO_PIXEL_RGBA8 == svo::kPixRgba8 &&
              SVO_PIXEL_GRAY16 == svo::kPixGray16, "convert_math.h restates SVO_PIXEL_*");

namespace {
// images one thread walks: SVO_CONVERT_PER_THREAD overrides the default (tools/convert_time.py)
int32_t convert_per_thread(int32_t count) {
    static const int32_t knob = [] {
        const char* e = std::getenv("SVO_CONVERT_PER_THREAD");
        const int v = e ? std::atoi(e) : 0;
        return v > 0 ? v : 4;
    }();
    const int32_t floor_for_grid = (count + 65534) / 65535;  // grid y <= 65535
    return knob > floor_for_grid ? knob : floor_for_grid;
}

// The layout with its strides resolved, and the bytes it spans; every message carries `entry`.
int resolve(const char* entry, const svo_image_layout* l, int32_t width, int32_t height, int32_t count,
            svo::ConvertArgs* a) {
    if (!l) return fail(SVO_ERR_ARG, "%s: null layout", entry);
    if (l->format < 0 || l->format >= svo::kPixFormats)
        return fail(SVO_ERR_ARG, "%s: unknown pixel format %d", entry, l->format);
    if (width < 1 || height < 1) return fail(SVO_ERR_ARG, "%s: bad image size %dx%d", entry, width, height);
    if (count < 0) return fail(SVO_ERR_ARG, "%s: count < 0", entry);
    const bool g16 = l->format == SVO_PIXEL_GRAY16;
    if (g16 && (l->shift < 0 || l->shift > 8))
        return fail(SVO_ERR_ARG, "%s: GRAY16 shift %d is outside 0..8", entry, l->shift);
    const int64_t row_bytes = (int64_t)width * svo::convert_bpp(l->format);
    const int64_t row_stride = l->row_stride ? l->row_stride : row_bytes;
    if (row_stride < row_bytes)
        return fail(SVO_ERR_ARG, "%s: row stride %lld is below the %lld bytes of a row", entry, (long long)row_stride,
                    (long long)row_bytes);
    const int64_t image_bytes = row_stride * (height - 1) + row_bytes;
    const int64_t image_stride = l->image_stride ? l->image_stride : row_stride * height;
    if (image_stride < image_bytes)
        return fail(SVO_ERR_ARG, "%s: image stride %lld is below the %lld bytes of an image", entry,
                    (long long)image_stride, (long long)image_bytes);
    if (g16 && ((row_stride | image_stride) & 1))
        return fail(SVO_ERR_ARG, "%s: a GRAY16 stride is odd (%lld, %lld)", entry, (long long)row_stride,
                    (long long)image_stride);
    a->row_stride = row_stride; a->image_stride = image_stride;
    a->src_bytes = count ? image_stride * (count - 1) + image_bytes : 0;
    a->width = width; a->height = height; a->count = count;
    a->shift = g16 ? l->shift : 0;
    a->groups = svo::convert_groups(width);
    a->per_thread = convert_per_thread(count);
    return SVO_OK;
}

int check_pointer(const char* entry, const svo_image_layout* l, const void* images) {
    if (l->format == SVO_PIXEL_GRAY16 && (reinterpret_cast<uintptr_t>(images) & 1))
        return fail(SVO_ERR_ARG, "%s: a GRAY16 image pointer is odd", entry);
    return SVO_OK;
}

int upload_format(svo_pyramid_set* p, int32_t first, int32_t count, const void* images, bool on_device,
                  const svo_image_layout* l, const svo_undistort_map* m, const char* entry) {
    if (!p || !images) return fail(SVO_ERR_ARG, "%s: null argument", entry);
    svo::ConvertArgs a{};
    if (int r = resolve(entry, l, p->width, p->height, count, &a)) return r;
    if (int r = check_pointer(entry, l, images)) return r;
    if (m)
        if (int r = check_map_for_set(p, m, entry)) return r;
    if (first < 0 || first + count > p->n_frames) return fail(SVO_ERR_ARG, "%s: frames out of range", entry);
    if (count == 0) return SVO_OK;
    svo_ctx* c = p->ctx;
    SVO_HIP(hipSetDevice(c->device));
    SVO_HIP(set_join(p));
    hipStream_t s = ctx_stream(c);
    const int64_t n = (int64_t)p->width * p->height;
    uint8_t* grey = nullptr;  // with a map: the converted planes, packed, between the two kernels
    a.src = static_cast<const uint8_t*>(images);
    Block blk(c, s);
    if (!on_device) blk.in(&a.src, static_cast<const uint8_t*>(images), (size_t)a.src_bytes);  // the raw bytes' staging
    if (m) blk.dev(&grey, (size_t)count * (size_t)n);
    if ((!on_device || m) && blk.alloc() == hipSuccess && !on_device) blk.upload();
    blk.launch([&] {
        a.dst = m ? grey : p->d_base + (size_t)first * p->stride;  // level 0 of the intensity stack
        a.dst_stride = m ? n : p->stride;
        svo::launch_convert(a, l->format, s);
        if (m) launch_remap_into_set(m, grey, p, first, count, s);
    });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "%s: %s", entry, hipGetErrorString(blk.err));
    return SVO_OK;
}
}  // namespace

extern "C" {
int svo_image_layout_bytes(const svo_image_layout* layout, int32_t width, int32_t height, int32_t count,
                           int64_t* bytes) {
    if (!bytes) return fail(SVO_ERR_ARG, "svo_image_layout_bytes: null argument");
    svo::ConvertArgs a{};
    if (int r = resolve("svo_image_layout_bytes", layout, width, height, count, &a)) return r;
    *bytes = a.src_bytes;
    return SVO_OK;
}

int svo_convert_images(svo_ctx* c, const svo_image_layout* layout, int32_t width, int32_t height, int32_t count,
                       const void* host_in, uint8_t* host_out) {
    if (!c || !host_in || !host_out) return fail(SVO_ERR_ARG, "svo_convert_images: null argument");
    svo::ConvertArgs a{};
    if (int r = resolve("svo_convert_images", layout, width, height, count, &a)) return r;
    if (int r = check_pointer("svo_convert_images", layout, host_in)) return r;
    if (count == 0) return SVO_OK;
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    a.dst_stride = (int64_t)width * height;
    Block blk(c, s);
    blk.in(&a.src, static_cast<const uint8_t*>(host_in), (size_t)a.src_bytes);
    blk.out(&a.dst, host_out, (size_t)count * (size_t)a.dst_stride);
    if (blk.alloc() == hipSuccess) blk.run([&] { svo::launch_convert(a, layout->format, s); });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_convert_images: %s", hipGetErrorString(blk.err));
    return SVO_OK;
}

int svo_pyramid_set_upload_format(svo_pyramid_set* set, int32_t first, int32_t count, const void* host_images,
                                  const svo_image_layout* layout, const svo_undistort_map* map) {
    return upload_format(set, first, count, host_images, false, layout, map, "svo_pyramid_set_upload_format");
}

int svo_pyramid_set_upload_format_device(svo_pyramid_set* set, int32_t first, int32_t count, const void* dev_images,
                                         const svo_image_layout* layout, const svo_undistort_map* map) {
    return upload_format(set, first, count, dev_images, true, layout, map, "svo_pyramid_set_upload_format_device");
}
}  // extern "C"
