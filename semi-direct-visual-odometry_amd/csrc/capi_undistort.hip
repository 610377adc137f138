// capi_undistort.hip — C ABI: the undistortion map of a camera and the remap ahead of the pyramid (kernels:
// undistort.hip).
#include <cmath>
#include <cstdlib>
#include <new>

#include "capi_ctx.h"
using namespace svo::shim;

struct svo_undistort_map {
    svo_ctx* ctx;
    int32_t width, height;
    int64_t n, n_padded;
    uint32_t* d_xy;    // one allocation: xy[n_padded], then frac[n_padded]
    uint16_t* d_frac;
};

namespace {
// images one remap thread walks with its map entries: SVO_UNDISTORT_PER_THREAD overrides the default (tools/undistort_time.py
// sweeps it; the choice is measured in DESIGN.md 27)
int32_t remap_per_thread(int32_t count) {
    static const int32_t knob = [] {
        const char* e = std::getenv("SVO_UNDISTORT_PER_THREAD");
        const int v = e ? std::atoi(e) : 0;
        return v > 0 ? v : 8;
    }();
    const int32_t floor_for_grid = (count + 65534) / 65535;  // grid y <= 65535
    return knob > floor_for_grid ? knob : floor_for_grid;
}

svo::UndistortArgs remap_args(const svo_undistort_map* m, int32_t count) {
    svo::UndistortArgs a{};
    a.xy = m->d_xy; a.frac = m->d_frac;
    a.n = m->n; a.width = m->width; a.height = m->height;
    a.count = count; a.per_thread = remap_per_thread(count);
    return a;
}

int check_map(const svo_ctx* c, const svo_undistort_map* m, const char* entry) {
    if (!m) return fail(SVO_ERR_ARG, "%s: null undistort map", entry);
    if (c && m->ctx != c) return fail(SVO_ERR_ARG, "%s: undistort map belongs to another context", entry);
    return SVO_OK;
}

int upload_undistort(svo_pyramid_set* p, int32_t first, int32_t count, const uint8_t* images, bool on_device,
                     const svo_undistort_map* m, const char* entry) {
    if (!p || !images) return fail(SVO_ERR_ARG, "%s: null argument", entry);
    if (int r = check_map_for_set(p, m, entry)) return r;
    if (first < 0 || count < 0 || first + count > p->n_frames) return fail(SVO_ERR_ARG, "%s: frames out of range", entry);
    if (count == 0) return SVO_OK;
    svo_ctx* c = p->ctx;
    SVO_HIP(hipSetDevice(c->device));
    SVO_HIP(set_join(p));
    hipStream_t s = ctx_stream(c);
    const uint8_t* src = images;
    Block blk(c, s);
    if (!on_device) blk.in(&src, images, (size_t)count * (size_t)m->n);  // the raw images' staging: the context's per-call block
    if (!on_device && blk.alloc() == hipSuccess) blk.upload();
    blk.launch([&] { launch_remap_into_set(m, src, p, first, count, s); });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "%s: %s", entry, hipGetErrorString(blk.err));
    return SVO_OK;
}
}  // namespace

namespace svo::shim {
int check_map_for_set(const svo_pyramid_set* p, const svo_undistort_map* m, const char* entry) {
    if (int r = check_map(p->ctx, m, entry)) return r;
    if (m->width != p->width || m->height != p->height)
        return fail(SVO_ERR_ARG, "%s: the undistort map is %dx%d, the pyramid set %dx%d", entry, m->width, m->height,
                    p->width, p->height);
    return SVO_OK;
}

void launch_remap_into_set(const svo_undistort_map* m, const uint8_t* dev_src, svo_pyramid_set* p, int32_t first,
                           int32_t count, hipStream_t s) {
    svo::UndistortArgs a = remap_args(m, count);
    a.src = dev_src;
    a.src_stride = m->n;
    a.dst = p->d_base + (size_t)first * p->stride;  // level 0 of the intensity stack
    a.dst_stride = p->stride;
    svo::launch_undistort_remap(a, s);
}
}  // namespace svo::shim

extern "C" {
int svo_undistort_map_create(svo_ctx* c, const svo_camera* cam, const svo_distortion* d, svo_undistort_map** out) {
    if (!c || !cam || !d || !out) return fail(SVO_ERR_ARG, "svo_undistort_map_create: null argument");
    *out = nullptr;
    if (cam->width < 1 || cam->height < 1)
        return fail(SVO_ERR_ARG, "svo_undistort_map_create: bad image size %dx%d", cam->width, cam->height);
    if (cam->width > 32767 || cam->height > 32767)
        return fail(SVO_ERR_ARG, "svo_undistort_map_create: image size %dx%d is past the int16 map (at most 32767 x 32767)",
                    cam->width, cam->height);
    const double vals[] = {cam->fx, cam->fy, cam->cx, cam->cy, d->k1, d->k2, d->p1, d->p2, d->k3};
    for (double v : vals)
        if (!std::isfinite(v)) return fail(SVO_ERR_ARG, "svo_undistort_map_create: non-finite camera or coefficient");
    if (cam->fx == 0.0 || cam->fy == 0.0) return fail(SVO_ERR_ARG, "svo_undistort_map_create: zero focal length");
    SVO_HIP(hipSetDevice(c->device));
    svo_undistort_map* m = new (std::nothrow) svo_undistort_map{};
    if (!m) return fail(SVO_ERR_ARG, "out of host memory");
    m->ctx = c; m->width = cam->width; m->height = cam->height;
    m->n = (int64_t)cam->width * cam->height;
    m->n_padded = (m->n + 3) / 4 * 4;
    const hipError_t e = hipMalloc(&m->d_xy, (size_t)m->n_padded * 6);
    if (e != hipSuccess) {
        delete m;
        return fail(SVO_ERR_HIP, "hipMalloc(undistort map): %s", hipGetErrorString(e));
    }
    m->d_frac = reinterpret_cast<uint16_t*>(m->d_xy + m->n_padded);
    svo::UndistortMapArgs a{};
    a.xy = m->d_xy; a.frac = m->d_frac; a.n = m->n; a.n_padded = m->n_padded;
    a.width = m->width; a.height = m->height;
    fill_camera(a, cam);
    a.k1 = d->k1; a.k2 = d->k2; a.p1 = d->p1; a.p2 = d->p2; a.k3 = d->k3;
    svo::launch_undistort_map(a, ctx_stream(c));
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) {
        svo_undistort_map_destroy(m);
        return fail(SVO_ERR_HIP, "svo_undistort_map_create: %s", hipGetErrorString(le));
    }
    *out = m;
    return SVO_OK;
}

int svo_undistort_map_destroy(svo_undistort_map* m) {
    if (!m) return SVO_OK;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(ctx_stream(m->ctx));
    (void)hipFree(m->d_xy);
    delete m;
    return SVO_OK;
}

int svo_undistort_map_download(const svo_undistort_map* m, int16_t* xy, uint16_t* frac) {
    if (int r = check_map(nullptr, m, "svo_undistort_map_download")) return r;
    if (!xy || !frac) return fail(SVO_ERR_ARG, "svo_undistort_map_download: null argument");
    SVO_HIP(hipSetDevice(m->ctx->device));
    hipStream_t s = ctx_stream(m->ctx);
    SVO_HIP(hipMemcpyAsync(xy, m->d_xy, (size_t)m->n * 4, hipMemcpyDeviceToHost, s));
    SVO_HIP(hipMemcpyAsync(frac, m->d_frac, (size_t)m->n * 2, hipMemcpyDeviceToHost, s));
    SVO_HIP(hipStreamSynchronize(s));
    return SVO_OK;
}

int svo_undistort_images(svo_ctx* c, const svo_undistort_map* m, const uint8_t* host_in, uint8_t* host_out,
                         int32_t count) {
    if (!c || !host_in || !host_out) return fail(SVO_ERR_ARG, "svo_undistort_images: null argument");
    if (int r = check_map(c, m, "svo_undistort_images")) return r;
    if (count < 0) return fail(SVO_ERR_ARG, "svo_undistort_images: count < 0");
    if (count == 0) return SVO_OK;
    SVO_HIP(hipSetDevice(c->device));
    hipStream_t s = ctx_stream(c);
    svo::UndistortArgs a = remap_args(m, count);
    a.src_stride = a.dst_stride = m->n;
    const size_t bytes = (size_t)count * (size_t)m->n;
    Block blk(c, s);
    blk.in(&a.src, host_in, bytes);
    blk.out(&a.dst, host_out, bytes);
    if (blk.alloc() == hipSuccess) blk.run([&] { svo::launch_undistort_remap(a, s); });
    if (!blk.ok()) return fail(SVO_ERR_HIP, "svo_undistort_images: %s", hipGetErrorString(blk.err));
    return SVO_OK;
}

int svo_pyramid_set_upload_undistort(svo_pyramid_set* p, int32_t first, int32_t count, const uint8_t* host_images,
                                     const svo_undistort_map* m) {
    return upload_undistort(p, first, count, host_images, false, m, "svo_pyramid_set_upload_undistort");
}

int svo_pyramid_set_upload_undistort_device(svo_pyramid_set* p, int32_t first, int32_t count, const uint8_t* dev_images,
                                            const svo_undistort_map* m) {
    return upload_undistort(p, first, count, dev_images, true, m, "svo_pyramid_set_upload_undistort_device");
}
}  // extern "C"
