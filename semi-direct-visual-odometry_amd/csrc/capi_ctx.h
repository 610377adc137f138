// capi_ctx.h — what the C ABI's translation units share: the context and pyramid-set objects (capi.hip owns them),
// the argument checks every stage repeats, and Block.  Nothing declared here is exported from the library.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdio>
#include <cstring>
#include <vector>

#include "svo_internal.h"

#pragma GCC visibility push(hidden)
#include "block_layout.h"  // (its templates stay out of the library's exports too)
#pragma GCC visibility pop

struct svo_align_batch; struct svo_pyramid_set;

struct svo_ctx {
    int32_t device;
    // the context stream; every use goes through ctx_stream(), which first joins a batch's pending chains (below)
    hipStream_t stream_raw;
    hipStream_t sides[4];         // extra streams: a batch runs as concurrent sub-batch chains
    hipEvent_t fork, joins[4];    // sides wait for stream at fork; stream waits for each side at its join
    // Chains of a batch run are joined into the context stream lazily: a run leaves its side chains pending, the
    // next run of the same batch (same split) lets each chain follow its own previous run on its own stream, and any
    // other use of the context stream joins them first (ctx_stream).  So back-to-back runs of one batch are ordered
    // per chain -- the only data dependency between them: chain i reads and writes only its own pairs -- instead of
    // every chain of run k + 1 waiting for the slowest chain of run k.  SVO_DEFER_JOIN=0 joins after every run.
    const svo_align_batch* pending_batch = nullptr;
    int pending_chains = 0;
    hipEvent_t chain_marks[3][2 + 3 * svo::kMaxLevels];  // launch marks of chains 0..2 (staggered starts)
    hipEvent_t events[16];
    // svo_align_batch_set_pairs uploads on its own stream, so the copies overlap a pyramid build queued
    // on `stream`; staged: the upload is done; stage_free: the last scatter out of a staging block is done
    hipStream_t copy;
    hipEvent_t staged, stage_free;
    // svo_pyramid_set_build_async builds on its own stream, after everything queued on `stream` so far (prep_gate),
    // so that the next batch's pyramids build while the current batch aligns
    hipStream_t prep = nullptr;
    hipEvent_t prep_gate = nullptr;
    // grow-only scratch of the synchronous per-call entry points (FeatureAlignment): no device
    // allocation per call once warm
    void* scratch = nullptr;
    size_t scratch_bytes = 0;
    // pinned host staging of the same calls (fixed size, ctx_pinned): one H2D and one D2H copy per call
    void* pinned = nullptr;
    void* pinned_dev = nullptr;  // the same block as the device addresses it (stage_copy)
    size_t pinned_bytes = 0;
    // svo_align_batch_set_pair stages into the same block as a ring without waiting for its copies;
    // every other user of the block first drains them (ctx_pinned)
    size_t ring_off = 0;
    bool ring_pending = false;
    // pyramid sets with a build_async the context stream has not waited for yet (set_join removes them); the
    // batches' runs join the sets their pairs read from this list (a batch never dereferences a set it keeps)
    std::vector<svo_pyramid_set*> pending_sets;
};

struct svo_pyramid_set {
    svo_ctx* ctx;
    int32_t n_frames, width, height, levels;
    svo::LevelGeom geom;
    int64_t grad_off, stride;
    uint8_t* d_base;
    hipEvent_t ready = nullptr;  // svo_pyramid_set_build_async: recorded on the prep stream after the build
    bool pending = false;        // a build_async whose `ready` the context stream has not waited for yet
};

#pragma GCC visibility push(hidden)
namespace svo::shim {
// sets svo_last_error() of this thread and returns `code`
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define SVO_HIP(call)                                                                                 \
    do {                                                                                              \
        hipError_t e_ = (call);                                                                       \
        if (e_ != hipSuccess) return fail(SVO_ERR_HIP, "%s: %s (%s:%d)", #call, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                        \
    } while (0)

hipStream_t ctx_stream(svo_ctx* c);  // the context stream after the pending chains of the last batch run
hipError_t ctx_scratch(svo_ctx* c, size_t bytes, void** out);  // at least `bytes` (previous contents not kept)
hipError_t ctx_pinned(svo_ctx* c, size_t bytes, void** out);   // the drained pinned block, if `bytes` fit it
hipError_t ctx_ring_drain(svo_ctx* c);
// a copy on `s`; one that touches the context's pinned block runs as a kernel (see capi.hip)
hipError_t stage_copy(svo_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind, hipStream_t s);
hipError_t set_join(const svo_pyramid_set* p);  // the context stream waits for the set's last asynchronous build

// off[0 .. n] starts at 0, ascends, ends below 2^cap_bits (0: no cap); big null: "<table> too large"; entry may be null
inline int check_offsets(const char* entry, const char* table, const char* item, int32_t n, const int32_t* off,
                         int cap_bits, const char* big) {
    const char* sep = entry ? ": " : "";
    if (!entry) entry = "";
    if (!off) return fail(SVO_ERR_ARG, "%s%snull argument (%s)", entry, sep, table);
    if (off[0] != 0) return fail(SVO_ERR_ARG, "%s%s%s[0] must be 0", entry, sep, table);
    for (int32_t i = 0; i < n; ++i)
        if (off[i + 1] < off[i]) return fail(SVO_ERR_ARG, "%s%s%s not ascending at %s %d", entry, sep, table, item, i);
    if (cap_bits && off[n] >= ((int32_t)1 << cap_bits))
        return fail(SVO_ERR_ARG, "%s%s%s%s", entry, sep, big ? "" : table, big ? big : " too large");
    return SVO_OK;
}
// the per-pair table of the two-view stages (sizes, then pointers: checked before the context is looked at)
inline int check_pair_offsets(const char* entry, int32_t n_pairs, const int32_t* feat_off, int64_t* total) {
    if (n_pairs < 0) return fail(SVO_ERR_ARG, "%s: n_pairs < 0", entry);
    if (int r = check_offsets(entry, "feat_off", "pair", n_pairs, feat_off, 28, "too many matches")) return r;
    *total = feat_off[n_pairs];
    return SVO_OK;
}

// A pyramid-set argument: not null, of context c, of the camera's size (cam null: any), in this order.  `who`
// prefixes the first two messages ("<who>" or, with an index, "<who> <idx>: ").  The caller checks its frame index
// and calls set_join before it queues work that reads the planes.
inline int check_set(const svo_ctx* c, const svo_pyramid_set* p, const svo_camera* cam, const char* who = "",
                     int idx = -1) {
    if (!p || p->ctx != c) {
        const char* what = p ? "pyramid set belongs to another context" : "null pyramid set";
        return idx < 0 ? fail(SVO_ERR_ARG, "%s%s", who, what) : fail(SVO_ERR_ARG, "%s %d: %s", who, idx, what);
    }
    if (cam && (p->width != cam->width || p->height != cam->height))
        return fail(SVO_ERR_ARG, "camera/pyramid size mismatch");
    return SVO_OK;
}

// The undistortion map as an argument of another stage's upload (capi_undistort.hip owns the object): not null, of
// the set's context and size; and the remap of `count` packed device planes at `dev_src` into level 0 of frames
// [first, first + count), queued on s.
int check_map_for_set(const svo_pyramid_set* p, const svo_undistort_map* m, const char* entry);
void launch_remap_into_set(const svo_undistort_map* m, const uint8_t* dev_src, svo_pyramid_set* p, int32_t first,
                           int32_t count, hipStream_t s);

// the pinhole intrinsics of a kernel argument block
template <class A>
void fill_camera(A& a, const svo_camera* cam) { a.fx = cam->fx; a.fy = cam->fy; a.cx = cam->cx; a.cy = cam->cy; }

// One call's device buffers: declared once (BlockLayout), placed in the context's scratch by alloc(), which sets every
// declared pointer.  The first error of any step stays in `err`; later steps then do nothing.
//   direct  alloc(): one copy per non-empty piece to / from the caller's array, which (like any vector handed to
//           put) must stay alive until the next sync() / finish().
//   staged  alloc(kPageable / kDirect): inputs packed into the context's pinned block, one copy up, one down, finish()
//           hands the outputs out.  Past the pinned block's size: pageable staging, or direct copies.
class Block : public svo::BlockLayout {
  public:
    enum Staging { kNone, kPageable, kDirect };
    hipError_t err = hipSuccess;
    Block(svo_ctx* c, hipStream_t s) : c_(c), s_(s) {}
    bool ok() const { return err == hipSuccess; }
    hipError_t alloc(Staging st = kNone) {
        void *base = nullptr, *host = nullptr;
        if (overflow) return err = hipErrorInvalidValue;  // more than kMaxPieces pieces
        if ((err = ctx_scratch(c_, total, &base)) != hipSuccess) return err;
        db_ = static_cast<char*>(base);
        for (int i = 0; i < n_binds; ++i) {
            const void* p = db_ + binds[i].off;
            std::memcpy(binds[i].field, &p, sizeof(p));
        }
        if (st == kNone) return err;
        if (ctx_pinned(c_, out_end, &host) != hipSuccess && st == kPageable) {
            pageable_.resize(out_end);
            host = pageable_.data();
        }
        (void)hipGetLastError();
        hb_ = static_cast<char*>(host);
        return err;
    }
    template <class T>
    T* host(svo::Slot<T> p) const { return static_cast<T*>(static_cast<void*>(hb_ + p.off)); }  // kPageable only
    void upload() {
        for (int i = 0; i < n_copies; ++i) {
            const Copy& p = copies[i];
            if (!p.src) continue;
            if (hb_) std::memcpy(hb_ + p.off, p.src, p.bytes);
            else copy(db_ + p.off, p.src, p.bytes, hipMemcpyHostToDevice);
        }
        if (hb_) copy(db_, hb_, in_end, hipMemcpyHostToDevice);
    }
    // one piece now, whatever its declared direction (mid-call round trips through the host)
    template <class T>
    void put(svo::Slot<T> p, const T* src) { copy(db_ + p.off, src, p.count * sizeof(T), hipMemcpyHostToDevice); }
    template <class T>
    void get(T* dst, svo::Slot<T> p) { copy(dst, db_ + p.off, p.count * sizeof(T), hipMemcpyDeviceToHost); }
    template <class T>
    void zero(svo::Slot<T> p) {
        if (ok()) err = hipMemsetAsync(db_ + p.off, 0, p.count * sizeof(T), s_);
    }
    template <class F>
    void launch(F&& kernels) {
        if (!ok()) return;
        kernels();
        err = hipGetLastError();
    }
    void sync() {
        if (ok()) err = hipStreamSynchronize(s_);
    }
    void finish() {  // the outputs to their host arrays, after the stream's work
        if (hb_) copy(hb_ + out_begin, db_ + out_begin, out_end - out_begin, hipMemcpyDeviceToHost);
        for (int i = 0; i < n_copies; ++i)
            if (!hb_ && copies[i].dst) copy(copies[i].dst, db_ + copies[i].off, copies[i].bytes, hipMemcpyDeviceToHost);
        sync();
        if (!hb_ || !ok()) return;
        for (int i = 0; i < n_copies; ++i)
            if (copies[i].dst) std::memcpy(copies[i].dst, hb_ + copies[i].off, copies[i].bytes);
    }
    template <class F>
    void run(F&& kernels) {  // the whole of a call that has one launch point
        upload();
        launch(kernels);
        finish();
    }
  private:
    svo_ctx* c_;
    hipStream_t s_;
    char *db_ = nullptr, *hb_ = nullptr;  // the device block; the staging block (staged strategy)
    std::vector<char> pageable_;
    void copy(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
        if (ok()) err = stage_copy(c_, dst, src, bytes, kind, s_);
    }
};
}  // namespace svo::shim
#pragma GCC visibility pop

