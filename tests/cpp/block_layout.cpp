// block_layout.cpp — csrc/block_layout.h against the offsets the entry points wrote out by hand before it existed.
// Each case declares an entry point's pieces as its capi_<stage>.hip does; the expected numbers are worked out by
// hand from the former expressions (pieces rounded up to 8 bytes, in declaration order), quoted in the comments.
// Host-only: build with g++ -std=c++17 -I<csrc>.
#include <cstdint>
#include <cstdio>

#include "block_layout.h"

static int g_bad = 0;
#define EXPECT(got, want)                                                                                    \
    do {                                                                                                     \
        const long long g_ = (long long)(got), w_ = (long long)(want);                                       \
        if (g_ != w_) { std::printf("%s:%d: %s = %lld, expected %lld\n", __FILE__, __LINE__, #got, g_, w_); ++g_bad; } \
    } while (0)

static bool copies_at(const svo::BlockLayout& b, size_t off) {
    for (int i = 0; i < b.n_copies; ++i)
        if (b.copies[i].off == off) return true;
    return false;
}

// the pointers a kernel argument block would hold
static const int32_t* ci32;
static const int64_t* ci64;
static const double* cf64;
static const uint8_t* cu8;
static int32_t* i32;
static double* f64;
static uint8_t* u8;
// host arrays
static int32_t h_i32[64];
static int64_t h_i64[8];
static double h_f64[64];
static uint8_t h_u8[8];

// svo_klt_track: take((P + 1) * 4), take(P * 8), take(N * 16), take(N * 16), take(N), take(trace ? N * L * 8 : 0)
static void klt(size_t P, size_t N, size_t L, bool with_trace, const size_t (&want)[7], int want_copies) {
    svo::BlockLayout b;
    const auto d_off = b.in(&ci32, h_i32, P + 1);
    const auto d_fr = b.in(&ci32, h_i32, P * 2);
    const auto d_rpx = b.in(&cf64, h_f64, N * 2);
    const auto d_cpx = b.inout(&f64, h_f64, N * 2);
    const auto d_st = b.out(&u8, h_u8, N);
    const auto d_tr = b.out(&i32, with_trace ? h_i32 : nullptr, with_trace ? N * L * 2 : 0);
    EXPECT(d_off.off, want[0]);
    EXPECT(d_fr.off, want[1]);
    EXPECT(d_rpx.off, want[2]);
    EXPECT(d_cpx.off, want[3]);
    EXPECT(d_st.off, want[4]);
    EXPECT(d_tr.off, want[5]);
    EXPECT(b.total, want[6]);
    EXPECT(b.n_binds, 6);
    EXPECT(b.binds[3].field == &f64 && b.binds[3].off == d_cpx.off, 1);
    EXPECT(b.n_copies, want_copies);
    EXPECT(copies_at(b, d_tr.off), with_trace);
    // cur_px goes up and comes back from the same piece; the status bytes are copied unrounded
    for (int i = 0; i < b.n_copies; ++i) {
        if (b.copies[i].off == d_cpx.off) EXPECT(b.copies[i].src == h_f64 && b.copies[i].dst == h_f64, 1);
        if (b.copies[i].off == d_st.off) EXPECT(b.copies[i].bytes, N);
    }
}

// svo_bundle_adjust at NP = 1, NF = 2, NX = 1, NO = 2, one table of 2 x 1 entries, trace null
static void bundle_adjust() {
    const size_t NP = 1, NF = 2, NX = 1, NO = 2, TAB = 2;
    double* trace = nullptr;
    svo::BlockLayout b;
    const size_t got[] = {
        b.in(&ci32, h_i32, NP + 1).off,   // frame_off  take((NP + 1) * 4) = 8
        b.in(&ci32, h_i32, NP + 1).off,   // point_off  8
        b.in(&ci32, h_i32, NP + 1).off,   // obs_off    8
        b.in(&ci32, h_i32, NX + 1).off,   // pobs       take((NX + 1) * 4) = 8
        b.in(&ci64, h_i64, NP + 1).off,   // tab_off    take((NP + 1) * 8) = 16
        b.inout(&f64, h_f64, NF * 7).off, // poses      take(NF * 56) = 112
        b.in(&ci32, h_i32, NF).off,       // ridx       take(NF * 4) = 8
        b.inout(&f64, h_f64, NX * 3).off, // points     take(NX * 24) = 24
        b.in(&ci32, h_i32, NO).off,       // obs_frame  take(NO * 4) = 8
        b.in(&cf64, h_f64, NO * 2).off,   // obs_px     take(NO * 16) = 32
        b.dev(&i32, TAB).off,             // tab        take(2 * 4) = 8
        b.dev(&f64, NO * 15).off,         // edge       take(NO * 120) = 240
        b.dev(&f64, NO * 18).off,         // W          take(NO * 144) = 288
        b.dev(&f64, NX * 9).off,          // Vg         take(NX * 72) = 72
        b.dev(&f64, NX * 6).off,          // Vi         take(NX * 48) = 48
        b.dev(&f64, NX * 3).off,          // dx         24
        b.dev(&f64, NX * 3).off,          // Xt         24
        b.out(&f64, h_f64, NO).off,       // obs_chi2   take(NO * 8) = 16
        b.out(&f64, h_f64, NP).off,       // init_chi   8
        b.out(&f64, h_f64, NP).off,       // final_chi  8
        b.out(&i32, h_i32, NP).off,       // iterations take(NP * 4) = 8
        b.out(&i32, h_i32, NP).off,       // status     8
        b.out(&f64, trace, 0).off,        // trace      take(0): takes no room
    };
    const size_t want[] = {0, 8, 16, 24, 32, 48, 160, 168, 192, 200, 232, 240, 480, 768, 840, 888, 912, 936, 952, 960, 968,
                           976, 984};
    for (int i = 0; i < 23; ++i) EXPECT(got[i], want[i]);
    EXPECT(b.total, 984);    // the empty trace piece moved nothing ...
    EXPECT(b.n_copies, 15);  // ... and is no copy: 10 pieces up (2 of them also down), 5 more down
    EXPECT(copies_at(b, 984), 0);
    EXPECT(b.n_binds, 23);
}

// svo_pose_optimize at F = 1, N = 3: r8((F + 1) * 4) | F * 56 | N * 24 | N * 24 | r8(N) | r8(N) = in_end,
// F * 56 | F * 8 | r8(F * 4) | r8(N) = out_end, N * 24 | N * 8 = total
static void pose_optimize() {
    const size_t F = 1, N = 3;
    svo::BlockLayout b;
    const size_t got[] = {b.in(&ci32, h_i32, F + 1).off, b.in(&cf64, h_f64, F * 7).off, b.in(&cf64, h_f64, N * 3).off,
                          b.in(&cf64, h_f64, N * 3).off, b.in(&cu8, h_u8, N).off,       b.in(&cu8, h_u8, N).off,
                          b.out(&f64, h_f64, F * 7).off, b.out(&f64, h_f64, F).off,     b.out(&i32, h_i32, F).off,
                          b.out(&u8, h_u8, N).off,       b.dev(&f64, N * 3).off,        b.dev(&f64, N).off};
    const size_t want[] = {0, 8, 64, 136, 208, 216, 224, 280, 288, 296, 304, 376};
    for (int i = 0; i < 12; ++i) EXPECT(got[i], want[i]);
    EXPECT(b.in_end, 224);
    EXPECT(b.out_begin, 224);
    EXPECT(b.out_end, 304);
    EXPECT(b.total, 400);
    EXPECT(b.n_copies, 10);
}

// feature_align_impl at n = 3: in_bytes = n * 40, out_off = n * 24, total = n * 56 (status keeps 8 bytes per candidate)
static void feature_align() {
    const size_t n = 3;
    static const uint8_t* h_planes[4];
    static const uint8_t* const* planes;
    svo::BlockLayout b;
    EXPECT(b.in(&planes, h_planes, n).off, 0);
    EXPECT(b.in(&cf64, h_f64, 2 * n).off, 24);
    EXPECT(b.inout(&f64, h_f64, 2 * n).off, 72);
    EXPECT(b.out(&f64, nullptr, n).off, 120);  // err not asked for: room, no copy
    EXPECT(b.out(&i32, h_i32, n, 2 * n).off, 144);
    EXPECT(b.in_end, 120);
    EXPECT(b.out_begin, 72);
    EXPECT(b.out_end, 168);
    EXPECT(b.total, 168);
    EXPECT(b.n_copies, 4);
    EXPECT(b.copies[3].bytes, 12);
}

// a piece past the capacity is dropped and flagged (Block::alloc then fails): nothing is written past the tables
static void capacity() {
    svo::BlockLayout b;
    for (int i = 0; i < svo::BlockLayout::kMaxPieces; ++i) b.inout(&f64, h_f64, 1);
    EXPECT(b.overflow, 0);
    EXPECT(b.in(&cf64, h_f64, 1).count, 0);
    EXPECT(b.overflow, 1);
    EXPECT(b.n_binds, svo::BlockLayout::kMaxPieces);
    EXPECT(b.n_copies, svo::BlockLayout::kMaxPieces);
}

int main() {
    capacity();
    //            feat_off frames ref_px cur_px status trace total
    klt(1, 1, 4, false, {0, 8, 16, 32, 48, 56, 56}, 5);
    klt(1, 1, 4, true, {0, 8, 16, 32, 48, 56, 88}, 6);        // trace: 1 * 4 * 8 = 32
    klt(3, 5, 3, false, {0, 16, 40, 120, 200, 208, 208}, 5);  // status: take(5) = 8
    klt(3, 5, 3, true, {0, 16, 40, 120, 200, 208, 328}, 6);   // trace: 5 * 3 * 8 = 120
    bundle_adjust();
    pose_optimize();
    feature_align();
    if (g_bad) return 1;
    std::printf("ok\n");
    return 0;
}
