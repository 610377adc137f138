// bundle_adjust.hip — windowed bundle adjustment (BundleAdjustment::twoViewBA / localBA,
// src/bundle_adjustment.cpp:397-625) for a batch of independent problems.
//
// The cost, the Levenberg-Marquardt schedule and the outputs are this project's contract (include/svo_c.h,
// svo_bundle_adjust), modelled on g2o's OptimizationAlgorithmLevenberg and not pinned to g2o; the per-edge
// arithmetic is bundle_adjust_math.h.
//   ba_structure_kernel  one lane per point: the whole per-point LM with every pose held (StructureOnlySolver<3>,
//                        :556-564).  No reduction, no synchronisation.
//   ba_joint_kernel      one 256-thread workgroup per problem runs the whole schedule on the device:
//     linearise   lanes stride over points and walk each point's contiguous observation block: V_j, g_j in
//                 registers, J_p / e / w and W_ij = w J_p^T J_x per observation to scratch;
//     U_i, b_i    one thread per (free frame, entry) sums over the points in ascending order through the
//                 frames x points observation table;
//     Schur       one thread per entry of S = U + lambda I - sum_j W_j (V_j + lambda I)^-1 W_j^T (packed lower
//                 triangle in LDS) and of rhs = b - sum_j W_j (V_j + lambda I)^-1 g_j, points ascending;
//     solve       right-looking Cholesky of S in LDS by the workgroup (a non-positive pivot fails the trial),
//                 column-oriented substitutions, dx_j per point;
//     trial       poses and points of the trial in copies, the robust chi by a fixed tree over the per-thread
//                 sums; every thread evaluates the same accept / reject expression on the same LDS values.
// Every sum has an order fixed by the problem's layout and no floating-point atomics are used, so equal inputs
// give equal bytes.
// Bound: latency (one workgroup per problem, dependent phases separated by barriers); the batch is the parallelism.
#include "bundle_adjust_math.h"
#include "svo_internal.h"

namespace svo {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxF = SVO_BA_MAX_FRAMES;  // free frames of a problem; fixed frames are not limited
constexpr int kMaxN = 6 * kMaxF;
constexpr int kFailLimit = 5;  // trials after a failure (setMaxTrialsAfterFailure(5), :330)

__device__ __forceinline__ V3 ld3(const double* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ int tri(int r, int c) { return r * (r + 1) / 2 + c; }  // c <= r
__device__ __forceinline__ int sym6(int a, int b) {  // index of (a, b) in the 21 upper-triangle entries
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo * 6 - lo * (lo - 1) / 2 + (hi - lo);
}

// the sums of a and b over the workgroup by a fixed tree; every thread returns both
__device__ void block_sum2(double& a, double& b, double (*red)[kThreads]) {
    __syncthreads();
    red[0][threadIdx.x] = a;
    red[1][threadIdx.x] = b;
    __syncthreads();
    for (int s = kThreads / 2; s >= 1; s >>= 1) {
        if ((int)threadIdx.x < s) {
            red[0][threadIdx.x] += red[0][threadIdx.x + s];
            red[1][threadIdx.x] += red[1][threadIdx.x + s];
        }
        __syncthreads();
    }
    a = red[0][0];
    b = red[1][0];
}

// ---------------------------------------------------------------- structure only
__global__ void __launch_bounds__(kThreads) ba_structure_kernel(BundleAdjustArgs a) {
    const int p = blockIdx.x;
    const int32_t P = a.point_off[p + 1] - a.point_off[p];
    const int j = blockIdx.y * kThreads + threadIdx.x;
    if (j >= P) return;
    const int64_t gj = (int64_t)a.point_off[p] + j;
    const int32_t o0 = a.pobs_off[gj], o1 = a.pobs_off[gj + 1];
    const double* poses = a.poses + 7 * (int64_t)a.frame_off[p];
    V3 X = ld3(a.points + 3 * gj);
    double lambda = 0.0, nu = 2.0;
    for (int it = 0; it < a.structure_iterations; ++it) {
        double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        V3 g{0.0, 0.0, 0.0};
        double cur = 0.0;
        for (int32_t o = o0; o < o1; ++o) {
            const BAPose T = ba_pose(poses + 7 * a.obs_frame[o]);
            const V3 c = ba_transform(T, X);
            const BAEdge e = ba_edge(c, a.f, a.cx, a.cy, a.obs_px[2 * (int64_t)o], a.obs_px[2 * (int64_t)o + 1], a.delta);
            double Jp[2][6], Jx[2][3];
            ba_jacobians(T, c, a.f, Jp, Jx);
            cur += e.rho;
            V[0] += e.w * (Jx[0][0] * Jx[0][0] + Jx[1][0] * Jx[1][0]);
            V[1] += e.w * (Jx[0][0] * Jx[0][1] + Jx[1][0] * Jx[1][1]);
            V[2] += e.w * (Jx[0][0] * Jx[0][2] + Jx[1][0] * Jx[1][2]);
            V[3] += e.w * (Jx[0][1] * Jx[0][1] + Jx[1][1] * Jx[1][1]);
            V[4] += e.w * (Jx[0][1] * Jx[0][2] + Jx[1][1] * Jx[1][2]);
            V[5] += e.w * (Jx[0][2] * Jx[0][2] + Jx[1][2] * Jx[1][2]);
            g.x += e.w * (Jx[0][0] * e.ex + Jx[1][0] * e.ey);
            g.y += e.w * (Jx[0][1] * e.ex + Jx[1][1] * e.ey);
            g.z += e.w * (Jx[0][2] * e.ex + Jx[1][2] * e.ey);
        }
        if (it == 0) lambda = 1e-5 * fmax(V[0], fmax(V[3], V[5]));
        bool accepted = false;
        for (int q = 0; q < kFailLimit && !accepted; ++q) {
            double Vi[6];
            const bool ok = ba_sym3_inverse(V, lambda, Vi);
            double r = 0.0;
            V3 Xn = X;
            bool fin = false;
            if (ok) {
                const V3 d = ba_sym3_mul(Vi, g);
                Xn = v3add(X, d);
                double tmp = 0.0;
                for (int32_t o = o0; o < o1; ++o) {
                    const BAPose T = ba_pose(poses + 7 * a.obs_frame[o]);
                    const BAEdge e = ba_edge(ba_transform(T, Xn), a.f, a.cx, a.cy, a.obs_px[2 * (int64_t)o],
                                             a.obs_px[2 * (int64_t)o + 1], a.delta);
                    tmp += e.rho;
                }
                const double scale = (d.x * (lambda * d.x + g.x) + d.y * (lambda * d.y + g.y) + d.z * (lambda * d.z + g.z)) + 1e-3;
                r = (cur - tmp) / scale;
                fin = isfinite(tmp);
            }
            if (ok && fin && r > 0.0) {
                X = Xn;
                lambda *= ba_lambda_factor(r);
                nu = 2.0;
                accepted = true;
            } else {
                lambda *= nu;
                nu *= 2.0;
            }
        }
        if (!accepted) break;
    }
    a.points[3 * gj] = X.x;
    a.points[3 * gj + 1] = X.y;
    a.points[3 * gj + 2] = X.z;
}

// ---------------------------------------------------------------- joint
struct JointShared {
    double S[kMaxN * (kMaxN + 1) / 2];  // packed lower triangle of the reduced system, then its Cholesky factor
    double U[kMaxF][21];
    double b[kMaxN];
    double x[kMaxN];                    // rhs, then dp
    double pose[2][kMaxF][7];           // of the free frames, by reduced index: [0] the estimate, [1] the trial
    BAPose T[2][kMaxF];
    double red[2][kThreads];
    int32_t fre[kMaxF];                 // frame of a reduced index
    int32_t flag;
};

// the transform of frame i: a free frame's from LDS (estimate or trial), a fixed frame's from its pose as given (it
// never changes; the same ba_pose on the same seven doubles, so the same bits wherever it is formed)
__device__ __forceinline__ BAPose frame_T(const JointShared& sh, const int32_t* ridx, const double* gposes, int which,
                                          int i) {
    const int32_t r = ridx[i];
    return r >= 0 ? sh.T[which][r] : ba_pose(gposes + 7 * (int64_t)i);
}

// the robust chi of the problem at T[which] / X; also sums `extra` (returned in it)
__device__ double robust_chi(const BundleAdjustArgs& a, JointShared& sh, const int32_t* ridx, const double* gposes,
                             int which, const double* X, int32_t P, const int32_t* pobs, int32_t obase,
                             const int32_t* of, const double* px, double& extra) {
    double part = 0.0;
    for (int j = threadIdx.x; j < P; j += kThreads) {
        const V3 Xj = ld3(X + 3 * (int64_t)j);
        for (int32_t o = pobs[j] - obase; o < pobs[j + 1] - obase; ++o) {
            const BAEdge e = ba_edge(ba_transform(frame_T(sh, ridx, gposes, which, of[o]), Xj), a.f, a.cx, a.cy, px[2 * (int64_t)o],
                                     px[2 * (int64_t)o + 1], a.delta);
            part += e.rho;
        }
    }
    block_sum2(part, extra, sh.red);
    return part;
}

__global__ void __launch_bounds__(kThreads) ba_joint_kernel(BundleAdjustArgs a) {
    __shared__ JointShared sh;
    const int p = blockIdx.x;
    const int tid = threadIdx.x;
    const int32_t F = a.frame_off[p + 1] - a.frame_off[p];
    const int32_t P = a.point_off[p + 1] - a.point_off[p];
    const int32_t obase = a.obs_off[p];
    double* trace = a.trace ? a.trace + (int64_t)p * SVO_BA_TRACE_CAP * 6 : nullptr;
    if (trace)
        for (int i = tid; i < SVO_BA_TRACE_CAP * 6; i += kThreads) trace[i] = (i % 6 == 0) ? -1.0 : 0.0;
    if (P == 0 || F == 0) {  // nothing to adjust: the poses stay as given
        if (tid == 0) {
            a.init_chi[p] = 0.0;
            a.final_chi[p] = 0.0;
            a.iterations[p] = 0;
            a.status[p] = -1;
        }
        return;
    }
    double* gposes = a.poses + 7 * (int64_t)a.frame_off[p];
    const int32_t* ridx = a.ridx + a.frame_off[p];  // reduced index of a frame, -1 when fixed (built by the host)
    const int64_t pbase = a.point_off[p];
    double* X = a.points + 3 * pbase;
    double* Xt = a.Xt + 3 * pbase;
    double* dxp = a.dx + 3 * pbase;
    double* Vg = a.Vg + 9 * pbase;
    double* Vinv = a.Vi + 6 * pbase;
    const int32_t* pobs = a.pobs_off + pbase;
    const int32_t* of = a.obs_frame + obase;
    const double* px = a.obs_px + 2 * (int64_t)obase;
    double* edge = a.edge + 15 * (int64_t)obase;
    double* W = a.W + 18 * (int64_t)obase;
    int32_t* tab = a.tab + a.tab_off[p];

    // ---- layout: reduced indices, the frames x points table, the poses
    if (tid == 0) {
        int n = 0;
        for (int i = 0; i < F; ++i)
            if (ridx[i] >= 0) sh.fre[n++] = i;  // (ridx counts the free frames in order: ridx[i] == n here)
        sh.flag = n;
    }
    for (int64_t i = tid; i < (int64_t)F * P; i += kThreads) tab[i] = -1;
    __syncthreads();
    const int nfree = sh.flag;
    const int n = 6 * nfree;
    if (tid < nfree) {
        for (int k = 0; k < 7; ++k) sh.pose[0][tid][k] = gposes[7 * sh.fre[tid] + k];
        sh.T[0][tid] = ba_pose(sh.pose[0][tid]);
    }
    for (int j = tid; j < P; j += kThreads)
        for (int32_t o = pobs[j] - obase; o < pobs[j + 1] - obase; ++o) tab[(int64_t)j * F + of[o]] = o;
    __syncthreads();

    double zero = 0.0;
    double cur = robust_chi(a, sh, ridx, gposes, 0, X, P, pobs, obase, of, px, zero);
    if (tid == 0) a.init_chi[p] = cur;
    double lambda = 0.0, nu = 2.0;
    int32_t iters = 0, status = 0, ntrace = 0;

    for (int it = 0; it < a.max_iterations && status == 0; ++it) {
        // ---- linearise at the estimate
        double vmax = 0.0;
        for (int j = tid; j < P; j += kThreads) {
            const V3 Xj = ld3(X + 3 * (int64_t)j);
            double V[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            V3 g{0.0, 0.0, 0.0};
            for (int32_t o = pobs[j] - obase; o < pobs[j + 1] - obase; ++o) {
                const int i = of[o];
                const BAPose Ti = frame_T(sh, ridx, gposes, 0, i);
                const V3 c = ba_transform(Ti, Xj);
                const BAEdge e = ba_edge(c, a.f, a.cx, a.cy, px[2 * (int64_t)o], px[2 * (int64_t)o + 1], a.delta);
                double Jp[2][6], Jx[2][3];
                ba_jacobians(Ti, c, a.f, Jp, Jx);
                V[0] += e.w * (Jx[0][0] * Jx[0][0] + Jx[1][0] * Jx[1][0]);
                V[1] += e.w * (Jx[0][0] * Jx[0][1] + Jx[1][0] * Jx[1][1]);
                V[2] += e.w * (Jx[0][0] * Jx[0][2] + Jx[1][0] * Jx[1][2]);
                V[3] += e.w * (Jx[0][1] * Jx[0][1] + Jx[1][1] * Jx[1][1]);
                V[4] += e.w * (Jx[0][1] * Jx[0][2] + Jx[1][1] * Jx[1][2]);
                V[5] += e.w * (Jx[0][2] * Jx[0][2] + Jx[1][2] * Jx[1][2]);
                g.x += e.w * (Jx[0][0] * e.ex + Jx[1][0] * e.ey);
                g.y += e.w * (Jx[0][1] * e.ex + Jx[1][1] * e.ey);
                g.z += e.w * (Jx[0][2] * e.ex + Jx[1][2] * e.ey);
                if (ridx[i] >= 0) {
                    double* ed = edge + 15 * (int64_t)o;
                    double* w = W + 18 * (int64_t)o;
                    for (int k = 0; k < 6; ++k) {
                        ed[k] = Jp[0][k];
                        ed[6 + k] = Jp[1][k];
                        for (int m = 0; m < 3; ++m) w[3 * k + m] = e.w * (Jp[0][k] * Jx[0][m] + Jp[1][k] * Jx[1][m]);
                    }
                    ed[12] = e.ex;
                    ed[13] = e.ey;
                    ed[14] = e.w;
                }
            }
            double* vg = Vg + 9 * (int64_t)j;
            for (int k = 0; k < 6; ++k) vg[k] = V[k];
            vg[6] = g.x; vg[7] = g.y; vg[8] = g.z;
            vmax = fmax(vmax, fmax(V[0], fmax(V[3], V[5])));
        }
        __syncthreads();
        // ---- U_i (21 entries) and b_i (6) of every free frame, points ascending
        for (int idx = tid; idx < nfree * 27; idx += kThreads) {
            const int fi = idx / 27, en = idx % 27, i = sh.fre[fi];
            int ea = 0, eb = 0;
            if (en < 21) {
                int t = en;
                while (t >= 6 - ea) { t -= 6 - ea; ++ea; }
                eb = ea + t;
            }
            double acc = 0.0;
            for (int j = 0; j < P; ++j) {
                const int32_t o = tab[(int64_t)j * F + i];
                if (o < 0) continue;
                const double* ed = edge + 15 * (int64_t)o;
                if (en < 21) acc += ed[14] * (ed[ea] * ed[eb] + ed[6 + ea] * ed[6 + eb]);
                else acc += ed[14] * (ed[en - 21] * ed[12] + ed[6 + en - 21] * ed[13]);
            }
            if (en < 21) sh.U[fi][en] = acc;
            else sh.b[6 * fi + en - 21] = acc;
        }
        __syncthreads();
        if (it == 0) {  // lambda = 1e-5 * max diag(H) at the first linearisation
            // (a maximum is exact in any order)
            __syncthreads();
            sh.red[0][tid] = vmax;
            __syncthreads();
            for (int s = kThreads / 2; s >= 1; s >>= 1) {
                if (tid < s) sh.red[0][tid] = fmax(sh.red[0][tid], sh.red[0][tid + s]);
                __syncthreads();
            }
            double mx = sh.red[0][0];
            for (int fi = 0; fi < nfree; ++fi)
                for (int k = 0; k < 6; ++k) mx = fmax(mx, sh.U[fi][sym6(k, k)]);
            lambda = 1e-5 * mx;
            __syncthreads();
        }
        // ---- trials
        bool accepted = false;
        for (int q = 0; q < kFailLimit && !accepted; ++q) {
            __syncthreads();
            if (tid == 0) sh.flag = 1;
            __syncthreads();
            for (int j = tid; j < P; j += kThreads)
                if (!ba_sym3_inverse(Vg + 9 * (int64_t)j, lambda, Vinv + 6 * (int64_t)j)) sh.flag = 0;
            __syncthreads();
            bool ok = sh.flag != 0;
            if (ok) {
                // Schur complement: 6 x 6 blocks (fi >= fk), one thread per entry
                const int nblk = nfree * (nfree + 1) / 2;
                for (int idx = tid; idx < nblk * 36; idx += kThreads) {
                    int blk = idx / 36, fi = 0;
                    while (blk > fi) { blk -= fi + 1; ++fi; }
                    const int fk = blk, ra = (idx % 36) / 6, cb = idx % 6;
                    const int r = 6 * fi + ra, c = 6 * fk + cb;
                    if (c > r) continue;
                    const int i = sh.fre[fi], k = sh.fre[fk];
                    double s = fi == fk ? sh.U[fi][sym6(ra, cb)] : 0.0;
                    if (r == c) s += lambda;
                    for (int j = 0; j < P; ++j) {
                        const int32_t oi = tab[(int64_t)j * F + i];
                        if (oi < 0) continue;
                        const int32_t ok2 = fi == fk ? oi : tab[(int64_t)j * F + k];
                        if (ok2 < 0) continue;
                        const double* wi = W + 18 * (int64_t)oi + 3 * ra;
                        const double* wk = W + 18 * (int64_t)ok2 + 3 * cb;
                        const V3 y = ba_sym3_mul(Vinv + 6 * (int64_t)j, {wi[0], wi[1], wi[2]});
                        s -= y.x * wk[0] + y.y * wk[1] + y.z * wk[2];
                    }
                    sh.S[tri(r, c)] = s;
                }
                for (int r = tid; r < n; r += kThreads) {
                    const int i = sh.fre[r / 6];
                    double s = sh.b[r];
                    for (int j = 0; j < P; ++j) {
                        const int32_t oi = tab[(int64_t)j * F + i];
                        if (oi < 0) continue;
                        const double* wi = W + 18 * (int64_t)oi + 3 * (r % 6);
                        const V3 y = ba_sym3_mul(Vinv + 6 * (int64_t)j, {wi[0], wi[1], wi[2]});
                        const double* vg = Vg + 9 * (int64_t)j;
                        s -= y.x * vg[6] + y.y * vg[7] + y.z * vg[8];
                    }
                    sh.x[r] = s;
                }
                __syncthreads();
                // Cholesky of S, right-looking, in place
                const int tr = tid / 16, tc = tid % 16;
                for (int k = 0; k < n && ok; ++k) {
                    const double d = sh.S[tri(k, k)];
                    if (!(d > 0.0)) { ok = false; break; }  // (every thread reads the same value)
                    const double l = sqrt(d);
                    __syncthreads();
                    if (tid == 0) sh.S[tri(k, k)] = l;
                    for (int r = k + 1 + tid; r < n; r += kThreads) sh.S[tri(r, k)] /= l;
                    __syncthreads();
                    for (int r = k + 1 + tr; r < n; r += 16) {
                        const double lr = sh.S[tri(r, k)];
                        for (int c = k + 1 + tc; c <= r; c += 16) sh.S[tri(r, c)] -= lr * sh.S[tri(c, k)];
                    }
                    __syncthreads();
                }
            }
            double tmp = cur, r = 0.0;
            if (ok) {
                // L y = rhs, L^T dp = y
                for (int k = 0; k < n; ++k) {
                    __syncthreads();
                    if (tid == 0) sh.x[k] /= sh.S[tri(k, k)];
                    __syncthreads();
                    const double xk = sh.x[k];
                    for (int rr = k + 1 + tid; rr < n; rr += kThreads) sh.x[rr] -= sh.S[tri(rr, k)] * xk;
                }
                for (int k = n - 1; k >= 0; --k) {
                    __syncthreads();
                    if (tid == 0) sh.x[k] /= sh.S[tri(k, k)];
                    __syncthreads();
                    const double xk = sh.x[k];
                    for (int rr = tid; rr < k; rr += kThreads) sh.x[rr] -= sh.S[tri(k, rr)] * xk;
                }
                __syncthreads();
                // the trial's poses
                if (tid < nfree) {
                    const SE3 Tn = se3_compose(se3_exp(&sh.x[6 * tid]), se3_load(sh.pose[0][tid]));
                    se3_store(Tn, sh.pose[1][tid]);
                    sh.T[1][tid] = ba_pose(sh.pose[1][tid]);
                }
                // the trial's points: dx_j = (V_j + lambda I)^-1 (g_j - sum_i W_ij^T dp_i)
                double sc = 0.0;
                for (int j = tid; j < P; j += kThreads) {
                    const double* vg = Vg + 9 * (int64_t)j;
                    V3 h{vg[6], vg[7], vg[8]};
                    for (int32_t o = pobs[j] - obase; o < pobs[j + 1] - obase; ++o) {
                        const int ri = ridx[of[o]];
                        if (ri < 0) continue;
                        const double* w = W + 18 * (int64_t)o;
                        for (int k = 0; k < 6; ++k) {
                            const double d = sh.x[6 * ri + k];
                            h.x -= w[3 * k] * d;
                            h.y -= w[3 * k + 1] * d;
                            h.z -= w[3 * k + 2] * d;
                        }
                    }
                    const V3 d = ba_sym3_mul(Vinv + 6 * (int64_t)j, h);
                    dxp[3 * (int64_t)j] = d.x; dxp[3 * (int64_t)j + 1] = d.y; dxp[3 * (int64_t)j + 2] = d.z;
                    Xt[3 * (int64_t)j] = X[3 * (int64_t)j] + d.x;
                    Xt[3 * (int64_t)j + 1] = X[3 * (int64_t)j + 1] + d.y;
                    Xt[3 * (int64_t)j + 2] = X[3 * (int64_t)j + 2] + d.z;
                    sc += d.x * (lambda * d.x + vg[6]) + d.y * (lambda * d.y + vg[7]) + d.z * (lambda * d.z + vg[8]);
                }
                __syncthreads();
                tmp = robust_chi(a, sh, ridx, gposes, 1, Xt, P, pobs, obase, of, px, sc);
                double scale = 0.0;
                for (int k = 0; k < n; ++k) scale += sh.x[k] * (lambda * sh.x[k] + sh.b[k]);
                scale = (scale + sc) + 1e-3;
                r = (cur - tmp) / scale;
            }
            const bool acc = ok && r > 0.0 && isfinite(tmp);
            if (trace && tid == 0 && ntrace < SVO_BA_TRACE_CAP) {
                double* t = trace + 6 * ntrace;
                t[0] = it; t[1] = q; t[2] = acc ? 1.0 : 0.0; t[3] = lambda; t[4] = r; t[5] = tmp;
            }
            ++ntrace;
            if (acc) {
                __syncthreads();
                for (int j = tid; j < P; j += kThreads)
                    for (int k = 0; k < 3; ++k) X[3 * (int64_t)j + k] = Xt[3 * (int64_t)j + k];
                if (tid < nfree) {
                    for (int k = 0; k < 7; ++k) sh.pose[0][tid][k] = sh.pose[1][tid][k];
                    sh.T[0][tid] = sh.T[1][tid];
                }
                __syncthreads();
                cur = tmp;
                lambda *= ba_lambda_factor(r);
                nu = 2.0;
                ++iters;
                accepted = true;
            } else {
                lambda *= nu;
                nu *= 2.0;
            }
        }
        if (!accepted) status = 1;
    }
    __syncthreads();
    // ---- outputs: the non-robust e2 of every edge at the final estimate, the poses, the sums
    for (int j = tid; j < P; j += kThreads) {
        const V3 Xj = ld3(X + 3 * (int64_t)j);
        for (int32_t o = pobs[j] - obase; o < pobs[j + 1] - obase; ++o) {
            const BAEdge e = ba_edge(ba_transform(frame_T(sh, ridx, gposes, 0, of[o]), Xj), a.f, a.cx, a.cy,
                                     px[2 * (int64_t)o], px[2 * (int64_t)o + 1], a.delta);
            a.obs_chi2[obase + o] = e.e2;
        }
    }
    if (tid < nfree)
        for (int k = 0; k < 7; ++k) gposes[7 * sh.fre[tid] + k] = sh.pose[0][tid][k];
    if (tid == 0) {
        a.final_chi[p] = cur;
        a.iterations[p] = iters;
        a.status[p] = status;
    }
}

}  // namespace

void launch_ba_structure(const BundleAdjustArgs& a, hipStream_t s) {
    if (a.n_problems > 0 && a.max_points > 0 && a.structure_iterations > 0)
        hipLaunchKernelGGL(ba_structure_kernel, dim3(a.n_problems, (a.max_points + kThreads - 1) / kThreads),
                           dim3(kThreads), 0, s, a);
}

void launch_ba_joint(const BundleAdjustArgs& a, hipStream_t s) {
    if (a.n_problems > 0) hipLaunchKernelGGL(ba_joint_kernel, dim3(a.n_problems), dim3(kThreads), 0, s, a);
}

}  // namespace svo
