// two_view.hip — two-view map initialisation (System::processSecondFrame, src/system.cpp:144-223) for a batch of
// frame pairs: algorithm::sampsonCorrection (src/algorithm.cpp:173-237), recoverPose (:261-333) over
// triangulate3DWorldPoints / triangulatePointDLT (:553-566, :655-680), the depth rescaling and the validity test.
//
// One 256-thread workgroup per frame pair, lanes striding the pair's matches (the same lane owns the same match in
// every phase, so a phase reads back what the lane itself wrote).
//   two_view_vote_kernel    Sampson-corrects both pixel lists, triangulates every match under the four hypotheses
//                           (R1,+t) (R1,-t) (R2,+t) (R2,-t) as poses[i] * ref_pose (:297), counts the matches in front
//                           of both cameras (integer: ballot + popcount per wave, LDS over the waves), picks the first
//                           hypothesis with the strictly largest count (:318) and triangulates once more against
//                           poses[winner] alone (:329, :169-171): world point, current-camera point, its norm.
//   (host)                  median of the norms by std::nth_element (computeMedian, :813-832), scale, new translation.
//   two_view_finish_kernel  scales the current-camera points, maps them to the world with the rescaled pose
//                           (src/system.cpp:189-190), the validity flag (:201-202) and the stable compaction of the
//                           survivors (remove_if, :217-223), as depth_compact_kernel does for seeds.
//   triangulate_dlt_kernel  triangulate3DWorldPoints alone, for caller-given poses.
// Everything is fp64 without contraction; the per-match arithmetic is a few hundred flops on 32 bytes of pixels, so
// the kernels are bound by the dependent fp64 chains of the 3x3 LDLT, not by memory.
// The per-match arithmetic (Sampson, projection matrices, DLT, the 3x3 LDLT) is in two_view_math.h; the host half
// (F, the SVD of E, the angle-axis round trip, the median) is at the end of this file.
#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

#include "svo_internal.h"
#include "svo_math.h"
#include "two_view_math.h"

namespace svo {

namespace {

constexpr int kTvThreads = 256;
constexpr int kTvWaves = kTvThreads / 64;

__global__ void __launch_bounds__(kTvThreads) two_view_vote_kernel(TwoViewArgs a) {
    __shared__ int32_t wcnt[4][kTvWaves];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t off = a.feat_off[pair], n = a.feat_off[pair + 1] - off;
    double* rpx = a.ref_px + 2 * (int64_t)off;
    double* cpx = a.cur_px + 2 * (int64_t)off;
    // ---- algorithm::sampsonCorrection (src/algorithm.cpp:196-235), the reference's expressions term by term
    {
        double F[3][3];
        for (int i = 0; i < 9; ++i) F[i / 3][i % 3] = a.F[9 * (int64_t)pair + i];
        for (int i = tid; i < n; i += kTvThreads) {
            double px[4] = {rpx[2 * i], rpx[2 * i + 1], cpx[2 * i], cpx[2 * i + 1]};
            sampson_correct(F, px);
            rpx[2 * i] = px[0]; rpx[2 * i + 1] = px[1];
            cpx[2 * i] = px[2]; cpx[2 * i + 1] = px[3];
        }
    }
    // ---- algorithm::recoverPose (:291-323): the cheirality vote over the four hypotheses
    const SE3 Tref = se3_load(a.ref_poses + 7 * (int64_t)pair);
    const Proj P1 = make_proj(a.fx, a.fy, a.cx, a.cy, Tref);
    const double* hyp = a.hyp + 28 * (int64_t)pair;
#pragma unroll 1
    for (int h = 0; h < 4; ++h) {
        const SE3 Tc = se3_compose(se3_load(hyp + 7 * h), Tref);  // curFrame->m_absPose = poses[i] * ref (:297)
        const Proj P2 = make_proj(a.fx, a.fy, a.cx, a.cy, Tc);
        int32_t c = 0;
        for (int base = 0; base < n; base += kTvThreads) {  // uniform trip count: every lane reaches the ballot
            const int i = base + tid;
            bool front = false;
            if (i < n) {
                const V3 X = triangulate_dlt(P1, P2, rpx[2 * i], rpx[2 * i + 1], cpx[2 * i], cpx[2 * i + 1]);
                front = se3_act(Tref, X).z > 0 && se3_act(Tc, X).z > 0;  // (:311)
            }
            c += __popcll(__ballot(front));
        }
        if (lane == 0) wcnt[h][wave] = c;
    }
    __syncthreads();
    int32_t winner = -1, best = 0;
    for (int h = 0; h < 4; ++h) {
        int32_t c = 0;
        for (int w = 0; w < kTvWaves; ++w) c += wcnt[h][w];
        if (tid == 0) a.counts[4 * (int64_t)pair + h] = c;
        if (c > best) {  // cntProjected > numberProjected: the first strictly largest (:318)
            best = c;
            winner = h;
        }
    }
    if (tid == 0) a.winner[pair] = winner;
    if (winner < 0) return;  // recoverPose returns false: nothing past it runs (src/system.cpp:152-156)
    // ---- the winner's pose is poses[winner] alone, without the reference frame's pose (:329); the triangulation
    // of src/system.cpp:169-171 runs against it
    const SE3 Tw = se3_load(hyp + 7 * winner);
    if (tid == 0) se3_store(Tw, a.cur_pose + 7 * (int64_t)pair);
    const Proj P2 = make_proj(a.fx, a.fy, a.cx, a.cy, Tw);
    for (int i = tid; i < n; i += kTvThreads) {
        const V3 X = triangulate_dlt(P1, P2, rpx[2 * i], rpx[2 * i + 1], cpx[2 * i], cpx[2 * i + 1]);
        const V3 pc = se3_act(Tw, X);  // transferPointsWorldToCam (:568-577)
        const int64_t k = off + (int64_t)i;
        a.points_world[3 * k] = X.x; a.points_world[3 * k + 1] = X.y; a.points_world[3 * k + 2] = X.z;
        a.points_cur[3 * k] = pc.x; a.points_cur[3 * k + 1] = pc.y; a.points_cur[3 * k + 2] = pc.z;
        a.depth[k] = v3norm(pc);  // normalizedDepthCamera (:590-599)
    }
}

__global__ void __launch_bounds__(kTvThreads) two_view_finish_kernel(TwoViewArgs a) {
    __shared__ int32_t wsum[kTvWaves];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int32_t off = a.feat_off[pair], n = a.feat_off[pair + 1] - off;
    const double* rpx = a.ref_px + 2 * (int64_t)off;
    const double* cpx = a.cur_px + 2 * (int64_t)off;
    uint8_t* valid = a.valid + off;
    int32_t* survivor = a.survivor + off;
    if (a.winner[pair] < 0) {  // a failed pair creates no points
        for (int i = tid; i < n; i += kTvThreads) {
            const int64_t k = off + (int64_t)i;
            a.points_world[3 * k] = 0.0; a.points_world[3 * k + 1] = 0.0; a.points_world[3 * k + 2] = 0.0;
            a.depth[k] = 0.0;
            valid[i] = 0;
            survivor[i] = -1;
        }
        if (tid == 0) a.n_valid[pair] = 0;
        return;
    }
    const double s = a.scale[pair];
    const SE3 Tinv = se3_inverse(se3_load(a.cur_pose + 7 * (int64_t)pair));  // Frame::camera2world (src/frame.cpp:94-97)
    int32_t done = 0;  // survivors of the chunks before this one (uniform)
    for (int base = 0; base < n; base += kTvThreads) {
        const int i = base + tid;
        bool keep = false;
        if (i < n) {
            const int64_t k = off + (int64_t)i;
            const V3 pc{a.points_cur[3 * k] * s, a.points_cur[3 * k + 1] * s, a.points_cur[3 * k + 2] * s};  // (:189)
            const V3 X = se3_act(Tinv, pc);                                                                 // (:190)
            a.points_world[3 * k] = X.x; a.points_world[3 * k + 1] = X.y; a.points_world[3 * k + 2] = X.z;
            keep = in_frame(rpx[2 * i], rpx[2 * i + 1], a.width, a.height, a.half_patch) &&
                   in_frame(cpx[2 * i], cpx[2 * i + 1], a.width, a.height, a.half_patch) && pc.z > 0;  // (:201-202)
            valid[i] = keep ? 1 : 0;
        }
        const uint64_t mk = __ballot(keep);
        if (lane == 0) wsum[wave] = __popcll(mk);
        __syncthreads();
        int32_t before = done, chunk = 0;
        for (int w = 0; w < kTvWaves; ++w) {
            if (w < wave) before += wsum[w];
            chunk += wsum[w];
        }
        if (keep) survivor[before + __popcll(mk & ((1ull << lane) - 1ull))] = i;  // slot <= i: inside the pair
        done += chunk;
        __syncthreads();
    }
    for (int i = done + tid; i < n; i += kTvThreads) survivor[i] = -1;
    if (tid == 0) a.n_valid[pair] = done;
}

__global__ void __launch_bounds__(kTvThreads) triangulate_dlt_kernel(TwoViewArgs a) {
    const int pair = blockIdx.x;
    const int32_t off = a.feat_off[pair], n = a.feat_off[pair + 1] - off;
    const double* rpx = a.ref_px + 2 * (int64_t)off;
    const double* cpx = a.cur_px + 2 * (int64_t)off;
    const Proj P1 = make_proj(a.fx, a.fy, a.cx, a.cy, se3_load(a.ref_poses + 7 * (int64_t)pair));
    const Proj P2 = make_proj(a.fx, a.fy, a.cx, a.cy, se3_load(a.cur_pose + 7 * (int64_t)pair));
    for (int i = threadIdx.x; i < n; i += kTvThreads) {
        const V3 X = triangulate_dlt(P1, P2, rpx[2 * i], rpx[2 * i + 1], cpx[2 * i], cpx[2 * i + 1]);
        const int64_t k = off + (int64_t)i;
        a.points_world[3 * k] = X.x; a.points_world[3 * k + 1] = X.y; a.points_world[3 * k + 2] = X.z;
    }
}

}  // namespace

void launch_two_view_vote(const TwoViewArgs& a, hipStream_t s) {
    if (a.n_pairs > 0) hipLaunchKernelGGL(two_view_vote_kernel, dim3(a.n_pairs), dim3(kTvThreads), 0, s, a);
}
void launch_two_view_finish(const TwoViewArgs& a, hipStream_t s) {
    if (a.n_pairs > 0) hipLaunchKernelGGL(two_view_finish_kernel, dim3(a.n_pairs), dim3(kTvThreads), 0, s, a);
}
void launch_triangulate_dlt(const TwoViewArgs& a, hipStream_t s) {
    if (a.n_pairs > 0) hipLaunchKernelGGL(triangulate_dlt_kernel, dim3(a.n_pairs), dim3(kTvThreads), 0, s, a);
}

// ------------------------------------------------------------------ host half
// F = invK^T * E * invK (src/system.cpp:144; invK of src/pinhole_camera.cpp:24), Eigen's left-to-right products
void two_view_fundamental(const svo_camera& cam, const double* E, double* F) {
    const double iK[3][3] = {{1 / cam.fx, 0.0, -cam.cx / cam.fx}, {0.0, 1 / cam.fy, -cam.cy / cam.fy}, {0.0, 0.0, 1.0}};
    double T[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T[i][j] = iK[0][i] * E[j] + iK[1][i] * E[3 + j] + iK[2][i] * E[6 + j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) F[3 * i + j] = T[i][0] * iK[0][j] + T[i][1] * iK[1][j] + T[i][2] * iK[2][j];
}

namespace {

// Eigen's Quaternion(Matrix3) (used by AngleAxisd(R) and by Sophus::SO3d(R))
Q quat_from_matrix(const double m[3][3]) {
    double q[4];  // x y z w
    double t = m[0][0] + m[1][1] + m[2][2];
    if (t > 0.0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[2][1] - m[1][2]) * t;
        q[1] = (m[0][2] - m[2][0]) * t;
        q[2] = (m[1][0] - m[0][1]) * t;
    } else {
        int i = 0;
        if (m[1][1] > m[0][0]) i = 1;
        if (m[2][2] > m[i][i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[k][j] - m[j][k]) * t;
        q[j] = (m[j][i] + m[i][j]) * t;
        q[k] = (m[k][i] + m[i][k]) * t;
    }
    return {q[0], q[1], q[2], q[3]};
}

// Eigen::AngleAxisd temp(R); temp.toRotationMatrix(): the reference's re-orthogonalisation (src/algorithm.cpp:281-286)
void angle_axis_round_trip(const double R[3][3], double out[3][3]) {
    const Q q = quat_from_matrix(R);
    double n = std::sqrt(q.x * q.x + q.y * q.y + q.z * q.z);
    if (n < std::numeric_limits<double>::epsilon()) n = std::hypot(std::hypot(q.x, q.y), q.z);  // stableNorm
    double angle = 0.0, ax[3] = {1.0, 0.0, 0.0};
    if (n != 0.0) {
        angle = 2.0 * std::atan2(n, std::fabs(q.w));
        if (q.w < 0.0) n = -n;
        ax[0] = q.x / n; ax[1] = q.y / n; ax[2] = q.z / n;
    }
    const double sn = std::sin(angle), c = std::cos(angle);
    const double sa[3] = {sn * ax[0], sn * ax[1], sn * ax[2]};
    const double ca[3] = {(1.0 - c) * ax[0], (1.0 - c) * ax[1], (1.0 - c) * ax[2]};
    double tmp = ca[0] * ax[1];
    out[0][1] = tmp - sa[2]; out[1][0] = tmp + sa[2];
    tmp = ca[0] * ax[2];
    out[0][2] = tmp + sa[1]; out[2][0] = tmp - sa[1];
    tmp = ca[1] * ax[2];
    out[1][2] = tmp - sa[0]; out[2][1] = tmp + sa[0];
    for (int i = 0; i < 3; ++i) out[i][i] = ca[i] * ax[i] + c;
}

double det3(const double m[3][3]) {
    return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
           m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// Full SVD E = U diag(s) V^T of a 3x3 by one-sided Jacobi rotations of the columns (Hestenes), singular values
// descending.  An essential matrix has s = (s, s, 0): the third left vector is taken as u0 x u1, since the third
// rotated column has no direction of its own.  Which of the valid sign / rotation conventions an SVD lands on only
// relabels the four hypotheses of recoverPose (the set {R1, R2} x {t, -t} is the same for all of them).
void svd3(const double* E, double U[3][3], double V[3][3]) {
    double A[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            A[i][j] = E[3 * i + j];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 60; ++sweep) {
        bool rotated = false;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                double al = 0.0, be = 0.0, ga = 0.0;
                for (int i = 0; i < 3; ++i) {
                    al += A[i][p] * A[i][p];
                    be += A[i][q] * A[i][q];
                    ga += A[i][p] * A[i][q];
                }
                if (ga == 0.0 || std::fabs(ga) <= 1e-16 * std::sqrt(al * be)) continue;
                rotated = true;
                const double zeta = (be - al) / (2.0 * ga);
                const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (std::fabs(zeta) + std::sqrt(1.0 + zeta * zeta));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = c * t;
                for (int i = 0; i < 3; ++i) {
                    const double ap = A[i][p], aq = A[i][q];
                    A[i][p] = c * ap - s * aq;
                    A[i][q] = s * ap + c * aq;
                    const double vp = V[i][p], vq = V[i][q];
                    V[i][p] = c * vp - s * vq;
                    V[i][q] = s * vp + c * vq;
                }
            }
        if (!rotated) break;
    }
    double nrm[3];
    int ord[3] = {0, 1, 2};
    for (int j = 0; j < 3; ++j) nrm[j] = std::sqrt(A[0][j] * A[0][j] + A[1][j] * A[1][j] + A[2][j] * A[2][j]);
    std::sort(ord, ord + 3, [&](int x, int y) { return nrm[x] > nrm[y]; });
    double Vs[3][3], u[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};  // u[k] = k-th left vector
    for (int k = 0; k < 3; ++k)
        for (int i = 0; i < 3; ++i) Vs[i][k] = V[i][ord[k]];
    const double tiny = nrm[ord[0]] * 1e-150;
    if (nrm[ord[0]] > 0.0) {
        for (int i = 0; i < 3; ++i) u[0][i] = A[i][ord[0]] / nrm[ord[0]];
        if (nrm[ord[1]] > tiny) {
            for (int i = 0; i < 3; ++i) u[1][i] = A[i][ord[1]] / nrm[ord[1]];
        } else {  // rank one: any unit vector orthogonal to u0
            int m = 0;
            for (int i = 1; i < 3; ++i)
                if (std::fabs(u[0][i]) < std::fabs(u[0][m])) m = i;
            double e[3] = {0, 0, 0};
            e[m] = 1.0;
            const double d = u[0][m];
            double w[3], wn = 0.0;
            for (int i = 0; i < 3; ++i) { w[i] = e[i] - d * u[0][i]; wn += w[i] * w[i]; }
            wn = std::sqrt(wn);
            for (int i = 0; i < 3; ++i) u[1][i] = w[i] / wn;
        }
        u[2][0] = u[0][1] * u[1][2] - u[0][2] * u[1][1];
        u[2][1] = u[0][2] * u[1][0] - u[0][0] * u[1][2];
        u[2][2] = u[0][0] * u[1][1] - u[0][1] * u[1][0];
    }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            U[i][k] = u[k][i];
            V[i][k] = Vs[i][k];
        }
}

}  // namespace

// algorithm::decomposeEssentialMatrix (src/algorithm.cpp:241-259) and the four poses of recoverPose (:279-286):
// hyp[4][7] = (R1, t) (R1, -t) (R2, t) (R2, -t) as Sophus params
void two_view_hypotheses(const double* E, double* hyp) {
    double U[3][3], V[3][3];
    svd3(E, U, V);
    // U * W * V^T = u1 v0^T - u0 v1^T + u2 v2^T, U * W^T * V^T = -u1 v0^T + u0 v1^T + u2 v2^T  (W: :246)
    double R[2][3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            const double a = U[i][1] * V[j][0] - U[i][0] * V[j][1], b = U[i][2] * V[j][2];
            R[0][i][j] = a + b;
            R[1][i][j] = -a + b;
        }
    const double t[3] = {U[0][2], U[1][2], U[2][2]};  // svd.matrixU().col(2) (:257)
    for (int r = 0; r < 2; ++r) {
        if (det3(R[r]) < 0)  // (:248-249, :253-254)
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) R[r][i][j] *= -1;
        double Ro[3][3];
        angle_axis_round_trip(R[r], Ro);
        const Q q = quat_from_matrix(Ro);  // Sophus::SE3d(R, t)
        for (int sgn = 0; sgn < 2; ++sgn) {
            double* o = hyp + 7 * (2 * r + sgn);
            o[0] = q.x; o[1] = q.y; o[2] = q.z; o[3] = q.w;
            for (int i = 0; i < 3; ++i) o[4 + i] = sgn ? -t[i] : t[i];
        }
    }
}

// algorithm::computeMedian(const Eigen::VectorXd&) (src/algorithm.cpp:813-832), statement by statement: the
// even-length vec[mid - 1] is whatever libstdc++'s std::nth_element leaves there
double two_view_median(const double* depth, int64_t n) {
    std::vector<double> vec(depth, depth + n);
    const auto middleSize = vec.size() / 2;
    std::nth_element(vec.begin(), vec.begin() + middleSize, vec.end());
    if (vec.size() == 0) return std::numeric_limits<double>::quiet_NaN();
    if (vec.size() % 2 != 0) return vec[middleSize];
    return (vec[middleSize - 1] + vec[middleSize]) / 2.0;
}

// The rescaled current pose (src/system.cpp:184-186): t = -R_cur * (C_ref + s * (C_cur - C_ref))
void two_view_rescale_pose(const double* ref_pose, double scale, double* cur_pose) {
    const SE3 Tr = se3_load(ref_pose);
    SE3 Tc = se3_load(cur_pose);
    const V3 Cr = camera_in_world(Tr), Cc = camera_in_world(Tc);
    const V3 C = v3add(Cr, v3scl(v3sub(Cc, Cr), scale));
    double R[3][3];
    rotmat(Tc.q, R);
    Tc.t = {(-R[0][0]) * C.x + (-R[0][1]) * C.y + (-R[0][2]) * C.z, (-R[1][0]) * C.x + (-R[1][1]) * C.y + (-R[1][2]) * C.z,
            (-R[2][0]) * C.x + (-R[2][1]) * C.y + (-R[2][2]) * C.z};
    se3_store(Tc, cur_pose);
}

}  // namespace svo
