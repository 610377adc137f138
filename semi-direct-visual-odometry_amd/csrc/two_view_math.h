// two_view_math.h — the per-match arithmetic of the two-view initialisation (two_view.hip), host and device:
// one match of algorithm::sampsonCorrection, the projection matrices, algorithm::triangulatePointDLT with its 3x3
// LDLT, and PinholeCamera::isInFrame, in the reference's order.
#pragma once
#include "svo_math.h"

namespace svo {

// One match of algorithm::sampsonCorrection (src/algorithm.cpp:196-235), the reference's expressions term by term.
// px = (x0.x, x0.y, x1.x, x1.y): the ref and cur pixel, corrected in place.
SVO_HD void sampson_correct(const double F[3][3], double px[4]) {
    const double x0x = px[0], x0y = px[1], x1x = px[2], x1y = px[3];
    const double upper = (x0x * ((x1x * F[0][0]) + (x1y * F[1][0]) + F[2][0])) +
                         (x0y * ((x1x * F[0][1]) + (x1y * F[1][1]) + F[2][1])) + (x1x * F[0][2]) +
                         (x1y * F[1][2]) + F[2][2];
    const double t0 = ((F[0][0] * x0x) + (F[0][1] * x0y) + F[0][2]);
    const double t1 = ((F[1][0] * x0x) + (F[1][1] * x0y) + F[1][2]);
    const double t2 = ((F[0][0] * x1x) + (F[1][0] * x1y) + F[2][0]);
    const double t3 = ((F[0][1] * x1x) + (F[1][1] * x1y) + F[2][1]);
    const double lower = ((t0 * t0) + (t1 * t1) + (t2 * t2) + (t3 * t3));
    const double factor = upper / lower;
    px[0] = x0x - (factor * t2);
    px[1] = x0y - (factor * t3);
    px[2] = x1x - (factor * t0);
    px[3] = x1y - (factor * t1);
}

SVO_HD void tv_cswap(bool c, double& a, double& b) {
    const double t = a;
    a = c ? b : a;
    b = c ? t : b;
}

// ldlt_solve_ws (svo_math.h: Eigen LDLT<.., Lower>) for n = 3, operation for operation, with the pivot swaps as
// selects on six named entries: no indexed local array, so nothing goes to scratch memory.
// H row-major symmetric (lower triangle read).
SVO_HD void ldlt3_solve(const double* H, const double* b, double* x) {
    double a00 = H[0], a10 = H[3], a11 = H[4], a20 = H[6], a21 = H[7], a22 = H[8];
    // k = 0: the first largest |diagonal|
    int p0 = 0;
    double best = fabs(a00);
    if (fabs(a11) > best) { best = fabs(a11); p0 = 1; }
    if (fabs(a22) > best) { best = fabs(a22); p0 = 2; }
    tv_cswap(p0 == 1, a00, a11);
    tv_cswap(p0 == 1, a20, a21);
    tv_cswap(p0 == 2, a00, a22);
    tv_cswap(p0 == 2, a10, a21);
    int p1 = 1;
    if (fabs(a00) > 0.0) {
        a10 /= a00;
        a20 /= a00;
        // k = 1
        p1 = fabs(a22) > fabs(a11) ? 2 : 1;
        tv_cswap(p1 == 2, a10, a20);
        tv_cswap(p1 == 2, a11, a22);
        const double t0 = a00 * a10;
        a11 -= 0.0 + a10 * t0;
        a21 -= 0.0 + a20 * t0;
        if (fabs(a11) > 0.0) a21 /= a11;
        // k = 2
        const double u0 = a00 * a20, u1 = a11 * a21;
        a22 -= (0.0 + a20 * u0) + a21 * u1;
    } else {  // a zero matrix: Eigen stops with the identity permutation
        p0 = 0;
    }
    double x0 = b[0], x1 = b[1], x2 = b[2];
    tv_cswap(p0 == 1, x0, x1);
    tv_cswap(p0 == 2, x0, x2);
    tv_cswap(p1 == 2, x1, x2);
    x1 = x1 - a10 * x0;
    x2 = (x2 - a20 * x0) - a21 * x1;
    x0 = fabs(a00) > 2.2250738585072014e-308 ? x0 / a00 : 0.0;
    x1 = fabs(a11) > 2.2250738585072014e-308 ? x1 / a11 : 0.0;
    x2 = fabs(a22) > 2.2250738585072014e-308 ? x2 / a22 : 0.0;
    x1 = x1 - a21 * x2;
    x0 = (x0 - a10 * x1) - a20 * x2;
    tv_cswap(p1 == 2, x1, x2);
    tv_cswap(p0 == 2, x0, x2);
    tv_cswap(p0 == 1, x0, x1);
    x[0] = x0; x[1] = x1; x[2] = x2;
}

struct Proj { double m[3][4]; };  // K * m_absPose.matrix3x4() (src/algorithm.cpp:662-663)

// Eigen's 3x3 * 3x4 coefficient sums run k = 0, 1, 2 with K's zeros as terms
SVO_HD Proj make_proj(double fx, double fy, double cx, double cy, const SE3& T) {
    double R[3][3];
    rotmat(T.q, R);
    const double M[3][4] = {{R[0][0], R[0][1], R[0][2], T.t.x}, {R[1][0], R[1][1], R[1][2], T.t.y},
                            {R[2][0], R[2][1], R[2][2], T.t.z}};
    Proj P;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        P.m[0][j] = fx * M[0][j] + 0.0 * M[1][j] + cx * M[2][j];
        P.m[1][j] = 0.0 * M[0][j] + fy * M[1][j] + cy * M[2][j];
        P.m[2][j] = 0.0 * M[0][j] + 0.0 * M[1][j] + 1.0 * M[2][j];
    }
    return P;
}

// algorithm::triangulatePointDLT (src/algorithm.cpp:655-680): the 4x3 system of both views, its normal equations
// and Eigen's LDLT on the 3x3 (ldlt3_solve restates it)
SVO_HD V3 triangulate_dlt(const Proj& P1, const Proj& P2, double x0, double y0, double x1,
                                              double y1) {
    double A[4][3], p[4];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        A[0][j] = P1.m[0][j] - x0 * P1.m[2][j];
        A[1][j] = P1.m[1][j] - y0 * P1.m[2][j];
        A[2][j] = P2.m[0][j] - x1 * P2.m[2][j];
        A[3][j] = P2.m[1][j] - y1 * P2.m[2][j];
    }
    p[0] = x0 * P1.m[2][3] - P1.m[0][3];
    p[1] = y0 * P1.m[2][3] - P1.m[1][3];
    p[2] = x1 * P2.m[2][3] - P2.m[0][3];
    p[3] = y1 * P2.m[2][3] - P2.m[1][3];
    double H[9], g[3], x[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = i; j < 3; ++j) {
            const double s = ((A[0][i] * A[0][j] + A[1][i] * A[1][j]) + A[2][i] * A[2][j]) + A[3][i] * A[3][j];
            H[3 * i + j] = s;
            H[3 * j + i] = s;
        }
        g[i] = ((A[0][i] * p[0] + A[1][i] * p[1]) + A[2][i] * p[2]) + A[3][i] * p[3];
    }
    ldlt3_solve(H, g, x);
    return {x[0], x[1], x[2]};
}

// PinholeCamera::isInFrame (src/pinhole_camera.cpp:163-168)
SVO_HD bool in_frame(double x, double y, int32_t width, int32_t height, double b) {
    return x >= b && y >= b && x < width - b && y < height - b;
}

}  // namespace svo
