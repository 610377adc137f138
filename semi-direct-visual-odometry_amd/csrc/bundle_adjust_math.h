// bundle_adjust_math.h — the per-edge and per-point arithmetic of the windowed bundle adjustment
// (bundle_adjust.hip), shared by the kernels and the host.
//
// This is the project's own contract (include/svo_c.h, svo_bundle_adjust), modelled on g2o's
// OptimizationAlgorithmLevenberg with EdgeProjectXYZ2UV edges as BundleAdjustment::twoViewBA / localBA set them
// up (src/bundle_adjustment.cpp:304-339, :397-625).  It is not pinned to g2o: g2o is not part of the reference
// tree, so nothing here was compared with its bits.
//   residual   e = u - proj(R X + t), proj(c) = (f c.x / c.z + cx, f c.y / c.z + cy) with f = fx on both axes
//              (setupG2o builds g2o::CameraParameters(fx, principalPoint, 0), :333), no cheirality test
//   Huber      on e2 = e.e with width delta: rho = e2, w = 1 while sqrt(e2) <= delta, else
//              rho = 2 delta sqrt(e2) - delta^2, w = delta / sqrt(e2)
//   Jacobians  A = d proj / d c; J_p = A [I | -hat(c)] for pose <- exp(dp) * pose, J_x = A R
#pragma once
#include "svo_math.h"

namespace svo {

struct BAPose { double R[3][3]; V3 t; };

SVO_HD BAPose ba_pose(const double* p7) {
    BAPose P;
    const Q q{p7[0], p7[1], p7[2], p7[3]};
    rotmat(q, P.R);
    P.t = {p7[4], p7[5], p7[6]};
    return P;
}

SVO_HD V3 ba_transform(const BAPose& P, V3 X) {
    return {P.R[0][0] * X.x + P.R[0][1] * X.y + P.R[0][2] * X.z + P.t.x,
            P.R[1][0] * X.x + P.R[1][1] * X.y + P.R[1][2] * X.z + P.t.y,
            P.R[2][0] * X.x + P.R[2][1] * X.y + P.R[2][2] * X.z + P.t.z};
}

struct BAEdge { double ex, ey, e2, w, rho; };

SVO_HD BAEdge ba_edge(V3 c, double f, double cx, double cy, double u, double v, double delta) {
    BAEdge e;
    e.ex = u - (f * c.x / c.z + cx);
    e.ey = v - (f * c.y / c.z + cy);
    e.e2 = e.ex * e.ex + e.ey * e.ey;
    const double s = sqrt(e.e2);
    if (s <= delta) {
        e.rho = e.e2;
        e.w = 1.0;
    } else {
        e.rho = 2.0 * delta * s - delta * delta;
        e.w = delta / s;
    }
    return e;
}

SVO_HD void ba_jacobians(const BAPose& P, V3 c, double f, double Jp[2][6], double Jx[2][3]) {
    const double iz = 1.0 / c.z;
    const double a0 = f * iz, a2 = -(f * c.x) * iz * iz, b2 = -(f * c.y) * iz * iz;  // A = [a0 0 a2; 0 a0 b2]
    // [I | -hat(c)]: column 3 = (0, -c.z, c.y), column 4 = (c.z, 0, -c.x), column 5 = (-c.y, c.x, 0)
    Jp[0][0] = a0; Jp[0][1] = 0.0; Jp[0][2] = a2;
    Jp[0][3] = a2 * c.y; Jp[0][4] = a0 * c.z + a2 * (-c.x); Jp[0][5] = a0 * (-c.y);
    Jp[1][0] = 0.0; Jp[1][1] = a0; Jp[1][2] = b2;
    Jp[1][3] = a0 * (-c.z) + b2 * c.y; Jp[1][4] = b2 * (-c.x); Jp[1][5] = a0 * c.x;
    for (int m = 0; m < 3; ++m) {
        Jx[0][m] = a0 * P.R[0][m] + a2 * P.R[2][m];
        Jx[1][m] = a0 * P.R[1][m] + b2 * P.R[2][m];
    }
}

// symmetric 3x3 as (xx, xy, xz, yy, yz, zz).  Vi = (V + lambda I)^-1 through its Cholesky factor; false at a
// non-positive (or NaN) pivot.
SVO_HD bool ba_sym3_inverse(const double V[6], double lambda, double Vi[6]) {
    const double a = V[0] + lambda;
    if (!(a > 0.0)) return false;
    const double l00 = sqrt(a), l10 = V[1] / l00, l20 = V[2] / l00;
    const double d1 = (V[3] + lambda) - l10 * l10;
    if (!(d1 > 0.0)) return false;
    const double l11 = sqrt(d1), l21 = (V[4] - l20 * l10) / l11;
    const double d2 = ((V[5] + lambda) - l20 * l20) - l21 * l21;
    if (!(d2 > 0.0)) return false;
    const double l22 = sqrt(d2);
    // M = L^-1 (lower), Vi = M^T M
    const double m00 = 1.0 / l00, m11 = 1.0 / l11, m22 = 1.0 / l22;
    const double m10 = -(l10 * m00) / l11;
    const double m20 = -(l20 * m00 + l21 * m10) / l22;
    const double m21 = -(l21 * m11) / l22;
    Vi[0] = m00 * m00 + m10 * m10 + m20 * m20;
    Vi[1] = m10 * m11 + m20 * m21;
    Vi[2] = m20 * m22;
    Vi[3] = m11 * m11 + m21 * m21;
    Vi[4] = m21 * m22;
    Vi[5] = m22 * m22;
    return true;
}

SVO_HD V3 ba_sym3_mul(const double S[6], V3 v) {
    return {S[0] * v.x + S[1] * v.y + S[2] * v.z, S[1] * v.x + S[3] * v.y + S[4] * v.z,
            S[2] * v.x + S[4] * v.y + S[5] * v.z};
}

// lambda *= max(1/3, min(1 - (2r - 1)^3, 2/3)) after an accepted step
SVO_HD double ba_lambda_factor(double r) {
    const double t = 2.0 * r - 1.0;
    double alpha = 1.0 - t * t * t;
    alpha = alpha < 2.0 / 3.0 ? alpha : 2.0 / 3.0;
    return alpha > 1.0 / 3.0 ? alpha : 1.0 / 3.0;
}

}  // namespace svo
