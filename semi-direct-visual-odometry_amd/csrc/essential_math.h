// essential_math.h — the per-sample and per-match arithmetic of the essential-matrix RANSAC (essential.hip), host and
// device: the counter-based sampler, the Sampson inlier test and the five-point minimal solver.  The contract is
// stated in include/svo_c.h ("essential-matrix RANSAC"); tests/essential_ref.py restates it in numpy.
//
// The solver works on a per-sample store of kEssStore doubles that the caller provides through an accessor `s(i)`:
// a strided slice of LDS on the device (one lane per sample), a plain array on the host.  Everything indexed by a
// run-time value lives in that store; what stays in local arrays is indexed by unrolled loop counters only, so the
// device code needs no private segment.
#pragma once
#include "two_view_math.h"

namespace svo {

constexpr int kEssStore = 240;       // doubles per sample: the 10 x 20 system (0..199), the null-space basis (200..235)
constexpr int kEssBasis = 200;
constexpr int kEssMaxModels = 10;
constexpr double kEssResidualMax = 1e-9;   // a polished root with a larger scaled residual is discarded
constexpr double kEssDuplicate = 1e-6;     // two unit models closer than this (up to sign) are one
constexpr int kEssPolishMax = 10;
constexpr int kEssAberthMax = 80;
constexpr int kEssRefineMax = 24;

// ------------------------------------------------------------------ sampling
SVO_HD uint64_t ess_mix(uint64_t z) {  // the splitmix64 finaliser
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// five distinct indices below n for sample h of pair p; false when draws 0..255 do not yield five
SVO_HD bool ess_sample(uint64_t seed, uint32_t p, uint32_t h, uint32_t n, int idx[5]) {
    int k = 0;
#pragma unroll
    for (int j = 0; j < 5; ++j) idx[j] = -1;
    for (uint32_t c = 0; c < 256 && k < 5; ++c) {
        const uint64_t r = ess_mix(seed ^ ((uint64_t)p << 44) ^ ((uint64_t)h << 8) ^ (uint64_t)c);
        const int v = (int)(((r >> 32) * (uint64_t)n) >> 32);
        bool dup = false;
#pragma unroll
        for (int j = 0; j < 5; ++j) dup = dup || idx[j] == v;
        if (dup) continue;
#pragma unroll
        for (int j = 0; j < 5; ++j) idx[j] = j == k ? v : idx[j];
        ++k;
    }
    return k == 5;
}

// ------------------------------------------------------------------ scoring
// a pixel coordinate as the reference holds it (a cv::Point2f), normalised
SVO_HD double ess_normalise(double u, double c, double f) { return ((double)(float)u - c) / f; }

// the Sampson test of one match on normalised coordinates, every operation rounded once in the written order
SVO_HD bool ess_inlier(const double* E, double x1x, double x1y, double x2x, double x2y, double thr2) {
    const double a0 = (E[0] * x1x + E[1] * x1y) + E[2];
    const double a1 = (E[3] * x1x + E[4] * x1y) + E[5];
    const double a2 = (E[6] * x1x + E[7] * x1y) + E[8];
    const double b0 = (E[0] * x2x + E[3] * x2y) + E[6];
    const double b1 = (E[1] * x2x + E[4] * x2y) + E[7];
    const double num = (x2x * a0 + x2y * a1) + a2;
    const double den = ((a0 * a0 + a1 * a1) + b0 * b0) + b1 * b1;
    const double err = (num * num) / den;
    return err <= thr2;  // false for a NaN
}

// ------------------------------------------------------------------ five-point solver
namespace ess {

// monomials of x, y, z, 1 (variables 0..3).  Quadratic index of the pair (a <= b):
SVO_HD constexpr int quad_index(int a, int b) {
    const int lo = a < b ? a : b, hi = a < b ? b : a;
    return lo == 0 ? hi : lo == 1 ? 3 + hi : lo == 2 ? 5 + hi : 9;
}
SVO_HD constexpr int quad_first(int q) { return q < 4 ? 0 : q < 7 ? 1 : q < 9 ? 2 : 3; }
SVO_HD constexpr int quad_second(int q) { return q < 4 ? q : q < 7 ? q - 3 : q < 9 ? q - 5 : 3; }
// column of the cubic monomial x^ex y^ey z^ez in the 10 x 20 system: the ten eliminated monomials first
//   x^3 y^3 x^2y xy^2 x^2z x^2 y^2z y^2 xyz xy | xz^2 xz x yz^2 yz y z^3 z^2 z 1
SVO_HD constexpr int cubic_column(int ex, int ey, int ez) {
    const int key = ex * 16 + ey * 4 + ez;
    return key == 48 ? 0 : key == 12 ? 1 : key == 36 ? 2 : key == 24 ? 3 : key == 33 ? 4 : key == 32 ? 5 :
           key == 9 ? 6 : key == 8 ? 7 : key == 21 ? 8 : key == 20 ? 9 : key == 18 ? 10 : key == 17 ? 11 :
           key == 16 ? 12 : key == 6 ? 13 : key == 5 ? 14 : key == 4 ? 15 : key == 3 ? 16 : key == 2 ? 17 :
           key == 1 ? 18 : 19;
}
SVO_HD constexpr int cubic_of(int q, int v) {
    const int a = quad_first(q), b = quad_second(q);
    return cubic_column((a == 0) + (b == 0) + (v == 0), (a == 1) + (b == 1) + (v == 1), (a == 2) + (b == 2) + (v == 2));
}

// quad += sign * (linear a) * (linear b)
SVO_HD void lin_mul_acc(const double* a, const double* b, double sign, double* quad) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int v = 0; v < 4; ++v) quad[quad_index(u, v)] += sign * (a[u] * b[v]);
}
// cubic (by column) += (quadratic q) * (linear l)
SVO_HD void quad_mul_acc(const double* q, const double* l, double* cubic) {
#pragma unroll
    for (int i = 0; i < 10; ++i)
#pragma unroll
        for (int v = 0; v < 4; ++v) cubic[cubic_of(i, v)] += q[i] * l[v];
}

// 3 x 3 row-major products on local arrays (unrolled: registers)
SVO_HD void mul_ab(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}
SVO_HD void mul_abt(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[3 * j] + a[3 * i + 1] * b[3 * j + 1]) + a[3 * i + 2] * b[3 * j + 2];
}
SVO_HD void mul_atb(const double* a, const double* b, double* c) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[i] * b[j] + a[3 + i] * b[3 + j]) + a[6 + i] * b[6 + j];
}

// the ten constraints at E (row-major): c[3i+j] = (E E^T E - tr(E E^T)/2 E)_ij, c[9] = det E; cof = cofactors of E
SVO_HD void constraints(const double* E, double* c, double* G, double* cof, double& half_tr) {
    mul_abt(E, E, G);
    half_tr = 0.5 * ((G[0] + G[4]) + G[8]);
    double T[9];
    mul_ab(G, E, T);
#pragma unroll
    for (int i = 0; i < 9; ++i) c[i] = T[i] - half_tr * E[i];
    cof[0] = E[4] * E[8] - E[5] * E[7];
    cof[1] = E[5] * E[6] - E[3] * E[8];
    cof[2] = E[3] * E[7] - E[4] * E[6];
    cof[3] = E[2] * E[7] - E[1] * E[8];
    cof[4] = E[0] * E[8] - E[2] * E[6];
    cof[5] = E[1] * E[6] - E[0] * E[7];
    cof[6] = E[1] * E[5] - E[2] * E[4];
    cof[7] = E[2] * E[3] - E[0] * E[5];
    cof[8] = E[0] * E[4] - E[1] * E[3];
    c[9] = (E[0] * cof[0] + E[1] * cof[1]) + E[2] * cof[2];
}

// E = x X + y Y + z Z + W from the basis in the store
template <class S>
SVO_HD void model_at(const S& s, double x, double y, double z, double* E) {
#pragma unroll
    for (int i = 0; i < 9; ++i)
        E[i] = ((x * s(kEssBasis + i) + y * s(kEssBasis + 9 + i)) + z * s(kEssBasis + 18 + i)) + s(kEssBasis + 27 + i);
}

// Gauss-Newton on the ten cubics in (x, y, z): steps while the scaled residual |c| / |E|^3 decreases, at most
// kEssPolishMax; returns the scaled residual at the (x, y, z) it leaves
template <class S>
SVO_HD double polish(const S& s, double& x, double& y, double& z) {
    double best = 0.0, px = x, py = y, pz = z;
    for (int it = 0;; ++it) {
        double E[9], c[10], G[9], cof[9], half_tr;
        model_at(s, x, y, z, E);
        constraints(E, c, G, cof, half_tr);
        double n2 = 0.0, r2 = 0.0;
#pragma unroll
        for (int i = 0; i < 9; ++i) n2 += E[i] * E[i];
#pragma unroll
        for (int i = 0; i < 10; ++i) r2 += c[i] * c[i];
        const double rho = sqrt(r2) / (n2 * sqrt(n2));
        if (it > 0 && !(rho < best)) {  // no improvement (or a NaN): keep the previous point
            x = px; y = py; z = pz;
            return best;
        }
        best = rho;
        if (it == kEssPolishMax || rho == 0.0) return best;
        // Jacobian columns: D = dE/dv
        double H[9], g[3], J[3][10], EtE[9];
        mul_atb(E, E, EtE);
#pragma unroll
        for (int v = 0; v < 3; ++v) {
            double D[9], A[9], B[9], C[9], DtE[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) D[i] = s(kEssBasis + 9 * v + i);
            mul_ab(D, EtE, A);    // D E^T E
            mul_atb(D, E, DtE);
            mul_ab(E, DtE, B);    // E D^T E
            mul_ab(G, D, C);      // E E^T D
            double trd = 0.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) trd += D[i] * E[i];
            double dd = 0.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                J[v][i] = ((A[i] + B[i]) + C[i]) - (trd * E[i] + half_tr * D[i]);
                dd += cof[i] * D[i];
            }
            J[v][9] = dd;
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                double acc = 0.0;
#pragma unroll
                for (int i = 0; i < 10; ++i) acc += J[a][i] * J[b][i];
                H[3 * a + b] = acc;
            }
            double acc = 0.0;
#pragma unroll
            for (int i = 0; i < 10; ++i) acc += J[a][i] * c[i];
            g[a] = acc;
        }
        double d[3];
        ldlt3_solve(H, g, d);
        px = x; py = y; pz = z;
        x -= d[0];
        y -= d[1];
        z -= d[2];
    }
}

struct Cx { double r, i; };
SVO_HD Cx cadd(Cx a, Cx b) { return {a.r + b.r, a.i + b.i}; }
SVO_HD Cx csub(Cx a, Cx b) { return {a.r - b.r, a.i - b.i}; }
SVO_HD Cx cmul(Cx a, Cx b) { return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r}; }
SVO_HD Cx cdet(const Cx* a, const Cx* b, const Cx* c) {  // rows a, b, c
    const Cx m0 = csub(cmul(b[1], c[2]), cmul(b[2], c[1])), m1 = csub(cmul(b[2], c[0]), cmul(b[0], c[2])),
             m2 = csub(cmul(b[0], c[1]), cmul(b[1], c[0]));
    return cadd(cadd(cmul(a[0], m0), cmul(a[1], m1)), cmul(a[2], m2));
}

// dst[0 .. na+nb-2] += sign * a * b for polynomials in the store (ascending powers)
template <class S>
SVO_HD void poly_mul_acc(const S& s, int dst, int a, int na, int b, int nb, double sign) {
    for (int i = 0; i < na; ++i)
        for (int j = 0; j < nb; ++j) s(dst + i + j) += sign * (s(a + i) * s(b + j));
}

}  // namespace ess

// The models of one minimal sample.  x1 / x2: the five normalised ref / cur points.  s: the sample's store.
// out: kEssMaxModels x 9, row-major, Frobenius norm 1; the slots past the returned count are zero.
template <class S>
SVO_HD int ess_five_point(const double (&x1)[5][2], const double (&x2)[5][2], const S& s, double* out) {
    using namespace ess;
    for (int i = 0; i < kEssMaxModels * 9; ++i) out[i] = 0.0;

    // ---- the null space of the 5 x 9 epipolar equations: Householder QR of their transpose A (9 x 5, A(r, k) at
    // store 5 r + k); the last four columns of Q span it
    for (int k = 0; k < 5; ++k) {
        const double a[3] = {x1[k][0], x1[k][1], 1.0}, b[3] = {x2[k][0], x2[k][1], 1.0};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) s(5 * (3 * i + j) + k) = b[i] * a[j];
    }
    for (int k = 0; k < 5; ++k) {  // reflector k: v in A(k.., k), 2 / v.v at store 45 + k
        double n2 = 0.0;
        for (int r = k; r < 9; ++r) n2 += s(5 * r + k) * s(5 * r + k);
        const double x0 = s(5 * k + k), alpha = x0 > 0.0 ? -sqrt(n2) : sqrt(n2);
        const double v0 = x0 - alpha, vv = (n2 - x0 * x0) + v0 * v0;
        if (!(vv > 0.0)) return 0;  // fewer than five independent equations
        s(5 * k + k) = v0;
        const double beta = 2.0 / vv;
        s(45 + k) = beta;
        for (int j = k + 1; j < 5; ++j) {
            double d = 0.0;
            for (int r = k; r < 9; ++r) d += s(5 * r + k) * s(5 * r + j);
            d *= beta;
            for (int r = k; r < 9; ++r) s(5 * r + j) -= d * s(5 * r + k);
        }
    }
    for (int m = 0; m < 4; ++m) {  // Q e_(5+m) = H_0 .. H_4 e_(5+m)
        const int o = kEssBasis + 9 * m;
        for (int r = 0; r < 9; ++r) s(o + r) = r == 5 + m ? 1.0 : 0.0;
        for (int k = 4; k >= 0; --k) {
            double d = 0.0;
            for (int r = k; r < 9; ++r) d += s(5 * r + k) * s(o + r);
            d *= s(45 + k);
            for (int r = k; r < 9; ++r) s(o + r) -= d * s(5 * r + k);
        }
    }

    // ---- the ten cubics in x, y, z as a 10 x 20 system, row r at store 20 r
    {
        double L[9][4];  // entry 3 i + j of E as a linear polynomial in (x, y, z, 1)
#pragma unroll
        for (int e = 0; e < 9; ++e)
#pragma unroll
            for (int v = 0; v < 4; ++v) L[e][v] = s(kEssBasis + 9 * v + e);
        double G[6][10];  // E E^T: 00 01 02 11 12 22
        constexpr int gi[6] = {0, 0, 0, 1, 1, 2}, gj[6] = {0, 1, 2, 1, 2, 2};
#pragma unroll
        for (int g = 0; g < 6; ++g) {
#pragma unroll
            for (int q = 0; q < 10; ++q) G[g][q] = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) lin_mul_acc(L[3 * gi[g] + k], L[3 * gj[g] + k], 1.0, G[g]);
        }
#pragma unroll
        for (int q = 0; q < 10; ++q) {  // minus half the trace on the diagonal
            const double ht = 0.5 * ((G[0][q] + G[3][q]) + G[5][q]);
            G[0][q] -= ht;
            G[3][q] -= ht;
            G[5][q] -= ht;
        }
        constexpr int sym[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                double c[20];
#pragma unroll
                for (int q = 0; q < 20; ++q) c[q] = 0.0;
#pragma unroll
                for (int k = 0; k < 3; ++k) quad_mul_acc(G[sym[i][k]], L[3 * k + j], c);
#pragma unroll
                for (int q = 0; q < 20; ++q) s(20 * (3 * i + j) + q) = c[q];
            }
        double c[20];
#pragma unroll
        for (int q = 0; q < 20; ++q) c[q] = 0.0;
        constexpr int ca[3] = {4, 5, 3}, cb[3] = {8, 6, 7}, cc[3] = {5, 3, 4}, cd[3] = {7, 8, 6};
#pragma unroll
        for (int j = 0; j < 3; ++j) {  // det E along the first row
            double cof[10];
#pragma unroll
            for (int q = 0; q < 10; ++q) cof[q] = 0.0;
            lin_mul_acc(L[ca[j]], L[cb[j]], 1.0, cof);
            lin_mul_acc(L[cc[j]], L[cd[j]], -1.0, cof);
            quad_mul_acc(cof, L[j], c);
        }
#pragma unroll
        for (int q = 0; q < 20; ++q) s(180 + q) = c[q];
    }

    // ---- Gauss-Jordan with row pivoting on the first ten columns (rows 0..3 are not needed once they have pivoted)
    for (int c = 0; c < 10; ++c) {
        int p = c;
        double big = fabs(s(20 * c + c));
        for (int r = c + 1; r < 10; ++r) {
            const double v = fabs(s(20 * r + c));
            if (v > big) { big = v; p = r; }
        }
        if (!(big > 0.0)) return 0;
        const double inv = 1.0 / s(20 * p + c);
        for (int j = c; j < 20; ++j) {
            const double t = s(20 * p + j);
            s(20 * p + j) = s(20 * c + j);
            s(20 * c + j) = t * inv;
        }
        for (int r = 0; r < 10; ++r) {
            if (r == c || (r < 4 && r < c)) continue;
            const double f = s(20 * r + c);
            for (int j = c + 1; j < 20; ++j) s(20 * r + j) -= f * s(20 * c + j);
        }
    }

    // ---- rows (x^2z, x^2), (y^2z, y^2), (xyz, xy): e - z f has the monomials x z^k, y z^k, z^k only.
    // Row t of B(z) at store 13 t: x-polynomial (4, ascending), y-polynomial (4), constant polynomial (5)
    for (int t = 0; t < 3; ++t) {
        const int e = 20 * (4 + 2 * t) + 10, f = e + 20, o = 13 * t;
        double X[4], Y[4], O[5];
        X[3] = -s(f + 0); X[2] = s(e + 0) - s(f + 1); X[1] = s(e + 1) - s(f + 2); X[0] = s(e + 2);
        Y[3] = -s(f + 3); Y[2] = s(e + 3) - s(f + 4); Y[1] = s(e + 4) - s(f + 5); Y[0] = s(e + 5);
        O[4] = -s(f + 6); O[3] = s(e + 6) - s(f + 7); O[2] = s(e + 7) - s(f + 8); O[1] = s(e + 8) - s(f + 9);
        O[0] = s(e + 9);
        // (rows 4..9 start at store 90: the writes below stay under 39)
#pragma unroll
        for (int i = 0; i < 4; ++i) { s(o + i) = X[i]; s(o + 4 + i) = Y[i]; }
#pragma unroll
        for (int i = 0; i < 5; ++i) s(o + 8 + i) = O[i];
    }
    // det B(z): eleven coefficients at store 60; minors at store 40 (8 coefficients)
    constexpr int kP = 60, kT = 40, kZr = 80, kZi = 90;
    for (int i = 0; i < 11; ++i) s(kP + i) = 0.0;
    for (int term = 0; term < 3; ++term) {
        // term 0: X0 (Y1 O2 - O1 Y2); 1: -Y0 (X1 O2 - O1 X2); 2: O0 (X1 Y2 - Y1 X2)
        const int a1 = 13 + (term == 0 ? 4 : 0), na = 4;
        const int b1 = 13 + (term == 2 ? 4 : 8), nb = term == 2 ? 4 : 5;
        const int a2 = a1 + 13, b2 = b1 + 13;
        for (int i = 0; i < 8; ++i) s(kT + i) = 0.0;
        poly_mul_acc(s, kT, a1, na, b2, nb, 1.0);
        poly_mul_acc(s, kT, b1, nb, a2, na, -1.0);
        const int lead = term == 0 ? 0 : term == 1 ? 4 : 8, nl = term == 2 ? 5 : 4;
        poly_mul_acc(s, kP, lead, nl, kT, na + nb - 1, term == 1 ? -1.0 : 1.0);
    }

    // ---- all ten roots of det B(z) by the Ehrlich-Aberth iteration (complex, simultaneous)
    const double lead = s(kP + 10);
    if (!(fabs(lead) > 0.0) || !(fabs(lead) < 1e300)) return 0;
    {
        double big = 0.0;  // Cauchy's bound on the root magnitudes; the start circle is well inside it
        for (int i = 0; i < 10; ++i) big = fmax(big, fabs(s(kP + i) / lead));
        if (!(big < 1e300)) return 0;
        const double radius = fmin(1.0 + big, 4.0);
        double cr = 0.7648421872844885, ci = 0.644217687237691;  // angle 0.7, then steps of 36 degrees
        for (int k = 0; k < 10; ++k) {
            s(kZr + k) = radius * cr;
            s(kZi + k) = radius * ci;
            const double nr = cr * 0.8090169943749475 - ci * 0.5877852522924731;
            ci = cr * 0.5877852522924731 + ci * 0.8090169943749475;
            cr = nr;
        }
    }
    for (int it = 0; it < kEssAberthMax; ++it) {
        double step = 0.0;  // the sweep's largest relative correction
        for (int k = 0; k < 10; ++k) {
            const double zr = s(kZr + k), zi = s(kZi + k);
            double pr = lead, pi = 0.0, dr = 0.0, di = 0.0;  // Horner: p and p'
            for (int i = 9; i >= 0; --i) {
                const double ndr = (dr * zr - di * zi) + pr, ndi = (dr * zi + di * zr) + pi;
                dr = ndr;
                di = ndi;
                const double npr = (pr * zr - pi * zi) + s(kP + i), npi = pr * zi + pi * zr;
                pr = npr;
                pi = npi;
            }
            if (pr == 0.0 && pi == 0.0) continue;
            // 1 / (p' / p - sum_j 1 / (z - z_j))
            const double pn = pr * pr + pi * pi;
            double qr = (dr * pr + di * pi) / pn, qi = (di * pr - dr * pi) / pn;
            for (int j = 0; j < 10; ++j) {
                if (j == k) continue;
                const double er = zr - s(kZr + j), ei = zi - s(kZi + j), en = er * er + ei * ei;
                if (en == 0.0) continue;
                qr -= er / en;
                qi += ei / en;
            }
            const double qn = qr * qr + qi * qi;
            if (!(qn > 0.0)) continue;
            const double wr = qr / qn, wi = -qi / qn;
            if (!(fabs(wr) < 1e300) || !(fabs(wi) < 1e300)) continue;
            s(kZr + k) = zr - wr;
            s(kZi + k) = zi - wi;
            step = fmax(step, (fabs(wr) + fabs(wi)) / (fabs(zr) + fabs(zi)));
        }
        if (!(step > 1e-10)) break;  // the second pass below finishes the job
    }

    // The expanded coefficients lose digits where roots cluster (measured: roots off by 1e-3 while the rows of B(z)
    // hold to 1e-16 at the true roots), so a copy of the roots is swept again on det B(z) itself, evaluated from the
    // 3 x 3 polynomial matrix with its derivative.  Where the elimination met small pivots it is that determinant
    // which cancels and the coefficients which hold, so both sets are candidates below: a candidate that polishes to
    // a root already kept is dropped as a duplicate.
    constexpr int kYr = 100, kYi = 110;
    for (int k = 0; k < 10; ++k) {
        s(kYr + k) = s(kZr + k);
        s(kYi + k) = s(kZi + k);
    }
    double last = 1.0;
    for (int it = 0; it < kEssRefineMax; ++it) {
        double step = 0.0;
        for (int k = 0; k < 10; ++k) {
            const Cx z{s(kYr + k), s(kYi + k)};
            Cx R[3][3], D[3][3];
#pragma unroll
            for (int t = 0; t < 3; ++t)
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int o = 13 * t + 4 * c, deg = c == 2 ? 4 : 3;
                    Cx p{s(o + deg), 0.0}, d{0.0, 0.0};
                    for (int i = deg - 1; i >= 0; --i) {
                        d = cadd(cmul(d, z), p);
                        p = cmul(p, z);
                        p.r += s(o + i);
                    }
                    R[t][c] = p;
                    D[t][c] = d;
                }
            const Cx f = cdet(R[0], R[1], R[2]);
            const Cx df = cadd(cadd(cdet(D[0], R[1], R[2]), cdet(R[0], D[1], R[2])), cdet(R[0], R[1], D[2]));
            const double fn = f.r * f.r + f.i * f.i;
            if (!(fn > 0.0)) continue;
            double qr = (df.r * f.r + df.i * f.i) / fn, qi = (df.i * f.r - df.r * f.i) / fn;
            for (int j = 0; j < 10; ++j) {
                if (j == k) continue;
                const double er = z.r - s(kYr + j), ei = z.i - s(kYi + j), en = er * er + ei * ei;
                if (en == 0.0) continue;
                qr -= er / en;
                qi += ei / en;
            }
            const double qn = qr * qr + qi * qi;
            if (!(qn > 0.0)) continue;
            const double wr = qr / qn, wi = -qi / qn;
            if (!(fabs(wr) < 1e300) || !(fabs(wi) < 1e300)) continue;
            s(kYr + k) = z.r - wr;
            s(kYi + k) = z.i - wi;
            step = fmax(step, (fabs(wr) + fabs(wi)) / (fabs(z.r) + fabs(z.i)));
        }
        // converged, or small corrections that no longer shrink (the rounding floor of an ill-conditioned root)
        if (!(step > 1e-14) || (step < 1e-7 && step >= last)) break;
        last = step;
    }

    // ---- every (nearly) real root: x, y from the null vector of B(z), polish, keep what converged and is new
    int count = 0;
    for (int k = 0; k < 20 && count < kEssMaxModels; ++k) {  // store 80 .. 119: both sets, real and imaginary parts
        const int at = k < 10 ? kZr + k : kYr + k - 10;
        double z = s(at);
        if (!(fabs(s(at + 10)) <= 1e-3 * (1.0 + fabs(z)))) continue;
        double R[3][3];
#pragma unroll
        for (int t = 0; t < 3; ++t) {
            const int o = 13 * t;
            R[t][0] = ((s(o + 3) * z + s(o + 2)) * z + s(o + 1)) * z + s(o);
            R[t][1] = ((s(o + 7) * z + s(o + 6)) * z + s(o + 5)) * z + s(o + 4);
            R[t][2] = (((s(o + 12) * z + s(o + 11)) * z + s(o + 10)) * z + s(o + 9)) * z + s(o + 8);
        }
        double nx = 0.0, ny = 0.0, nz = 0.0;
#pragma unroll
        for (int t = 0; t < 3; ++t) {  // the cross product of two rows with the largest last component
            const int u = t == 2 ? 0 : t + 1;
            const double cx = R[t][1] * R[u][2] - R[t][2] * R[u][1], cy = R[t][2] * R[u][0] - R[t][0] * R[u][2],
                         cz = R[t][0] * R[u][1] - R[t][1] * R[u][0];
            if (fabs(cz) > fabs(nz)) { nx = cx; ny = cy; nz = cz; }
        }
        if (!(fabs(nz) > 0.0)) continue;
        double x = nx / nz, y = ny / nz;
        const double rho = polish(s, x, y, z);
        if (!(rho <= kEssResidualMax)) continue;
        double E[9], n2 = 0.0;
        model_at(s, x, y, z, E);
#pragma unroll
        for (int i = 0; i < 9; ++i) n2 += E[i] * E[i];
        const double inv = 1.0 / sqrt(n2);
        if (!(inv < 1e300)) continue;
#pragma unroll
        for (int i = 0; i < 9; ++i) E[i] *= inv;
        bool dup = false;
        for (int m = 0; m < count; ++m) {
            double dm = 0.0, dp = 0.0;
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                dm = fmax(dm, fabs(E[i] - out[9 * m + i]));
                dp = fmax(dp, fabs(E[i] + out[9 * m + i]));
            }
            dup = dup || fmin(dm, dp) < kEssDuplicate;
        }
        if (dup) continue;
#pragma unroll
        for (int i = 0; i < 9; ++i) out[9 * count + i] = E[i];
        ++count;
    }
    return count;
}

}  // namespace svo
