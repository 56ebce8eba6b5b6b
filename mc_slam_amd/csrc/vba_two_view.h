// vba_two_view.h -- batched monocular two-view initialisation on the GPU.
// Replaces, for a batch of frame pairs, Initializer::Initialize (src/Initializer.cpp:36-130) behind the drawing of the 8-sets:
// Normalize (:893-946), ComputeH21 (:263-305) / ComputeF21 (:320-356) of every set, CheckHomography (:362-461) / CheckFundamental
// (:465-545) of every hypothesis over all matches, the two scans (:179, :233), the model choice (:120-126), ReconstructH (:673-835)
// or ReconstructF (:555-667) with DecomposeE (:1095-1117), CheckRT (:950-1082) and Triangulate (:859-880).
//
// One 256-lane workgroup per frame pair, ONE launch, phases separated by workgroup barriers only (no wait on another workgroup, no
// flag in memory, no floating-point atomic; every loop is bounded by n_hyp, n_matches or n_keys, every reduction has a fixed shape
// that does not depend on where the pair stands in the batch):
//   N  means and mean absolute deviations of both frames' keypoints: lanes stride over the keypoints, block_sum256.
//   A  fitting: a (hypothesis, model) job per 16-lane group, four per wave, sixteen per pass.  Lane c < 9 of the group holds column c
//      of A (16x9 for H, 8x9 for F) and of V; a one-sided (Hestenes) Jacobi iteration orthogonalises the columns in TV_SWEEPS
//      round-robin sweeps of nine rounds (in round r column c meets column (r - c) mod 9: four disjoint pairs, one column idle),
//      partners exchanged with __shfl.  The column of the smallest norm (the first among equals, picked with ?:) is the null
//      vector, taken from A itself and not from A^T A.  Lane 0 of the group then forms H21 = T2^-1 Hn T1 and H12 = H21^-1, or the
//      rank-2 projection (3x3 Jacobi SVD) and F21 = T2^T Fn T1, and stores the record in the device-only arena.
//   B  scoring: waves stride over the 2 n_hyp jobs, lanes over the matches (not staged in LDS: n_matches has no bound); butterfly
//      sum; lane 0 stores the score.
//   C  the two scans in hypothesis order by two lanes (strict > against 0.0: a tie keeps the earlier one, a NaN never wins).
//   D  flags and counts of the two winners by all lanes; RH and the model; one lane decomposes H (eight Faugeras hypotheses) or E
//      (four) into LDS.
//   E  CheckRT: waves stride over the 4 or 8 (R, t), lanes over the matches; Triangulate is the 4x4 Hestenes iteration of
//      vba_triangulate.h (tr_rotate).  State, cosine and point of every (hypothesis, match) go to the device-only arena.
//   F  the order statistic min(50, nGood - 1) of the cosines by rank counting (values below, ties broken by index).
//   G  one lane decides; H  the winner's points are scattered by match[.][0] (distinct: checked on the host).
// Sign convention of the 3x3 SVD (tv_svd3): singular values descending (the first among equals first), (u_i, v_i) flipped together
// so that the largest-magnitude component of u_i (the first among equals) is positive; `complete` (DecomposeE, sigma_3 = 0):
// u_3 = u_1 x u_2, v_3 = v_1 x v_2.  DESIGN.md (f-9) shows that ok, reason, R21, t21 and the points do not depend on it.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_triangulate.h"

#define TV_NT 256
#define TV_SWEEPS 10    // round-robin sweeps over the 36 column pairs of a 9-column A
#define TV_SWEEPS3 8    // cyclic sweeps over the three column pairs of a 3x3

DEVI double tv_sel3(int k, double a0, double a1, double a2) { return (k == 0) ? a0 : (k == 1) ? a1 : a2; }
DEVI double tv_det3(const double* m) {
    return (m[0] * (m[4] * m[8] - m[5] * m[7]) - m[1] * (m[3] * m[8] - m[5] * m[6])) + m[2] * (m[3] * m[7] - m[4] * m[6]);
}
// inverse by cofactors; a singular matrix gives non-finite entries (and the hypothesis a NaN score that never wins)
DEVI void tv_inv3(const double* m, double* o) {
    const double id = 1.0 / tv_det3(m);
    o[0] = (m[4] * m[8] - m[5] * m[7]) * id; o[1] = (m[2] * m[7] - m[1] * m[8]) * id; o[2] = (m[1] * m[5] - m[2] * m[4]) * id;
    o[3] = (m[5] * m[6] - m[3] * m[8]) * id; o[4] = (m[0] * m[8] - m[2] * m[6]) * id; o[5] = (m[2] * m[3] - m[0] * m[5]) * id;
    o[6] = (m[3] * m[7] - m[4] * m[6]) * id; o[7] = (m[1] * m[6] - m[0] * m[7]) * id; o[8] = (m[0] * m[4] - m[1] * m[3]) * id;
}

template <int P, int Q>
DEVI void tv_rotate3(double (&U)[3][3], double (&V)[3][3]) {
    const double alpha = (U[0][P] * U[0][P] + U[1][P] * U[1][P]) + U[2][P] * U[2][P];
    const double beta = (U[0][Q] * U[0][Q] + U[1][Q] * U[1][Q]) + U[2][Q] * U[2][Q];
    const double gamma = (U[0][P] * U[0][Q] + U[1][P] * U[1][Q]) + U[2][P] * U[2][Q];
    const double zeta = (beta - alpha) / (2.0 * gamma);
    double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
    t = (gamma == 0.0) ? 0.0 : t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        const double up = U[r][P], uq = U[r][Q];
        U[r][P] = c * up - s * uq;
        U[r][Q] = s * up + c * uq;
        const double vp = V[r][P], vq = V[r][Q];
        V[r][P] = c * vp - s * vq;
        V[r][Q] = s * vp + c * vq;
    }
}

// SVD of the row-major 3x3 A under the convention above.  Uo / Vo: row-major, COLUMNS are u_i / v_i; w descending.  Without
// `complete` the third pair is (A v_3 / w_3, v_3) like the others; with it u_3 = u_1 x u_2, v_3 = v_1 x v_2
DEVI void tv_svd3(const double* A, bool complete, double* Uo, double* w, double* Vo) {
    double U[3][3], V[3][3];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) { U[i][j] = A[3 * i + j]; V[i][j] = (i == j) ? 1.0 : 0.0; }
#pragma unroll 1
    for (int sw = 0; sw < TV_SWEEPS3; sw++) {
        tv_rotate3<0, 1>(U, V);
        tv_rotate3<0, 2>(U, V);
        tv_rotate3<1, 2>(U, V);
    }
    double n[3];
#pragma unroll
    for (int k = 0; k < 3; k++) n[k] = (U[0][k] * U[0][k] + U[1][k] * U[1][k]) + U[2][k] * U[2][k];
    const int i0 = (n[0] >= n[1] && n[0] >= n[2]) ? 0 : (n[1] >= n[2]) ? 1 : 2;
    const int i2 = (n[2] <= n[0] && n[2] <= n[1]) ? 2 : (n[1] <= n[0]) ? 1 : 0;
    const int i1 = 3 - i0 - i2;
#pragma unroll
    for (int i = 0; i < 3; i++) {
        const int k = (i == 0) ? i0 : (i == 1) ? i1 : i2;
        const double wi = sqrt(tv_sel3(k, n[0], n[1], n[2]));
        double u[3], v[3];
#pragma unroll
        for (int r = 0; r < 3; r++) { u[r] = tv_sel3(k, U[r][0], U[r][1], U[r][2]) / wi; v[r] = tv_sel3(k, V[r][0], V[r][1], V[r][2]); }
        double big = u[0];
        if (fabs(u[1]) > fabs(big)) big = u[1];
        if (fabs(u[2]) > fabs(big)) big = u[2];
        const double sg = (big < 0.0) ? -1.0 : 1.0;
        w[i] = wi;
#pragma unroll
        for (int r = 0; r < 3; r++) { Uo[3 * r + i] = sg * u[r]; Vo[3 * r + i] = sg * v[r]; }
    }
    if (complete) {
        Uo[2] = Uo[3] * Uo[7] - Uo[6] * Uo[4]; Uo[5] = Uo[6] * Uo[1] - Uo[0] * Uo[7]; Uo[8] = Uo[0] * Uo[4] - Uo[3] * Uo[1];
        Vo[2] = Vo[3] * Vo[7] - Vo[6] * Vo[4]; Vo[5] = Vo[6] * Vo[1] - Vo[0] * Vo[7]; Vo[8] = Vo[0] * Vo[4] - Vo[3] * Vo[1];
    }
}

// the normalisation of a frame: vNormalizedPoints = (pt - mean) * s, T = [s 0 -mean s]
struct TvNorm { double mx, my, sx, sy; };

// The null vector of the NR x 9 matrix whose column c this lane holds in U (lanes c >= 9 of the 16-lane group idle): every lane of
// the group gets all nine entries.  gbase: the wave lane of the group's lane 0
template <int NR>
DEVI void tv_null9(double (&U)[NR], int c, int gbase, double (&v)[9]) {
    double V[9];
#pragma unroll
    for (int r = 0; r < 9; r++) V[r] = (r == c) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sw = 0; sw < TV_SWEEPS; sw++) {
#pragma unroll 1
        for (int rd = 0; rd < 9; rd++) {
            int p = rd - c;
            p += (p < 0) ? 9 : 0;
            const bool act = (c < 9) && (p != c);
            p = act ? p : c;
            const int src = gbase + p;
            const bool lo = c < p;   // this lane holds the column of the lower index: the "P" of the rotation
            double Up[NR], own = 0.0, part = 0.0, gamma = 0.0;
#pragma unroll
            for (int r = 0; r < NR; r++) {
                Up[r] = __shfl(U[r], src, 64);
                own += U[r] * U[r];
                part += Up[r] * Up[r];
                gamma += U[r] * Up[r];
            }
            const double alpha = lo ? own : part, beta = lo ? part : own;
            const double zeta = (beta - alpha) / (2.0 * gamma);
            double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
            t = (gamma == 0.0 || !act) ? 0.0 : t;
            const double cs = 1.0 / sqrt(t * t + 1.0), sn = t * cs;
            const double sq = lo ? -sn : sn;   // P: c up - s uq, Q: s up + c uq
#pragma unroll
            for (int r = 0; r < NR; r++) U[r] = cs * U[r] + sq * Up[r];
#pragma unroll
            for (int r = 0; r < 9; r++) {
                const double vp = __shfl(V[r], src, 64);
                V[r] = cs * V[r] + sq * vp;
            }
        }
    }
    double own = 0.0;
#pragma unroll
    for (int r = 0; r < NR; r++) own += U[r] * U[r];
    int k = 0;
    double best = __shfl(own, gbase, 64);
#pragma unroll
    for (int q = 1; q < 9; q++) {
        const double nq = __shfl(own, gbase + q, 64);
        if (nq < best) { best = nq; k = q; }
    }
#pragma unroll
    for (int r = 0; r < 9; r++) v[r] = __shfl(V[r], gbase + k, 64);
}

// CheckHomography (:399-452) of one match: the score it adds and its flag.  H: H21 (9) H12 (9)
DEVI bool tv_check_h(const double* H, double u1, double v1, double u2, double v2, double inv_s2, double& sc) {
    const double th = (double)5.991f;
    bool in = true;
    const double w2 = 1.0 / ((H[15] * u2 + H[16] * v2) + H[17]);
    const double u2in1 = ((H[9] * u2 + H[10] * v2) + H[11]) * w2, v2in1 = ((H[12] * u2 + H[13] * v2) + H[14]) * w2;
    const double chi1 = ((u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1)) * inv_s2;
    if (chi1 > th) in = false; else sc += th - chi1;
    const double w1 = 1.0 / ((H[6] * u1 + H[7] * v1) + H[8]);
    const double u1in2 = ((H[0] * u1 + H[1] * v1) + H[2]) * w1, v1in2 = ((H[3] * u1 + H[4] * v1) + H[5]) * w1;
    const double chi2 = ((u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2)) * inv_s2;
    if (chi2 > th) in = false; else sc += th - chi2;
    return in;
}

// CheckFundamental (:500-537) of one match
DEVI bool tv_check_f(const double* F, double u1, double v1, double u2, double v2, double inv_s2, double& sc) {
    const double th = (double)3.841f, th_score = (double)5.991f;
    bool in = true;
    const double a2 = (F[0] * u1 + F[1] * v1) + F[2], b2 = (F[3] * u1 + F[4] * v1) + F[5], c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const double num2 = (a2 * u2 + b2 * v2) + c2;
    const double chi1 = (num2 * num2 / (a2 * a2 + b2 * b2)) * inv_s2;
    if (chi1 > th) in = false; else sc += th_score - chi1;
    const double a1 = (F[0] * u2 + F[3] * v2) + F[6], b1 = (F[1] * u2 + F[4] * v2) + F[7], c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const double num1 = (a1 * u1 + b1 * v1) + c1;
    const double chi2 = (num1 * num1 / (a1 * a1 + b1 * b1)) * inv_s2;
    if (chi2 > th) in = false; else sc += th_score - chi2;
    return in;
}

// the body of CheckRT's loop (:1003-1064) for one inlier match: 0 rejected, 1 counted in nGood, 2 counted and cosParallax < 0.99998.
// Rt: R (9) t (3); P2: K [R | t] (12, row-major 3x4); O2 = -R^T t
DEVI int tv_check_rt(const double* Rt, const double* P2, const double* O2, const double* K, double u1, double v1, double u2, double v2,
                     double th2, double (&x)[3], double& cosp) {
    double U[4][4], V[4][4];   // A of Triangulate (:864-868) with P1 = K [I | 0]
    U[0][0] = -K[0]; U[0][1] = 0.0; U[0][2] = u1 - K[2]; U[0][3] = 0.0;
    U[1][0] = 0.0; U[1][1] = -K[1]; U[1][2] = v1 - K[3]; U[1][3] = 0.0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        U[2][j] = u2 * P2[8 + j] - P2[j];
        U[3][j] = v2 * P2[8 + j] - P2[4 + j];
    }
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sw = 0; sw < TR_SWEEPS; sw++) {
        tr_rotate<0, 1>(U, V);
        tr_rotate<0, 2>(U, V);
        tr_rotate<0, 3>(U, V);
        tr_rotate<1, 2>(U, V);
        tr_rotate<1, 3>(U, V);
        tr_rotate<2, 3>(U, V);
    }
    double s2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) s2[k] = (U[0][k] * U[0][k] + U[1][k] * U[1][k]) + (U[2][k] * U[2][k] + U[3][k] * U[3][k]);
    int k = 0;
    double lo = s2[0];
    if (s2[1] < lo) { lo = s2[1]; k = 1; }
    if (s2[2] < lo) { lo = s2[2]; k = 2; }
    if (s2[3] < lo) { lo = s2[3]; k = 3; }
    double v[4];
#pragma unroll
    for (int r = 0; r < 4; r++) v[r] = (k == 0) ? V[r][0] : (k == 1) ? V[r][1] : (k == 2) ? V[r][2] : V[r][3];
    x[0] = v[0] / v[3]; x[1] = v[1] / v[3]; x[2] = v[2] / v[3];   // :879
    if (!isfinite(x[0]) || !isfinite(x[1]) || !isfinite(x[2])) return 0;   // :1014
    const double n2[3] = {x[0] - O2[0], x[1] - O2[1], x[2] - O2[2]};
    const double dist1 = sqrt((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]), dist2 = sqrt((n2[0] * n2[0] + n2[1] * n2[1]) + n2[2] * n2[2]);
    cosp = ((x[0] * n2[0] + x[1] * n2[1]) + x[2] * n2[2]) / (dist1 * dist2);
    if (x[2] <= 0.0 && cosp < 0.99998) return 0;   // :1031
    double y[3];
    mv3(Rt, x, y);
    y[0] += Rt[9]; y[1] += Rt[10]; y[2] += Rt[11];
    if (y[2] <= 0.0 && cosp < 0.99998) return 0;   // :1038
    const double iz1 = 1.0 / x[2];
    const double e1x = (K[0] * x[0] * iz1 + K[2]) - u1, e1y = (K[1] * x[1] * iz1 + K[3]) - v1;
    if (e1x * e1x + e1y * e1y > th2) return 0;     // :1049
    const double iz2 = 1.0 / y[2];
    const double e2x = (K[0] * y[0] * iz2 + K[2]) - u2, e2y = (K[1] * y[1] * iz2 + K[3]) - v2;
    if (e2x * e2x + e2y * e2y > th2) return 0;     // :1060
    return (cosp < 0.99998) ? 2 : 1;               // :1062-1065
}

// (R, t) hypotheses of the chosen model into rt [VBA_TV_RT][12] (R row-major, t); returns how many: 4 (F), 8 (H), 0 with reason 2
DEVI int tv_decompose(bool is_h, const double* M, const double* K, double* rt, int& reason) {
    const double Km[9] = {K[0], 0.0, K[2], 0.0, K[1], K[3], 0.0, 0.0, 1.0};
    double U[9], w[3], V[9], T[9], A[9];
    if (!is_h) {   // ReconstructF (:569-576), DecomposeE (:1095-1117)
        mtm3(Km, M, T);
        mm3(T, Km, A);
        tv_svd3(A, true, U, w, V);
        double t[3] = {U[2], U[5], U[8]};
        const double tn = nrm3(t);
        t[0] /= tn; t[1] /= tn; t[2] /= tn;
        double R1[9], R2[9];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) {
                R1[3 * i + j] = (U[3 * i + 1] * V[3 * j] - U[3 * i] * V[3 * j + 1]) + U[3 * i + 2] * V[3 * j + 2];
                R2[3 * i + j] = (U[3 * i] * V[3 * j + 1] - U[3 * i + 1] * V[3 * j]) + U[3 * i + 2] * V[3 * j + 2];
            }
        const double s1 = (tv_det3(R1) < 0.0) ? -1.0 : 1.0, s2 = (tv_det3(R2) < 0.0) ? -1.0 : 1.0;
#pragma unroll
        for (int h = 0; h < 4; h++) {
#pragma unroll
            for (int i = 0; i < 9; i++) rt[12 * h + i] = (h & 1) ? s2 * R2[i] : s1 * R1[i];
#pragma unroll
            for (int i = 0; i < 3; i++) rt[12 * h + 9 + i] = (h < 2) ? t[i] : -t[i];
        }
        return 4;
    }
    // ReconstructH (:687-790): A = K^-1 H21 K
    const double Ki[9] = {1.0 / K[0], 0.0, -K[2] / K[0], 0.0, 1.0 / K[1], -K[3] / K[1], 0.0, 0.0, 1.0};
    mm3(Ki, M, T);
    mm3(T, Km, A);
    tv_svd3(A, false, U, w, V);
    double Vt[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Vt[3 * i + j] = V[3 * j + i];
    const double s = tv_det3(U) * tv_det3(Vt);
    const double d1 = w[0], d2 = w[1], d3 = w[2];
    if (d1 / d2 < 1.00001 || d2 / d3 < 1.00001) { reason = 2; return 0; }   // :699
    const double aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3)), aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));
    const double aux_st = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2), ct = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);
    const double aux_sp = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2), cp = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);
    double sU[9];
#pragma unroll
    for (int i = 0; i < 9; i++) sU[i] = s * U[i];
#pragma unroll
    for (int h = 0; h < 8; h++) {
        const int i = h & 3;
        const double x1 = (i < 2) ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
        const double sgn = (i == 0 || i == 3) ? 1.0 : -1.0;
        double Rp[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tp[3];
        if (h < 4) {
            const double st = sgn * aux_st;
            Rp[0] = ct; Rp[2] = -st; Rp[6] = st; Rp[8] = ct;
            tp[0] = x1 * (d1 - d3); tp[1] = 0.0; tp[2] = -x3 * (d1 - d3);
        } else {
            const double sp = sgn * aux_sp;
            Rp[0] = cp; Rp[2] = sp; Rp[4] = -1.0; Rp[6] = sp; Rp[8] = -cp;
            tp[0] = x1 * (d1 + d3); tp[1] = 0.0; tp[2] = x3 * (d1 + d3);
        }
        double T1[9], R[9], t[3];
        mm3(sU, Rp, T1);
        mm3(T1, Vt, R);
        mv3(U, tp, t);
        const double tn = nrm3(t);
#pragma unroll
        for (int k = 0; k < 9; k++) rt[12 * h + k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; k++) rt[12 * h + 9 + k] = t[k] / tn;
    }
    return 8;
}

__global__ void __launch_bounds__(TV_NT) k_two_view(TvBatch B) {
    __shared__ double sm4[4];
    __shared__ double s_rt[VBA_TV_RT * 12];
    __shared__ double s_par[VBA_TV_RT];
    __shared__ double s_best[2];
    __shared__ int s_good[VBA_TV_RT];
    __shared__ int s_i[8];   // best_h, best_f, model, n_rt, reason, ok, best_rt
    const TvDesc& d = B.desc[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = d.n_matches, nh = d.n_hyp, nk1 = d.n_keys1, nk2 = d.n_keys2;
    const size_t m0 = (size_t)d.match0, h0 = (size_t)d.hyp0;
    const double* uv1 = B.uv1 + 2 * (size_t)d.key1_0;
    const double* uv2 = B.uv2 + 2 * (size_t)d.key2_0;
    const int* match = B.match + 2 * m0;
    const int* sets = B.sets + 8 * h0;
    double* hyp_h = B.hyp_h + h0 * VBA_TV_HYP_H;
    double* hyp_f = B.hyp_f + h0 * VBA_TV_HYP_F;
    double* score_h = B.score_h + h0;
    double* score_f = B.score_f + h0;
    unsigned char* flag_h = B.flag_h + m0;
    unsigned char* flag_f = B.flag_f + m0;
    unsigned char* rt_state = B.rt_state + VBA_TV_RT * m0;
    double* rt_cos = B.rt_cos + VBA_TV_RT * m0;
    double* rt_x = B.rt_x + 3 * VBA_TV_RT * m0;
    double K[4];
#pragma unroll
    for (int k = 0; k < 4; k++) K[k] = d.K[k];
    const double inv_s2 = 1.0 / (d.sigma * d.sigma), th2 = 4.0 * (d.sigma * d.sigma);

    // ---- N: Normalize (:893-946) of both frames
    TvNorm N1, N2;
    {
        double a = 0.0, b = 0.0, c = 0.0, e = 0.0;
        for (int i = tid; i < nk1; i += TV_NT) { a += uv1[2 * i]; b += uv1[2 * i + 1]; }
        for (int i = tid; i < nk2; i += TV_NT) { c += uv2[2 * i]; e += uv2[2 * i + 1]; }
        N1.mx = block_sum256(a, sm4) / nk1; N1.my = block_sum256(b, sm4) / nk1;
        N2.mx = block_sum256(c, sm4) / nk2; N2.my = block_sum256(e, sm4) / nk2;
        a = b = c = e = 0.0;
        for (int i = tid; i < nk1; i += TV_NT) { a += fabs(uv1[2 * i] - N1.mx); b += fabs(uv1[2 * i + 1] - N1.my); }
        for (int i = tid; i < nk2; i += TV_NT) { c += fabs(uv2[2 * i] - N2.mx); e += fabs(uv2[2 * i + 1] - N2.my); }
        N1.sx = 1.0 / (block_sum256(a, sm4) / nk1); N1.sy = 1.0 / (block_sum256(b, sm4) / nk1);
        N2.sx = 1.0 / (block_sum256(c, sm4) / nk2); N2.sy = 1.0 / (block_sum256(e, sm4) / nk2);
    }

    // ---- A: fitting, one (hypothesis, model) job per 16-lane group: jobs [0, nh) are H, [nh, 2 nh) are F
    {
        const int c = tid & 15, gbase = lane & 48, grp = tid >> 4;
        const int cm = (c < 9) ? c % 3 : 0, cg = (c < 9) ? c / 3 : 3;   // column c = 3 cg + cm; cg = 3: an idle lane, a zero column
        for (int j0 = 0; j0 < 2 * nh; j0 += TV_NT / 16) {
            const int j = j0 + grp;
            if (j < 2 * nh) {
                const bool is_h = j < nh;
                const int h = is_h ? j : j - nh;
                const int* sp = sets + 8 * (size_t)h;
                double v[9];
                if (is_h) {
                    double U[16];
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const int m = sp[i], k1 = match[2 * m], k2 = match[2 * m + 1];
                        const double u1 = (uv1[2 * k1] - N1.mx) * N1.sx, v1 = (uv1[2 * k1 + 1] - N1.my) * N1.sy;
                        const double u2 = (uv2[2 * k2] - N2.mx) * N2.sx, v2 = (uv2[2 * k2 + 1] - N2.my) * N2.sy;
                        const double b = (cm == 0) ? u1 : (cm == 1) ? v1 : 1.0;
                        U[2 * i] = (cg == 1) ? -b : (cg == 2) ? v2 * b : 0.0;       // :277-285
                        U[2 * i + 1] = (cg == 0) ? b : (cg == 2) ? -u2 * b : 0.0;   // :288-296
                    }
                    tv_null9<16>(U, c, gbase, v);
                } else {
                    double U[8];
#pragma unroll
                    for (int i = 0; i < 8; i++) {
                        const int m = sp[i], k1 = match[2 * m], k2 = match[2 * m + 1];
                        const double u1 = (uv1[2 * k1] - N1.mx) * N1.sx, v1 = (uv1[2 * k1 + 1] - N1.my) * N1.sy;
                        const double u2 = (uv2[2 * k2] - N2.mx) * N2.sx, v2 = (uv2[2 * k2 + 1] - N2.my) * N2.sy;
                        const double b = (cm == 0) ? u1 : (cm == 1) ? v1 : 1.0;
                        U[i] = (cg == 0) ? u2 * b : (cg == 1) ? v2 * b : (cg == 2) ? b : 0.0;   // :333-341
                    }
                    tv_null9<8>(U, c, gbase, v);
                }
                if (c == 0) {
                    const double T1[9] = {N1.sx, 0.0, -N1.mx * N1.sx, 0.0, N1.sy, -N1.my * N1.sy, 0.0, 0.0, 1.0};
                    double X[9], Y[9];
                    if (is_h) {   // H21 = T2inv Hn T1, H12 = H21^-1 (:172-173)
                        const double T2i[9] = {1.0 / N2.sx, 0.0, N2.mx, 0.0, 1.0 / N2.sy, N2.my, 0.0, 0.0, 1.0};
                        mm3(T2i, v, X);
                        mm3(X, T1, Y);
                        tv_inv3(Y, X);
                        double* rec = hyp_h + (size_t)h * VBA_TV_HYP_H;
#pragma unroll
                        for (int i = 0; i < 9; i++) { rec[i] = Y[i]; rec[9 + i] = X[i]; }
                    } else {      // the rank-2 projection (:350-354), F21 = T2^T Fn T1 (:228)
                        const double T2[9] = {N2.sx, 0.0, -N2.mx * N2.sx, 0.0, N2.sy, -N2.my * N2.sy, 0.0, 0.0, 1.0};
                        double Us[9], w[3], Vs[9];
                        tv_svd3(v, false, Us, w, Vs);
#pragma unroll
                        for (int i = 0; i < 3; i++)
#pragma unroll
                            for (int q = 0; q < 3; q++) X[3 * i + q] = (Us[3 * i] * w[0]) * Vs[3 * q] + (Us[3 * i + 1] * w[1]) * Vs[3 * q + 1];
                        mtm3(T2, X, Y);
                        mm3(Y, T1, X);
                        double* rec = hyp_f + (size_t)h * VBA_TV_HYP_F;
#pragma unroll
                        for (int i = 0; i < 9; i++) rec[i] = X[i];
                    }
                }
            }
        }
    }
    __syncthreads();   // the records are global data read by other waves below

    // ---- B: the score of every hypothesis, one wave per (hypothesis, model)
    for (int j = wave; j < 2 * nh; j += TV_NT / 64) {
        const bool is_h = j < nh;
        const int h = is_h ? j : j - nh;
        double M[18];
#pragma unroll
        for (int i = 0; i < 18; i++) M[i] = is_h ? hyp_h[(size_t)h * VBA_TV_HYP_H + i] : (i < 9) ? hyp_f[(size_t)h * VBA_TV_HYP_F + i] : 0.0;
        double sc = 0.0;
        for (int i = lane; i < n; i += 64) {
            const int k1 = match[2 * i], k2 = match[2 * i + 1];
            const double u1 = uv1[2 * k1], v1 = uv1[2 * k1 + 1], u2 = uv2[2 * k2], v2 = uv2[2 * k2 + 1];
            if (is_h) tv_check_h(M, u1, v1, u2, v2, inv_s2, sc);
            else tv_check_f(M, u1, v1, u2, v2, inv_s2, sc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) sc += __shfl_xor(sc, o, 64);
        if (lane == 0) (is_h ? score_h : score_f)[h] = sc;
    }
    __syncthreads();

    // ---- C: the scans (:179, :233) in hypothesis order: lane 0 over H, lane 1 over F
    if (tid < 2) {
        const double* sc = (tid == 0) ? score_h : score_f;
        double best = 0.0;
        int bi = -1;
        for (int h = 0; h < nh; h++) {
            const double s = sc[h];
            if (s > best) { best = s; bi = h; }
        }
        s_best[tid] = best;
        s_i[tid] = bi;
    }
    __syncthreads();

    // ---- D: flags and counts of the two winners, RH, the model, its (R, t) hypotheses
    const int best_h = s_i[0], best_f = s_i[1];
    const double SH = s_best[0], SF = s_best[1];
    double MH[18], MF[9];
#pragma unroll
    for (int i = 0; i < 18; i++) MH[i] = (best_h >= 0) ? hyp_h[(size_t)best_h * VBA_TV_HYP_H + i] : 0.0;
#pragma unroll
    for (int i = 0; i < 9; i++) MF[i] = (best_f >= 0) ? hyp_f[(size_t)best_f * VBA_TV_HYP_F + i] : 0.0;
    int n_in_h, n_in_f;
    {
        double ch = 0.0, cf = 0.0, dummy = 0.0;
        for (int i = tid; i < n; i += TV_NT) {
            const int k1 = match[2 * i], k2 = match[2 * i + 1];
            const double u1 = uv1[2 * k1], v1 = uv1[2 * k1 + 1], u2 = uv2[2 * k2], v2 = uv2[2 * k2 + 1];
            const bool ih = (best_h >= 0) && tv_check_h(MH, u1, v1, u2, v2, inv_s2, dummy);
            const bool jf = (best_f >= 0) && tv_check_f(MF, u1, v1, u2, v2, inv_s2, dummy);
            flag_h[i] = ih ? 1 : 0;
            flag_f[i] = jf ? 1 : 0;
            ch += ih ? 1.0 : 0.0;
            cf += jf ? 1.0 : 0.0;
        }
        n_in_h = (int)block_sum256(ch, sm4);   // whole numbers: exact
        n_in_f = (int)block_sum256(cf, sm4);
    }
    const double RH = SH / (SH + SF);
    const bool is_h = RH > 0.40;   // a NaN goes to F (:123)
    const int N_in = is_h ? n_in_h : n_in_f;
    if (tid == 0) {
        int reason = 0, n_rt = 0;
        if ((is_h ? best_h : best_f) < 0) reason = 1;
        else n_rt = tv_decompose(is_h, is_h ? MH : MF, K, s_rt, reason);
        s_i[3] = n_rt;
        s_i[4] = reason;
    }
#pragma unroll
    for (int k = tid; k < VBA_TV_RT; k += TV_NT) { s_good[k] = 0; s_par[k] = 0.0; }
    __syncthreads();   // also: the flags are global data read by other lanes below
    const int n_rt = s_i[3];
    const unsigned char* flag = is_h ? flag_h : flag_f;

    // ---- E: CheckRT (:950-1082) of every (R, t), one wave each
    for (int k = wave; k < n_rt; k += TV_NT / 64) {
        double Rt[12], P2[12], O2[3];
#pragma unroll
        for (int i = 0; i < 12; i++) Rt[i] = s_rt[12 * k + i];
#pragma unroll
        for (int q = 0; q < 4; q++) {   // P2 = K [R | t] (:982-985)
            const double r0 = (q < 3) ? Rt[q] : Rt[9], r1 = (q < 3) ? Rt[3 + q] : Rt[10], r2 = (q < 3) ? Rt[6 + q] : Rt[11];
            P2[q] = K[0] * r0 + K[2] * r2;
            P2[4 + q] = K[1] * r1 + K[3] * r2;
            P2[8 + q] = r2;
        }
        mtv3(Rt, Rt + 9, O2);           // O2 = -R^T t (:987)
        O2[0] = -O2[0]; O2[1] = -O2[1]; O2[2] = -O2[2];
        int good = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            int st = 0;
            if (i < n && flag[i]) {
                const int k1 = match[2 * i], k2 = match[2 * i + 1];
                double x[3], cosp = 0.0;
                st = tv_check_rt(Rt, P2, O2, K, uv1[2 * k1], uv1[2 * k1 + 1], uv2[2 * k2], uv2[2 * k2 + 1], th2, x, cosp);
                const size_t g = (size_t)k * (size_t)n + (size_t)i;
                rt_cos[g] = cosp;
                rt_x[3 * g] = x[0]; rt_x[3 * g + 1] = x[1]; rt_x[3 * g + 2] = x[2];
            }
            if (i < n) rt_state[(size_t)k * (size_t)n + (size_t)i] = (unsigned char)st;
            good += __popcll(__ballot(st != 0));
        }
        if (lane == 0) s_good[k] = good;
    }
    __syncthreads();

    // ---- F: parallax = acos of the element min(50, nGood - 1) of the ascending cosines (:1067-1079), by rank counting
    for (int k = wave; k < n_rt; k += TV_NT / 64) {
        const int ng = s_good[k];
        if (ng > 0) {
            const int want = (ng - 1 < 50) ? ng - 1 : 50;
            const unsigned char* st = rt_state + (size_t)k * (size_t)n;
            const double* cs = rt_cos + (size_t)k * (size_t)n;
            for (int i = lane; i < n; i += 64) {
                if (!st[i]) continue;
                const double ci = cs[i];
                int rank = 0;
                for (int q = 0; q < n; q++) {
                    if (!st[q]) continue;
                    const double cq = cs[q];
                    rank += (cq < ci || (cq == ci && q < i)) ? 1 : 0;
                }
                if (rank == want) s_par[k] = acos(ci) * 180.0 / 3.14159265358979323846;
            }
        }
    }
    __syncthreads();

    // ---- G: the decision (:590-667, :793-835) and the result record
    if (tid == 0) {
        int reason = s_i[4], ok = 0, best_rt = -1;
        if (reason == 0 && !is_h) {
            int max_good = 0;
            for (int k = 0; k < 4; k++) max_good = (s_good[k] > max_good) ? s_good[k] : max_good;
            const int n90 = (int)(0.9 * N_in);
            const int n_min_good = (n90 > d.min_triangulated) ? n90 : d.min_triangulated;
            int nsimilar = 0;
            for (int k = 0; k < 4; k++) nsimilar += ((double)s_good[k] > 0.7 * max_good) ? 1 : 0;
            if (max_good < n_min_good || nsimilar > 1) reason = 4;
            else {
                int k = 0;
                while (k < 3 && s_good[k] != max_good) k++;   // the if / else-if chain: the first hypothesis with maxGood
                if (s_par[k] > d.min_parallax) { ok = 1; best_rt = k; }
                else reason = 5;
            }
        } else if (reason == 0) {
            int best_good = 0, second = 0, bi = -1;
            double best_par = -1.0;
            for (int k = 0; k < 8; k++) {
                const int g = s_good[k];
                if (g > best_good) { second = best_good; best_good = g; bi = k; best_par = s_par[k]; }
                else if (g > second) second = g;
            }
            if ((double)second < 0.75 * best_good && best_par >= d.min_parallax && best_good > d.min_triangulated && (double)best_good > 0.9 * N_in) {
                ok = 1;
                best_rt = bi;
            } else reason = 3;
        }
        s_i[5] = ok;
        s_i[6] = best_rt;
        TvOut& O = B.out[blockIdx.x];
        O.status = VBA_OK; O.ok = ok; O.model = is_h ? 1 : 2; O.reason = reason;
        O.best_hyp_h = best_h; O.best_hyp_f = best_f; O.n_inliers_h = n_in_h; O.n_inliers_f = n_in_f;
        O.n_rt = n_rt; O.best_rt = best_rt;
        for (int k = 0; k < VBA_TV_RT; k++) { O.rt_good[k] = (k < n_rt) ? s_good[k] : 0; O.rt_parallax[k] = (k < n_rt) ? s_par[k] : 0.0; }
        O.score_h = SH; O.score_f = SF; O.rh = RH;
        for (int i = 0; i < 9; i++) { O.H21[i] = MH[i]; O.F21[i] = MF[i]; }
        for (int i = 0; i < 9; i++) O.R21[i] = (best_rt >= 0) ? s_rt[12 * best_rt + i] : 0.0;
        for (int i = 0; i < 3; i++) O.t21[i] = (best_rt >= 0) ? s_rt[12 * best_rt + 9 + i] : 0.0;
    }
    __syncthreads();

    // ---- H: vP3D / vbTriangulated of the winner, scattered by match[.][0] (distinct within a pair)
    if (!s_i[5]) return;
    const int win = s_i[6];
    double* x3d = B.x3d + 3 * (size_t)d.key1_0;
    unsigned char* tri = B.tri + (size_t)d.key1_0;
    for (int i = tid; i < nk1; i += TV_NT) { x3d[3 * i] = 0.0; x3d[3 * i + 1] = 0.0; x3d[3 * i + 2] = 0.0; tri[i] = 0; }
    __syncthreads();
    for (int i = tid; i < n; i += TV_NT) {
        const size_t g = (size_t)win * (size_t)n + (size_t)i;
        const int st = rt_state[g];
        if (st) {
            const int k1 = match[2 * i];
            x3d[3 * k1] = rt_x[3 * g]; x3d[3 * k1 + 1] = rt_x[3 * g + 1]; x3d[3 * k1 + 2] = rt_x[3 * g + 2];
            tri[k1] = (st == 2) ? 1 : 0;
        }
    }
}
