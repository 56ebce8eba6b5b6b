// vba_triangulate.h -- batched two-view triangulation of new map points on the GPU.
// Replaces, for a batch of keyframe pairs, the per-match loop body of LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:
// 1358-1517, monocular): rays and parallax gate, linear triangulation (the right singular vector of the smallest singular value of
// the 4x4 A), two depth tests, two chi-square reprojection tests, scale consistency.  The reason codes are those of
// include/vislam_ba.h, numbered in the order of the reference's `continue`s.
//
// One lane per match, 256-lane workgroups, ONE launch.  Every workgroup belongs to exactly one pair: the host lays out the
// block-to-pair map (TriBlock: the pair and the first match of the workgroup inside it), pairs without matches get no workgroup.
// The pair's constants (41 doubles: both poses, centres and intrinsics, the three thresholds) and its level tables are staged once
// per workgroup into LDS and read from there at workgroup-uniform addresses (broadcast reads).  The four pixel coordinates of a
// match are one 32-byte record read as two 16-byte loads, its two octaves one 2-byte load.  No atomics, no communication between
// workgroups, one barrier (after the staging); a lane's arithmetic reads nothing but its own match and its pair's constants, so
// its outputs do not depend on where the pair stands in the batch.
//
// The singular vector comes from A itself: a one-sided (Hestenes) Jacobi iteration over A's four columns, TR_SWEEPS cyclic sweeps
// of six plane rotations over named registers (every index below is a compile-time constant; the column of the smallest norm is
// selected with ?:).  A's fourth column scales with |t|, so the eigenvector of A^T A would lose (sigma1 / sigma3)^2 * eps.
// x3D = v[0..2] / v[3] is the same for v and -v, so no sign convention is needed.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"

#define TR_NT VBA_TRI_NT
#define TR_SWEEPS 8   // cyclic sweeps over the six column pairs (4 columns converge quadratically: 5-6 suffice in FP64)

// one rotation in the plane of columns P, Q of U that makes them orthogonal, accumulated into V (columns = right singular vectors)
template <int P, int Q>
DEVI void tr_rotate(double (&U)[4][4], double (&V)[4][4]) {
    const double alpha = (U[0][P] * U[0][P] + U[1][P] * U[1][P]) + (U[2][P] * U[2][P] + U[3][P] * U[3][P]);
    const double beta = (U[0][Q] * U[0][Q] + U[1][Q] * U[1][Q]) + (U[2][Q] * U[2][Q] + U[3][Q] * U[3][Q]);
    const double gamma = (U[0][P] * U[0][Q] + U[1][P] * U[1][Q]) + (U[2][P] * U[2][Q] + U[3][P] * U[3][Q]);
    const double zeta = (beta - alpha) / (2.0 * gamma);
    double t = copysign(1.0, zeta) / (fabs(zeta) + sqrt(zeta * zeta + 1.0));
    t = (gamma == 0.0) ? 0.0 : t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const double up = U[r][P], uq = U[r][Q];
        U[r][P] = c * up - s * uq;
        U[r][Q] = s * up + c * uq;
        const double vp = V[r][P], vq = V[r][Q];
        V[r][P] = c * vp - s * vq;
        V[r][Q] = s * vp + c * vq;
    }
}

// offsets of a pair's constants in TriDesc::c (and in the LDS copy)
#define TR_R1 0
#define TR_T1 9
#define TR_O1 12
#define TR_K1 15
#define TR_R2 19
#define TR_T2 28
#define TR_O2 31
#define TR_K2 34
#define TR_RATIO 38
#define TR_COS 39
#define TR_CHI2 40

DEVI double tr_dot3(const double* r, const double* x) { return (r[0] * x[0] + r[1] * x[1]) + r[2] * x[2]; }

// squared reprojection error of x in the keyframe whose constants start at R / t / K against the pixel (u, v), and the depth z
DEVI double tr_reproj(const double* R, const double* t, const double* K, const double* x, double z, double u, double v) {
    const double xc = tr_dot3(R, x) + t[0], yc = tr_dot3(R + 3, x) + t[1];
    const double invz = 1.0 / z;
    const double ex = (K[0] * xc * invz + K[2]) - u, ey = (K[1] * yc * invz + K[3]) - v;
    return ex * ex + ey * ey;
}

// one match (:1358-1517): the reason, and x3D where the reference had one.  c: the pair's constants, sg1 / sc1 / sg2 / sc2: its
// level tables (all in LDS)
DEVI int tr_match(const double* c, const double* sg1, const double* sc1, const double* sg2, const double* sc2, double u1, double v1,
                  double u2, double v2, int o1, int o2, double (&x)[3]) {
    const double xn1[3] = {(u1 - c[TR_K1 + 2]) * (1.0 / c[TR_K1]), (v1 - c[TR_K1 + 3]) * (1.0 / c[TR_K1 + 1]), 1.0};
    const double xn2[3] = {(u2 - c[TR_K2 + 2]) * (1.0 / c[TR_K2]), (v2 - c[TR_K2 + 3]) * (1.0 / c[TR_K2 + 1]), 1.0};
    double ray1[3], ray2[3];   // Rwc * xn = Rcw^T xn (:1364-1365)
#pragma unroll
    for (int k = 0; k < 3; k++) {
        ray1[k] = (c[TR_R1 + k] * xn1[0] + c[TR_R1 + 3 + k] * xn1[1]) + c[TR_R1 + 6 + k] * xn1[2];
        ray2[k] = (c[TR_R2 + k] * xn2[0] + c[TR_R2 + 3 + k] * xn2[1]) + c[TR_R2 + 6 + k] * xn2[2];
    }
    const double cosp = tr_dot3(ray1, ray2) / (sqrt(tr_dot3(ray1, ray1)) * sqrt(tr_dot3(ray2, ray2)));
    if (!(cosp > 0.0 && cosp < c[TR_COS])) return 1;   // :1389, :1423 (a NaN lands here)
    double U[4][4], V[4][4];   // A (:1393-1397), Tcw = [Rcw | tcw]
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const double a0 = (j < 3) ? c[TR_R1 + j] : c[TR_T1], a1 = (j < 3) ? c[TR_R1 + 3 + j] : c[TR_T1 + 1], a2 = (j < 3) ? c[TR_R1 + 6 + j] : c[TR_T1 + 2];
        const double b0 = (j < 3) ? c[TR_R2 + j] : c[TR_T2], b1 = (j < 3) ? c[TR_R2 + 3 + j] : c[TR_T2 + 1], b2 = (j < 3) ? c[TR_R2 + 6 + j] : c[TR_T2 + 2];
        U[0][j] = xn1[0] * a2 - a0;
        U[1][j] = xn1[1] * a2 - a1;
        U[2][j] = xn2[0] * b2 - b0;
        U[3][j] = xn2[1] * b2 - b1;
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
    // the smallest singular value (the first one among equals) and its column of V
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
    if (v[3] == 0.0) return 2;                           // :1404
    x[0] = v[0] / v[3]; x[1] = v[1] / v[3]; x[2] = v[2] / v[3];   // :1408
    const double z1 = tr_dot3(c + TR_R1 + 6, x) + c[TR_T1 + 2];
    if (z1 <= 0.0) return 3;                             // :1429
    const double z2 = tr_dot3(c + TR_R2 + 6, x) + c[TR_T2 + 2];
    if (z2 <= 0.0) return 4;                             // :1433
    if (tr_reproj(c + TR_R1, c + TR_T1, c + TR_K1, x, z1, u1, v1) > c[TR_CHI2] * sg1[o1]) return 5;   // :1450
    if (tr_reproj(c + TR_R2, c + TR_T2, c + TR_K2, x, z2, u2, v2) > c[TR_CHI2] * sg2[o2]) return 6;   // :1479
    const double n1[3] = {x[0] - c[TR_O1], x[1] - c[TR_O1 + 1], x[2] - c[TR_O1 + 2]};
    const double n2[3] = {x[0] - c[TR_O2], x[1] - c[TR_O2 + 1], x[2] - c[TR_O2 + 2]};
    const double dist1 = sqrt(tr_dot3(n1, n1)), dist2 = sqrt(tr_dot3(n2, n2));
    if (dist1 == 0.0 || dist2 == 0.0) return 7;          // :1505
    const double ratio_dist = dist2 / dist1, ratio_oct = sc1[o1] / sc2[o2], rf = c[TR_RATIO];
    if (ratio_dist * rf < ratio_oct || ratio_dist > ratio_oct * rf) return 8;   // :1516
    return 0;
}

__global__ void __launch_bounds__(TR_NT) k_triangulate(TriBatch B) {
    __shared__ double sc[VBA_TRI_CONST];
    __shared__ double slev[4 * VBA_TRI_LEVELS];
    const TriBlock b = B.blk[blockIdx.x];
    const TriDesc& d = B.desc[b.pair];
    const int tid = threadIdx.x;
    const int nl1 = d.n_levels1, nl2 = d.n_levels2;     // 1 .. VBA_TRI_LEVELS each (checked on the host)
    if (tid < VBA_TRI_CONST) sc[tid] = d.c[tid];
    if (tid < 2 * (nl1 + nl2)) slev[tid] = B.lev[(size_t)d.lev0 + tid];
    __syncthreads();
    const int i = b.first + tid;
    if (i >= d.n_matches) return;
    const size_t g = (size_t)d.match0 + (size_t)i;
    const double2 p1 = reinterpret_cast<const double2*>(B.uv)[2 * g], p2 = reinterpret_cast<const double2*>(B.uv)[2 * g + 1];
    const uchar2 oc = reinterpret_cast<const uchar2*>(B.oct)[g];
    double x[3] = {0.0, 0.0, 0.0};
    const int reason = tr_match(sc, slev, slev + nl1, slev + 2 * nl1, slev + 2 * nl1 + nl2, p1.x, p1.y, p2.x, p2.y, oc.x, oc.y, x);
    const bool has_point = reason != 1 && reason != 2;
    B.x3d[3 * g] = has_point ? x[0] : 0.0;
    B.x3d[3 * g + 1] = has_point ? x[1] : 0.0;
    B.x3d[3 * g + 2] = has_point ? x[2] : 0.0;
    B.reason[g] = (unsigned char)reason;
}
