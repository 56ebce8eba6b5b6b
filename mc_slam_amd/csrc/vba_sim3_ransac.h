// vba_sim3_ransac.h -- batched Sim3 RANSAC over loop candidates on the GPU.
// Replaces, for a batch of independent candidates, the loop body of Sim3Solver::iterate (src/Sim3Solver.cpp:138-220) for a list of
// triples the caller drew: ComputeSim3 (:253-359, Horn's closed form on three pairs), CheckInliers (:363-388, the two-sided
// reprojection test of every pair) and the accept rule (:193-211).
//
// One 256-lane workgroup per candidate, ONE launch, four phases separated by workgroup barriers only (no wait on another
// workgroup, no flag in memory, no floating-point atomic; every loop is bounded by n_hyp or n_pairs):
//   A  one lane per hypothesis (lanes stride over n_hyp): Horn on the three sampled pairs.  The dominant eigenvector of the
//      symmetric 4x4 N comes from a cyclic Jacobi iteration with a fixed number of sweeps (RS_SWEEPS) over named registers: every
//      index below is a compile-time constant under a full unroll, the dominant column is selected with ?:.  The lane writes
//      sR | t of T12 and of T21 and (t, q, s) into the hypothesis record [VBA_RANSAC_HYP] of the device-only arena region.
//   B  one wave per hypothesis (waves stride over n_hyp, lanes over the pairs in chunks of 64): both projections of a pair, the
//      test err1 < max_err1 && err2 < max_err2, the count as popcount of the wave's 64-bit ballot summed into a wave-uniform
//      integer; lane 0 stores c[h].  The image points mvP1im1 / mvP2im2 are recomputed from the pairs (two divisions) and not
//      stored; the pairs of a candidate (64 B each) stay in the caches across its hypotheses, so n_pairs has no bound.
//   C  wave 0 runs iterate's accept rule over c[h] in hypothesis order, 64 counts per load, every lane identically (the counts are
//      read lane by lane into scalars), and publishes (best_inliers, best_hyp, hit) through 12 bytes of LDS.
//   D  (t, q, s) of best_hyp and of the hit go to the result record; on a hit all lanes recompute the flags of that hypothesis.
//
// A degenerate triple (a repeated index, collinear points) takes the same path as any other: 0/0 in the scale gives NaN, NaN makes
// every `<` of phase B false and the count 0, as in the reference; nothing traps and no loop depends on the data.
// The rotation is formed from the unit eigenvector directly; the reference goes through atan2 and cv::Rodrigues (:305-312), which
// is the same matrix (and the same for q and -q).  The quaternion handed out is that eigenvector with w >= 0.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"

#define RS_NT 256
#define RS_SWEEPS 8   // cyclic Jacobi sweeps over the six off-diagonal entries of N (4x4 converges quadratically: 5-6 suffice in FP64)

// one Jacobi rotation in the (P, Q) plane of the symmetric A (both triangles kept), accumulated into V (columns = eigenvectors)
template <int P, int Q>
DEVI void rs_rotate(double (&A)[4][4], double (&V)[4][4]) {
    const double apq = A[P][Q];
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
    t = (apq == 0.0) ? 0.0 : t;
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    A[P][P] -= t * apq;
    A[Q][Q] += t * apq;
    A[P][Q] = 0.0;
    A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            A[r][P] = A[P][r] = c * arp - s * arq;
            A[r][Q] = A[Q][r] = s * arp + c * arq;
        }
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

// ComputeSim3 (:253-359) on pairs i0, i1, i2 of the candidate: the record of the hypothesis
DEVI void rs_horn(const double* __restrict__ pp, int i0, int i1, int i2, int fix_scale, double* __restrict__ rec) {
    double P1[3][3], P2[3][3];   // [point][xyz]
    const int idx[3] = {i0, i1, i2};
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) {
            P1[i][k] = pp[6 * (size_t)idx[i] + k];
            P2[i][k] = pp[6 * (size_t)idx[i] + 3 + k];
        }
    double O1[3], O2[3];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        O1[k] = ((P1[0][k] + P1[1][k]) + P1[2][k]) / 3.0;
        O2[k] = ((P2[0][k] + P2[1][k]) + P2[2][k]) / 3.0;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int k = 0; k < 3; k++) { P1[i][k] -= O1[k]; P2[i][k] -= O2[k]; }
    double M[3][3];   // M = Pr2 Pr1^T
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = 0; b < 3; b++) M[a][b] = (P2[0][a] * P1[0][b] + P2[1][a] * P1[1][b]) + P2[2][a] * P1[2][b];
    double A[4][4], V[4][4];
    A[0][0] = (M[0][0] + M[1][1]) + M[2][2];
    A[0][1] = A[1][0] = M[1][2] - M[2][1];
    A[0][2] = A[2][0] = M[2][0] - M[0][2];
    A[0][3] = A[3][0] = M[0][1] - M[1][0];
    A[1][1] = (M[0][0] - M[1][1]) - M[2][2];
    A[1][2] = A[2][1] = M[0][1] + M[1][0];
    A[1][3] = A[3][1] = M[2][0] + M[0][2];
    A[2][2] = (-M[0][0] + M[1][1]) - M[2][2];
    A[2][3] = A[3][2] = M[1][2] + M[2][1];
    A[3][3] = (-M[0][0] - M[1][1]) + M[2][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sw = 0; sw < RS_SWEEPS; sw++) {
        rs_rotate<0, 1>(A, V);
        rs_rotate<0, 2>(A, V);
        rs_rotate<0, 3>(A, V);
        rs_rotate<1, 2>(A, V);
        rs_rotate<1, 3>(A, V);
        rs_rotate<2, 3>(A, V);
    }
    // the largest eigenvalue (the first one among equals) and its column of V: (w, x, y, z)
    int k = 0;
    double lam = A[0][0];
    if (A[1][1] > lam) { lam = A[1][1]; k = 1; }
    if (A[2][2] > lam) { lam = A[2][2]; k = 2; }
    if (A[3][3] > lam) { lam = A[3][3]; k = 3; }
    double e[4];
#pragma unroll
    for (int r = 0; r < 4; r++) e[r] = (k == 0) ? V[r][0] : (k == 1) ? V[r][1] : (k == 2) ? V[r][2] : V[r][3];
    const double en = sqrt((e[0] * e[0] + e[1] * e[1]) + (e[2] * e[2] + e[3] * e[3]));
    const double sg = (e[0] < 0.0) ? -1.0 : 1.0;
    const double q[4] = {sg * e[1] / en, sg * e[2] / en, sg * e[3] / en, sg * e[0] / en};   // xyzw
    double R[9];
    q2R(q, R);
    // scale (:317-334): nom = Pr1 . (R Pr2), den = |R Pr2|^2
    double s = 1.0;
    if (!fix_scale) {
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            double y[3];
            mv3(R, P2[i], y);
            nom += (P1[i][0] * y[0] + P1[i][1] * y[1]) + P1[i][2] * y[2];
            den += (y[0] * y[0] + y[1] * y[1]) + y[2] * y[2];
        }
        s = nom / den;
    }
    double RO2[3], t[3];
    mv3(R, O2, RO2);
#pragma unroll
    for (int k2 = 0; k2 < 3; k2++) t[k2] = O1[k2] - s * RO2[k2];
    const double is = 1.0 / s;
#pragma unroll
    for (int i = 0; i < 9; i++) rec[i] = s * R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) rec[9 + i] = t[i];
    double Ri[9];   // sRinv = (1 / s) R^T
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) Ri[3 * i + j] = is * R[3 * j + i];
    double ti[3];
    mv3(Ri, t, ti);
#pragma unroll
    for (int i = 0; i < 9; i++) rec[12 + i] = Ri[i];
#pragma unroll
    for (int i = 0; i < 3; i++) rec[21 + i] = -ti[i];
#pragma unroll
    for (int i = 0; i < 3; i++) rec[24 + i] = t[i];
#pragma unroll
    for (int i = 0; i < 4; i++) rec[27 + i] = q[i];
    rec[31] = s;
}

// Project (:408-437) / FromCameraToImage (:441-460): the pixel of a camera-frame point
DEVI void rs_pixel(const double* K, double X, double Y, double Z, double& u, double& v) {
    const double invz = 1.0 / Z;
    u = K[0] * (X * invz) + K[2];
    v = K[1] * (Y * invz) + K[3];
}

// CheckInliers (:371-386) of one pair under T = [sR12 | t12 | sR21 | t21]
DEVI bool rs_inlier(const double* T, const double* K1, const double* K2, const double* __restrict__ pp, const double* __restrict__ gg, size_t g) {
    const double a[3] = {pp[6 * g], pp[6 * g + 1], pp[6 * g + 2]}, b[3] = {pp[6 * g + 3], pp[6 * g + 4], pp[6 * g + 5]};
    double y[3], z[3];
    mv3(T, b, y);        // P2c in camera 1
    mv3(T + 12, a, z);   // P1c in camera 2
    double u1, v1, u2, v2, pu1, pv1, pu2, pv2;
    rs_pixel(K1, a[0], a[1], a[2], u1, v1);
    rs_pixel(K2, b[0], b[1], b[2], u2, v2);
    rs_pixel(K1, y[0] + T[9], y[1] + T[10], y[2] + T[11], pu1, pv1);
    rs_pixel(K2, z[0] + T[21], z[1] + T[22], z[2] + T[23], pu2, pv2);
    const double d1u = u1 - pu1, d1v = v1 - pv1, d2u = pu2 - u2, d2v = pv2 - v2;
    const double err1 = d1u * d1u + d1v * d1v, err2 = d2u * d2u + d2v * d2v;
    return err1 < gg[2 * g] && err2 < gg[2 * g + 1];
}

__global__ void __launch_bounds__(RS_NT) k_sim3_ransac(RansacBatch B) {
    __shared__ int sh[3];
    const RansacDesc& d = B.desc[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = d.n_pairs, nh = d.n_hyp;
    const size_t p0 = (size_t)d.pair0, h0 = (size_t)d.hyp0;
    const double* pp = B.p + 6 * p0;
    const double* gg = B.gate + 2 * p0;
    double* hyp = B.hyp + h0 * VBA_RANSAC_HYP;
    int* cnt = B.cnt + h0;
    double K1[4], K2[4];
#pragma unroll
    for (int k = 0; k < 4; k++) { K1[k] = d.K1[k]; K2[k] = d.K2[k]; }

    // ---- A: Horn, one lane per hypothesis
    for (int h = tid; h < nh; h += RS_NT) {
        const int* sp = B.sample + 3 * (h0 + (size_t)h);
        double rec[VBA_RANSAC_HYP];
        rs_horn(pp, sp[0], sp[1], sp[2], d.fix_scale, rec);
#pragma unroll
        for (int i = 0; i < VBA_RANSAC_HYP; i++) hyp[(size_t)h * VBA_RANSAC_HYP + i] = rec[i];
    }
    __syncthreads();   // the records are global data read by other waves below

    // ---- B: the inlier count of every hypothesis, one wave each
    for (int h = wave; h < nh; h += RS_NT / 64) {
        double T[24];
#pragma unroll
        for (int i = 0; i < 24; i++) T[i] = hyp[(size_t)h * VBA_RANSAC_HYP + i];
        int c = 0;
        for (int base = 0; base < n; base += 64) {
            const int i = base + lane;
            const bool in = (i < n) && rs_inlier(T, K1, K2, pp, gg, (size_t)i);
            c += __popcll(__ballot(in));
        }
        if (lane == 0) cnt[h] = c;
    }
    __syncthreads();

    // ---- C: the accept rule of iterate (:193-211) in hypothesis order, by every lane of wave 0 alike
    if (wave == 0) {
        int b = d.best_inliers, best = -1, hit = -1;
        for (int base = 0; base < nh && hit < 0; base += 64) {
            const int v = (base + lane < nh) ? cnt[base + lane] : -1;
#pragma unroll
            for (int j = 0; j < 64; j++) {
                const int cj = __builtin_amdgcn_readlane(v, j);   // -1 past the end: never >= b
                if (hit < 0 && cj >= b) {
                    b = cj;
                    best = base + j;
                    if (cj > d.min_inliers) hit = base + j;
                }
            }
        }
        if (lane == 0) { sh[0] = b; sh[1] = best; sh[2] = hit; }
    }
    __syncthreads();

    // ---- D: the result record, and the flags of the hit
    const int b = sh[0], best = sh[1], hit = sh[2];
    RansacOut& O = B.out[blockIdx.x];
    if (tid == 0) {
        O.status = VBA_OK;
        O.hit = hit;
        O.its_done = (hit >= 0) ? hit + 1 : nh;
        O.best_hyp = best;
        O.n_inliers = (hit >= 0) ? cnt[hit] : 0;
        O.best_inliers = b;
        O.pad[0] = O.pad[1] = 0;
    }
    if (tid < 8) {
        O.best_S[tid] = (best >= 0) ? hyp[(size_t)best * VBA_RANSAC_HYP + 24 + tid] : 0.0;
        O.S[tid] = (hit >= 0) ? hyp[(size_t)hit * VBA_RANSAC_HYP + 24 + tid] : 0.0;
    }
    if (hit >= 0) {
        double T[24];
#pragma unroll
        for (int i = 0; i < 24; i++) T[i] = hyp[(size_t)hit * VBA_RANSAC_HYP + i];
        for (int i = tid; i < n; i += RS_NT) B.flag[p0 + (size_t)i] = rs_inlier(T, K1, K2, pp, gg, (size_t)i) ? 1 : 0;
    }
}
