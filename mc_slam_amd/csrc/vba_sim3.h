// vba_sim3.h -- batched loop-closure Sim3 refinement on the GPU.
// Replaces, for a batch of independent loop candidates, what Optimizer::OptimizeSim3 (src/Optimizer.cpp:4579-4785) runs between its
// edge set-up and its write-back: optimize(5) with Levenberg-Marquardt (levenberg.cpp:61-164) on the 7-dimensional Sim3 vertex
// (types_seven_dof_expmap.h:48-94), the chi2 > th2 test of both edges of every pair (:4728-4746), the "fewer than 10 left" exit
// (:4755), optimize(10 or 5) on the survivors and the final inlier count (:4762-4778).
//
// One 64-lane workgroup per candidate, the whole protocol in ONE launch, no LDS: the estimate (q, t, s), the 7x7 system and every
// LM scalar live in registers of every lane.  Lanes stride over the pairs and accumulate the 28 + 7 entries of H and b and the cost
// in constant-indexed arrays; a fixed xor butterfly (s3_lane_sum; po_wave_sum for the scalars) leaves the same sums in every lane, so the LDL^T solve, the
// manifold update and every accept / reject decision are computed redundantly and identically by all lanes (wave-uniform control
// flow), and the result of a candidate does not depend on what else is in the batch.  No floating-point atomics.
//
// Jacobians are analytic (the reference differentiates both edges numerically, base_binary_edge.hpp:147-148): with y = S.map(P2c),
// z = S^-1.map(P1c), update S <- exp(d) S, d = (omega, upsilon, sigma):
//     J12 = -dpi(y) [ -[y]x | I | y ]            J21 = +dpi(z) (R^T / s) [ -[P1c]x | I | P1c ]
//
// chi2 of an edge, as g2o's chi2() gives it, comes from the error STORED at the last computeActiveErrors -- after a rejected last
// trial that is the error of the rejected estimate, not of the restored one.  The kernel keeps the two chi2 of every pair in a
// global scratch array of the arena (Sim3Batch::c), rewritten by every evaluation over the active pairs; the outlier tests read them.
// Lane l is the only reader and writer of the entries of pairs l, l + 64, ...: no synchronisation is needed.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_pose.h"   // po_wave_sum

struct Sim3State { double q[4], t[3], s; };

// Sum over the wave that leaves the SAME bits in every lane without a closing broadcast: the 16 lanes of a row by data-parallel-
// primitive moves (row16_sum: plain VALU work), the four rows by two xor exchanges.  Every step adds a lane's value and its
// partner's; IEEE addition commutes, so both partners hold the same bits after it, and after six steps all 64 lanes do.  The 35
// sums of the system stay in vector registers this way; broadcast through scalar reads (po_wave_sum) they would occupy 70 scalar
// registers at once and the compiler would have to spill them.  Needs all 64 lanes active, which holds wherever it is called
// (outside the per-pair loops; every other branch of the kernel is wave-uniform).
DEVI double s3_lane_sum(double v) {
    v = row16_sum(v);
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    return v;
}

// sin(theta), cos(theta), exp(sigma) of one update.  Kept out of line on purpose: inlined into the LM loop, the argument
// reduction and the polynomial constants of the three functions cost the kernel its last scalar registers (the compiler then
// spills scalars into vector lanes); called, they take and return plain registers and need no stack.
__device__ __noinline__ d4_t s3_trig(double theta, double sigma) {
    double sn, cs;
    sincos(theta, &sn, &cs);
    d4_t r = {sn, cs, exp(sigma), 0.0};
    return r;
}

struct Sim3Step { double x[7]; };
DEVI Sim3State s3_oplus(Sim3State S, Sim3Step u, int fix_scale) {
    const double* x = u.x;
    const double om[3] = {x[0], x[1], x[2]}, up[3] = {x[3], x[4], x[5]};
    const double sigma = fix_scale ? 0.0 : x[6];   // VertexSim3Expmap::oplusImpl: update[6] = 0
    const double theta = nrm3(om);
    double Om[9], Om2[9], R[9];
    hat3(om, Om);
    mm3(Om, Om, Om2);
    const d4_t tr = s3_trig(theta, sigma);
    const double sn = tr.x, cs = tr.y, s = tr.z;
    const double eps = 0.00001;
    double A, B, C;
    double r1 = 1.0, r2 = 1.0;   // R = I + r1 Omega + r2 Omega^2
    if (fabs(sigma) < eps) {
        C = 1;
        if (theta < eps) {
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta2 = theta * theta;
            A = (1 - cs) / theta2;
            B = (theta - sn) / (theta2 * theta);
            r1 = sn / theta;
            r2 = (1 - cs) / (theta * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (theta < eps) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            r1 = sn / theta;
            r2 = (1 - cs) / (theta * theta);
            const double a = s * sn, b = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
#pragma unroll
    for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + r1 * Om[i] + r2 * Om2[i];
    double qd[4], td[3], W[9];
    R2q(R, qd);
    qnorm(qd);
#pragma unroll
    for (int i = 0; i < 9; i++) W[i] = A * Om[i] + B * Om2[i] + ((i % 4 == 0) ? C : 0.0);
    mv3(W, up, td);
    // ret.r = r * other.r; ret.t = s * (r * other.t) + t; ret.s = s * other.s
    double qn[4], Rd[9], rt[3];
    qmul(qd, S.q, qn);
    q2R(qd, Rd);
    mv3(Rd, S.t, rt);
    Sim3State N;
#pragma unroll
    for (int k = 0; k < 4; k++) N.q[k] = qn[k];
#pragma unroll
    for (int k = 0; k < 3; k++) N.t[k] = s * rt[k] + td[k];
    N.s = s * S.s;
    return N;
}

// what every evaluation needs of the estimate: R, s, t and the inverse's translation (Sim3::inverse, sim3.h:233-236)
struct Sim3Map { double R[9], t[3], ti[3], s, is; };
DEVI void s3_map(const Sim3State& S, Sim3Map& m) {
    q2R(S.q, m.R);
    m.s = S.s;
    m.is = 1.0 / S.s;
#pragma unroll
    for (int k = 0; k < 3; k++) m.t[k] = S.t[k];
    const double mt[3] = {(-1.0 / S.s) * S.t[0], (-1.0 / S.s) * S.t[1], (-1.0 / S.s) * S.t[2]};
    mtv3(m.R, mt, m.ti);
}

// both computeError() of pair g (types_seven_dof_expmap.h:138-167): y, z, e12, e21
DEVI void s3_pair(const Sim3Batch& B, const Sim3Desc& d, const Sim3Map& m, size_t g, double* y, double* z, double* e12, double* e21) {
    const double P1[3] = {B.p[6 * g], B.p[6 * g + 1], B.p[6 * g + 2]};
    const double P2[3] = {B.p[6 * g + 3], B.p[6 * g + 4], B.p[6 * g + 5]};
    double r[3];
    mv3(m.R, P2, r);
#pragma unroll
    for (int k = 0; k < 3; k++) y[k] = m.s * r[k] + m.t[k];
    mtv3(m.R, P1, r);
#pragma unroll
    for (int k = 0; k < 3; k++) z[k] = m.is * r[k] + m.ti[k];
    e12[0] = B.uv[4 * g] - (y[0] / y[2] * d.K1[0] + d.K1[2]);
    e12[1] = B.uv[4 * g + 1] - (y[1] / y[2] * d.K1[1] + d.K1[3]);
    e21[0] = B.uv[4 * g + 2] - (z[0] / z[2] * d.K2[0] + d.K2[2]);
    e21[1] = B.uv[4 * g + 3] - (z[1] / z[2] * d.K2[1] + d.K2[3]);
}

// computeActiveErrors + activeRobustChi2 (Huber on every active edge); stores the chi2 of both edges of every active pair
DEVI double s3_errors(const Sim3Batch& B, const Sim3Desc& d, const Sim3State& S) {
    Sim3Map m;
    s3_map(S, m);
    double chi = 0.0;
    for (int i = threadIdx.x; i < d.n_pairs; i += 64) {
        const size_t g = (size_t)d.pair0 + i;
        if (B.flag[g]) continue;
        double y[3], z[3], e12[2], e21[2], w;
        s3_pair(B, d, m, g, y, z, e12, e21);
        const double w1 = B.w[2 * g], w2 = B.w[2 * g + 1];
        const double c12 = e12[0] * (w1 * e12[0]) + e12[1] * (w1 * e12[1]);
        const double c21 = e21[0] * (w2 * e21[0]) + e21[1] * (w2 * e21[1]);
        B.c[2 * g] = c12;
        B.c[2 * g + 1] = c21;
        chi += huber(c12, d.huber, &w) + huber(c21, d.huber, &w);
    }
    return po_wave_sum(chi);
}

// rows of M [ -[P]x | I | P ] for a 2x3 matrix M: the 2x7 Jacobian of one edge
DEVI void s3_jrows(const double* M, const double* P, int fix_scale, double* J0, double* J1) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
        double* J = r ? J1 : J0;
        const double a = M[3 * r], b = M[3 * r + 1], c = M[3 * r + 2];
        J[0] = -b * P[2] + c * P[1];
        J[1] = a * P[2] - c * P[0];
        J[2] = -a * P[1] + b * P[0];
        J[3] = a; J[4] = b; J[5] = c;
        J[6] = fix_scale ? 0.0 : a * P[0] + b * P[1] + c * P[2];
    }
}

// H (upper triangle, row by row) += Wt J^T J, b -= Wt J^T e
DEVI void s3_accum(const double* J0, const double* J1, const double* e, double Wt, double* acc, double* bb) {
    int gi = 0;
#pragma unroll
    for (int a = 0; a < 7; a++) {
        bb[a] -= J0[a] * Wt * e[0] + J1[a] * Wt * e[1];
#pragma unroll
        for (int c = a; c < 7; c++) acc[gi++] += J0[a] * Wt * J0[c] + J1[a] * Wt * J1[c];
    }
}

// computeActiveErrors + activeRobustChi2 + buildSystem at the estimate S in one pass over the pairs (what the head of every LM
// iteration does, levenberg.cpp:75-87): returns the robust chi2 (the same per-lane sums in the same order as s3_errors), stores
// the chi2 of both edges of every active pair, and leaves the full sums of H and b in every lane
DEVI double s3_build(const Sim3Batch& B, const Sim3Desc& d, const Sim3State& S, double* acc, double* bb) {
    Sim3Map m;
    s3_map(S, m);
    double chi = 0.0;
#pragma unroll
    for (int i = 0; i < 28; i++) acc[i] = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) bb[i] = 0;
    for (int i = threadIdx.x; i < d.n_pairs; i += 64) {
        const size_t g = (size_t)d.pair0 + i;
        if (B.flag[g]) continue;
        double y[3], z[3], e12[2], e21[2], rw, J0[7], J1[7], M[6];
        s3_pair(B, d, m, g, y, z, e12, e21);
        const double w1 = B.w[2 * g], w2 = B.w[2 * g + 1];
        const double c12 = e12[0] * (w1 * e12[0]) + e12[1] * (w1 * e12[1]);
        const double c21 = e21[0] * (w2 * e21[0]) + e21[1] * (w2 * e21[1]);
        B.c[2 * g] = c12;
        B.c[2 * g + 1] = c21;
        double r12;
        // e12: M = -dpi(y), point y
        {
            const double iz = 1.0 / y[2];
            M[0] = -d.K1[0] * iz; M[1] = 0; M[2] = d.K1[0] * y[0] * iz * iz;
            M[3] = 0; M[4] = -d.K1[1] * iz; M[5] = d.K1[1] * y[1] * iz * iz;
            s3_jrows(M, y, d.fix_scale, J0, J1);
            r12 = huber(c12, d.huber, &rw);
            s3_accum(J0, J1, e12, rw * w1, acc, bb);
        }
        // e21: M = dpi(z) R^T / s, point P1c
        {
            const double iz = 1.0 / z[2];
            const double a0 = d.K2[0] * iz, a2 = -d.K2[0] * z[0] * iz * iz, b1 = d.K2[1] * iz, b2 = -d.K2[1] * z[1] * iz * iz;
#pragma unroll
            for (int c = 0; c < 3; c++) {   // (dpi R^T)[r][c] = sum_k dpi[r][k] R[c][k]
                M[c] = (a0 * m.R[3 * c] + a2 * m.R[3 * c + 2]) * m.is;
                M[3 + c] = (b1 * m.R[3 * c + 1] + b2 * m.R[3 * c + 2]) * m.is;
            }
            const double P1[3] = {B.p[6 * g], B.p[6 * g + 1], B.p[6 * g + 2]};
            s3_jrows(M, P1, d.fix_scale, J0, J1);
            chi += r12 + huber(c21, d.huber, &rw);
            s3_accum(J0, J1, e21, rw * w2, acc, bb);
        }
    }
#pragma unroll
    for (int i = 0; i < 28; i++) acc[i] = s3_lane_sum(acc[i]);
#pragma unroll
    for (int i = 0; i < 7; i++) bb[i] = s3_lane_sum(bb[i]);
    return po_wave_sum(chi);
}

// (H + lambda I) x = b by L D L^T without pivoting, H given as its packed upper triangle; false (and x = 0) when a pivot is not
// positive and finite (LinearSolverDense: the factorisation reports "not positive definite" -> solve() fails).  Every loop has
// constant bounds and is unrolled, so L, D and x stay in registers.
DEVI bool s3_solve(const double* acc, const double* bb, double lambda, double* x) {
    double L[7][7], D[7];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        // packed index of (j, i), i >= j: j * 7 - j (j - 1) / 2 + (i - j)
        double dj = acc[j * 7 - j * (j - 1) / 2] + lambda;
#pragma unroll
        for (int k = 0; k < j; k++) dj -= L[j][k] * L[j][k] * D[k];
        ok = ok && (dj > 0.0) && isfinite(dj);
        D[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double v = acc[j * 7 - j * (j - 1) / 2 + (i - j)];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * D[k];
            L[i][j] = v / dj;
        }
    }
    double yv[7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        double v = bb[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= L[i][k] * yv[k];
        yv[i] = v;
    }
#pragma unroll
    for (int i = 6; i >= 0; i--) {
        double v = yv[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < 7; k++) v -= L[k][i] * x[k];
        x[i] = v;
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        ok = ok && isfinite(x[i]);
    }
    if (!ok) {
#pragma unroll
        for (int i = 0; i < 7; i++) x[i] = 0.0;
    }
    return ok;
}

// SparseOptimizer::optimize(its) with OptimizationAlgorithmLevenberg (levenberg.cpp:61-164; the same schedule as k_pose_opt):
// returns cjIterations, *chi = currentChi of the last iteration
DEVI int s3_lm(const Sim3Batch& B, const Sim3Desc& d, Sim3State& S, int its, double* chi) {
    double lambda = 0, ni = 2, cur = 0;
    int cj = 0, nb = 0;
    for (int it = 0; it < its; it++) {
        double acc[28], bb[7];
        Sim3Step st;
        double* x = st.x;
        cur = s3_build(B, d, S, acc, bb);
        const double iniChi = cur;
        if (it == 0) {   // computeLambdaInit: tau * max |H_jj|
            double mx = 0;
#pragma unroll
            for (int j = 0; j < 7; j++) mx = fmax(fabs(acc[j * 7 - j * (j - 1) / 2]), mx);
            lambda = 1e-5 * mx;
            ni = 2;
            nb = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            const Sim3State bk = S;   // push()
            const bool ok2 = s3_solve(acc, bb, lambda, x);
            if (ok2) S = s3_oplus(S, st, d.fix_scale);
            double tempChi = s3_errors(B, d, S);
            if (!ok2) tempChi = 1.7976931348623157e308;
            rho = cur - tempChi;
            double scale = 0;
#pragma unroll
            for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + bb[j]);
            scale += 1e-3;
            rho /= scale;
            if (rho > 0 && isfinite(tempChi)) {
                const double r3 = 2 * rho - 1;
                double alpha = 1. - r3 * r3 * r3;
                alpha = fmin(alpha, 2. / 3.);
                lambda *= fmax(1. / 3., alpha);
                ni = 2;
                cur = tempChi;
            } else {
                lambda *= ni;
                ni *= 2;
                S = bk;   // pop(): the estimate goes back, the stored chi2 stay those of the rejected trial
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        ++cj;
        if (qmax == 10 || rho == 0) break;
        if ((iniChi - cur) * 1e3 < iniChi) nb++;
        else nb = 0;
        if (nb >= 3) break;
    }
    *chi = cur;
    return cj;
}

__global__ void __launch_bounds__(64) k_sim3_opt(Sim3Batch B) {
    const int f = blockIdx.x, t = threadIdx.x;
    const Sim3Desc& d = B.desc[f];
    Sim3Out& out = B.out[f];
    const int n = d.n_pairs;
    for (int i = t; i < n; i += 64) {
        const size_t g = (size_t)d.pair0 + i;
        B.flag[g] = 0;
        B.c[2 * g] = 0.0;
        B.c[2 * g + 1] = 0.0;
    }
    if (t == 0) {
        out.n_inliers = 0; out.status = 0; out.n_bad1 = 0; out.its[0] = 0; out.its[1] = 0;
        out.chi2_stage[0] = 0.0; out.chi2_stage[1] = 0.0;
        for (int k = 0; k < 8; k++) out.S[k] = d.S[k];
    }
    if (n == 0) return;
    Sim3State S;
#pragma unroll
    for (int k = 0; k < 3; k++) S.t[k] = d.S[k];
#pragma unroll
    for (int k = 0; k < 4; k++) S.q[k] = d.S[3 + k];
    S.s = d.S[7];
    // Both optimize() calls run through ONE copy of the LM code (the stage loop is not unrolled: two inlined copies cost registers).
    int nBad = 0;
#pragma nounroll
    for (int stage = 0; stage < 2; stage++) {
        // ---- optimize(its_stage1), :4723-4724; optimize(nBad > 0 ? 10 : 5) from the stage-1 estimate, :4759-4760 (iteration 0
        //      re-initialises lambda) ----
        double chi;
        const int its = stage == 0 ? d.its1 : (nBad > 0 ? d.its2_bad : d.its2_clean);
        const int cj = s3_lm(B, d, S, its, &chi);
        // ---- the test of both edges of every pair still in the problem (:4728-4746, :4762-4778): a pair leaves when either is
        //      beyond the gate ----
        double cnt = 0.0;
        for (int i = t; i < n; i += 64) {
            const size_t g = (size_t)d.pair0 + i;
            if (B.flag[g]) continue;
            const bool b = B.c[2 * g] > d.th2 || B.c[2 * g + 1] > d.th2;
            B.flag[g] = b ? 1 : 0;
            cnt += b ? 1.0 : 0.0;
        }
        const int bad = (int)(po_wave_sum(cnt) + 0.5);
        if (t == 0) { out.its[stage] = cj; out.chi2_stage[stage] = chi; }
        if (stage == 0) {
            nBad = bad;
            if (t == 0) out.n_bad1 = nBad;
            if (n - nBad < d.min_inliers) return;   // :4755: returns 0, S12 not written back, the bad pairs stay flagged
        } else if (t == 0) {
            out.n_inliers = n - nBad - bad;
            for (int k = 0; k < 3; k++) out.S[k] = S.t[k];
            for (int k = 0; k < 4; k++) out.S[3 + k] = S.q[k];
            out.S[7] = S.s;
        }
    }
}
