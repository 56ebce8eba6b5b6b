// vba_posegraph.h -- essential-graph optimisation (Sim3 pose graph) on the GPU.
// Replaces, for a batch of independent graphs, what Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:4243-4552) runs between
// its edge set-up and its write-back: optimize(20) with Levenberg-Marquardt (levenberg.cpp:61-164, setUserLambdaInit(1e-16)) over
// VertexSim3Expmap vertices (types_seven_dof_expmap.h:48-94) and EdgeSim3 edges (:100-124) with identity information and no
// robust kernel, and the map-point correction (:4511-4546).
//
// k_posegraph_opt: ONE workgroup of 256 lanes per graph, the whole optimize(its) in ONE launch.  Passes are separated by workgroup
// barriers only: no wait on another workgroup, no flag in memory, no floating-point atomic; every sum has one owner and a fixed
// order, so the result of a graph does not depend on what else is in the batch.  Every loop is bounded by `its`, the ten trials and
// the graph's sizes.
//   256 lanes: the passes with the most work items (28 error evaluations per edge, 49 entries per H block) fill any workgroup
//   size, but the factorisation walks the block columns one after the other with two barriers per column and has only
//   (rows reaching the column) x 7 work items in each -- 7 x 36 = 252 for the essential graph's band of a few dozen keyframes.
//   Four waves cover that; more waves would only make each of the 4 n barriers of a trial solve dearer.
//
// Error (EdgeSim3::computeError, :106-114): log(Sji * Si * Sj^-1), ordered (omega, upsilon, sigma); Sim3::log, inverse and
// operator* are restated from sim3.h:148-272 branch by branch.  The exponential and the update exp(x) * S are s3_oplus of
// vba_sim3.h (the update's quaternion is normalised there: DESIGN.md section 8).
// Jacobians: EdgeSim3 has no linearizeOplus, so g2o differentiates numerically (base_binary_edge.hpp:131-205): central differences
// with delta = 1e-9 through oplus, one work item per (edge, side, direction) here; with fix_scale, oplus zeroes the scale update
// and the scale column is exactly zero.
// Linear system: H in block-envelope storage (vba_host_posegraph.h), b; both assembled by owners from the host's lists in edge
// order (base_binary_edge.hpp:68-90).  Trial solve: F = H + lambda I (setLambda; H itself stays, which is restoreDiagonal), scalar
// L D L^T of F in envelope storage, column by column: phase A subtracts the finished columns from every block of column j, phase B
// factors the 7x7 diagonal block (redundantly in every lane that needs it) and solves the blocks below it.  Forward solve by
// columns, backward solve by rows.  A pivot that is not positive and finite fails the trial (tempChi = DBL_MAX).
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_sim3.h"   // Sim3State, Sim3Step, s3_oplus

#define PG_NT 256

DEVI Sim3State pg_load(const double* p) {
    Sim3State S;
#pragma unroll
    for (int k = 0; k < 3; k++) S.t[k] = p[k];
#pragma unroll
    for (int k = 0; k < 4; k++) S.q[k] = p[3 + k];
    S.s = p[7];
    return S;
}
DEVI void pg_store(double* p, const Sim3State& S) {
#pragma unroll
    for (int k = 0; k < 3; k++) p[k] = S.t[k];
#pragma unroll
    for (int k = 0; k < 4; k++) p[3 + k] = S.q[k];
    p[7] = S.s;
}

// Sim3::operator* (sim3.h:266-272): ret.r = r * other.r; ret.t = s * (r * other.t) + t; ret.s = s * other.s
DEVI Sim3State pg_mul(const Sim3State& a, const Sim3State& b) {
    Sim3State o;
    double R[9], rt[3];
    qmul(a.q, b.q, o.q);
    q2R(a.q, R);
    mv3(R, b.t, rt);
#pragma unroll
    for (int k = 0; k < 3; k++) o.t[k] = a.s * rt[k] + a.t[k];
    o.s = a.s * b.s;
    return o;
}
// Sim3::inverse (sim3.h:233-236): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
DEVI Sim3State pg_inv(const Sim3State& a) {
    Sim3State o;
    o.q[0] = -a.q[0]; o.q[1] = -a.q[1]; o.q[2] = -a.q[2]; o.q[3] = a.q[3];
    double R[9];
    q2R(o.q, R);
    const double mt[3] = {(-1. / a.s) * a.t[0], (-1. / a.s) * a.t[1], (-1. / a.s) * a.t[2]};
    mv3(R, mt, o.t);
    o.s = 1. / a.s;
    return o;
}
// Sim3::map (sim3.h:144-146)
DEVI void pg_map(const Sim3State& a, const double* p, double* o) {
    double R[9], r[3];
    q2R(a.q, R);
    mv3(R, p, r);
#pragma unroll
    for (int k = 0; k < 3; k++) o[k] = a.s * r[k] + a.t[k];
}

// W.lu().solve(t) of a 3x3 W (Eigen PartialPivLU: the largest |entry| of the column at or below the diagonal becomes the pivot,
// the first one on ties).  Rows are named variables and swaps are selects, so nothing is indexed at run time.
DEVI void pg_lu3(const double* W, const double* t, double* u) {
    double r0[4] = {W[0], W[1], W[2], t[0]}, r1[4] = {W[3], W[4], W[5], t[1]}, r2[4] = {W[6], W[7], W[8], t[2]};
    {   // column 0
        const int p = (fabs(r1[0]) > fabs(r0[0])) ? ((fabs(r2[0]) > fabs(r1[0])) ? 2 : 1) : ((fabs(r2[0]) > fabs(r0[0])) ? 2 : 0);
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double a = r0[k], b = (p == 1) ? r1[k] : r2[k];
            if (p != 0) {
                r0[k] = b;
                if (p == 1) r1[k] = a;
                else r2[k] = a;
            }
        }
        const double l1 = r1[0] / r0[0], l2 = r2[0] / r0[0];
#pragma unroll
        for (int k = 1; k < 4; k++) { r1[k] -= l1 * r0[k]; r2[k] -= l2 * r0[k]; }
    }
    {   // column 1
        const bool sw = fabs(r2[1]) > fabs(r1[1]);
#pragma unroll
        for (int k = 1; k < 4; k++) {
            const double a = r1[k], b = r2[k];
            r1[k] = sw ? b : a;
            r2[k] = sw ? a : b;
        }
        const double l2 = r2[1] / r1[1];
#pragma unroll
        for (int k = 2; k < 4; k++) r2[k] -= l2 * r1[k];
    }
    u[2] = r2[3] / r2[2];
    u[1] = (r1[3] - r1[2] * u[2]) / r1[1];
    u[0] = (r0[3] - r0[1] * u[1] - r0[2] * u[2]) / r0[0];
}

// Sim3::log (sim3.h:148-230): res = (omega, upsilon, sigma); the four branches as they stand
DEVI void pg_log(const Sim3State& S, double* res) {
    const double s = S.s, sigma = log(s);
    double R[9];
    q2R(S.q, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR
    const double eps = 0.00001;
    double A, B, C, f;
    if (fabs(sigma) < eps) {
        C = 1;
        if (d > 1 - eps) {
            f = 0.5;
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            const double theta = acos(d), theta2 = theta * theta;
            f = theta / (2 * sqrt(1 - d * d));
            A = (1 - cos(theta)) / (theta2);
            B = (theta - sin(theta)) / (theta2 * theta);
        }
    } else {
        C = (s - 1) / sigma;
        if (d > 1 - eps) {
            const double sigma2 = sigma * sigma;
            f = 0.5;
            A = ((sigma - 1) * s + 1) / (sigma2);
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double theta = acos(d);
            f = theta / (2 * sqrt(1 - d * d));
            const double theta2 = theta * theta;
            const double a = s * sin(theta), b = s * cos(theta);
            const double c = theta2 + sigma * sigma;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
        }
    }
    const double om[3] = {f * dR[0], f * dR[1], f * dR[2]};
    double Om[9], Om2[9], W[9];
    hat3(om, Om);
    mm3(Om, Om, Om2);
#pragma unroll
    for (int i = 0; i < 9; i++) W[i] = A * Om[i] + B * Om2[i] + ((i % 4 == 0) ? C : 0.0);
    double up[3];
    pg_lu3(W, S.t, up);
#pragma unroll
    for (int k = 0; k < 3; k++) { res[k] = om[k]; res[3 + k] = up[k]; }
    res[6] = sigma;
}

// EdgeSim3::computeError: log(C * v1->estimate() * v2->estimate().inverse())
DEVI void pg_error(const Sim3State& M, const Sim3State& Si, const Sim3State& Sj, double* e) {
    const Sim3State P = pg_mul(M, Si);
    const Sim3State Q = pg_inv(Sj);
    pg_log(pg_mul(P, Q), e);
}

// computeActiveErrors + activeChi2: a lane per edge, per-lane sums in edge order, then the fixed butterfly / LDS tree; the same
// bits in every lane.  The errors are stored for the assembly of b.
DEVI double pg_errors(const PgBatch& B, const PgDesc& d, double* sm4) {
    double chi = 0.0;
    for (int e = threadIdx.x; e < d.ne; e += PG_NT) {
        const size_t g = (size_t)d.e0 + e;
        const Sim3State M = pg_load(B.meas + 8 * g);
        const Sim3State Si = pg_load(B.S + 8 * ((size_t)d.v0 + B.ei[g]));
        const Sim3State Sj = pg_load(B.S + 8 * ((size_t)d.v0 + B.ej[g]));
        double r[7];
        pg_error(M, Si, Sj, r);
        double c = 0.0;
#pragma unroll
        for (int k = 0; k < 7; k++) {
            B.err[7 * g + k] = r[k];
            c += r[k] * r[k];
        }
        chi += c;
    }
    return block_sum256(chi, sm4);
}

// linearizeOplus of every edge (base_binary_edge.hpp:131-205): one work item per (edge, side, direction); columns of a fixed
// vertex are not computed
DEVI void pg_jacobians(const PgBatch& B, const PgDesc& d) {
    const double delta = 1e-9;
    const double scalar = 1.0 / (2 * delta);
    for (long long item = threadIdx.x; item < 14LL * d.ne; item += PG_NT) {
        const int e = (int)(item / 14), rem = (int)(item % 14), side = rem / 7, dir = rem % 7;
        const size_t g = (size_t)d.e0 + e;
        const int vi = B.ei[g], vj = B.ej[g];
        if (B.free_of[(size_t)d.v0 + (side ? vj : vi)] < 0) continue;
        const Sim3State M = pg_load(B.meas + 8 * g);
        const Sim3State Si = pg_load(B.S + 8 * ((size_t)d.v0 + vi));
        const Sim3State Sj = pg_load(B.S + 8 * ((size_t)d.v0 + vj));
        double acc[7] = {0, 0, 0, 0, 0, 0, 0};
#pragma nounroll
        for (int sg = 0; sg < 2; sg++) {
            const double sgn = sg ? -1.0 : 1.0;
            Sim3Step u;
#pragma unroll
            for (int k = 0; k < 7; k++) u.x[k] = (k == dir) ? sgn * delta : 0.0;
            const Sim3State Sp = s3_oplus(side ? Sj : Si, u, d.fix_scale);
            double r[7];
            pg_error(M, side ? Si : Sp, side ? Sp : Sj, r);
#pragma unroll
            for (int k = 0; k < 7; k++) acc[k] += sgn * r[k];   // errorBak = e(+delta) - e(-delta), exactly
        }
        double* Jc = B.J + 98 * g + 49 * side + dir;
#pragma unroll
        for (int k = 0; k < 7; k++) Jc[7 * k] = scalar * acc[k];
    }
}

// constructQuadraticForm of every edge, by owners: work item (free vertex, row) sums row `a` of its diagonal block and its entry
// of b over the vertex' edges in edge order; work item (pair, row) does the same for the block (hi, lo)
DEVI void pg_assemble(const PgBatch& B, const PgDesc& d) {
    const int* roff = B.row_off + d.r0;
    const int* first = B.first + d.f0;
    double* H = B.H + 49 * (size_t)d.env0;
    for (int item = threadIdx.x; item < 7 * d.nf; item += PG_NT) {
        const int f = item / 7, a = item % 7;
        const int* ib = B.inc_begin + d.r0 + f;
        double h[7] = {0, 0, 0, 0, 0, 0, 0}, bb = 0.0;
        for (int q = ib[0]; q < ib[1]; q++) {
            const int es = B.inc[(size_t)d.inc0 + q];
            const size_t g = (size_t)d.e0 + (es >> 1);
            const double* Jv = B.J + 98 * g + 49 * (es & 1);
            const double* er = B.err + 7 * g;
            double ja[7];
#pragma unroll
            for (int k = 0; k < 7; k++) ja[k] = Jv[7 * k + a];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 7; k++) s += ja[k] * er[k];
            bb -= s;
#pragma unroll
            for (int c = 0; c < 7; c++) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 7; k++) v += ja[k] * Jv[7 * k + c];
                h[c] += v;
            }
        }
        double* Hd = H + 49 * (size_t)(roff[f + 1] - 1) + 7 * a;   // the diagonal block is the last of its row
#pragma unroll
        for (int c = 0; c < 7; c++) Hd[c] = h[c];
        B.b[7 * ((size_t)d.f0 + f) + a] = bb;
    }
    for (int item = threadIdx.x; item < 7 * d.npair; item += PG_NT) {
        const int p = item / 7, a = item % 7;
        const int hi = B.pair_hi[(size_t)d.pair0 + p], lo = B.pair_lo[(size_t)d.pair0 + p];
        const int* pb = B.pair_begin + d.pb0 + p;
        double h[7] = {0, 0, 0, 0, 0, 0, 0};
        for (int q = pb[0]; q < pb[1]; q++) {
            const int es = B.pair_edge[(size_t)d.pe0 + q];
            const size_t g = (size_t)d.e0 + (es >> 1);
            const int hs = (es & 1) ? 0 : 1;   // side of hi: es & 1 says hi is vertex 0
            const double* Jh = B.J + 98 * g + 49 * hs;
            const double* Jl = B.J + 98 * g + 49 * (1 - hs);
#pragma unroll
            for (int c = 0; c < 7; c++) {
                double v = 0.0;
#pragma unroll
                for (int k = 0; k < 7; k++) v += Jh[7 * k + a] * Jl[7 * k + c];
                h[c] += v;
            }
        }
        double* Hb = H + 49 * (size_t)(roff[hi] + lo - first[hi]) + 7 * a;
#pragma unroll
        for (int c = 0; c < 7; c++) Hb[c] = h[c];
    }
}

// L D L^T of the 7x7 block T (its lower triangle is read): L unit lower, D; false when a pivot is not positive and finite
DEVI bool pg_ldl7(const double* T, double (*L)[7], double* D) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 7; j++) {
        double dj = T[8 * j];
#pragma unroll
        for (int k = 0; k < j; k++) dj -= L[j][k] * L[j][k] * D[k];
        ok = ok && (dj > 0.0) && isfinite(dj);
        D[j] = dj;
#pragma unroll
        for (int i = j + 1; i < 7; i++) {
            double v = T[7 * i + j];
#pragma unroll
            for (int k = 0; k < j; k++) v -= L[i][k] * L[j][k] * D[k];
            L[i][j] = v / dj;
        }
    }
    return ok;
}

// (H + lambda I) x = b in envelope storage; returns false (the same in every lane) when the trial fails
DEVI bool pg_solve(const PgBatch& B, const PgDesc& d, double lambda, int* s_fail) {
    const int t = threadIdx.x, nf = d.nf;
    const int* roff = B.row_off + d.r0;
    const int* first = B.first + d.f0;
    const int* lastr = B.last_row + d.f0;
    const double* H = B.H + 49 * (size_t)d.env0;
    double* F = B.F + 49 * (size_t)d.env0;
    double* Ld = B.Ld + 49 * (size_t)d.f0;
    const double* b = B.b + 7 * (size_t)d.f0;
    double* w = B.w + 7 * (size_t)d.f0;
    double* y = B.y + 7 * (size_t)d.f0;
    double* x = B.x + 7 * (size_t)d.f0;
    const long long nent = 49LL * roff[nf];
    for (long long k = t; k < nent; k += PG_NT) F[k] = H[k];
    for (int k = t; k < 7 * nf; k += PG_NT) w[k] = b[k];
    if (t == 0) *s_fail = 0;
    __syncthreads();
    for (int k = t; k < 7 * nf; k += PG_NT) F[49 * (size_t)(roff[k / 7 + 1] - 1) + 8 * (k % 7)] += lambda;   // setLambda
    __syncthreads();
    // ---- factorisation, block column by block column ----
    for (int j = 0; j < nf; j++) {
        const int nit = 7 * (lastr[j] - j + 1), fj = first[j];
        const double* Tjj = F + 49 * (size_t)(roff[j] + j - fj);
        // phase A: block (i, j) -= sum_k L(i, k) D_k L(j, k)^T over the finished columns both rows hold
        for (int item = t; item < nit; item += PG_NT) {
            const int i = j + item / 7, r = item % 7, fi = first[i];
            if (fi > j) continue;
            double* Tr = F + 49 * (size_t)(roff[i] + j - fi) + 7 * r;
            double T[7];
#pragma unroll
            for (int c = 0; c < 7; c++) T[c] = Tr[c];
            for (int k = (fi > fj ? fi : fj); k < j; k++) {
                const double* Lik = F + 49 * (size_t)(roff[i] + k - fi) + 7 * r;
                const double* Ljk = F + 49 * (size_t)(roff[j] + k - fj);
                const double* Dk = Ld + 49 * (size_t)k;
                double a[7];
#pragma unroll
                for (int m = 0; m < 7; m++) a[m] = Lik[m] * Dk[8 * m];
#pragma unroll
                for (int c = 0; c < 7; c++) {
                    double v = 0.0;
#pragma unroll
                    for (int m = 0; m < 7; m++) v += a[m] * Ljk[7 * c + m];
                    T[c] -= v;
                }
            }
#pragma unroll
            for (int c = 0; c < 7; c++) Tr[c] = T[c];
        }
        __syncthreads();
        // phase B: the diagonal block's factor, then row r of L(i, j) from  L(i, j) D_j L_jj^T = T(i, j)
        if (t < nit) {
            double L[7][7], D[7];
            const bool ok = pg_ldl7(Tjj, L, D);
            for (int item = t; item < nit; item += PG_NT) {
                const int i = j + item / 7, r = item % 7, fi = first[i];
                if (fi > j) continue;
                if (i == j) {
                    if (r != 0) continue;
                    double* o = Ld + 49 * (size_t)j;
#pragma unroll
                    for (int a = 0; a < 7; a++)
#pragma unroll
                        for (int c = 0; c < 7; c++) o[7 * a + c] = (c < a) ? L[a][c] : (c == a ? D[a] : 0.0);
                    if (!ok) *s_fail = 1;
                } else {
                    double* Tr = F + 49 * (size_t)(roff[i] + j - fi) + 7 * r;
                    double X[7];
#pragma unroll
                    for (int c = 0; c < 7; c++) {
                        double v = Tr[c];
#pragma unroll
                        for (int m = 0; m < c; m++) v -= X[m] * D[m] * L[c][m];
                        X[c] = v / D[c];
                    }
#pragma unroll
                    for (int c = 0; c < 7; c++) Tr[c] = X[c];
                }
            }
        }
        __syncthreads();
    }
    // ---- forward solve L y = b by columns ----
    for (int j = 0; j < nf; j++) {
        const int nit = 7 * (lastr[j] - j + 1);
        if (t < nit) {
            const double* Lj = Ld + 49 * (size_t)j;
            double yj[7];
#pragma unroll
            for (int a = 0; a < 7; a++) {
                double v = w[7 * j + a];
#pragma unroll
                for (int c = 0; c < a; c++) v -= Lj[7 * a + c] * yj[c];
                yj[a] = v;
            }
            for (int item = t; item < nit; item += PG_NT) {
                const int i = j + item / 7, r = item % 7, fi = first[i];
                if (fi > j) continue;
                if (i == j) {
                    if (r != 0) continue;
#pragma unroll
                    for (int a = 0; a < 7; a++) y[7 * j + a] = yj[a] / Lj[8 * a];   // and the diagonal solve: y <- D^-1 y
                } else {
                    const double* Lr = F + 49 * (size_t)(roff[i] + j - fi) + 7 * r;
                    double v = 0.0;
#pragma unroll
                    for (int c = 0; c < 7; c++) v += Lr[c] * yj[c];
                    w[7 * i + r] -= v;
                }
            }
        }
        __syncthreads();
    }
    // ---- backward solve L^T x = y by rows ----
    for (int i = nf - 1; i >= 0; i--) {
        const int fi = first[i], nit = 7 * (i - fi);
        if (t < nit || t == 0) {
            const double* Li = Ld + 49 * (size_t)i;
            double xi[7];
#pragma unroll
            for (int a = 6; a >= 0; a--) {
                double v = y[7 * i + a];
#pragma unroll
                for (int c = a + 1; c < 7; c++) v -= Li[7 * c + a] * xi[c];
                xi[a] = v;
            }
            if (t == 0) {
#pragma unroll
                for (int a = 0; a < 7; a++) x[7 * i + a] = xi[a];
            }
            for (int item = t; item < nit; item += PG_NT) {
                const int k = fi + item / 7, c = item % 7;
                const double* Lc = F + 49 * (size_t)(roff[i] + k - fi) + c;
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 7; r++) v += Lc[7 * r] * xi[r];
                y[7 * k + c] -= v;
            }
        }
        __syncthreads();
    }
    bool fin = true;
    for (int k = t; k < 7 * nf; k += PG_NT) fin = fin && isfinite(x[k]);
    if (!fin) *s_fail = 1;
    __syncthreads();
    const bool ok = *s_fail == 0;
    __syncthreads();
    return ok;
}

__global__ void __launch_bounds__(PG_NT) k_posegraph_opt(PgBatch B) {
    __shared__ double sm4[4];
    __shared__ int s_fail;
    const int t = threadIdx.x;
    const PgDesc& d = B.desc[blockIdx.x];
    PgOut& out = B.out[blockIdx.x];
    const int nf = d.nf;
    {
        const long long nent = 49LL * B.row_off[d.r0 + nf];
        double* H = B.H + 49 * (size_t)d.env0;
        for (long long k = t; k < nent; k += PG_NT) H[k] = 0.0;   // blocks without an edge (fill) stay zero; the owners rewrite theirs
        for (long long k = t; k < 8LL * d.nv; k += PG_NT) {
            B.S[8 * (size_t)d.v0 + k] = B.Sin[8 * (size_t)d.v0 + k];
            B.Sbk[8 * (size_t)d.v0 + k] = B.Sin[8 * (size_t)d.v0 + k];
        }
        for (int k = t; k < 7 * nf; k += PG_NT) B.x[7 * (size_t)d.f0 + k] = 0.0;
    }
    __syncthreads();
    // SparseOptimizer::optimize(its) with OptimizationAlgorithmLevenberg (levenberg.cpp:61-164), the schedule of s3_lm
    double lambda = 0, ni = 2, cur = 0, chi0 = 0;
    int cj = 0, nb = 0, trials = 0, stop = 0;
    for (int it = 0; it < d.its; it++) {
        cur = pg_errors(B, d, sm4);
        const double iniChi = cur;
        pg_jacobians(B, d);
        __syncthreads();
        pg_assemble(B, d);
        __syncthreads();
        if (it == 0) {   // computeLambdaInit: the user's value (setUserLambdaInit)
            chi0 = cur;
            lambda = d.lambda_init;
            ni = 2;
            nb = 0;
        }
        double rho = 0;
        int qmax = 0;
        do {
            for (int k = t; k < 8 * nf; k += PG_NT) {   // push()
                const size_t o = 8 * ((size_t)d.v0 + B.vert_of[(size_t)d.f0 + k / 8]) + k % 8;
                B.Sbk[o] = B.S[o];
            }
            const bool ok2 = pg_solve(B, d, lambda, &s_fail);
            if (d.debug) return;
            if (ok2) {   // update: exp(x_v) * S_v
                for (int f = t; f < nf; f += PG_NT) {
                    double* p = B.S + 8 * ((size_t)d.v0 + B.vert_of[(size_t)d.f0 + f]);
                    Sim3Step u;
#pragma unroll
                    for (int k = 0; k < 7; k++) u.x[k] = B.x[7 * ((size_t)d.f0 + f) + k];
                    pg_store(p, s3_oplus(pg_load(p), u, d.fix_scale));
                }
            }
            __syncthreads();
            double tempChi = pg_errors(B, d, sm4);
            if (!ok2) tempChi = 1.7976931348623157e308;
            rho = cur - tempChi;
            double sc = 0.0;   // computeScale: sum x (lambda x + b)
            if (ok2)
                for (int k = t; k < 7 * nf; k += PG_NT) {
                    const double xv = B.x[7 * (size_t)d.f0 + k];
                    sc += xv * (lambda * xv + B.b[7 * (size_t)d.f0 + k]);
                }
            double scale = block_sum256(sc, sm4);
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
                for (int k = t; k < 8 * nf; k += PG_NT) {   // pop()
                    const size_t o = 8 * ((size_t)d.v0 + B.vert_of[(size_t)d.f0 + k / 8]) + k % 8;
                    B.S[o] = B.Sbk[o];
                }
                __syncthreads();
            }
            qmax++;
        } while (rho < 0 && qmax < 10);
        ++cj;
        trials += qmax;
        if (qmax == 10) { stop = 1; break; }
        if (rho == 0) { stop = 2; break; }
        if ((iniChi - cur) * 1e3 < iniChi) nb++;
        else nb = 0;
        if (nb >= 3) { stop = 3; break; }
    }
    if (t == 0) {
        out.status = 0; out.its_done = cj; out.lm_trials = trials; out.stop = stop;
        out.chi2_initial = chi0; out.chi2_final = cur; out.lambda_final = lambda;
    }
}

// the map-point correction (src/Optimizer.cpp:4511-4546): P <- correctedSwr.map(Srw.map(P)) with the initial and the final
// estimate of the point's reference vertex; a lane per point
__global__ void __launch_bounds__(256) k_posegraph_points(PgBatch B) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= B.n_pt_total) return;
    const size_t v = (size_t)B.pt_ref[p];
    const Sim3State S0 = pg_load(B.Sin + 8 * v);
    const Sim3State Swr = pg_inv(pg_load(B.S + 8 * v));
    const double P[3] = {B.pt_in[3 * p], B.pt_in[3 * p + 1], B.pt_in[3 * p + 2]};
    double c[3], o[3];
    pg_map(S0, P, c);
    pg_map(Swr, c, o);
    B.pt_out[3 * p] = o[0]; B.pt_out[3 * p + 1] = o[1]; B.pt_out[3 * p + 2] = o[2];
}
