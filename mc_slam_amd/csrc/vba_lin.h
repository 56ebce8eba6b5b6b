// vba_lin.h -- linearisation and the Gauss-Newton control kernel.
// Reads the working state (pose, vel, bias, kfR, pt), the observations and the IMU measurements; writes chi2_e / depth_e / imu_chi,
// the slot, edge and landmark / run records (slot, erec, prec, lm_sd) and the IMU Hessians (imu_jrec, imuH) the Schur stage reads;
// k_ctrl_gn sums the chi2 and advances WinCtrl.  Needs vba_batch.h.
#pragma once
#include "vba_batch.h"

// ------------------------------------------------------------------------------------------------
// Linearisation: residuals + analytic Jacobians + Huber + per-landmark products.  Replaces
// computeActiveErrors (sparse_optimizer.cpp:61-88) + the vision/IMU part of buildSystem
// (block_solver.hpp:502-560); Jacobians never reach HBM unreduced: only their products do.
// ------------------------------------------------------------------------------------------------
// EdgeNavStatePRV + EdgeNavStateBias of one keyframe pair (the fused 15-D IMU factor): error, chi2, and in
// LIN_FULL mode the 30x30 local Hessian J^T (rho' Omega) J and rhs in local order [PR_i V_i B_i | PR_j V_j B_j].
// Two steps.  lin_imu_res: the Lie-group part -- residuals, Huber weights, the 9x30 Jacobian -- is scalar work, ONE LANE per
// keyframe pair (64 pairs per wave side by side; round 1 ran it on lane 0 of a wave per pair, 63 lanes idle for ~1500
// instructions); its products go to a 104-double record per pair (imu_jrec): the six 3x3 matrices the Jacobian is made of (R_i^T,
// hat(R_i^T vP), JrInv R_j^T R_i, hat(R_i^T vV), JrInv Exp(r_phi)^T Jr JRg, JrInv: 54), the errors, weights and column masks (47),
// the Huber weight and the active flags (3).  The records of a window are stored ELEMENT-major (element q of pair k at
// q * n_imu + k): the lanes of k_lin_imu_res -- one pair each -- store to consecutive addresses.  (Round 2 first wrote the whole
// 9x30 Jacobian and the weighted 9x9 information, 400 doubles pair-major: 400 store instructions of 49 scattered 8-byte pieces each,
// 2 GB of partial-line writes per pass and 0.6 of the kernel's 0.89 ms.)  lin_imu_hess: one wave per pair rebuilds J (preintegration
// Jacobians from imu_meas) and Omega = w * info, then H = J^T (Omega J) and the rhs.
#define IMU_JREC 104
DEVI void lin_imu_res(const Batch& B, const WinDesc& d, int k, int mode) {
    const size_t gk = d.imu0 + k;
    const int i = B.imu_i[gk], j = B.imu_j[gk];
    const int act = imu_act(B, d, i, j);
    if (!act) return;  // every vertex fixed: not in the active set
    const double* meas = B.imu_meas + 61 * gk;
    double* jr = B.imu_jrec + IMU_JREC * (size_t)d.imu0 + k;   // element q of this pair: jr[q * n_imu]
    const int js = d.n_imu;
    {
        const double* Ti = B.pose + 7 * (size_t)(d.kf0 + i);
        const double* Tj = B.pose + 7 * (size_t)(d.kf0 + j);
        const double* Vi = B.vel + 3 * (size_t)(d.kf0 + i);
        const double* Vj = B.vel + 3 * (size_t)(d.kf0 + j);
        const double* bi = B.bias + 12 * (size_t)(d.kf0 + i);
        const double* bj = B.bias + 12 * (size_t)(d.kf0 + j);
        const double dT = meas[0], dT2 = dT * dT;
        const double *dP = meas + 1, *dV = meas + 4, *dRm = meas + 7;
        const double *JPg = meas + 16, *JPa = meas + 25, *JVg = meas + 34, *JVa = meas + 43, *JRg = meas + 52;
        const double *dbg = bi + 6, *dba = bi + 9;
        double Ri[9], Rj[9];
        q2R(Ti + 3, Ri);
        q2R(Tj + 3, Rj);
        // residuals (g2otypes.cpp:207-215)
        double vP[3], vV[3], rvP[3], rvV[3], c1[3], c2[3], e[9];
        for (int m = 0; m < 3; m++) {
            vP[m] = Tj[m] - Ti[m] - Vi[m] * dT - 0.5 * d.g[m] * dT2;
            vV[m] = Vj[m] - Vi[m] - d.g[m] * dT;
        }
        double qiT[4];
        so3inv(Ti + 3, qiT);
        qrot(qiT, vP, rvP);
        qrot(qiT, vV, rvV);
        mv3(JPg, dbg, c1); mv3(JPa, dba, c2);
        for (int m = 0; m < 3; m++) e[m] = rvP[m] - (dP[m] + c1[m] + c2[m]);
        mv3(JVg, dbg, c1); mv3(JVa, dba, c2);
        for (int m = 0; m < 3; m++) e[6 + m] = rvV[m] - (dV[m] + c1[m] + c2[m]);
        double wv[3], qd[4], qR[4], qA[4], qAi[4], qB[4], qC[4];
        mv3(JRg, dbg, wv);
        so3exp(wv, qd);
        R2q(dRm, qR);
        qnorm(qR);
        so3mul(qR, qd, qA);
        so3inv(qA, qAi);
        so3mul(qAi, qiT, qB);
        so3mul(qB, Tj + 3, qC);
        so3log(qC, e + 3);
        const double* info = B.imu_info + 81 * gk;
        double s = 0;
        for (int a = 0; a < 9; a++) {
            double tt = 0;
            for (int b = 0; b < 9; b++) tt += info[9 * a + b] * e[b];
            s += e[a] * tt;
        }
        double rw = 1.0, rwb = 1.0;
        const bool rk = imu_robust(d);
        const double rob = rk ? huber(s, d.hub_prv, &rw) : s;
        double eb[6];
        for (int m = 0; m < 3; m++) {
            eb[m] = (bj[m] + bj[6 + m]) - (bi[m] + bi[6 + m]);
            eb[3 + m] = (bj[3 + m] + bj[9 + m]) - (bi[3 + m] + bi[9 + m]);
        }
        const double wg = d.inv_bg / dT, wa = d.inv_ba / dT;
        const double sb = wg * (eb[0] * eb[0] + eb[1] * eb[1] + eb[2] * eb[2]) + wa * (eb[3] * eb[3] + eb[4] * eb[4] + eb[5] * eb[5]);
        const double robb = rk ? huber(sb, d.hub_bias, &rwb) : sb;
        double* ch = B.imu_chi + 4 * gk;
        ch[0] = (act & 1) ? rob : 0.0; ch[1] = (act & 2) ? robb : 0.0; ch[2] = (act & 1) ? s : 0.0; ch[3] = (act & 2) ? sb : 0.0;
        if (mode == LIN_FULL) {
            // record elements 54..100: 9 err + 6 bias err + 2 weights (bias wg, wa scaled) + 30 column masks; 101: Huber weight of the
            // PRV edge (0: edge inactive), so that Omega = w * info is formed by the reader
            for (int a = 0; a < 9; a++) jr[(54 + a) * js] = e[a];
            for (int a = 0; a < 6; a++) jr[(54 + 9 + a) * js] = eb[a];
            jr[(54 + 15) * js] = (act & 2) ? rwb * wg : 0.0; jr[(54 + 16) * js] = (act & 2) ? rwb * wa : 0.0;
            {   // column mask of the 30 local variables: 0 where the vertex is fixed through kf_fix
                const int fi = (i < d.n_free) ? kf_free(B, d, i) : 7, fj = (j < d.n_free) ? kf_free(B, d, j) : 7;
                for (int q = 0; q < 15; q++) {
                    const int part = (q < 6) ? 0 : ((q < 9) ? 1 : 2);
                    jr[(54 + 17 + q) * js] = ((fi >> part) & 1) ? 1.0 : 0.0;
                    jr[(54 + 32 + q) * js] = ((fj >> part) & 1) ? 1.0 : 0.0;
                }
            }
            jr[101 * js] = rw;
            jr[102 * js] = (act & 1) ? 1.0 : 0.0;
            // Jacobians (g2otypes.cpp:296-359); local columns: PR_i 0..5, V_i 6..8, B_i 9..14, PR_j 15..20, V_j 21..23
            double RiT[9], RjT[9], JrI[9], H1[9], H2[9], T1[9], T2[9];
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) { RiT[3 * a + b] = Ri[3 * b + a]; RjT[3 * a + b] = Rj[3 * b + a]; }
            so3jrinv(e + 3, JrI);
            double mP[3], mV[3];
            mv3(RiT, vP, mP);
            mv3(RiT, vV, mV);
            hat3(mP, H1);
            hat3(mV, H2);
            mm3(JrI, RjT, T1);
            mm3(T1, Ri, T2);  // JrInv Rj^T Ri
            double qe[4], qei[4], ExpT[9], JrB[9], T3[9];
            so3exp(e + 3, qe);
            so3inv(qe, qei);
            q2R(qei, ExpT);
            so3jr(wv, JrB);
            mm3(JrI, ExpT, T1);
            mm3(T1, JrB, T3);
            mm3(T3, JRg, T1);  // JrInv Exp(rphi)^T Jr(JRg dbg) JRg
            for (int a = 0; a < 3; a++)
                for (int b = 0; b < 3; b++) {
                    const int q = 3 * a + b;
                    // the Jacobian's building blocks (assembled by lin_imu_fill_J): record elements 0..53
                    jr[(0 + q) * js] = RiT[q];
                    jr[(9 + q) * js] = H1[q];
                    jr[(18 + q) * js] = T2[q];
                    jr[(27 + q) * js] = H2[q];
                    jr[(36 + q) * js] = T1[q];
                    jr[(45 + q) * js] = JrI[q];
                }
        }
    }
}

// H = J^T (Omega J) + the bias edge's -I / +I terms, rhs = -J^T Omega e, of one keyframe pair.  ONE WAVE by contract (sm: 672 doubles):
// the phases are ordered with wave_lds_sync(), not with a workgroup barrier -- k_lin2_imu calls it from wave 0 of a 256-thread
// workgroup whose other waves have left (a barrier behind a divergent exit is undefined in the HIP model)
DEVI void lin_imu_hess(const Batch& B, const WinDesc& d, int k, double* sm) {
    const size_t gk = d.imu0 + k;
    const int i = B.imu_i[gk], j = B.imu_j[gk];
    if (!imu_act(B, d, i, j)) return;
    double* J = sm;            // 9 x 30
    double* Om = sm + 270;     // 9 x 9 weighted information
    double* T = sm + 351;      // 9 x 30 = Om J ; before that: the 54 building blocks of J
    double* er = sm + 621;     // 9 err + 6 bias err + 2 weights + 30 column masks
    const int t = threadIdx.x;
    const double* jr = B.imu_jrec + IMU_JREC * (size_t)d.imu0 + k;
    const int js = d.n_imu;
    const double* meas = B.imu_meas + 61 * gk;
    const double* info = B.imu_info + 81 * gk;
    const double rw = jr[101 * js];
    const bool on = jr[102 * js] != 0.0;
    for (int q = t; q < 270; q += 64) J[q] = 0.0;
    if (t < 54) T[t] = jr[t * js];
    if (t < 47) er[t] = jr[(54 + t) * js];
    for (int q = t; q < 81; q += 64) Om[q] = on ? rw * info[q] : 0.0;
    wave_lds_sync();
    if (t < 9) {   // Jacobians (g2otypes.cpp:296-359); local columns: PR_i 0..5, V_i 6..8, B_i 9..14, PR_j 15..20, V_j 21..23
        const int a = t / 3, b = t % 3, q = t;
        const double dT = meas[0];
        const double *JPg = meas + 16, *JPa = meas + 25, *JVg = meas + 34, *JVa = meas + 43;
        const double *RiT = T, *H1 = T + 9, *T2 = T + 18, *H2 = T + 27, *T1 = T + 36, *JrI = T + 45;
        J[(0 + a) * 30 + 0 + b] = -RiT[q];            // d rP / d P_i
        J[(0 + a) * 30 + 3 + b] = H1[q];              // d rP / d phi_i
        J[(3 + a) * 30 + 3 + b] = -T2[q];             // d rphi / d phi_i
        J[(6 + a) * 30 + 3 + b] = H2[q];              // d rV / d phi_i
        J[(0 + a) * 30 + 6 + b] = -RiT[q] * dT;       // d rP / d V_i
        J[(6 + a) * 30 + 6 + b] = -RiT[q];            // d rV / d V_i
        J[(0 + a) * 30 + 9 + b] = -JPg[q];            // d rP / d dbg_i
        J[(0 + a) * 30 + 12 + b] = -JPa[q];           // d rP / d dba_i
        J[(3 + a) * 30 + 9 + b] = -T1[q];             // d rphi / d dbg_i
        J[(6 + a) * 30 + 9 + b] = -JVg[q];
        J[(6 + a) * 30 + 12 + b] = -JVa[q];
        J[(0 + a) * 30 + 15 + b] = RiT[q];            // d rP / d P_j
        J[(3 + a) * 30 + 18 + b] = JrI[q];            // d rphi / d phi_j
        J[(6 + a) * 30 + 21 + b] = RiT[q];            // d rV / d V_j
    }
    wave_lds_sync();
    for (int q = t; q < 270; q += 64) {  // T = Om J
        const int a = q / 30, col = q % 30;
        double s = 0;
#pragma unroll
        for (int b = 0; b < 9; b++) s += Om[9 * a + b] * J[b * 30 + col];
        T[q] = s;
    }
    wave_lds_sync();
    double* H = B.imuH + VBA_IMUH * gk;
    for (int q = t; q < 900; q += 64) {  // H = J^T T  (+ bias edge: -I/+I Jacobians on B_i (9..14), B_j (24..29))
        const int r = q / 30, col = q % 30;
        double s = 0;
#pragma unroll
        for (int a = 0; a < 9; a++) s += J[a * 30 + r] * T[a * 30 + col];
        const int rb = (r >= 9 && r < 15) ? r - 9 : ((r >= 24) ? r - 24 : -1);
        const int cb = (col >= 9 && col < 15) ? col - 9 : ((col >= 24) ? col - 24 : -1);
        if (rb >= 0 && rb == cb) {
            const double wq = (rb < 3) ? er[15] : er[16];
            const double sr = (r < 15) ? -1.0 : 1.0, scn = (col < 15) ? -1.0 : 1.0;
            s += sr * scn * wq;
        }
        H[q] = s * er[17 + r] * er[17 + col];
    }
    if (t < 30) {  // rhs = -J^T Om e  (+ bias edge)
        double s = 0;
        for (int a = 0; a < 9; a++) s -= T[a * 30 + t] * er[a];
        const int rb = (t >= 9 && t < 15) ? t - 9 : ((t >= 24) ? t - 24 : -1);
        if (rb >= 0) {
            const double wq = (rb < 3) ? er[15] : er[16];
            const double sr = (t < 15) ? -1.0 : 1.0;
            s -= sr * wq * er[9 + rb];
        }
        H[900 + t] = s * er[17 + t];
    }
}

// ------------------------------------------------------------------------------------------------
// K_lin2 (inverse-depth variant), edge-parallel.  A 256-thread workgroup owns a
// run of consecutive landmarks with <= 256 edges (ranges built at upload): one lane per EDGE evaluates the
// residual and Jacobians (coalesced observation loads), the per-landmark sums (D, b_l, W0, g0, G0) are taken by
// one lane per LANDMARK from LDS, and the 256-B edge records leave through an LDS transpose as contiguous
// 16-B chunks instead of 64 scattered records per store instruction.
// ------------------------------------------------------------------------------------------------
#define LIN2_ES 15   // LDS row stride (doubles) of one edge: phase B/C [0..5] A [6..7] a [8..9] r ; phase D/E [0..11] Bi [12..13] r
#define LIN2_PS 19   // LDS row stride of one landmark: dd, y(3), Xw(3), N0(9), ref_free, sD (+ one spare: the stride stays odd)
#define LIN2_LDS ((256 * LIN2_ES + 64 * LIN2_PS + 4) * 8)   // 40 480 B: four workgroups per CU

// what a launch in `mode` is for window c: LIN_FULL, LIN_ERR, or LIN_SKIP (nothing to do).  Modes other than LIN_AUTO / LIN_REDO
// pass through.
DEVI int lin_mode_of(const WinCtrl& c, int mode) {
    if (mode == LIN_AUTO) return c.lin_probe ? LIN_ERR : LIN_FULL;
    if (mode == LIN_REDO) return c.lin_redo ? LIN_FULL : LIN_SKIP;
    return mode;
}

// The IMU factors: a launch of their own behind the vision linearisation (same stream) -- inlined into k_lin2 their ~60 live
// doubles of Lie algebra set the register budget of the 130x more numerous edge workgroups.  k_lin_imu_res: a lane per keyframe
// pair; k_lin_imu_hess (LIN_FULL only): a wave per pair.  `gate_lm`: the XYZ / Levenberg-Marquardt gating of k_lin_xyz.
// `mode` comes in as launched and leaves resolved for the window (lin_mode_of).
DEVI bool lin_imu_gate(const WinDesc& d, const WinCtrl& c, int& mode) {
    if (!c.active) return false;
    mode = lin_mode_of(c, mode);
    if (mode == LIN_SKIP) return false;
    if (d.variant == 2) return true;
    if (mode == 2 /* LIN_ERR_TRIAL */ && !win_on(d, c)) return false;
    if (mode == LIN_FULL && d.algo == 1 && c.lm_need_trial) return false;
    return true;
}
__global__ void __launch_bounds__(64) k_lin_imu_res(Batch B, int mode) {
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    if (!lin_imu_gate(d, B.ctrl[w], mode)) return;   // (mode: resolved for the window from here on)
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= d.n_imu) return;
    lin_imu_res(B, d, k, (mode == LIN_FULL) ? LIN_FULL : LIN_ERR);
}
// few windows: both steps in one launch, a wave per pair (lane 0 runs the Lie-group part), one launch gap less per pass
__global__ void __launch_bounds__(64) k_lin_imu_pair(Batch B, int mode) {
    __shared__ double sm[672];
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    if (!lin_imu_gate(d, B.ctrl[w], mode)) return;
    const int k = blockIdx.x;
    if (k >= d.n_imu) return;
    if (threadIdx.x == 0) lin_imu_res(B, d, k, (mode == LIN_FULL) ? LIN_FULL : LIN_ERR);
    if (mode != LIN_FULL) return;
    __threadfence_block();
    __syncthreads();
    lin_imu_hess(B, d, k, sm);
}
// mode: LIN_FULL, or LIN_AUTO / LIN_REDO -- a probing window has no record to read and owes no Hessian
__global__ void __launch_bounds__(64) k_lin_imu_hess(Batch B, int mode) {
    __shared__ double sm[672];
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    if (!lin_imu_gate(d, B.ctrl[w], mode) || mode != LIN_FULL) return;
    const int k = blockIdx.x;
    if (k >= d.n_imu) return;
    lin_imu_hess(B, d, k, sm);
}

// The geometry of one inverse-depth edge (g2otypes.cpp:25-60), shared by the linearisation and by the two passes that classify
// edges (k_classify, k_final_edges): those evaluate chi2 and depth again at the estimates instead of reading a per-edge copy the
// linearisation used to leave behind on EVERY pass (16 of its 218 bytes per edge; the estimates do not move between a window's last
// linearisation and its classification, and the expressions are these same ones, so the values are the same).
DEVI void idp_point_world(const WinDesc& d, const double* C0, double rho, double xb, double yb, double& dd, double (&c0)[3], double (&b0)[3],
                          double (&Xw)[3]) {   // C0: R|t of the reference keyframe
    if (rho < 1e-6) rho = 1e-6;  // g2otypes.cpp:42-47
    dd = 1.0 / rho;
    const double P0[3] = {xb * dd, yb * dd, dd};
    double tb[3];
    mtv3(d.Rcb, P0, c0);
    mtv3(d.Rcb, d.tcb, tb);
    b0[0] = c0[0] - tb[0]; b0[1] = c0[1] - tb[1]; b0[2] = c0[2] - tb[2];
    mv3(C0, b0, Xw);
    Xw[0] += C0[9]; Xw[1] += C0[10]; Xw[2] += C0[11];
}
DEVI void idp_edge_pc(const WinDesc& d, const double* Xw, const double* Ri, const double* ti, double (&ta)[3], double (&Pc)[3]) {
    const double v[3] = {Xw[0] - ti[0], Xw[1] - ti[1], Xw[2] - ti[2]};
    mtv3(Ri, v, ta);
    mv3(d.Rcb, ta, Pc);
    Pc[0] += d.tcb[0]; Pc[1] += d.tcb[1]; Pc[2] += d.tcb[2];
}
DEVI void idp_edge_err(const WinDesc& d, const double (&Pc)[3], double u, double v, double& iz, double& ex, double& ey) {
    iz = 1.0 / Pc[2];
    ex = u - (Pc[0] * iz * d.K[0] + d.K[2]);
    ey = v - (Pc[1] * iz * d.K[1] + d.K[3]);
}
DEVI double idp_edge_chi2(const WinDesc& d, const double (&Pc)[3], double u, double v, double wgt, double& iz, double& ex, double& ey) {
    idp_edge_err(d, Pc, u, v, iz, ex, ey);
    return ex * (wgt * ex) + ey * (wgt * ey);
}
// The weighted residual sc r of an edge, sc = sqrt(rho' w).  The linearisation (lin2_body, phase B) sums it into b_l and the reference
// keyframe's g0; the diagonal Schur walk forms it AGAIN from the edge record (P_c, sc) and the pixel for b_p = -sum Bi^T r, instead of
// reading a copy the linearisation used to store per edge and pass.  Both call this one function: the same expression, the same bits.
DEVI void idp_edge_wres(const WinDesc& d, const double (&Pc)[3], double u, double v, double sc, double& r0, double& r1) {
    double iz, ex, ey;
    idp_edge_err(d, Pc, u, v, iz, ex, ey);
    r0 = sc * ex; r1 = sc * ey;
}
// chi2 and depth of edge go at the current estimates (the classification passes)
DEVI void idp_edge_eval(const Batch& B, const WinDesc& d, size_t go, double& s, double& depth) {
    const size_t gp = d.pt0 + B.obs_pt[go];
    const double* C0 = B.kfR + 12 * (size_t)(d.kf0 + B.pt_ref[gp]);
    const double* Ci = B.kfR + 12 * (size_t)(d.kf0 + B.obs_kf[go]);
    double dd, c0[3], b0[3], Xw[3], ta[3], Pc[3], iz, ex, ey;
    idp_point_world(d, C0, B.pt[3 * gp], B.pt[3 * gp + 1], B.pt[3 * gp + 2], dd, c0, b0, Xw);
    idp_edge_pc(d, Xw, Ci, Ci + 9, ta, Pc);
    depth = Pc[2];
    s = idp_edge_chi2(d, Pc, B.obs_uv[2 * go], B.obs_uv[2 * go + 1], B.obs_w[go], iz, ex, ey);
}

DEVI void lin2_body(const Batch& B, int nblk_lin, int mode, double* lsm) {
    double* ER = lsm;                       // 256 x LIN2_ES
    double* PT = lsm + 256 * LIN2_ES;       // 64 x LIN2_PS
    double* red = PT + 64 * LIN2_PS;        // 4
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    const WinCtrl& c = B.ctrl[w];
    if (!c.active) return;
    const bool probe = mode == LIN_AUTO && c.lin_probe;   // (uniform over the workgroup: one window, one flag)
    mode = lin_mode_of(c, mode);
    if (mode == LIN_SKIP) return;
    const int t = threadIdx.x;
    const int lb = blockIdx.x;
    if (lb >= d.n_part_lin) return;
    const int4 run = reinterpret_cast<const int4*>(B.lin_blk)[d.lb0 + lb];  // one load instead of the chain table -> CSR
    const int p0 = run.x, p1 = run.y, e0 = run.z, e1 = run.w;
    const int* ob = B.pt_obs_begin + d.pt0 + d.win;
    const int ne = e1 - e0, npb = p1 - p0;
    const double fx = d.K[0], fy = d.K[1], cx = d.K[2], cy = d.K[3];
    // the edge lanes fetch their own inputs BEFORE phase A: the chain obs_kf -> keyframe R|t then overlaps with phase A's
    // pt_ref -> reference R|t instead of following it behind the barrier
    int pl = 0, e_kf = 0, e_pe = 0;
    bool e_out = true;
    double Ri[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, e_t[3] = {0, 0, 0}, e_u = 0, e_v = 0, e_w = 0;
    if (t < ne) {
        const size_t go = d.obs0 + e0 + t;
        pl = B.obs_pt[go] - p0;
        e_kf = B.obs_kf[go];
        e_pe = B.slot_perm[go];
        e_out = B.lvl[go] != 0;
        e_u = B.obs_uv[2 * go]; e_v = B.obs_uv[2 * go + 1];
        e_w = B.obs_w[go];
        const double* Ci = B.kfR + 12 * (size_t)(d.kf0 + e_kf);
#pragma unroll
        for (int i = 0; i < 9; i++) Ri[i] = Ci[i];
        e_t[0] = Ci[9]; e_t[1] = Ci[10]; e_t[2] = Ci[11];
    }
    // likewise the phase-C lanes (four per landmark): CSR bounds and record position of their landmark
    int c_ob = 0, c_oe = 0, c_pp = 0;
    if (t < 4 * npb) {
        const int p = p0 + (t >> 2);
        c_ob = ob[p] - e0;
        c_oe = ob[p + 1] - e0;
        c_pp = B.pt_perm[d.pt0 + p];
    }
    // A. one lane per landmark: quantities shared by all its edges
    int a_run = 0, a_nruns = 0;   // (landmark lanes, all in wave 0: run of consecutive landmarks with one reference keyframe; runs of the workgroup)
    bool a_first = false;
    if (t < npb) {
        const size_t gp = d.pt0 + p0 + t;
        const int rf = B.pt_ref[gp];
        const double* C0 = B.kfR + 12 * (size_t)(d.kf0 + rf);
        double R0[9], c0[3], b0[3], y[3], Xw[3], Hb[9], N0[9], dd;
#pragma unroll
        for (int i = 0; i < 9; i++) R0[i] = C0[i];
        idp_point_world(d, C0, B.pt[3 * gp], B.pt[3 * gp + 1], B.pt[3 * gp + 2], dd, c0, b0, Xw);
        mv3(R0, c0, y);
        hat3(b0, Hb);
        mm3(R0, Hb, N0);
        double* q = PT + t * LIN2_PS;
        q[0] = dd;
#pragma unroll
        for (int i = 0; i < 3; i++) { q[1 + i] = y[i]; q[4 + i] = Xw[i]; }
#pragma unroll
        for (int i = 0; i < 9; i++) q[7 + i] = N0[i];
        q[16] = (kf_free(B, d, rf) & 1) ? 1.0 : 0.0;
        if (mode == LIN_FULL) {
            const int rf_prev = __shfl_up(rf, 1, 64);
            a_first = (t == 0) || (rf != rf_prev);
            const unsigned long long fm = __ballot(a_first);
            a_run = __popcll(fm & ((2ull << t) - 1ull)) - 1;
            a_nruns = __popcll(fm);
        }
    }
    __syncthreads();
    // B. one lane per edge.  With A = sqrt(rho' w) J_pi R_cb R_i^T (2x3) the two pose Jacobians of the edge are
    //    Bi = [A | -sqrt(.) (J_pi R_cb) x ta] (observer) and Br = A [-I | N0] (reference keyframe, N0 per landmark).
    double chi = 0.0;
    double ub[6] = {0, 0, 0, 0, 0, 0};      // Bi^T a: numerator of the edge's slot record
    double rpc[3] = {0, 0, 1}, rsc = 0.0;   // edge record: P_c and the Jacobian scale (0: no Jacobian for the readers)
    double a[2] = {0, 0}, r2[2] = {0, 0};
    if (t < ne) {
        const size_t go = d.obs0 + e0 + t;
        const double* q = PT + pl * LIN2_PS;
        const int kf = e_kf;
        double ta[3], Pc[3];
        idp_edge_pc(d, q + 4, Ri, e_t, ta, Pc);
        rpc[0] = Pc[0]; rpc[1] = Pc[1]; rpc[2] = Pc[2];
        double A[6] = {0, 0, 0, 0, 0, 0};
        if (!e_out) {
            double iz, ex, ey;
            const double wgt = e_w;
            const double s = idp_edge_chi2(d, Pc, e_u, e_v, wgt, iz, ex, ey);
            double rw = 1.0;
            if (c.robust_vis) chi = huber(s, d.hub_vis, &rw);
            else chi = s;
            if (mode == LIN_FULL) {
                const double sc = sqrt(rw * wgt);
                const double Jp[6] = {fx * iz, 0.0, -Pc[0] * iz * fx * iz, 0.0, fy * iz, -Pc[1] * iz * fy * iz};
                double Jc[6];
#pragma unroll
                for (int rr = 0; rr < 2; rr++)
#pragma unroll
                    for (int k = 0; k < 3; k++)
                        Jc[3 * rr + k] = Jp[3 * rr] * d.Rcb[k] + Jp[3 * rr + 1] * d.Rcb[3 + k] + Jp[3 * rr + 2] * d.Rcb[6 + k];
                const bool of = kf_free(B, d, kf) & 1;
                rsc = of ? sc : 0.0;
                double Bi[12];
#pragma unroll
                for (int rr = 0; rr < 2; rr++) {
#pragma unroll
                    for (int k = 0; k < 3; k++) {
                        A[3 * rr + k] = sc * (Jc[3 * rr] * Ri[3 * k] + Jc[3 * rr + 1] * Ri[3 * k + 1] + Jc[3 * rr + 2] * Ri[3 * k + 2]);
                        Bi[6 * rr + k] = of ? A[3 * rr + k] : 0.0;
                    }
                    a[rr] = q[0] * (A[3 * rr] * q[1] + A[3 * rr + 1] * q[2] + A[3 * rr + 2] * q[3]);
                    const double j0 = Jc[3 * rr], j1 = Jc[3 * rr + 1], j2 = Jc[3 * rr + 2];
                    Bi[6 * rr + 3] = of ? -sc * (j1 * ta[2] - j2 * ta[1]) : 0.0;
                    Bi[6 * rr + 4] = of ? -sc * (j2 * ta[0] - j0 * ta[2]) : 0.0;
                    Bi[6 * rr + 5] = of ? -sc * (j0 * ta[1] - j1 * ta[0]) : 0.0;
                }
#pragma unroll
                for (int i = 0; i < 6; i++) ub[i] = Bi[i] * a[0] + Bi[6 + i] * a[1];
                idp_edge_wres(d, Pc, e_u, e_v, sc, r2[0], r2[1]);
            }
        }
        if (mode == LIN_FULL) {
            double* er = ER + t * LIN2_ES;
#pragma unroll
            for (int i = 0; i < 6; i++) er[i] = A[i];
            er[6] = a[0]; er[7] = a[1]; er[8] = r2[0]; er[9] = r2[1];
        }
    }
    if (mode != LIN_FULL) {
        const double tot = block_sum256(chi, red);
        if (t == 0) {
            B.part[d.part0 + lb] = tot;
            // a probe is counted once per pass, by the window's first workgroup (here, behind the last load of the pass: a store to the
            // control block ahead of them costs k_lin2 three registers)
            if (probe && lb == 0) B.ctrl[w].n_probe++;
        }
        return;
    }
    __syncthreads();
    // C. FOUR lanes per landmark: each sums every fourth edge (fixed order), the quad adds up (fixed order again), then
    //    all four hold D, b_l and, for the reference keyframe, sum Br^T Br = Q^T (sum A^T A) Q, sum Br^T a = Q^T sum A^T a,
    //    sum Br^T r = Q^T sum A^T r with Q = [-I | N0].  The landmark's reference slot record leaves from lane 0 of the quad; the
    //    reference keyframe's direct terms (G0: 21, g0: 6) go to LDS -- over the edge rows, which nobody reads any more after the
    //    barrier -- and leave summed over RUNS of consecutive landmarks with one reference keyframe (phase E): one 256-byte record
    //    per run instead of one per landmark (a quarter of the bytes of a pass when the caller's landmarks come track by track).
    double* GS = ER;                                            // 64 x 28
    int* RS = reinterpret_cast<int*>(ER + 64 * 28);             // run starts [nruns + 1], then the number of runs
    double gv[7];
    const int c_jl = t >> 2, c_sub = t & 3;
    if (t < 4 * npb) {
        const int jl = c_jl, sub = c_sub;
        double D = 0, bl = 0, M[6] = {0, 0, 0, 0, 0, 0}, wa[3] = {0, 0, 0}, wr[3] = {0, 0, 0};
        for (int o = c_ob + sub; o < c_oe; o += 4) {
            const double* er = ER + o * LIN2_ES;
            const double a0 = er[6], a1 = er[7], q0 = er[8], q1 = er[9];
            D += a0 * a0 + a1 * a1;
            bl -= a0 * q0 + a1 * q1;
            int gi = 0;
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double b0 = er[i], b1 = er[3 + i];
                wa[i] += b0 * a0 + b1 * a1;
                wr[i] += b0 * q0 + b1 * q1;
#pragma unroll
                for (int j = i; j < 3; j++) M[gi++] += b0 * er[j] + b1 * er[3 + j];
            }
        }
#define QUADSUM(v) { v = quad_sum(v); }
        QUADSUM(D) QUADSUM(bl)
#pragma unroll
        for (int i = 0; i < 6; i++) QUADSUM(M[i])
#pragma unroll
        for (int i = 0; i < 3; i++) { QUADSUM(wa[i]) QUADSUM(wr[i]) }
#undef QUADSUM
        const double sD = (D > 0.0) ? sqrt(1.0 / D) : 0.0;
        const double beta = sD * bl;
        double* q = PT + jl * LIN2_PS;
        const double rfm = q[16];  // 1: reference keyframe is free, 0: fixed (no Hessian block)
        double N0[9];
#pragma unroll
        for (int i = 0; i < 9; i++) N0[i] = q[7 + i];
        const int pp = c_pp;  // landmark records grouped by reference keyframe
        if (sub == 0) {
            q[17] = sD;
            double* sr = B.slot + VBA_SLOT * (size_t)(d.obs0 + d.pt0 + d.n_obs + pp);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                sr[k] = -wa[k] * rfm * sD;
                sr[3 + k] = (N0[k] * wa[0] + N0[3 + k] * wa[1] + N0[6 + k] * wa[2]) * rfm * sD;
            }
            B.lm_sd[d.pt0 + p0 + jl] = make_double2(sD, beta);   // once per landmark, not in every one of its slots
        }
        // (N0 = R0 hat(b0) had a 128-byte record of its own, 10 % of the bytes of a pass: its readers -- the reference items of the
        //  off-diagonal Schur pairs -- rebuild it from the landmark and the reference keyframe's rotation)
        {   // G0 (21) and g0 (6): every lane of the quad forms them, lane `sub` keeps values 7 sub .. 7 sub + 6 across the barrier
            double Ms[9], MN[9], G[28];
            Ms[0] = M[0]; Ms[1] = M[1]; Ms[2] = M[2]; Ms[3] = M[1]; Ms[4] = M[3]; Ms[5] = M[4]; Ms[6] = M[2]; Ms[7] = M[4]; Ms[8] = M[5];
            mm3(Ms, N0, MN);
            int gi = 0;
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = i; j < 6; j++) {
                    double v;
                    if (i < 3 && j < 3) v = Ms[3 * i + j];
                    else if (i < 3) v = -MN[3 * i + (j - 3)];
                    else v = N0[i - 3] * MN[j - 3] + N0[3 + i - 3] * MN[3 + j - 3] + N0[6 + i - 3] * MN[6 + j - 3];
                    G[gi++] = v * rfm;
                }
#pragma unroll
            for (int k = 0; k < 3; k++) {
                G[21 + k] = wr[k] * rfm;
                G[24 + k] = -(N0[k] * wr[0] + N0[3 + k] * wr[1] + N0[6 + k] * wr[2]) * rfm;
            }
            G[27] = 0.0;
#pragma unroll
            for (int i = 0; i < 7; i++) gv[i] = (sub == 0) ? G[i] : (sub == 1) ? G[7 + i] : (sub == 2) ? G[14 + i] : G[21 + i];
        }
    }
    __syncthreads();   // every quad has read its edge rows: they become GS / RS
    if (t < 4 * npb) {
        double* g = GS + c_jl * 28 + 7 * c_sub;   // [0..20] G0, [21..26] g0
#pragma unroll
        for (int i = 0; i < 7; i++) g[i] = gv[i];
    }
    if (t < npb) {
        if (a_first) RS[a_run] = t;
        if (t == 0) { RS[a_nruns] = npb; RS[65] = a_nruns; }
    }
    __syncthreads();
    // D. one lane per edge: its 48-B slot record U = Bi^T a / sqrt(D) and its 32-B edge record (P_c, scale), from which the Schur
    //    kernels rebuild Bi and Br = [-A | A N0], and with the pixel (obs_uvk) the weighted residual of g = -Bi^T r (idp_edge_wres:
    //    r2 stays here, it went into b_l and g0 through LDS).  Records live keyframe-major (slot_perm).
    if (t < ne) {
        const double sD = PT[pl * LIN2_PS + 17];
        const int pe = e_pe;
        double* sl = B.slot + VBA_SLOT * (size_t)(d.obs0 + d.pt0 + pe);
#pragma unroll
        for (int i = 0; i < 6; i++) sl[i] = ub[i] * sD;
        double2* dst = reinterpret_cast<double2*>(B.erec + VBA_EREC1 * (size_t)(d.obs0 + pe));
        dst[0] = make_double2(rpc[0], rpc[1]);
        dst[1] = make_double2(rpc[2], rsc);
    }
    // E. the reference-keyframe terms, one record per run: value v of run r is the sum over the run's landmarks, in order
    {
        const int nruns = RS[65];
        double* pr0 = B.prec + VBA_PREC * (size_t)(d.pt0 + B.prun0[d.lb0 + lb]);
        for (int idx = t; idx < nruns * 27; idx += 256) {
            const int r = idx / 27, v = idx - 27 * r;
            double sum = 0.0;
            for (int jl = RS[r]; jl < RS[r + 1]; jl++) sum += GS[jl * 28 + v];
            pr0[VBA_PREC * r + v] = sum;
        }
    }
    const double tot = block_sum256(chi, red);
    if (t == 0) B.part[d.part0 + lb] = tot;
}
__global__ void __launch_bounds__(256, 4) k_lin2(Batch B, int nblk_lin, int mode) {
    extern __shared__ double lsm[];
    lin2_body(B, nblk_lin, mode, lsm);
}
// Few windows: the IMU factors of the window in the SAME launch (the workgroups behind the edge workgroups, one keyframe pair
// each, wave 0) -- one launch and its latency less per linearisation pass; no occupancy to protect here, so no register cap
__global__ void __launch_bounds__(256) k_lin2_imu(Batch B, int nblk_lin, int mode) {
    extern __shared__ double lsm[];
    if ((int)blockIdx.x < nblk_lin) {
        lin2_body(B, nblk_lin, mode, lsm);
        return;
    }
    if (threadIdx.x >= 64) return;
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    if (!lin_imu_gate(d, B.ctrl[w], mode)) return;
    const int k = blockIdx.x - nblk_lin;
    if (k >= d.n_imu) return;
    if (threadIdx.x == 0) lin_imu_res(B, d, k, (mode == LIN_FULL) ? LIN_FULL : LIN_ERR);
    if (mode != LIN_FULL) return;
    __threadfence_block();              // lane 0's record (global memory) before the other lanes of this wave read it
    __builtin_amdgcn_wave_barrier();
    lin_imu_hess(B, d, k, lsm);
}

// ------------------------------------------------------------------------------------------------
// K_ctrl: one workgroup per window.  Sums the robust chi2 in a fixed order and runs the outer-loop
// logic of OptimizationAlgorithmGaussNewton::solve (gauss_newton.cpp:50-105) as driven by
// SparseOptimizer::optimize (sparse_optimizer.cpp:354-419).  final != 0: evaluation after the last iteration.
// ------------------------------------------------------------------------------------------------
DEVI double window_chi2(const Batch& B, const WinDesc& d, double* sm) {
    const int t = threadIdx.x;
    double s = 0;
    for (int k = t; k < d.n_imu; k += 64) {
        const int i = B.imu_i[d.imu0 + k], j = B.imu_j[d.imu0 + k];
        if (i < d.n_free || j < d.n_free) s += B.imu_chi[4 * (size_t)(d.imu0 + k)] + B.imu_chi[4 * (size_t)(d.imu0 + k) + 1];
    }
    for (int k = t; k < d.n_part_lin; k += 64) s += B.part[d.part0 + k];
    return block_sum<64>(s, sm);
}

// host_slot >= 0 (a single window, no profile): the launch reports through the pinned word alive_cnt[host_slot] itself -- 1: done, the
// window has stopped; 2: done, it goes on -- and the host reads that word instead of waiting for an event behind this kernel (an
// event record between two kernels of a stream costs the next one ~4 us).
__global__ void __launch_bounds__(64) k_ctrl_gn(Batch B, int final_eval, int host_slot) {
    __shared__ double sm[64];
    const int w = blockIdx.x;
    const WinDesc& d = B.desc[w];
    WinCtrl& c = B.ctrl[w];
    if (!c.active) {
        if (host_slot >= 0 && threadIdx.x == 0) __hip_atomic_store(B.alive_cnt + host_slot, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const double cur = window_chi2(B, d, sm);
    if (threadIdx.x != 0) return;
    const int st = c.stage, it = c.it;
    int active = 1;
    if (it >= 1) {
        c.its_done[st] = it;  // iterations 0..it-1 have run (++cjIterations)
        // solver Fail (zero / non-finite pivot, linear_solver_eigen.h:105-111): the step was dropped (k_update), this optimize() ends
        // (Terminate or Fail both leave the loop of sparse_optimizer.cpp:376), the window reports VBA_SOLVER_FAILED
        if (c.chol_fail) { c.status = -2; active = 0; }
        if (fabs(c.chi_prev - cur) < 1e-3) active = 0;  // Terminate, gauss_newton.cpp:97
    }
    if (final_eval || it >= d.its[st]) active = 0;
    if (active && poll_stop(B, c)) {  // terminate() before each iteration, sparse_optimizer.cpp:376
        c.aborted = 1;
        if (st == 0) c.status = 1;
        active = 0;
    }
    // the trace holds preChi2 of iteration 0 and afterChi2 of every iteration run: an optimize() stopped before its first
    // iteration has evaluated nothing
    if ((it >= 1 || active) && c.n_trace < VBA_TRACE) c.trace[c.n_trace++] = cur;
    // the probe (LIN_AUTO / LIN_REDO): a window that goes on behind a chi2-only pass owes the full one; its next pass is a probe when
    // this stage has a decrease to judge by (it >= 1) and that decrease was small.  The final evaluation is LIN_ERR for every window.
    if (final_eval) c.lin_probe = c.lin_redo = 0;
    else {
        const int redo = c.lin_probe && active;
        c.lin_redo = redo;
        c.n_redo += redo;
        c.lin_probe = B.lin_probe && active && it >= 1 && (B.lin_probe == 2 || fabs(c.chi_prev - cur) < LIN_PROBE_DCHI2);
    }
    c.chi_prev = cur;
    c.active = active;
    c.chol_fail = 0;
    c.it = it + 1;
    if (host_slot >= 0) {
        __hip_atomic_store(B.alive_cnt + host_slot, active ? 2 : 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    if (active && B.alive_cnt && it < 32 && atomicExch(B.alive_dev + st * 32 + it, 1) == 0)  // lets the host skip dead iterations
        __hip_atomic_store(B.alive_cnt + st * 32 + it, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);   // a posted store, not a PCIe atomic
}
