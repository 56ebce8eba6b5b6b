// vba_update.h -- what follows the solve: landmark back-substitution fused with the vertex retractions (k_update), the outlier
// pass between the stages (k_classify) and the final chi2 (k_final_edges, k_final_sum).
// Reads the pose step vec and the records of the linearisation; writes pose, vel, bias, pt, kfR, lvl, chi2_f and the outputs
// out_outlier / out_chi2.  Needs vba_batch.h and vba_lin.h (idp_edge_eval).
#pragma once
#include "vba_batch.h"
#include "vba_lin.h"

// ------------------------------------------------------------------------------------------------
// K_update: landmark back-substitution x_l = Dinv (b_l - W^T x_p) (block_solver.hpp:461-481) fused with the
// vertex retractions (SparseOptimizer::update -> oplusImpl): blocks [0,nblk_pt) landmarks, then keyframes.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_update(Batch B, int nblk_pt) {
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    const WinCtrl& c = B.ctrl[w];
    if (!c.active || c.chol_fail) return;
    const double* x = B.vec + d.vec0;
    const int P = d.pdim;
    if ((int)blockIdx.x < nblk_pt) {
        const int p = blockIdx.x * 64 + threadIdx.x;
        if (p >= d.n_pt) return;
        const size_t gp = d.pt0 + p;
        const double2 sb = B.lm_sd[gp];   // (sqrt(Dinv), beta): coalesced, and ahead of the pt_perm hop to the reference record
        const int pp = B.pt_perm[gp];
        const double sD = sb.x;
        if (!(sD > 0.0)) return;  // landmark outside the active set: 16 bytes read, no slot line
        const double* slots = B.slot + VBA_SLOT * (size_t)(d.obs0 + d.pt0);
        const double* sr = slots + VBA_SLOT * (size_t)(d.n_obs + pp);
        double cl = sb.y;         // beta - sum U . x_p
        const int rf = B.pt_ref[gp];
        if (rf < d.n_free)
#pragma unroll
            for (int i = 0; i < 6; i++) cl -= sr[i] * x[vpos(d, rf, i)];
        const int* ob = B.pt_obs_begin + d.pt0 + d.win;
        // two edges per trip, their indices fetched one trip ahead: per landmark ~n/2 + 1 dependent round trips instead of 2 n
        const int o0 = ob[p], o1 = ob[p + 1];
        int kfn[2] = {0, 0}, spn[2] = {0, 0};
#pragma unroll
        for (int u = 0; u < 2; u++)
            if (o0 + u < o1) { kfn[u] = B.obs_kf[d.obs0 + o0 + u]; spn[u] = B.slot_perm[d.obs0 + o0 + u]; }
        for (int o = o0; o < o1; o += 2) {
            const int kf0 = kfn[0], kf1 = kfn[1], sp0 = spn[0], sp1 = spn[1];
            const bool two = o + 1 < o1;
#pragma unroll
            for (int u = 0; u < 2; u++)
                if (o + 2 + u < o1) { kfn[u] = B.obs_kf[d.obs0 + o + 2 + u]; spn[u] = B.slot_perm[d.obs0 + o + 2 + u]; }
            const bool on0 = kf0 < d.n_free, on1 = two && kf1 < d.n_free;
            const double* sl0 = slots + VBA_SLOT * (size_t)sp0;
            const double* sl1 = slots + VBA_SLOT * (size_t)(on1 ? sp1 : sp0);
            double u0[6], u1[6], x0[6], x1[6];
#pragma unroll
            for (int i = 0; i < 6; i++) {
                u0[i] = sl0[i]; u1[i] = sl1[i];
                x0[i] = x[vpos(d, on0 ? kf0 : 0, i)]; x1[i] = x[vpos(d, on1 ? kf1 : 0, i)];
            }
            if (on0) {
#pragma unroll
                for (int i = 0; i < 6; i++) cl -= u0[i] * x0[i];
            }
            if (on1) {
#pragma unroll
                for (int i = 0; i < 6; i++) cl -= u1[i] * x1[i];
            }
        }
        double rho = B.pt[3 * gp] + sD * cl;
        if (rho < 1e-6) rho = 1e-6;  // VertexIDP::oplusImpl, g2otypes.h:50-55
        B.pt[3 * gp] = rho;
    } else {
        const int a = (blockIdx.x - nblk_pt) * 64 + threadIdx.x;
        if (a >= d.n_free) return;
        const int* va = B.var_act + d.vec0;
        double dx[15];
        for (int i = 0; i < P; i++) dx[i] = x[vpos(d, a, i)];
        const size_t gk = d.kf0 + a;
        if (va[vpos(d, a, 0)]) {  // NavState::IncSmallPR, NavState.cpp:63-70
            double* T = B.pose + 7 * gk;
            T[0] += dx[0]; T[1] += dx[1]; T[2] += dx[2];
            double dq[4], qn[4];
            so3exp(dx + 3, dq);
            so3mul(T + 3, dq, qn);
            T[3] = qn[0]; T[4] = qn[1]; T[5] = qn[2]; T[6] = qn[3];
            kf_cache(B, d, a);
        }
        if (P == 15) {
            if (va[vpos(d, a, 6)])
                for (int i = 0; i < 3; i++) B.vel[3 * gk + i] += dx[6 + i];
            if (va[vpos(d, a, 9)])
                for (int i = 0; i < 6; i++) B.bias[12 * gk + 6 + i] += dx[9 + i];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K_classify: outlier pass between the stages (src/Optimizer.cpp:475-490): chi2 from the stored error,
// depth and rho at the current estimate.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_classify(Batch B) {
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    const WinCtrl& c = B.ctrl[w];
    if (!c.active) return;  // bDoMore == false (latched by k_stage_clear(1)) or aborted on entry
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= d.n_obs) return;
    const size_t go = d.obs0 + o;
    double s, depth;
    if (d.variant == 2) {   // inverse depth: evaluated here (idp_edge_eval); the value is kept for the edges this pass takes out --
        idp_edge_eval(B, d, go, s, depth);   // e->chi2() of a level-1 edge stays what it was when the edge left the optimisation
        B.chi2_e[go] = s;
    } else { s = B.chi2_e[go]; depth = B.depth_e[go]; }
    bool bad = (s > d.chi2_th) || !(depth > d.depth_min);
    if (d.variant == 2 && B.pt[3 * (size_t)(d.pt0 + B.obs_pt[go])] < d.rho_min) bad = true;
    if (bad) B.lvl[go] = 1;
}

// K_final: erase list + chi2 of the level-0 edges at the final estimates (src/Optimizer.cpp:496-517)
__global__ void __launch_bounds__(64) k_final_edges(Batch B) {
    __shared__ double sm[64];
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    const int o = blockIdx.x * 64 + threadIdx.x;
    if ((int)blockIdx.x * 64 >= d.n_obs) return;
    // a window stopped at the very first terminate() of its first optimize() has evaluated nothing: e->chi2() then reads an _error
    // no computeError() ever wrote (uninitialised in g2o; zero here and in the oracle) -- the launch schedule has linearised once
    // before that poll, but those values do not exist for the protocol
    const bool never = B.ctrl[w].n_trace == 0;
    double chi = 0.0, cnt = 0.0;
    if (o < d.n_obs) {
        const size_t go = d.obs0 + o;
        // e->chi2() at the final estimates (what the last linearisation computed); for an edge the outlier pass took out: its value
        // at that pass (k_classify); the depth is evaluated at the final estimates for every edge (isDepthPositive())
        double stored, depth;
        if (d.variant == 2) {
            idp_edge_eval(B, d, go, stored, depth);
            if (B.lvl[go]) stored = B.chi2_e[go];
        } else { stored = B.chi2_e[go]; depth = B.depth_e[go]; }
        const double s = never ? 0.0 : stored;
        bool bad = (s > d.chi2_th) || !(depth > d.depth_min);
        if (d.variant == 2 && (B.pt[3 * (size_t)(d.pt0 + B.obs_pt[go])] < d.rho_min || B.lvl[go])) bad = true;
        if (d.protocol == 1) bad = false;  // global BA classifies nothing
        B.out_outlier[go] = bad ? 1 : 0;
        B.out_chi2[go] = s;
        if (!B.lvl[go]) chi = B.chi2_f ? B.chi2_f[go] : stored;
        cnt = bad ? 1.0 : 0.0;
    }
    const double tc = block_sum<64>(chi, sm);
    const double tn = block_sum<64>(cnt, sm);
    if (threadIdx.x == 0) {
        B.part[d.part0 + 2 * blockIdx.x] = tc;
        B.part[d.part0 + 2 * blockIdx.x + 1] = tn;
    }
}

__global__ void __launch_bounds__(64) k_final_sum(Batch B) {
    __shared__ double sm[64];
    const int w = blockIdx.x;
    const WinDesc& d = B.desc[w];
    WinCtrl& c = B.ctrl[w];
    const int t = threadIdx.x;
    const int nblk = (d.n_obs + 63) / 64;
    double s = 0, nn = 0, sp = 0, sbias = 0;
    for (int k = t; k < nblk; k += 64) { s += B.part[d.part0 + 2 * k]; nn += B.part[d.part0 + 2 * k + 1]; }
    for (int k = t; k < d.n_imu; k += 64) {
        const int i = B.imu_i[d.imu0 + k], j = B.imu_j[d.imu0 + k];
        if (i < d.n_free || j < d.n_free) { sp += B.imu_chi[4 * (size_t)(d.imu0 + k) + 2]; sbias += B.imu_chi[4 * (size_t)(d.imu0 + k) + 3]; }
    }
    s = block_sum<64>(s, sm);
    nn = block_sum<64>(nn, sm);
    sp = block_sum<64>(sp, sm);
    sbias = block_sum<64>(sbias, sm);
    if (t == 0) {
        if (c.status == 2) { c.n_outliers = 0; return; }
        c.chi2_vis = s; c.chi2_prv = sp; c.chi2_bias = sbias; c.n_outliers = (int)(nn + 0.5);
    }
}
