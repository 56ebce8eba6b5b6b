// vba_batch.h -- the Batch struct every solver kernel takes by value, the linearisation modes, and the kernels that set a
// run up: pads of S, the stop-flag mirror, reset of the working state, the active set of a stage.
// Reads the uploaded state (pose0, vel0, bias0, pt0, kf_fix, the record index lists) and the caller's stop word; writes the working
// copies, the R|t cache kfR, lvl / chi2_e, var_act and the control block WinCtrl.  Needs vba_device.h only; every other stage
// header needs this one.
#pragma once
#include "vba_device.h"

struct Batch {
    const WinDesc* desc;
    WinCtrl* ctrl;
    int n_win;
    // keyframe state: working copy, uploaded initial copy, LM backup, and the R|t cache the edges read
    double *pose, *vel, *bias, *kfR;
    const double *pose0, *vel0, *bias0;
    double *pose_bk, *vel_bk, *bias_bk;
    // landmarks
    double *pt;
    const double* pt0;
    double* pt_bk;
    const int *pt_ref, *pt_obs_begin;
    // observations (CSR by point)
    const int *obs_kf, *obs_pt;
    const double *obs_uv, *obs_w;
    const double* obs_uvk;        // [n_obs][2] inverse depth: obs_uv in RECORD order (slot_perm), beside the edge records (k_st_rec_fill)
    unsigned char* lvl;
    double *chi2_e, *depth_e, *chi2_f;  // chi2_f: chi2 recomputed at the final estimates (LM: chi2_e may be stale)
    double *erec, *prec, *slot;
    double2* lm_sd;               // [n_pt] inverse depth: (sqrt(Dinv), beta) of every landmark, at the caller's landmark index
    const int* slot_perm;         // [n_obs] record position of every observation edge (keyframe-major for inverse-depth windows)
    const int* pt_perm;           // [n_pt] record position of every landmark (grouped by reference keyframe)
    const unsigned char* kf_fix;  // [n_kf] per-vertex setFixed() of listed-free keyframes: bit0 PR, bit1 V, bit2 Bias
    // IMU factors
    const int *imu_i, *imu_j;
    const double *imu_meas, *imu_info;
    double *imuH, *imu_chi;  // imu_chi: [4] per edge: robust prv, robust bias, raw prv, raw bias
    double* imu_jrec;        // [IMU_JREC] per edge: Jacobian, weighted information, errors of the last linearisation (lin_imu_res -> lin_imu_hess)
    // reduced system
    double *S, *vec, *bpose;
    double *Lf, *yv;  // factor tiles and forward-substituted rhs (written out of place: S tiles are read by
                      // other workgroups of the same launch)
    int l_packed;     // Lf holds the factor tile by tile in MFMA operand order (left-looking kernels, ll_pk) instead of row-major
    int* var_act;
    // structure (g2o buildStructure analogue, built on the host at upload)
    const int *pair_a, *pair_b, *item_begin, *items, *pimu_begin, *pimu;
    const int *adj_begin, *adj;         // PCG: per free keyframe the other free keyframes it shares a landmark or an IMU edge with
    double* kf_dir;                     // XYZ landmarks: per keyframe the damping-independent part of its diagonal block and b_p (32 doubles)
    double *pcg_v, *pcg_m, *pcg_s;      // PCG: x r z p q (5 nS per window); preconditioner blocks (450 per keyframe); CG state (8 per window)
    int pcg_tri;                        // PCG: block-tridiagonal (keyframe chain) preconditioner instead of block-Jacobi
    const int *slot_o, *rec_lm;         // [n_obs] observation of the record in every slot; [n_pt] landmark of every landmark record
    const int* slot_lm;                 // [n_obs] landmark of the record in every slot (XYZ gathers fetch the landmark's Sigma through it)
    const int* item_mid;                // per pair: its first item that involves the landmark's reference keyframe
    const unsigned long long* lmask;    // [n_pt x mwords] observing keyframes of every landmark (host-built while validating)
    const int *kf_seg, *ref_seg;        // [n_kf + 1] per window: record range of every keyframe -- slot / edge records by observing
                                        // keyframe, landmark records by reference keyframe (the items of the diagonal pair (a,a))
    const int *off_pair, *pair_mask;  // off-diagonal pair indices; per pair: which sub-blocks of S are ever read
    const int* lin_blk;  // k_lin2: per workgroup its run of landmarks and edges (p0, p1, e0, e1), n_part_lin records per window
    // inverse depth: the reference-keyframe terms (G0, g0) leave k_lin2 summed over runs of consecutive landmarks with one reference
    // keyframe -- prun0[workgroup]: id of its first run record; per keyframe (rows at kf0 + win) the run records it is the
    // reference of: pref_list[pt0 + pref_begin[k] .. pref_begin[k + 1])
    const int *prun0, *pref_begin, *pref_list;
    // tile structure of the factor (symbolic factorisation on 32x32 tiles, built at upload)
    const int *tl_step_begin, *tl_pairs, *tl_pan_begin, *tl_pan;
    const int *tl_kl_begin, *tl_kl;  // left-looking factorisation: per column entry (J,J),(I,J).. the steps k < J that update it
    const int* tl_ct;                // per chain column: row mask (two words), rides, 0 (Structure::chain_tab)
    const int* tl_cu;                // few-window regime: tiles behind the chain columns that collect updates from them (I << 16 | J, first, end of the chain columns in its k list, 0)
    double *dvec, *winv;             // D of the factor (nS per window); L_JJ^-T D_J^-1 of the current step (32x32 per window)
    int w_total, w_stride;           // behind those: W_J of every chain column, w_stride tiles per window (batch-wide window index d.win)
    double* part;
    const volatile int* stop_word;   // DEVICE copy of the caller's stop flag (word 1023 of the group's mirror words), refreshed by k_poll_stop
                                     // before every control launch: thousands of windows reading the pinned host word cost 0.5 ms per launch
    const volatile int* stop_host_word;   // the pinned host word itself
    int* alive_cnt;  // pinned host words: [stage * 32 + it] = 1 if a window is still iterating after control call `it`
    int* alive_dev;  // device mirror of the group's words ([0,64): Gauss-Newton slots, [64,1024): LM slot groups), zeroed at run start:
                     // only the FIRST window that flips a mirror word writes the host word (thousands of windows posting the same
                     // 4 bytes over PCIe cost 0.4 ms per control launch)
    unsigned char* out_outlier;
    double* out_chi2;
    double* dbg;  // 4 KiB scratch for diagnostic builds (in-kernel stamps); never read by the product path
    int dbg_stop_after;  // test hook (vba_debug_set_stop_after): >= 0 -- the stop flag reads 1 from that poll of a window on; -1: off
    int lin_probe;       // the run's RunPlan::lin_probe (k_ctrl_gn): 0 no window ever probes, 1 by the last chi2 decrease, 2 every pass it may
};

#define LIN_FULL 0
#define LIN_ERR 1
// (2: LIN_ERR_TRIAL of the Levenberg-Marquardt schedule, vba_kernels_lm.h)
// Gauss-Newton, inverse-depth variant, probing on (vba_host::plan_lin_probe).  The pass in which a window stops by |dchi2| < 1e-3
// is read for its chi2 alone: its Jacobians, its 80 B of records per edge and its IMU Hessians are never used.  So after an
// iteration whose chi2 decrease was below LIN_PROBE_DCHI2 the window's next pass is a PROBE -- the LIN_ERR path, the same chi2
// from the same instructions, no stores -- and only if the window then goes on is the full pass run, before the solve:
//   LIN_AUTO  a window with WinCtrl::lin_probe takes LIN_ERR, every other one LIN_FULL
//   LIN_REDO  behind the control launch: the windows with WinCtrl::lin_redo take LIN_FULL, the others exit at once
// Both resolve per window, hence uniformly over a workgroup (lin_mode_of).
#define LIN_AUTO 3
#define LIN_REDO 4
#define LIN_SKIP (-1)
#define LIN_PROBE_DCHI2 10.0

// One read of the caller's stop flag by one window: g2o's terminate() before an iteration (sparse_optimizer.cpp:376), inside the
// Levenberg-Marquardt trial loop (levenberg.cpp:149), and the bDoMore check between the stages (src/Optimizer.cpp:462-466).  The
// polls of a window are counted from the first terminate() of its first optimize() so that a test can raise the flag at a chosen
// poll (dbg_stop_after) -- the deterministic stand-in for LocalMapping::InterruptBA firing in the middle of a solve; the oracle
// counts the same polls (stop_now in oracle/vba_oracle.c).  Thread 0 of the window's control workgroup only.
DEVI int poll_stop(const Batch& B, WinCtrl& c) {
    const int n = c.polls++;
    return ((B.stop_word && *B.stop_word) || (B.dbg_stop_after >= 0 && n >= B.dbg_stop_after)) ? 1 : 0;
}

// window takes part in the current solve: GN -> while its optimize() loop runs; LM -> only while a trial is due
DEVI bool win_on(const WinDesc& d, const WinCtrl& c) { return c.active && (d.algo == 0 || c.lm_need_trial); }

// ------------------------------------------------------------------------------------------------
// K_reset: working state <- uploaded state, R|t cache, control block
// ------------------------------------------------------------------------------------------------
DEVI void kf_cache(const Batch& B, const WinDesc& d, int a) {
    const double* T = B.pose + 7 * (size_t)(d.kf0 + a);
    double* C = B.kfR + 12 * (size_t)(d.kf0 + a);
    double R[9];
    q2R(T + 3, R);
#pragma unroll
    for (int i = 0; i < 9; i++) C[i] = R[i];
    C[9] = T[0]; C[10] = T[1]; C[11] = T[2];
}

// free vertices of keyframe kf: bit0 PR, bit1 V, bit2 Bias (0 for the keyframes listed as fixed)
DEVI int kf_free(const Batch& B, const WinDesc& d, int kf) {
    if (kf >= d.n_free) return 0;
    return 7 & ~(int)B.kf_fix[d.kf0 + kf];
}
// allVerticesFixed edges are dropped (sparse_optimizer.cpp:236): bit0 EdgeNavStatePRV (PR_i PR_j V_i V_j Bias_i),
// bit1 EdgeNavStateBias (Bias_i Bias_j)
DEVI int imu_act(const Batch& B, const WinDesc& d, int i, int j) {
    const int fi = kf_free(B, d, i), fj = kf_free(B, d, j);
    return ((fi | (fj & 3)) ? 1 : 0) | (((fi | fj) & 4) ? 2 : 0);
}
DEVI bool imu_robust(const WinDesc& d) { return !(d.protocol == 1 && !d.robust); }

// upload: identity on the padded diagonal of S (rows np..nS, fewer than VBA_NB of them); the solve never touches the pads
__global__ void __launch_bounds__(64) k_init_pads(Batch B) {
    const WinDesc& d = B.desc[blockIdx.x];
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int i = d.pad0[q] + threadIdx.x;
        if ((int)threadIdx.x < d.padn[q]) B.S[d.S0 + (size_t)i * d.nS + i] = 1.0;
    }
}

// one PCIe read per control launch instead of one per window
__global__ void k_poll_stop(Batch B) { *const_cast<int*>(B.stop_word) = *B.stop_host_word; }

__global__ void __launch_bounds__(256) k_reset(Batch B) {
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    // flat, coalesced copies: consecutive threads take consecutive doubles of each array (the first version gave every thread a
    // whole keyframe / landmark: stride-7 / -3 / -12 scalar loops, 6 ms per 4096 windows)
    const int stride = gridDim.x * 256, t0 = blockIdx.x * 256 + threadIdx.x;
    const size_t k0 = d.kf0, p0 = d.pt0, o0 = d.obs0;
    for (int i = t0; i < 7 * d.n_kf; i += stride) B.pose[7 * k0 + i] = B.pose0[7 * k0 + i];
    for (int i = t0; i < 3 * d.n_kf; i += stride) B.vel[3 * k0 + i] = B.vel0[3 * k0 + i];
    for (int i = t0; i < 12 * d.n_kf; i += stride) B.bias[12 * k0 + i] = B.bias0[12 * k0 + i];
    for (int i = t0; i < 3 * d.n_pt; i += stride) B.pt[3 * p0 + i] = B.pt0[3 * p0 + i];
    for (int i = t0; i < d.n_obs; i += stride) { B.lvl[o0 + i] = 0; B.chi2_e[o0 + i] = 0.0; }
    for (int a = t0; a < d.n_kf; a += stride) {   // R|t cache from the UPLOADED pose (the working copy is being written by other threads)
        const double* T = B.pose0 + 7 * (k0 + a);
        double* C = B.kfR + 12 * (k0 + a);
        double R[9];
        q2R(T + 3, R);
#pragma unroll
        for (int i = 0; i < 9; i++) C[i] = R[i];
        C[9] = T[0]; C[10] = T[1]; C[11] = T[2];
    }
    if (t0 == 0) {
        WinCtrl& c = B.ctrl[w];
        c.stage = 0; c.it = 0; c.active = 0; c.status = 0;
        c.its_done[0] = c.its_done[1] = 0;
        c.robust_vis = (d.protocol == 1) ? (d.robust != 0) : 1;
        c.chol_fail = 0; c.aborted = 0;
        c.n_trace = 0; c.n_outliers = 0;
        c.lm_trial = 0; c.lm_need_trial = 0; c.nbad = 0; c.lin_its = 0; c.polls = 0;
        c.lambda = 0; c.ni = 2; c.chi_prev = 0; c.chi_ini = 0;
        c.chi2_vis = c.chi2_prv = c.chi2_bias = 0;
        c.lin_probe = c.lin_redo = 0; c.n_probe = c.n_redo = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// K_stage: initializeOptimization(level) -- active set of the stage (sparse_optimizer.cpp:199-267)
//   phase 0: clear var_act, arm the control block.  phase 1: mark variables touched by an active edge.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_stage_clear(Batch B, int stage) {
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    WinCtrl& c = B.ctrl[w];
    const int t = blockIdx.x * 64 + threadIdx.x;
    if (t < d.nS) B.var_act[d.vec0 + t] = 0;
    if (t == 0) {
        if (stage == 0) {
            const int stop = B.stop_word ? *B.stop_word : 0;   // the check on entry: not one of the counted polls
            if (stop) { c.aborted = 1; c.status = 2; c.active = 0; }  // src/Optimizer.cpp:453-455
            else c.active = 1;
        } else if (d.protocol == 1) {
            c.active = 0;  // BundleAdjustment: a single optimize(nIterations), no second stage (:3517, :835)
        } else {
            const int stop = (c.status == 2) ? 1 : poll_stop(B, c);
            if (c.aborted || stop) {  // :462-470 -- skip stage 2
                if (!c.aborted) { c.aborted = 1; c.status = 1; }
                c.active = 0;
            } else {
                c.active = 1;
                c.lambda = 0;  // the second optimize() starts its own lambda (computeLambdaInit at its iteration 0)
            }
            c.robust_vis = 0;  // e->setRobustKernel(0) on every vision edge, :489
        }
        if (d.its[stage] <= 0) c.active = 0;  // optimize(0) runs nothing
        c.stage = stage; c.it = 0; c.chol_fail = 0;
        c.lm_trial = 0; c.lm_need_trial = 0; c.nbad = 0; c.ni = 2;
        c.lin_probe = c.lin_redo = 0;   // a stage starts with no chi2 decrease behind it
    }
}

// One wave per (window, keyframe): the keyframe's PR block is in the index mapping if one of its edges is active -- as the
// observer (its slot records, in slot order) or, for inverse-depth landmarks, as the reference keyframe of a landmark with an
// active edge.  The wave stops at the first hit, which is almost always in its first 64 records.  (Round 1: a thread per edge,
// five dependent loads each, 1.9 ms per 4096 windows.)  Blocks behind the keyframes: the IMU edges, a thread each.
__global__ void __launch_bounds__(64) k_stage_mark(Batch B, int nblk_kf) {
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    int* va = B.var_act + d.vec0;
    const int lane = threadIdx.x;
    if ((int)blockIdx.x < nblk_kf) {
        const int a = blockIdx.x;
        if (a >= d.n_free || !(kf_free(B, d, a) & 1)) return;
        const int* kseg = B.kf_seg + d.kf0 + d.win;
        bool hit = false;
        for (int c = kseg[a]; c < kseg[a + 1] && !hit; c += 64) {
            const int slot = c + lane;
            const bool on = slot < kseg[a + 1] && !B.lvl[d.obs0 + B.slot_o[d.obs0 + slot]];
            hit = __ballot(on) != 0ull;
        }
        if (!hit && d.variant == 2) {
            const int* rseg = B.ref_seg + d.kf0 + d.win;
            const int* ob = B.pt_obs_begin + d.pt0 + d.win;
            for (int c = rseg[a]; c < rseg[a + 1] && !hit; c += 64) {
                const int rec = c + lane;
                bool on = false;
                if (rec < rseg[a + 1]) {
                    const int p = B.rec_lm[d.pt0 + rec];
                    for (int o = ob[p]; o < ob[p + 1] && !on; o++) on = !B.lvl[d.obs0 + o];
                }
                hit = __ballot(on) != 0ull;
            }
        }
        if (hit && lane < 6) va[vpos(d, a, lane)] = 1;
        return;
    }
    const int t = (blockIdx.x - nblk_kf) * 64 + lane;
    if (t < d.n_imu) {
        const int i = B.imu_i[d.imu0 + t], j = B.imu_j[d.imu0 + t];
        const int fi = kf_free(B, d, i), fj = kf_free(B, d, j), act = imu_act(B, d, i, j);
        // the PRV edge touches PR_i, PR_j, V_i, V_j, Bias_i; the bias edge Bias_i, Bias_j
        for (int k = 0; k < 15; k++) {
            const int part = (k < 6) ? 0 : ((k < 9) ? 1 : 2);
            if (((fi >> part) & 1) && ((act & 1) || (part == 2 && (act & 2)))) va[vpos(d, i, k)] = 1;
            if (((fj >> part) & 1) && ((part < 2 && (act & 1)) || (part == 2 && (act & 2)))) va[vpos(d, j, k)] = 1;
        }
    }
}
