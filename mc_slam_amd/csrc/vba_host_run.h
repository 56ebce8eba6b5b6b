// vba_host_run.h -- host side of the library, part 3: the launch schedule of a run (Gauss-Newton and Levenberg-Marquardt, on
// explicit window groups), vba_batch_run and vba_batch_download.
#pragma once

namespace {

// The caller's stop flag (g2o's forceStopFlag, sparse_optimizer.h:188) at ITS width: the reference hands over `bool* pbStopFlag` =
// &LocalMapping::mbAbortBA, one byte that the Tracking thread writes (include/Optimizer.h:22-24, src/LocalMapping.cpp:1769-1772);
// a C caller may keep an int.  The byte / word is read, never written.
struct StopRef {
    const volatile void* p = nullptr;
    int width = 0;   // bytes: 1 (vba_*_b) or 4
    bool set() const {
        if (!p) return false;
        return width == 1 ? *reinterpret_cast<const volatile unsigned char*>(p) != 0 : *reinterpret_cast<const volatile int*>(p) != 0;
    }
    explicit operator bool() const { return p != nullptr; }
};
StopRef stop_int(const volatile int* f) { StopRef r; r.p = f; r.width = 4; return r; }
StopRef stop_byte(const volatile unsigned char* f) { StopRef r; r.p = f; r.width = 1; return r; }

// ---- the launch schedule ------------------------------------------------------------------------------
// g2o polls forceStopFlag before every iteration (sparse_optimizer.cpp:376).  The device reads a pinned word; whoever enqueues or
// waits on the host copies the caller's flag into it -- at every iteration it enqueues and while it waits for the device.
inline void forward_stop(Handle* h, StopRef stop_flag) {
    if (stop_flag.set()) *h->stop_host = 1;
}
hipError_t wait_event_forwarding(Handle* h, hipEvent_t ev, StopRef stop_flag) {
    if (!stop_flag) return hipEventSynchronize(ev);
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        forward_stop(h, stop_flag);
        std::this_thread::yield();
    }
}
// One group of windows of a batch with its own stream (the whole batch is the only group unless VBA_STREAMS > 1): what the
// enqueue functions launch on -- they read the batch's kernel choice and launch geometry from the handle, never its B / n_win / stream
struct Group {
    Batch B;
    int n_win;
    int index;            // which group of the run: its pinned words
    hipStream_t stream;
    volatile int* alive;  // pinned words of this group: [stage * 32 + it]
    bool dead;
};
using vba_host::xcd_windows;

#ifdef VBA_TEST_HOOKS
// vba_debug_capture: the captured items (per window: vba_debug_capture_get) and the kernel paths an iteration took
enum { CAP_POSE_A, CAP_VEL_A, CAP_BIAS_A, CAP_PT_A, CAP_CTRL_A, CAP_LVL_A, CAP_VARACT_A, CAP_S_B, CAP_VEC_B, CAP_LF_C, CAP_YV_C,
       CAP_VEC_C, CAP_POSE_D, CAP_VEL_D, CAP_BIAS_D, CAP_PT_D, CAP_N };
// the device buffer and the batch-wide byte count of every captured item
void cap_source(Handle* h, int what, int& buf, size_t& bytes) {
    static const int ids[CAP_N] = {BUF_POSE, BUF_VEL, BUF_BIAS, BUF_PT, BUF_CTRL, BUF_LVL, BUF_VARACT, BUF_S, BUF_VEC, BUF_LF, BUF_YV,
                                   BUF_VEC, BUF_POSE, BUF_VEL, BUF_BIAS, BUF_PT};
    const WinDesc& e = h->desc.back();
    const size_t kf = (size_t)e.kf0 + e.n_kf, pt = (size_t)e.pt0 + e.n_pt, vec = (size_t)e.vec0 + e.nS;
    const size_t sz[CAP_N] = {56 * kf, 24 * kf, 96 * kf, 24 * pt, sizeof(WinCtrl) * h->desc.size(), (size_t)e.obs0 + e.n_obs, 4 * vec,
                              8 * ((size_t)e.S0 + (size_t)e.nS * e.nS), 8 * vec, 8 * ((size_t)e.S0 + (size_t)e.nS * e.nS), 8 * vec, 8 * vec,
                              56 * kf, 24 * kf, 96 * kf, 24 * pt};
    buf = ids[what];
    bytes = sz[what];
}
// enqueue the device-to-device copies of items [first, last) on the run stream (the batch runs as one group: checked in do_run)
void cap_copy(Handle* h, hipStream_t stream, int first, int last) {
    if (h->cap_call < 0 || h->cap_count != h->cap_call) return;
    for (int q = first; q < last; q++) {
        int id;
        size_t bytes;
        cap_source(h, q, id, bytes);
        if (bytes > h->cap[q].cap) continue;   // (do_run sized every capture buffer)
        (void)hipMemcpyAsync(h->cap[q].p, h->buf[id].ptr(), bytes, hipMemcpyDeviceToDevice, stream);
        h->cap_bytes[q] = bytes;
    }
}
#define CAP_COPY(h, st, a, b) cap_copy(h, st, a, b)
#define CAP_PATH(h, i, v) do { if ((h)->cap_call >= 0 && (h)->cap_count == (h)->cap_call) (h)->cap_path[i] = (v); } while (0)
#else
#define CAP_COPY(h, st, a, b) do { } while (0)
#define CAP_PATH(h, i, v) do { } while (0)
#endif

// One solve iteration of a group.  WHICH kernels: the run's plan (h->rp, decided for the whole batch: vba_host_plan.h); grid sizes:
// the group's n_win; what is tested here is geometry only.  CAP_PATH records what was launched (vba_debug_window_layout [10..12]).
void enqueue_solve_iteration(Handle* h, const Group& g, StopRef stop_flag = StopRef()) {
    const Batch& B = g.B;
    const LaunchGeom& L = h->geom;
    hipStream_t stream = g.stream;
    const vba_host::RunPlan& P = h->rp;
    const int n = g.n_win;          // windows of this group: grid sizes
    const bool idp = h->variant == VBA_VARIANT_PRV_IDP;
    const int ngrp = xcd_windows(n);
    CAP_COPY(h, stream, CAP_POSE_A, CAP_VARACT_A + 1);
    {
        ProfScope ps(h, stream, VBA_PROF_SCHUR);
        using namespace vba_host;   // (CAP_SCHUR_*: the plan's value selects, the launch site records what it launched)
        const bool quads = P.schur == CAP_SCHUR_SPLIT || P.schur == CAP_SCHUR3;   // off-diagonal blocks per quad of pairs, XCD-mapped
        switch (P.schur) {
        case CAP_SCHUR_ALL:
            CAP_PATH(h, 0, CAP_SCHUR_ALL);
            VBA_LAUNCH(k_schur_all, dim3((L.max_free + L.max_quads) * ngrp), dim3(64), 0, stream, B, L.max_free, L.max_quads);
            break;
        case CAP_SCHUR_ALL_W:
            CAP_PATH(h, 0, CAP_SCHUR_ALL_W);
            VBA_LAUNCH(k_schur_all_w, dim3((L.max_free + L.max_offp) * ngrp), dim3(64), 0, stream, B, L.max_free, L.max_offp);
            break;
        case CAP_SCHUR_SPLIT:
        case CAP_SCHUR_SPLIT_W:
            CAP_PATH(h, 0, quads ? CAP_SCHUR_SPLIT : CAP_SCHUR_SPLIT_W);
            VBA_LAUNCH(k_schur_diag, dim3(L.max_free * ngrp), dim3(64), 0, stream, B, L.max_free);
            if (quads) VBA_LAUNCH(k_schur_off, dim3(L.max_quads * ngrp), dim3(64), 0, stream, B, L.max_quads);
            else VBA_LAUNCH(k_schur_off_w, dim3(L.max_offp * ngrp), dim3(64), 0, stream, B, L.max_offp);
            break;
        default:   // CAP_SCHUR3, CAP_SCHUR3_W
            CAP_PATH(h, 0, quads ? CAP_SCHUR3 : CAP_SCHUR3_W);
            VBA_LAUNCH(k_dinv, dim3(L.max_pt_blk, n), dim3(64), 0, stream, B);
            VBA_LAUNCH(k_schur_diag3, dim3(L.max_free * ngrp), dim3(64), 0, stream, B, L.max_free, 0);
            if (quads) VBA_LAUNCH(k_schur_off3, dim3(L.max_quads * ngrp), dim3(64), 0, stream, B, L.max_quads);
            else VBA_LAUNCH(k_schur_off3_w, dim3(L.max_offp * ngrp), dim3(64), 0, stream, B, L.max_offp);
        }
    }
    CAP_COPY(h, stream, CAP_S_B, CAP_VEC_B + 1);
    if (P.factor == vba_host::CAP_FACTOR_PCG) {
        // Two launches per CG iteration for all windows of the group; the host enqueues BATCHES of iterations and reads one pinned
        // word per batch (did any window go on?) two batches behind the device.  Converged windows exit at the first instruction.
        ProfScope ps(h, stream, VBA_PROF_FACTOR);
        const size_t pcg_shm = (size_t)L.max_free * 16 * sizeof(double);   // the sweeps of the tridiagonal preconditioner
        VBA_LAUNCH(k_pcg_init, dim3(n), dim3(256), pcg_shm, stream, B);
        const int per_batch = 32, RING = 16, row_blocks = (L.max_nS + PCG_ROWS - 1) / PCG_ROWS;
        volatile int* ring = h->stop_host + 1024 + 16 * g.index;
        int* ring_dev = h->stop_dev + 1024 + 16 * g.index;
        std::vector<hipEvent_t> ev;
        const int max_batches = (20 * L.max_nS + 50) / per_batch + 2;
        for (int b = 0; b < max_batches; b++) {
            if (b >= 2) {
                (void)wait_event_forwarding(h, ev[b - 2], stop_flag);
                if (ring[(b - 2) % RING] == 0) break;   // every window had converged (or broken down) by the end of batch b-2
            }
            forward_stop(h, stop_flag);
            ring[b % RING] = 0;
            for (int it = 0; it < per_batch; it++) {
                VBA_LAUNCH(k_pcg_matvec, dim3(row_blocks, n), dim3(256), 0, stream, B);
                VBA_LAUNCH(k_pcg_step, dim3(n), dim3(256), pcg_shm, stream, B, ring_dev + (b % RING));
            }
            ev.push_back(get_evt(h));
            (void)hipEventRecord(ev.back(), stream);
        }
        VBA_LAUNCH(k_pcg_finish, dim3(n), dim3(256), 0, stream, B);
        CAP_PATH(h, 1, vba_host::CAP_FACTOR_PCG);
        CAP_COPY(h, stream, CAP_VEC_C, CAP_VEC_C + 1);
    } else {
    {
        ProfScope ps(h, stream, VBA_PROF_FACTOR);
        // the chain columns [0, nc) of every window in one launch (vba_chain.h); the per-column kernels start behind them
        const int k_first = L.max_nc > 0 ? std::min(L.min_nc, L.max_nc) : 0;
        if (L.max_nc > 0) {
            if (P.factor == vba_host::CAP_FACTOR_LL) {
                VBA_LAUNCH(k_chol_chain_diag, dim3(n), dim3(64), 0, stream, B);
                if (L.max_chain_rows > 0) VBA_LAUNCH(k_chol_chain_panel, dim3(L.max_chain_rows * ngrp), dim3(64), 0, stream, B, L.max_chain_rows);
            }
            else {
                VBA_LAUNCH(k_chol_chain_rows, dim3(std::max(1, L.max_chain_rows), n), dim3(L.max_split > 0 ? 512 : 256), 0, stream, B);   // (two chains: two halves)
                if (L.max_cu > 0) VBA_LAUNCH(k_chol_chain_upd, dim3(L.max_cu, n), dim3(512), 0, stream, B);
            }
        }
        if (P.factor == vba_host::CAP_FACTOR_LL) {
            CAP_PATH(h, 1, vba_host::CAP_FACTOR_LL);
            for (int k = k_first; k < L.max_nb; k++) {  // every tile read once, updated in registers, written once
                VBA_LAUNCH(k_chol_diag_ll2, dim3(n), dim3(64), 0, stream, B, k);
                if (L.pan_grid[k] > 0) VBA_LAUNCH(k_chol_panel_ll, dim3(L.pan_grid[k] * ngrp), dim3(64), 0, stream, B, k, L.pan_grid[k]);
            }
        } else {
            for (int k = k_first; k < L.max_nb; k++) {
                // one window: descriptor and step table ride in the kernel arguments, for the columns the step table covers
                const bool one = P.factor == vba_host::CAP_FACTOR_STEP4_ONE && (int)h->one_sb.size() > k + 1;
                // (the capture reports the step kernel of the columns; columns that took different ones: CAP_FACTOR_MIXED)
                const int form = (P.factor == vba_host::CAP_FACTOR_STEP4_ONE && !one) ? vba_host::CAP_FACTOR_STEP4 : P.factor;
                CAP_PATH(h, 1, (k == k_first || h->cap_path[1] == form) ? form : vba_host::CAP_FACTOR_MIXED);
                (void)form;
                if (P.factor == vba_host::CAP_FACTOR_STEP1) VBA_LAUNCH(k_chol_step, dim3(L.step_grid[k], n), dim3(64), 0, stream, B, k);
                else if (one) {
                    const WinDesc& d0 = h->desc[0];
                    StepOne so;
                    so.algo = d0.algo; so.nS = d0.nS; so.nb = d0.nb; so.vec0 = d0.vec0; so.S0 = d0.S0;
                    so.pair_off = d0.tl_pair0 + h->one_sb[k]; so.npair = h->one_sb[k + 1] - h->one_sb[k];
                    VBA_LAUNCH(k_chol_step4<true>, dim3(L.step_grid[k], 1), dim3(128), 0, stream, B, k, so);
                } else VBA_LAUNCH(k_chol_step4<false>, dim3(L.step_grid[k], n), dim3(128), 0, stream, B, k, StepOne());
            }
        }
    }
    {
        ProfScope ps(h, stream, VBA_PROF_TRSV);
        if (P.trsv == vba_host::CAP_TRSV) {
            CAP_PATH(h, 2, vba_host::CAP_TRSV);
            const size_t shm = ((size_t)L.max_nS + 256 + 32 * 33) * sizeof(double);
            VBA_LAUNCH(k_trsv, dim3(n), dim3(256), shm, stream, B);
        } else {
            CAP_PATH(h, 2, vba_host::CAP_TRSV_P);
            const size_t shm = ((size_t)L.max_nS + 2 * TRSV_P_DW * 32 + 2 * 32 * 65 + 32) * sizeof(double) + ((size_t)L.max_pan + L.max_nb + 2) * sizeof(int);
            VBA_LAUNCH(k_trsv_p, dim3(n), dim3(512), shm, stream, B);
        }
    }
    CAP_COPY(h, stream, CAP_LF_C, CAP_VEC_C + 1);
    }
    {
        ProfScope ps(h, stream, VBA_PROF_UPDATE);
        if (idp) VBA_LAUNCH(k_update, dim3(L.max_pt_blk + L.max_kf_blk, n), dim3(64), 0, stream, B, L.max_pt_blk);
        else VBA_LAUNCH(k_update_xyz, dim3(L.max_pt_blk + L.max_kf_blk, n), dim3(64), 0, stream, B, L.max_pt_blk);
    }
    CAP_COPY(h, stream, CAP_POSE_D, CAP_N);
#ifdef VBA_TEST_HOOKS
    if (h->cap_call >= 0 && h->cap_count++ == h->cap_call) h->cap_done = 1;
#endif
}

void enqueue_lin(Handle* h, const Group& g, int mode) {
    const LaunchGeom& L = h->geom;
    const int imu_lin = L.max_imu > 0 ? h->rp.imu_lin : -1;
    ProfScope ps(h, g.stream, VBA_PROF_LINEARIZE);
    if (mode == LIN_REDO) ps.e.counts = 0;   // the second half of the pass LIN_AUTO opened
    if (h->variant == VBA_VARIANT_PRV_IDP) {
        const size_t shm = LIN2_LDS;
        if (imu_lin == vba_host::LIN_IMU_FUSED) {   // edges and IMU factors in one launch
            VBA_LAUNCH(k_lin2_imu, dim3(L.max_lin_blk + L.max_imu, g.n_win), dim3(256), shm, g.stream, g.B, L.max_lin_blk, mode);
            return;
        }
        VBA_LAUNCH(k_lin2, dim3(L.max_lin_blk, g.n_win), dim3(256), shm, g.stream, g.B, L.max_lin_blk, mode);
    } else {
        VBA_LAUNCH(k_lin_xyz_e, dim3(L.max_lin_blk, g.n_win), dim3(256), 0, g.stream, g.B, mode);
        if (L.any_lin_fallback) VBA_LAUNCH(k_lin_xyz, dim3(L.max_pt_blk, g.n_win), dim3(64), 0, g.stream, g.B, L.max_pt_blk, mode);
    }
    if (imu_lin == vba_host::LIN_IMU_PAIR) {
        VBA_LAUNCH(k_lin_imu_pair, dim3(L.max_imu, g.n_win), dim3(64), 0, g.stream, g.B, mode);
    } else if (imu_lin == vba_host::LIN_IMU_RES_HESS) {   // a lane per keyframe pair for the Lie-group part, then a wave per pair for J^T Omega J
        VBA_LAUNCH(k_lin_imu_res, dim3((L.max_imu + 63) / 64, g.n_win), dim3(64), 0, g.stream, g.B, mode);
        if (mode != LIN_ERR && mode != LIN_ERR_TRIAL) VBA_LAUNCH(k_lin_imu_hess, dim3(L.max_imu, g.n_win), dim3(64), 0, g.stream, g.B, mode);
    }
}

// ---- what the Gauss-Newton and the Levenberg-Marquardt schedule share: the launches that open and close a run and a stage
void sched_reset(Handle* h, const Group& g) {
    const LaunchGeom& L = h->geom;
    const int big_blk = std::max(std::max(L.max_kf_blk, L.max_pt_blk), L.max_obs_blk);
    ProfScope ps(h, g.stream, VBA_PROF_MISC);
    VBA_LAUNCH(k_reset, dim3(std::max(1, std::min(32, big_blk / 4)), g.n_win), dim3(256), 0, g.stream, g.B);
}
void sched_stage_begin(Handle* h, const Group& g, int stage) {
    const LaunchGeom& L = h->geom;
    ProfScope ps(h, g.stream, VBA_PROF_MISC);
    if (h->rp.poll) VBA_LAUNCH(k_poll_stop, dim3(1), dim3(1), 0, g.stream, g.B);
    VBA_LAUNCH(k_stage_clear, dim3(L.max_ns_blk, g.n_win), dim3(64), 0, g.stream, g.B, stage);
    if (stage == 1) VBA_LAUNCH(k_classify, dim3(L.max_obs_blk, g.n_win), dim3(64), 0, g.stream, g.B);
    VBA_LAUNCH(k_stage_mark, dim3(L.max_free + (L.max_imu + 63) / 64, g.n_win), dim3(64), 0, g.stream, g.B, L.max_free);
}
void sched_stage_end(Handle* h, const Group& g) {
    if (h->variant == VBA_VARIANT_PRV_IDP) return;
    ProfScope ps(h, g.stream, VBA_PROF_MISC);
    VBA_LAUNCH(k_depth_xyz, dim3(std::max(h->geom.max_obs_blk, 1), g.n_win), dim3(64), 0, g.stream, g.B);
}
void sched_finish(Handle* h, const Group& g) {
    const LaunchGeom& L = h->geom;
    ProfScope ps(h, g.stream, VBA_PROF_MISC);
    if (h->variant != VBA_VARIANT_PRV_IDP)
        VBA_LAUNCH(k_chi2_fresh_xyz, dim3(std::max(L.max_obs_blk, 1), g.n_win), dim3(64), 0, g.stream, g.B);
    VBA_LAUNCH(k_final_edges, dim3(std::max(L.max_obs_blk, 1), g.n_win), dim3(64), 0, g.stream, g.B);
    VBA_LAUNCH(k_final_sum, dim3(g.n_win), dim3(64), 0, g.stream, g.B);
}

// Levenberg-Marquardt schedule (levenberg.cpp:61-164) of a batch cut into window groups, device-resident.
// The launch stream of a group is a sequence of SLOT GROUPS [outer, trial]:
//   outer = linearise + computeLambdaInit + the bookkeeping that opens an outer iteration   -- for windows that owe no trial
//   trial = damp, Schur, factor, solve, update, re-evaluate, accept / reject (+ restore)    -- for windows that owe one
// Every kernel is gated per window on WinCtrl (active, lm_need_trial), so each window consumes the slots that apply to it:
// the usual outer iteration takes one [outer, trial]; a window whose step is rejected skips the next group's outer slot (its
// workgroups exit at once) and retries in that group's trial slot -- windows drift apart by whole slots, never inside one, and a
// window that needs no retry never pays for one (a speculative second trial slot per group cost 6 % at C2: ~20 launches whose
// 300 k workgroups only exit).  The host learns through one
// pinned word per slot group whether any window of the group of windows is still going, and stays two slot groups ahead of
// the device (as the Gauss-Newton schedule does): no host round trip per trial, none per outer iteration on the critical path.
int enqueue_schedule_lm(Handle* h, std::vector<Group>& groups, StopRef stop_flag) {
    const LaunchGeom& L = h->geom;
    const int kp_blk = std::max(L.max_kf_blk, L.max_pt_blk);
    auto outer = [&](Group& g) {   // linearise + computeLambdaInit of one outer iteration
        enqueue_lin(h, g, LIN_FULL);
        {   // H_pp diagonal for computeLambdaInit (the block it writes into S is rewritten by the first trial): a Schur diagonal pass
            ProfScope ps(h, g.stream, VBA_PROF_SCHUR);
            VBA_LAUNCH(k_schur_diag3, dim3(L.max_free * xcd_windows(g.n_win)), dim3(64), 0, g.stream, g.B, L.max_free, 1);
        }
        ProfScope ps(h, g.stream, VBA_PROF_CONTROL);
        if (h->rp.poll) VBA_LAUNCH(k_poll_stop, dim3(1), dim3(1), 0, g.stream, g.B);
        VBA_LAUNCH(k_ctrl_lm_outer, dim3(g.n_win), dim3(64), 0, g.stream, g.B);
    };
    auto trial = [&](Group& g, int* alive_dev, int* alive_mirror) {
        {
            ProfScope ps(h, g.stream, VBA_PROF_MISC);
            VBA_LAUNCH(k_backup, dim3(kp_blk, g.n_win), dim3(64), 0, g.stream, g.B);
        }
        enqueue_solve_iteration(h, g, stop_flag);
        enqueue_lin(h, g, LIN_ERR_TRIAL);
        {
            ProfScope ps(h, g.stream, VBA_PROF_CONTROL);
            if (h->rp.poll) VBA_LAUNCH(k_poll_stop, dim3(1), dim3(1), 0, g.stream, g.B);
            VBA_LAUNCH(k_ctrl_lm_trial, dim3(g.n_win), dim3(64), 0, g.stream, g.B, alive_dev, alive_mirror);
        }
        {
            ProfScope ps(h, g.stream, VBA_PROF_MISC);   // pop of a rejected step (with k_backup, the push)
            VBA_LAUNCH(k_restore, dim3(kp_blk, g.n_win), dim3(64), 0, g.stream, g.B);
        }
    };
    for (auto& g : groups) sched_reset(h, g);
    const int RING = 32;   // pinned alive words per window group (its 64-word block: [0, RING) used here)
    int rc = 0;
    for (int stage = 0; stage < 2 && rc == 0; stage++) {
        for (auto& g : groups) sched_stage_begin(h, g, stage);
        if (L.max_its[stage] > 0) {
            // upper bound of the slot groups a stage can need: every outer iteration may take up to 10 trials
            const int max_groups = std::min(478, 10 * L.max_its[stage] + 2);
            std::vector<std::vector<hipEvent_t>> ev(groups.size());
            for (auto& g : groups) g.dead = false;
            for (int j = 0; j < max_groups; j++) {
                bool any = false;
                for (size_t gi = 0; gi < groups.size(); gi++) {
                    Group& g = groups[gi];
                    if (g.dead) continue;
                    if (j >= 2) {
                        if (wait_event_forwarding(h, ev[gi][j - 2], stop_flag) != hipSuccess) { rc = -1; break; }
                        if (g.alive[(j - 2) % RING] == 0) { g.dead = true; continue; }   // nobody went on after slot group j-2
                    }
                    any = true;
                    forward_stop(h, stop_flag);
                    g.alive[j % RING] = 0;   // the word's previous user (group j - RING) was consumed long ago
                    int* alive_dev = h->stop_dev + (g.alive - h->stop_host) + (j % RING);
                    outer(g);
                    trial(g, alive_dev, g.B.alive_dev + 64 + stage * 480 + j);   // a mirror word of its own per slot group (never reused inside a run)
                    ev[gi].push_back(get_evt(h));
                    if (hipEventRecord(ev[gi][j], g.stream) != hipSuccess) { rc = -1; break; }
                }
                if (!any || rc) break;
            }
        }
        for (auto& g : groups) sched_stage_end(h, g);
    }
    for (auto& g : groups) {
        if (rc) break;
        sched_finish(h, g);
    }
    return rc;
}

// The two-stage schedule of a batch cut into window groups.  The groups are independent; their launches are enqueued
// INTERLEAVED, iteration by iteration, each on its own stream, so that while one group sits in the latency-bound block
// columns of its factorisation another one streams through its bandwidth-bound linearise / Schur kernels.
int enqueue_schedule(Handle* h, std::vector<Group>& groups, StopRef stop_flag) {
    if (h->algo == VBA_ALGO_LM) return enqueue_schedule_lm(h, groups, stop_flag);
    const LaunchGeom& L = h->geom;
    for (auto& g : groups) sched_reset(h, g);
    for (int stage = 0; stage < 2; stage++) {
        for (auto& g : groups) sched_stage_begin(h, g, stage);
        {
            // The host stays at most two iterations ahead of the device: before enqueuing iteration it of a group it waits
            // for that group's control kernel of iteration it-2 and stops enqueuing for the group once none of its windows is
            // iterating any more (the |dchi2| < 1e-3 stop usually ends stage 2 after 3 of its 10 iterations).  The device
            // never starves: one full iteration is always queued behind the one being waited for.
            const int nit = L.max_its[stage];
            std::vector<std::vector<hipEvent_t>> ev(groups.size(), std::vector<hipEvent_t>(nit, nullptr));
            const bool word_report = h->rp.word_report && nit <= 32;   // see k_ctrl_gn
            const bool pace = nit <= 32;  // also when profiling: the launch counts (and hence the per-launch averages) then equal those of a normal run
            const int depth = h->rp.pace_depth;   // how far ahead
            const bool probe = h->rp.lin_probe != 0;
            for (auto& g : groups) g.dead = false;
            for (int it = 0; it < nit; it++) {
                bool any = false;
                for (size_t gi = 0; gi < groups.size(); gi++) {
                    Group& g = groups[gi];
                    if (g.dead) continue;
                    if (pace && it >= depth) {
                        const int slot = stage * 32 + it - depth;
                        if (word_report) {   // the control kernel writes 1 (stopped) / 2 (goes on) into the pinned word when it is done
                            long spins = 0;
                            while (g.alive[slot] == 0) {
                                forward_stop(h, stop_flag);
                                if ((++spins & 1023) == 0 && hipStreamQuery(g.stream) != hipErrorNotReady) break;   // drained or failed: nothing will write it
                                std::this_thread::yield();
                            }
                            if (g.alive[slot] != 2) { g.dead = true; continue; }
                        } else {
                            (void)wait_event_forwarding(h, ev[gi][it - depth], stop_flag);
                            if (g.alive[slot] == 0) { g.dead = true; continue; }
                        }
                    }
                    any = true;
                    forward_stop(h, stop_flag);   // InterruptBA raised while the host paces itself: the device sees it at its next poll
                    // probing (plan_lin_probe): windows whose last chi2 decrease predicts a stop evaluate chi2 only, and the ones
                    // that go on all the same get their full pass behind the control launch.  k_ctrl_gn sets no probe before its
                    // call of iteration 1, so the first pass that can be one -- and the first redo -- is that of iteration 2.
                    enqueue_lin(h, g, probe ? LIN_AUTO : LIN_FULL);
                    {
                        ProfScope ps(h, g.stream, VBA_PROF_CONTROL);
                        if (h->rp.poll) VBA_LAUNCH(k_poll_stop, dim3(1), dim3(1), 0, g.stream, g.B);
                        VBA_LAUNCH(k_ctrl_gn, dim3(g.n_win), dim3(64), 0, g.stream, g.B, 0, word_report ? stage * 32 + it : -1);
                    }
                    if (pace && !word_report) {
                        ev[gi][it] = get_evt(h);
                        (void)hipEventRecord(ev[gi][it], g.stream);
                    }
                    if (probe && it >= 2) enqueue_lin(h, g, LIN_REDO);
                    enqueue_solve_iteration(h, g, stop_flag);
                }
                if (!any) break;
            }
            for (auto& g : groups) {
                enqueue_lin(h, g, LIN_ERR);
                ProfScope ps(h, g.stream, VBA_PROF_CONTROL);
                VBA_LAUNCH(k_ctrl_gn, dim3(g.n_win), dim3(64), 0, g.stream, g.B, 1, -1);
            }
        }
        for (auto& g : groups) sched_stage_end(h, g);
    }
    for (auto& g : groups) sched_finish(h, g);
    return 0;
}

int do_run(Handle* h, StopRef stop_flag) {
    const bool timing = vba_host::process_knobs().timing;
    const double t_run0 = timing ? now_ms() : 0.0;
    if (!h->uploaded) return fail(h, "vba_batch_run before vba_batch_upload");
    HIPCHK(h, hipSetDevice(h->device));
    const int n = h->n_win;
    // (the hooks may have changed since the upload, and between runs of one upload)
    h->rp = vba_host::plan_run(h->up, n, h->variant, h->algo, h->ov, vba_host::process_knobs(), h->profile, h->is_lane,
                               (int)h->xstreams.size() + (h->owns_streams ? 11 : 1));
    h->B.dbg_stop_after = h->rp.dbg_stop_after;
    h->B.pcg_tri = h->rp.pcg_tri;
    h->B.lin_probe = h->rp.lin_probe;
    const Batch B = h->B;
    *h->stop_host = stop_flag.set() ? 1 : 0;
    for (int i = 64; i < 1024; i++) h->stop_host[i] = 0;
    const long long launch0 = h->n_launch;
    h->evts.clear();
    h->evt_used = 0;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    if (h->profile) {
        ev_begin = get_evt(h);
        ev_end = get_evt(h);
        (void)hipEventRecord(ev_begin, h->stream);
    }
    const int ngroups = h->rp.ngroups;   // window groups, each with its own stream (enqueue_schedule)
    while ((int)h->xstreams.size() < ngroups - 1) {
        hipStream_t st;
        HIPCHK(h, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        h->xstreams.push_back(st);
    }
#ifdef VBA_TEST_HOOKS
    h->cap_count = 0;
    h->cap_done = 0;
    for (int i = 0; i < 4; i++) h->cap_path[i] = -1;
    for (int q = 0; q < CAP_N; q++) h->cap_bytes[q] = 0;
    if (h->cap_call >= 0) {
        if (ngroups > 1) { h->cap_call = -1; return fail(h, "vba_debug_capture: the batch runs as more than one window group (vba_debug_set_streams(h, 1))"); }
        for (int q = 0; q < CAP_N; q++) {
            int id;
            size_t bytes;
            cap_source(h, q, id, bytes);
            HIPCHK(h, h->cap[q].ensure(bytes));
        }
    }
#endif
    std::vector<Group> groups(ngroups);
    std::vector<hipEvent_t> done(ngroups);
    const std::vector<int> gb = vba_host::group_bounds(n, ngroups);
    for (int g = 0; g < ngroups; g++) {
        const int w0 = gb[g], w1 = gb[g + 1];
        groups[g].B = B;
        groups[g].B.desc = B.desc + w0;
        groups[g].B.ctrl = B.ctrl + w0;
        groups[g].B.n_win = w1 - w0;
        groups[g].B.alive_cnt = h->stop_dev + 64 + 64 * g;
        groups[g].B.alive_dev = dp<int>(h, BUF_ALIVE) + 1024 * g;
        groups[g].B.stop_word = stop_word_of(h, groups[g].B);
        groups[g].n_win = w1 - w0;
        groups[g].index = g;
        groups[g].stream = (g == 0) ? h->stream : h->xstreams[g - 1];
        groups[g].alive = h->stop_host + 64 + 64 * g;
        groups[g].dead = false;
    }
    if (h->up_pending) {   // (vba_solve: the upload was not waited for on the host)
        HIPCHK(h, hipStreamWaitEvent(h->stream, h->up_done, 0));
        h->up_pending = false;
    }
    HIPCHK(h, hipMemsetAsync(h->buf[BUF_ALIVE].p, 0, 14 * 1024 * sizeof(int), h->stream));   // the mirror words of this run
    // the other streams start after everything already queued on the main stream (upload, previous run)
    if (ngroups > 1) {
        hipEvent_t e0 = get_evt(h);
        HIPCHK(h, hipEventRecord(e0, h->stream));
        for (int g = 1; g < ngroups; g++) HIPCHK(h, hipStreamWaitEvent(groups[g].stream, e0, 0));
    }
    int rc = enqueue_schedule(h, groups, stop_flag);
    for (int g = 0; g < ngroups && rc == 0; g++) {
        done[g] = get_evt(h);
        if (hipEventRecord(done[g], groups[g].stream) != hipSuccess) rc = -1;
    }
    if (rc) return fail(h, h->err.empty() ? "enqueue failed" : h->err);
    if (h->profile) (void)hipEventRecord(ev_end, h->stream);
    HIPCHK(h, hipGetLastError());
    // behind the last kernel, on the main stream: the control blocks and -- for a few windows, where every synchronous copy of the
    // download is a 20-us round trip on a 3-ms solve -- the result arrays, into pinned staging (do_download only scatters them)
    for (int g = 1; g < ngroups; g++) HIPCHK(h, hipStreamWaitEvent(h->stream, done[g], 0));
    h->hctrl.resize(n);
    if (!h->hctrl.ok) return fail(h, "out of pinned host memory (control blocks)");
    h->dl_prefetched = false;
    if (h->res_bytes) {   // few windows: ONE copy brings the control blocks and every result array (do_upload laid them out in one block)
        HIPCHK(h, hipMemcpyAsync(h->res_host.p, h->buf[BUF_RESULTS].p, h->res_bytes, hipMemcpyDeviceToHost, h->stream));
        h->dl_prefetched = true;
    } else
        HIPCHK(h, hipMemcpyAsync(h->hctrl.data(), B.ctrl, sizeof(WinCtrl) * n, hipMemcpyDeviceToHost, h->stream));
    hipEvent_t ev_all = get_evt(h);
    HIPCHK(h, hipEventRecord(ev_all, h->stream));
    // wait, forwarding the caller's stop flag (g2o forceStopFlag) into the device-visible word
    if (stop_flag) {
        while (hipEventQuery(ev_all) == hipErrorNotReady) {
            if (stop_flag.set()) *h->stop_host = 1;
            std::this_thread::yield();
        }
    }
    HIPCHK(h, hipEventSynchronize(ev_all));
    if (h->dl_prefetched) memcpy(h->hctrl.data(), h->res_host.p, sizeof(WinCtrl) * n);
    h->prof.kernel_launches = h->n_launch - launch0;
    if (h->profile) {
        vba_profile& pf = h->prof;
        memset(&pf, 0, sizeof pf);
        pf.kernel_launches = h->n_launch - launch0;
        for (auto& e : h->evts) {
            float ms = 0;
            (void)hipEventElapsedTime(&ms, e.a, e.b);
            pf.ms[e.cls] += ms;
            pf.launches[e.cls] += e.counts;
        }
        float tot = 0;
        (void)hipEventElapsedTime(&tot, ev_begin, ev_end);
        pf.total_ms = tot;
        // algorithmic bytes: 32 B observation record + 36 B landmark per linearisation pass;
        // reduced system written once and read once per solve
        for (int w = 0; w < n; w++) {
            const WinDesc& d = h->desc[w];
            const WinCtrl& c = h->hctrl[w];
            double passes = 0, solves = 0;
            for (int s = 0; s < 2; s++)
                if (c.its_done[s] > 0) { passes += c.its_done[s] + 1; solves += c.its_done[s]; }
            pf.bytes[VBA_PROF_LINEARIZE] += passes * (32.0 * d.n_obs + 36.0 * d.n_pt + 432.0 * d.n_free);
            // reduced system ("write n_p^2 8 B + read once by solver"): the Schur class writes S once, the factorisation
            // reads S and writes L once, the two triangular solves read L once each (half the square each)
            pf.bytes[VBA_PROF_SCHUR] += solves * ((double)d.np * d.np * 8.0);
            pf.bytes[VBA_PROF_FACTOR] += solves * ((double)d.np * d.np * 8.0 * 2.0);
            pf.bytes[VBA_PROF_TRSV] += solves * ((double)d.np * d.np * 8.0);
            pf.bytes[VBA_PROF_UPDATE] += solves * (36.0 * d.n_pt + 432.0 * d.n_free);   // per point 28 B read + 8 B write, per free KF 432 B
            pf.factor_flops += solves * h->win_tiles[w] * (2.0 * VBA_NB * VBA_NB * VBA_NB);
        }
    }
    h->ran = true;
#ifdef VBA_TEST_HOOKS
    h->cap_call = -1;   // one capture per request
#endif
    if (timing) fprintf(stderr, "[vba] %p t=%.1f run %d windows: %.3f ms\n", (void*)h, now_ms(), n, now_ms() - t_run0);
    return 0;
}

int do_download(Handle* h, int n, vba_problem* const* inout, vba_result* const* out) {
    const bool timing = vba_host::process_knobs().timing;
    const double t_dl0 = timing ? now_ms() : 0.0;
    if (!h->ran) return fail(h, "vba_batch_download before vba_batch_run");
    if (n != h->n_win) return fail(h, "window count mismatch");
    HIPCHK(h, hipSetDevice(h->device));
    const Batch& B = h->B;
    // Many windows: every result array crosses PCIe ONCE into host staging and host threads scatter it to the callers'
    // arrays (per-window copies cost ~12 synchronous hipMemcpy calls per window, 0.25 ms).  Few windows: the run has left them in the staging already (do_run).
    const bool staged = !h->up.results_block || h->dl_prefetched;
    if (staged && !h->dl_prefetched) {
        bool want_state = false, want_outl = false, want_chi2 = false;
        for (int w = 0; w < n; w++) {
            if (inout && inout[w] && h->hctrl[w].status != VBA_ABORTED_BEFORE) want_state = true;
            if (out && out[w] && out[w]->obs_outlier) want_outl = true;
            if (out && out[w] && out[w]->obs_chi2) want_chi2 = true;
        }
        const WinDesc& dl = h->desc[n - 1];
        const size_t nkf = (size_t)dl.kf0 + dl.n_kf, npt = (size_t)dl.pt0 + dl.n_pt, nobs = (size_t)dl.obs0 + dl.n_obs;
        const bool vi = h->variant != VBA_VARIANT_SE3_XYZ;
        Staging& G = h->stg;
        if (want_state) { G.dl_pose.resize(7 * nkf); G.dl_pt.resize(3 * npt); }
        if (want_state && vi) { G.dl_vel.resize(3 * nkf); G.dl_bias.resize(12 * nkf); }
        if (want_outl) G.dl_outl.resize(nobs);
        if (want_chi2) G.dl_chi2.resize(nobs);
        if (!G.ok()) return fail(h, "out of pinned host memory (download staging)");
        if (want_state) {
            HIPCHK(h, hipMemcpyAsync(G.dl_pose.data(), B.pose, 56 * nkf, hipMemcpyDeviceToHost, h->dl_stream));
            HIPCHK(h, hipMemcpyAsync(G.dl_pt.data(), B.pt, 24 * npt, hipMemcpyDeviceToHost, h->dl_stream));
            if (vi) {
                HIPCHK(h, hipMemcpyAsync(G.dl_vel.data(), B.vel, 24 * nkf, hipMemcpyDeviceToHost, h->dl_stream));
                HIPCHK(h, hipMemcpyAsync(G.dl_bias.data(), B.bias, 96 * nkf, hipMemcpyDeviceToHost, h->dl_stream));
            }
        }
        if (want_outl) HIPCHK(h, hipMemcpyAsync(G.dl_outl.data(), B.out_outlier, nobs, hipMemcpyDeviceToHost, h->dl_stream));
        if (want_chi2) HIPCHK(h, hipMemcpyAsync(G.dl_chi2.data(), B.out_chi2, 8 * nobs, hipMemcpyDeviceToHost, h->dl_stream));
        HIPCHK(h, hipStreamSynchronize(h->dl_stream));
    }
    // where the staged arrays are: the per-array staging of a big batch, or the one block a small one came back in
    const char* rb = reinterpret_cast<const char*>(h->res_host.p);
    const bool one = h->dl_prefetched;
    const double* s_pose = one ? reinterpret_cast<const double*>(rb + h->res_off[1]) : h->stg.dl_pose.data();
    const double* s_vel = one ? reinterpret_cast<const double*>(rb + h->res_off[2]) : h->stg.dl_vel.data();
    const double* s_bias = one ? reinterpret_cast<const double*>(rb + h->res_off[3]) : h->stg.dl_bias.data();
    const double* s_pt = one ? reinterpret_cast<const double*>(rb + h->res_off[4]) : h->stg.dl_pt.data();
    const unsigned char* s_outl = one ? reinterpret_cast<const unsigned char*>(rb + h->res_off[5]) : h->stg.dl_outl.data();
    const double* s_chi2 = one ? reinterpret_cast<const double*>(rb + h->res_off[6]) : h->stg.dl_chi2.data();
    std::atomic<int> bad(0);
    host_parallel_for(h, n, staged ? std::max(1, std::min(host_threads(), n / 8)) : 1, [&](int w) {
        const WinDesc& d = h->desc[w];
        const WinCtrl& c = h->hctrl[w];
        vba_problem* P = inout ? inout[w] : nullptr;
        vba_result* R = out ? out[w] : nullptr;
        auto get = [&](void* dst, const void* dev, const void* host, size_t bytes) {
            if (!bytes) return;
            if (staged) memcpy(dst, host, bytes);
            else if (hipMemcpy(dst, dev, bytes, hipMemcpyDeviceToHost) != hipSuccess) bad.store(1);
        };
        if (P && c.status != VBA_ABORTED_BEFORE) {
            get(P->kf_pose, B.pose + 7 * (size_t)d.kf0, s_pose + 7 * (size_t)d.kf0, 56 * (size_t)d.n_free);
            if (d.pdim == 15) {
                if (P->kf_vel) get(P->kf_vel, B.vel + 3 * (size_t)d.kf0, s_vel + 3 * (size_t)d.kf0, 24 * (size_t)d.n_free);
                if (P->kf_bias) get(P->kf_bias, B.bias + 12 * (size_t)d.kf0, s_bias + 12 * (size_t)d.kf0, 96 * (size_t)d.n_free);
            }
            get(P->pt, B.pt + 3 * (size_t)d.pt0, s_pt + 3 * (size_t)d.pt0, 24 * (size_t)d.n_pt);
        }
        if (R) {
            R->chi2_vis = c.chi2_vis; R->chi2_prv = c.chi2_prv; R->chi2_bias = c.chi2_bias;
            R->its_done[0] = c.its_done[0]; R->its_done[1] = c.its_done[1];
            R->n_outliers = c.n_outliers; R->status = c.status;
            R->n_trace = c.n_trace;
            for (int i = 0; i < c.n_trace && i < VBA_TRACE_MAX; i++) R->chi2_trace[i] = c.trace[i];
            R->lambda_final = c.lambda;
            R->lin_iterations = c.lin_its;
            if (c.status != VBA_ABORTED_BEFORE && d.n_obs) {
                if (R->obs_outlier) get(R->obs_outlier, B.out_outlier + d.obs0, s_outl + d.obs0, (size_t)d.n_obs);
                if (R->obs_chi2) get(R->obs_chi2, B.out_chi2 + d.obs0, s_chi2 + d.obs0, 8 * (size_t)d.n_obs);
            }
        }
    });
    if (bad.load()) return fail(h, "hipMemcpy (download) failed");
    if (timing) fprintf(stderr, "[vba] %p t=%.1f download %d windows: %.3f ms\n", (void*)h, now_ms(), n, now_ms() - t_dl0);
    return 0;
}

}  // namespace
