// vislam_ba.hip -- C-ABI (include/vislam_ba.h) of the MI355X local-BA backend, one translation unit: the kernel headers, the host
// side by topic (vba_host_structure.h / vba_host_posegraph.h: the plain-C++ structure builds, vba_host_handle.h: handle and buffers, vba_host_upload.h: H2D + structure build, vba_host_run.h: the lock-step
// launch schedule of the two-stage solve and the download, vba_host_batch.h: lanes and tickets, vba_host_hooks.h), and below the
// extern "C" entry points.
//
// Host-side control flow restated from src/Optimizer.cpp:453-517 (two-stage protocol) and
// Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:354-419 (optimize loop); all per-iteration decisions are taken
// on the device (k_ctrl_*), the host only enqueues.  No CPU fallback exists: without a HIP device every entry
// point fails with an error.
#include "../../include/vislam_ba.h"
#include "vba_host_structure.h"
#include "vba_host_posegraph.h"
#include "vba_problem_io.h"
#include "vba_kernels_lm.h"
#include "vba_preint.h"
#include "vba_pose.h"
#include "vba_sim3.h"
#include "vba_posegraph.h"
#include "vba_structure.h"
#include "vba_pcg.h"
#include "vba_chain.h"

#include "vba_host_handle.h"
#include "vba_host_upload.h"
#include "vba_host_run.h"
#include "vba_host_batch.h"
#include "vba_host_hooks.h"

extern "C" {

int vba_create(int device, void** handle) {
    if (!handle) return -1;
    *handle = nullptr;
    Handle* h = nullptr;
    const int rc = make_handle(device, nullptr, &h);
    if (rc == 0) *handle = h;
    return rc;
}

int vba_destroy(void* handle) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    if (h->as) async_shutdown(h);
    for (Handle* l : h->lanes) (void)vba_destroy(l);
    h->lanes.clear();
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    (void)hipStreamSynchronize(h->up_stream);
    (void)hipStreamSynchronize(h->dl_stream);
    h->stg.release();
    h->hctrl.release();
    h->res_host.release();
    h->up_arena.release();
    h->up_arena_host.release();
    for (auto& b : h->buf) b.release();
#ifdef VBA_TEST_HOOKS
    for (auto& b : h->cap) b.release();
#endif
    h->preint.release();
    h->pose_arena.release();
    h->pose_host_in.release();
    h->pose_host_out.release();
    h->sim3_arena.release();
    h->sim3_host_in.release();
    h->sim3_host_out.release();
    h->pg_arena.release();
    h->pg_host_in.release();
    h->pg_host_out.release();
    for (auto e : h->evt_pool) (void)hipEventDestroy(e);
    if (h->up_done) (void)hipEventDestroy(h->up_done);
    if (h->owns_streams)
        for (auto st : h->xstreams) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (h->stop_host) (void)hipHostFree((void*)h->stop_host);
    if (h->owns_streams) (void)hipStreamDestroy(h->stream);
    delete h;
    return 0;
}

const char* vba_last_error(void* handle) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    return h ? h->err.c_str() : "null handle";
}

int vba_batch_upload(void* handle, int32_t n, vba_problem* const* problems) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    return do_upload(h, n, problems);
}
int vba_batch_run(void* handle, const volatile int* stop_flag) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    return do_run(h, stop_int(stop_flag));
}
int vba_batch_run_b(void* handle, const volatile unsigned char* stop_flag) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    return do_run(h, stop_byte(stop_flag));
}
int vba_batch_download(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    return do_download(h, n, inout, out);
}
int vba_solve(void* handle, vba_problem* inout, vba_result* out, const volatile int* stop_flag) { return solve_one(handle, inout, out, stop_int(stop_flag)); }
int vba_solve_b(void* handle, vba_problem* inout, vba_result* out, const volatile unsigned char* stop_flag) { return solve_one(handle, inout, out, stop_byte(stop_flag)); }
int vba_batch_solve(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out, const volatile int* stop_flag) {
    return batch_solve(handle, n, inout, out, stop_int(stop_flag));
}
int vba_batch_solve_b(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out, const volatile unsigned char* stop_flag) {
    return batch_solve(handle, n, inout, out, stop_byte(stop_flag));
}

int vba_batch_set_depth(void* handle, int32_t depth) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    if (depth < 1 || depth > 4) return fail(h, "vba_batch_set_depth: depth must be 1..4");
    if (h->as) {   // idle: the workers leave, arenas beyond the new depth free their device buffers and staging
        AsyncState& A = *h->as;
        async_stop_workers(A);
        while ((int)A.arenas.size() > depth) {
            (void)vba_destroy(A.arenas.back());
            A.arenas.pop_back();
        }
    }
    h->async_depth = depth;
    return 0;
}
int vba_batch_submit(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out, const volatile int* stop_flag,
                     int64_t* ticket) {
    return submit(reinterpret_cast<Handle*>(handle), n, inout, out, stop_int(stop_flag), ticket);
}
int vba_batch_submit_b(void* handle, int32_t n, vba_problem* const* inout, vba_result* const* out,
                       const volatile unsigned char* stop_flag, int64_t* ticket) {
    return submit(reinterpret_cast<Handle*>(handle), n, inout, out, stop_byte(stop_flag), ticket);
}
int vba_batch_poll(void* handle, int64_t ticket) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    if (!h->as || !h->as->tickets.count(ticket)) return fail(h, "vba_batch_poll: unknown or retired ticket " + std::to_string(ticket));
    AsyncState& A = *h->as;
    std::lock_guard<std::mutex> lk(A.mu);
    return A.tickets[ticket]->done ? 0 : 1;
}
int vba_batch_wait(void* handle, int64_t ticket) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h) return -1;
    if (!h->as || !h->as->tickets.count(ticket)) return fail(h, "vba_batch_wait: unknown or retired ticket " + std::to_string(ticket));
    AsyncState& A = *h->as;
    std::shared_ptr<AsyncTicket> t = A.tickets[ticket];
    {
        std::unique_lock<std::mutex> lk(A.mu);
        A.cv.wait(lk, [&] { return t->done; });
    }
    A.tickets.erase(ticket);
    if (t->rc)
        return fail(h, "vba_batch_submit, ticket " + std::to_string(ticket) + ", windows 0.." + std::to_string(t->inout.size() - 1) + ": " + t->err);
    return 0;
}

// the size of the host thread pool of a handle in this process (this rank's share of the cores: host_threads above)
int vba_host_threads(void) { return host_threads(); }

int vba_preintegrate(void* handle, int32_t n_edges, const int32_t* sample_begin, const double* gyr, const double* acc,
                     const double* dt, double gyr_meas_cov, double acc_meas_cov, double* imu_meas, double* cov_pvphi,
                     double* imu_info_prv) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    if (n_edges <= 0 || !sample_begin || !gyr || !acc || !dt || !imu_meas || !cov_pvphi) return fail(h, "vba_preintegrate: bad arguments");
    HIPCHK(h, hipSetDevice(h->device));
    const int ns = sample_begin[n_edges];
    for (int e = 0; e < n_edges; e++)
        if (sample_begin[e] > sample_begin[e + 1] || sample_begin[e] < 0) return fail(h, "vba_preintegrate: sample_begin is not a CSR");
    // a small private arena: inputs | outputs
    const size_t b_sb = ((size_t)(n_edges + 1) * 4 + 255) / 256 * 256, b_v = ((size_t)ns * 24 + 255) / 256 * 256, b_d = ((size_t)ns * 8 + 255) / 256 * 256;
    const size_t b_m = (size_t)n_edges * 61 * 8, b_c = (size_t)n_edges * 81 * 8;
    const size_t total = b_sb + 2 * b_v + b_d + b_m + 2 * b_c + 1024;
    HIPCHK(h, h->preint.ensure(total));
    char* base = reinterpret_cast<char*>(h->preint.p);
    int* d_sb = reinterpret_cast<int*>(base);
    double* d_g = reinterpret_cast<double*>(base + b_sb);
    double* d_a = reinterpret_cast<double*>(base + b_sb + b_v);
    double* d_dt = reinterpret_cast<double*>(base + b_sb + 2 * b_v);
    double* d_m = reinterpret_cast<double*>(base + b_sb + 2 * b_v + b_d);
    double* d_c = d_m + (size_t)n_edges * 61;
    double* d_i = d_c + (size_t)n_edges * 81;
    HIPCHK(h, hipMemcpyAsync(d_sb, sample_begin, (size_t)(n_edges + 1) * 4, hipMemcpyHostToDevice, h->stream));
    if (ns > 0) {
        HIPCHK(h, hipMemcpyAsync(d_g, gyr, (size_t)ns * 24, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_a, acc, (size_t)ns * 24, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_dt, dt, (size_t)ns * 8, hipMemcpyHostToDevice, h->stream));
    }
    VBA_LAUNCH(k_preint, dim3(n_edges), dim3(128), 0, h->stream, n_edges, d_sb, d_g, d_a, d_dt, gyr_meas_cov, acc_meas_cov,
                       d_m, d_c, imu_info_prv ? d_i : nullptr);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(imu_meas, d_m, b_m, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(cov_pvphi, d_c, b_c, hipMemcpyDeviceToHost, h->stream));
    if (imu_info_prv) HIPCHK(h, hipMemcpyAsync(imu_info_prv, d_i, b_c, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

namespace {
// Matrix::inverse() of the small dense matrices of the set-up code (Gauss-Jordan, partial pivoting)
bool inverse_host(int n, const double* A, double* Ai) {
    double M[15][30];
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) { M[i][j] = A[i * n + j]; M[i][n + j] = (i == j) ? 1.0 : 0.0; }
    for (int c = 0; c < n; c++) {
        int p = c;
        for (int r = c + 1; r < n; r++)
            if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
        if (p != c)
            for (int j = 0; j < 2 * n; j++) std::swap(M[c][j], M[p][j]);
        if (!(std::fabs(M[c][c]) > 0.0) || !std::isfinite(M[c][c])) return false;   // singular or non-finite: no information matrix
        const double inv = 1.0 / M[c][c];
        for (int j = 0; j < 2 * n; j++) M[c][j] *= inv;
        for (int r = 0; r < n; r++) {
            if (r == c) continue;
            const double f = M[r][c];
            if (f == 0.0) continue;
            for (int j = 0; j < 2 * n; j++) M[r][j] -= f * M[c][j];
        }
    }
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) {
            Ai[i * n + j] = M[i][n + j];
            if (!std::isfinite(Ai[i * n + j])) return false;
        }
    return true;
}
}  // namespace

int vba_pose_optimize(void* handle, int32_t n_frames, vba_frame_problem* const* inout, vba_frame_result* const* out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    if (n_frames <= 0 || !inout || !out) return fail(h, "vba_pose_optimize: bad arguments");
    HIPCHK(h, hipSetDevice(h->device));
    size_t n_tot = 0;
    for (int f = 0; f < n_frames; f++) {
        const vba_frame_problem* F = inout[f];
        if (!F || !out[f] || F->n_obs < 0 || (F->n_obs > 0 && (!F->obs_pw || !F->obs_uv || !F->obs_w || !out[f]->outlier)))
            return fail(h, "vba_pose_optimize: bad frame");
        if (F->last_is_frame < 0 || F->last_is_frame > 2) return fail(h, "vba_pose_optimize: unknown frame kind");
        if (F->last_is_frame == VBA_FRAME_FRAME && F->n_obs_last < 0) return fail(h, "vba_pose_optimize: negative n_obs_last");
        if (F->last_is_frame == VBA_FRAME_FRAME && F->n_obs_last > 0 && (!F->last_pw || !F->last_uv || !F->last_w)) return fail(h, "vba_pose_optimize: bad last frame");
        n_tot += (size_t)F->n_obs + (F->last_is_frame == VBA_FRAME_FRAME ? (size_t)F->n_obs_last : 0);
    }
    // one device arena and one pinned staging block with the same layout: [desc | pw | uv | w] go up in one copy,
    // [out | lvl] come back in one
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    const size_t b_desc = up(sizeof(FrameDesc) * n_frames), b_pw = up((3 * n_tot + 3) * 8), b_uv = up((2 * n_tot + 2) * 8), b_w = up((n_tot + 1) * 8);
    const size_t b_in = b_desc + b_pw + b_uv + b_w;
    const size_t b_out = up(sizeof(FrameOut) * n_frames), b_lvl = up(n_tot + 1), b_err = up((2 * n_tot + 2) * 8);
    HIPCHK(h, h->pose_arena.ensure(b_in + b_out + b_lvl + b_err));
    HIPCHK(h, h->pose_host_in.ensure(b_in));
    HIPCHK(h, h->pose_host_out.ensure(b_out + b_lvl));
    char* hin = reinterpret_cast<char*>(h->pose_host_in.p);
    FrameDesc* desc = reinterpret_cast<FrameDesc*>(hin);
    double* pw = reinterpret_cast<double*>(hin + b_desc);
    double* uv = reinterpret_cast<double*>(hin + b_desc + b_pw);
    double* ww = reinterpret_cast<double*>(hin + b_desc + b_pw + b_uv);
    {   // offsets first, then the frames are packed by a few host threads
        size_t o = 0;
        for (int f = 0; f < n_frames; f++) {
            const vba_frame_problem* F = inout[f];
            FrameDesc& d = desc[f];
            std::memset(&d, 0, sizeof d);
            d.last_is_frame = F->last_is_frame;
            d.n_obs = F->n_obs;
            d.n_last = (d.last_is_frame == VBA_FRAME_FRAME) ? F->n_obs_last : 0;
            d.obs0 = (int)o; o += d.n_obs;
            d.last0 = (int)o; o += d.n_last;
        }
    }
    std::atomic<int> bad_cov(0);
    auto pack = [&](int f) {
        const vba_frame_problem* F = inout[f];
        FrameDesc& d = desc[f];
        d.compute_marg = F->compute_marg ? 1 : 0;
        size_t o = (size_t)d.obs0;
        std::memcpy(&pw[3 * o], F->obs_pw, 24 * (size_t)d.n_obs);
        std::memcpy(&uv[2 * o], F->obs_uv, 16 * (size_t)d.n_obs);
        std::memcpy(&ww[o], F->obs_w, 8 * (size_t)d.n_obs);
        o = (size_t)d.last0;
        if (d.n_last) {
            std::memcpy(&pw[3 * o], F->last_pw, 24 * (size_t)d.n_last);
            std::memcpy(&uv[2 * o], F->last_uv, 16 * (size_t)d.n_last);
            std::memcpy(&ww[o], F->last_w, 8 * (size_t)d.n_last);
        }
        std::memcpy(d.nav, F->nav, sizeof d.nav);
        std::memcpy(d.nav_last, F->nav_last, sizeof d.nav_last);
        std::memcpy(d.prior_nav, F->prior_nav, sizeof d.prior_nav);
        std::memcpy(d.prior_info, F->prior_info, sizeof d.prior_info);
        std::memcpy(d.K, F->K, sizeof d.K);
        quat_to_R_host(F->T_cb + 3, d.Rcb);
        for (int i = 0; i < 3; i++) { d.tcb[i] = F->T_cb[i]; d.g[i] = F->g_w[i]; }
        std::memcpy(d.meas, F->imu_meas, sizeof d.meas);
        if (F->last_is_frame != VBA_FRAME_VISION && !inverse_host(9, F->imu_cov_pvphi, d.info_pvr))   // Matrix9d InvCovPVR = imupreint.getCovPVPhi().inverse(), :2103
            bad_cov.store(1);
        d.inv_bg = F->inv_bg_rw2; d.inv_ba = F->inv_ba_rw2;
        d.hub_prior = (double)(float)std::sqrt(30.5779); d.hub_pvr = (double)(float)std::sqrt(21.666);
        d.hub_bias = (double)(float)std::sqrt(16.812); d.hub_mono = (double)(float)std::sqrt(5.991);
    };
    host_parallel_for(h, n_frames, (n_frames >= 256) ? std::max(1, std::min(8, host_threads())) : 1, pack);
    if (bad_cov.load()) return fail(h, "vba_pose_optimize: imu_cov_pvphi is singular or not finite");
    char* base = reinterpret_cast<char*>(h->pose_arena.p);
    PoseBatch B;
    B.desc = reinterpret_cast<const FrameDesc*>(base);
    B.pw = reinterpret_cast<const double*>(base + b_desc);
    B.uv = reinterpret_cast<const double*>(base + b_desc + b_pw);
    B.w = reinterpret_cast<const double*>(base + b_desc + b_pw + b_uv);
    B.out = reinterpret_cast<FrameOut*>(base + b_in);
    B.lvl = reinterpret_cast<unsigned char*>(base + b_in + b_out);
    B.err = reinterpret_cast<double*>(base + b_in + b_out + b_lvl);
    B.n_frames = n_frames;
    HIPCHK(h, hipMemcpyAsync(base, hin, b_in, hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_pose_opt, dim3(n_frames), dim3(64), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    char* hout = reinterpret_cast<char*>(h->pose_host_out.p);
    HIPCHK(h, hipMemcpyAsync(hout, base + b_in, b_out + b_lvl, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    const FrameOut* res = reinterpret_cast<const FrameOut*>(hout);
    const unsigned char* lvl = reinterpret_cast<const unsigned char*>(hout + b_out);
    for (int f = 0; f < n_frames; f++) {
        vba_frame_problem* F = inout[f];
        vba_frame_result* R = out[f];
        const FrameDesc& d = desc[f];
        const FrameOut& r = res[f];
        R->n_inliers = r.n_inliers; R->status = r.status;
        for (int k = 0; k < 4; k++) { R->its_done[k] = r.its[k]; R->chi2_round[k] = r.chi2_round[k]; }
        std::memcpy(R->marg_cov_inv, r.marg, sizeof r.marg);
        std::memcpy(F->nav, r.nav, sizeof r.nav);
        for (int i = 0; i < d.n_obs; i++) R->outlier[i] = lvl[d.obs0 + i];
        if (R->outlier_last)
            for (int i = 0; i < d.n_last; i++) R->outlier_last[i] = lvl[d.last0 + i];
    }
    return 0;
}

// Optimizer::OptimizeSim3 (src/Optimizer.cpp:4579-4785) between edge set-up and write-back, for a batch of independent loop
// candidates: one arena [desc | points | keypoints | weights] goes up in one copy, k_sim3_opt runs one workgroup per candidate,
// [out | flags (| chi2 of both edges, when a caller asked for them)] come back in one copy.
int vba_sim3_optimize(void* handle, int32_t n_problems, vba_sim3_problem* const* inout, vba_sim3_result* const* out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    if (n_problems < 0 || (n_problems > 0 && (!inout || !out))) return fail(h, "vba_sim3_optimize: bad arguments");
    if (n_problems == 0) return 0;
    size_t n_tot = 0;
    bool want_chi2 = false;
    for (int f = 0; f < n_problems; f++) {
        const vba_sim3_problem* P = inout[f];
        const vba_sim3_result* R = out[f];
        auto who = [f](const char* m) { return "vba_sim3_optimize: problem " + std::to_string(f) + ": " + m; };
        if (!P || !R) return fail(h, who("NULL problem or result"));
        if (P->n_pairs < 0) return fail(h, who("negative n_pairs"));
        if (P->n_pairs > 0 && (!P->p1c || !P->p2c || !P->uv1 || !P->uv2 || !P->w1 || !P->w2 || !R->outlier))
            return fail(h, who("NULL array with n_pairs > 0"));
        for (int k = 0; k < 8; k++)
            if (!std::isfinite(P->S12[k])) return fail(h, who("S12 is not finite"));
        if (!(P->S12[7] > 0.0)) return fail(h, who("scale of S12 is not positive"));
        if (!(P->S12[3] * P->S12[3] + P->S12[4] * P->S12[4] + P->S12[5] * P->S12[5] + P->S12[6] * P->S12[6] > 0.0))
            return fail(h, who("zero quaternion in S12"));
        if (P->its_stage1 < 1 || P->its_stage2_bad < 1 || P->its_stage2_clean < 1) return fail(h, who("iteration budgets must be at least 1"));
        if (P->min_inliers < 0) return fail(h, who("negative min_inliers"));
        if (!std::isfinite(P->th2) || !std::isfinite(P->huber) || !(P->huber > 0.0)) return fail(h, who("th2 / huber are not usable"));
        n_tot += (size_t)P->n_pairs;
        want_chi2 = want_chi2 || R->chi2_12 || R->chi2_21;
    }
    HIPCHK(h, hipSetDevice(h->device));
    auto up = [](size_t b) { return (b + 255) / 256 * 256; };
    // per-pair arrays with the two sides of a pair interleaved: p [6] = P1c P2c, uv [4] = uv1 uv2, w [2] = w1 w2
    const size_t b_desc = up(sizeof(Sim3Desc) * n_problems), b_p = up((6 * n_tot + 6) * 8), b_uv = up((4 * n_tot + 4) * 8), b_w = up((2 * n_tot + 2) * 8);
    const size_t b_in = b_desc + b_p + b_uv + b_w;
    const size_t b_out = up(sizeof(Sim3Out) * n_problems), b_flag = up(n_tot + 1), b_c = up((2 * n_tot + 2) * 8);
    const size_t b_back = b_out + b_flag + (want_chi2 ? b_c : 0);
    HIPCHK(h, h->sim3_arena.ensure(b_in + b_out + b_flag + b_c));
    HIPCHK(h, h->sim3_host_in.ensure(b_in));
    HIPCHK(h, h->sim3_host_out.ensure(b_back));
    char* hin = reinterpret_cast<char*>(h->sim3_host_in.p);
    Sim3Desc* desc = reinterpret_cast<Sim3Desc*>(hin);
    double* hp = reinterpret_cast<double*>(hin + b_desc);
    double* huv = reinterpret_cast<double*>(hin + b_desc + b_p);
    double* hw = reinterpret_cast<double*>(hin + b_desc + b_p + b_uv);
    {
        size_t o = 0;
        for (int f = 0; f < n_problems; f++) {
            desc[f].pair0 = (long long)o;
            o += (size_t)inout[f]->n_pairs;
        }
    }
    auto pack = [&](int f) {
        const vba_sim3_problem* P = inout[f];
        Sim3Desc& d = desc[f];
        d.n_pairs = P->n_pairs;
        d.fix_scale = P->fix_scale ? 1 : 0;
        d.its1 = P->its_stage1; d.its2_bad = P->its_stage2_bad; d.its2_clean = P->its_stage2_clean;
        d.min_inliers = P->min_inliers;
        std::memcpy(d.S, P->S12, sizeof d.S);
        std::memcpy(d.K1, P->K1, sizeof d.K1);
        std::memcpy(d.K2, P->K2, sizeof d.K2);
        d.th2 = P->th2; d.huber = P->huber;
        const size_t o = (size_t)d.pair0, n = (size_t)d.n_pairs;
        double *qp = hp + 6 * o, *quv = huv + 4 * o, *qw = hw + 2 * o;
        for (size_t i = 0; i < n; i++) {
            for (int k = 0; k < 3; k++) { qp[6 * i + k] = P->p1c[3 * i + k]; qp[6 * i + 3 + k] = P->p2c[3 * i + k]; }
            for (int k = 0; k < 2; k++) { quv[4 * i + k] = P->uv1[2 * i + k]; quv[4 * i + 2 + k] = P->uv2[2 * i + k]; }
            qw[2 * i] = P->w1[i];
            qw[2 * i + 1] = P->w2[i];
        }
    };
    host_parallel_for(h, n_problems, (n_problems >= 256) ? std::max(1, std::min(8, host_threads())) : 1, pack);
    char* base = reinterpret_cast<char*>(h->sim3_arena.p);
    Sim3Batch B;
    B.desc = reinterpret_cast<const Sim3Desc*>(base);
    B.p = reinterpret_cast<const double*>(base + b_desc);
    B.uv = reinterpret_cast<const double*>(base + b_desc + b_p);
    B.w = reinterpret_cast<const double*>(base + b_desc + b_p + b_uv);
    B.out = reinterpret_cast<Sim3Out*>(base + b_in);
    B.flag = reinterpret_cast<unsigned char*>(base + b_in + b_out);
    B.c = reinterpret_cast<double*>(base + b_in + b_out + b_flag);
    const long long launch0 = h->n_launch;
    HIPCHK(h, hipMemcpyAsync(base, hin, b_in, hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_sim3_opt, dim3(n_problems), dim3(64), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    char* hout = reinterpret_cast<char*>(h->sim3_host_out.p);
    HIPCHK(h, hipMemcpyAsync(hout, base + b_in, b_back, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->prof.kernel_launches = h->n_launch - launch0;
    const Sim3Out* res = reinterpret_cast<const Sim3Out*>(hout);
    const unsigned char* flag = reinterpret_cast<const unsigned char*>(hout + b_out);
    const double* cc = reinterpret_cast<const double*>(hout + b_out + b_flag);
    for (int f = 0; f < n_problems; f++) {
        vba_sim3_problem* P = inout[f];
        vba_sim3_result* R = out[f];
        const Sim3Out& r = res[f];
        const size_t o = (size_t)desc[f].pair0, n = (size_t)desc[f].n_pairs;
        R->n_inliers = r.n_inliers; R->status = r.status; R->n_bad_stage1 = r.n_bad1;
        for (int k = 0; k < 2; k++) { R->its_done[k] = r.its[k]; R->chi2_stage[k] = r.chi2_stage[k]; }
        std::memcpy(P->S12, r.S, sizeof r.S);   // the input, bit for bit, when the candidate is rejected (:4755)
        if (n) std::memcpy(R->outlier, flag + o, n);
        for (size_t i = 0; i < n && R->chi2_12; i++) R->chi2_12[i] = cc[2 * (o + i)];
        for (size_t i = 0; i < n && R->chi2_21; i++) R->chi2_21[i] = cc[2 * (o + i) + 1];
    }
    return 0;
}

namespace {
// what vba_debug_posegraph_system asks of a run: graph 0 stops after the solve of its first trial, and H, b, x come back
struct PgDebug { double *H, *b, *x; };

// Optimizer::OptimizeEssentialGraph (src/Optimizer.cpp:4243-4552) between edge set-up and write-back, for a batch of independent
// graphs: the host validates every graph and lays out its envelope (vba_host_posegraph.h), one staging block [desc | estimates |
// measurements | index lists | points] goes up in one copy, k_posegraph_opt runs one workgroup per graph, k_posegraph_points moves
// the map points when there are any, and [out | estimates | points] come back in one copy.
static int posegraph_run(Handle* h, int32_t n_graphs, vba_posegraph_problem* const* inout, vba_posegraph_result* const* out, PgDebug* dbg) {
    if (n_graphs < 0 || (n_graphs > 0 && (!inout || !out))) return fail(h, "vba_posegraph_optimize: bad arguments");
    if (n_graphs == 0) return 0;
    std::vector<vba_host::PoseGraphLayout> lay(n_graphs);
    std::vector<PgDesc> hd(n_graphs);
    size_t nv = 0, ne = 0, nf = 0, nenv = 0, ninc = 0, npair = 0, npe = 0, npt = 0;
    for (int g = 0; g < n_graphs; g++) {
        std::string err;
        if (!inout[g] || !out[g]) return fail(h, "vba_posegraph_optimize: graph " + std::to_string(g) + ": NULL problem or result");
        if (vba_host::build_posegraph(inout[g], lay[g], err, (long long)nenv))
            return fail(h, "vba_posegraph_optimize: graph " + std::to_string(g) + ": " + err);
        const vba_posegraph_problem* P = inout[g];
        const vba_host::PoseGraphLayout& L = lay[g];
        PgDesc& d = hd[g];
        std::memset(&d, 0, sizeof d);
        d.nv = P->n_vertices; d.ne = P->n_edges; d.nf = L.n_free; d.npair = (int)L.pair_lo.size();
        d.fix_scale = P->fix_scale ? 1 : 0; d.its = P->its; d.n_pt = P->n_pt; d.debug = (dbg && g == 0) ? 1 : 0;
        d.lambda_init = P->lambda_init;
        d.v0 = (long long)nv; d.e0 = (long long)ne; d.f0 = (long long)nf; d.r0 = (long long)nf + g; d.env0 = (long long)nenv;
        d.inc0 = (long long)ninc; d.pair0 = (long long)npair; d.pb0 = (long long)npair + g; d.pe0 = (long long)npe; d.pt0 = (long long)npt;
        nv += (size_t)d.nv; ne += (size_t)d.ne; nf += (size_t)d.nf; nenv += (size_t)L.env_blocks; ninc += L.inc.size();
        npair += L.pair_lo.size(); npe += L.pair_edge.size(); npt += (size_t)d.n_pt;
    }
    HIPCHK(h, hipSetDevice(h->device));
    // regions of the arena, each a multiple of 256 bytes: [upload | back | work]
    size_t cur = 0;
    auto take = [&cur](size_t bytes) { const size_t o = cur; cur += (bytes + 8 + 255) / 256 * 256; return o; };
    const size_t G = (size_t)n_graphs;
    const size_t o_desc = take(sizeof(PgDesc) * G), o_Sin = take(64 * nv), o_meas = take(64 * ne), o_ei = take(4 * ne), o_ej = take(4 * ne);
    const size_t o_free = take(4 * nv), o_vert = take(4 * nf), o_first = take(4 * nf), o_last = take(4 * nf), o_roff = take(4 * (nf + G));
    const size_t o_incb = take(4 * (nf + G)), o_inc = take(4 * ninc), o_plo = take(4 * npair), o_phi = take(4 * npair);
    const size_t o_pb = take(4 * (npair + G)), o_pe = take(4 * npe), o_pt = take(24 * npt), o_ref = take(4 * npt);
    const size_t b_in = cur;
    const size_t o_out = take(sizeof(PgOut) * G), o_S = take(64 * nv), o_pto = take(24 * npt);
    const size_t b_back = cur - b_in;
    const size_t o_Sbk = take(64 * nv), o_err = take(56 * ne), o_J = take(784 * ne), o_H = take(392 * nenv), o_F = take(392 * nenv);
    const size_t o_Ld = take(392 * nf), o_b = take(56 * nf), o_w = take(56 * nf), o_y = take(56 * nf), o_x = take(56 * nf);
    HIPCHK(h, h->pg_arena.ensure(cur));
    HIPCHK(h, h->pg_host_in.ensure(b_in));
    HIPCHK(h, h->pg_host_out.ensure(b_back));
    char* hin = reinterpret_cast<char*>(h->pg_host_in.p);
    std::memcpy(hin + o_desc, hd.data(), sizeof(PgDesc) * G);
    auto pack = [&](int g) {
        const vba_posegraph_problem* P = inout[g];
        const vba_host::PoseGraphLayout& L = lay[g];
        const PgDesc& d = hd[g];
        auto put = [hin](size_t o, size_t at, const void* src, size_t bytes) { if (bytes) std::memcpy(hin + o + at, src, bytes); };
        put(o_Sin, 64 * (size_t)d.v0, P->S, 64 * (size_t)d.nv);
        put(o_meas, 64 * (size_t)d.e0, P->edge_S, 64 * (size_t)d.ne);
        put(o_ei, 4 * (size_t)d.e0, P->edge_i, 4 * (size_t)d.ne);
        put(o_ej, 4 * (size_t)d.e0, P->edge_j, 4 * (size_t)d.ne);
        put(o_free, 4 * (size_t)d.v0, L.free_of.data(), 4 * (size_t)d.nv);
        put(o_vert, 4 * (size_t)d.f0, L.vert_of.data(), 4 * (size_t)d.nf);
        put(o_first, 4 * (size_t)d.f0, L.first.data(), 4 * (size_t)d.nf);
        put(o_last, 4 * (size_t)d.f0, L.last_row.data(), 4 * (size_t)d.nf);
        put(o_roff, 4 * (size_t)d.r0, L.row_off.data(), 4 * ((size_t)d.nf + 1));
        put(o_incb, 4 * (size_t)d.r0, L.inc_begin.data(), 4 * ((size_t)d.nf + 1));
        put(o_inc, 4 * (size_t)d.inc0, L.inc.data(), 4 * L.inc.size());
        put(o_plo, 4 * (size_t)d.pair0, L.pair_lo.data(), 4 * L.pair_lo.size());
        put(o_phi, 4 * (size_t)d.pair0, L.pair_hi.data(), 4 * L.pair_hi.size());
        put(o_pb, 4 * (size_t)d.pb0, L.pair_begin.data(), 4 * L.pair_begin.size());
        put(o_pe, 4 * (size_t)d.pe0, L.pair_edge.data(), 4 * L.pair_edge.size());
        put(o_pt, 24 * (size_t)d.pt0, P->pt, 24 * (size_t)d.n_pt);
        int* ref = reinterpret_cast<int*>(hin + o_ref) + d.pt0;
        for (int p = 0; p < d.n_pt; p++) ref[p] = (int)d.v0 + P->pt_ref[p];   // index into the concatenated vertices
    };
    for (int g = 0; g < n_graphs; g++) pack(g);
    char* base = reinterpret_cast<char*>(h->pg_arena.p);
    PgBatch B;
    auto cd = [base](size_t o) { return reinterpret_cast<const double*>(base + o); };
    auto ci = [base](size_t o) { return reinterpret_cast<const int*>(base + o); };
    auto md = [base](size_t o) { return reinterpret_cast<double*>(base + o); };
    B.desc = reinterpret_cast<const PgDesc*>(base + o_desc);
    B.out = reinterpret_cast<PgOut*>(base + o_out);
    B.Sin = cd(o_Sin); B.meas = cd(o_meas); B.ei = ci(o_ei); B.ej = ci(o_ej); B.free_of = ci(o_free);
    B.vert_of = ci(o_vert); B.first = ci(o_first); B.last_row = ci(o_last); B.row_off = ci(o_roff); B.inc_begin = ci(o_incb);
    B.inc = ci(o_inc); B.pair_lo = ci(o_plo); B.pair_hi = ci(o_phi); B.pair_begin = ci(o_pb); B.pair_edge = ci(o_pe);
    B.pt_in = cd(o_pt); B.pt_ref = ci(o_ref);
    B.S = md(o_S); B.Sbk = md(o_Sbk); B.err = md(o_err); B.J = md(o_J); B.H = md(o_H); B.F = md(o_F); B.Ld = md(o_Ld);
    B.b = md(o_b); B.w = md(o_w); B.y = md(o_y); B.x = md(o_x); B.pt_out = md(o_pto);
    B.n_pt_total = (long long)npt;
    const long long launch0 = h->n_launch;
    HIPCHK(h, hipMemcpyAsync(base, hin, b_in, hipMemcpyHostToDevice, h->stream));
    VBA_LAUNCH(k_posegraph_opt, dim3(n_graphs), dim3(PG_NT), 0, h->stream, B);
    HIPCHK(h, hipGetLastError());
    if (npt > 0 && !dbg) {
        VBA_LAUNCH(k_posegraph_points, dim3((unsigned)((npt + 255) / 256)), dim3(256), 0, h->stream, B);
        HIPCHK(h, hipGetLastError());
    }
    char* hout = reinterpret_cast<char*>(h->pg_host_out.p);
    HIPCHK(h, hipMemcpyAsync(hout, base + b_in, b_back, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->prof.kernel_launches = h->n_launch - launch0;
    if (dbg) {   // graph 0 as the kernel formed it: the envelope expanded to a dense symmetric matrix, b, x
        const vba_host::PoseGraphLayout& L = lay[0];
        const size_t n = 7 * (size_t)L.n_free;
        std::vector<double> env(49 * (size_t)L.env_blocks);
        HIPCHK(h, hipMemcpy(env.data(), base + o_H, env.size() * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(dbg->b, base + o_b, n * 8, hipMemcpyDeviceToHost));
        HIPCHK(h, hipMemcpy(dbg->x, base + o_x, n * 8, hipMemcpyDeviceToHost));
        std::fill(dbg->H, dbg->H + n * n, 0.0);
        for (int r = 0; r < L.n_free; r++)
            for (int c = L.first[r]; c <= r; c++) {
                const double* blk = env.data() + 49 * (size_t)(L.row_off[r] + c - L.first[r]);
                for (int a = 0; a < 7; a++)
                    for (int k = 0; k < 7; k++) {
                        dbg->H[(7 * (size_t)r + a) * n + 7 * (size_t)c + k] = blk[7 * a + k];
                        if (c < r) dbg->H[(7 * (size_t)c + k) * n + 7 * (size_t)r + a] = blk[7 * a + k];
                    }
            }
        return 0;
    }
    const PgOut* res = reinterpret_cast<const PgOut*>(hout + (o_out - b_in));
    const double* Sf = reinterpret_cast<const double*>(hout + (o_S - b_in));
    const double* pf = reinterpret_cast<const double*>(hout + (o_pto - b_in));
    for (int g = 0; g < n_graphs; g++) {
        vba_posegraph_problem* P = inout[g];
        vba_posegraph_result* R = out[g];
        const PgDesc& d = hd[g];
        const PgOut& r = res[g];
        R->status = r.status; R->its_done = r.its_done; R->lm_trials = r.lm_trials; R->stop = r.stop;
        R->chi2_initial = r.chi2_initial; R->chi2_final = r.chi2_final; R->lambda_final = r.lambda_final;
        if (d.nv) std::memcpy(P->S, Sf + 8 * (size_t)d.v0, 64 * (size_t)d.nv);   // fixed vertices: the input, bit for bit
        if (d.n_pt) std::memcpy(P->pt, pf + 3 * (size_t)d.pt0, 24 * (size_t)d.n_pt);
    }
    return 0;
}
}  // namespace

int vba_posegraph_optimize(void* handle, int32_t n_graphs, vba_posegraph_problem* const* inout, vba_posegraph_result* const* out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    return posegraph_run(h, n_graphs, inout, out, nullptr);
}

#ifdef VBA_TEST_HOOKS
// test hook (not part of include/vislam_ba.h): H (dense, [7 n_free]^2 row-major), b and the x of the first trial of the first
// iteration of one graph, as k_posegraph_opt formed them; the graph's arrays are left untouched
int vba_debug_posegraph_system(void* handle, vba_posegraph_problem* graph, double* H, double* b, double* x) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    if (!graph || !H || !b || !x) return fail(h, "vba_debug_posegraph_system: bad arguments");
    PgDebug dbg{H, b, x};
    vba_posegraph_result r;
    vba_posegraph_result* rp = &r;
    return posegraph_run(h, 1, &graph, &rp, &dbg);
}
#endif

int vba_set_profile(void* handle, int32_t enable) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || async_busy(h)) return -1;
    h->profile = enable != 0;
    return 0;
}
int vba_get_profile(void* handle, vba_profile* out) {
    Handle* h = reinterpret_cast<Handle*>(handle);
    if (!h || !out) return -1;
    *out = h->prof;
    return 0;
}

}  // extern "C"
