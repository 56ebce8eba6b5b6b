// vba_host_pose.h -- host half of vba_pose_optimize (plain C++17, no HIP): which frames are refused, the arena of a call, the
// descriptor of a frame and its packing into the staging block, the write-back.  Included by vislam_ba.hip (vba_host_small.h) and
// by the sanitizer harness tests/host_small_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_small.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_host_layout.h"   // quat_to_R_host

#include <cmath>
#include <cstring>
#include <string>
#include <utility>

namespace vba_host {

// Matrix::inverse() of the small dense matrices of the set-up code (Gauss-Jordan, partial pivoting)
inline bool inverse_host(int n, const double* A, double* Ai) {
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

// why the frames cannot be optimised (nullptr: they can); n_tot: observations of the call, the last frames' included
inline const char* check_pose(int n_frames, const vba_frame_problem* const* in, const vba_frame_result* const* out, size_t& n_tot) {
    n_tot = 0;
    for (int f = 0; f < n_frames; f++) {
        const vba_frame_problem* F = in[f];
        if (!F || !out[f] || F->n_obs < 0 || (F->n_obs > 0 && (!F->obs_pw || !F->obs_uv || !F->obs_w || !out[f]->outlier))) return "bad frame";
        if (F->last_is_frame < 0 || F->last_is_frame > 2) return "unknown frame kind";
        if (F->last_is_frame == VBA_FRAME_FRAME && F->n_obs_last < 0) return "negative n_obs_last";
        if (F->last_is_frame == VBA_FRAME_FRAME && F->n_obs_last > 0 && (!F->last_pw || !F->last_uv || !F->last_w)) return "bad last frame";
        n_tot += (size_t)F->n_obs + (F->last_is_frame == VBA_FRAME_FRAME ? (size_t)F->n_obs_last : 0);
    }
    return nullptr;
}

// [desc | pw | uv | w] go up in one copy, [out | lvl] come back in one, err stays on the device
struct PoseArena {
    ArenaLayout L;
    size_t desc, pw, uv, w, out, lvl, err;
    PoseArena(size_t n_frames, size_t n_tot) {
        desc = L.take(sizeof(FrameDesc) * n_frames); pw = L.take((3 * n_tot + 3) * 8); uv = L.take((2 * n_tot + 2) * 8); w = L.take((n_tot + 1) * 8);
        L.end_upload();
        out = L.take(sizeof(FrameOut) * n_frames); lvl = L.take(n_tot + 1);
        L.end_back();
        err = L.take((2 * n_tot + 2) * 8);
    }
};

// sizes and offsets of every frame into the concatenated observation arrays (the rest of a descriptor comes with the packing)
inline void describe_pose(int n_frames, const vba_frame_problem* const* in, FrameDesc* desc) {
    size_t o = 0;
    for (int f = 0; f < n_frames; f++) {
        const vba_frame_problem* F = in[f];
        FrameDesc& d = desc[f];
        std::memset(&d, 0, sizeof d);
        d.last_is_frame = F->last_is_frame;
        d.n_obs = F->n_obs;
        d.n_last = (d.last_is_frame == VBA_FRAME_FRAME) ? F->n_obs_last : 0;
        d.obs0 = (int)o; o += d.n_obs;
        d.last0 = (int)o; o += d.n_last;
    }
}

// one frame into the staging block: its observations at obs0 / last0 of pw, uv, ww and the rest of its descriptor.  false: the
// preintegration covariance is singular or not finite
inline bool pack_frame(const vba_frame_problem* F, FrameDesc& d, double* pw, double* uv, double* ww) {
    bool ok = true;
    d.compute_marg = F->compute_marg ? 1 : 0;
    size_t o = (size_t)d.obs0;
    if (d.n_obs) {
        std::memcpy(&pw[3 * o], F->obs_pw, 24 * (size_t)d.n_obs);
        std::memcpy(&uv[2 * o], F->obs_uv, 16 * (size_t)d.n_obs);
        std::memcpy(&ww[o], F->obs_w, 8 * (size_t)d.n_obs);
    }
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
        ok = false;
    d.inv_bg = F->inv_bg_rw2; d.inv_ba = F->inv_ba_rw2;
    d.hub_prior = (double)(float)std::sqrt(30.5779); d.hub_pvr = (double)(float)std::sqrt(21.666);
    d.hub_bias = (double)(float)std::sqrt(16.812); d.hub_mono = (double)(float)std::sqrt(5.991);
    return ok;
}

inline void unpack_frame(vba_frame_problem* F, vba_frame_result* R, const FrameDesc& d, const FrameOut& r, const unsigned char* lvl) {
    R->n_inliers = r.n_inliers; R->status = r.status;
    for (int k = 0; k < 4; k++) { R->its_done[k] = r.its[k]; R->chi2_round[k] = r.chi2_round[k]; }
    std::memcpy(R->marg_cov_inv, r.marg, sizeof r.marg);
    std::memcpy(F->nav, r.nav, sizeof r.nav);
    for (int i = 0; i < d.n_obs; i++) R->outlier[i] = lvl[d.obs0 + i];
    if (R->outlier_last)
        for (int i = 0; i < d.n_last; i++) R->outlier_last[i] = lvl[d.last0 + i];
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct PoseCall {
    int n = 0;
    size_t n_tot = 0;
    PoseArena A = PoseArena(0, 0);
    int prepare(int n_frames, const vba_frame_problem* const* in, const vba_frame_result* const* out, std::string& err) {
        n = n_frames;
        if (const char* m = check_pose(n, in, out, n_tot)) { err = m; return 1; }
        A = PoseArena((size_t)n, n_tot);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return (size_t)n; }   // k_pose_opt: one workgroup per frame
    FrameDesc* desc(void* hin) const { return at<FrameDesc>(hin, A.desc); }
    void describe(const vba_frame_problem* const* in, void* hin) const { describe_pose(n, in, desc(hin)); }
    // not nullptr: why the frame is refused after all
    const char* pack(int f, const vba_frame_problem* F, void* hin) const {
        return pack_frame(F, desc(hin)[f], at<double>(hin, A.pw), at<double>(hin, A.uv), at<double>(hin, A.w)) ? nullptr
                                                                                                             : "imu_cov_pvphi is singular or not finite";
    }
    PoseBatch bind(void* base) const {
        PoseBatch B;
        B.desc = desc(base); B.out = at<FrameOut>(base, A.out); B.pw = at<double>(base, A.pw); B.uv = at<double>(base, A.uv);
        B.w = at<double>(base, A.w); B.err = at<double>(base, A.err); B.lvl = at<unsigned char>(base, A.lvl);
        B.n_frames = n;
        return B;
    }
    void unpack(int f, vba_frame_problem* F, vba_frame_result* R, void* hin, void* hout) const {
        unpack_frame(F, R, desc(hin)[f], at<FrameOut>(hout, A.L.in_back(A.out))[f], at<unsigned char>(hout, A.L.in_back(A.lvl)));
    }
};

}  // namespace vba_host
