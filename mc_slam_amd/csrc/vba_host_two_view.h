// vba_host_two_view.h -- host half of vba_two_view_init (plain C++17, no HIP): which pairs are refused, the arena of a call, the
// descriptor of a pair, the packing into the staging block, the write-back.  Included by vislam_ba.hip (vba_host_small.h) and by
// the sanitizer harness tests/host_two_view_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_two_view.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace vba_host {

// totals of a call: keypoints of the frames 1 / 2, matches, hypotheses; want_scores: a caller asked for the score of every hypothesis
struct TwoViewTotals {
    size_t k1 = 0, k2 = 0, m = 0, h = 0;
    bool want_scores = false;
};

// 0: every pair is usable; otherwise err says which is not and why
inline int check_two_view(int n, const vba_two_view_problem* const* in, const vba_two_view_result* const* out, TwoViewTotals& T, std::string& err) {
    T = TwoViewTotals();
    std::vector<unsigned char> seen;
    for (int f = 0; f < n; f++) {
        const vba_two_view_problem* P = in[f];
        const vba_two_view_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "pair " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->n_keys1 < 0 || P->n_keys2 < 0) return fail("negative n_keys");
        if (P->n_matches < 0) return fail("negative n_matches");
        if (P->n_hyp < 0) return fail("negative n_hyp");
        if ((P->n_keys1 > 0 && (!P->uv1 || !R->x3d || !R->triangulated)) || (P->n_keys2 > 0 && !P->uv2)) return fail("NULL array with n_keys > 0");
        if (P->n_matches > 0 && (!P->match || !R->inlier_h || !R->inlier_f)) return fail("NULL array with n_matches > 0");
        if (P->n_hyp > 0 && !P->sets) return fail("NULL sets with n_hyp > 0");
        if (P->n_hyp > 0 && P->n_matches < 8) return fail("n_matches < 8 with n_hyp > 0");
        for (int k = 0; k < 4; k++)
            if (!std::isfinite(P->K[k])) return fail("K is not finite");
        if (P->K[0] == 0.0 || P->K[1] == 0.0) return fail("zero fx / fy");
        if (!std::isfinite(P->sigma) || !std::isfinite(P->min_parallax)) return fail("sigma / min_parallax is not finite");
        if (P->sigma == 0.0) return fail("zero sigma");
        for (size_t i = 0, e = 2 * (size_t)P->n_keys1; i < e; i++)
            if (!std::isfinite(P->uv1[i])) return fail("keypoint " + std::to_string(i / 2) + " of frame 1: a pixel is not finite");
        for (size_t i = 0, e = 2 * (size_t)P->n_keys2; i < e; i++)
            if (!std::isfinite(P->uv2[i])) return fail("keypoint " + std::to_string(i / 2) + " of frame 2: a pixel is not finite");
        seen.assign((size_t)P->n_keys1, 0);
        for (size_t i = 0, e = (size_t)P->n_matches; i < e; i++) {
            const int a = P->match[2 * i], b = P->match[2 * i + 1];
            if (a < 0 || a >= P->n_keys1 || b < 0 || b >= P->n_keys2) return fail("match " + std::to_string(i) + ": index outside its frame");
            if (seen[(size_t)a]) return fail("match " + std::to_string(i) + ": repeated first index");
            seen[(size_t)a] = 1;
        }
        for (size_t i = 0, e = 8 * (size_t)P->n_hyp; i < e; i++)
            if (P->sets[i] < 0 || P->sets[i] >= P->n_matches) return fail("hypothesis " + std::to_string(i / 8) + ": set index out of range");
        T.k1 += (size_t)P->n_keys1; T.k2 += (size_t)P->n_keys2; T.m += (size_t)P->n_matches; T.h += (size_t)P->n_hyp;
        T.want_scores = T.want_scores || R->hyp_score_h || R->hyp_score_f;
    }
    return 0;
}

// [desc | uv1 | uv2 | match | sets] go up in one copy, [out | flag_h | flag_f | tri | x3d | score_h | score_f] come back in one -- the
// two score regions only when a caller asked for them -- and the rest never leaves the device: the hypothesis records and, per
// ((R, t) hypothesis, match), the state (0 rejected, 1 counted in nGood, 2 counted and cosParallax < 0.99998), the cosine and the
// point CheckRT left: region of a pair at VBA_TV_RT * match0, hypothesis k at + k * n_matches
struct TwoViewArena {
    ArenaLayout L;
    size_t desc, uv1, uv2, match, sets, out, flag_h, flag_f, tri, x3d, score_h, score_f, hyp_h, hyp_f, rt_state, rt_cos, rt_x;
    TwoViewArena(size_t n, const TwoViewTotals& T) {
        desc = L.take(sizeof(TvDesc) * n); uv1 = L.take((2 * T.k1 + 2) * 8); uv2 = L.take((2 * T.k2 + 2) * 8);
        match = L.take((2 * T.m + 2) * 4); sets = L.take((8 * T.h + 8) * 4);
        L.end_upload();
        out = L.take(sizeof(TvOut) * n); flag_h = L.take(T.m + 1); flag_f = L.take(T.m + 1); tri = L.take(T.k1 + 1); x3d = L.take((3 * T.k1 + 3) * 8);
        score_h = L.take((T.h + 1) * 8); score_f = L.take((T.h + 1) * 8);
        L.end_back();
        hyp_h = L.take((T.h + 1) * VBA_TV_HYP_H * 8); hyp_f = L.take((T.h + 1) * VBA_TV_HYP_F * 8);
        rt_state = L.take(VBA_TV_RT * T.m + 1); rt_cos = L.take((VBA_TV_RT * T.m + 1) * 8); rt_x = L.take((VBA_TV_RT * T.m + 1) * 24);
    }
    size_t download_bytes(bool want_scores) const { return want_scores ? L.back_bytes() : L.in_back(score_h); }
};

// offsets of every pair's keypoints, matches and hypotheses in the concatenated arrays (the rest of a descriptor comes with the packing)
inline void describe_two_view(int n, const vba_two_view_problem* const* in, TvDesc* desc) {
    size_t k1 = 0, k2 = 0, m = 0, h = 0;
    for (int f = 0; f < n; f++) {
        desc[f].key1_0 = (long long)k1; desc[f].key2_0 = (long long)k2; desc[f].match0 = (long long)m; desc[f].hyp0 = (long long)h;
        k1 += (size_t)in[f]->n_keys1; k2 += (size_t)in[f]->n_keys2; m += (size_t)in[f]->n_matches; h += (size_t)in[f]->n_hyp;
    }
}

// one pair into the staging block: the rest of its descriptor and its four arrays at their offsets
inline void pack_two_view(const vba_two_view_problem* P, TvDesc& d, double* huv1, double* huv2, int32_t* hmatch, int32_t* hsets) {
    d.n_keys1 = P->n_keys1; d.n_keys2 = P->n_keys2; d.n_matches = P->n_matches; d.n_hyp = P->n_hyp;
    d.min_triangulated = P->min_triangulated;
    d.pad = 0;
    std::memcpy(d.K, P->K, sizeof d.K);
    d.sigma = P->sigma;
    d.min_parallax = P->min_parallax;
    if (d.n_keys1) std::memcpy(huv1 + 2 * (size_t)d.key1_0, P->uv1, 16 * (size_t)d.n_keys1);
    if (d.n_keys2) std::memcpy(huv2 + 2 * (size_t)d.key2_0, P->uv2, 16 * (size_t)d.n_keys2);
    if (d.n_matches) std::memcpy(hmatch + 2 * (size_t)d.match0, P->match, 8 * (size_t)d.n_matches);
    if (d.n_hyp) std::memcpy(hsets + 8 * (size_t)d.hyp0, P->sets, 32 * (size_t)d.n_hyp);
}

// the call's back regions as they came back (sh / sf are read only where the caller gave an array).  R21, t21, x3d and triangulated
// are written when ok, and only then
inline void unpack_two_view(vba_two_view_result* R, const TvDesc& d, const TvOut& r, const unsigned char* fh, const unsigned char* ff,
                            const unsigned char* tri, const double* x3d, const double* sh, const double* sf) {
    const size_t n = (size_t)d.n_matches, nk = (size_t)d.n_keys1, nh = (size_t)d.n_hyp;
    R->status = r.status; R->ok = r.ok; R->model = r.model; R->reason = r.reason;
    R->best_hyp_h = r.best_hyp_h; R->best_hyp_f = r.best_hyp_f; R->n_inliers_h = r.n_inliers_h; R->n_inliers_f = r.n_inliers_f;
    R->n_rt = r.n_rt; R->best_rt = r.best_rt;
    std::memcpy(R->rt_good, r.rt_good, sizeof r.rt_good);
    R->score_h = r.score_h; R->score_f = r.score_f; R->rh = r.rh;
    std::memcpy(R->H21, r.H21, sizeof r.H21);
    std::memcpy(R->F21, r.F21, sizeof r.F21);
    std::memcpy(R->rt_parallax, r.rt_parallax, sizeof r.rt_parallax);
    if (n) {
        std::memcpy(R->inlier_h, fh + (size_t)d.match0, n);
        std::memcpy(R->inlier_f, ff + (size_t)d.match0, n);
    }
    if (r.ok) {
        std::memcpy(R->R21, r.R21, sizeof r.R21);
        std::memcpy(R->t21, r.t21, sizeof r.t21);
        if (nk) {
            std::memcpy(R->x3d, x3d + 3 * (size_t)d.key1_0, 24 * nk);
            std::memcpy(R->triangulated, tri + (size_t)d.key1_0, nk);
        }
    }
    if (R->hyp_score_h && nh) std::memcpy(R->hyp_score_h, sh + (size_t)d.hyp0, 8 * nh);
    if (R->hyp_score_f && nh) std::memcpy(R->hyp_score_f, sf + (size_t)d.hyp0, 8 * nh);
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct TwoViewCall {
    int n = 0;
    TwoViewTotals T;
    TwoViewArena A = TwoViewArena(0, TwoViewTotals());
    int prepare(int n_problems, const vba_two_view_problem* const* in, const vba_two_view_result* const* out, std::string& err) {
        n = n_problems;
        if (check_two_view(n, in, out, T, err)) return 1;
        A = TwoViewArena((size_t)n, T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.download_bytes(T.want_scores); }
    size_t grid() const { return (size_t)n; }   // k_two_view: one workgroup per pair
    TvDesc* desc(void* hin) const { return at<TvDesc>(hin, A.desc); }
    void describe(const vba_two_view_problem* const* in, void* hin) const { describe_two_view(n, in, desc(hin)); }
    const char* pack(int f, const vba_two_view_problem* P, void* hin) const {
        pack_two_view(P, desc(hin)[f], at<double>(hin, A.uv1), at<double>(hin, A.uv2), at<int32_t>(hin, A.match), at<int32_t>(hin, A.sets));
        return nullptr;
    }
    TvBatch bind(void* base) const {
        TvBatch B;
        B.desc = desc(base); B.uv1 = at<double>(base, A.uv1); B.uv2 = at<double>(base, A.uv2); B.match = at<int>(base, A.match);
        B.sets = at<int>(base, A.sets); B.out = at<TvOut>(base, A.out); B.flag_h = at<unsigned char>(base, A.flag_h);
        B.flag_f = at<unsigned char>(base, A.flag_f); B.tri = at<unsigned char>(base, A.tri); B.x3d = at<double>(base, A.x3d);
        B.score_h = at<double>(base, A.score_h); B.score_f = at<double>(base, A.score_f); B.hyp_h = at<double>(base, A.hyp_h);
        B.hyp_f = at<double>(base, A.hyp_f); B.rt_state = at<unsigned char>(base, A.rt_state); B.rt_cos = at<double>(base, A.rt_cos);
        B.rt_x = at<double>(base, A.rt_x);
        return B;
    }
    void unpack(int f, vba_two_view_problem*, vba_two_view_result* R, void* hin, void* hout) const {
        auto u8 = [&](size_t o) { return at<unsigned char>(hout, A.L.in_back(o)); };
        auto f64 = [&](size_t o) { return at<double>(hout, A.L.in_back(o)); };
        unpack_two_view(R, desc(hin)[f], at<TvOut>(hout, A.L.in_back(A.out))[f], u8(A.flag_h), u8(A.flag_f), u8(A.tri), f64(A.x3d), f64(A.score_h),
                        f64(A.score_f));
    }
};

}  // namespace vba_host
