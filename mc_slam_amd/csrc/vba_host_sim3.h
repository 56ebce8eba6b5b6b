// vba_host_sim3.h -- host half of vba_sim3_optimize (plain C++17, no HIP): which candidates are refused, the arena of a call, the
// descriptor of a candidate and its packing into the staging block, the write-back.  Included by vislam_ba.hip (vba_host_small.h)
// and by the sanitizer harness tests/host_small_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_small.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>

namespace vba_host {

// 0: every candidate is usable; otherwise err says which is not and why.  n_tot: pairs of the call; want_chi2: a caller asked for
// the chi2 of the edges
inline int check_sim3(int n, const vba_sim3_problem* const* in, const vba_sim3_result* const* out, size_t& n_tot, bool& want_chi2, std::string& err) {
    n_tot = 0;
    want_chi2 = false;
    for (int f = 0; f < n; f++) {
        const vba_sim3_problem* P = in[f];
        const vba_sim3_result* R = out[f];
        auto fail = [&err, f](const char* m) { err = "problem " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->n_pairs < 0) return fail("negative n_pairs");
        if (P->n_pairs > 0 && (!P->p1c || !P->p2c || !P->uv1 || !P->uv2 || !P->w1 || !P->w2 || !R->outlier)) return fail("NULL array with n_pairs > 0");
        for (int k = 0; k < 8; k++)
            if (!std::isfinite(P->S12[k])) return fail("S12 is not finite");
        if (!(P->S12[7] > 0.0)) return fail("scale of S12 is not positive");
        if (!(P->S12[3] * P->S12[3] + P->S12[4] * P->S12[4] + P->S12[5] * P->S12[5] + P->S12[6] * P->S12[6] > 0.0)) return fail("zero quaternion in S12");
        if (P->its_stage1 < 1 || P->its_stage2_bad < 1 || P->its_stage2_clean < 1) return fail("iteration budgets must be at least 1");
        if (P->min_inliers < 0) return fail("negative min_inliers");
        if (!std::isfinite(P->th2) || !std::isfinite(P->huber) || !(P->huber > 0.0)) return fail("th2 / huber are not usable");
        n_tot += (size_t)P->n_pairs;
        want_chi2 = want_chi2 || R->chi2_12 || R->chi2_21;
    }
    return 0;
}

// [desc | p | uv | w] go up in one copy, [out | flag | c] come back in one -- c, the chi2 of both edges of every pair, only when
// a caller asked for it.  Per-pair arrays with the two sides of a pair interleaved: p [6] = P1c P2c, uv [4] = uv1 uv2, w [2] = w1 w2
struct Sim3Arena {
    ArenaLayout L;
    size_t desc, p, uv, w, out, flag, c;
    Sim3Arena(size_t n, size_t n_tot) {
        desc = L.take(sizeof(Sim3Desc) * n); p = L.take((6 * n_tot + 6) * 8); uv = L.take((4 * n_tot + 4) * 8); w = L.take((2 * n_tot + 2) * 8);
        L.end_upload();
        out = L.take(sizeof(Sim3Out) * n); flag = L.take(n_tot + 1); c = L.take((2 * n_tot + 2) * 8);
        L.end_back();
    }
    size_t download_bytes(bool want_chi2) const { return want_chi2 ? L.back_bytes() : L.in_back(c); }
};

// offset of every candidate's pairs in the concatenated arrays (the rest of a descriptor comes with the packing)
inline void describe_sim3(int n, const vba_sim3_problem* const* in, Sim3Desc* desc) {
    size_t o = 0;
    for (int f = 0; f < n; f++) {
        desc[f].pair0 = (long long)o;
        o += (size_t)in[f]->n_pairs;
    }
}

// one candidate into the staging block: the rest of its descriptor, its pairs interleaved at pair0 of hp, huv, hw
inline void pack_sim3(const vba_sim3_problem* P, Sim3Desc& d, double* hp, double* huv, double* hw) {
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
}

// flag, cc: the call's flag and chi2 regions as they came back (cc is read only where the caller gave an array)
inline void unpack_sim3(vba_sim3_problem* P, vba_sim3_result* R, const Sim3Desc& d, const Sim3Out& r, const unsigned char* flag, const double* cc) {
    const size_t o = (size_t)d.pair0, n = (size_t)d.n_pairs;
    R->n_inliers = r.n_inliers; R->status = r.status; R->n_bad_stage1 = r.n_bad1;
    for (int k = 0; k < 2; k++) { R->its_done[k] = r.its[k]; R->chi2_stage[k] = r.chi2_stage[k]; }
    std::memcpy(P->S12, r.S, sizeof r.S);   // the input, bit for bit, when the candidate is rejected (:4755)
    if (n) std::memcpy(R->outlier, flag + o, n);
    for (size_t i = 0; i < n && R->chi2_12; i++) R->chi2_12[i] = cc[2 * (o + i)];
    for (size_t i = 0; i < n && R->chi2_21; i++) R->chi2_21[i] = cc[2 * (o + i) + 1];
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct Sim3Call {
    int n = 0;
    size_t n_tot = 0;
    bool want_chi2 = false;
    Sim3Arena A = Sim3Arena(0, 0);
    int prepare(int n_problems, const vba_sim3_problem* const* in, const vba_sim3_result* const* out, std::string& err) {
        n = n_problems;
        if (check_sim3(n, in, out, n_tot, want_chi2, err)) return 1;
        A = Sim3Arena((size_t)n, n_tot);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.download_bytes(want_chi2); }
    size_t grid() const { return (size_t)n; }   // k_sim3_opt: one workgroup per candidate
    Sim3Desc* desc(void* hin) const { return at<Sim3Desc>(hin, A.desc); }
    void describe(const vba_sim3_problem* const* in, void* hin) const { describe_sim3(n, in, desc(hin)); }
    const char* pack(int f, const vba_sim3_problem* P, void* hin) const {
        pack_sim3(P, desc(hin)[f], at<double>(hin, A.p), at<double>(hin, A.uv), at<double>(hin, A.w));
        return nullptr;
    }
    Sim3Batch bind(void* base) const {
        Sim3Batch B;
        B.desc = desc(base); B.out = at<Sim3Out>(base, A.out); B.p = at<double>(base, A.p); B.uv = at<double>(base, A.uv);
        B.w = at<double>(base, A.w); B.c = at<double>(base, A.c); B.flag = at<unsigned char>(base, A.flag);
        return B;
    }
    void unpack(int f, vba_sim3_problem* P, vba_sim3_result* R, void* hin, void* hout) const {
        unpack_sim3(P, R, desc(hin)[f], at<Sim3Out>(hout, A.L.in_back(A.out))[f], at<unsigned char>(hout, A.L.in_back(A.flag)),
                    at<double>(hout, A.L.in_back(A.c)));
    }
};

}  // namespace vba_host
