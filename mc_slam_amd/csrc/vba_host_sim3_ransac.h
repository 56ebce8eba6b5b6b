// vba_host_sim3_ransac.h -- host half of vba_sim3_ransac (plain C++17, no HIP): which candidates are refused, the arena of a call,
// the descriptor of a candidate and its packing into the staging block, the write-back.  Included by vislam_ba.hip
// (vba_host_small.h) and by the sanitizer harness tests/host_sim3_ransac_check.cpp (g++ -fsanitize=address,undefined,
// tests/test_host_sim3_ransac.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>

namespace vba_host {

// 0: every candidate is usable; otherwise err says which is not and why.  n_tot / h_tot: pairs and hypotheses of the call;
// want_counts: a caller asked for the inlier count of every hypothesis
inline int check_sim3_ransac(int n, const vba_sim3_ransac_problem* const* in, const vba_sim3_ransac_result* const* out, size_t& n_tot,
                             size_t& h_tot, bool& want_counts, std::string& err) {
    n_tot = h_tot = 0;
    want_counts = false;
    for (int f = 0; f < n; f++) {
        const vba_sim3_ransac_problem* P = in[f];
        const vba_sim3_ransac_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "problem " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->n_pairs < 0) return fail("negative n_pairs");
        if (P->n_hyp < 0) return fail("negative n_hyp");
        if (P->min_inliers < 0) return fail("negative min_inliers");
        if (P->best_inliers < 0) return fail("negative best_inliers");
        if (P->n_pairs > 0 && (!P->p1c || !P->p2c || !P->max_err1 || !P->max_err2 || !R->inlier)) return fail("NULL array with n_pairs > 0");
        if (P->n_hyp > 0 && !P->sample) return fail("NULL sample with n_hyp > 0");
        if (P->n_hyp > 0 && P->n_pairs < 3) return fail("n_pairs < 3 with n_hyp > 0");
        for (int k = 0; k < 4; k++)
            if (!std::isfinite(P->K1[k]) || !std::isfinite(P->K2[k])) return fail("K1 / K2 is not finite");
        for (size_t i = 0, e = 3 * (size_t)P->n_pairs; i < e; i++)
            if (!std::isfinite(P->p1c[i]) || !std::isfinite(P->p2c[i])) return fail("pair " + std::to_string(i / 3) + ": a point is not finite");
        for (size_t i = 0, e = (size_t)P->n_pairs; i < e; i++)
            if (!std::isfinite(P->max_err1[i]) || !std::isfinite(P->max_err2[i])) return fail("pair " + std::to_string(i) + ": a gate is not finite");
        for (size_t i = 0, e = 3 * (size_t)P->n_hyp; i < e; i++)
            if (P->sample[i] < 0 || P->sample[i] >= P->n_pairs) return fail("hypothesis " + std::to_string(i / 3) + ": sample index out of range");
        n_tot += (size_t)P->n_pairs;
        h_tot += (size_t)P->n_hyp;
        want_counts = want_counts || R->hyp_inliers;
    }
    return 0;
}

// [desc | p | gate | sample] go up in one copy, [out | flag | cnt] come back in one -- cnt, the inlier count of every hypothesis,
// only when a caller asked for it -- and hyp, the hypothesis records, never leaves the device.  Per-pair arrays with the two sides
// of a pair interleaved: p [6] = P1c P2c, gate [2] = max_err1 max_err2; sample [3] per hypothesis
struct RansacArena {
    ArenaLayout L;
    size_t desc, p, gate, sample, out, flag, cnt, hyp;
    RansacArena(size_t n, size_t n_tot, size_t h_tot) {
        desc = L.take(sizeof(RansacDesc) * n); p = L.take((6 * n_tot + 6) * 8); gate = L.take((2 * n_tot + 2) * 8); sample = L.take((3 * h_tot + 3) * 4);
        L.end_upload();
        out = L.take(sizeof(RansacOut) * n); flag = L.take(n_tot + 1); cnt = L.take((h_tot + 1) * 4);
        L.end_back();
        hyp = L.take((h_tot + 1) * VBA_RANSAC_HYP * 8);
    }
    size_t download_bytes(bool want_counts) const { return want_counts ? L.back_bytes() : L.in_back(cnt); }
};

// offsets of every candidate's pairs and hypotheses in the concatenated arrays (the rest of a descriptor comes with the packing)
inline void describe_sim3_ransac(int n, const vba_sim3_ransac_problem* const* in, RansacDesc* desc) {
    size_t o = 0, oh = 0;
    for (int f = 0; f < n; f++) {
        desc[f].pair0 = (long long)o;
        desc[f].hyp0 = (long long)oh;
        o += (size_t)in[f]->n_pairs;
        oh += (size_t)in[f]->n_hyp;
    }
}

// one candidate into the staging block: the rest of its descriptor, its pairs interleaved at pair0 of hp, hg, its triples at hyp0
inline void pack_sim3_ransac(const vba_sim3_ransac_problem* P, RansacDesc& d, double* hp, double* hg, int32_t* hs) {
    d.n_pairs = P->n_pairs;
    d.fix_scale = P->fix_scale ? 1 : 0;
    d.min_inliers = P->min_inliers;
    d.n_hyp = P->n_hyp;
    d.best_inliers = P->best_inliers;
    d.pad = 0;
    std::memcpy(d.K1, P->K1, sizeof d.K1);
    std::memcpy(d.K2, P->K2, sizeof d.K2);
    const size_t o = (size_t)d.pair0, n = (size_t)d.n_pairs;
    double *qp = hp + 6 * o, *qg = hg + 2 * o;
    for (size_t i = 0; i < n; i++) {
        for (int k = 0; k < 3; k++) { qp[6 * i + k] = P->p1c[3 * i + k]; qp[6 * i + 3 + k] = P->p2c[3 * i + k]; }
        qg[2 * i] = P->max_err1[i];
        qg[2 * i + 1] = P->max_err2[i];
    }
    if (d.n_hyp) std::memcpy(hs + 3 * (size_t)d.hyp0, P->sample, 12 * (size_t)d.n_hyp);
}

// flag, cnt: the call's flag and count regions as they came back (cnt is read only where the caller gave an array)
inline void unpack_sim3_ransac(vba_sim3_ransac_problem* P, vba_sim3_ransac_result* R, const RansacDesc& d, const RansacOut& r,
                               const unsigned char* flag, const int32_t* cnt) {
    const size_t n = (size_t)d.n_pairs, nh = (size_t)d.n_hyp;
    R->status = r.status; R->hit = r.hit; R->its_done = r.its_done; R->best_hyp = r.best_hyp; R->n_inliers = r.n_inliers;
    P->best_inliers = r.best_inliers;
    if (r.best_hyp >= 0) std::memcpy(P->best_S12, r.best_S, sizeof r.best_S);
    if (r.hit >= 0) {
        std::memcpy(R->S12, r.S, sizeof r.S);
        if (n) std::memcpy(R->inlier, flag + (size_t)d.pair0, n);
    }
    if (R->hyp_inliers && nh) std::memcpy(R->hyp_inliers, cnt + (size_t)d.hyp0, 4 * nh);
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct RansacCall {
    int n = 0;
    size_t n_tot = 0, h_tot = 0;
    bool want_counts = false;
    RansacArena A = RansacArena(0, 0, 0);
    int prepare(int n_problems, const vba_sim3_ransac_problem* const* in, const vba_sim3_ransac_result* const* out, std::string& err) {
        n = n_problems;
        if (check_sim3_ransac(n, in, out, n_tot, h_tot, want_counts, err)) return 1;
        A = RansacArena((size_t)n, n_tot, h_tot);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.download_bytes(want_counts); }
    size_t grid() const { return (size_t)n; }   // k_sim3_ransac: one workgroup per candidate
    RansacDesc* desc(void* hin) const { return at<RansacDesc>(hin, A.desc); }
    void describe(const vba_sim3_ransac_problem* const* in, void* hin) const { describe_sim3_ransac(n, in, desc(hin)); }
    const char* pack(int f, const vba_sim3_ransac_problem* P, void* hin) const {
        pack_sim3_ransac(P, desc(hin)[f], at<double>(hin, A.p), at<double>(hin, A.gate), at<int32_t>(hin, A.sample));
        return nullptr;
    }
    RansacBatch bind(void* base) const {
        RansacBatch B;
        B.desc = desc(base); B.out = at<RansacOut>(base, A.out); B.p = at<double>(base, A.p); B.gate = at<double>(base, A.gate);
        B.sample = at<int>(base, A.sample); B.hyp = at<double>(base, A.hyp); B.cnt = at<int>(base, A.cnt); B.flag = at<unsigned char>(base, A.flag);
        return B;
    }
    void unpack(int f, vba_sim3_ransac_problem* P, vba_sim3_ransac_result* R, void* hin, void* hout) const {
        unpack_sim3_ransac(P, R, desc(hin)[f], at<RansacOut>(hout, A.L.in_back(A.out))[f], at<unsigned char>(hout, A.L.in_back(A.flag)),
                           at<int32_t>(hout, A.L.in_back(A.cnt)));
    }
};

}  // namespace vba_host
