// vba_host_triangulate.h -- host half of vba_triangulate (plain C++17, no HIP): which pairs are refused, the arena of a call, the
// descriptor of a pair and the block-to-pair map, the packing into the staging block, the write-back.  Included by vislam_ba.hip
// (vba_host_small.h) and by the sanitizer harness tests/host_triangulate_check.cpp (g++ -fsanitize=address,undefined,
// tests/test_host_triangulate.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>

namespace vba_host {

// 0: every pair is usable; otherwise err says which is not and why.  n_tot: matches of the call, l_tot: doubles of all level
// tables, n_blocks: workgroups (VBA_TRI_NT matches of ONE pair each; a pair without matches gets none)
inline int check_triangulate(int n, const vba_triangulate_problem* const* in, const vba_triangulate_result* const* out, size_t& n_tot,
                             size_t& l_tot, size_t& n_blocks, std::string& err) {
    n_tot = l_tot = n_blocks = 0;
    for (int f = 0; f < n; f++) {
        const vba_triangulate_problem* P = in[f];
        const vba_triangulate_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "pair " + std::to_string(f) + ": " + m; return 1; };
        auto finite = [](const double* a, int k) { for (int i = 0; i < k; i++) if (!std::isfinite(a[i])) return false; return true; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->n_matches < 0) return fail("negative n_matches");
        if (P->n_levels1 < 1 || P->n_levels1 > VBA_TRI_LEVELS || P->n_levels2 < 1 || P->n_levels2 > VBA_TRI_LEVELS) return fail("n_levels outside 1 .. 64");
        if (!P->level_sigma2_1 || !P->scale_1 || !P->level_sigma2_2 || !P->scale_2) return fail("NULL level table");
        if (P->n_matches > 0 && (!P->uv1 || !P->uv2 || !P->oct1 || !P->oct2 || !R->x3d || !R->reason)) return fail("NULL array with n_matches > 0");
        if (!finite(P->Rcw1, 9) || !finite(P->tcw1, 3) || !finite(P->Ow1, 3) || !finite(P->Rcw2, 9) || !finite(P->tcw2, 3) || !finite(P->Ow2, 3))
            return fail("a pose is not finite");
        if (!finite(P->K1, 4) || !finite(P->K2, 4)) return fail("K1 / K2 is not finite");
        if (P->K1[0] == 0.0 || P->K1[1] == 0.0 || P->K2[0] == 0.0 || P->K2[1] == 0.0) return fail("zero fx / fy");
        if (!finite(&P->ratio_factor, 1) || !finite(&P->cos_max, 1) || !finite(&P->chi2_th, 1)) return fail("a threshold is not finite");
        if (!finite(P->level_sigma2_1, P->n_levels1) || !finite(P->scale_1, P->n_levels1) || !finite(P->level_sigma2_2, P->n_levels2) ||
            !finite(P->scale_2, P->n_levels2))
            return fail("a level table is not finite");
        for (int l = 0; l < P->n_levels1; l++)
            if (!(P->scale_1[l] > 0.0)) return fail("level " + std::to_string(l) + ": scale <= 0");
        for (int l = 0; l < P->n_levels2; l++)
            if (!(P->scale_2[l] > 0.0)) return fail("level " + std::to_string(l) + ": scale <= 0");
        for (size_t i = 0, e = (size_t)P->n_matches; i < e; i++) {
            if (!finite(P->uv1 + 2 * i, 2) || !finite(P->uv2 + 2 * i, 2)) return fail("match " + std::to_string(i) + ": a pixel is not finite");
            if (P->oct1[i] >= P->n_levels1 || P->oct2[i] >= P->n_levels2) return fail("match " + std::to_string(i) + ": octave >= n_levels");
        }
        n_tot += (size_t)P->n_matches;
        l_tot += 2 * ((size_t)P->n_levels1 + (size_t)P->n_levels2);
        n_blocks += ((size_t)P->n_matches + VBA_TRI_NT - 1) / VBA_TRI_NT;
    }
    if (n_blocks > 0x7fffffffu) { err = "more than 2^31 - 1 workgroups"; return 1; }
    return 0;
}

// [desc | blk | lev | uv | oct] go up in one copy, [x3d | reason] come back in one.  Per-match arrays with the two sides of a match
// interleaved: uv [4] = u1 v1 u2 v2 (32 bytes, 16-byte loads), oct [2] = octave 1, octave 2
struct TriArena {
    ArenaLayout L;
    size_t desc, blk, lev, uv, oct, x3d, reason;
    TriArena(size_t n, size_t n_tot, size_t l_tot, size_t n_blocks) {
        desc = L.take(sizeof(TriDesc) * n); blk = L.take(sizeof(TriBlock) * (n_blocks + 1)); lev = L.take((l_tot + 1) * 8);
        uv = L.take((4 * n_tot + 4) * 8); oct = L.take(2 * n_tot + 2);
        L.end_upload();
        x3d = L.take((3 * n_tot + 3) * 8); reason = L.take(n_tot + 1);
        L.end_back();
    }
};

// offsets of every pair's matches and level tables in the concatenated arrays, and the block-to-pair map: the workgroups of a pair
// follow each other, pairs in the caller's order, a pair without matches has none (the rest of a descriptor comes with the packing)
inline void describe_triangulate(int n, const vba_triangulate_problem* const* in, TriDesc* desc, TriBlock* blk) {
    size_t o = 0, ol = 0, b = 0;
    for (int f = 0; f < n; f++) {
        desc[f].match0 = (long long)o;
        desc[f].lev0 = (long long)ol;
        for (int first = 0; first < in[f]->n_matches; first += VBA_TRI_NT) { blk[b].pair = f; blk[b].first = first; b++; }
        o += (size_t)in[f]->n_matches;
        ol += 2 * ((size_t)in[f]->n_levels1 + (size_t)in[f]->n_levels2);
    }
}

// one pair into the staging block: the rest of its descriptor, its level tables at lev0 of hl, its matches interleaved at match0
inline void pack_triangulate(const vba_triangulate_problem* P, TriDesc& d, double* hl, double* huv, unsigned char* hoct) {
    d.n_matches = P->n_matches;
    d.n_levels1 = P->n_levels1;
    d.n_levels2 = P->n_levels2;
    d.pad = 0;
    double* c = d.c;
    std::memcpy(c, P->Rcw1, 72); std::memcpy(c + 9, P->tcw1, 24); std::memcpy(c + 12, P->Ow1, 24); std::memcpy(c + 15, P->K1, 32);
    std::memcpy(c + 19, P->Rcw2, 72); std::memcpy(c + 28, P->tcw2, 24); std::memcpy(c + 31, P->Ow2, 24); std::memcpy(c + 34, P->K2, 32);
    c[38] = P->ratio_factor; c[39] = P->cos_max; c[40] = P->chi2_th;
    double* ql = hl + (size_t)d.lev0;
    const size_t n1 = (size_t)d.n_levels1, n2 = (size_t)d.n_levels2;
    std::memcpy(ql, P->level_sigma2_1, 8 * n1); std::memcpy(ql + n1, P->scale_1, 8 * n1);
    std::memcpy(ql + 2 * n1, P->level_sigma2_2, 8 * n2); std::memcpy(ql + 2 * n1 + n2, P->scale_2, 8 * n2);
    const size_t o = (size_t)d.match0, n = (size_t)d.n_matches;
    double* q = huv + 4 * o;
    unsigned char* qo = hoct + 2 * o;
    for (size_t i = 0; i < n; i++) {
        q[4 * i] = P->uv1[2 * i]; q[4 * i + 1] = P->uv1[2 * i + 1]; q[4 * i + 2] = P->uv2[2 * i]; q[4 * i + 3] = P->uv2[2 * i + 1];
        qo[2 * i] = P->oct1[i]; qo[2 * i + 1] = P->oct2[i];
    }
}

// x3d, reason: the call's regions as they came back (NULL when the call had no match at all)
inline void unpack_triangulate(vba_triangulate_result* R, const TriDesc& d, const double* x3d, const unsigned char* reason) {
    const size_t o = (size_t)d.match0, n = (size_t)d.n_matches;
    int acc = 0;
    if (n) {
        std::memcpy(R->x3d, x3d + 3 * o, 24 * n);
        std::memcpy(R->reason, reason + o, n);
        for (size_t i = 0; i < n; i++) acc += reason[o + i] == 0;
    }
    R->status = VBA_OK;
    R->n_accepted = acc;
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct TriCall {
    int n = 0;
    size_t n_tot = 0, l_tot = 0, n_blocks = 0;
    TriArena A = TriArena(0, 0, 0, 0);
    int prepare(int n_pairs, const vba_triangulate_problem* const* in, const vba_triangulate_result* const* out, std::string& err) {
        n = n_pairs;
        if (check_triangulate(n, in, out, n_tot, l_tot, n_blocks, err)) return 1;
        A = TriArena((size_t)n, n_tot, l_tot, n_blocks);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return n_blocks; }   // k_triangulate: one lane per match; a call without a single match launches nothing
    TriDesc* desc(void* hin) const { return at<TriDesc>(hin, A.desc); }
    void describe(const vba_triangulate_problem* const* in, void* hin) const { describe_triangulate(n, in, desc(hin), at<TriBlock>(hin, A.blk)); }
    const char* pack(int f, const vba_triangulate_problem* P, void* hin) const {
        pack_triangulate(P, desc(hin)[f], at<double>(hin, A.lev), at<double>(hin, A.uv), at<unsigned char>(hin, A.oct));
        return nullptr;
    }
    TriBatch bind(void* base) const {
        TriBatch B;
        B.desc = desc(base); B.blk = at<TriBlock>(base, A.blk); B.lev = at<double>(base, A.lev); B.uv = at<double>(base, A.uv);
        B.oct = at<unsigned char>(base, A.oct); B.x3d = at<double>(base, A.x3d); B.reason = at<unsigned char>(base, A.reason);
        return B;
    }
    void unpack(int f, vba_triangulate_problem*, vba_triangulate_result* R, void* hin, void* hout) const {
        unpack_triangulate(R, desc(hin)[f], at<double>(hout, A.L.in_back(A.x3d)), at<unsigned char>(hout, A.L.in_back(A.reason)));
    }
};

}  // namespace vba_host
