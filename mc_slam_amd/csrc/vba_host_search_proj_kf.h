// vba_host_search_proj_kf.h -- host half of vba_search_by_projection_kf (plain C++17, no HIP): which problems are refused, the arena
// of a call, the packing of the query records into the staging block, and the write-back, which replays the reference's apply loop
// in query order (replay_matches, vba_host_orient.h): the vpMatched / mvpMapPoints writes (key_match), nmatches and, in reloc mode,
// the rotation histogram, ComputeThreeMaxima and the drop.  The records are those of vba_search_by_projection (SpDesc, SpQuery,
// FuKey), and so are the common checks, the upload half of the arena, the descriptor walk and the common packing
// (vba_host_search_proj.h); this file keeps the mode logic, the fields and the messages of its own.  Included by vislam_ba.hip
// (vba_host_small.h) and by the sanitizer harness tests/host_search_proj_kf_check.cpp (g++ -fsanitize=address,undefined,
// tests/test_host_search_proj_kf.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_host_keygrid.h"
#include "vba_host_search_proj.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace vba_host {

static_assert(VBA_SEARCH_PROJ_KF_MAX_KEYS == VBA_SP_MAX_KEYS, "the header's limit is the kernel's");

// 0: every problem is usable; otherwise err says which is not and why.  The totals are those of vba_search_by_projection
inline int check_search_proj_kf(int n, const vba_search_proj_kf_problem* const* in, const vba_search_proj_kf_result* const* out, SearchProjTotals& T,
                                std::string& err) {
    T = SearchProjTotals();
    std::vector<unsigned char> seen;
    std::string why;
    for (int f = 0; f < n; f++) {
        const vba_search_proj_kf_problem* P = in[f];
        const vba_search_proj_kf_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "problem " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->mode != VBA_SEARCH_PROJ_KF_LOOP && P->mode != VBA_SEARCH_PROJ_KF_RELOC) return fail("unknown mode");
        const bool reloc = P->mode == VBA_SEARCH_PROJ_KF_RELOC;
        const bool ori = reloc && P->check_orientation;
        if (!(why = sp_sizes_fault(*P, "target")).empty()) return fail(why);
        if (P->th_dist < 0 || P->th_dist > 256) return fail("th_dist outside 0 .. 256");
        if (!(why = sp_key_arrays_fault(*P, *R, ori)).empty()) return fail(why);
        if (P->n_q > 0 && (!P->q_pos || !P->q_desc || !P->q_skip || !P->q_dist_min || !P->q_dist_max || !P->q_pred_max || !R->best_idx || !R->best_dist ||
                           !R->level || !R->uv || !R->bin || !R->state))
            return fail("NULL array with n_q > 0");
        if (P->n_q > 0 && !reloc && !P->q_normal) return fail("NULL loop array with n_q > 0");
        if (P->n_q > 0 && ori && !P->q_angle) return fail("NULL reloc array with n_q > 0");
        if (!(why = sp_camera_fault(*P, true)).empty()) return fail(why);
        if (!all_finite(&P->th, 1) || (!reloc && !all_finite(&P->cos_view, 1))) return fail("a threshold is not finite");
        if (!(why = sp_keys_fault(*P, true, ori)).empty()) return fail(why);
        for (size_t i = 0, e = (size_t)P->n_q; i < e; i++) {
            if (!all_finite(P->q_pos + 3 * i, 3)) return fail("query " + std::to_string(i) + ": the position is not finite");
            if (!reloc && !all_finite(P->q_normal + 3 * i, 3)) return fail("query " + std::to_string(i) + ": the normal is not finite");
            if (!all_finite(P->q_dist_min + i, 1) || !all_finite(P->q_dist_max + i, 1) || !all_finite(P->q_pred_max + i, 1))
                return fail("query " + std::to_string(i) + ": a distance is not finite");
            if (ori && !(P->q_angle[i] >= 0.0f && P->q_angle[i] < 360.0f)) return fail("query " + std::to_string(i) + ": angle outside [0, 360)");
        }
        if (!(why = sp_cells_fault(*P, seen, T)).empty()) return fail(why);
    }
    return 0;
}

// behind the upload half, [rounds | best_idx | best_dist | level | uv | state] come back in one copy, [rad | prev] never leave the
// device
struct SearchProjKfArena : SpUploadArena {
    size_t rounds, best_idx, best_dist, level, uv, state, rad, prev;
    SearchProjKfArena(size_t n, const SearchProjTotals& T) : SpUploadArena(n, T) {
        rounds = L.take((n + 1) * 4); best_idx = L.take((T.qs + 1) * 4); best_dist = L.take((T.qs + 1) * 2);
        level = L.take(T.qs + 1); uv = L.take((T.qs + 1) * 16); state = L.take(T.qs + 1);
        L.end_back();
        rad = L.take((T.qs + 1) * 8); prev = L.take((T.qs + 1) * 4);
    }
};

// one problem into the staging block: the rest of its descriptor, its records, its copy of the grid, its scale table.  What a mode
// does not read is packed as zero; every query blocks
inline void pack_search_proj_kf(const vba_search_proj_kf_problem* P, SpDesc& d, const SpUploadArena& A, void* hin) {
    const bool reloc = P->mode == VBA_SEARCH_PROJ_KF_RELOC;
    pack_sp_common(*P, reloc ? 1 : 0, d, A, hin);
    d.th_high = P->th_dist; d.nn_ratio = 0.0f;
    std::memcpy(d.c + 12, P->Ow, 24);
    d.c[25] = P->log_scale_factor; d.c[27] = reloc ? 0.0 : P->cos_view;
    SpQuery* q = at<SpQuery>(hin, A.query) + (size_t)d.q0;
    for (size_t i = 0, e = (size_t)P->n_q; i < e; i++) {
        std::memset(&q[i], 0, sizeof q[i]);
        std::memcpy(q[i].d, P->q_desc + 32 * i, 32);
        std::memcpy(q[i].pos, P->q_pos + 3 * i, 24);
        if (!reloc) std::memcpy(q[i].normal, P->q_normal + 3 * i, 24);
        q[i].dist_min = P->q_dist_min[i]; q[i].dist_max = P->q_dist_max[i]; q[i].pred_max = P->q_pred_max[i];
        q[i].skip = P->q_skip[i] ? 1 : 0;
        q[i].blocks = 1;
    }
}

// The call's back regions as they came back, then the apply loop of the reference replayed in query order (:468-469, :1754-1768) and,
// in reloc mode, the orientation filter (:1775-1794; the bin :1760-1765).  Every match blocks, so a keypoint is written by one query
// at most; a dropped bin clears the keypoint of each of its entries, and its queries leave with state 7
inline void unpack_search_proj_kf(const vba_search_proj_kf_problem* P, vba_search_proj_kf_result* R, const SpDesc& d, int rounds, const int32_t* best_idx,
                                  const uint16_t* best_dist, const int8_t* level, const double* uv, const unsigned char* state) {
    const size_t o = (size_t)d.q0, n = (size_t)d.n_q, nk = (size_t)d.n_keys;
    R->status = VBA_OK;
    R->rounds = rounds;
    for (size_t k = 0; k < nk; k++) R->key_match[k] = -1;
    if (n) {
        std::memcpy(R->best_idx, best_idx + o, 4 * n);
        std::memcpy(R->best_dist, best_dist + o, 2 * n);
        std::memcpy(R->level, level + o, n);
        std::memcpy(R->uv, uv + 2 * o, 16 * n);
        std::memcpy(R->state, state + o, n);
    }
    replay_matches(R, n, nk, P->mode == VBA_SEARCH_PROJ_KF_RELOC && P->check_orientation, P->q_angle, P->angle, 7,
                   [R](size_t i, int32_t b) { R->key_match[b] = (int32_t)i; },
                   [R](size_t i) { R->key_match[R->best_idx[i]] = -2; });   // :1789
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers: k_search_proj_kf takes
// SpBatch and never touches best_dist2 and view_cos, which have no region here and stay null
struct SearchProjKfCall {
    int n = 0;
    SearchProjTotals T;
    SearchProjKfArena A = SearchProjKfArena(0, SearchProjTotals());
    int prepare(int n_problems, const vba_search_proj_kf_problem* const* in, const vba_search_proj_kf_result* const* out, std::string& err) {
        n = n_problems;
        if (check_search_proj_kf(n, in, out, T, err)) return 1;
        A = SearchProjKfArena((size_t)n, T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return (size_t)n; }                   // k_search_proj_kf: one workgroup per problem
    size_t lds_bytes() const { return 4 * (T.max_keys + 1); }   // the claim table of the largest target
    SpDesc* desc(void* hin) const { return at<SpDesc>(hin, A.desc); }
    void describe(const vba_search_proj_kf_problem* const* in, void* hin) const { describe_sp(n, in, desc(hin)); }
    const char* pack(int f, const vba_search_proj_kf_problem* P, void* hin) const {
        pack_search_proj_kf(P, desc(hin)[f], A, hin);
        return nullptr;
    }
    SpBatch bind(void* base) const {
        SpBatch B;
        bind_sp_upload(B, A, base);
        B.rounds = at<int>(base, A.rounds); B.best_idx = at<int>(base, A.best_idx); B.best_dist = at<unsigned short>(base, A.best_dist);
        B.best_dist2 = nullptr; B.level = at<signed char>(base, A.level); B.view_cos = nullptr;
        B.uv = at<double>(base, A.uv); B.state = at<unsigned char>(base, A.state); B.rad = at<double>(base, A.rad); B.prev = at<int>(base, A.prev);
        return B;
    }
    void unpack(int f, vba_search_proj_kf_problem* P, vba_search_proj_kf_result* R, void* hin, void* hout) const {
        auto back = [&](size_t off) { return A.L.in_back(off); };
        unpack_search_proj_kf(P, R, desc(hin)[f], at<int32_t>(hout, back(A.rounds))[f], at<int32_t>(hout, back(A.best_idx)), at<uint16_t>(hout, back(A.best_dist)),
                              at<int8_t>(hout, back(A.level)), at<double>(hout, back(A.uv)), at<unsigned char>(hout, back(A.state)));
    }
};

}  // namespace vba_host
