// vba_host_search_proj_kf.h -- host half of vba_search_by_projection_kf (plain C++17, no HIP): which problems are refused, the arena
// of a call, the descriptor of a problem, the packing of the keypoint and query records and of the grid copy into the staging
// block, and the write-back, which replays the reference's apply loop in query order: the vpMatched / mvpMapPoints writes
// (key_match), nmatches and, in reloc mode, the rotation histogram, ComputeThreeMaxima and the drop.  The records are those of
// vba_search_by_projection (SpDesc, SpQuery, FuKey); three_maxima and rot_bin are its too.  Included by vislam_ba.hip
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

static_assert(VBA_SEARCH_PROJ_KF_MAX_KEYS == VBA_SK_MAX_KEYS, "the header's limit is the kernel's");

// 0: every problem is usable; otherwise err says which is not and why.  The totals are those of vba_search_by_projection
inline int check_search_proj_kf(int n, const vba_search_proj_kf_problem* const* in, const vba_search_proj_kf_result* const* out, SearchProjTotals& T,
                                std::string& err) {
    T = SearchProjTotals();
    std::vector<unsigned char> seen;
    for (int f = 0; f < n; f++) {
        const vba_search_proj_kf_problem* P = in[f];
        const vba_search_proj_kf_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "problem " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->mode != VBA_SEARCH_PROJ_KF_LOOP && P->mode != VBA_SEARCH_PROJ_KF_RELOC) return fail("unknown mode");
        const bool reloc = P->mode == VBA_SEARCH_PROJ_KF_RELOC;
        const bool ori = reloc && P->check_orientation;
        if (P->n_keys < 0) return fail("negative n_keys");
        if (P->n_keys > VBA_SK_MAX_KEYS) return fail("n_keys above 16384: the claim table of a target lives in LDS");
        if (P->n_q < 0) return fail("negative n_q");
        if (P->n_levels < 1 || P->n_levels > VBA_TRI_LEVELS) return fail("n_levels outside 1 .. 64");
        if (!P->scale) return fail("NULL level table");
        if (P->th_dist < 0 || P->th_dist > 256) return fail("th_dist outside 0 .. 256");
        if (!grid_size_ok(*P)) return fail("grid size outside 1 .. 65536 cells");
        if (P->n_keys > 0 && (!P->desc || !P->uv || !P->oct || !P->occupied || !R->key_match || (ori && !P->angle))) return fail("NULL array with n_keys > 0");
        if (P->n_q > 0 && (!P->q_pos || !P->q_desc || !P->q_skip || !P->q_dist_min || !P->q_dist_max || !P->q_pred_max || !R->best_idx || !R->best_dist ||
                           !R->level || !R->uv || !R->bin || !R->state))
            return fail("NULL array with n_q > 0");
        if (P->n_q > 0 && !reloc && !P->q_normal) return fail("NULL loop array with n_q > 0");
        if (P->n_q > 0 && ori && !P->q_angle) return fail("NULL reloc array with n_q > 0");
        if (!P->cell_begin) return fail("NULL cell_begin");
        if (!all_finite(P->Rcw, 9) || !all_finite(P->tcw, 3) || !all_finite(P->Ow, 3)) return fail("the pose is not finite");
        if (!all_finite(P->K, 4)) return fail("an intrinsic is not finite");
        if (!all_finite(P->bounds, 4) || !all_finite(&P->grid_inv_w, 1) || !all_finite(&P->grid_inv_h, 1)) return fail("a bound or cell size is not finite");
        if (!all_finite(&P->th, 1) || (!reloc && !all_finite(&P->cos_view, 1))) return fail("a threshold is not finite");
        if (!all_finite(P->scale, (size_t)P->n_levels) || !all_finite(&P->log_scale_factor, 1)) return fail("a level table is not finite");
        for (size_t i = 0, e = (size_t)P->n_keys; i < e; i++) {
            if (const char* why = keypoint_fault(*P, i)) return fail("keypoint " + std::to_string(i) + ": " + why);
            if (ori && !(P->angle[i] >= 0.0f && P->angle[i] < 360.0f)) return fail("keypoint " + std::to_string(i) + ": angle outside [0, 360)");
        }
        for (size_t i = 0, e = (size_t)P->n_q; i < e; i++) {
            if (!all_finite(P->q_pos + 3 * i, 3)) return fail("query " + std::to_string(i) + ": the position is not finite");
            if (!reloc && !all_finite(P->q_normal + 3 * i, 3)) return fail("query " + std::to_string(i) + ": the normal is not finite");
            if (!all_finite(P->q_dist_min + i, 1) || !all_finite(P->q_dist_max + i, 1) || !all_finite(P->q_pred_max + i, 1))
                return fail("query " + std::to_string(i) + ": a distance is not finite");
            if (ori && !(P->q_angle[i] >= 0.0f && P->q_angle[i] < 360.0f)) return fail("query " + std::to_string(i) + ": angle outside [0, 360)");
        }
        int nf = 0;
        const std::string why = check_cell_lists(P->grid_cols, P->grid_rows, P->n_keys, P->cell_begin, P->cell_feat, seen, nf);
        if (!why.empty()) return fail(why);
        T.keys += (size_t)P->n_keys; T.qs += (size_t)P->n_q;
        T.cells += grid_cells(*P) + 1; T.feat += (size_t)nf; T.lev += (size_t)P->n_levels;
        if ((size_t)P->n_keys > T.max_keys) T.max_keys = (size_t)P->n_keys;
    }
    return 0;
}

// [desc | key | occupied | query | cell | feat | lev] go up in one copy, [rounds | best_idx | best_dist | level | uv | state] come back
// in one, [rad | prev] never leave the device
struct SearchProjKfArena {
    ArenaLayout L;
    size_t desc, key, occupied, query, cell, feat, lev, rounds, best_idx, best_dist, level, uv, state, rad, prev;
    SearchProjKfArena(size_t n, const SearchProjTotals& T) {
        desc = L.take(sizeof(SpDesc) * n); key = L.take(sizeof(FuKey) * (T.keys + 1)); occupied = L.take(T.keys + 1);
        query = L.take(sizeof(SpQuery) * (T.qs + 1)); cell = L.take((T.cells + 1) * 4); feat = L.take((T.feat + 1) * 4); lev = L.take((T.lev + 1) * 8);
        L.end_upload();
        rounds = L.take((n + 1) * 4); best_idx = L.take((T.qs + 1) * 4); best_dist = L.take((T.qs + 1) * 2);
        level = L.take(T.qs + 1); uv = L.take((T.qs + 1) * 16); state = L.take(T.qs + 1);
        L.end_back();
        rad = L.take((T.qs + 1) * 8); prev = L.take((T.qs + 1) * 4);
    }
};

// offsets of every problem's regions in the concatenated arrays
inline void describe_search_proj_kf(int n, const vba_search_proj_kf_problem* const* in, SpDesc* desc) {
    size_t k = 0, q = 0, c = 0, ft = 0, lv = 0;
    for (int f = 0; f < n; f++) {
        desc[f].key0 = (long long)k; desc[f].q0 = (long long)q; desc[f].cell0 = (long long)c; desc[f].feat0 = (long long)ft; desc[f].lev0 = (long long)lv;
        k += (size_t)in[f]->n_keys; q += (size_t)in[f]->n_q; c += grid_cells(*in[f]) + 1;
        ft += grid_feat(*in[f]); lv += (size_t)in[f]->n_levels;
    }
}

// one problem into the staging block: the rest of its descriptor, its records, its copy of the grid, its scale table.  What a mode
// does not read is packed as zero; every query blocks
inline void pack_search_proj_kf(const vba_search_proj_kf_problem* P, SpDesc& d, FuKey* hkey, unsigned char* hocc, SpQuery* hq, int32_t* hcell, int32_t* hfeat,
                                double* hlev) {
    const bool reloc = P->mode == VBA_SEARCH_PROJ_KF_RELOC;
    d.n_keys = P->n_keys; d.n_q = P->n_q; d.n_levels = P->n_levels; d.th_high = P->th_dist;
    d.cols = P->grid_cols; d.rows = P->grid_rows; d.mode = reloc ? 1 : 0; d.pad0 = 0;
    d.nn_ratio = 0.0f; d.pad1 = 0;
    std::memcpy(d.c, P->Rcw, 72); std::memcpy(d.c + 9, P->tcw, 24); std::memcpy(d.c + 12, P->Ow, 24);
    std::memcpy(d.c + 15, P->K, 32); std::memcpy(d.c + 19, P->bounds, 32);
    d.c[23] = P->grid_inv_w; d.c[24] = P->grid_inv_h; d.c[25] = P->log_scale_factor; d.c[26] = P->th; d.c[27] = reloc ? 0.0 : P->cos_view;
    pack_keys(*P, hkey + (size_t)d.key0);
    unsigned char* oc = hocc + (size_t)d.key0;
    for (size_t i = 0, e = (size_t)P->n_keys; i < e; i++) oc[i] = P->occupied[i] ? 1 : 0;
    SpQuery* q = hq + (size_t)d.q0;
    for (size_t i = 0, e = (size_t)P->n_q; i < e; i++) {
        std::memset(&q[i], 0, sizeof q[i]);
        std::memcpy(q[i].d, P->q_desc + 32 * i, 32);
        std::memcpy(q[i].pos, P->q_pos + 3 * i, 24);
        if (!reloc) std::memcpy(q[i].normal, P->q_normal + 3 * i, 24);
        q[i].dist_min = P->q_dist_min[i]; q[i].dist_max = P->q_dist_max[i]; q[i].pred_max = P->q_pred_max[i];
        q[i].skip = P->q_skip[i] ? 1 : 0;
        q[i].blocks = 1;
    }
    pack_grid(*P, hcell + (size_t)d.cell0, hfeat + (size_t)d.feat0);
    std::memcpy(hlev + (size_t)d.lev0, P->scale, 8 * (size_t)P->n_levels);
}

// The call's back regions as they came back, then the apply loop of the reference replayed in query order (:468-469, :1754-1768) and,
// in reloc mode, the orientation filter (:1775-1794).  Every match blocks, so a keypoint is written by one query at most; a dropped
// bin clears the keypoint of each of its entries, and its queries leave with state 7
inline void unpack_search_proj_kf(const vba_search_proj_kf_problem* P, vba_search_proj_kf_result* R, const SpDesc& d, int rounds, const int32_t* best_idx,
                                  const uint16_t* best_dist, const int8_t* level, const double* uv, const unsigned char* state) {
    const size_t o = (size_t)d.q0, n = (size_t)d.n_q, nk = (size_t)d.n_keys;
    const bool ori = P->mode == VBA_SEARCH_PROJ_KF_RELOC && P->check_orientation;
    R->status = VBA_OK;
    R->rounds = rounds;
    for (int i = 0; i < VBA_ST_HISTO; i++) R->hist[i] = 0;
    R->ind[0] = R->ind[1] = R->ind[2] = -1;
    for (size_t k = 0; k < nk; k++) R->key_match[k] = -1;
    int nmatches = 0;
    if (n) {
        std::memcpy(R->best_idx, best_idx + o, 4 * n);
        std::memcpy(R->best_dist, best_dist + o, 2 * n);
        std::memcpy(R->level, level + o, n);
        std::memcpy(R->uv, uv + 2 * o, 16 * n);
        std::memcpy(R->state, state + o, n);
    }
    for (size_t i = 0; i < n; i++) {
        R->bin[i] = 255;
        const int32_t b = R->best_idx[i];
        if (R->state[i] != 0 || b < 0 || (size_t)b >= nk) continue;   // a state 0 always brings a keypoint of the target
        R->key_match[b] = (int32_t)i;
        nmatches++;
        if (ori) {
            const int bin = rot_bin(P->q_angle[i], P->angle[b]);     // :1760-1765
            R->bin[i] = (uint8_t)bin;
            R->hist[bin]++;
        }
    }
    R->n_before_filter = nmatches;
    if (ori) {
        three_maxima(R->hist, R->ind);
        for (size_t i = 0; i < n; i++) {
            const int bin = R->bin[i];
            if (bin == 255 || bin == R->ind[0] || bin == R->ind[1] || bin == R->ind[2]) continue;
            R->key_match[R->best_idx[i]] = -2;   // :1789
            R->state[i] = 7;
            nmatches--;
        }
    }
    R->n_matches = nmatches;
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
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
    void describe(const vba_search_proj_kf_problem* const* in, void* hin) const { describe_search_proj_kf(n, in, desc(hin)); }
    const char* pack(int f, const vba_search_proj_kf_problem* P, void* hin) const {
        pack_search_proj_kf(P, desc(hin)[f], at<FuKey>(hin, A.key), at<unsigned char>(hin, A.occupied), at<SpQuery>(hin, A.query), at<int32_t>(hin, A.cell),
                            at<int32_t>(hin, A.feat), at<double>(hin, A.lev));
        return nullptr;
    }
    SkBatch bind(void* base) const {
        SkBatch B;
        B.desc = desc(base); B.key = at<FuKey>(base, A.key); B.occupied = at<unsigned char>(base, A.occupied); B.query = at<SpQuery>(base, A.query);
        B.cell_begin = at<int>(base, A.cell); B.cell_feat = at<int>(base, A.feat); B.lev = at<double>(base, A.lev);
        B.rounds = at<int>(base, A.rounds); B.best_idx = at<int>(base, A.best_idx); B.best_dist = at<unsigned short>(base, A.best_dist);
        B.level = at<signed char>(base, A.level); B.uv = at<double>(base, A.uv); B.state = at<unsigned char>(base, A.state);
        B.rad = at<double>(base, A.rad); B.prev = at<int>(base, A.prev);
        return B;
    }
    void unpack(int f, vba_search_proj_kf_problem* P, vba_search_proj_kf_result* R, void* hin, void* hout) const {
        auto back = [&](size_t off) { return A.L.in_back(off); };
        unpack_search_proj_kf(P, R, desc(hin)[f], at<int32_t>(hout, back(A.rounds))[f], at<int32_t>(hout, back(A.best_idx)), at<uint16_t>(hout, back(A.best_dist)),
                              at<int8_t>(hout, back(A.level)), at<double>(hout, back(A.uv)), at<unsigned char>(hout, back(A.state)));
    }
};

}  // namespace vba_host
