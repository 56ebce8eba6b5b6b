// vba_host_search_proj.h -- host half of vba_search_by_projection (plain C++17, no HIP): which problems are refused, the arena of a
// call, the descriptor of a problem, the packing of the keypoint and query records and of the grid copy into the staging block, and
// the write-back, which replays the reference's apply loop in query order (replay_matches, vba_host_orient.h): the mvpMapPoints
// writes (key_match), nmatches, the rotation histogram, ComputeThreeMaxima and the drop.  The first part is what this half shares
// with vba_search_by_projection_kf (vba_host_search_proj_kf.h): both work over SpDesc, SpQuery and FuKey, and their problem structs
// name the common fields alike, so the shared pieces are templates over the struct.  Included by vislam_ba.hip (vba_host_small.h)
// and by the sanitizer harness tests/host_search_proj_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_search_proj.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_host_keygrid.h"
#include "vba_host_orient.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace vba_host {

// totals of a call: keypoints, queries, entries of all cell_begin and cell_feat copies, doubles of all scale tables; the largest frame
struct SearchProjTotals {
    size_t keys = 0, qs = 0, cells = 0, feat = 0, lev = 0, max_keys = 0;
};

// The checks both halves make: an empty string, or the fault.  They come in five groups, which a half calls between its own checks
// in this order, so that of two faults of a problem the same one is reported as before.  Group 1, the sizes; owner: whose claim
// table lives in LDS
template <class P>
std::string sp_sizes_fault(const P& p, const char* owner) {
    if (p.n_keys < 0) return "negative n_keys";
    if (p.n_keys > VBA_SP_MAX_KEYS) return std::string("n_keys above 16384: the claim table of a ") + owner + " lives in LDS";
    if (p.n_q < 0) return "negative n_q";
    if (p.n_levels < 1 || p.n_levels > VBA_TRI_LEVELS) return "n_levels outside 1 .. 64";
    if (!p.scale) return "NULL level table";
    return "";
}

// group 2: the grid size and the keypoint arrays.  ori: the orientation filter is on
template <class P, class R>
std::string sp_key_arrays_fault(const P& p, const R& r, bool ori) {
    if (!grid_size_ok(p)) return "grid size outside 1 .. 65536 cells";
    if (p.n_keys > 0 && (!p.desc || !p.uv || !p.oct || !p.occupied || !r.key_match || (ori && !p.angle))) return "NULL array with n_keys > 0";
    return "";
}

// group 3: cell_begin, the pose (with Ow where the mode reads it), the intrinsics, the bounds
template <class P>
std::string sp_camera_fault(const P& p, bool with_ow) {
    if (!p.cell_begin) return "NULL cell_begin";
    if (!all_finite(p.Rcw, 9) || !all_finite(p.tcw, 3) || (with_ow && !all_finite(p.Ow, 3))) return "the pose is not finite";
    if (!all_finite(p.K, 4)) return "an intrinsic is not finite";
    if (!all_finite(p.bounds, 4) || !all_finite(&p.grid_inv_w, 1) || !all_finite(&p.grid_inv_h, 1)) return "a bound or cell size is not finite";
    return "";
}

// group 4: the level table (with log_scale_factor where the mode reads it) and the keypoints
template <class P>
std::string sp_keys_fault(const P& p, bool with_logsf, bool ori) {
    if (!all_finite(p.scale, (size_t)p.n_levels) || (with_logsf && !all_finite(&p.log_scale_factor, 1))) return "a level table is not finite";
    for (size_t i = 0, e = (size_t)p.n_keys; i < e; i++) {
        if (const char* why = keypoint_fault(p, i)) return "keypoint " + std::to_string(i) + ": " + why;
        if (ori && !(p.angle[i] >= 0.0f && p.angle[i] < 360.0f)) return "keypoint " + std::to_string(i) + ": angle outside [0, 360)";
    }
    return "";
}

// group 5: the cell lists; a problem that passes is added to the totals.  seen is scratch
template <class P>
std::string sp_cells_fault(const P& p, std::vector<unsigned char>& seen, SearchProjTotals& T) {
    int nf = 0;
    const std::string why = check_cell_lists(p.grid_cols, p.grid_rows, p.n_keys, p.cell_begin, p.cell_feat, seen, nf);
    if (!why.empty()) return why;
    T.keys += (size_t)p.n_keys; T.qs += (size_t)p.n_q;
    T.cells += grid_cells(p) + 1; T.feat += (size_t)nf; T.lev += (size_t)p.n_levels;
    if ((size_t)p.n_keys > T.max_keys) T.max_keys = (size_t)p.n_keys;
    return "";
}

// the upload half of both arenas: [desc | key | occupied | query | cell | feat | lev] go up in one copy
struct SpUploadArena {
    ArenaLayout L;
    size_t desc, key, occupied, query, cell, feat, lev;
    SpUploadArena(size_t n, const SearchProjTotals& T) {
        desc = L.take(sizeof(SpDesc) * n); key = L.take(sizeof(FuKey) * (T.keys + 1)); occupied = L.take(T.keys + 1);
        query = L.take(sizeof(SpQuery) * (T.qs + 1)); cell = L.take((T.cells + 1) * 4); feat = L.take((T.feat + 1) * 4); lev = L.take((T.lev + 1) * 8);
        L.end_upload();
    }
};

// the upload regions of the device block, as the kernels' argument names them: the upload half of bind
inline void bind_sp_upload(SpBatch& B, const SpUploadArena& A, void* base) {
    B.desc = at<SpDesc>(base, A.desc); B.key = at<FuKey>(base, A.key); B.occupied = at<unsigned char>(base, A.occupied); B.query = at<SpQuery>(base, A.query);
    B.cell_begin = at<int>(base, A.cell); B.cell_feat = at<int>(base, A.feat); B.lev = at<double>(base, A.lev);
}

// offsets of every problem's regions in the concatenated arrays
template <class P>
void describe_sp(int n, const P* const* in, SpDesc* desc) {
    size_t k = 0, q = 0, c = 0, ft = 0, lv = 0;
    for (int f = 0; f < n; f++) {
        desc[f].key0 = (long long)k; desc[f].q0 = (long long)q; desc[f].cell0 = (long long)c; desc[f].feat0 = (long long)ft; desc[f].lev0 = (long long)lv;
        k += (size_t)in[f]->n_keys; q += (size_t)in[f]->n_q; c += grid_cells(*in[f]) + 1;
        ft += grid_feat(*in[f]); lv += (size_t)in[f]->n_levels;
    }
}

// What both halves pack alike: the sizes, the grid and the mode, the camera block but Ow, log_scale_factor and cos_view (c[12 .. 14],
// c[25], c[27]), the keypoint records, the occupied flags, the grid copy and the scale table.  A half adds th_high, nn_ratio, the
// three entries of c and its query records
template <class P>
void pack_sp_common(const P& p, int mode, SpDesc& d, const SpUploadArena& A, void* hin) {
    d.n_keys = p.n_keys; d.n_q = p.n_q; d.n_levels = p.n_levels;
    d.cols = p.grid_cols; d.rows = p.grid_rows; d.mode = mode; d.pad0 = 0; d.pad1 = 0;
    std::memcpy(d.c, p.Rcw, 72); std::memcpy(d.c + 9, p.tcw, 24);
    std::memcpy(d.c + 15, p.K, 32); std::memcpy(d.c + 19, p.bounds, 32);
    d.c[23] = p.grid_inv_w; d.c[24] = p.grid_inv_h; d.c[26] = p.th;
    pack_keys(p, at<FuKey>(hin, A.key) + (size_t)d.key0);
    unsigned char* oc = at<unsigned char>(hin, A.occupied) + (size_t)d.key0;
    for (size_t i = 0, e = (size_t)p.n_keys; i < e; i++) oc[i] = p.occupied[i] ? 1 : 0;
    pack_grid(p, at<int32_t>(hin, A.cell) + (size_t)d.cell0, at<int32_t>(hin, A.feat) + (size_t)d.feat0);
    std::memcpy(at<double>(hin, A.lev) + (size_t)d.lev0, p.scale, 8 * (size_t)p.n_levels);
}

// ---- vba_search_by_projection's own

// 0: every problem is usable; otherwise err says which is not and why
inline int check_search_proj(int n, const vba_search_proj_problem* const* in, const vba_search_proj_result* const* out, SearchProjTotals& T,
                             std::string& err) {
    T = SearchProjTotals();
    std::vector<unsigned char> seen;
    std::string why;
    for (int f = 0; f < n; f++) {
        const vba_search_proj_problem* P = in[f];
        const vba_search_proj_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "problem " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->mode != VBA_SEARCH_PROJ_LAST_FRAME && P->mode != VBA_SEARCH_PROJ_LOCAL_MAP) return fail("unknown mode");
        const bool local = P->mode == VBA_SEARCH_PROJ_LOCAL_MAP;
        const bool ori = !local && P->check_orientation;
        if (!(why = sp_sizes_fault(*P, "frame")).empty()) return fail(why);
        if (P->th_high < 0 || P->th_high > 256) return fail("th_high outside 0 .. 256");
        if (!(why = sp_key_arrays_fault(*P, *R, ori)).empty()) return fail(why);
        if (P->n_q > 0 && (!P->q_pos || !P->q_desc || !P->q_skip || !P->q_blocks || !R->best_idx || !R->best_dist || !R->best_dist2 || !R->level ||
                           !R->view_cos || !R->uv || !R->bin || !R->state))
            return fail("NULL array with n_q > 0");
        if (P->n_q > 0 && !local && (!P->q_oct || (ori && !P->q_angle))) return fail("NULL last-frame array with n_q > 0");
        if (P->n_q > 0 && local && (!P->q_normal || !P->q_dist_min || !P->q_dist_max || !P->q_pred_max)) return fail("NULL local-map array with n_q > 0");
        if (!(why = sp_camera_fault(*P, local)).empty()) return fail(why);
        if (!all_finite(&P->th, 1) || (local && (!all_finite(&P->cos_view, 1) || !std::isfinite(P->nn_ratio)))) return fail("a threshold is not finite");
        if (!(why = sp_keys_fault(*P, local, ori)).empty()) return fail(why);
        for (size_t i = 0, e = (size_t)P->n_q; i < e; i++) {
            if (!all_finite(P->q_pos + 3 * i, 3)) return fail("query " + std::to_string(i) + ": the position is not finite");
            if (!local) {
                if (P->q_oct[i] >= P->n_levels) return fail("query " + std::to_string(i) + ": octave >= n_levels");
                if (ori && !(P->q_angle[i] >= 0.0f && P->q_angle[i] < 360.0f)) return fail("query " + std::to_string(i) + ": angle outside [0, 360)");
            } else {
                if (!all_finite(P->q_normal + 3 * i, 3)) return fail("query " + std::to_string(i) + ": the normal is not finite");
                if (!all_finite(P->q_dist_min + i, 1) || !all_finite(P->q_dist_max + i, 1) || !all_finite(P->q_pred_max + i, 1))
                    return fail("query " + std::to_string(i) + ": a distance is not finite");
            }
        }
        if (!(why = sp_cells_fault(*P, seen, T)).empty()) return fail(why);
    }
    return 0;
}

// behind the upload half, [rounds | best_idx | best_dist | best_dist2 | level | view_cos | uv | state] come back in one copy,
// [rad | prev] never leave the device
struct SearchProjArena : SpUploadArena {
    size_t rounds, best_idx, best_dist, best_dist2, level, view_cos, uv, state, rad, prev;
    SearchProjArena(size_t n, const SearchProjTotals& T) : SpUploadArena(n, T) {
        rounds = L.take((n + 1) * 4); best_idx = L.take((T.qs + 1) * 4); best_dist = L.take((T.qs + 1) * 2); best_dist2 = L.take((T.qs + 1) * 2);
        level = L.take(T.qs + 1); view_cos = L.take((T.qs + 1) * 8); uv = L.take((T.qs + 1) * 16); state = L.take(T.qs + 1);
        L.end_back();
        rad = L.take((T.qs + 1) * 8); prev = L.take((T.qs + 1) * 4);
    }
};

// one problem into the staging block: the rest of its descriptor, its records, its copy of the grid, its scale table.  What a mode
// does not read is packed as zero
inline void pack_search_proj(const vba_search_proj_problem* P, SpDesc& d, const SpUploadArena& A, void* hin) {
    const bool local = P->mode == VBA_SEARCH_PROJ_LOCAL_MAP;
    pack_sp_common(*P, local ? 1 : 0, d, A, hin);
    d.th_high = P->th_high; d.nn_ratio = local ? P->nn_ratio : 0.0f;
    for (int i = 0; i < 3; i++) d.c[12 + i] = local ? P->Ow[i] : 0.0;
    d.c[25] = local ? P->log_scale_factor : 0.0; d.c[27] = local ? P->cos_view : 0.0;
    SpQuery* q = at<SpQuery>(hin, A.query) + (size_t)d.q0;
    for (size_t i = 0, e = (size_t)P->n_q; i < e; i++) {
        std::memset(&q[i], 0, sizeof q[i]);
        std::memcpy(q[i].d, P->q_desc + 32 * i, 32);
        std::memcpy(q[i].pos, P->q_pos + 3 * i, 24);
        if (local) {
            std::memcpy(q[i].normal, P->q_normal + 3 * i, 24);
            q[i].dist_min = P->q_dist_min[i]; q[i].dist_max = P->q_dist_max[i]; q[i].pred_max = P->q_pred_max[i];
        } else
            q[i].oct = P->q_oct[i];
        q[i].skip = P->q_skip[i] ? 1 : 0;
        q[i].blocks = P->q_blocks[i] ? 1 : 0;
    }
}

// The call's back regions as they came back, then the apply loop of the reference replayed in query order (:150-151, :1623-1636) and
// the orientation filter (:1643-1662): a query in state 0 writes its keypoint, a later one may overwrite it (only a non-blocking
// claim can be overwritten); a dropped bin clears the KEYPOINT of each of its entries, whoever wrote it last, and its queries
// leave with state 6
inline void unpack_search_proj(const vba_search_proj_problem* P, vba_search_proj_result* R, const SpDesc& d, int rounds, const int32_t* best_idx,
                               const uint16_t* best_dist, const uint16_t* best_dist2, const int8_t* level, const double* view_cos, const double* uv,
                               const unsigned char* state) {
    const size_t o = (size_t)d.q0, n = (size_t)d.n_q, nk = (size_t)d.n_keys;
    R->status = VBA_OK;
    R->rounds = rounds;
    for (size_t k = 0; k < nk; k++) R->key_match[k] = -1;
    if (n) {
        std::memcpy(R->best_idx, best_idx + o, 4 * n);
        std::memcpy(R->best_dist, best_dist + o, 2 * n);
        std::memcpy(R->best_dist2, best_dist2 + o, 2 * n);
        std::memcpy(R->level, level + o, n);
        std::memcpy(R->view_cos, view_cos + o, 8 * n);
        std::memcpy(R->uv, uv + 2 * o, 16 * n);
        std::memcpy(R->state, state + o, n);
    }
    replay_matches(R, n, nk, P->mode == VBA_SEARCH_PROJ_LAST_FRAME && P->check_orientation, P->q_angle, P->angle, 6,
                   [R](size_t i, int32_t b) { R->key_match[b] = (int32_t)i; },
                   [R](size_t i) { R->key_match[R->best_idx[i]] = -2; });   // :1657
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct SearchProjCall {
    int n = 0;
    SearchProjTotals T;
    SearchProjArena A = SearchProjArena(0, SearchProjTotals());
    int prepare(int n_problems, const vba_search_proj_problem* const* in, const vba_search_proj_result* const* out, std::string& err) {
        n = n_problems;
        if (check_search_proj(n, in, out, T, err)) return 1;
        A = SearchProjArena((size_t)n, T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return (size_t)n; }                   // k_search_proj: one workgroup per problem
    size_t lds_bytes() const { return 4 * (T.max_keys + 1); }   // the claim table of the largest frame
    SpDesc* desc(void* hin) const { return at<SpDesc>(hin, A.desc); }
    void describe(const vba_search_proj_problem* const* in, void* hin) const { describe_sp(n, in, desc(hin)); }
    const char* pack(int f, const vba_search_proj_problem* P, void* hin) const {
        pack_search_proj(P, desc(hin)[f], A, hin);
        return nullptr;
    }
    SpBatch bind(void* base) const {
        SpBatch B;
        bind_sp_upload(B, A, base);
        B.rounds = at<int>(base, A.rounds); B.best_idx = at<int>(base, A.best_idx); B.best_dist = at<unsigned short>(base, A.best_dist);
        B.best_dist2 = at<unsigned short>(base, A.best_dist2); B.level = at<signed char>(base, A.level); B.view_cos = at<double>(base, A.view_cos);
        B.uv = at<double>(base, A.uv); B.state = at<unsigned char>(base, A.state); B.rad = at<double>(base, A.rad); B.prev = at<int>(base, A.prev);
        return B;
    }
    void unpack(int f, vba_search_proj_problem* P, vba_search_proj_result* R, void* hin, void* hout) const {
        auto back = [&](size_t off) { return A.L.in_back(off); };
        unpack_search_proj(P, R, desc(hin)[f], at<int32_t>(hout, back(A.rounds))[f], at<int32_t>(hout, back(A.best_idx)), at<uint16_t>(hout, back(A.best_dist)),
                           at<uint16_t>(hout, back(A.best_dist2)), at<int8_t>(hout, back(A.level)), at<double>(hout, back(A.view_cos)),
                           at<double>(hout, back(A.uv)), at<unsigned char>(hout, back(A.state)));
    }
};

}  // namespace vba_host
