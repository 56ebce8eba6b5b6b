// vba_host_fuse.h -- host half of vba_fuse (plain C++17, no HIP): which problems are refused, the arena of a call, the descriptor of
// a problem, the tile table, the packing of the keypoint and point records and of the grid copy into the staging block, the
// write-back with n_found.  Included by vislam_ba.hip (vba_host_small.h) and by the sanitizer harness tests/host_fuse_check.cpp
// (g++ -fsanitize=address,undefined, tests/test_host_fuse.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_host_keygrid.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace vba_host {

// totals of a call: keypoints, points, entries of all cell_begin and cell_feat copies, doubles of all level tables, tiles
struct FuseTotals {
    size_t keys = 0, pts = 0, cells = 0, feat = 0, lev = 0, tiles = 0;
};

inline size_t fuse_tiles(int n_pt) { return ((size_t)n_pt + VBA_FU_NT - 1) / VBA_FU_NT; }

// 0: every problem is usable; otherwise err says which is not and why
inline int check_fuse(int n, const vba_fuse_problem* const* in, const vba_fuse_result* const* out, FuseTotals& T, std::string& err) {
    T = FuseTotals();
    std::vector<unsigned char> seen;
    for (int f = 0; f < n; f++) {
        const vba_fuse_problem* P = in[f];
        const vba_fuse_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "problem " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->n_keys < 0) return fail("negative n_keys");
        if (P->n_pt < 0) return fail("negative n_pt");
        if (P->n_levels < 1 || P->n_levels > VBA_TRI_LEVELS) return fail("n_levels outside 1 .. 64");
        if (!P->scale || !P->inv_level_sigma2) return fail("NULL level table");
        if (P->th_low < 0 || P->th_low > 256) return fail("th_low outside 0 .. 256");
        if (!grid_size_ok(*P)) return fail("grid size outside 1 .. 65536 cells");
        if (P->n_keys > 0 && (!P->desc || !P->uv || !P->oct)) return fail("NULL array with n_keys > 0");
        if (P->n_pt > 0 && (!P->pos || !P->normal || !P->dist_min || !P->dist_max || !P->pred_max || !P->pt_desc || !P->skip || !R->best_idx ||
                            !R->best_dist || !R->level || !R->uv || !R->state))
            return fail("NULL array with n_pt > 0");
        if (!P->cell_begin) return fail("NULL cell_begin");
        if (!all_finite(P->Rcw, 9) || !all_finite(P->tcw, 3) || !all_finite(P->Ow, 3)) return fail("the pose is not finite");
        if (!all_finite(P->K, 4)) return fail("an intrinsic is not finite");
        if (!all_finite(P->bounds, 4) || !all_finite(&P->grid_inv_w, 1) || !all_finite(&P->grid_inv_h, 1)) return fail("a bound or cell size is not finite");
        if (!all_finite(&P->th, 1) || !all_finite(&P->cos_view, 1) || !all_finite(&P->chi2_reproj, 1)) return fail("a threshold is not finite");
        if (!all_finite(P->scale, (size_t)P->n_levels) || !all_finite(P->inv_level_sigma2, (size_t)P->n_levels) || !all_finite(&P->log_scale_factor, 1))
            return fail("a level table is not finite");
        for (size_t i = 0, e = (size_t)P->n_keys; i < e; i++) {
            if (const char* why = keypoint_fault(*P, i)) return fail("keypoint " + std::to_string(i) + ": " + why);
        }
        for (size_t i = 0, e = (size_t)P->n_pt; i < e; i++) {
            if (!all_finite(P->pos + 3 * i, 3)) return fail("point " + std::to_string(i) + ": the position is not finite");
            if (!all_finite(P->normal + 3 * i, 3)) return fail("point " + std::to_string(i) + ": the normal is not finite");
            if (!all_finite(P->dist_min + i, 1) || !all_finite(P->dist_max + i, 1) || !all_finite(P->pred_max + i, 1))
                return fail("point " + std::to_string(i) + ": a distance is not finite");
        }
        int nf = 0;
        const std::string why = check_cell_lists(P->grid_cols, P->grid_rows, P->n_keys, P->cell_begin, P->cell_feat, seen, nf);
        if (!why.empty()) return fail(why);
        T.keys += (size_t)P->n_keys; T.pts += (size_t)P->n_pt;
        T.cells += grid_cells(*P) + 1; T.feat += (size_t)nf;
        T.lev += 2 * (size_t)P->n_levels; T.tiles += fuse_tiles(P->n_pt);
    }
    return 0;
}

// [desc | tile | key | pt | cell | feat | lev] go up in one copy, [best_idx | best_dist | level | uv | state] come back in one.
// Records are 64 and 128 bytes and every region starts at a multiple of 256, so descriptor rows are 16-byte aligned
struct FuseArena {
    ArenaLayout L;
    size_t desc, tile, key, pt, cell, feat, lev, best_idx, best_dist, level, uv, state;
    FuseArena(size_t n, const FuseTotals& T) {
        desc = L.take(sizeof(FuDesc) * n); tile = L.take(sizeof(FuTile) * (T.tiles + 1)); key = L.take(sizeof(FuKey) * (T.keys + 1));
        pt = L.take(sizeof(FuPoint) * (T.pts + 1)); cell = L.take((T.cells + 1) * 4); feat = L.take((T.feat + 1) * 4); lev = L.take((T.lev + 1) * 8);
        L.end_upload();
        best_idx = L.take((T.pts + 1) * 4); best_dist = L.take((T.pts + 1) * 2); level = L.take(T.pts + 1); uv = L.take((T.pts + 1) * 16);
        state = L.take(T.pts + 1);
        L.end_back();
    }
};

// offsets of every problem's regions in the concatenated arrays, and the tile table: the tiles of problem 0, then those of
// problem 1, ...; a problem without points gets none.  Returns the number of tiles
inline size_t describe_fuse(int n, const vba_fuse_problem* const* in, FuDesc* desc, FuTile* tile) {
    size_t k = 0, p = 0, c = 0, ft = 0, lv = 0, nt = 0;
    for (int f = 0; f < n; f++) {
        desc[f].key0 = (long long)k; desc[f].pt0 = (long long)p; desc[f].cell0 = (long long)c; desc[f].feat0 = (long long)ft; desc[f].lev0 = (long long)lv;
        for (int first = 0; first < in[f]->n_pt; first += VBA_FU_NT) { tile[nt].prob = f; tile[nt].first = first; nt++; }
        k += (size_t)in[f]->n_keys; p += (size_t)in[f]->n_pt; c += grid_cells(*in[f]) + 1;
        ft += grid_feat(*in[f]); lv += 2 * (size_t)in[f]->n_levels;
    }
    return nt;
}

// one problem into the staging block: the rest of its descriptor, its records, its copy of the grid, its level tables
inline void pack_fuse(const vba_fuse_problem* P, FuDesc& d, FuKey* hkey, FuPoint* hpt, int32_t* hcell, int32_t* hfeat, double* hlev) {
    d.n_keys = P->n_keys; d.n_pt = P->n_pt; d.n_levels = P->n_levels; d.th_low = P->th_low;
    d.cols = P->grid_cols; d.rows = P->grid_rows; d.check_reproj = P->check_reproj ? 1 : 0; d.pad = 0;
    std::memcpy(d.c, P->Rcw, 72); std::memcpy(d.c + 9, P->tcw, 24); std::memcpy(d.c + 12, P->Ow, 24);
    std::memcpy(d.c + 15, P->K, 32); std::memcpy(d.c + 19, P->bounds, 32);
    d.c[23] = P->grid_inv_w; d.c[24] = P->grid_inv_h; d.c[25] = P->log_scale_factor; d.c[26] = P->th; d.c[27] = P->cos_view; d.c[28] = P->chi2_reproj;
    pack_keys(*P, hkey + (size_t)d.key0);
    FuPoint* q = hpt + (size_t)d.pt0;
    for (size_t i = 0, e = (size_t)P->n_pt; i < e; i++) {
        std::memcpy(q[i].d, P->pt_desc + 32 * i, 32);
        std::memcpy(q[i].pos, P->pos + 3 * i, 24); std::memcpy(q[i].normal, P->normal + 3 * i, 24);
        q[i].dist_min = P->dist_min[i]; q[i].dist_max = P->dist_max[i]; q[i].pred_max = P->pred_max[i];
        q[i].skip = P->skip[i] ? 1 : 0;
        std::memset(q[i].pad, 0, sizeof q[i].pad);
    }
    const size_t nl = (size_t)P->n_levels;
    pack_grid(*P, hcell + (size_t)d.cell0, hfeat + (size_t)d.feat0);
    std::memcpy(hlev + (size_t)d.lev0, P->scale, 8 * nl);
    std::memcpy(hlev + (size_t)d.lev0 + nl, P->inv_level_sigma2, 8 * nl);
}

// the call's back regions as they came back; n_found counts the points in state 0
inline void unpack_fuse(vba_fuse_result* R, const FuDesc& d, const int32_t* best_idx, const uint16_t* best_dist, const int8_t* level, const double* uv,
                        const unsigned char* state) {
    const size_t o = (size_t)d.pt0, n = (size_t)d.n_pt;
    R->status = VBA_OK;
    int found = 0;
    if (n) {
        std::memcpy(R->best_idx, best_idx + o, 4 * n);
        std::memcpy(R->best_dist, best_dist + o, 2 * n);
        std::memcpy(R->level, level + o, n);
        std::memcpy(R->uv, uv + 2 * o, 16 * n);
        std::memcpy(R->state, state + o, n);
        for (size_t i = 0; i < n; i++) found += state[o + i] == 0;
    }
    R->n_found = found;
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct FuseCall {
    int n = 0;
    FuseTotals T;
    FuseArena A = FuseArena(0, FuseTotals());
    int prepare(int n_problems, const vba_fuse_problem* const* in, const vba_fuse_result* const* out, std::string& err) {
        n = n_problems;
        if (check_fuse(n, in, out, T, err)) return 1;
        A = FuseArena((size_t)n, T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return T.tiles; }   // k_fuse: one workgroup per tile; a call whose problems all have no points has nothing to search
    FuDesc* desc(void* hin) const { return at<FuDesc>(hin, A.desc); }
    void describe(const vba_fuse_problem* const* in, void* hin) const { describe_fuse(n, in, desc(hin), at<FuTile>(hin, A.tile)); }
    const char* pack(int f, const vba_fuse_problem* P, void* hin) const {
        pack_fuse(P, desc(hin)[f], at<FuKey>(hin, A.key), at<FuPoint>(hin, A.pt), at<int32_t>(hin, A.cell), at<int32_t>(hin, A.feat), at<double>(hin, A.lev));
        return nullptr;
    }
    FuBatch bind(void* base) const {
        FuBatch B;
        B.desc = desc(base); B.tile = at<FuTile>(base, A.tile); B.key = at<FuKey>(base, A.key); B.pt = at<FuPoint>(base, A.pt);
        B.cell_begin = at<int>(base, A.cell); B.cell_feat = at<int>(base, A.feat); B.lev = at<double>(base, A.lev);
        B.best_idx = at<int>(base, A.best_idx); B.best_dist = at<unsigned short>(base, A.best_dist); B.level = at<signed char>(base, A.level);
        B.uv = at<double>(base, A.uv); B.state = at<unsigned char>(base, A.state);
        return B;
    }
    void unpack(int f, vba_fuse_problem*, vba_fuse_result* R, void* hin, void* hout) const {
        unpack_fuse(R, desc(hin)[f], at<int32_t>(hout, A.L.in_back(A.best_idx)), at<uint16_t>(hout, A.L.in_back(A.best_dist)),
                    at<int8_t>(hout, A.L.in_back(A.level)), at<double>(hout, A.L.in_back(A.uv)), at<unsigned char>(hout, A.L.in_back(A.state)));
    }
};

}  // namespace vba_host
