// vba_host_search_sim3.h -- host half of vba_search_by_sim3 (plain C++17, no HIP): which pairs are refused, the arena of a call, the
// two direction descriptors of a pair, the tile table, the compaction of the queries (only keypoints with has_pt && !matched get
// a record), the packing of the keypoint records and of the grid copies into the staging block, and the write-back: the states 1
// and 2, the scatter of what came back, and the agreement loop of src/ORBmatcher.cpp:1480-1493 with n_found.  Included by
// vislam_ba.hip (vba_host_small.h) and by the sanitizer harness tests/host_search_sim3_check.cpp (g++ -fsanitize=address,undefined,
// tests/test_host_search_sim3.py).
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

// totals of a call: keypoints of all keyframes, queries, entries of all cell_begin and cell_feat copies, doubles of all scale
// tables, tiles
struct SearchSim3Totals {
    size_t keys = 0, queries = 0, cells = 0, feat = 0, lev = 0, tiles = 0;
};

inline size_t search_sim3_tiles(size_t n_q) { return (n_q + VBA_SS_NT - 1) / VBA_SS_NT; }

// one keyframe side of a pair with its result arrays: an empty string, or why it is refused.  n_q: its keypoints with has_pt && !matched
inline std::string check_search_sim3_kf(const vba_search_sim3_kf& P, const int32_t* match, const uint16_t* best_dist, const int8_t* level,
                                        const uint8_t* state, bool match12_ok, std::vector<unsigned char>& seen, size_t& n_q) {
    n_q = 0;
    if (P.n_keys < 0) return "negative n_keys";
    if (P.n_levels < 1 || P.n_levels > VBA_TRI_LEVELS) return "n_levels outside 1 .. 64";
    if (!P.scale) return "NULL level table";
    if (!grid_size_ok(P)) return "grid size outside 1 .. 65536 cells";
    if (P.n_keys > 0 && (!P.desc || !P.uv || !P.oct || !P.has_pt || !P.matched || !P.pos || !P.dist_min || !P.dist_max || !P.pred_max || !P.pt_desc ||
                         !match || !best_dist || !level || !state || !match12_ok))
        return "NULL array with n_keys > 0";
    if (!P.cell_begin) return "NULL cell_begin";
    if (!all_finite(P.Rcw, 9) || !all_finite(P.tcw, 3)) return "the pose is not finite";
    if (!all_finite(P.bounds, 4) || !all_finite(&P.grid_inv_w, 1) || !all_finite(&P.grid_inv_h, 1)) return "a bound or cell size is not finite";
    if (!all_finite(P.scale, (size_t)P.n_levels) || !all_finite(&P.log_scale_factor, 1)) return "a level table is not finite";
    for (size_t i = 0, e = (size_t)P.n_keys; i < e; i++) {
        if (const char* why = keypoint_fault(P, i)) return "keypoint " + std::to_string(i) + ": " + why;
        if (!P.has_pt[i]) continue;
        if (!all_finite(P.pos + 3 * i, 3)) return "keypoint " + std::to_string(i) + ": the position is not finite";
        if (!all_finite(P.dist_min + i, 1) || !all_finite(P.dist_max + i, 1) || !all_finite(P.pred_max + i, 1))
            return "keypoint " + std::to_string(i) + ": a distance is not finite";
        n_q += !P.matched[i];
    }
    int nf = 0;
    return check_cell_lists(P.grid_cols, P.grid_rows, P.n_keys, P.cell_begin, P.cell_feat, seen, nf);
}

// 0: every pair is usable; otherwise err says which is not and why.  nq: the queries of every direction, [2 * pair + dir]
inline int check_search_sim3(int n, const vba_search_sim3_problem* const* in, const vba_search_sim3_result* const* out, SearchSim3Totals& T,
                             std::vector<size_t>& nq, std::string& err) {
    T = SearchSim3Totals();
    nq.assign(2 * (size_t)n, 0);
    std::vector<unsigned char> seen;
    for (int f = 0; f < n; f++) {
        const vba_search_sim3_problem* P = in[f];
        const vba_search_sim3_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "pair " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        std::string why = check_search_sim3_kf(P->kf1, R->match1, R->best_dist1, R->level1, R->state1, R->match12 != nullptr, seen, nq[2 * (size_t)f]);
        if (!why.empty()) return fail("keyframe 1: " + why);
        why = check_search_sim3_kf(P->kf2, R->match2, R->best_dist2, R->level2, R->state2, true, seen, nq[2 * (size_t)f + 1]);
        if (!why.empty()) return fail("keyframe 2: " + why);
        if (!std::isfinite(P->s12) || !(P->s12 > 0.0)) return fail("s12 is not finite or not positive");
        if (!all_finite(P->R12, 9) || !all_finite(P->t12, 3)) return fail("the Sim3 is not finite");
        if (!all_finite(P->K, 4)) return fail("an intrinsic is not finite");
        if (!all_finite(&P->th, 1)) return fail("a threshold is not finite");
        if (P->th_high < 0 || P->th_high > 256) return fail("th_high outside 0 .. 256");
        for (int s = 0; s < 2; s++) {
            const vba_search_sim3_kf& Kf = s ? P->kf2 : P->kf1;
            T.keys += (size_t)Kf.n_keys; T.cells += grid_cells(Kf) + 1; T.feat += grid_feat(Kf); T.lev += (size_t)Kf.n_levels;
            T.queries += nq[2 * (size_t)f + s]; T.tiles += search_sim3_tiles(nq[2 * (size_t)f + s]);
        }
    }
    return 0;
}

// [dir | tile | key | query | cell | feat | lev] go up in one copy, [match | best_dist | level | state] come back in one.
// Records are 64 and 96 bytes and every region starts at a multiple of 256, so descriptor rows are 16-byte aligned
struct SearchSim3Arena {
    ArenaLayout L;
    size_t dir, tile, key, query, cell, feat, lev, match, best_dist, level, state;
    SearchSim3Arena(size_t n, const SearchSim3Totals& T) {
        dir = L.take(sizeof(SsDir) * 2 * n); tile = L.take(sizeof(SsTile) * (T.tiles + 1)); key = L.take(sizeof(FuKey) * (T.keys + 1));
        query = L.take(sizeof(SsQuery) * (T.queries + 1)); cell = L.take((T.cells + 1) * 4); feat = L.take((T.feat + 1) * 4); lev = L.take((T.lev + 1) * 8);
        L.end_upload();
        match = L.take((T.queries + 1) * 4); best_dist = L.take((T.queries + 1) * 2); level = L.take(T.queries + 1); state = L.take(T.queries + 1);
        L.end_back();
    }
};

// offsets of every direction's regions in the concatenated arrays, and the tile table: the tiles of direction 0 of pair 0, of
// direction 1 of pair 0, of direction 0 of pair 1, ...; a tile never spans two directions and a direction without queries gets
// none.  Direction 0 (keyframe 1 into keyframe 2) reads the records of keyframe 2, direction 1 those of keyframe 1.  Returns the
// number of tiles
inline size_t describe_search_sim3(int n, const vba_search_sim3_problem* const* in, const std::vector<size_t>& nq, SsDir* dir, SsTile* tile) {
    size_t k = 0, q = 0, c = 0, ft = 0, lv = 0, nt = 0;
    for (int f = 0; f < n; f++) {
        for (int s = 0; s < 2; s++) {   // side s is the SOURCE of direction s and the TARGET of direction 1 - s
            const vba_search_sim3_kf& Kf = s ? in[f]->kf2 : in[f]->kf1;
            SsDir& src = dir[2 * (size_t)f + s];
            SsDir& tgt = dir[2 * (size_t)f + 1 - s];
            src.q0 = (long long)q; src.n_q = (int)nq[2 * (size_t)f + s];
            tgt.key0 = (long long)k; tgt.cell0 = (long long)c; tgt.feat0 = (long long)ft; tgt.lev0 = (long long)lv;
            for (size_t first = 0; first < nq[2 * (size_t)f + s]; first += VBA_SS_NT) {
                tile[nt].pair = f; tile[nt].dir = s; tile[nt].first = (int)first; tile[nt].pad = 0;
                nt++;
            }
            k += (size_t)Kf.n_keys; q += nq[2 * (size_t)f + s]; c += grid_cells(Kf) + 1; ft += grid_feat(Kf); lv += (size_t)Kf.n_levels;
        }
    }
    return nt;
}

// sR12 = s12 R12, sR21 = (1 / s12) R12^T, t21 = -sR21 t12, in the order src/ORBmatcher.cpp:1277-1279 write them
inline void search_sim3_transforms(const vba_search_sim3_problem* P, double* sR12, double* sR21, double* t21) {
    const double inv = 1.0 / P->s12;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            sR12[3 * i + j] = P->s12 * P->R12[3 * i + j];
            sR21[3 * i + j] = inv * P->R12[3 * j + i];
        }
    for (int i = 0; i < 3; i++)
        t21[i] = ((-sR21[3 * i]) * P->t12[0] + (-sR21[3 * i + 1]) * P->t12[1]) + (-sR21[3 * i + 2]) * P->t12[2];
}

// one pair into the staging block: the rest of its two descriptors, the keypoint records, grid copies and scale tables of both
// keyframes, and the compacted queries of both directions
inline void pack_search_sim3(const vba_search_sim3_problem* P, SsDir* d2, FuKey* hkey, SsQuery* hq, int32_t* hcell, int32_t* hfeat, double* hlev) {
    double sR12[9], sR21[9], t21[3];
    search_sim3_transforms(P, sR12, sR21, t21);
    for (int s = 0; s < 2; s++) {
        const vba_search_sim3_kf& Src = s ? P->kf2 : P->kf1;
        const vba_search_sim3_kf& Tgt = s ? P->kf1 : P->kf2;
        SsDir& d = d2[s];
        d.n_keys = Tgt.n_keys; d.n_levels = Tgt.n_levels; d.th_high = P->th_high; d.cols = Tgt.grid_cols; d.rows = Tgt.grid_rows;
        d.pad[0] = d.pad[1] = 0;
        std::memcpy(d.c, Src.Rcw, 72); std::memcpy(d.c + 9, Src.tcw, 24);
        std::memcpy(d.c + 12, s ? sR12 : sR21, 72); std::memcpy(d.c + 21, s ? P->t12 : t21, 24);
        std::memcpy(d.c + 24, P->K, 32); std::memcpy(d.c + 28, Tgt.bounds, 32);
        d.c[32] = Tgt.grid_inv_w; d.c[33] = Tgt.grid_inv_h; d.c[34] = Tgt.log_scale_factor; d.c[35] = P->th;
        // the records of the target of this direction sit where describe put them
        pack_keys(Tgt, hkey + (size_t)d.key0);
        pack_grid(Tgt, hcell + (size_t)d.cell0, hfeat + (size_t)d.feat0);
        std::memcpy(hlev + (size_t)d.lev0, Tgt.scale, 8 * (size_t)Tgt.n_levels);
        SsQuery* q = hq + (size_t)d.q0;
        size_t m = 0;
        for (size_t i = 0, e = (size_t)Src.n_keys; i < e; i++) {
            if (!Src.has_pt[i] || Src.matched[i]) continue;
            std::memcpy(q[m].d, Src.pt_desc + 32 * i, 32);
            std::memcpy(q[m].pos, Src.pos + 3 * i, 24);
            q[m].dist_min = Src.dist_min[i]; q[m].dist_max = Src.dist_max[i]; q[m].pred_max = Src.pred_max[i];
            q[m].idx = (int)i;
            q[m].pad[0] = q[m].pad[1] = q[m].pad[2] = 0;
            m++;
        }
    }
}

// one side of a pair: the states 1 and 2 for the keypoints without a query, then the scatter of what came back for its queries
inline void unpack_search_sim3_side(const vba_search_sim3_kf& Src, const SsDir& d, const SsQuery* hq, const int32_t* match, const uint16_t* best_dist,
                                    const int8_t* level, const unsigned char* state, int32_t* r_match, uint16_t* r_best, int8_t* r_level, uint8_t* r_state) {
    for (size_t i = 0, e = (size_t)Src.n_keys; i < e; i++) {
        r_match[i] = -1; r_best[i] = 256; r_level[i] = -128;
        r_state[i] = !Src.has_pt[i] ? 1 : (Src.matched[i] ? 2 : 255);
    }
    const size_t o = (size_t)d.q0;
    for (size_t m = 0, e = (size_t)d.n_q; m < e; m++) {
        const size_t i = (size_t)hq[o + m].idx;
        r_match[i] = match[o + m]; r_best[i] = best_dist[o + m]; r_level[i] = level[o + m]; r_state[i] = state[o + m];
    }
}

// the call's back regions as they came back; then the agreement loop of :1480-1493 in one pass over match1
inline void unpack_search_sim3(const vba_search_sim3_problem* P, vba_search_sim3_result* R, const SsDir* d2, const SsQuery* hq, const int32_t* match,
                               const uint16_t* best_dist, const int8_t* level, const unsigned char* state) {
    unpack_search_sim3_side(P->kf1, d2[0], hq, match, best_dist, level, state, R->match1, R->best_dist1, R->level1, R->state1);
    unpack_search_sim3_side(P->kf2, d2[1], hq, match, best_dist, level, state, R->match2, R->best_dist2, R->level2, R->state2);
    int found = 0;
    for (int i1 = 0; i1 < P->kf1.n_keys; i1++) {
        const int idx2 = R->match1[i1];
        const bool agreed = idx2 >= 0 && idx2 < P->kf2.n_keys && R->match2[idx2] == i1;
        R->match12[i1] = agreed ? idx2 : -1;
        found += agreed;
    }
    R->n_found = found;
    R->status = VBA_OK;
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct SearchSim3Call {
    int n = 0;
    SearchSim3Totals T;
    std::vector<size_t> nq;
    SearchSim3Arena A = SearchSim3Arena(0, SearchSim3Totals());
    int prepare(int n_pairs, const vba_search_sim3_problem* const* in, const vba_search_sim3_result* const* out, std::string& err) {
        n = n_pairs;
        if (check_search_sim3(n, in, out, T, nq, err)) return 1;
        A = SearchSim3Arena((size_t)n, T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return T.tiles; }   // k_search_sim3: one workgroup per tile; a call without queries has nothing to search
    SsDir* dir(void* hin) const { return at<SsDir>(hin, A.dir); }
    void describe(const vba_search_sim3_problem* const* in, void* hin) const { describe_search_sim3(n, in, nq, dir(hin), at<SsTile>(hin, A.tile)); }
    const char* pack(int f, const vba_search_sim3_problem* P, void* hin) const {
        pack_search_sim3(P, dir(hin) + 2 * (size_t)f, at<FuKey>(hin, A.key), at<SsQuery>(hin, A.query), at<int32_t>(hin, A.cell), at<int32_t>(hin, A.feat),
                         at<double>(hin, A.lev));
        return nullptr;
    }
    SsBatch bind(void* base) const {
        SsBatch B;
        B.dir = dir(base); B.tile = at<SsTile>(base, A.tile); B.key = at<FuKey>(base, A.key); B.query = at<SsQuery>(base, A.query);
        B.cell_begin = at<int>(base, A.cell); B.cell_feat = at<int>(base, A.feat); B.lev = at<double>(base, A.lev);
        B.match = at<int>(base, A.match); B.best_dist = at<unsigned short>(base, A.best_dist); B.level = at<signed char>(base, A.level);
        B.state = at<unsigned char>(base, A.state);
        return B;
    }
    void unpack(int f, vba_search_sim3_problem* P, vba_search_sim3_result* R, void* hin, void* hout) const {
        unpack_search_sim3(P, R, dir(hin) + 2 * (size_t)f, at<SsQuery>(hin, A.query), at<int32_t>(hout, A.L.in_back(A.match)),
                           at<uint16_t>(hout, A.L.in_back(A.best_dist)), at<int8_t>(hout, A.L.in_back(A.level)),
                           at<unsigned char>(hout, A.L.in_back(A.state)));
    }
};

}  // namespace vba_host
