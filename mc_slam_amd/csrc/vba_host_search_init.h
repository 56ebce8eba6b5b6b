// vba_host_search_init.h -- host half of vba_search_for_initialization (plain C++17, no HIP): which pairs are refused, the arena of a
// call, the descriptor of a pair, the packing of frame 2's keypoint records and grid copy (vba_host_keygrid.h) and of the ordered
// query list -- the level-0 keypoints of frame 1, compacted so that only they cost device work -- into the staging block, and the
// write-back, which replays the reference's apply loop (src/ORBmatcher.cpp:538-558) in query order from the per-query (accepted,
// keypoint, distance): the steals and vnMatches21, the histogram with stolen entries kept, ComputeThreeMaxima (vba_host_orient.h),
// the drop (:572-585) and the vbPrevMatched update (:590-592).  Included by vislam_ba.hip (vba_host_small.h) and by the sanitizer
// harness tests/host_search_init_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_search_init.py).
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

// totals of a call: keypoints of frame 2, queries, entries of all cell_begin and cell_feat copies; the largest frame 2
struct SearchInitTotals {
    size_t keys = 0, qs = 0, cells = 0, feat = 0, max_keys = 0;
};

// frame 2 of a pair under the field names vba_host_keygrid.h is written against.  An octave is a uint8 and no level table is read,
// so n_levels = 256 lets every octave pass keypoint_fault
struct SiFrame2 {
    int32_t n_keys, n_levels, grid_cols, grid_rows;
    const uint8_t* desc;
    const double* uv;
    const uint8_t* oct;
    const int32_t *cell_begin, *cell_feat;
    explicit SiFrame2(const vba_search_init_problem& p)
        : n_keys(p.n_keys2), n_levels(256), grid_cols(p.grid_cols), grid_rows(p.grid_rows), desc(p.desc2), uv(p.uv2), oct(p.oct2),
          cell_begin(p.cell_begin), cell_feat(p.cell_feat) {}
};

// the level-0 keypoints of frame 1 (:495): the queries of a checked pair
inline size_t search_init_queries(const vba_search_init_problem& p) {
    size_t n = 0;
    for (size_t i = 0, e = (size_t)p.n_keys1; i < e; i++) n += p.oct1[i] == 0;
    return n;
}

// 0: every pair is usable; otherwise err says which is not and why
inline int check_search_init(int n, const vba_search_init_problem* const* in, const vba_search_init_result* const* out, SearchInitTotals& T,
                             std::string& err) {
    T = SearchInitTotals();
    std::vector<unsigned char> seen;
    for (int f = 0; f < n; f++) {
        const vba_search_init_problem* P = in[f];
        const vba_search_init_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "pair " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        const bool ori = P->check_orientation != 0;
        if (P->n_keys1 < 0) return fail("negative n_keys1");
        if (P->n_keys2 < 0) return fail("negative n_keys2");
        if (P->n_keys2 > VBA_SI_MAX_KEYS) return fail("n_keys2 above 16384: the claimer lists of frame 2 live in LDS");
        if (P->th_low < 0 || P->th_low > 255) return fail("th_low outside 0 .. 255");
        if (!std::isfinite(P->nn_ratio) || !std::isfinite(P->window_size)) return fail("a threshold is not finite");
        const SiFrame2 F2(*P);
        if (!grid_size_ok(F2)) return fail("grid size outside 1 .. 65536 cells");
        if (P->n_keys1 > 0 && (!P->desc1 || !P->oct1 || !P->prev_matched || (ori && !P->angle1) || !R->match12 || !R->best_idx || !R->best_dist ||
                               !R->best_dist2 || !R->bin || !R->state || !R->prev_matched))
            return fail("NULL array with n_keys1 > 0");
        if (P->n_keys2 > 0 && (!P->desc2 || !P->uv2 || !P->oct2 || (ori && !P->angle2) || !R->match21 || !R->matched_dist))
            return fail("NULL array with n_keys2 > 0");
        if (!P->cell_begin) return fail("NULL cell_begin");
        if (!all_finite(P->bounds, 4) || !all_finite(&P->grid_inv_w, 1) || !all_finite(&P->grid_inv_h, 1)) return fail("a bound or cell size is not finite");
        for (size_t i = 0, e = (size_t)P->n_keys1; i < e; i++) {
            if (!std::isfinite(P->prev_matched[2 * i]) || !std::isfinite(P->prev_matched[2 * i + 1]))
                return fail("keypoint " + std::to_string(i) + " of frame 1: prev_matched is not finite");
            if (ori && !(P->angle1[i] >= 0.0f && P->angle1[i] < 360.0f)) return fail("keypoint " + std::to_string(i) + " of frame 1: angle outside [0, 360)");
        }
        for (size_t i = 0, e = (size_t)P->n_keys2; i < e; i++) {
            if (const char* why = keypoint_fault(F2, i)) return fail("keypoint " + std::to_string(i) + " of frame 2: " + why);
            if (ori && !(P->angle2[i] >= 0.0f && P->angle2[i] < 360.0f)) return fail("keypoint " + std::to_string(i) + " of frame 2: angle outside [0, 360)");
        }
        int nf = 0;
        const std::string why = check_cell_lists(P->grid_cols, P->grid_rows, P->n_keys2, P->cell_begin, P->cell_feat, seen, nf);
        if (!why.empty()) return fail(why);
        T.keys += (size_t)P->n_keys2; T.qs += search_init_queries(*P);
        T.cells += grid_cells(F2) + 1; T.feat += (size_t)nf;
        if ((size_t)P->n_keys2 > T.max_keys) T.max_keys = (size_t)P->n_keys2;
    }
    return 0;
}

// [desc | key | query | cell | feat] go up in one copy, [rounds | best_idx | best_dist | best_dist2 | state] come back in one copy,
// [next | cdist] never leave the device
struct SearchInitArena {
    ArenaLayout L;
    size_t desc, key, query, cell, feat, rounds, best_idx, best_dist, best_dist2, state, next, cdist;
    SearchInitArena(size_t n, const SearchInitTotals& T) {
        desc = L.take(sizeof(SiDesc) * n); key = L.take(sizeof(FuKey) * (T.keys + 1)); query = L.take(sizeof(SiQuery) * (T.qs + 1));
        cell = L.take((T.cells + 1) * 4); feat = L.take((T.feat + 1) * 4);
        L.end_upload();
        rounds = L.take((n + 1) * 4); best_idx = L.take((T.qs + 1) * 4); best_dist = L.take((T.qs + 1) * 2); best_dist2 = L.take((T.qs + 1) * 2);
        state = L.take(T.qs + 1);
        L.end_back();
        next = L.take((T.qs + 1) * 4); cdist = L.take((T.qs + 1) * 4);
    }
};

// offsets of every pair's regions in the concatenated arrays, and its query count
inline void describe_search_init(int n, const vba_search_init_problem* const* in, SiDesc* desc) {
    size_t k = 0, q = 0, c = 0, ft = 0;
    for (int f = 0; f < n; f++) {
        const SiFrame2 F2(*in[f]);
        const size_t nq = search_init_queries(*in[f]);
        desc[f].key0 = (long long)k; desc[f].q0 = (long long)q; desc[f].cell0 = (long long)c; desc[f].feat0 = (long long)ft;
        desc[f].n_q = (int)nq;
        k += (size_t)F2.n_keys; q += nq; c += grid_cells(F2) + 1; ft += grid_feat(F2);
    }
}

// one pair into the staging block: the rest of its descriptor, frame 2's records and grid copy, the query records in index order
inline void pack_search_init(const vba_search_init_problem* P, SiDesc& d, const SearchInitArena& A, void* hin) {
    const SiFrame2 F2(*P);
    d.n_keys = P->n_keys2; d.cols = P->grid_cols; d.rows = P->grid_rows;
    d.th_low = P->th_low; d.nn_ratio = P->nn_ratio; d.pad[0] = d.pad[1] = 0;
    std::memcpy(d.c, P->bounds, 32);
    d.c[4] = P->grid_inv_w; d.c[5] = P->grid_inv_h; d.c[6] = P->window_size; d.c[7] = 0.0;
    pack_keys(F2, at<FuKey>(hin, A.key) + (size_t)d.key0);
    pack_grid(F2, at<int32_t>(hin, A.cell) + (size_t)d.cell0, at<int32_t>(hin, A.feat) + (size_t)d.feat0);
    SiQuery* q = at<SiQuery>(hin, A.query) + (size_t)d.q0;
    size_t j = 0;
    for (size_t i = 0, e = (size_t)P->n_keys1; i < e; i++) {
        if (P->oct1[i] != 0) continue;
        std::memset(&q[j], 0, sizeof q[j]);
        std::memcpy(q[j].d, P->desc1 + 32 * i, 32);
        q[j].u = (double)P->prev_matched[2 * i]; q[j].v = (double)P->prev_matched[2 * i + 1];
        q[j].idx1 = (int)i;
        j++;
    }
}

// The call's back regions as they came back, spread from the query list over the keypoints of frame 1, then the apply loop of the
// reference replayed in query order: an accepted query takes its keypoint and the query that held it loses its match (state 5,
// n_stolen; :538-546); its bin keeps counting (:557).  Then the three maxima; the drop touches only what still holds a match
// (:579-582, state 6) and leaves vnMatches21 alone.  Last, vbPrevMatched (:590-592) on the copy.  replay_matches (vba_host_orient.h)
// does not fit: the steal has to run inside its loop, and its drop would decrement for entries whose match12 is already -1
inline void unpack_search_init(const vba_search_init_problem* P, vba_search_init_result* R, const SiDesc& d, const SiQuery* query, int rounds,
                               const int32_t* best_idx, const uint16_t* best_dist, const uint16_t* best_dist2, const unsigned char* state) {
    const size_t o = (size_t)d.q0, nq = (size_t)d.n_q, n1 = (size_t)P->n_keys1, n2 = (size_t)P->n_keys2;
    const bool ori = P->check_orientation != 0;
    R->status = VBA_OK;
    R->rounds = rounds;
    for (int i = 0; i < VBA_ST_HISTO; i++) R->hist[i] = 0;
    R->ind[0] = R->ind[1] = R->ind[2] = -1;
    for (size_t i = 0; i < n1; i++) {
        R->match12[i] = -1; R->best_idx[i] = -1; R->best_dist[i] = 256; R->best_dist2[i] = 256; R->bin[i] = 255;
        R->state[i] = 1;                                                             // :495; a query overwrites it below
    }
    for (size_t k = 0; k < n2; k++) { R->match21[k] = -1; R->matched_dist[k] = 256; }
    if (n1) std::memcpy(R->prev_matched, P->prev_matched, 8 * n1);
    int nmatches = 0, stolen = 0;
    for (size_t j = 0; j < nq; j++) {
        const size_t i = (size_t)query[o + j].idx1;
        const int32_t b = best_idx[o + j];
        R->best_idx[i] = b; R->best_dist[i] = best_dist[o + j]; R->best_dist2[i] = best_dist2[o + j];
        R->state[i] = state[o + j];
        if (state[o + j] != 0 || b < 0 || (size_t)b >= n2) continue;                 // a state 0 always brings a keypoint of frame 2
        const int32_t held = R->match21[b];
        if (held >= 0) { R->match12[held] = -1; R->state[held] = 5; nmatches--; stolen++; }   // :538-542
        R->match12[i] = b; R->match21[b] = (int32_t)i; R->matched_dist[b] = best_dist[o + j];
        nmatches++;
        if (ori) {
            const int bin = rot_bin(P->angle1[i], P->angle2[b]);
            R->bin[i] = (uint8_t)bin;
            R->hist[bin]++;
        }
    }
    R->n_before_filter = nmatches;
    R->n_stolen = stolen;
    if (ori) {
        three_maxima(R->hist, R->ind);
        for (size_t i = 0; i < n1; i++) {
            const int bin = R->bin[i];
            if (bin == 255 || bin == R->ind[0] || bin == R->ind[1] || bin == R->ind[2] || R->match12[i] < 0) continue;
            R->match12[i] = -1;
            R->state[i] = 6;
            nmatches--;
        }
    }
    R->n_matches = nmatches;
    for (size_t i = 0; i < n1; i++) {
        const int32_t b = R->match12[i];
        if (b < 0) continue;
        R->prev_matched[2 * i] = (float)P->uv2[2 * (size_t)b]; R->prev_matched[2 * i + 1] = (float)P->uv2[2 * (size_t)b + 1];
    }
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct SearchInitCall {
    int n = 0;
    SearchInitTotals T;
    SearchInitArena A = SearchInitArena(0, SearchInitTotals());
    int prepare(int n_pairs, const vba_search_init_problem* const* in, const vba_search_init_result* const* out, std::string& err) {
        n = n_pairs;
        if (check_search_init(n, in, out, T, err)) return 1;
        A = SearchInitArena((size_t)n, T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return (size_t)n; }                   // k_search_init: one workgroup per pair
    size_t lds_bytes() const { return 4 * (T.max_keys + 1); }   // the list heads of the largest frame 2
    SiDesc* desc(void* hin) const { return at<SiDesc>(hin, A.desc); }
    void describe(const vba_search_init_problem* const* in, void* hin) const { describe_search_init(n, in, desc(hin)); }
    const char* pack(int f, const vba_search_init_problem* P, void* hin) const {
        pack_search_init(P, desc(hin)[f], A, hin);
        return nullptr;
    }
    SiBatch bind(void* base) const {
        SiBatch B;
        B.desc = at<SiDesc>(base, A.desc); B.key = at<FuKey>(base, A.key); B.query = at<SiQuery>(base, A.query);
        B.cell_begin = at<int>(base, A.cell); B.cell_feat = at<int>(base, A.feat);
        B.rounds = at<int>(base, A.rounds); B.best_idx = at<int>(base, A.best_idx); B.best_dist = at<unsigned short>(base, A.best_dist);
        B.best_dist2 = at<unsigned short>(base, A.best_dist2); B.state = at<unsigned char>(base, A.state);
        B.next = at<int>(base, A.next); B.cdist = at<int>(base, A.cdist);
        return B;
    }
    void unpack(int f, vba_search_init_problem* P, vba_search_init_result* R, void* hin, void* hout) const {
        auto back = [&](size_t off) { return A.L.in_back(off); };
        unpack_search_init(P, R, desc(hin)[f], at<SiQuery>(hin, A.query), at<int32_t>(hout, back(A.rounds))[f], at<int32_t>(hout, back(A.best_idx)),
                           at<uint16_t>(hout, back(A.best_dist)), at<uint16_t>(hout, back(A.best_dist2)), at<unsigned char>(hout, back(A.state)));
    }
};

}  // namespace vba_host
