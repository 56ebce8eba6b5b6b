// vba_host_search_tri.h -- host half of vba_search_triangulation (plain C++17, no HIP): which pairs are refused, the arena of a
// call, the descriptor of a pair, the node join of src/ORBmatcher.cpp:801-921 with the query list it yields, the packing of the
// interleaved keypoint records into the staging block, the write-back with vMatchedPairs.  Included by vislam_ba.hip
// (vba_host_small.h) and by the sanitizer harness tests/host_search_tri_check.cpp (g++ -fsanitize=address,undefined,
// tests/test_host_search_tri.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace vba_host {

// totals of a call: keypoints of the keyframes 1 / 2, entries of all node_feat_2, doubles of all level tables
struct SearchTriTotals {
    size_t k1 = 0, k2 = 0, feat = 0, lev = 0;
};

// one side's feature vector: "" or why it is refused
inline std::string check_feat_vec(int side, int n_keys, int n_nodes, const uint32_t* id, const int32_t* begin, const int32_t* feat,
                                  std::vector<unsigned char>& seen) {
    const std::string s = " of keyframe " + std::to_string(side);
    if (n_nodes < 0) return "negative n_nodes" + s;
    if (!begin) return "NULL node_begin" + s;
    if (n_nodes > 0 && !id) return "NULL node_id" + s;
    if (begin[0] != 0) return "node_begin" + s + " does not start at 0";
    for (int k = 0; k < n_nodes; k++) {
        if (k > 0 && !(id[k] > id[k - 1])) return "node_id" + s + " is not strictly ascending at node " + std::to_string(k);
        if (begin[k + 1] < begin[k]) return "node_begin" + s + " decreases at node " + std::to_string(k);
    }
    const int n = begin[n_nodes];
    if (n > 0 && !feat) return "NULL node_feat" + s;
    seen.assign((size_t)n_keys, 0);
    for (int i = 0; i < n; i++) {
        const int a = feat[i];
        if (a < 0 || a >= n_keys) return "node_feat" + s + " entry " + std::to_string(i) + ": keypoint index out of range";
        if (seen[(size_t)a]) return "node_feat" + s + " entry " + std::to_string(i) + ": keypoint " + std::to_string(a) + " listed twice";
        seen[(size_t)a] = 1;
    }
    return "";
}

// 0: every pair is usable; otherwise err says which is not and why
inline int check_search_tri(int n, const vba_search_tri_problem* const* in, const vba_search_tri_result* const* out, SearchTriTotals& T,
                            std::string& err) {
    T = SearchTriTotals();
    std::vector<unsigned char> seen;
    for (int f = 0; f < n; f++) {
        const vba_search_tri_problem* P = in[f];
        const vba_search_tri_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "pair " + std::to_string(f) + ": " + m; return 1; };
        auto finite = [](const double* a, size_t k) { for (size_t i = 0; i < k; i++) if (!std::isfinite(a[i])) return false; return true; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->n_keys1 < 0 || P->n_keys2 < 0) return fail("negative n_keys");
        if (P->n_levels2 < 1 || P->n_levels2 > VBA_TRI_LEVELS) return fail("n_levels2 outside 1 .. 64");
        if (!P->level_sigma2_2 || !P->scale_2) return fail("NULL level table");
        if (P->th_low < 0 || P->th_low > 255) return fail("th_low outside 0 .. 255");
        if (P->n_keys1 > 0 && (!P->desc1 || !P->has_mp1 || !P->uv1 || !R->match12 || !R->best_dist || !R->state || !R->pairs))
            return fail("NULL array with n_keys1 > 0");
        if (P->n_keys2 > 0 && (!P->desc2 || !P->has_mp2 || !P->uv2 || !P->oct2)) return fail("NULL array with n_keys2 > 0");
        if (P->check_orientation && ((P->n_keys1 > 0 && !P->angle1) || (P->n_keys2 > 0 && !P->angle2))) return fail("NULL angles with check_orientation");
        if (!finite(P->F12, 9)) return fail("F12 is not finite");
        if (!finite(P->epipole, 2)) return fail("the epipole is not finite");
        if (!finite(&P->chi2_epi, 1) || !finite(&P->epipole_r2, 1)) return fail("a threshold is not finite");
        if (!finite(P->level_sigma2_2, (size_t)P->n_levels2) || !finite(P->scale_2, (size_t)P->n_levels2)) return fail("a level table is not finite");
        for (size_t i = 0, e = (size_t)P->n_keys1; i < e; i++) {
            if (!finite(P->uv1 + 2 * i, 2)) return fail("keypoint " + std::to_string(i) + " of keyframe 1: a pixel is not finite");
            if (P->check_orientation && !(P->angle1[i] >= 0.0f && P->angle1[i] < 360.0f))
                return fail("keypoint " + std::to_string(i) + " of keyframe 1: angle outside [0, 360)");
        }
        for (size_t i = 0, e = (size_t)P->n_keys2; i < e; i++) {
            if (!finite(P->uv2 + 2 * i, 2)) return fail("keypoint " + std::to_string(i) + " of keyframe 2: a pixel is not finite");
            if (P->oct2[i] >= P->n_levels2) return fail("keypoint " + std::to_string(i) + " of keyframe 2: octave >= n_levels2");
            if (P->check_orientation && !(P->angle2[i] >= 0.0f && P->angle2[i] < 360.0f))
                return fail("keypoint " + std::to_string(i) + " of keyframe 2: angle outside [0, 360)");
        }
        std::string why = check_feat_vec(1, P->n_keys1, P->n_nodes1, P->node_id1, P->node_begin1, P->node_feat1, seen);
        if (why.empty()) why = check_feat_vec(2, P->n_keys2, P->n_nodes2, P->node_id2, P->node_begin2, P->node_feat2, seen);
        if (!why.empty()) return fail(why);
        T.k1 += (size_t)P->n_keys1; T.k2 += (size_t)P->n_keys2;
        T.feat += (size_t)P->node_begin2[P->n_nodes2];
        T.lev += 2 * (size_t)P->n_levels2;
    }
    return 0;
}

// [desc | key1 | key2 | query | feat | lev] go up in one copy, [out | match12 | best_dist | state] come back in one.  A keypoint
// record is 64 bytes and every region starts at a multiple of 256, so descriptor rows are 16-byte aligned.  The query region has
// one slot per keypoint of keyframe 1 (a keypoint is listed at most once); a pair uses the first n_q of its slots
struct SearchTriArena {
    ArenaLayout L;
    size_t desc, key1, key2, query, feat, lev, out, match12, best_dist, state;
    SearchTriArena(size_t n, const SearchTriTotals& T) {
        desc = L.take(sizeof(StDesc) * n); key1 = L.take(sizeof(StKey) * (T.k1 + 1)); key2 = L.take(sizeof(StKey) * (T.k2 + 1));
        query = L.take(sizeof(StQuery) * (T.k1 + 1)); feat = L.take((T.feat + 1) * 4); lev = L.take((T.lev + 1) * 8);
        L.end_upload();
        out = L.take(sizeof(StOut) * n); match12 = L.take((T.k1 + 1) * 4); best_dist = L.take(T.k1 + 1); state = L.take(T.k1 + 1);
        L.end_back();
    }
};

// offsets of every pair's regions in the concatenated arrays (the rest of a descriptor comes with the packing)
inline void describe_search_tri(int n, const vba_search_tri_problem* const* in, StDesc* desc) {
    size_t k1 = 0, k2 = 0, ft = 0, lv = 0;
    for (int f = 0; f < n; f++) {
        desc[f].key1_0 = (long long)k1; desc[f].key2_0 = (long long)k2; desc[f].feat0 = (long long)ft; desc[f].lev0 = (long long)lv;
        k1 += (size_t)in[f]->n_keys1; k2 += (size_t)in[f]->n_keys2;
        ft += (size_t)in[f]->node_begin2[in[f]->n_nodes2]; lv += 2 * (size_t)in[f]->n_levels2;
    }
}

// The walk of :801-921 over the two node lists.  Every keypoint of keyframe 1 that a shared node lists and that has no map point
// becomes a query with that node's range of node_feat_2, in the order of the walk; role[idx1] (n_keys1 entries) becomes 1 for a
// map point, 0 for a query, 2 for the rest.  Returns the number of queries (q has room for n_keys1)
inline int join_search_tri(const vba_search_tri_problem* P, StQuery* q, unsigned char* role) {
    for (int i = 0; i < P->n_keys1; i++) role[i] = P->has_mp1[i] ? 1 : 2;
    int i1 = 0, i2 = 0, nq = 0;
    while (i1 < P->n_nodes1 && i2 < P->n_nodes2) {
        if (P->node_id1[i1] == P->node_id2[i2]) {
            for (int k = P->node_begin1[i1]; k < P->node_begin1[i1 + 1]; k++) {
                const int idx1 = P->node_feat1[k];
                if (role[idx1] == 1) continue;   // :817
                role[idx1] = 0;
                q[nq].idx1 = idx1; q[nq].c_begin = P->node_begin2[i2]; q[nq].c_end = P->node_begin2[i2 + 1]; q[nq].pad = 0;
                nq++;
            }
            i1++; i2++;
        } else if (P->node_id1[i1] < P->node_id2[i2]) {
            while (i1 < P->n_nodes1 && P->node_id1[i1] < P->node_id2[i2]) i1++;   // lower_bound (:915)
        } else {
            while (i2 < P->n_nodes2 && P->node_id2[i2] < P->node_id1[i1]) i2++;   // :919
        }
    }
    return nq;
}

inline void pack_key(StKey& k, const uint8_t* desc, const double* uv, const float* angle, size_t i, unsigned char oct, unsigned char role) {
    std::memcpy(k.d, desc + 32 * i, 32);
    k.u = uv[2 * i]; k.v = uv[2 * i + 1];
    k.angle = angle ? angle[i] : 0.0f;
    k.oct = oct; k.role = role;
    std::memset(k.pad, 0, sizeof k.pad);
}

// one pair into the staging block: the rest of its descriptor, the join, its records, its copy of node_feat_2, its level tables
inline void pack_search_tri(const vba_search_tri_problem* P, StDesc& d, StKey* hk1, StKey* hk2, StQuery* hq, int32_t* hfeat, double* hlev) {
    d.n_keys1 = P->n_keys1; d.n_keys2 = P->n_keys2; d.n_levels2 = P->n_levels2;
    d.th_low = P->th_low; d.check_orientation = P->check_orientation ? 1 : 0;
    std::memcpy(d.c, P->F12, 72);
    d.c[9] = P->epipole[0]; d.c[10] = P->epipole[1]; d.c[11] = P->chi2_epi; d.c[12] = P->epipole_r2;
    StKey* k1 = hk1 + (size_t)d.key1_0;
    StKey* k2 = hk2 + (size_t)d.key2_0;
    std::vector<unsigned char> role((size_t)P->n_keys1 + 1);
    d.n_q = join_search_tri(P, hq + (size_t)d.key1_0, role.data());
    const float* a1 = P->check_orientation ? P->angle1 : nullptr;
    const float* a2 = P->check_orientation ? P->angle2 : nullptr;
    for (size_t i = 0, e = (size_t)P->n_keys1; i < e; i++) pack_key(k1[i], P->desc1, P->uv1, a1, i, 0, role[i]);
    for (size_t i = 0, e = (size_t)P->n_keys2; i < e; i++) pack_key(k2[i], P->desc2, P->uv2, a2, i, P->oct2[i], P->has_mp2[i] ? 1 : 0);
    const size_t nf = (size_t)P->node_begin2[P->n_nodes2], nl = (size_t)P->n_levels2;
    if (nf) std::memcpy(hfeat + (size_t)d.feat0, P->node_feat2, 4 * nf);
    std::memcpy(hlev + (size_t)d.lev0, P->level_sigma2_2, 8 * nl);
    std::memcpy(hlev + (size_t)d.lev0 + nl, P->scale_2, 8 * nl);
}

// the call's back regions as they came back; vMatchedPairs (:947-952) is rebuilt from match12
inline void unpack_search_tri(vba_search_tri_result* R, const StDesc& d, const StOut& r, const int32_t* match12, const unsigned char* best_dist,
                              const unsigned char* state) {
    const size_t o = (size_t)d.key1_0, n = (size_t)d.n_keys1;
    R->status = r.status; R->n_matches = r.n_matches; R->n_before_filter = r.n_before_filter;
    std::memcpy(R->hist, r.hist, sizeof r.hist);
    std::memcpy(R->ind, r.ind, sizeof r.ind);
    if (n) {
        std::memcpy(R->match12, match12 + o, 4 * n);
        std::memcpy(R->best_dist, best_dist + o, n);
        std::memcpy(R->state, state + o, n);
        size_t k = 0;
        for (size_t i = 0; i < n; i++)
            if (match12[o + i] >= 0) { R->pairs[2 * k] = (int32_t)i; R->pairs[2 * k + 1] = match12[o + i]; k++; }
    }
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct SearchTriCall {
    int n = 0;
    SearchTriTotals T;
    SearchTriArena A = SearchTriArena(0, SearchTriTotals());
    int prepare(int n_pairs, const vba_search_tri_problem* const* in, const vba_search_tri_result* const* out, std::string& err) {
        n = n_pairs;
        if (check_search_tri(n, in, out, T, err)) return 1;
        A = SearchTriArena((size_t)n, T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return (size_t)n; }   // k_search_tri: one workgroup per pair
    StDesc* desc(void* hin) const { return at<StDesc>(hin, A.desc); }
    void describe(const vba_search_tri_problem* const* in, void* hin) const { describe_search_tri(n, in, desc(hin)); }
    const char* pack(int f, const vba_search_tri_problem* P, void* hin) const {
        pack_search_tri(P, desc(hin)[f], at<StKey>(hin, A.key1), at<StKey>(hin, A.key2), at<StQuery>(hin, A.query), at<int32_t>(hin, A.feat),
                        at<double>(hin, A.lev));
        return nullptr;
    }
    StBatch bind(void* base) const {
        StBatch B;
        B.desc = desc(base); B.key1 = at<StKey>(base, A.key1); B.key2 = at<StKey>(base, A.key2); B.query = at<StQuery>(base, A.query);
        B.feat = at<int>(base, A.feat); B.lev = at<double>(base, A.lev); B.out = at<StOut>(base, A.out); B.match12 = at<int>(base, A.match12);
        B.best_dist = at<unsigned char>(base, A.best_dist); B.state = at<unsigned char>(base, A.state);
        return B;
    }
    void unpack(int f, vba_search_tri_problem*, vba_search_tri_result* R, void* hin, void* hout) const {
        unpack_search_tri(R, desc(hin)[f], at<StOut>(hout, A.L.in_back(A.out))[f], at<int32_t>(hout, A.L.in_back(A.match12)),
                          at<unsigned char>(hout, A.L.in_back(A.best_dist)), at<unsigned char>(hout, A.L.in_back(A.state)));
    }
};

}  // namespace vba_host
