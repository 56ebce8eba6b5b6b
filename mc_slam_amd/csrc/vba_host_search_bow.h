// vba_host_search_bow.h -- host half of vba_search_by_bow (plain C++17, no HIP): which pairs are refused, the arena of a call, the
// descriptor of a pair, the node join of src/ORBmatcher.cpp:229-322 / :639-725 with the ordered query list it yields (every query
// with its rank among the queries of its node), the packing of the descriptor records into the staging block, and the write-back:
// match12 and match21, the rotation histogram, ComputeThreeMaxima and the drop (:325-347, :727-745).  The feature-vector check is
// check_feat_vec of vba_host_search_tri.h; the replay with the bin and the three maxima is replay_matches of vba_host_orient.h.
// Included by vislam_ba.hip (vba_host_small.h) and by the sanitizer harness tests/host_search_bow_check.cpp
// (g++ -fsanitize=address,undefined, tests/test_host_search_bow.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_host_orient.h"
#include "vba_host_search_tri.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace vba_host {

// totals of a call: keypoints of the sides 1 / 2, entries of all node_feat2; the largest side 2
struct SearchBowTotals {
    size_t k1 = 0, k2 = 0, feat = 0, max_keys2 = 0;
};

// 0: every pair is usable; otherwise err says which is not and why
inline int check_search_bow(int n, const vba_search_bow_problem* const* in, const vba_search_bow_result* const* out, SearchBowTotals& T,
                            std::string& err) {
    T = SearchBowTotals();
    std::vector<unsigned char> seen;
    for (int f = 0; f < n; f++) {
        const vba_search_bow_problem* P = in[f];
        const vba_search_bow_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "pair " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->mode != VBA_SEARCH_BOW_KF_FRAME && P->mode != VBA_SEARCH_BOW_KF_KF) return fail("unknown mode");
        const bool kfkf = P->mode == VBA_SEARCH_BOW_KF_KF;
        if (P->n_keys1 < 0 || P->n_keys2 < 0) return fail("negative n_keys");
        if (P->n_keys2 > VBA_SB_MAX_KEYS) return fail("n_keys2 above 16384: the claim table of side 2 lives in LDS");
        if (P->th_low < 0 || P->th_low > 255) return fail("th_low outside 0 .. 255");
        if (!std::isfinite(P->nn_ratio)) return fail("nn_ratio is not finite");
        if (P->n_keys1 > 0 && (!P->desc1 || !P->good_mp1 || !R->match12 || !R->best_idx || !R->best_dist || !R->best_dist2 || !R->bin || !R->state))
            return fail("NULL array with n_keys1 > 0");
        if (P->n_keys2 > 0 && (!P->desc2 || !R->match21 || (kfkf && !P->good_mp2))) return fail("NULL array with n_keys2 > 0");
        if (P->check_orientation) {
            if ((P->n_keys1 > 0 && !P->angle1) || (P->n_keys2 > 0 && !P->angle2)) return fail("NULL angles with check_orientation");
            for (size_t i = 0, e = (size_t)P->n_keys1; i < e; i++)
                if (!(P->angle1[i] >= 0.0f && P->angle1[i] < 360.0f)) return fail("keypoint " + std::to_string(i) + " of keyframe 1: angle outside [0, 360)");
            for (size_t i = 0, e = (size_t)P->n_keys2; i < e; i++)
                if (!(P->angle2[i] >= 0.0f && P->angle2[i] < 360.0f)) return fail("keypoint " + std::to_string(i) + " of keyframe 2: angle outside [0, 360)");
        }
        std::string why = check_feat_vec(1, P->n_keys1, P->n_nodes1, P->node_id1, P->node_begin1, P->node_feat1, seen);
        if (why.empty()) why = check_feat_vec(2, P->n_keys2, P->n_nodes2, P->node_id2, P->node_begin2, P->node_feat2, seen);
        if (!why.empty()) return fail(why);
        T.k1 += (size_t)P->n_keys1; T.k2 += (size_t)P->n_keys2;
        T.feat += (size_t)P->node_begin2[P->n_nodes2];
        if ((size_t)P->n_keys2 > T.max_keys2) T.max_keys2 = (size_t)P->n_keys2;
    }
    return 0;
}

// [desc | key1 | key2 | role | blocked | query | feat] go up in one copy, [rounds | best_idx | best_dist | best_dist2 | state] come
// back in one, [prev] never leaves the device.  The query region has one slot per keypoint of side 1 (a keypoint is listed at most
// once); a pair uses the first n_q of its slots
struct SearchBowArena {
    ArenaLayout L;
    size_t desc, key1, key2, role, blocked, query, feat, rounds, best_idx, best_dist, best_dist2, state, prev;
    SearchBowArena(size_t n, const SearchBowTotals& T) {
        desc = L.take(sizeof(SbDesc) * n); key1 = L.take(sizeof(SbKey) * (T.k1 + 1)); key2 = L.take(sizeof(SbKey) * (T.k2 + 1));
        role = L.take(T.k1 + 1); blocked = L.take(T.k2 + 1); query = L.take(sizeof(SbQuery) * (T.k1 + 1)); feat = L.take((T.feat + 1) * 4);
        L.end_upload();
        rounds = L.take((n + 1) * 4); best_idx = L.take((T.k1 + 1) * 4); best_dist = L.take((T.k1 + 1) * 2); best_dist2 = L.take((T.k1 + 1) * 2);
        state = L.take(T.k1 + 1);
        L.end_back();
        prev = L.take((T.k1 + 1) * 4);
    }
};

// offsets of every pair's regions in the concatenated arrays (the rest of a descriptor comes with the packing)
inline void describe_search_bow(int n, const vba_search_bow_problem* const* in, SbDesc* desc) {
    size_t k1 = 0, k2 = 0, ft = 0;
    for (int f = 0; f < n; f++) {
        desc[f].key1_0 = (long long)k1; desc[f].key2_0 = (long long)k2; desc[f].feat0 = (long long)ft;
        k1 += (size_t)in[f]->n_keys1; k2 += (size_t)in[f]->n_keys2; ft += (size_t)in[f]->node_begin2[in[f]->n_nodes2];
    }
}

// The walk of :229-322 / :639-725 over the two node lists, as join_search_tri does it.  Every keypoint of side 1 that a shared node
// lists and that has a good map point becomes a query with that node's range of node_feat2 and its rank among the queries of the
// node, in the order of the walk; role[idx1] (n_keys1 entries) becomes 1 without a good map point, 0 for a query, 2 for the rest.
// Returns the number of queries (q has room for n_keys1); max_rank is the largest number of queries in one node
inline int join_search_bow(const vba_search_bow_problem* P, SbQuery* q, unsigned char* role, int& max_rank) {
    for (int i = 0; i < P->n_keys1; i++) role[i] = P->good_mp1[i] ? 2 : 1;
    int i1 = 0, i2 = 0, nq = 0;
    max_rank = 0;
    while (i1 < P->n_nodes1 && i2 < P->n_nodes2) {
        if (P->node_id1[i1] == P->node_id2[i2]) {
            int rank = 0;
            for (int k = P->node_begin1[i1]; k < P->node_begin1[i1 + 1]; k++) {
                const int idx1 = P->node_feat1[k];
                if (role[idx1] == 1) continue;   // :243-247, :649-652
                role[idx1] = 0;
                q[nq].idx1 = idx1; q[nq].c_begin = P->node_begin2[i2]; q[nq].c_end = P->node_begin2[i2 + 1]; q[nq].rank = rank++;
                nq++;
            }
            if (rank > max_rank) max_rank = rank;
            i1++; i2++;
        } else if (P->node_id1[i1] < P->node_id2[i2]) {
            while (i1 < P->n_nodes1 && P->node_id1[i1] < P->node_id2[i2]) i1++;   // lower_bound (:316, :719)
        } else {
            while (i2 < P->n_nodes2 && P->node_id2[i2] < P->node_id1[i1]) i2++;   // :320, :723
        }
    }
    return nq;
}

// one pair into the staging block: the rest of its descriptor, the join, its records, its copy of node_feat2
inline void pack_search_bow(const vba_search_bow_problem* P, SbDesc& d, SbKey* hk1, SbKey* hk2, unsigned char* hrole, unsigned char* hblocked, SbQuery* hq,
                            int32_t* hfeat) {
    const bool kfkf = P->mode == VBA_SEARCH_BOW_KF_KF;
    d.n_keys1 = P->n_keys1; d.n_keys2 = P->n_keys2;
    d.th_pass = kfkf ? P->th_low - 1 : P->th_low;   // :691 `<` against :280 `<=`, on integers
    d.nn_ratio = P->nn_ratio;
    d.n_q = join_search_bow(P, hq + (size_t)d.key1_0, hrole + (size_t)d.key1_0, d.max_rank);
    if (P->n_keys1 > 0) std::memcpy(hk1 + (size_t)d.key1_0, P->desc1, 32 * (size_t)P->n_keys1);
    if (P->n_keys2 > 0) std::memcpy(hk2 + (size_t)d.key2_0, P->desc2, 32 * (size_t)P->n_keys2);
    unsigned char* bl = hblocked + (size_t)d.key2_0;
    for (size_t i = 0, e = (size_t)P->n_keys2; i < e; i++) bl[i] = (kfkf && !P->good_mp2[i]) ? 1 : 0;   // :667-671
    const size_t nf = (size_t)P->node_begin2[P->n_nodes2];
    if (nf) std::memcpy(hfeat + (size_t)d.feat0, P->node_feat2, 4 * nf);
}

// The call's back regions as they came back, then what the reference does with a match (:287-305, :695-709) and the orientation
// filter (:325-347, :727-745): a keypoint of side 2 is taken by at most one query, so match21 does not depend on the order; a
// dropped bin clears match12 and marks match21 with -2, and its queries leave with state 5
inline void unpack_search_bow(const vba_search_bow_problem* P, vba_search_bow_result* R, const SbDesc& d, int rounds, const int32_t* best_idx,
                              const uint16_t* best_dist, const uint16_t* best_dist2, const unsigned char* state) {
    const size_t o = (size_t)d.key1_0, n = (size_t)d.n_keys1, n2 = (size_t)d.n_keys2;
    R->status = VBA_OK;
    R->rounds = rounds;
    for (size_t i = 0; i < n; i++) R->match12[i] = -1;
    for (size_t k = 0; k < n2; k++) R->match21[k] = -1;
    if (n) {
        std::memcpy(R->best_idx, best_idx + o, 4 * n);
        std::memcpy(R->best_dist, best_dist + o, 2 * n);
        std::memcpy(R->best_dist2, best_dist2 + o, 2 * n);
        std::memcpy(R->state, state + o, n);
    }
    replay_matches(R, n, n2, P->check_orientation != 0, P->angle1, P->angle2, 5,
                   [R](size_t i, int32_t b) { R->match12[i] = b; R->match21[b] = (int32_t)i; },
                   [R](size_t i) { R->match21[R->match12[i]] = -2; R->match12[i] = -1; });   // :343, :741
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct SearchBowCall {
    int n = 0;
    SearchBowTotals T;
    SearchBowArena A = SearchBowArena(0, SearchBowTotals());
    int prepare(int n_pairs, const vba_search_bow_problem* const* in, const vba_search_bow_result* const* out, std::string& err) {
        n = n_pairs;
        if (check_search_bow(n, in, out, T, err)) return 1;
        A = SearchBowArena((size_t)n, T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return (size_t)n; }                    // k_search_bow: one workgroup per pair
    size_t lds_bytes() const { return 4 * (T.max_keys2 + 1); }   // the claim table of the largest side 2
    SbDesc* desc(void* hin) const { return at<SbDesc>(hin, A.desc); }
    void describe(const vba_search_bow_problem* const* in, void* hin) const { describe_search_bow(n, in, desc(hin)); }
    const char* pack(int f, const vba_search_bow_problem* P, void* hin) const {
        pack_search_bow(P, desc(hin)[f], at<SbKey>(hin, A.key1), at<SbKey>(hin, A.key2), at<unsigned char>(hin, A.role), at<unsigned char>(hin, A.blocked),
                        at<SbQuery>(hin, A.query), at<int32_t>(hin, A.feat));
        return nullptr;
    }
    SbBatch bind(void* base) const {
        SbBatch B;
        B.desc = desc(base); B.key1 = at<SbKey>(base, A.key1); B.key2 = at<SbKey>(base, A.key2); B.role = at<unsigned char>(base, A.role);
        B.blocked = at<unsigned char>(base, A.blocked); B.query = at<SbQuery>(base, A.query); B.feat = at<int>(base, A.feat);
        B.rounds = at<int>(base, A.rounds); B.best_idx = at<int>(base, A.best_idx); B.best_dist = at<unsigned short>(base, A.best_dist);
        B.best_dist2 = at<unsigned short>(base, A.best_dist2); B.state = at<unsigned char>(base, A.state); B.prev = at<int>(base, A.prev);
        return B;
    }
    void unpack(int f, vba_search_bow_problem* P, vba_search_bow_result* R, void* hin, void* hout) const {
        auto back = [&](size_t off) { return A.L.in_back(off); };
        unpack_search_bow(P, R, desc(hin)[f], at<int32_t>(hout, back(A.rounds))[f], at<int32_t>(hout, back(A.best_idx)), at<uint16_t>(hout, back(A.best_dist)),
                          at<uint16_t>(hout, back(A.best_dist2)), at<unsigned char>(hout, back(A.state)));
    }
};

}  // namespace vba_host
