// vba_search_init.h -- batched matching for the monocular initialisation on the GPU.
// Replaces, for a batch of frame pairs, the query loop of ORBmatcher::SearchForInitialization (src/ORBmatcher.cpp:477-562) over
// Frame::GetFeaturesInArea(x, y, windowSize, 0, 0) (src/Frame.cpp:562-620).  The state codes are those of include/vislam_ba.h; the
// apply loop with its steals, the rotation histogram, the drop and the vbPrevMatched update are replayed on the host
// (vba_host_search_init.h).
//
// The queries of a pair are NOT independent, and differently from the other ordered matchers: a query does not skip a TAKEN keypoint,
// it skips a keypoint whose vMatchedDistance is <= its own distance (:518), and an accepted query lowers that value (:545), so a later
// query can take a keypoint away from an earlier one.  What query q reads for keypoint k is
//     D_q[k] = min { bestDist_p : p < q, p accepted, bestIdx_p = k },  INT_MAX for the empty set
// (an accepted claim on k is strictly smaller than the value before it, so the last one is the minimum).  One index per keypoint, the
// claim table of vba_search_claim.h, cannot express a value that depends on q; the structure here keeps per keypoint the LIST of its
// current claimers: head[k] in LDS, next[q] and cdist[q] in the call's arena, and the visitor takes the minimum over the entries < q.
//
// The pass (init_rounds below) is the fixed-point iteration of vba_search_claim.h over that structure.  In a round every open query
// walks its area against the lists of the round before and writes its outputs, which are its claim (accepted, keypoint, distance);
// __syncthreads_or joins "my claim changed"; if any did, the heads are reset and the lists rebuilt from the new claims with an LDS
// exchange push between two barriers.  Push order is arbitrary, a minimum over p < q does not depend on it.  The pass stops after the
// first round in which no claim changed.  Any fixed point is the sequential answer, by induction on q: query q reads claims of
// queries < q only.  After round t the queries 0 .. t are final, so a visitor skips q < round and the pass ends after at most
// n_q + 1 rounds.
//
// Who may read what.  head, next and cdist are read by the visitors only and written only between the barriers of the rebuild.  A
// query's outputs are written by the lane that visits it and read by that lane alone (in the visitor for `changed`, in the rebuild
// for the push), which is why the rebuild copies the distance into cdist: a visitor must not read another query's best_dist while
// its lane rewrites it.  A list holds each query at most once, so a list walk takes at most n_q steps.  One 256-lane workgroup owns
// a pair; nothing waits on another workgroup, and every loop is bounded by sizes the host checked.  The area comparison is FP64 on
// the float32 inputs widened; the ratio test is one float32 product, as the reference computes it, with INT_MAX for "no second".
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_search_area.h"

#define SI_NT VBA_SI_NT

// the heads before any claim, and a barrier
template <int NT>
DEVI void init_reset(int* head, int n_keys) {
    for (int k = threadIdx.x; k < n_keys; k += NT) head[k] = -1;
    __syncthreads();
}

// The rounds 0 .. n_q over heads that init_reset has set; returns the number of rounds run.  visit(q, round): walk query q (or skip
// it) and return whether its claim changed; claim_of(q, dist): the keypoint q claims now with its distance, < 0 for none
template <int NT, class ClaimOf, class Visit>
DEVI int init_rounds(int* head, int* next, int* cdist, int n_keys, int n_q, ClaimOf&& claim_of, Visit&& visit) {
    int n_rounds = 0;
    for (int round = 0; round <= n_q; ++round) {
        int changed = 0;
        for (int q = threadIdx.x; q < n_q; q += NT) changed |= visit(q, round) ? 1 : 0;
        changed = __syncthreads_or(changed);   // every walk of the round has read the lists
        n_rounds = round + 1;
        if (!changed) break;
        init_reset<NT>(head, n_keys);
        for (int q = threadIdx.x; q < n_q; q += NT) {
            int dist;
            const int c = claim_of(q, dist);
            if (c >= 0) {
                cdist[q] = dist;
                next[q] = atomicExch(&head[c], q);
            }
        }
        __syncthreads();
    }
    return n_rounds;
}

__global__ void __launch_bounds__(SI_NT) k_search_init(SiBatch B) {
#pragma clang fp contract(off)
    extern __shared__ int si_head[];   // [n_keys of the call's largest frame 2]
    __shared__ double sc[VBA_SI_CONST];
    const SiDesc& d = B.desc[blockIdx.x];
    const int tid = threadIdx.x;
    const int nk = d.n_keys, nq = d.n_q;   // nk <= VBA_SI_MAX_KEYS (checked on the host)
    if (tid < VBA_SI_CONST) sc[tid] = d.c[tid];
    const double* tb = sc;                 // bounds, grid_inv_w, grid_inv_h where sa_walk reads them
    const SaGrid grid = {B.key + (size_t)d.key0, B.cell_begin + (size_t)d.cell0, B.cell_feat + (size_t)d.feat0, d.cols, d.rows};
    const SiQuery* query = B.query + (size_t)d.q0;
    int* next = B.next + (size_t)d.q0;
    int* cdist = B.cdist + (size_t)d.q0;
    for (int q = tid; q < nq; q += SI_NT) {
        const size_t o = (size_t)d.q0 + (size_t)q;
        B.best_idx[o] = -1;
        B.best_dist[o] = 256;
        B.best_dist2[o] = 256;
        B.state[o] = 255;                  // not walked yet: no claim
    }
    init_reset<SI_NT>(si_head, nk);        // (the barrier also publishes sc)

    const double r = tb[SA_LOGSF];         // windowSize
    const int th_low = d.th_low;
    const float nn_ratio = d.nn_ratio;
    const auto claim_of = [&](int q, int& dist) {
        const size_t o = (size_t)d.q0 + (size_t)q;
        dist = (int)B.best_dist[o];
        return (B.state[o] == 0) ? B.best_idx[o] : -1;
    };
    const int n_rounds = init_rounds<SI_NT>(si_head, next, cdist, nk, nq, claim_of, [&](int q, int round) {
        const size_t o = (size_t)d.q0 + (size_t)q;
        const int st_before = B.state[o];
        if (q < round || st_before == 2) return false;   // final since round q; the area holds no candidate whatever the claims
        const int key_before = (st_before == 0) ? B.best_idx[o] : -1, dist_before = (int)B.best_dist[o];
        const SiQuery& Q = query[q];
        const double u = Q.u, v = Q.v;
        int bestDist = 0x7fffffff, bestDist2 = 0x7fffffff, bestIdx = -1;
        bool any = false;
        unsigned int a[8];
        sa_load_desc(a, Q.d);
        // Frame::GetFeaturesInArea(u, v, r, 0, 0): bCheckLevels is true, the level test stands in front of the pixel test
        sa_walk(grid, tb, u, v, r, [&](int idx, const FuKey& k) {
            if (k.oct != 0) return;                                                  // Frame.cpp:602-606
            if (!(fabs(k.u - u) < r && fabs(k.v - v) < r)) return;                   // Frame.cpp:612
            any = true;
            const int dist = sa_hamming(a, k.d);
            // :518 vMatchedDistance[i2] <= dist, the value as the queries < q left it
            int steps = 0;
            for (int p = si_head[idx]; p >= 0 && steps < nq; p = next[p], ++steps)
                if (p < q && cdist[p] <= dist) return;
            if (dist < bestDist) {                                                   // :521-530
                bestDist2 = bestDist; bestDist = dist;
                bestIdx = idx;
            } else if (dist < bestDist2) {
                bestDist2 = dist;
            }
        });
        int state;
        if (!any) state = 2;                                                         // :501
        else if (!(bestDist <= th_low)) state = 3;                                   // :534
        else if (!((float)bestDist < (float)bestDist2 * nn_ratio)) state = 4;        // :536
        else state = 0;
        B.best_idx[o] = bestIdx;
        B.best_dist[o] = (unsigned short)((bestDist < 256) ? bestDist : 256);
        B.best_dist2[o] = (unsigned short)((bestDist2 < 256) ? bestDist2 : 256);
        B.state[o] = (unsigned char)state;
        const int key_now = (state == 0) ? bestIdx : -1;
        return key_now != key_before || (key_now >= 0 && bestDist != dist_before);
    });
    if (tid == 0) B.rounds[blockIdx.x] = n_rounds;
}
