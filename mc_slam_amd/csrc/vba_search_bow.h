// vba_search_bow.h -- batched bag-of-words matching on the GPU.
// Replaces, for a batch of pairs, both ORBmatcher::SearchByBoW overloads (src/ORBmatcher.cpp:207-350 keyframe -> frame, :609-748
// keyframe -> keyframe) behind the node join, which the host does (vba_host_search_bow.h): the candidate loop of every keypoint of
// side 1 that has a good map point (:251-306, :656-711) with the taken flags it reads and writes.  The state codes are those of
// include/vislam_ba.h; the rotation histogram, ComputeThreeMaxima and the drop are replayed on the host in the write-back.
//
// One 256-lane workgroup per pair, ONE launch.  Lanes stride over the query list the host laid out in the order of the reference's
// walk, so neighbouring lanes sit in the same node and run through the same candidates.  A query's descriptor lives in 8 VGPRs; a
// candidate is one 32-byte SbKey record, two 16-byte loads.
//
// The queries of a pair are NOT independent: a query skips the keypoints of side 2 an earlier query has taken (:260, :667) and then
// takes its own (:287, :696).  The conflict pass is the one of vba_search_claim.h (the protocol and its proof are there) over the
// walk indices: a query claims keypoint k when its current result is a MATCH on k (threshold and ratio test passed), and a keypoint
// is statically taken when it is no candidate at all (KF_KF mode without a good map point).
//
// The node-local bound.  A keypoint of side 2 is listed in at most one node (checked on the host), and a query walks the candidates
// of its own node only.  So claim[k] < q can hold, for a k that q reads, only through a query of q's node with a smaller walk index,
// that is with a smaller rank (SbQuery::rank, the place among the queries of the node).  Induction on the rank r: a query of rank 0
// reads static entries only and is final after round 0; in round r a query of rank r reads the table rebuilt after round r - 1, in
// which every query of a rank < r of its node has its final claim, so what it computes in round r is final.  A query is therefore
// skipped from round rank + 1 on, in round max_rank (the largest number of queries in one shared node) no query is open, nothing
// changes and the loop `round <= max_rank` ends by itself: rounds <= max_rank + 1, not n_q + 1.
//
// The claim table is n_keys2 int32 of dynamic LDS (n_keys2 <= VBA_SB_MAX_KEYS, checked on the host); the kernel declares no static
// LDS (the code object reports the 256 bytes of the workgroup reduction behind __syncthreads_or), and the table is read and
// written in 32-bit words only.  No atomic touches memory, and every output address is written by one lane only.  The ratio test is
// one float32 product, as the reference computes it.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_search_area.h"   // sa_load_desc, sa_hamming
#include "vba_search_claim.h"

#define SB_NT VBA_SB_NT

__global__ void __launch_bounds__(SB_NT) k_search_bow(SbBatch B) {
    extern __shared__ int sb_claim[];   // [n_keys2 of the call's largest pair]
    const SbDesc& d = B.desc[blockIdx.x];
    const int tid = threadIdx.x;
    const int n1 = d.n_keys1, n2 = d.n_keys2, nq = d.n_q;   // n2 <= VBA_SB_MAX_KEYS (checked on the host)
    const int th_pass = d.th_pass, max_rank = d.max_rank;
    const float nn_ratio = d.nn_ratio;
    const SbKey* key1 = B.key1 + (size_t)d.key1_0;
    const SbKey* key2 = B.key2 + (size_t)d.key2_0;
    const unsigned char* role = B.role + (size_t)d.key1_0;
    const unsigned char* blocked = B.blocked + (size_t)d.key2_0;
    const SbQuery* query = B.query + (size_t)d.key1_0;
    const int* feat = B.feat + (size_t)d.feat0;
    int* best_idx = B.best_idx + (size_t)d.key1_0;
    unsigned short* best_dist = B.best_dist + (size_t)d.key1_0;
    unsigned short* best_dist2 = B.best_dist2 + (size_t)d.key1_0;
    unsigned char* state = B.state + (size_t)d.key1_0;
    int* prev = B.prev + (size_t)d.key1_0;

    // every keypoint of side 1 that is no query leaves with the state the host found; the table before any claim
    for (int i = tid; i < n1; i += SB_NT) {
        const unsigned char r = role[i];
        if (r != 0) { best_idx[i] = -1; best_dist[i] = 256; best_dist2[i] = 256; state[i] = r; }
    }
    for (int q = tid; q < nq; q += SB_NT) prev[q] = -1;
    const auto taken = [&](int k) { return blocked[k] != 0; };
    claim_reset<SB_NT>(sb_claim, n2, taken);

    // the conflict pass: at most max_rank + 1 rounds.  The visitor walks one query against the table of the round before
    const int n_rounds = claim_rounds<SB_NT>(sb_claim, n2, nq, max_rank, taken, [&](int q) { return prev[q]; }, [&](int q, int round) {
        const SbQuery Q = query[q];
        if (Q.rank < round) return false;   // final since round rank
        unsigned int a[8];
        sa_load_desc(a, key1[Q.idx1].d);
        int bestDist1 = 256, bestDist2 = 256, bestIdx = -1;
        for (int c = Q.c_begin; c < Q.c_end; c++) {
            const int idx2 = feat[c];
            if (sb_claim[idx2] < q) continue;                                        // :260, :667-671
            const int dist = sa_hamming(a, key2[idx2].d);
            if (dist < bestDist1) {                                                  // :267-276, :677-686
                bestDist2 = bestDist1; bestDist1 = dist;
                bestIdx = idx2;
            } else if (dist < bestDist2) {
                bestDist2 = dist;
            }
        }
        int st;
        if (!(bestDist1 <= th_pass)) st = 3;                                         // :280, :691
        else if (!((float)bestDist1 < nn_ratio * (float)bestDist2)) st = 4;          // :284, :693
        else st = 0;
        const int now = (st == 0) ? bestIdx : -1;
        const bool changed = now != prev[q];
        prev[q] = now;
        best_idx[Q.idx1] = bestIdx;
        best_dist[Q.idx1] = (unsigned short)bestDist1;
        best_dist2[Q.idx1] = (unsigned short)bestDist2;
        state[Q.idx1] = (unsigned char)st;
        return changed;
    });
    if (tid == 0) B.rounds[blockIdx.x] = n_rounds;
}
