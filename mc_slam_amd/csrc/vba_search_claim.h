// vba_search_claim.h -- the conflict pass of the ordered matchers (k_search_proj, k_search_proj_kf, k_search_bow), written once.
// In an ordered matcher the queries of a problem are NOT independent: a query skips the keypoints an earlier query of the call has
// taken and then takes its own.  One workgroup of NT lanes owns a problem, its lanes stride over the queries, and the claim table
// lives in its LDS: claim[k] is the smallest index of a query whose current result takes keypoint k, -1 for a keypoint that is
// statically taken (occupied before the call, or no candidate at all), INT_MAX otherwise, and query q treats k as taken iff
// claim[k] < q.
//
// The pass is a fixed-point iteration.  In a round every query still open is visited: the kernel's visitor walks the query's
// candidates against the table of the round before, writes its outputs and the query's new claim, and says whether the claim
// changed.  __syncthreads_or then joins the answers -- behind it every walk of the round has read the table --, and if any claim
// changed the table is reset and rebuilt from the new claims with an LDS atomic min between two barriers.  The pass stops after the
// first round in which no claim changed: the table the next round would read equals the one this round read, so every result stands.
//
// Why the result is the sequential one: any fixed point is the sequential answer, by induction on q -- query 0 reads no claim (no
// entry is < 0 but the static -1), and query q reads claims of queries < q only, which are the sequential ones by hypothesis.
// Why it ends: after round t (counted from 0) the queries 0 .. t are final, by the same induction -- in round t query t reads the
// table rebuilt after round t - 1, in which every query < t has its final claim.  So a visitor may skip q < round, and at round n_q
// no query is left to change: `round <= last_round` with last_round = n_q always ends by itself, after at most n_q + 1 rounds.  A
// kernel that knows a tighter bound passes it (k_search_bow: the node-local bound, vba_search_bow.h).
//
// Who may read what.  The table is read by the visitors only, and written only between the barriers here.  The claim of a query
// (the kernel's prev slot) is written by the lane that visits the query and read by that lane alone -- in the visitor, for
// `changed`, and in the rebuild through claim_of --, so it needs no barrier of its own.  The helpers use no LDS besides what
// __syncthreads_or uses, add no barrier to the ones named above, and are forced inline with the kernel's callables, so the
// kernel's state stays in registers.  Nothing waits on another workgroup, and every loop is bounded by the problem's sizes.
#pragma once
#include "vba_device.h"

// the table before any claim, and a barrier.  taken(k): keypoint k is statically taken
template <int NT, class Taken>
DEVI void claim_reset(int* claim, int n_keys, Taken&& taken) {
    for (int k = threadIdx.x; k < n_keys; k += NT) claim[k] = taken(k) ? -1 : 0x7fffffff;
    __syncthreads();
}

// The rounds 0 .. last_round over a table that claim_reset has set; returns the number of rounds run.  visit(q, round): walk query q
// (or skip it) and return whether its claim changed; claim_of(q): the keypoint q claims now, < 0 for none
template <int NT, class Taken, class ClaimOf, class Visit>
DEVI int claim_rounds(int* claim, int n_keys, int n_q, int last_round, Taken&& taken, ClaimOf&& claim_of, Visit&& visit) {
    int n_rounds = 0;
    for (int round = 0; round <= last_round; ++round) {
        int changed = 0;
        for (int q = threadIdx.x; q < n_q; q += NT) changed |= visit(q, round) ? 1 : 0;
        changed = __syncthreads_or(changed);   // every walk of the round has read the table
        n_rounds = round + 1;
        if (!changed) break;
        claim_reset<NT>(claim, n_keys, taken);
        for (int q = threadIdx.x; q < n_q; q += NT) {
            const int c = claim_of(q);
            if (c >= 0) atomicMin(&claim[c], q);
        }
        __syncthreads();
    }
    return n_rounds;
}
