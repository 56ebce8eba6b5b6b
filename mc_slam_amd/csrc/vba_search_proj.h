// vba_search_proj.h -- batched projection matching for tracking on the GPU.
// Replaces, for a batch of (frame, ordered query list) problems, ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
// (src/ORBmatcher.cpp:1511-1665, monocular) and Frame::isInFrustum (src/Frame.cpp:492-550) fused with
// ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cpp:63-156), both over Frame::GetFeaturesInArea
// (src/Frame.cpp:562-620).  The state codes are those of include/vislam_ba.h; the rotation histogram and the writes into mvpMapPoints
// are replayed on the host (vba_host_search_proj.h).
//
// The queries of a problem are NOT independent: a query skips the keypoints an earlier query of the call has claimed (:113-115,
// :1596-1598) and then claims its own (:150, :1623).  One 256-lane workgroup owns a problem; its lanes stride over the queries.
// Phase 1 evaluates the gates and the projection once per query.  Then rounds of a fixed-point iteration run: in a round every
// query still open walks its area against the claim table of the round before -- claim[k] is the smallest index of a blocking
// query (Observations() > 0) whose result is keypoint k, -1 for a keypoint occupied before the call, and query q treats k as taken
// iff claim[k] < q --, then the table is cleared and rebuilt from the new results with an LDS atomic min between barriers.  The
// iteration stops after the first round in which no blocking query changed its keypoint.  Any fixed point is the sequential answer
// (induction on q: query 0 reads no claim, query q reads claims of queries < q only), and after round t (counted from 0) the queries
// 0 .. t are final, so a round only walks the queries q >= t and the loop `round <= n_q` always ends by itself: at round n_q no
// query is left to change.  The walk is repeated each round, not cached: a query's candidates are few, and a cache per query would
// have to live in global memory.  The claim table is n_keys int32 of dynamic LDS (n_keys <= VBA_SP_MAX_KEYS, checked on the host).
// Nothing waits on another workgroup, every loop is bounded by the problem's sizes, every output address is written by one lane
// only.  Plain log, floor, ceil and sqrt in FP64, contraction off so that the operations are the ones the header names; the ratio
// test is one float32 product, as the reference computes it.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"

#define SP_NT VBA_SP_NT
// offsets in SpDesc::c (and in the LDS copy)
#define SP_R 0
#define SP_T 9
#define SP_OW 12
#define SP_K 15
#define SP_B 19
#define SP_GIW 23
#define SP_GIH 24
#define SP_LOGSF 25
#define SP_TH 26
#define SP_COS 27

__global__ void __launch_bounds__(SP_NT) k_search_proj(SpBatch B) {
#pragma clang fp contract(off)
    extern __shared__ int sp_claim[];   // [n_keys of the call's largest frame]
    __shared__ double sc[VBA_SP_CONST];
    const SpDesc& d = B.desc[blockIdx.x];
    const int tid = threadIdx.x;
    const int nk = d.n_keys, nq = d.n_q, nl = d.n_levels;   // nk <= VBA_SP_MAX_KEYS, nl: 1 .. VBA_TRI_LEVELS (checked on the host)
    const bool local = d.mode != 0;
    if (tid < VBA_SP_CONST) sc[tid] = d.c[tid];
    const FuKey* key = B.key + (size_t)d.key0;
    const unsigned char* occupied = B.occupied + (size_t)d.key0;
    const int* cell_begin = B.cell_begin + (size_t)d.cell0;
    const int* cell_feat = B.cell_feat + (size_t)d.feat0;
    const double* scale = B.lev + (size_t)d.lev0;
    const SpQuery* query = B.query + (size_t)d.q0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int k = tid; k < nk; k += SP_NT) sp_claim[k] = occupied[k] ? -1 : 0x7fffffff;
    __syncthreads();

    // phase 1: the gates and the projection, once per query
    for (int q = tid; q < nq; q += SP_NT) {
        const size_t o = (size_t)d.q0 + (size_t)q;
        const SpQuery& Q = query[q];
        int state = 255, level = -128;
        double u = qnan, v = qnan, vc = qnan, r = 0.0;
        do {
            if (Q.skip) { state = 1; break; }
            const double px = Q.pos[0], py = Q.pos[1], pz = Q.pos[2];
            const double xc = ((sc[SP_R + 0] * px + sc[SP_R + 1] * py) + sc[SP_R + 2] * pz) + sc[SP_T + 0];
            const double yc = ((sc[SP_R + 3] * px + sc[SP_R + 4] * py) + sc[SP_R + 5] * pz) + sc[SP_T + 1];
            const double zc = ((sc[SP_R + 6] * px + sc[SP_R + 7] * py) + sc[SP_R + 8] * pz) + sc[SP_T + 2];
            const double invz = 1.0 / zc;
            if (local ? (zc < 0.0) : (invz < 0.0)) { state = 2; break; }                 // Frame.cpp:506, ORBmatcher.cpp:1553
            u = (sc[SP_K + 0] * xc) * invz + sc[SP_K + 2];
            v = (sc[SP_K + 1] * yc) * invz + sc[SP_K + 3];
            // :513-516, :1559-1562; a NaN passes the reference's tests and leaves here (the one deviation)
            if (!(isfinite(u) && isfinite(v)) || u < sc[SP_B + 0] || u > sc[SP_B + 1] || v < sc[SP_B + 2] || v > sc[SP_B + 3]) { state = 3; break; }
            if (!local) {
                r = sc[SP_TH] * scale[Q.oct];                                            // :1567
                break;
            }
            const double ox = px - sc[SP_OW + 0], oy = py - sc[SP_OW + 1], oz = pz - sc[SP_OW + 2];
            const double dist = sqrt((ox * ox + oy * oy) + oz * oz);
            if (dist < Q.dist_min || dist > Q.dist_max) { state = 4; break; }            // Frame.cpp:525
            vc = ((ox * Q.normal[0] + oy * Q.normal[1]) + oz * Q.normal[2]) / dist;
            if (vc < sc[SP_COS]) { state = 5; break; }                                   // Frame.cpp:532
            const double lv = ceil(log(Q.pred_max / dist) / sc[SP_LOGSF]);               // PredictScale
            if (!(lv >= 0.0 && lv < (double)nl)) {                                       // Frame.cpp:537
                state = 6;
                level = (lv >= 127.0) ? 127 : ((lv > -128.0) ? (int)lv : -128);          // NaN gives -128
                break;
            }
            level = (int)lv;
            r = (vc > 0.998) ? 2.5 : 4.0;                                                // RadiusByViewingCos
            if (sc[SP_TH] != 1.0) r = r * sc[SP_TH];                                     // :67, :88
            r = r * scale[level];                                                        // :93
        } while (false);
        B.best_idx[o] = -1;
        B.best_dist[o] = 256;
        B.best_dist2[o] = 256;
        B.level[o] = (signed char)level;
        B.view_cos[o] = (state == 255 || state >= 5) ? vc : qnan;
        B.uv[2 * o] = (state >= 3) ? u : qnan;
        B.uv[2 * o + 1] = (state >= 3) ? v : qnan;
        B.state[o] = (unsigned char)state;
        B.rad[o] = r;
        B.prev[o] = (state == 255) ? -1 : -2;
    }

    // the conflict pass: at most n_q + 1 rounds
    const int cols = d.cols, rows = d.rows, th_high = d.th_high;
    const float nn_ratio = d.nn_ratio;
    int n_rounds = 0;
    for (int round = 0; round <= nq; ++round) {
        int changed = 0;
        for (int q = tid; q < nq; q += SP_NT) {
            const size_t o = (size_t)d.q0 + (size_t)q;
            const int before = B.prev[o];
            if (q < round || before == -2) continue;   // final since round q; never reaches the area
            const SpQuery& Q = query[q];
            const double u = B.uv[2 * o], v = B.uv[2 * o + 1], r = B.rad[o];
            const int lo = local ? (int)B.level[o] - 1 : (int)Q.oct - 1, hi = local ? (int)B.level[o] : (int)Q.oct + 1;
            int bestDist = 256, bestDist2 = 256, bestLevel = -1, bestLevel2 = -1, bestIdx = -1;
            bool any = false;
            do {
                // Frame::GetFeaturesInArea(u, v, r, lo, hi): the cell range in double, clamped as max(0, .) and min(n - 1, .) do
                const double fx0 = floor(((u - sc[SP_B + 0]) - r) * sc[SP_GIW]);
                if (fx0 >= (double)cols) break;
                const double fx1 = ceil(((u - sc[SP_B + 0]) + r) * sc[SP_GIW]);
                if (fx1 < 0.0) break;
                const double fy0 = floor(((v - sc[SP_B + 2]) - r) * sc[SP_GIH]);
                if (fy0 >= (double)rows) break;
                const double fy1 = ceil(((v - sc[SP_B + 2]) + r) * sc[SP_GIH]);
                if (fy1 < 0.0) break;
                const int x0 = (fx0 > 0.0) ? (int)fx0 : 0, x1 = (fx1 < (double)(cols - 1)) ? (int)fx1 : cols - 1;
                const int y0 = (fy0 > 0.0) ? (int)fy0 : 0, y1 = (fy1 < (double)(rows - 1)) ? (int)fy1 : rows - 1;
                if (y1 < y0) break;   // a negative radius: no cell
                const bool check_levels = lo > 0 || hi >= 0;
                unsigned int a[8];
#pragma unroll
                for (int w = 0; w < 8; w++) a[w] = Q.d[w];
                for (int ix = x0; ix <= x1; ix++) {
                    // the cells (ix, y0 .. y1) are neighbours in cell_begin: one range of cell_feat, in the order of the reference's loops
                    const int jb = cell_begin[ix * rows + y0], je = cell_begin[ix * rows + y1 + 1];
                    for (int j = jb; j < je; j++) {
                        const int idx = cell_feat[j];
                        const FuKey& k = key[idx];
                        const int kl = k.oct;
                        if (check_levels) {                                              // Frame.cpp:600-607
                            if (kl < lo) continue;
                            if (hi >= 0 && kl > hi) continue;
                        }
                        if (!(fabs(k.u - u) < r && fabs(k.v - v) < r)) continue;         // Frame.cpp:612
                        any = true;
                        if (sp_claim[idx] < q) continue;                                 // :113-115, :1596-1598
                        int dist = 0;
#pragma unroll
                        for (int w = 0; w < 8; w++) dist += __popc(a[w] ^ k.d[w]);
                        if (dist < bestDist) {                                           // :129-141, :1613
                            bestDist2 = bestDist; bestDist = dist;
                            bestLevel2 = bestLevel; bestLevel = kl;
                            bestIdx = idx;
                        } else if (dist < bestDist2) {
                            bestLevel2 = kl; bestDist2 = dist;
                        }
                    }
                }
            } while (false);
            int state;
            if (!any) state = local ? 7 : 4;                                             // :96, :1582
            else if (!(bestDist <= th_high && bestIdx >= 0)) state = local ? 8 : 5;      // :145, :1621
            else if (local && bestLevel == bestLevel2 && (float)bestDist > nn_ratio * (float)bestDist2) state = 9;   // :147
            else state = 0;
            const int now = (state == 0 && Q.blocks) ? bestIdx : -1;
            changed |= now != before;
            B.prev[o] = now;
            B.best_idx[o] = bestIdx;
            B.best_dist[o] = (unsigned short)bestDist;
            B.best_dist2[o] = (unsigned short)(local ? bestDist2 : 256);
            B.state[o] = (unsigned char)state;
        }
        changed = __syncthreads_or(changed);   // every walk of the round has read the table
        n_rounds = round + 1;
        if (!changed) break;
        for (int k = tid; k < nk; k += SP_NT) sp_claim[k] = occupied[k] ? -1 : 0x7fffffff;
        __syncthreads();
        for (int q = tid; q < nq; q += SP_NT) {
            const int c = B.prev[(size_t)d.q0 + (size_t)q];
            if (c >= 0) atomicMin(&sp_claim[c], q);
        }
        __syncthreads();
    }
    if (tid == 0) B.rounds[blockIdx.x] = n_rounds;
}
