// vba_search_proj.h -- batched projection matching for tracking on the GPU.
// Replaces, for a batch of (frame, ordered query list) problems, ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono)
// (src/ORBmatcher.cpp:1511-1665, monocular) and Frame::isInFrustum (src/Frame.cpp:492-550) fused with
// ORBmatcher::SearchByProjection(F, vpMapPoints, th) (src/ORBmatcher.cpp:63-156), both over Frame::GetFeaturesInArea
// (src/Frame.cpp:562-620).  The state codes are those of include/vislam_ba.h; the rotation histogram and the writes into mvpMapPoints
// are replayed on the host (vba_host_search_proj.h).
//
// The queries of a problem are NOT independent: a query skips the keypoints an earlier query of the call has claimed (:113-115,
// :1596-1598) and then claims its own (:150, :1623).  One 256-lane workgroup owns a problem; its lanes stride over the queries.
// Phase 1 evaluates the gates and the projection once per query.  Then the conflict pass of vba_search_claim.h runs (the protocol,
// its proof and the bound of n_q + 1 rounds are there): only a blocking query (Observations() > 0) claims its keypoint, a keypoint
// occupied before the call is statically taken, and the visitor skips a query that never reaches the area.  The walk is repeated each
// round, not cached: a query's candidates are few, and a cache per query would have to live in global memory.  The claim table is
// n_keys int32 of dynamic LDS (n_keys <= VBA_SP_MAX_KEYS, checked on the host).  Every output address is written by one lane only.
// Plain log, floor, ceil and sqrt in FP64, contraction off so that the operations are the ones the header names; the ratio test is
// one float32 product, as the reference computes it.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_search_area.h"
#include "vba_search_claim.h"

#define SP_NT VBA_SP_NT   // SpDesc::c is the camera block (SA_*, vba_search_area.h)

__global__ void __launch_bounds__(SP_NT) k_search_proj(SpBatch B) {
#pragma clang fp contract(off)
    extern __shared__ int sp_claim[];   // [n_keys of the call's largest frame]
    __shared__ double sc[VBA_SP_CONST];
    const SpDesc& d = B.desc[blockIdx.x];
    const int tid = threadIdx.x;
    const int nk = d.n_keys, nq = d.n_q, nl = d.n_levels;   // nk <= VBA_SP_MAX_KEYS, nl: 1 .. VBA_TRI_LEVELS (checked on the host)
    const bool local = d.mode != 0;
    if (tid < VBA_SP_CONST) sc[tid] = d.c[tid];
    const double* tb = sc + SA_TB;
    const SaGrid grid = {B.key + (size_t)d.key0, B.cell_begin + (size_t)d.cell0, B.cell_feat + (size_t)d.feat0, d.cols, d.rows};
    const unsigned char* occupied = B.occupied + (size_t)d.key0;
    const double* scale = B.lev + (size_t)d.lev0;
    const SpQuery* query = B.query + (size_t)d.q0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const auto taken = [&](int k) { return occupied[k] != 0; };
    claim_reset<SP_NT>(sp_claim, nk, taken);

    // phase 1: the gates and the projection, once per query
    for (int q = tid; q < nq; q += SP_NT) {
        const size_t o = (size_t)d.q0 + (size_t)q;
        const SpQuery& Q = query[q];
        int state = 255, level = -128;
        double u = qnan, v = qnan, vc = qnan, r = 0.0;
        do {
            if (Q.skip) { state = 1; break; }
            const double px = Q.pos[0], py = Q.pos[1], pz = Q.pos[2];
            double xc, yc, zc;
            sa_rigid(sc + SA_R, sc + SA_T, px, py, pz, xc, yc, zc);
            const double invz = 1.0 / zc;
            if (local ? (zc < 0.0) : (invz < 0.0)) { state = 2; break; }                 // Frame.cpp:506, ORBmatcher.cpp:1553
            u = (sc[SA_K + 0] * xc) * invz + sc[SA_K + 2];
            v = (sc[SA_K + 1] * yc) * invz + sc[SA_K + 3];
            // :513-516, :1559-1562; a NaN passes the reference's tests and leaves here (the one deviation)
            if (!(isfinite(u) && isfinite(v)) || u < tb[SA_B + 0] || u > tb[SA_B + 1] || v < tb[SA_B + 2] || v > tb[SA_B + 3]) { state = 3; break; }
            if (!local) {
                r = tb[SA_TH] * scale[Q.oct];                                            // :1567
                break;
            }
            const double ox = px - sc[SA_OW + 0], oy = py - sc[SA_OW + 1], oz = pz - sc[SA_OW + 2];
            const double dist = sqrt((ox * ox + oy * oy) + oz * oz);
            if (dist < Q.dist_min || dist > Q.dist_max) { state = 4; break; }            // Frame.cpp:525
            vc = ((ox * Q.normal[0] + oy * Q.normal[1]) + oz * Q.normal[2]) / dist;
            if (vc < sc[SA_COS]) { state = 5; break; }                                   // Frame.cpp:532
            if (!sa_predict_level(Q.pred_max, dist, tb[SA_LOGSF], nl, level)) { state = 6; break; }   // Frame.cpp:537
            r =(vc > 0.998) ? 2.5 : 4.0;                                                // RadiusByViewingCos
            if (tb[SA_TH] != 1.0) r = r * tb[SA_TH];                                     // :67, :88
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

    // the conflict pass: at most n_q + 1 rounds.  The visitor walks one query against the table of the round before
    const int th_high = d.th_high;
    const float nn_ratio = d.nn_ratio;
    const auto claim_of = [&](int q) { return B.prev[(size_t)d.q0 + (size_t)q]; };
    const int n_rounds = claim_rounds<SP_NT>(sp_claim, nk, nq, nq, taken, claim_of, [&](int q, int round) {
        const size_t o = (size_t)d.q0 + (size_t)q;
        const int before = B.prev[o];
        if (q < round || before == -2) return false;   // final since round q; never reaches the area
        const SpQuery& Q = query[q];
        const double u = B.uv[2 * o], v = B.uv[2 * o + 1], r = B.rad[o];
        const int lo = local ? (int)B.level[o] - 1 : (int)Q.oct - 1, hi = local ? (int)B.level[o] : (int)Q.oct + 1;
        int bestDist = 256, bestDist2 = 256, bestLevel = -1, bestLevel2 = -1, bestIdx = -1;
        bool any = false;
        const bool check_levels = lo > 0 || hi >= 0;
        unsigned int a[8];
        sa_load_desc(a, Q.d);
        // Frame::GetFeaturesInArea(u, v, r, lo, hi)
        sa_walk(grid, tb, u, v, r, [&](int idx, const FuKey& k) {
            const int kl = k.oct;
            if (check_levels) {                                                      // Frame.cpp:600-607
                if (kl < lo) return;
                if (hi >= 0 && kl > hi) return;
            }
            if (!(fabs(k.u - u) < r && fabs(k.v - v) < r)) return;                   // Frame.cpp:612
            any = true;
            if (sp_claim[idx] < q) return;                                           // :113-115, :1596-1598
            const int dist = sa_hamming(a, k.d);
            if (dist < bestDist) {                                                   // :129-141, :1613
                bestDist2 = bestDist; bestDist = dist;
                bestLevel2 = bestLevel; bestLevel = kl;
                bestIdx = idx;
            } else if (dist < bestDist2) {
                bestLevel2 = kl; bestDist2 = dist;
            }
        });
        int state;
        if (!any) state = local ? 7 : 4;                                             // :96, :1582
        else if (!(bestDist <= th_high && bestIdx >= 0)) state = local ? 8 : 5;      // :145, :1621
        else if (local && bestLevel == bestLevel2 && (float)bestDist > nn_ratio * (float)bestDist2) state = 9;   // :147
        else state = 0;
        const int now = (state == 0 && Q.blocks) ? bestIdx : -1;
        B.prev[o] = now;
        B.best_idx[o] = bestIdx;
        B.best_dist[o] = (unsigned short)bestDist;
        B.best_dist2[o] = (unsigned short)(local ? bestDist2 : 256);
        B.state[o] = (unsigned char)state;
        return now != before;
    });
    if (tid == 0) B.rounds[blockIdx.x] = n_rounds;
}
