// vba_search_sim3.h -- batched Sim3 projection matching for loop candidates on the GPU.
// Replaces, for a batch of keyframe pairs, both projection searches of ORBmatcher::SearchBySim3 (src/ORBmatcher.cpp:1310-1392 and
// :1398-1475, monocular) with KeyFrame::GetFeaturesInArea (src/KeyFrame.cpp:1071-1115), IsInImage and MapPoint::PredictScale
// (src/MapPoint.cpp:529-540).  The agreement loop (:1480-1493) needs both directions complete and runs on the host in the write-back
// (vba_host_search_sim3.h).  The state codes are those of include/vislam_ba.h.
//
// A query is a keypoint of the source keyframe with a usable map point and no prior match; the host compacts them, so the states 1
// and 2 never reach the device.  Queries are independent and every output is per query, so the host lays out a flat table of tiles
// (pair, direction, first query), at most 256 queries each, and the grid is one 256-lane workgroup per tile, ONE launch.
// What the lanes of a tile SHARE: the pair and the direction, hence the 36 constants of the direction (source pose, the Sim3 into the
// target camera, K, the target's bounds and cell sizes, log scale factor, th) and the target's scale table, both staged in LDS once
// per workgroup, and the target's keypoint records, cell_begin and cell_feat, which stay in global memory, one copy per keyframe.
// What they do NOT share: a lane owns one query, its 96-byte SsQuery record is read once, the descriptor lives in 8 VGPRs, and the
// lane writes its own four outputs at the query's offset; no lane reads what another wrote.  The geometry gates come first, then
// the cell walk of GetFeaturesInArea runs sequentially inside the lane (sa_walk, vba_search_area.h: the order, the bounds of its
// loops and the helpers shared with the other matchers).  A target keypoint is one 64-byte FuKey record; a candidate that cannot
// beat bestDist never has its second half read once the area is known to hold a keypoint (every test of a candidate is a plain
// `return` of the visitor, so their order is free).  No atomics, nothing waits on another workgroup, every output address is
// written by exactly one lane.  Plain log, floor, ceil and sqrt in FP64, contraction off.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_search_area.h"

#define SS_NT VBA_SS_NT
// offsets in SsDir::c (and in the LDS copy)
#define SS_RS 0
#define SS_TS 9
#define SS_SR 12
#define SS_T 21
#define SS_K 24
#define SS_TB 28   // the target block (SA_B .. SA_TH, vba_search_area.h)

__global__ void __launch_bounds__(SS_NT) k_search_sim3(SsBatch B) {
#pragma clang fp contract(off)
    __shared__ double sc[VBA_SS_CONST];
    __shared__ double s_scale[VBA_TRI_LEVELS];
    const SsTile t = B.tile[blockIdx.x];
    const SsDir& d = B.dir[2 * (size_t)t.pair + (size_t)t.dir];
    const int tid = threadIdx.x;
    const int nl = d.n_levels;   // 1 .. VBA_TRI_LEVELS (checked on the host)
    if (tid < VBA_SS_CONST) sc[tid] = d.c[tid];
    if (tid < nl) s_scale[tid] = B.lev[(size_t)d.lev0 + tid];
    __syncthreads();
    const int iq = t.first + tid;
    if (iq >= d.n_q) return;
    const double* tb = sc + SS_TB;
    const SaGrid grid = {B.key + (size_t)d.key0, B.cell_begin + (size_t)d.cell0, B.cell_feat + (size_t)d.feat0, d.cols, d.rows};
    const size_t o = (size_t)d.q0 + (size_t)iq;
    const SsQuery& Q = B.query[o];

    int state, bestIdx = -1, bestDist = 256, level = -128;
    do {
        // the point in the source camera (:1321), then through the Sim3 into the target camera (:1322)
        double xs, ys, zs, xc, yc, zc;
        sa_rigid(sc + SS_RS, sc + SS_TS, Q.pos[0], Q.pos[1], Q.pos[2], xs, ys, zs);
        sa_rigid(sc + SS_SR, sc + SS_T, xs, ys, zs, xc, yc, zc);
        if (zc < 0.0) { state = 3; break; }                                              // :1325
        const double invz = 1.0 / zc;
        const double u = sc[SS_K + 0] * (xc * invz) + sc[SS_K + 2];
        const double v = sc[SS_K + 1] * (yc * invz) + sc[SS_K + 3];
        if (!(u >= tb[SA_B + 0] && u < tb[SA_B + 1] && v >= tb[SA_B + 2] && v < tb[SA_B + 3])) { state = 4; break; }   // :1337
        const double dist3D = sqrt((xc * xc + yc * yc) + zc * zc);
        if (dist3D < Q.dist_min || dist3D > Q.dist_max) { state = 5; break; }            // :1345
        // the deviation: :1354 reads the scale table unchecked
        if (!sa_predict_level(Q.pred_max, dist3D, tb[SA_LOGSF], nl, level)) { state = 6; break; }
        const double r = tb[SA_TH] * s_scale[level];                                     // :1354
        state = 7;
        unsigned int a[8];
        sa_load_desc(a, Q.d);
        bool any = false;
        sa_walk(grid, tb, u, v, r, [&](int idx, const FuKey& k) {
            const int dist = sa_hamming(a, k.d);
            if (any && dist >= bestDist) return;                                         // :1381, ahead of the tests it cannot change
            if (!(fabs(k.u - u) < r && fabs(k.v - v) < r)) return;                       // KeyFrame.cpp:1107
            any = true;
            const int kl = k.oct;
            if (kl < level - 1 || kl > level) return;                                    // :1374
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }                     // :1381
        });
        if (!any) break;                                                                  // :1359
        state = (bestIdx >= 0 && bestDist <= d.th_high) ? 0 : 8;                         // :1388
    } while (false);
    B.match[o] = (state == 0) ? bestIdx : -1;
    B.best_dist[o] = (unsigned short)bestDist;
    B.level[o] = (signed char)level;
    B.state[o] = (unsigned char)state;
}
