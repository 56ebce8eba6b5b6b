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
// the cell walk of GetFeaturesInArea runs sequentially inside the lane exactly as written (ix outer, iy inner, list order inside a
// cell), so the strict `dist < bestDist` keeps the first of equal distances without code of its own.  A target keypoint is one
// 64-byte FuKey record; a candidate that cannot beat bestDist never has its second half read once the area is known to hold a
// keypoint (every test of a candidate is a plain `continue`, so their order is free).  No atomics, nothing waits on another
// workgroup, every loop is bounded by sizes the host checked (the cell range is clamped to the grid, a cell's range is checked on
// the host), every output address is written by exactly one lane.  Plain log, floor, ceil and sqrt in FP64, contraction off.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"

#define SS_NT VBA_SS_NT
// offsets in SsDir::c (and in the LDS copy)
#define SS_RS 0
#define SS_TS 9
#define SS_SR 12
#define SS_T 21
#define SS_K 24
#define SS_B 28
#define SS_GIW 32
#define SS_GIH 33
#define SS_LOGSF 34
#define SS_TH 35

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
    const FuKey* key = B.key + (size_t)d.key0;
    const int* cell_begin = B.cell_begin + (size_t)d.cell0;
    const int* cell_feat = B.cell_feat + (size_t)d.feat0;
    const size_t o = (size_t)d.q0 + (size_t)iq;
    const SsQuery& Q = B.query[o];

    int state, bestIdx = -1, bestDist = 256, level = -128;
    do {
        const double px = Q.pos[0], py = Q.pos[1], pz = Q.pos[2];
        // the point in the source camera (:1321), then through the Sim3 into the target camera (:1322)
        const double xs = ((sc[SS_RS + 0] * px + sc[SS_RS + 1] * py) + sc[SS_RS + 2] * pz) + sc[SS_TS + 0];
        const double ys = ((sc[SS_RS + 3] * px + sc[SS_RS + 4] * py) + sc[SS_RS + 5] * pz) + sc[SS_TS + 1];
        const double zs = ((sc[SS_RS + 6] * px + sc[SS_RS + 7] * py) + sc[SS_RS + 8] * pz) + sc[SS_TS + 2];
        const double xc = ((sc[SS_SR + 0] * xs + sc[SS_SR + 1] * ys) + sc[SS_SR + 2] * zs) + sc[SS_T + 0];
        const double yc = ((sc[SS_SR + 3] * xs + sc[SS_SR + 4] * ys) + sc[SS_SR + 5] * zs) + sc[SS_T + 1];
        const double zc = ((sc[SS_SR + 6] * xs + sc[SS_SR + 7] * ys) + sc[SS_SR + 8] * zs) + sc[SS_T + 2];
        if (zc < 0.0) { state = 3; break; }                                              // :1325
        const double invz = 1.0 / zc;
        const double u = sc[SS_K + 0] * (xc * invz) + sc[SS_K + 2];
        const double v = sc[SS_K + 1] * (yc * invz) + sc[SS_K + 3];
        if (!(u >= sc[SS_B + 0] && u < sc[SS_B + 1] && v >= sc[SS_B + 2] && v < sc[SS_B + 3])) { state = 4; break; }   // :1337
        const double dist3D = sqrt((xc * xc + yc * yc) + zc * zc);
        if (dist3D < Q.dist_min || dist3D > Q.dist_max) { state = 5; break; }            // :1345
        const double lv = ceil(log(Q.pred_max / dist3D) / sc[SS_LOGSF]);                 // PredictScale
        if (!(lv >= 0.0 && lv < (double)nl)) {                                           // the deviation: :1354 reads unchecked
            state = 6;
            level = (lv >= 127.0) ? 127 : ((lv > -128.0) ? (int)lv : -128);              // NaN gives -128
            break;
        }
        level = (int)lv;
        const double r = sc[SS_TH] * s_scale[level];                                     // :1354
        // GetFeaturesInArea(u, v, r): the cell range in double, clamped as max(0, .) and min(n - 1, .) do
        const int cols = d.cols, rows = d.rows;
        state = 7;
        const double fx0 = floor(((u - sc[SS_B + 0]) - r) * sc[SS_GIW]);
        if (fx0 >= (double)cols) break;
        const double fx1 = ceil(((u - sc[SS_B + 0]) + r) * sc[SS_GIW]);
        if (fx1 < 0.0) break;
        const double fy0 = floor(((v - sc[SS_B + 2]) - r) * sc[SS_GIH]);
        if (fy0 >= (double)rows) break;
        const double fy1 = ceil(((v - sc[SS_B + 2]) + r) * sc[SS_GIH]);
        if (fy1 < 0.0) break;
        const int x0 = (fx0 > 0.0) ? (int)fx0 : 0, x1 = (fx1 < (double)(cols - 1)) ? (int)fx1 : cols - 1;
        const int y0 = (fy0 > 0.0) ? (int)fy0 : 0, y1 = (fy1 < (double)(rows - 1)) ? (int)fy1 : rows - 1;
        unsigned int a[8];
#pragma unroll
        for (int w = 0; w < 8; w++) a[w] = Q.d[w];
        bool any = false;
        for (int ix = x0; ix <= x1; ix++) {
            // the cells (ix, y0 .. y1) are neighbours in cell_begin: one range of cell_feat, in the order of the reference's two loops
            const int jb = cell_begin[ix * rows + y0], je = cell_begin[ix * rows + y1 + 1];
            for (int j = jb; j < je; j++) {
                const int idx = cell_feat[j];
                const FuKey& k = key[idx];
                int dist = 0;
#pragma unroll
                for (int w = 0; w < 8; w++) dist += __popc(a[w] ^ k.d[w]);
                if (any && dist >= bestDist) continue;                                   // :1381, ahead of the tests it cannot change
                if (!(fabs(k.u - u) < r && fabs(k.v - v) < r)) continue;                 // KeyFrame.cpp:1107
                any = true;
                const int kl = k.oct;
                if (kl < level - 1 || kl > level) continue;                              // :1374
                if (dist < bestDist) { bestDist = dist; bestIdx = idx; }                 // :1381
            }
        }
        if (!any) break;                                                                  // :1359
        state = (bestIdx >= 0 && bestDist <= d.th_high) ? 0 : 8;                         // :1388
    } while (false);
    B.match[o] = (state == 0) ? bestIdx : -1;
    B.best_dist[o] = (unsigned short)bestDist;
    B.level[o] = (signed char)level;
    B.state[o] = (unsigned char)state;
}
