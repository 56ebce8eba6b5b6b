// vba_fuse.h -- batched projection search for map-point fusion on the GPU.
// Replaces, for a batch of (keyframe, point list) problems, the search half of both ORBmatcher::Fuse overloads
// (src/ORBmatcher.cpp:986-1092 and :1157-1231, monocular) with KeyFrame::GetFeaturesInArea (src/KeyFrame.cpp:1071-1115), IsInImage
// and MapPoint::PredictScale (src/MapPoint.cpp:529-540).  The apply loops (:1095-1115, :1234-1250) stay with the caller.  The state
// codes are those of include/vislam_ba.h.
//
// Points are independent and every output is per point, so a problem is not tied to a workgroup: the host lays out a flat table of
// tiles (problem, first point), at most 256 points each, and the grid is one 256-lane workgroup per tile, ONE launch.  A lane owns
// one point: its 128-byte FuPoint record is read once, the descriptor lives in 8 VGPRs, the geometry gates come first, then the
// cell walk of GetFeaturesInArea runs sequentially inside the lane exactly as written (ix outer, iy inner, list order inside a
// cell), so the strict `dist < bestDist` keeps the first of equal distances without code of its own.  A keypoint is one 64-byte
// FuKey record; its first half brings the descriptor, and once the area is known to hold a keypoint a candidate that cannot beat
// bestDist never has its second half read (every test of a candidate is a plain `continue`, so their order is free).  The
// problem's constants and level tables are staged in LDS once per workgroup; cell_begin and cell_feat stay in global memory, one
// copy per problem.  No atomics, nothing waits on another workgroup, every loop is bounded by the problem's sizes (the cell range
// is clamped to the grid, a cell's range is checked on the host), every output address is written by exactly one lane.  Plain
// log, floor, ceil and sqrt in FP64, contraction off in the gates so that they are the operations the header names.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"

#define FU_NT VBA_FU_NT
// offsets in FuDesc::c (and in the LDS copy)
#define FU_R 0
#define FU_T 9
#define FU_OW 12
#define FU_K 15
#define FU_B 19
#define FU_GIW 23
#define FU_GIH 24
#define FU_LOGSF 25
#define FU_TH 26
#define FU_COS 27
#define FU_CHI2 28

__global__ void __launch_bounds__(FU_NT) k_fuse(FuBatch B) {
#pragma clang fp contract(off)
    __shared__ double sc[VBA_FU_CONST];
    __shared__ double slev[2 * VBA_TRI_LEVELS];
    const FuTile t = B.tile[blockIdx.x];
    const FuDesc& d = B.desc[t.prob];
    const int tid = threadIdx.x;
    const int nl = d.n_levels;   // 1 .. VBA_TRI_LEVELS (checked on the host)
    if (tid < VBA_FU_CONST) sc[tid] = d.c[tid];
    if (tid < 2 * nl) slev[tid] = B.lev[(size_t)d.lev0 + tid];
    __syncthreads();
    const int ip = t.first + tid;
    if (ip >= d.n_pt) return;
    const double* s_scale = slev;
    const double* s_inv_sigma2 = slev + nl;
    const FuKey* key = B.key + (size_t)d.key0;
    const int* cell_begin = B.cell_begin + (size_t)d.cell0;
    const int* cell_feat = B.cell_feat + (size_t)d.feat0;
    const size_t o = (size_t)d.pt0 + (size_t)ip;
    const FuPoint& P = B.pt[o];
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    int state, bestIdx = -1, bestDist = 256, level = -128;
    double u = qnan, v = qnan;
    do {
        if (P.skip) { state = 1; break; }
        const double px = P.pos[0], py = P.pos[1], pz = P.pos[2];
        const double xc = ((sc[FU_R + 0] * px + sc[FU_R + 1] * py) + sc[FU_R + 2] * pz) + sc[FU_T + 0];
        const double yc = ((sc[FU_R + 3] * px + sc[FU_R + 4] * py) + sc[FU_R + 5] * pz) + sc[FU_T + 1];
        const double zc = ((sc[FU_R + 6] * px + sc[FU_R + 7] * py) + sc[FU_R + 8] * pz) + sc[FU_T + 2];
        if (zc < 0.0) { state = 2; break; }                                              // :991
        const double invz = 1.0 / zc;
        u = sc[FU_K + 0] * (xc * invz) + sc[FU_K + 2];
        v = sc[FU_K + 1] * (yc * invz) + sc[FU_K + 3];
        if (!(u >= sc[FU_B + 0] && u < sc[FU_B + 1] && v >= sc[FU_B + 2] && v < sc[FU_B + 3])) { state = 3; break; }   // :1004
        const double ox = px - sc[FU_OW + 0], oy = py - sc[FU_OW + 1], oz = pz - sc[FU_OW + 2];
        const double dist3D = sqrt((ox * ox + oy * oy) + oz * oz);
        if (dist3D < P.dist_min || dist3D > P.dist_max) { state = 4; break; }            // :1016
        const double dot = (ox * P.normal[0] + oy * P.normal[1]) + oz * P.normal[2];
        if (dot < sc[FU_COS] * dist3D) { state = 5; break; }                             // :1023
        const double lv = ceil(log(P.pred_max / dist3D) / sc[FU_LOGSF]);                 // PredictScale
        if (!(lv >= 0.0 && lv < (double)nl)) {                                           // :1027
            state = 6;
            level = (lv >= 127.0) ? 127 : ((lv > -128.0) ? (int)lv : -128);              // NaN gives -128
            break;
        }
        level = (int)lv;
        const double r = sc[FU_TH] * s_scale[level];                                     // :1031
        // GetFeaturesInArea(u, v, r): the cell range in double, clamped as max(0, .) and min(n - 1, .) do
        const int cols = d.cols, rows = d.rows;
        state = 7;
        const double fx0 = floor(((u - sc[FU_B + 0]) - r) * sc[FU_GIW]);
        if (fx0 >= (double)cols) break;
        const double fx1 = ceil(((u - sc[FU_B + 0]) + r) * sc[FU_GIW]);
        if (fx1 < 0.0) break;
        const double fy0 = floor(((v - sc[FU_B + 2]) - r) * sc[FU_GIH]);
        if (fy0 >= (double)rows) break;
        const double fy1 = ceil(((v - sc[FU_B + 2]) + r) * sc[FU_GIH]);
        if (fy1 < 0.0) break;
        const int x0 = (fx0 > 0.0) ? (int)fx0 : 0, x1 = (fx1 < (double)(cols - 1)) ? (int)fx1 : cols - 1;
        const int y0 = (fy0 > 0.0) ? (int)fy0 : 0, y1 = (fy1 < (double)(rows - 1)) ? (int)fy1 : rows - 1;
        unsigned int a[8];
#pragma unroll
        for (int w = 0; w < 8; w++) a[w] = P.d[w];
        const bool check_reproj = d.check_reproj != 0;
        const double chi2 = sc[FU_CHI2];
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
                if (any && dist >= bestDist) continue;                                   // :1087, ahead of the tests it cannot change
                const double ku = k.u, kv = k.v;
                if (!(fabs(ku - u) < r && fabs(kv - v) < r)) continue;                   // KeyFrame.cpp:1107
                any = true;
                const int kl = k.oct;
                if (kl < level - 1 || kl > level) continue;                              // :1052
                if (check_reproj) {
                    const double ex = u - ku, ey = v - kv;
                    if ((ex * ex + ey * ey) * s_inv_sigma2[kl] > chi2) continue;         // :1079
                }
                if (dist < bestDist) { bestDist = dist; bestIdx = idx; }                 // :1087
            }
        }
        if (!any) break;                                                                  // :1034
        state = (bestDist <= d.th_low) ? 0 : 8;                                          // :1095
    } while (false);
    B.best_idx[o] = bestIdx;
    B.best_dist[o] = (unsigned short)bestDist;
    B.level[o] = (signed char)level;
    B.uv[2 * o] = (state >= 3 || state == 0) ? u : qnan;
    B.uv[2 * o + 1] = (state >= 3 || state == 0) ? v : qnan;
    B.state[o] = (unsigned char)state;
}
