// vba_fuse.h -- batched projection search for map-point fusion on the GPU.
// Replaces, for a batch of (keyframe, point list) problems, the search half of both ORBmatcher::Fuse overloads
// (src/ORBmatcher.cpp:986-1092 and :1157-1231, monocular) with KeyFrame::GetFeaturesInArea (src/KeyFrame.cpp:1071-1115), IsInImage
// and MapPoint::PredictScale (src/MapPoint.cpp:529-540).  The apply loops (:1095-1115, :1234-1250) stay with the caller.  The state
// codes are those of include/vislam_ba.h.
//
// Points are independent and every output is per point, so a problem is not tied to a workgroup: the host lays out a flat table of
// tiles (problem, first point), at most 256 points each, and the grid is one 256-lane workgroup per tile, ONE launch.  A lane owns
// one point: its 128-byte FuPoint record is read once, the descriptor lives in 8 VGPRs, the geometry gates come first, then the
// cell walk of GetFeaturesInArea runs sequentially inside the lane (sa_walk, vba_search_area.h: the order, the bounds of its loops
// and the helpers shared with the other matchers).  A keypoint is one 64-byte FuKey record; its first half brings the descriptor,
// and once the area is known to hold a keypoint a candidate that cannot beat bestDist never has its second half read (every test of
// a candidate is a plain `return` of the visitor, so their order is free).  The problem's constants and level tables are staged in
// LDS once per workgroup; cell_begin and cell_feat stay in global memory, one copy per problem.  No atomics, nothing waits on
// another workgroup, every output address is written by exactly one lane.  Plain log, floor, ceil and sqrt in FP64, contraction
// off in the gates so that they are the operations the header names.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_search_area.h"

#define FU_NT VBA_FU_NT
#define FU_CHI2 28   // in FuDesc::c behind the camera block (SA_*, vba_search_area.h)

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
    const double* tb = sc + SA_TB;
    const SaGrid grid = {B.key + (size_t)d.key0, B.cell_begin + (size_t)d.cell0, B.cell_feat + (size_t)d.feat0, d.cols, d.rows};
    const size_t o = (size_t)d.pt0 + (size_t)ip;
    const FuPoint& P = B.pt[o];
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);

    int state, bestIdx = -1, bestDist = 256, level = -128;
    double u = qnan, v = qnan;
    do {
        if (P.skip) { state = 1; break; }
        const double px = P.pos[0], py = P.pos[1], pz = P.pos[2];
        double xc, yc, zc;
        sa_rigid(sc + SA_R, sc + SA_T, px, py, pz, xc, yc, zc);
        if (zc < 0.0) { state = 2; break; }                                              // :991
        const double invz = 1.0 / zc;
        u = sc[SA_K + 0] * (xc * invz) + sc[SA_K + 2];
        v = sc[SA_K + 1] * (yc * invz) + sc[SA_K + 3];
        if (!(u >= tb[SA_B + 0] && u < tb[SA_B + 1] && v >= tb[SA_B + 2] && v < tb[SA_B + 3])) { state = 3; break; }   // :1004
        const double ox = px - sc[SA_OW + 0], oy = py - sc[SA_OW + 1], oz = pz - sc[SA_OW + 2];
        const double dist3D = sqrt((ox * ox + oy * oy) + oz * oz);
        if (dist3D < P.dist_min || dist3D > P.dist_max) { state = 4; break; }            // :1016
        const double dot = (ox * P.normal[0] + oy * P.normal[1]) + oz * P.normal[2];
        if (dot < sc[SA_COS] * dist3D) { state = 5; break; }                             // :1023
        if (!sa_predict_level(P.pred_max, dist3D, tb[SA_LOGSF], nl, level)) { state = 6; break; }   // :1027
        const double r = tb[SA_TH] * s_scale[level];                                     // :1031
        state = 7;
        unsigned int a[8];
        sa_load_desc(a, P.d);
        const bool check_reproj = d.check_reproj != 0;
        const double chi2 = sc[FU_CHI2];
        bool any = false;
        sa_walk(grid, tb, u, v, r, [&](int idx, const FuKey& k) {
#pragma clang fp contract(off)
            const int dist = sa_hamming(a, k.d);
            if (any && dist >= bestDist) return;                                         // :1087, ahead of the tests it cannot change
            const double ku = k.u, kv = k.v;
            if (!(fabs(ku - u) < r && fabs(kv - v) < r)) return;                         // KeyFrame.cpp:1107
            any = true;
            const int kl = k.oct;
            if (kl < level - 1 || kl > level) return;                                    // :1052
            if (check_reproj) {
                const double ex = u - ku, ey = v - kv;
                if ((ex * ex + ey * ey) * s_inv_sigma2[kl] > chi2) return;               // :1079
            }
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }                     // :1087
        });
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
