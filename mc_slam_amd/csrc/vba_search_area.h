// vba_search_area.h -- what the projection matchers share on the device (k_fuse, k_search_sim3, k_search_proj, k_search_proj_kf, k_search_init; the descriptor
// helpers also k_search_tri): the rigid transform, MapPoint::PredictScale (src/MapPoint.cpp:529-540), the descriptor load and the
// Hamming distance, and the cell walk of GetFeaturesInArea (src/KeyFrame.cpp:1071-1115, src/Frame.cpp:562-620) over a keyframe grid
// in CSR form.  A kernel keeps its gates, its candidate tests and its outputs; the next matcher is written against sa_walk.  What the
// ORDERED matchers share beyond this (k_search_proj, k_search_proj_kf, k_search_bow), the conflict pass over a claim table in LDS, is
// vba_search_claim.h; k_search_init is ordered too, over claimer lists of its own (vba_search_init.h).
//
// The walk: the cell range in double, clamped as max(0, .) and min(n - 1, .) do, with the reference's four early returns.  The
// cells (ix, y0 .. y1) are neighbours in cell_begin, so a column of the range is ONE range of cell_feat, in the order of the
// reference's loops (ix outer, iy inner, list order inside a cell): a strict `dist < bestDist` in the visitor keeps the first of
// equal distances.  The visitor holds the kernel's candidate tests (the reference's `continue` is its `return`) and captures the
// kernel's state by reference; everything is inlined, so that state stays in registers.  Every loop is bounded by what the host
// checked (vba_host_keygrid.h): cell_begin is non-decreasing and ends at most at n_keys, every cell_feat entry is a keypoint.
// `y1 < y0` (a negative radius) returns in front of the loops.  It cannot change an output: with y1 + 1 <= y0 the range
// [cell_begin[ix * rows + y0], cell_begin[ix * rows + y1 + 1]) is empty because cell_begin is non-decreasing.
// Contraction: `#pragma clang fp contract(off)` holds for the compound statement it stands in and a callee does not inherit it, so
// every helper with FP64 arithmetic opens with its own; at file scope it would reach the kernels included afterwards.
// The pinhole projection is NOT here: k_fuse and k_search_sim3 compute K0 * (xc * invz) + K2, k_search_proj (K0 * xc) * invz + K2,
// k_search_proj_kf the first in loop mode and the second in reloc mode, each as the reference lines it cites, and the two round
// differently.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"

// offsets in the camera block, the entries 0 .. 27 of FuDesc::c and SpDesc::c (and of their LDS copies)
#define SA_R 0
#define SA_T 9
#define SA_OW 12
#define SA_K 15
#define SA_TB 19     // the target block
#define SA_COS 27
// offsets in the target block, 8 doubles: at SA_TB in FuDesc::c and SpDesc::c, at SS_TB in SsDir::c
#define SA_B 0       // bounds: min x, max x, min y, max y
#define SA_GIW 4
#define SA_GIH 5
#define SA_LOGSF 6
#define SA_TH 7

struct SaGrid {      // the grid of one keyframe or frame: keypoint records and the cell lists in CSR form, cell (ix, iy) at ix * rows + iy
    const FuKey* key;
    const int* cell_begin;
    const int* cell_feat;
    int cols, rows;
};

// R p + t, rows of R left to right
DEVI void sa_rigid(const double* R, const double* t, double px, double py, double pz, double& x, double& y, double& z) {
#pragma clang fp contract(off)
    x = ((R[0] * px + R[1] * py) + R[2] * pz) + t[0];
    y = ((R[3] * px + R[4] * py) + R[5] * pz) + t[1];
    z = ((R[6] * px + R[7] * py) + R[8] * pz) + t[2];
}

// PredictScale with the range check 0 <= level < nl.  false: outside (state 6), and level holds the int8 the state reports
DEVI bool sa_predict_level(double pred_max, double dist, double logsf, int nl, int& level) {
#pragma clang fp contract(off)
    const double lv = ceil(log(pred_max / dist) / logsf);
    if (!(lv >= 0.0 && lv < (double)nl)) {
        level = (lv >= 127.0) ? 127 : ((lv > -128.0) ? (int)lv : -128);   // NaN gives -128
        return false;
    }
    level = (int)lv;
    return true;
}

DEVI void sa_load_desc(unsigned int (&a)[8], const unsigned int* d) {
#pragma unroll
    for (int w = 0; w < 8; w++) a[w] = d[w];
}

// ORBmatcher::DescriptorDistance.  The accumulating bit count is written out: a helper (and a visitor's body) is optimised before
// it is inlined, and a plain `dist += __popc(..)` chain unrolled there compiles to eight counts and three v_add3, not eight
// accumulating counts (measured: 1 to 2 % of the kernels' time)
DEVI int sa_hamming(const unsigned int (&a)[8], const unsigned int* d) {
    int dist = __popc(a[0] ^ d[0]);
#pragma unroll
    for (int w = 1; w < 8; w++) asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(dist) : "v"(a[w] ^ d[w]));
    return dist;
}

// GetFeaturesInArea(u, v, r) without its pixel test: visit(idx, key[idx]) for every keypoint of the cell range, in the reference's order
template <class V>
DEVI void sa_walk(const SaGrid& g, const double* tb, double u, double v, double r, V&& visit) {
#pragma clang fp contract(off)
    const int cols = g.cols, rows = g.rows;
    const double fx0 = floor(((u - tb[SA_B + 0]) - r) * tb[SA_GIW]);
    if (fx0 >= (double)cols) return;
    const double fx1 = ceil(((u - tb[SA_B + 0]) + r) * tb[SA_GIW]);
    if (fx1 < 0.0) return;
    const double fy0 = floor(((v - tb[SA_B + 2]) - r) * tb[SA_GIH]);
    if (fy0 >= (double)rows) return;
    const double fy1 = ceil(((v - tb[SA_B + 2]) + r) * tb[SA_GIH]);
    if (fy1 < 0.0) return;
    const int x0 = (fx0 > 0.0) ? (int)fx0 : 0, x1 = (fx1 < (double)(cols - 1)) ? (int)fx1 : cols - 1;
    const int y0 = (fy0 > 0.0) ? (int)fy0 : 0, y1 = (fy1 < (double)(rows - 1)) ? (int)fy1 : rows - 1;
    if (y1 < y0) return;   // a negative radius: no cell
    for (int ix = x0; ix <= x1; ix++) {
        const int jb = g.cell_begin[ix * rows + y0], je = g.cell_begin[ix * rows + y1 + 1];
        for (int j = jb; j < je; j++) {
            const int idx = g.cell_feat[j];
            visit(idx, g.key[idx]);
        }
    }
}
