// vba_host_keygrid.h -- what the host halves of the projection matchers share (plain C++17, no HIP): the checks, the sizes and the
// packing of a keyframe's or frame's keypoints and of its grid in CSR form (cell (ix, iy) at ix * grid_rows + iy, cell_begin of
// grid_cols * grid_rows + 1 entries, cell_feat of cell_begin[last] keypoint indices).  vba_fuse_problem, vba_search_sim3_kf and
// vba_search_proj_problem name these fields alike (n_keys, desc, uv, oct, n_levels, grid_cols, grid_rows, cell_begin, cell_feat),
// so the helpers are templates over the struct.  What check_cell_lists accepts is what bounds the loops of sa_walk
// (vba_search_area.h).  Included by vba_host_fuse.h, vba_host_search_sim3.h, vba_host_search_proj.h and vba_host_search_proj_kf.h, and
// through them by their sanitizer harnesses.  What only the two SearchByProjection halves share (SpDesc and SpQuery: common checks,
// the upload half of the arena, describe_sp, pack_sp_common) is at the head of vba_host_search_proj.h; the ordered replay of the
// write-backs is vba_host_orient.h.
#pragma once
#include "vba_layout.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

namespace vba_host {

inline bool all_finite(const double* a, size_t k) {
    for (size_t i = 0; i < k; i++)
        if (!std::isfinite(a[i])) return false;
    return true;
}

// 1 .. 65536 cells: cell indices and the sums below stay far inside an int
template <class K>
bool grid_size_ok(const K& kf) {
    return kf.grid_cols >= 1 && kf.grid_rows >= 1 && (long long)kf.grid_cols * kf.grid_rows <= 65536;
}

// cells of the grid (cell_begin has one entry more) and entries of cell_feat; of a checked struct
template <class K>
size_t grid_cells(const K& kf) { return (size_t)kf.grid_cols * (size_t)kf.grid_rows; }
template <class K>
size_t grid_feat(const K& kf) { return (size_t)kf.cell_begin[grid_cells(kf)]; }

// an empty string, or why the cell lists are refused.  nf: the entries of cell_feat.  seen is scratch
inline std::string check_cell_lists(int cols, int rows, int n_keys, const int32_t* cell_begin, const int32_t* cell_feat, std::vector<unsigned char>& seen,
                                    int& nf) {
    const int nc = cols * rows;
    if (cell_begin[0] != 0) return "cell_begin does not start at 0";
    for (int c = 0; c < nc; c++)
        if (cell_begin[c + 1] < cell_begin[c]) return "cell_begin decreases at cell " + std::to_string(c);
    nf = cell_begin[nc];
    if (nf > n_keys) return "cell_begin ends above n_keys";
    if (nf > 0 && !cell_feat) return "NULL cell_feat";
    seen.assign((size_t)n_keys, 0);
    for (int i = 0; i < nf; i++) {
        const int a = cell_feat[i];
        if (a < 0 || a >= n_keys) return "cell_feat entry " + std::to_string(i) + ": keypoint index out of range";
        if (seen[(size_t)a]) return "cell_feat entry " + std::to_string(i) + ": keypoint " + std::to_string(a) + " listed twice";
        seen[(size_t)a] = 1;
    }
    return "";
}

// keypoint i: nullptr, or why it is refused (the caller puts "keypoint i: " in front).  Runs once per keypoint of a call: no string
// is built for a keypoint that passes
template <class K>
const char* keypoint_fault(const K& kf, size_t i) {
    if (!all_finite(kf.uv + 2 * i, 2)) return "a pixel is not finite";
    if (kf.oct[i] >= kf.n_levels) return "octave >= n_levels";
    return nullptr;
}

template <class K>
void pack_keys(const K& kf, FuKey* k) {
    for (size_t i = 0, e = (size_t)kf.n_keys; i < e; i++) {
        std::memcpy(k[i].d, kf.desc + 32 * i, 32);
        k[i].u = kf.uv[2 * i]; k[i].v = kf.uv[2 * i + 1];
        k[i].oct = kf.oct[i];
        std::memset(k[i].pad, 0, sizeof k[i].pad);
    }
}

template <class K>
void pack_grid(const K& kf, int32_t* hcell, int32_t* hfeat) {
    const size_t nf = grid_feat(kf);
    std::memcpy(hcell, kf.cell_begin, 4 * (grid_cells(kf) + 1));
    if (nf) std::memcpy(hfeat, kf.cell_feat, 4 * nf);
}

}  // namespace vba_host
