// vba_host_orient.h -- what the write-backs of the ordered matchers share (plain C++17, no HIP): the rotation bin, ComputeThreeMaxima
// and the replay of the reference's apply loop with its orientation filter, in query order.  Used by unpack_search_proj,
// unpack_search_proj_kf and unpack_search_bow (vba_host_search_proj.h, vba_host_search_proj_kf.h, vba_host_search_bow.h) and through
// them by their sanitizer harnesses; unpack_search_init (vba_host_search_init.h) uses rot_bin and three_maxima with an apply loop of its
// own, because a match there can be stolen.  The replay runs on the host and not in the kernels: it needs the angles, which the device then
// never sees, and it touches outputs only.
#pragma once
#include "vba_layout.h"

#include <cmath>
#include <cstdint>

namespace vba_host {

// ComputeThreeMaxima (src/ORBmatcher.cpp:1800-1841) over bin counts, as k_search_tri has it
inline void three_maxima(const int32_t* histo, int32_t* ind) {
    int max1 = 0, max2 = 0, max3 = 0, i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < VBA_ST_HISTO; i++) {
        const int s = histo[i];
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; i3 = i2; i2 = i1; i1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; i3 = i2; i2 = i; }
        else if (s > max3) { max3 = s; i3 = i; }
    }
    if ((float)max2 < 0.1f * (float)max1) { i2 = -1; i3 = -1; }
    else if ((float)max3 < 0.1f * (float)max1) i3 = -1;
    ind[0] = i1; ind[1] = i2; ind[2] = i3;
}

// the bin of :1628-1633: float32, C round
inline int rot_bin(float angle_q, float angle_k) {
    float rot = angle_q - angle_k;
    if (rot < 0.0f) rot += 360.0f;
    const float factor = 1.0f / VBA_ST_HISTO;
    int bin = (int)std::round(rot * factor);
    if (bin == VBA_ST_HISTO) bin = 0;
    return bin;
}

// The apply loop over res->best_idx / res->state as they came back (n queries, keypoints 0 .. n_keys - 1 on the other side), in query
// order: every query in state 0 is a match, match(i, b) writes it where the matcher keeps its matches, and with the filter on (ori)
// it is binned by rot_bin(angle_q[i], angle_k[b]).  Then the three maxima; every match of another bin is taken back by drop(i), and
// its query leaves with drop_state.  Sets hist, ind, bin, n_before_filter and n_matches
template <class R, class Match, class Drop>
void replay_matches(R* res, size_t n, size_t n_keys, bool ori, const float* angle_q, const float* angle_k, uint8_t drop_state, Match&& match, Drop&& drop) {
    for (int i = 0; i < VBA_ST_HISTO; i++) res->hist[i] = 0;
    res->ind[0] = res->ind[1] = res->ind[2] = -1;
    int nmatches = 0;
    for (size_t i = 0; i < n; i++) {
        res->bin[i] = 255;
        const int32_t b = res->best_idx[i];
        if (res->state[i] != 0 || b < 0 || (size_t)b >= n_keys) continue;   // a state 0 always brings a keypoint of the other side
        match(i, b);
        nmatches++;
        if (ori) {
            const int bin = rot_bin(angle_q[i], angle_k[b]);
            res->bin[i] = (uint8_t)bin;
            res->hist[bin]++;
        }
    }
    res->n_before_filter = nmatches;
    if (ori) {
        three_maxima(res->hist, res->ind);
        for (size_t i = 0; i < n; i++) {
            const int bin = res->bin[i];
            if (bin == 255 || bin == res->ind[0] || bin == res->ind[1] || bin == res->ind[2]) continue;
            drop(i);
            res->state[i] = drop_state;
            nmatches--;
        }
    }
    res->n_matches = nmatches;
}

}  // namespace vba_host
