// ORBmatcherInit.cpp -- ORBmatcher::SearchForInitialization (src/ORBmatcher.cpp:477-595, monocular) over
// vba_search_for_initialization: frame 1 as flat arrays (descriptors, octaves, angles) with vbPrevMatched, frame 2 with its keypoints
// and its grid in CSR form (cell (ix, iy) at ix * mnGridRows + iy), ONE call, then vnMatches12 and vbPrevMatched from the result.  A
// source of its own: the matcher reads no map point and no level table, so it shares nothing with the projection matchers of
// ORBmatcher.cpp but the class.
#include <cstdint>
#include <iostream>
#include <string>
#include <vector>

#include "../../include/vislam_ba.h"
#include "BackendCall.h"
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

int ORBmatcher::SearchForInitialization(Frame& F1, Frame& F2, std::vector<Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize) {
    const char* who = "ORBmatcher::SearchForInitialization";
    const auto refuse = [&](const std::string& why) { std::cerr << who << ": " << why << std::endl; return -1; };
    const size_t n1 = F1.mvKeysUn.size(), n2 = F2.mvKeysUn.size();
    if ((size_t)F1.N != n1 || F1.mDescriptors.size() != 32 * n1 || F1.mvuRight.size() != n1) return refuse("N, mvKeysUn, mvuRight and mDescriptors of frame 1 disagree");
    if ((size_t)F2.N != n2 || F2.mDescriptors.size() != 32 * n2 || F2.mvuRight.size() != n2) return refuse("N, mvKeysUn, mvuRight and mDescriptors of frame 2 disagree");
    if (vbPrevMatched.size() != n1) return refuse("vbPrevMatched has not one entry per keypoint of frame 1");
    if (F2.mnGridCols < 1 || F2.mnGridRows < 1 || F2.mGrid.size() != (size_t)F2.mnGridCols) return refuse("frame 2 has no grid");
    std::vector<uint8_t> oct1(n1), oct2(n2);
    std::vector<float> angle1(n1), angle2(n2);
    std::vector<double> uv2(2 * n2);
    for (size_t i = 0; i < n1; i++) {
        const KeyPoint& kp = F1.mvKeysUn[i];
        if (F1.mvuRight[i] >= 0) return refuse("frame 1 has a stereo keypoint (the backend is monocular)");
        if (kp.octave < 0 || kp.octave > 255) return refuse("a keypoint's octave is outside 0 .. 255");   // the ABI carries octaves as uint8
        oct1[i] = (uint8_t)kp.octave; angle1[i] = kp.angle;
    }
    for (size_t i = 0; i < n2; i++) {
        const KeyPoint& kp = F2.mvKeysUn[i];
        if (F2.mvuRight[i] >= 0) return refuse("frame 2 has a stereo keypoint (the backend is monocular)");
        if (kp.octave < 0 || kp.octave > 255) return refuse("a keypoint's octave is outside 0 .. 255");
        oct2[i] = (uint8_t)kp.octave; angle2[i] = kp.angle;
        uv2[2 * i] = kp.pt.x; uv2[2 * i + 1] = kp.pt.y;
    }
    std::vector<int32_t> cell_begin(1, 0), cell_feat;
    cell_begin.reserve((size_t)F2.mnGridCols * (size_t)F2.mnGridRows + 1); cell_feat.reserve(n2);
    for (int ix = 0; ix < F2.mnGridCols; ix++) {
        if (F2.mGrid[(size_t)ix].size() != (size_t)F2.mnGridRows) return refuse("frame 2 has no grid");   // a ragged column
        for (int iy = 0; iy < F2.mnGridRows; iy++) {
            for (size_t idx : F2.mGrid[(size_t)ix][(size_t)iy]) cell_feat.push_back((int32_t)idx);
            cell_begin.push_back((int32_t)cell_feat.size());
        }
    }
    static_assert(sizeof(Point2f) == 8, "vbPrevMatched is read as [n][2] float");
    vba_search_init_problem P{};
    vba_search_init_result R{};
    P.check_orientation = mbCheckOrientation ? 1 : 0; P.th_low = TH_LOW; P.nn_ratio = mfNNratio; P.window_size = windowSize;
    P.n_keys1 = (int32_t)n1; P.desc1 = F1.mDescriptors.data(); P.oct1 = oct1.data(); P.angle1 = angle1.data();
    P.prev_matched = n1 ? &vbPrevMatched[0].x : nullptr;
    P.n_keys2 = (int32_t)n2; P.desc2 = F2.mDescriptors.data(); P.uv2 = uv2.data(); P.oct2 = oct2.data(); P.angle2 = angle2.data();
    P.bounds[0] = F2.mnMinX; P.bounds[1] = F2.mnMaxX; P.bounds[2] = F2.mnMinY; P.bounds[3] = F2.mnMaxY;
    P.grid_cols = F2.mnGridCols; P.grid_rows = F2.mnGridRows; P.grid_inv_w = F2.mfGridElementWidthInv; P.grid_inv_h = F2.mfGridElementHeightInv;
    P.cell_begin = cell_begin.data(); P.cell_feat = cell_feat.data();
    std::vector<int32_t> match12(n1, -1), best_idx(n1), match21(n2);
    std::vector<uint16_t> best_dist(n1), best_dist2(n1), matched_dist(n2);
    std::vector<uint8_t> bin(n1), state(n1);
    std::vector<Point2f> prev(n1);
    R.match12 = match12.data(); R.best_idx = best_idx.data(); R.best_dist = best_dist.data(); R.best_dist2 = best_dist2.data(); R.bin = bin.data();
    R.state = state.data(); R.prev_matched = n1 ? &prev[0].x : nullptr; R.match21 = match21.data(); R.matched_dist = matched_dist.data();
    if (!BackendCall(who, vba_search_for_initialization, P, R)) return -1;
    vnMatches12.assign(match12.begin(), match12.end());           // :481, :543, :581
    vbPrevMatched = prev;                                         // :590-592
    return R.n_matches;
}

}  // namespace ORB_SLAM2
