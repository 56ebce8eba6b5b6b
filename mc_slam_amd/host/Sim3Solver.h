// Sim3Solver.h -- host facade with the reference's Sim3Solver class (include/Sim3Solver.h:17-115 of mc275/MC_SLAM) over
// orbslam_min.h, whose hypotheses run on the MI355X backend through vba_sim3_ransac (include/vislam_ba.h).
//
// Kept from the reference: the constructor's pair filters and the float32 camera-frame points (src/Sim3Solver.cpp:29-95), the gates
// 9.210 * sigma2 as the reference stores them (in a vector<size_t>: truncated to whole pixels^2, :78-79 with include/Sim3Solver.h:63-64),
// SetRansacParameters with its float epsilon (:109-134), the draw of the triples through rand() (:163-184), the running best and
// the iteration count carried from one iterate() to the next, bNoMore.  Replaced: ComputeSim3, CheckInliers and the accept rule of
// every hypothesis (one vba_sim3_ransac call per iterate()).
//
// Differences from the reference:
//   * iterate() / find() return bool (false where the reference returns an empty cv::Mat) and hand T12 out through a Mat4f.
//   * iterate() draws the triples of all its hypotheses before the call, so after a hit inside one call the rand() stream has been
//     consumed for the hypotheses behind the hit as well; the reference stops drawing at the hit.  Draws happen per iterate() call,
//     not ahead, so up to the first hit the stream is consumed exactly as in the reference.
//   * the removal step of the draw writes vAvailableIndices[idx] where [randi] is meant (:182), which lets a triple hold a pair
//     twice and, in the reference, writes past the vector's size.  It is restated as it stands, without the out-of-bounds write:
//     the vector stays at its capacity and a logical size shrinks.
//   * FP64 arithmetic in the hypotheses.
#pragma once
#include <array>
#include <vector>

#include "../../include/vislam_ba.h"
#include "orbslam_min.h"

namespace ORB_SLAM2 {

class Sim3Solver {
public:
    Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale = true);

    void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300);

    bool find(std::vector<bool>& vbInliers12, int& nInliers, Mat4f& T12);
    bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Mat4f& T12);

    std::array<float, 9> GetEstimatedRotation();      // row-major
    std::array<float, 3> GetEstimatedTranslation();
    float GetEstimatedScale();

    // DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/Random.cpp:47-50) on rand()
    static int RandomInt(int min, int max);
    // the triples of n hypotheses as :163-184 draw them, appended to `triples` (3 per hypothesis)
    void DrawTriples(int n, std::vector<int32_t>& triples);

    // state (public here: the test harness reads it)
    KeyFrame *mpKF1, *mpKF2;
    std::vector<double> mvX3Dc1, mvX3Dc2;             // [N][3] float32 values, widened
    std::vector<MapPoint*> mvpMapPoints1, mvpMapPoints2, mvpMatches12;
    std::vector<size_t> mvnIndices1;
    std::vector<size_t> mvnMaxError1, mvnMaxError2;
    int N, mN1;
    int mnIterations, mnBestInliers;
    double mBestS12[8];                               // t(3) q(4, xyzw) s: mBestTranslation / Rotation / Scale
    bool mbFixScale;
    std::vector<size_t> mvAllIndices;
    double mRansacProb;
    int mRansacMinInliers, mRansacMaxIts;
    double mK1[4], mK2[4];
    std::vector<int32_t> mvLastTriples;               // of the last iterate()
};

}  // namespace ORB_SLAM2
