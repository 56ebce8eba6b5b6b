// Initializer.h -- host facade with the reference's Initializer class (include/Initializer.h of mc275/MC_SLAM) over
// orbslam_min.h's Frame, whose whole computation runs on the MI355X backend through vba_two_view_init (include/vislam_ba.h).
//
// Kept from the reference: the constructor (src/Initializer.cpp:27-36: mK, mvKeys1, mSigma, mMaxIterations), in Initialize the
// building of mvMatches12 / mvbMatched1 (:51-62), the draw of the 8-sets through rand() with DUtils::Random::SeedRandOnce(0)
// semantics (:78-101: the first Initialize of the process seeds rand() with 0, later ones continue the stream), the thresholds
// 1.0 / 50 of :124-126, vP3D as float32.  Replaced: FindHomography, FindFundamental, the model choice, ReconstructH / ReconstructF
// (one vba_two_view_init call per Initialize()).
//
// Differences from the reference:
//   * R21 / t21 are row-major float arrays where the reference has cv::Mat; on failure they, vP3D and vbTriangulated are left
//     untouched (the reference clears R21 / t21 in ReconstructF only).
//   * FP64 arithmetic behind the call.
//   * Fewer than eight matches: the reference would index past vAvailableIndices; here Initialize returns false.
#pragma once
#include <array>
#include <utility>
#include <vector>

#include "../../include/vislam_ba.h"
#include "orbslam_min.h"

namespace ORB_SLAM2 {

struct Point3f { float x = 0, y = 0, z = 0; };   // cv::Point3f

class Initializer {
    typedef std::pair<int, int> Match;

public:
    Initializer(const Frame& ReferenceFrame, float sigma = 1.0, int iterations = 200);

    bool Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, std::array<float, 9>& R21, std::array<float, 3>& t21,
                    std::vector<Point3f>& vP3D, std::vector<bool>& vbTriangulated);

    // DUtils::Random::SeedRandOnce (Thirdparty/DBoW2/DUtils/Random.cpp): srand(seed) the first time only, per process
    static void SeedRandOnce(int seed);
    // the sets of :80-101 for N matches, into mvSets
    void DrawSets(int N);

    // state (public here: the test harness reads it)
    std::vector<KeyPoint> mvKeys1, mvKeys2;
    std::vector<Match> mvMatches12;
    std::vector<bool> mvbMatched1;
    double mK[4];
    float mSigma, mSigma2;
    int mMaxIterations;
    std::vector<std::vector<size_t>> mvSets;
    vba_two_view_result mLast;   // the scalar fields of the last call (its pointers are cleared)
};

}  // namespace ORB_SLAM2
