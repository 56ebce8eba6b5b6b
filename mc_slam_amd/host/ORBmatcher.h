// ORBmatcher.h -- the reference's ORBmatcher (include/ORBmatcher.h) as far as this backend carries it: SearchForTriangulation
// (src/ORBmatcher.cpp:760-955, monocular) over vba_search_triangulation.  The other searches stay matcher code of the caller.
#pragma once
#include <utility>
#include <vector>

#include "orbslam_min.h"

namespace ORB_SLAM2 {

class ORBmatcher {
public:
    static const int TH_LOW = 50;         // src/ORBmatcher.cpp:41
    static const int HISTO_LENGTH = 30;   // :42
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    // Matches between the keypoints of pKF1 and pKF2 that have no map point, inside shared vocabulary nodes and under the epipolar
    // constraint of F12; vMatchedPairs is cleared and filled in ascending idx1.  Returns the number of matches, -1 when the backend
    // failed or bOnlyStereo is set (this backend is monocular), with a message on std::cerr.  ONE vba_search_triangulation call
    int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, const Mat3f& F12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                               const bool bOnlyStereo);
    // the epipole of :768-775 in float32: the centre of pKF1 in the image of pKF2
    static void Epipole(KeyFrame* pKF1, KeyFrame* pKF2, float& ex, float& ey);

protected:
    float mfNNratio;
    bool mbCheckOrientation;
};

}  // namespace ORB_SLAM2
