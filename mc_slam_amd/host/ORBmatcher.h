// ORBmatcher.h -- the reference's ORBmatcher (include/ORBmatcher.h) as far as this backend carries it: SearchForTriangulation
// (src/ORBmatcher.cpp:760-955, monocular) over vba_search_triangulation, both Fuse overloads (:958-1254, monocular) over vba_fuse and
// SearchBySim3 (:1258-1496, monocular) over vba_search_by_sim3, and the two tracking matchers SearchByProjection(F, vpMapPoints, th)
// (:63-156) and SearchByProjection(CurrentFrame, LastFrame, th, bMono) (:1511-1665) over vba_search_by_projection, and both SearchByBoW
// overloads (:207-350 keyframe -> frame, :609-748 keyframe -> keyframe) over vba_search_by_bow, each also as a batch form that makes
// one call for a vector of keyframes, and the loop-closure overload SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (:354-475)
// and the relocalisation overload SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1667-1797) over
// vba_search_by_projection_kf, and SearchForInitialization (:477-595) over vba_search_for_initialization.
#pragma once
#include <array>
#include <cstdint>
#include <set>
#include <utility>
#include <vector>

#include "orbslam_min.h"

namespace ORB_SLAM2 {

struct Point2f { float x = 0, y = 0; };   // cv::Point2f

class ORBmatcher {
public:
    static const int TH_LOW = 50;         // src/ORBmatcher.cpp:41
    static const int TH_HIGH = 100;       // :41
    static const int HISTO_LENGTH = 30;   // :42
    ORBmatcher(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
    // Matches between the keypoints of pKF1 and pKF2 that have no map point, inside shared vocabulary nodes and under the epipolar
    // constraint of F12; vMatchedPairs is cleared and filled in ascending idx1.  Returns the number of matches, -1 when the backend
    // failed or bOnlyStereo is set (this backend is monocular), with a message on std::cerr.  ONE vba_search_triangulation call
    int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, const Mat3f& F12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                               const bool bOnlyStereo);
    // the epipole of :768-775 in float32: the centre of pKF1 in the image of pKF2
    static void Epipole(KeyFrame* pKF1, KeyFrame* pKF2, float& ex, float& ey);
    // src/ORBmatcher.cpp:958-1119: vpMapPoints projected into pKF; a point whose best keypoint has a map point replaces it or is
    // replaced by it (the one with more observations stays), otherwise it gains the observation.  ONE vba_fuse call for the search,
    // then the reference's apply loop in list order on the live map; the loop tests :983 again in front of each point, because an
    // earlier point of the same call may have made a later one bad or put it into the keyframe.  Returns nFused, -1 when the
    // backend failed or pKF has a stereo keypoint (this backend is monocular), with a message on std::cerr
    int Fuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const float th = 3.0);
    // src/ORBmatcher.cpp:1123-1254: the same search under the Sim3 pose Scw (decomposed in float32 as :1134-1138), without the
    // reprojection gate; a point whose best keypoint has a good map point is recorded in vpReplacePoint[iMP] instead of replaced.
    // vba_fuse applies the level range check of :1027 here, too (include/vislam_ba.h).  A NULL entry of vpPoints is skipped
    int Fuse(KeyFrame* pKF, const Mat4f& Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint);
    // src/ORBmatcher.cpp:1258-1496: the map points of pKF1 projected into pKF2 through the inverse of the Sim3 (s12, R12 row-major,
    // t12), those of pKF2 into pKF1 through the Sim3, both with the intrinsics of pKF1 as the reference does; where both directions
    // agree, vpMatches12[i1] becomes the map point of pKF2.  vpMatches12 has one entry per keypoint of pKF1; its non-NULL entries
    // are the prior matches (:1291-1301).  ONE vba_search_by_sim3 call.  Returns nFound, -1 when the backend failed, vpMatches12 has
    // the wrong size or a keyframe has a stereo keypoint (this backend is monocular), with a message on std::cerr
    int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const Mat3f& R12,
                     const std::array<float, 3>& t12, const float th);
    // src/ORBmatcher.cpp:63-156: the points of vpMapPoints that are in view (mbTrackInView, not bad) matched to the keypoints of F, best
    // against second best with mfNNratio; a match is written into F.mvpMapPoints.  ONE vba_search_by_projection call in local-map
    // mode: the entry point is fused with Frame::isInFrustum, so the projection, mnTrackScaleLevel and mTrackViewCos are formed again
    // from F's pose (what isInFrustum(pMP, 0.5) stored for this frame) instead of read from the point.  Returns nmatches, -1 when the
    // backend failed or F has a stereo keypoint (this backend is monocular), with a message on std::cerr
    int SearchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th = 3);
    // src/ORBmatcher.cpp:1511-1665: the map points of LastFrame projected into CurrentFrame with the octave window of the monocular
    // case, then the orientation filter.  ONE vba_search_by_projection call in last-frame mode.  Returns nmatches, -1 when the backend
    // failed, bMono is false or CurrentFrame has a stereo keypoint
    int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono);
    // src/ORBmatcher.cpp:354-475, the last step of LoopClosing::ComputeSim3: vpPoints projected into pKF under the Sim3 pose Scw (decomposed
    // in float32 as :364-368); a point takes the best free keypoint of its area at its predicted level or the one below, and a
    // match is written into vpMatched, which has one entry per keypoint of pKF and whose non-NULL entries are taken from the start.
    // ONE vba_search_by_projection_kf call in loop mode.  A NULL entry of vpPoints is skipped.  Returns nmatches, the matches of this
    // call only, -1 when the backend failed, vpMatched has the wrong size or pKF has a stereo keypoint (this backend is monocular),
    // with a message on std::cerr
    int SearchByProjection(KeyFrame* pKF, const Mat4f& Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th);
    // src/ORBmatcher.cpp:1667-1797, the calls of Tracking::Relocalization (src/Tracking.cpp:2513, :2527): the map points of pKF that are not
    // in sAlreadyFound projected into CurrentFrame with its pose mTcw (no depth test, as the reference has none), matched to the keypoints
    // that hold no point, then the orientation filter.  ONE vba_search_by_projection_kf call in reloc mode.  Returns nmatches, -1
    // when the backend failed or CurrentFrame has a stereo keypoint
    int SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound, const float th, const int ORBdist);
    // src/ORBmatcher.cpp:207-350: the map points of pKF matched to the keypoints of F inside shared vocabulary nodes, best against second
    // best with mfNNratio, then the orientation filter; vpMapPointMatches gets one entry per keypoint of F.  ONE vba_search_by_bow call
    // in KF_FRAME mode.  Returns nmatches, -1 when the backend failed or the arrays of pKF or F disagree, with a message on std::cerr
    int SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches);
    // src/ORBmatcher.cpp:609-748: the same between two keyframes, over the keypoints of pKF2 that have a good map point and with the
    // strict threshold; vpMatches12 gets one entry per keypoint of pKF1, the map point of pKF2.  ONE call in KF_KF mode
    int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12);
    // The loop of Tracking::Relocalization (src/Tracking.cpp:2429): every keyframe of vpKFs against F, ONE vba_search_by_bow call for
    // all of them.  vvpMapPointMatches[i] and vnMatches[i] are what SearchByBoW(vpKFs[i], F, ...) gives.  Returns 0, -1 on failure
    int SearchByBoW(const std::vector<KeyFrame*>& vpKFs, Frame& F, std::vector<std::vector<MapPoint*>>& vvpMapPointMatches, std::vector<int>& vnMatches);
    // The loop of LoopClosing::ComputeSim3 (src/LoopClosing.cpp:317): pKF1 against every keyframe of vpKFs2, ONE call for all of them
    int SearchByBoW(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKFs2, std::vector<std::vector<MapPoint*>>& vvpMatches12, std::vector<int>& vnMatches);
    // src/ORBmatcher.cpp:477-595, the matcher of Tracking::MonocularInitialization: every level-0 keypoint of F1 searches the window of
    // windowSize pixels around vbPrevMatched[i1] in F2 among the level-0 keypoints, best against second best with mfNNratio, a later
    // keypoint steals a keypoint of F2 from an earlier one when it is strictly nearer, then the orientation filter; vnMatches12 gets
    // one entry per keypoint of F1 and vbPrevMatched the pixel of every match kept.  ONE vba_search_for_initialization call.  Returns
    // nmatches, -1 when the backend failed, vbPrevMatched has not one entry per keypoint of F1, the arrays of a frame disagree or a
    // frame has a stereo keypoint (this backend is monocular), with a message on std::cerr; vnMatches12 and vbPrevMatched are then
    // left as they were
    int SearchForInitialization(Frame& F1, Frame& F2, std::vector<Point2f>& vbPrevMatched, std::vector<int>& vnMatches12, int windowSize = 10);
    // vbAlreadyMatched1 / vbAlreadyMatched2 of :1287-1301: a keypoint of pKF1 with a prior match, and the keypoint of pKF2 where
    // GetIndexInKeyFrame finds that match
    static void AlreadyMatched(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatches12, std::vector<uint8_t>& vb1,
                               std::vector<uint8_t>& vb2);

protected:
    float mfNNratio;
    bool mbCheckOrientation;
};

// What SearchByProjection(F, vpMapPoints, th) and Tracking::SearchLocalPoints share: ONE vba_search_by_projection call in local-map
// mode over the points whose skip flag is 0.  On success every such point has mbTrackInView as Frame::isInFrustum(pMP, 0.5) leaves it
// and, when in view, mTrackProjX / Y, mnTrackScaleLevel and mTrackViewCos; *in_view counts them; the matches are in F.mvpMapPoints.
// Returns nmatches, -1 when the backend failed or F has a stereo keypoint, with a message that starts with `who` on std::cerr
int SearchLocalMap(const char* who, Frame& F, const std::vector<MapPoint*>& vpMapPoints, const std::vector<uint8_t>& skip, float th, float nnratio,
                   int* in_view);

}  // namespace ORB_SLAM2
