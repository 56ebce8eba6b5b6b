// Tracking.h -- the slice of the reference's Tracking (include/Tracking.h) that sits directly in front of its two PoseOptimization
// calls: SearchLocalPoints (src/Tracking.cpp:2111-2174) and the matching half of TrackWithMotionModel (:1749-1770), each ONE
// vba_search_by_projection call (two with the retry), and the matching half of TrackReferenceKeyFrame (:1600-1609), ONE
// vba_search_by_bow call.  And the matching part of MonocularInitialization (:1360-1381) in front of Initializer::Initialize, ONE
// vba_search_for_initialization call.  Monocular.
#pragma once
#include <memory>
#include <vector>

#include "Initializer.h"
#include "ORBmatcher.h"
#include "orbslam_min.h"

namespace ORB_SLAM2 {

class Tracking {
public:
    Frame mCurrentFrame, mLastFrame;
    KeyFrame* mpReferenceKF = nullptr;
    std::vector<MapPoint*> mvpLocalMapPoints;
    long unsigned int mnLastRelocFrameId = 0;
    // src/Tracking.cpp:2111-2174: the points the frame already holds are marked as seen (bad ones leave the frame), every other
    // local point goes through isInFrustum(pMP, 0.5) and, when in view, IncreaseVisible and the search with ORBmatcher(0.8) and th = 1
    // (5 directly behind a relocalisation).  Returns nToMatch, -1 when the backend failed
    int SearchLocalPoints();
    // src/Tracking.cpp:1749-1770: mvpMapPoints of the current frame filled with NULL, SearchByProjection(mCurrentFrame, mLastFrame, 15,
    // true) with ORBmatcher(0.9, true), and once more with twice the radius when fewer than 20 matches came back.  The pose of
    // mCurrentFrame is the caller's (:1746).  Returns nmatches, -1 when the backend failed
    int TrackWithMotionModelMatches();
    // src/Tracking.cpp:1597-1607: SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches) with ORBmatcher(0.7, true); with fewer than
    // 15 matches the frame is left as it is (the reference returns false), otherwise the matches become mCurrentFrame.mvpMapPoints and
    // the pose of the last frame the initial pose.  The feature vector of mCurrentFrame is the caller's (:1593).  Returns nmatches, -1
    // when the backend failed
    int TrackReferenceKeyFrameMatches();
    // what MonocularInitialization keeps between frames (src/Tracking.cpp:1333-1349): the first frame, the last matched positions,
    // the matches and the initializer made of the first frame
    Frame mInitialFrame;
    std::vector<Point2f> mvbPrevMatched;
    std::vector<int> mvIniMatches;
    std::unique_ptr<Initializer> mpInitializer;
    // src/Tracking.cpp:1360-1381, the branch with an initializer: with 100 keypoints or fewer in mCurrentFrame the initializer is
    // deleted, mvIniMatches filled with -1 and -2 returned (the matcher is not called); otherwise
    // ORBmatcher(0.9, true).SearchForInitialization(mInitialFrame, mCurrentFrame, mvbPrevMatched, mvIniMatches, 100), and with fewer
    // than 100 matches the initializer is deleted.  While mpInitializer is still set the caller goes on to
    // mpInitializer->Initialize(mCurrentFrame, mvIniMatches, ...) (:1388).  Returns nmatches, -1 when the backend failed or refused
    // (the initializer is deleted then too)
    int MonocularInitializationMatches();
};

}  // namespace ORB_SLAM2
