// Tracking.h -- the slice of the reference's Tracking (include/Tracking.h) that sits directly in front of its two PoseOptimization
// calls: SearchLocalPoints (src/Tracking.cpp:2111-2174) and the matching half of TrackWithMotionModel (:1749-1770), each ONE
// vba_search_by_projection call (two with the retry), and the matching half of TrackReferenceKeyFrame (:1600-1609), ONE
// vba_search_by_bow call.  Monocular.
#pragma once
#include <vector>

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
};

}  // namespace ORB_SLAM2
