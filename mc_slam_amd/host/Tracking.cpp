// Tracking.cpp -- Tracking::SearchLocalPoints (src/Tracking.cpp:2111-2174) and the matching half of Tracking::TrackWithMotionModel
// (:1749-1770) over vba_search_by_projection, and the matching half of Tracking::TrackReferenceKeyFrame (:1597-1607) over
// vba_search_by_bow, and the matching part of Tracking::MonocularInitialization (:1360-1381) over vba_search_for_initialization
// (ORBmatcher.cpp), monocular.
#include "Tracking.h"

#include <algorithm>

#include "ORBmatcher.h"

namespace ORB_SLAM2 {

int Tracking::SearchLocalPoints() {
    for (MapPoint*& pMP : mCurrentFrame.mvpMapPoints) {           // :2114-2134
        if (!pMP) continue;
        if (pMP->isBad()) {
            pMP = nullptr;
        } else {
            pMP->IncreaseVisible();
            pMP->mnLastFrameSeen = mCurrentFrame.mnId;
            pMP->mbTrackInView = false;
        }
    }
    const size_t n = mvpLocalMapPoints.size();
    std::vector<uint8_t> skip(n);
    for (size_t i = 0; i < n; i++) {
        MapPoint* pMP = mvpLocalMapPoints[i];
        skip[i] = pMP->mnLastFrameSeen == mCurrentFrame.mnId || pMP->isBad();   // :2145-2148
    }
    const float th = (mCurrentFrame.mnId < mnLastRelocFrameId + 2) ? 5.0f : 1.0f;   // :2163-2169, monocular
    int nToMatch = 0;
    if (SearchLocalMap("Tracking::SearchLocalPoints", mCurrentFrame, mvpLocalMapPoints, skip, th, 0.8f, &nToMatch) < 0) return -1;
    for (size_t i = 0; i < n; i++)
        if (!skip[i] && mvpLocalMapPoints[i]->mbTrackInView) mvpLocalMapPoints[i]->IncreaseVisible();   // :2154
    return nToMatch;
}

int Tracking::TrackWithMotionModelMatches() {
    ORBmatcher matcher(0.9, true);                                // :1738
    std::fill(mCurrentFrame.mvpMapPoints.begin(), mCurrentFrame.mvpMapPoints.end(), static_cast<MapPoint*>(nullptr));   // :1749
    const int th = 15;                                            // :1752-1756, monocular
    int nmatches = matcher.SearchByProjection(mCurrentFrame, mLastFrame, th, true);
    if (nmatches >= 0 && nmatches < 20) {                         // :1763-1767
        std::fill(mCurrentFrame.mvpMapPoints.begin(), mCurrentFrame.mvpMapPoints.end(), static_cast<MapPoint*>(nullptr));
        nmatches = matcher.SearchByProjection(mCurrentFrame, mLastFrame, 2 * th, true);
    }
    return nmatches;
}

int Tracking::TrackReferenceKeyFrameMatches() {
    ORBmatcher matcher(0.7, true);                                // :1597
    std::vector<MapPoint*> vpMapPointMatches;
    const int nmatches = matcher.SearchByBoW(mpReferenceKF, mCurrentFrame, vpMapPointMatches);   // :1600
    if (nmatches < 15) return nmatches;                           // :1602-1603
    mCurrentFrame.mvpMapPoints = vpMapPointMatches;               // :1606
    mCurrentFrame.SetPose(mLastFrame.mTcw);                       // :1607
    return nmatches;
}

int Tracking::MonocularInitializationMatches() {
    if ((int)mCurrentFrame.mvKeys.size() <= 100) {                // :1360-1366
        mpInitializer.reset();
        std::fill(mvIniMatches.begin(), mvIniMatches.end(), -1);
        return -2;
    }
    ORBmatcher matcher(0.9, true);                                // :1371
    const int nmatches = matcher.SearchForInitialization(mInitialFrame, mCurrentFrame, mvbPrevMatched, mvIniMatches, 100);
    if (nmatches < 100) mpInitializer.reset();                    // :1376-1381
    return nmatches;
}

}  // namespace ORB_SLAM2
