// LoopClosing.cpp -- steps 6-9 of LoopClosing::ComputeSim3 (src/LoopClosing.cpp:442-495) over the loop-closure overload of
// ORBmatcher::SearchByProjection (ORBmatcher.cpp, ONE vba_search_by_projection_kf call): LoopClosing.h.
#include "LoopClosing.h"

#include "ORBmatcher.h"

namespace ORB_SLAM2 {

bool LoopClosing::MatchLoopMapPoints() {
    // step 6: the covisible keyframes of the matched keyframe, then the keyframe itself (:442-444), every good point once (:455-459)
    std::vector<KeyFrame*> vpLoopConnectedKFs = mpMatchedKF->GetVectorCovisibleKeyFrames();
    vpLoopConnectedKFs.push_back(mpMatchedKF);
    mvpLoopMapPoints.clear();
    for (KeyFrame* pKF : vpLoopConnectedKFs) {
        const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
        for (MapPoint* pMP : vpMapPoints) {
            if (!pMP) continue;
            if (!pMP->isBad() && pMP->mnLoopPointForKF != mpCurrentKF->mnId) {
                mvpLoopMapPoints.push_back(pMP);
                pMP->mnLoopPointForKF = mpCurrentKF->mnId;
            }
        }
    }
    // step 7 (:470)
    ORBmatcher matcher(0.75, true);
    if (matcher.SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10) < 0) {
        mnLoopTotalMatches = -1;
        return false;
    }
    // step 8 (:473-478)
    int nTotalMatches = 0;
    for (MapPoint* pMP : mvpCurrentMatchedPoints)
        if (pMP) nTotalMatches++;
    mnLoopTotalMatches = nTotalMatches;
    return nTotalMatches >= 40;   // step 9 (:481)
}

}  // namespace ORB_SLAM2
