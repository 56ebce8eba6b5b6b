// LoopClosing.h -- the reference's LoopClosing (include/LoopClosing.h) as far as this backend carries it.  The class itself is declared
// in orbslam_min.h (Optimizer::OptimizeEssentialGraph takes its KeyFrameAndPose); this header names the slice of
// LoopClosing::ComputeSim3 that LoopClosing.cpp implements.
//
//   bool LoopClosing::MatchLoopMapPoints()
// Steps 6-9 of ComputeSim3 (src/LoopClosing.cpp:442-495), behind the candidate loop whose stages are vba_search_by_bow,
// vba_sim3_ransac, vba_search_by_sim3 and vba_sim3_optimize: with mpCurrentKF, mpMatchedKF, mScw and mvpCurrentMatchedPoints (one
// entry per keypoint of mpCurrentKF) as the accepted candidate left them,
//   6  mvpLoopMapPoints is gathered from the covisible keyframes of mpMatchedKF and mpMatchedKF itself, in that order: every map
//      point that is not bad, once, through the mnLoopPointForKF mark (:442-463);
//   7  ORBmatcher::SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10) (:470), ONE
//      vba_search_by_projection_kf call;
//   8  nTotalMatches counts the non-NULL entries of mvpCurrentMatchedPoints (:473-478) and is left in mnLoopTotalMatches;
//   9  the loop is accepted iff nTotalMatches >= 40 (:481): the return value.  SetErase on the candidates (:483-493) is the
//      caller's: the keyframes here carry no erase flag.
// A backend failure returns false with mnLoopTotalMatches = -1 and a message on std::cerr; mvpLoopMapPoints stays gathered.
#pragma once
#include "orbslam_min.h"
