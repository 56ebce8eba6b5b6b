// LocalMapping.cpp -- LocalMapping::CreateNewMapPoints (src/LocalMapping.cpp:1237-1546, monocular) over vba_triangulate: the
// reference's loop over the neighbours with its gate, the matcher -- the caller's function object, or ComputeF12 and
// ORBmatcher::SearchForTriangulation over vba_search_triangulation in the overload without one --, ONE vba_triangulate call
// per neighbour (the matcher of neighbour i + 1 must see the points created from neighbour i, so the pairs of a keyframe cannot
// share a call here), and the map-point construction for every accepted match in match order.
// LocalMapping::SearchInNeighbors (:1550-1655), steps 2 and 3, over ORBmatcher::Fuse: ONE vba_fuse call per Fuse call, in the
// reference's order.  MapPoint::Replace ends in ComputeDistinctiveDescriptors, so the Fuse call of target i + 1 may see a
// descriptor that the call of target i changed (and points it made bad or put into keyframes): the targets cannot share a call
// without changing an answer.
#include <cmath>

#include "../../include/vislam_ba.h"
#include "BackendCall.h"
#include "ORBmatcher.h"

namespace ORB_SLAM2 {

namespace {
// the keyframe's side of a vba_triangulate_problem: pose, centre, intrinsics (float32 widened) and the level tables
struct TriSide {
    double R[9], t[3], O[3], K[4];
    std::vector<double> sigma2, scale;
    explicit TriSide(KeyFrame* kf) : sigma2(kf->mvLevelSigma2.begin(), kf->mvLevelSigma2.end()), scale(kf->mvScaleFactors.begin(), kf->mvScaleFactors.end()) {
        kf->GetRotation(R);
        kf->GetTranslation(t);
        kf->GetCameraCenter(O);
        K[0] = kf->fx; K[1] = kf->fy; K[2] = kf->cx; K[3] = kf->cy;
    }
};
// a matcher that can fail: false ends the walk over the neighbours at once
typedef std::function<bool(KeyFrame*, KeyFrame*, std::vector<std::pair<size_t, size_t>>&)> FallibleMatcher;

// the loop of both overloads.  -1 when the matcher or the backend failed: nothing is done for the neighbour that failed or for
// the ones behind it; the points made from the neighbours in front of it stay in the map
int create_new_map_points(KeyFrame* pKF, const std::vector<KeyFrame*>& vpNeighKFs, const FallibleMatcher& matcher, Map* pMap,
                          std::list<MapPoint*>& lpRecentAddedMapPoints) {
    const TriSide s1(pKF);
    const float ratioFactor = 1.5f * pKF->mfScaleFactor;   // :1272
    int nnew = 0;
    for (size_t i = 0; i < vpNeighKFs.size(); i++) {
        KeyFrame* pKF2 = vpNeighKFs[i];
        // :1287-1311 the baseline against the median scene depth of the neighbour, in float32
        double Ow2[3];
        pKF2->GetCameraCenter(Ow2);
        const float b[3] = {(float)Ow2[0] - (float)s1.O[0], (float)Ow2[1] - (float)s1.O[1], (float)Ow2[2] - (float)s1.O[2]};
        const float baseline = (float)std::sqrt((double)b[0] * b[0] + (double)b[1] * b[1] + (double)b[2] * b[2]);   // cv::norm accumulates in double
        const float medianDepthKF2 = pKF2->ComputeSceneMedianDepth(2);
        const float ratioBaselineDepth = baseline / medianDepthKF2;
        if (ratioBaselineDepth < 0.01) continue;
        // :1318 the matcher (ComputeF12 of :1314 belongs to it)
        std::vector<std::pair<size_t, size_t>> vMatchedIndices;
        if (!matcher(pKF, pKF2, vMatchedIndices)) return -1;
        const int nmatches = (int)vMatchedIndices.size();
        if (nmatches == 0) continue;
        const TriSide s2(pKF2);
        std::vector<double> uv1(2 * (size_t)nmatches), uv2(2 * (size_t)nmatches), x3d(3 * (size_t)nmatches);
        std::vector<uint8_t> oct1(nmatches), oct2(nmatches), reason(nmatches);
        for (int ikp = 0; ikp < nmatches; ikp++) {
            const KeyPoint& kp1 = pKF->mvKeysUn[vMatchedIndices[ikp].first];
            const KeyPoint& kp2 = pKF2->mvKeysUn[vMatchedIndices[ikp].second];
            uv1[2 * ikp] = kp1.pt.x; uv1[2 * ikp + 1] = kp1.pt.y;
            uv2[2 * ikp] = kp2.pt.x; uv2[2 * ikp + 1] = kp2.pt.y;
            oct1[ikp] = (uint8_t)kp1.octave; oct2[ikp] = (uint8_t)kp2.octave;
        }
        vba_triangulate_problem P{};
        std::copy(s1.R, s1.R + 9, P.Rcw1); std::copy(s1.t, s1.t + 3, P.tcw1); std::copy(s1.O, s1.O + 3, P.Ow1); std::copy(s1.K, s1.K + 4, P.K1);
        std::copy(s2.R, s2.R + 9, P.Rcw2); std::copy(s2.t, s2.t + 3, P.tcw2); std::copy(s2.O, s2.O + 3, P.Ow2); std::copy(s2.K, s2.K + 4, P.K2);
        P.n_levels1 = (int32_t)s1.sigma2.size(); P.n_levels2 = (int32_t)s2.sigma2.size();
        P.level_sigma2_1 = s1.sigma2.data(); P.scale_1 = s1.scale.data();
        P.level_sigma2_2 = s2.sigma2.data(); P.scale_2 = s2.scale.data();
        P.ratio_factor = ratioFactor; P.cos_max = 0.9998; P.chi2_th = 5.991;
        P.n_matches = nmatches;
        P.uv1 = uv1.data(); P.uv2 = uv2.data(); P.oct1 = oct1.data(); P.oct2 = oct2.data();
        vba_triangulate_result R{};
        R.x3d = x3d.data(); R.reason = reason.data();
        if (!BackendCall("CreateNewMapPoints", vba_triangulate, P, R)) return -1;
        // :1520-1542 for every accepted match, in match order
        for (int ikp = 0; ikp < nmatches; ikp++) {
            if (reason[ikp] != 0) continue;
            const size_t idx1 = vMatchedIndices[ikp].first, idx2 = vMatchedIndices[ikp].second;
            const float x3D[3] = {(float)x3d[3 * ikp], (float)x3d[3 * ikp + 1], (float)x3d[3 * ikp + 2]};
            MapPoint* pMP = new MapPoint(x3D, pKF);
            pMP->AddObservation(pKF, idx1);
            pMP->AddObservation(pKF2, idx2);
            pKF->AddMapPoint(pMP, idx1);
            pKF2->AddMapPoint(pMP, idx2);
            pMP->UpdateNormalAndDepth();   // a counter here (existing tests pin it); the batched form of the pair is UpdateMapPoints
            pMap->AddMapPoint(pMP);
            lpRecentAddedMapPoints.push_back(pMP);
            nnew++;
        }
    }
    return nnew;
}

}  // namespace

int LocalMapping::CreateNewMapPoints(KeyFrame* pKF, const std::vector<KeyFrame*>& vpNeighKFs, const TriangulationMatcher& matcher, Map* pMap,
                                     std::list<MapPoint*>& lpRecentAddedMapPoints) {
    const FallibleMatcher m = [&matcher](KeyFrame* pKF1, KeyFrame* pKF2, std::vector<std::pair<size_t, size_t>>& v) { matcher(pKF1, pKF2, v); return true; };
    return create_new_map_points(pKF, vpNeighKFs, m, pMap, lpRecentAddedMapPoints);
}

Mat3f LocalMapping::ComputeF12(KeyFrame* pKF1, KeyFrame* pKF2) {
    double R1w[9], t1w[3], R2w[9], t2w[3];
    pKF1->GetRotation(R1w); pKF1->GetTranslation(t1w);
    pKF2->GetRotation(R2w); pKF2->GetTranslation(t2w);
    double R12[9], t12[3];   // R12 = R1w R2w^T, t12 = -R12 t2w + t1w (:1670-1671)
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R12[3 * i + j] = (R1w[3 * i] * R2w[3 * j] + R1w[3 * i + 1] * R2w[3 * j + 1]) + R1w[3 * i + 2] * R2w[3 * j + 2];
    for (int i = 0; i < 3; i++) t12[i] = -((R12[3 * i] * t2w[0] + R12[3 * i + 1] * t2w[1]) + R12[3 * i + 2] * t2w[2]) + t1w[i];
    const double tx[9] = {0, -t12[2], t12[1], t12[2], 0, -t12[0], -t12[1], t12[0], 0};   // SkewSymmetricMatrix (:1673)
    // K^-1 = [1/fx 0 -cx/fx; 0 1/fy -cy/fy; 0 0 1]
    const double K1i[9] = {1.0 / pKF1->fx, 0, -(double)pKF1->cx / pKF1->fx, 0, 1.0 / pKF1->fy, -(double)pKF1->cy / pKF1->fy, 0, 0, 1};
    const double K2i[9] = {1.0 / pKF2->fx, 0, -(double)pKF2->cx / pKF2->fx, 0, 1.0 / pKF2->fy, -(double)pKF2->cy / pKF2->fy, 0, 0, 1};
    auto mul = [](const double* A, const double* B, double* C) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) C[3 * i + j] = (A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j]) + A[3 * i + 2] * B[6 + j];
    };
    const double K1it[9] = {K1i[0], K1i[3], K1i[6], K1i[1], K1i[4], K1i[7], K1i[2], K1i[5], K1i[8]};
    double A[9], B[9], F[9];   // K1.t().inv() * t12x * R12 * K2.inv(), left to right (:1678)
    mul(K1it, tx, A); mul(A, R12, B); mul(B, K2i, F);
    Mat3f out;
    for (int i = 0; i < 9; i++) out[i] = (float)F[i];
    return out;
}

int LocalMapping::SearchInNeighbors(KeyFrame* pKF, const std::vector<KeyFrame*>& vpTargetKFs) {
    ORBmatcher matcher;                                                                    // :1584
    int nFusedAll = 0;
    // step 2 (:1588-1597): the current keyframe's map points into every target
    const std::vector<MapPoint*> vpMapPointMatches = pKF->GetMapPointMatches();
    for (KeyFrame* pKFi : vpTargetKFs) {
        const int n = matcher.Fuse(pKFi, vpMapPointMatches);
        if (n < 0) return -1;
        nFusedAll += n;
    }
    // step 3 (:1600-1632): every good map point of the targets, once, into the current keyframe
    std::vector<MapPoint*> vpFuseCandidates;
    vpFuseCandidates.reserve(vpTargetKFs.size() * vpMapPointMatches.size());
    for (KeyFrame* pKFi : vpTargetKFs) {
        const std::vector<MapPoint*> vpMapPointsKFi = pKFi->GetMapPointMatches();
        for (MapPoint* pMP : vpMapPointsKFi) {
            if (!pMP) continue;
            if (pMP->isBad() || pMP->mnFuseCandidateForKF == pKF->mnId) continue;
            pMP->mnFuseCandidateForKF = pKF->mnId;
            vpFuseCandidates.push_back(pMP);
        }
    }
    const int n = matcher.Fuse(pKF, vpFuseCandidates);
    if (n < 0) return -1;
    return nFusedAll + n;
}

int LocalMapping::CreateNewMapPoints(KeyFrame* pKF, const std::vector<KeyFrame*>& vpNeighKFs, Map* pMap, std::list<MapPoint*>& lpRecentAddedMapPoints) {
    const FallibleMatcher matcher = [](KeyFrame* pKF1, KeyFrame* pKF2, std::vector<std::pair<size_t, size_t>>& vMatchedIndices) {
        const Mat3f F12 = ComputeF12(pKF1, pKF2);                                          // :1314
        ORBmatcher m(0.6, false);                                                          // :1270
        return m.SearchForTriangulation(pKF1, pKF2, F12, vMatchedIndices, false) >= 0;     // :1318
    };
    return create_new_map_points(pKF, vpNeighKFs, matcher, pMap, lpRecentAddedMapPoints);
}

}  // namespace ORB_SLAM2
