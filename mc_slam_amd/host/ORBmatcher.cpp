// ORBmatcher.cpp -- ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:760-955, monocular) over vba_search_triangulation: the
// keyframe pair as flat arrays (descriptors, map-point flags, the feature vectors in CSR form, keypoints, the level tables of
// keyframe 2), the epipole in float32 as :768-775, ONE call, vMatchedPairs from the result.
#include "ORBmatcher.h"

#include <iostream>

#include "../../include/vislam_ba.h"
#include "Optimizer.h"

namespace ORB_SLAM2 {

namespace {
// one keyframe's side of a vba_search_tri_problem
struct MatchSide {
    std::vector<uint8_t> has_mp, oct;
    std::vector<uint32_t> node_id;
    std::vector<int32_t> node_begin, node_feat;
    std::vector<double> uv;
    std::vector<float> angle;
    explicit MatchSide(KeyFrame* kf) {
        const size_t n = (size_t)kf->N;
        has_mp.resize(n); oct.resize(n); uv.resize(2 * n); angle.resize(n);
        for (size_t i = 0; i < n; i++) {
            has_mp[i] = kf->mvpMapPoints[i] != nullptr;
            const KeyPoint& kp = kf->mvKeysUn[i];
            oct[i] = (uint8_t)kp.octave;
            uv[2 * i] = kp.pt.x; uv[2 * i + 1] = kp.pt.y;
            angle[i] = kp.angle;
        }
        node_begin.push_back(0);
        for (const auto& node : kf->mFeatVec) {   // a std::map: ascending node ids
            node_id.push_back(node.first);
            for (unsigned int idx : node.second) node_feat.push_back((int32_t)idx);
            node_begin.push_back((int32_t)node_feat.size());
        }
    }
};
}  // namespace

void ORBmatcher::Epipole(KeyFrame* pKF1, KeyFrame* pKF2, float& ex, float& ey) {
    double Cw[3];
    pKF1->GetCameraCenter(Cw);            // float32 values
    const Mat4f& T2 = pKF2->GetPose();
    float C2[3];                          // R2w * Cw + t2w in float32, left to right like cv::Mat
    for (int i = 0; i < 3; i++) {
        float s = 0;
        for (int k = 0; k < 3; k++) s += T2[4 * i + k] * (float)Cw[k];
        C2[i] = s + T2[4 * i + 3];
    }
    const float invz = 1.0f / C2[2];
    ex = pKF2->fx * C2[0] * invz + pKF2->cx;
    ey = pKF2->fy * C2[1] * invz + pKF2->cy;
}

int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, const Mat3f& F12, std::vector<std::pair<size_t, size_t>>& vMatchedPairs,
                                       const bool bOnlyStereo) {
    vMatchedPairs.clear();
    if (bOnlyStereo) {
        std::cerr << "ORBmatcher::SearchForTriangulation: bOnlyStereo is not supported (the backend is monocular)" << std::endl;
        return -1;
    }
    if ((size_t)pKF1->N != pKF1->mvKeysUn.size() || pKF1->mDescriptors.size() != 32 * (size_t)pKF1->N || pKF1->mvpMapPoints.size() != (size_t)pKF1->N ||
        (size_t)pKF2->N != pKF2->mvKeysUn.size() || pKF2->mDescriptors.size() != 32 * (size_t)pKF2->N || pKF2->mvpMapPoints.size() != (size_t)pKF2->N) {
        std::cerr << "ORBmatcher::SearchForTriangulation: N, mvKeysUn, mvpMapPoints and mDescriptors of a keyframe disagree" << std::endl;
        return -1;
    }
    if (pKF2->mvLevelSigma2.size() != pKF2->mvScaleFactors.size()) {
        std::cerr << "ORBmatcher::SearchForTriangulation: mvLevelSigma2 and mvScaleFactors of keyframe 2 differ in length" << std::endl;
        return -1;
    }
    for (KeyFrame* kf : {pKF1, pKF2})
        for (const KeyPoint& kp : kf->mvKeysUn)
            if (kp.octave < 0 || kp.octave > 255) {   // the ABI carries octaves as uint8; the library checks them against n_levels2
                std::cerr << "ORBmatcher::SearchForTriangulation: a keypoint's octave is outside 0 .. 255" << std::endl;
                return -1;
            }
    const MatchSide s1(pKF1), s2(pKF2);
    const std::vector<double> sigma2(pKF2->mvLevelSigma2.begin(), pKF2->mvLevelSigma2.end()), scale(pKF2->mvScaleFactors.begin(), pKF2->mvScaleFactors.end());
    float ex, ey;
    Epipole(pKF1, pKF2, ex, ey);
    vba_search_tri_problem P{};
    P.n_keys1 = pKF1->N; P.n_keys2 = pKF2->N;
    P.desc1 = pKF1->mDescriptors.data(); P.desc2 = pKF2->mDescriptors.data();
    P.has_mp1 = s1.has_mp.data(); P.has_mp2 = s2.has_mp.data();
    P.n_nodes1 = (int32_t)s1.node_id.size(); P.n_nodes2 = (int32_t)s2.node_id.size();
    P.node_id1 = s1.node_id.data(); P.node_id2 = s2.node_id.data();
    P.node_begin1 = s1.node_begin.data(); P.node_begin2 = s2.node_begin.data();
    P.node_feat1 = s1.node_feat.data(); P.node_feat2 = s2.node_feat.data();
    P.uv1 = s1.uv.data(); P.uv2 = s2.uv.data();
    P.angle1 = s1.angle.data(); P.angle2 = s2.angle.data();
    P.oct2 = s2.oct.data();
    P.n_levels2 = (int32_t)sigma2.size();
    P.level_sigma2_2 = sigma2.data(); P.scale_2 = scale.data();
    for (int i = 0; i < 9; i++) P.F12[i] = F12[i];
    P.epipole[0] = ex; P.epipole[1] = ey;
    P.th_low = TH_LOW;
    P.check_orientation = mbCheckOrientation ? 1 : 0;
    P.chi2_epi = 3.84;
    P.epipole_r2 = 100.0;
    const size_t n1 = (size_t)pKF1->N;
    std::vector<int32_t> match12(n1), pairs(2 * n1);
    std::vector<uint8_t> best_dist(n1), state(n1);
    vba_search_tri_result R{};
    R.match12 = match12.data(); R.best_dist = best_dist.data(); R.state = state.data(); R.pairs = pairs.data();
    vba_search_tri_problem* pp = &P;
    vba_search_tri_result* pr = &R;
    void* h = Optimizer::BackendHandle();
    if (!h || vba_search_triangulation(h, 1, &pp, &pr) != 0) {
        std::cerr << "ORBmatcher::SearchForTriangulation: " << (h ? vba_last_error(h) : "no HIP device (the backend has no CPU path)") << std::endl;
        return -1;
    }
    vMatchedPairs.reserve((size_t)R.n_matches);
    for (int k = 0; k < R.n_matches; k++) vMatchedPairs.emplace_back((size_t)pairs[2 * k], (size_t)pairs[2 * k + 1]);
    return R.n_matches;
}

}  // namespace ORB_SLAM2
