// Sim3Solver.cpp -- see Sim3Solver.h.  Line numbers refer to src/Sim3Solver.cpp of the reference.
#include "Sim3Solver.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "BackendCall.h"

namespace ORB_SLAM2 {

Sim3Solver::Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatched12, const bool bFixScale)
    : mnIterations(0), mnBestInliers(0), mbFixScale(bFixScale) {
    mpKF1 = pKF1;
    mpKF2 = pKF2;
    std::memset(mBestS12, 0, sizeof mBestS12);
    const std::vector<MapPoint*> vpKeyFrameMP1 = pKF1->GetMapPointMatches();
    mN1 = (int)vpMatched12.size();
    mvpMatches12 = vpMatched12;
    const Mat4f& T1 = pKF1->GetPose();
    const Mat4f& T2 = pKF2->GetPose();
    // cv::Mat Rcw * X3Dw + tcw (:86-90): CV_32F arithmetic
    auto toCamera = [](const Mat4f& T, const float* Pw, std::vector<double>& out) {
        for (int i = 0; i < 3; i++) {
            float a = T[4 * i] * Pw[0];
            a += T[4 * i + 1] * Pw[1];
            a += T[4 * i + 2] * Pw[2];
            a += T[4 * i + 3];
            out.push_back((double)a);
        }
    };
    size_t idx = 0;
    for (int i1 = 0; i1 < mN1; i1++) {
        if (!vpMatched12[i1]) continue;                                                       // :51
        MapPoint* pMP1 = vpKeyFrameMP1[i1];
        MapPoint* pMP2 = vpMatched12[i1];
        if (!pMP1) continue;                                                                  // :56
        if (pMP1->isBad() || pMP2->isBad()) continue;                                         // :59
        const int indexKF1 = pMP1->GetIndexInKeyFrame(pKF1);
        const int indexKF2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (indexKF1 < 0 || indexKF2 < 0) continue;                                           // :67
        const KeyPoint& kp1 = pKF1->mvKeysUn[indexKF1];
        const KeyPoint& kp2 = pKF2->mvKeysUn[indexKF2];
        const float sigmaSquare1 = pKF1->mvLevelSigma2[kp1.octave];
        const float sigmaSquare2 = pKF2->mvLevelSigma2[kp2.octave];
        mvnMaxError1.push_back((size_t)(9.210 * sigmaSquare1));                               // :78-79 into vector<size_t>
        mvnMaxError2.push_back((size_t)(9.210 * sigmaSquare2));
        mvpMapPoints1.push_back(pMP1);
        mvpMapPoints2.push_back(pMP2);
        mvnIndices1.push_back(i1);
        toCamera(T1, pMP1->mWorldPos, mvX3Dc1);
        toCamera(T2, pMP2->mWorldPos, mvX3Dc2);
        mvAllIndices.push_back(idx);
        idx++;
    }
    mK1[0] = pKF1->fx; mK1[1] = pKF1->fy; mK1[2] = pKF1->cx; mK1[3] = pKF1->cy;               // :97-98
    mK2[0] = pKF2->fx; mK2[1] = pKF2->fy; mK2[2] = pKF2->cx; mK2[3] = pKF2->cy;
    SetRansacParameters();
}

void Sim3Solver::SetRansacParameters(double probability, int minInliers, int maxIterations) {     // :109-134
    mRansacProb = probability;
    mRansacMinInliers = minInliers;
    mRansacMaxIts = maxIterations;
    N = (int)mvpMapPoints1.size();
    const float epsilon = (float)mRansacMinInliers / N;
    int nIterations;
    if (mRansacMinInliers == N)
        nIterations = 1;
    else {
        const double v = std::ceil(std::log(1 - mRansacProb) / std::log(1 - std::pow(epsilon, 3)));
        // the reference converts whatever this is to int; out of range (epsilon > 1, or so small that the logarithm is 0) that
        // conversion gives INT_MIN on x86-64, and the budget becomes 1 below
        nIterations = (v >= (double)INT_MIN && v <= (double)INT_MAX) ? (int)v : INT_MIN;
    }
    mRansacMaxIts = std::max(1, std::min(nIterations, mRansacMaxIts));
    mnIterations = 0;
}

int Sim3Solver::RandomInt(int min, int max) {
    const int d = max - min + 1;
    return int(((double)rand() / ((double)RAND_MAX + 1.0)) * d) + min;
}

void Sim3Solver::DrawTriples(int n, std::vector<int32_t>& triples) {                            // :163-184
    std::vector<size_t> vAvailableIndices;
    for (int h = 0; h < n; h++) {
        vAvailableIndices = mvAllIndices;
        size_t size = vAvailableIndices.size();   // the logical size: the vector itself stays at its capacity
        for (short i = 0; i < 3; i++) {
            const int randi = RandomInt(0, (int)size - 1);
            const int idx = (int)vAvailableIndices[randi];
            triples.push_back(idx);
            vAvailableIndices[idx] = vAvailableIndices[size - 1];   // [idx], not [randi], as it stands (:182)
            size--;
        }
    }
}

bool Sim3Solver::iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, Mat4f& T12) {   // :138-220
    bNoMore = false;
    vbInliers = std::vector<bool>(mN1, false);
    nInliers = 0;
    mvLastTriples.clear();
    if (N < mRansacMinInliers) {
        bNoMore = true;
        return false;
    }
    const int nHyp = std::max(0, std::min(nIterations, mRansacMaxIts - mnIterations));
    DrawTriples(nHyp, mvLastTriples);
    if (nHyp > 0) {
        vba_sim3_ransac_problem P;
        std::memset(&P, 0, sizeof P);
        vba_sim3_ransac_result R;
        std::memset(&R, 0, sizeof R);
        std::vector<double> g1(mvnMaxError1.begin(), mvnMaxError1.end()), g2(mvnMaxError2.begin(), mvnMaxError2.end());
        std::vector<uint8_t> inl((size_t)N + 1, 0);
        P.n_pairs = N;
        P.fix_scale = mbFixScale ? 1 : 0;
        P.p1c = mvX3Dc1.data(); P.p2c = mvX3Dc2.data();
        P.max_err1 = g1.data(); P.max_err2 = g2.data();
        std::memcpy(P.K1, mK1, sizeof mK1);
        std::memcpy(P.K2, mK2, sizeof mK2);
        P.min_inliers = mRansacMinInliers;
        P.n_hyp = nHyp;
        P.sample = mvLastTriples.data();
        P.best_inliers = mnBestInliers;
        std::memcpy(P.best_S12, mBestS12, sizeof mBestS12);
        R.inlier = inl.data();
        if (!BackendCall("Sim3Solver::iterate", vba_sim3_ransac, P, R)) {
            bNoMore = true;
            return false;
        }
        mnIterations += R.its_done;
        mnBestInliers = P.best_inliers;
        std::memcpy(mBestS12, P.best_S12, sizeof mBestS12);
        if (R.hit >= 0) {                                                                     // :203-211
            nInliers = R.n_inliers;
            for (int i = 0; i < N; i++)
                if (inl[i]) vbInliers[mvnIndices1[i]] = true;
            const Matrix3d Rm = QuatToMatrix({{R.S12[3], R.S12[4], R.S12[5], R.S12[6]}});
            T12 = Mat4f{};
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) T12[4 * i + j] = (float)(R.S12[7] * Rm[3 * i + j]);
                T12[4 * i + 3] = (float)R.S12[i];
            }
            T12[15] = 1.0f;
            return true;
        }
    }
    if (mnIterations >= mRansacMaxIts) bNoMore = true;                                        // :215-216
    return false;
}

bool Sim3Solver::find(std::vector<bool>& vbInliers12, int& nInliers, Mat4f& T12) {                // :224-229
    bool bFlag;
    return iterate(mRansacMaxIts, bFlag, vbInliers12, nInliers, T12);
}

std::array<float, 9> Sim3Solver::GetEstimatedRotation() {
    const Matrix3d R = QuatToMatrix({{mBestS12[3], mBestS12[4], mBestS12[5], mBestS12[6]}});
    std::array<float, 9> r;
    for (int i = 0; i < 9; i++) r[i] = (float)R[i];
    return r;
}
std::array<float, 3> Sim3Solver::GetEstimatedTranslation() { return {{(float)mBestS12[0], (float)mBestS12[1], (float)mBestS12[2]}}; }
float Sim3Solver::GetEstimatedScale() { return (float)mBestS12[7]; }

}  // namespace ORB_SLAM2
