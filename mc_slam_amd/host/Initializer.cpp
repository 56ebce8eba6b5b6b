// Initializer.cpp -- see Initializer.h.  Line numbers refer to src/Initializer.cpp of the reference.
#include "Initializer.h"

#include <cstdlib>
#include <cstring>

#include "BackendCall.h"
#include "Sim3Solver.h"

namespace ORB_SLAM2 {

Initializer::Initializer(const Frame& ReferenceFrame, float sigma, int iterations) {                // :27-36
    mK[0] = ReferenceFrame.fx; mK[1] = ReferenceFrame.fy; mK[2] = ReferenceFrame.cx; mK[3] = ReferenceFrame.cy;
    mvKeys1 = ReferenceFrame.mvKeysUn;
    mSigma = sigma;
    mSigma2 = sigma * sigma;
    mMaxIterations = iterations;
    std::memset(&mLast, 0, sizeof mLast);
}

void Initializer::SeedRandOnce(int seed) {
    static bool already_seeded = false;
    if (!already_seeded) {
        srand((unsigned)seed);
        already_seeded = true;
    }
}

void Initializer::DrawSets(int N) {                                                                 // :67-101
    std::vector<size_t> vAllIndices, vAvailableIndices;
    vAllIndices.reserve(N);
    for (int i = 0; i < N; i++) vAllIndices.push_back(i);
    mvSets = std::vector<std::vector<size_t>>(mMaxIterations, std::vector<size_t>(8, 0));
    SeedRandOnce(0);
    for (int it = 0; it < mMaxIterations; it++) {
        vAvailableIndices = vAllIndices;
        for (size_t j = 0; j < 8; j++) {
            const int randi = Sim3Solver::RandomInt(0, (int)vAvailableIndices.size() - 1);
            mvSets[it][j] = vAvailableIndices[randi];
            vAvailableIndices[randi] = vAvailableIndices.back();   // [randi]: the eight indices of a set are distinct
            vAvailableIndices.pop_back();
        }
    }
}

bool Initializer::Initialize(const Frame& CurrentFrame, const std::vector<int>& vMatches12, std::array<float, 9>& R21, std::array<float, 3>& t21,
                             std::vector<Point3f>& vP3D, std::vector<bool>& vbTriangulated) {
    mvKeys2 = CurrentFrame.mvKeysUn;                                                                // :42
    mvMatches12.clear();
    mvMatches12.reserve(mvKeys2.size());
    mvbMatched1.resize(mvKeys1.size());
    for (size_t i = 0, iend = vMatches12.size(); i < iend; i++) {                                   // :51-62
        if (vMatches12[i] >= 0) {
            mvMatches12.push_back(std::make_pair((int)i, vMatches12[i]));
            mvbMatched1[i] = true;
        } else
            mvbMatched1[i] = false;
    }
    const int N = (int)mvMatches12.size();
    if (N < 8) return false;
    DrawSets(N);

    const size_t n1 = mvKeys1.size(), n2 = mvKeys2.size();
    std::vector<double> uv1(2 * n1 + 2), uv2(2 * n2 + 2), x3d(3 * n1 + 3, 0.0);
    for (size_t i = 0; i < n1; i++) { uv1[2 * i] = mvKeys1[i].pt.x; uv1[2 * i + 1] = mvKeys1[i].pt.y; }
    for (size_t i = 0; i < n2; i++) { uv2[2 * i] = mvKeys2[i].pt.x; uv2[2 * i + 1] = mvKeys2[i].pt.y; }
    std::vector<int32_t> match(2 * (size_t)N), sets(8 * (size_t)mMaxIterations + 8);
    for (int i = 0; i < N; i++) { match[2 * i] = mvMatches12[i].first; match[2 * i + 1] = mvMatches12[i].second; }
    for (int it = 0; it < mMaxIterations; it++)
        for (int j = 0; j < 8; j++) sets[8 * (size_t)it + j] = (int32_t)mvSets[it][j];
    std::vector<uint8_t> ih((size_t)N, 0), jf((size_t)N, 0), tri(n1 + 1, 0);

    vba_two_view_problem P;
    std::memset(&P, 0, sizeof P);
    vba_two_view_result R;
    std::memset(&R, 0, sizeof R);
    P.n_keys1 = (int32_t)n1; P.n_keys2 = (int32_t)n2;
    P.uv1 = uv1.data(); P.uv2 = uv2.data();
    P.n_matches = N; P.n_hyp = mMaxIterations;
    P.match = match.data(); P.sets = sets.data();
    std::memcpy(P.K, mK, sizeof mK);
    P.sigma = mSigma;
    P.min_parallax = 1.0;                                                                           // :124-126
    P.min_triangulated = 50;
    R.inlier_h = ih.data(); R.inlier_f = jf.data(); R.x3d = x3d.data(); R.triangulated = tri.data();
    if (!BackendCall("Initializer::Initialize", vba_two_view_init, P, R)) return false;
    mLast = R;
    mLast.inlier_h = mLast.inlier_f = mLast.triangulated = nullptr;
    mLast.x3d = mLast.hyp_score_h = mLast.hyp_score_f = nullptr;
    if (!R.ok) return false;
    for (int i = 0; i < 9; i++) R21[i] = (float)R.R21[i];
    for (int i = 0; i < 3; i++) t21[i] = (float)R.t21[i];
    vP3D.assign(n1, Point3f());
    vbTriangulated.assign(n1, false);
    for (size_t i = 0; i < n1; i++) {
        vP3D[i].x = (float)x3d[3 * i]; vP3D[i].y = (float)x3d[3 * i + 1]; vP3D[i].z = (float)x3d[3 * i + 2];
        vbTriangulated[i] = tri[i] != 0;
    }
    return true;
}

}  // namespace ORB_SLAM2
