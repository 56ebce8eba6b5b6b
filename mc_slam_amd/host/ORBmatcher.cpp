// ORBmatcher.cpp -- ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:760-955, monocular) over vba_search_triangulation: the
// keyframe pair as flat arrays (descriptors, map-point flags, the feature vectors in CSR form, keypoints, the level tables of
// keyframe 2), the epipole in float32 as :768-775, ONE call, vMatchedPairs from the result.  And both ORBmatcher::Fuse overloads
// (:958-1254, monocular) over vba_fuse: the keyframe with its grid in CSR form and the point list as flat arrays, ONE call for the
// search, then the reference's apply loop in list order on the live map.  And ORBmatcher::SearchBySim3 (:1258-1496, monocular) over
// vba_search_by_sim3: both keyframes as flat arrays with their own map points per keypoint, the vbAlreadyMatched flags of
// :1291-1301, ONE call, vpMatches12 from the agreed matches.  And the two tracking matchers, SearchByProjection(F, vpMapPoints, th)
// (:63-156, fused with Frame::isInFrustum) and SearchByProjection(CurrentFrame, LastFrame, th, bMono) (:1511-1665), over
// vba_search_by_projection: the frame with its grid in CSR form and its occupied flags, the ordered queries, ONE call, then key_match
// applied to mvpMapPoints.  And both ORBmatcher::SearchByBoW overloads (:207-350, :609-748) and their batch forms over vba_search_by_bow:
// every side as flat arrays (descriptors, good-map-point flags, angles, the feature vector in CSR form), ONE call for all pairs,
// then match21 (keyframe -> frame) or match12 (keyframe -> keyframe) turned into map points.  And the loop-closure and the
// relocalisation overload of SearchByProjection (:354-475, :1667-1797) over vba_search_by_projection_kf: the target with its grid in CSR
// form and its occupied flags, the ordered queries, ONE call, then key_match applied to vpMatched / mvpMapPoints.
#include "ORBmatcher.h"

#include <cstring>
#include <iostream>
#include <map>
#include <set>
#include <string>

#include "../../include/vislam_ba.h"
#include "BackendCall.h"

namespace ORB_SLAM2 {

namespace {
// mFeatVec of a KeyFrame or Frame in CSR form: node k lists node_feat[node_begin[k] .. node_begin[k + 1])
struct FeatVecCsr {
    std::vector<uint32_t> node_id;
    std::vector<int32_t> node_begin, node_feat;
    void fill(const std::map<unsigned int, std::vector<unsigned int>>& fv) {
        node_begin.push_back(0);
        for (const auto& node : fv) {   // a std::map: ascending node ids
            node_id.push_back(node.first);
            for (unsigned int idx : node.second) node_feat.push_back((int32_t)idx);
            node_begin.push_back((int32_t)node_feat.size());
        }
    }
};

// one keyframe's side of a vba_search_tri_problem
struct MatchSide : FeatVecCsr {
    std::vector<uint8_t> has_mp, oct;
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
        fill(kf->mFeatVec);
    }
};

// A KeyFrame or Frame as the target of a projection search: the checks every entry point makes, the keypoints and the level table
// as flat arrays, mGrid in CSR form (cell (ix, iy) at ix * mnGridRows + iy), and the fields the four problem structs share
template <class T>
struct SearchTarget {
    const T* f = nullptr;
    std::vector<double> uv, scale;
    std::vector<uint8_t> oct;
    std::vector<float> angle;
    std::vector<int32_t> cell_begin, cell_feat;
    // noun: "the keyframe", "a keyframe", "the frame".  n_points: the length of the map-point list that goes with the keypoints.
    // more_levels: a further per-level table, which level_tables then names.  false: refused, with the message on std::cerr
    bool fill(const char* who, const std::string& noun, const T& F, size_t n_points, const char* level_tables = "mnScaleLevels and mvScaleFactors",
              const std::vector<float>* more_levels = nullptr) {
        const auto refuse = [&](const std::string& why) { std::cerr << who << ": " << why << std::endl; return false; };
        const size_t nk = (size_t)F.N, nl = (size_t)F.mnScaleLevels;
        if (nk != F.mvKeysUn.size() || F.mDescriptors.size() != 32 * nk || n_points != nk || F.mvuRight.size() != nk)
            return refuse("N, mvKeysUn, mvuRight, mvpMapPoints and mDescriptors of " + noun + " disagree");
        if (F.mnScaleLevels < 1 || F.mvScaleFactors.size() != nl || (more_levels && more_levels->size() != nl))
            return refuse(level_tables + (" of " + noun) + " disagree");
        if (F.mnGridCols < 1 || F.mnGridRows < 1 || F.mGrid.size() != (size_t)F.mnGridCols) return refuse(noun + " has no grid");
        uv.resize(2 * nk); oct.resize(nk);
        for (size_t i = 0; i < nk; i++) {
            const KeyPoint& kp = F.mvKeysUn[i];
            if (F.mvuRight[i] >= 0) return refuse(noun + " has a stereo keypoint (the backend is monocular)");
            if (kp.octave < 0 || kp.octave > 255)   // the ABI carries octaves as uint8; the library checks them against n_levels
                return refuse("a keypoint's octave is outside 0 .. 255");
            uv[2 * i] = kp.pt.x; uv[2 * i + 1] = kp.pt.y; oct[i] = (uint8_t)kp.octave;
        }
        cell_begin.reserve((size_t)F.mnGridCols * (size_t)F.mnGridRows + 1); cell_feat.reserve(nk);
        cell_begin.assign(1, 0);
        for (int ix = 0; ix < F.mnGridCols; ix++) {
            if (F.mGrid[(size_t)ix].size() != (size_t)F.mnGridRows) return refuse(noun + " has no grid");   // a ragged column
            for (int iy = 0; iy < F.mnGridRows; iy++) {
                for (size_t idx : F.mGrid[(size_t)ix][(size_t)iy]) cell_feat.push_back((int32_t)idx);
                cell_begin.push_back((int32_t)cell_feat.size());
            }
        }
        scale.assign(F.mvScaleFactors.begin(), F.mvScaleFactors.end());
        f = &F;
        return true;
    }
    // vba_fuse_problem, vba_search_sim3_kf, vba_search_proj_problem, vba_search_proj_kf_problem: K and the keypoints' angles where the
    // struct has them
    template <class P>
    void bind(P& p) {
        BindK(p, 0); BindAngle(p, 0);
        p.bounds[0] = f->mnMinX; p.bounds[1] = f->mnMaxX; p.bounds[2] = f->mnMinY; p.bounds[3] = f->mnMaxY;
        p.n_keys = f->N; p.n_levels = f->mnScaleLevels;
        p.desc = f->mDescriptors.data(); p.uv = uv.data(); p.oct = oct.data(); p.scale = scale.data();
        p.log_scale_factor = f->mfLogScaleFactor;
        p.grid_cols = f->mnGridCols; p.grid_rows = f->mnGridRows; p.grid_inv_w = f->mfGridElementWidthInv; p.grid_inv_h = f->mfGridElementHeightInv;
        p.cell_begin = cell_begin.data(); p.cell_feat = cell_feat.data();
    }
    template <class P> auto BindK(P& p, int) const -> decltype((void)p.K) { p.K[0] = f->fx; p.K[1] = f->fy; p.K[2] = f->cx; p.K[3] = f->cy; }
    template <class P> void BindK(P&, long) const {}
    template <class P> auto BindAngle(P& p, int) -> decltype((void)p.angle) {
        angle.resize(f->mvKeysUn.size());
        for (size_t i = 0; i < angle.size(); i++) angle[i] = f->mvKeysUn[i].angle;
        p.angle = angle.data();
    }
    template <class P> void BindAngle(P&, long) {}
};

// the arrays of a list of map points; zeros where point() was not called.  normals: false for vba_search_sim3_kf, which has none
struct PointBlock {
    std::vector<double> pos, normal, dmin, dmax, pmax;
    std::vector<uint8_t> desc;
    explicit PointBlock(size_t n = 0, bool normals = true) : pos(3 * n), normal(normals ? 3 * n : 0), dmin(n), dmax(n), pmax(n), desc(32 * n) {}
    void point(size_t i, MapPoint* pMP) {
        pMP->GetWorldPos(&pos[3 * i]);
        if (!normal.empty()) pMP->GetNormal(&normal[3 * i]);
        dmin[i] = pMP->GetMinDistanceInvariance(); dmax[i] = pMP->GetMaxDistanceInvariance(); pmax[i] = pMP->mfMaxDistance;
        std::memcpy(&desc[32 * i], pMP->GetDescriptor(), 32);
    }
    template <class P>   // vba_fuse_problem (which also takes `normal`), vba_search_sim3_kf
    void bind_points(P& p) const {
        p.pos = pos.data(); p.dist_min = dmin.data(); p.dist_max = dmax.data(); p.pred_max = pmax.data(); p.pt_desc = desc.data();
    }
    template <class P>   // the queries of vba_search_proj_problem, vba_search_proj_kf_problem
    void bind_queries(P& p) const {
        p.q_pos = pos.data(); p.q_desc = desc.data(); p.q_normal = normal.data(); p.q_dist_min = dmin.data(); p.q_dist_max = dmax.data();
        p.q_pred_max = pmax.data();
    }
};

// R, t and Ow = -R^T t of the float32 4x4 T with its upper three rows divided by `div`, in float32 like cv::Mat
void PoseParts(const Mat4f& T, float div, double Rcw[9], double tcw[3], double Ow[3]) {
    float Rf[9], tf[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Rf[3 * i + j] = T[4 * i + j] / div;
        tf[i] = T[4 * i + 3] / div;
    }
    for (int i = 0; i < 9; i++) Rcw[i] = Rf[i];
    for (int i = 0; i < 3; i++) {
        tcw[i] = tf[i];
        float a = 0;
        for (int k = 0; k < 3; k++) a += -Rf[3 * k + i] * tf[k];
        Ow[i] = a;
    }
}

// src/ORBmatcher.cpp:364-368 and :1134-1138: scw = |row 0 of sRcw|, Rcw = sRcw / scw, tcw = Scw[0:3, 3] / scw, Ow = -Rcw^T tcw
void DecomposeScw(const Mat4f& Scw, double Rcw[9], double tcw[3], double Ow[3]) {
    PoseParts(Scw, std::sqrt(Scw[0] * Scw[0] + Scw[1] * Scw[1] + Scw[2] * Scw[2]), Rcw, tcw, Ow);
}
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
    if (!BackendCall("ORBmatcher::SearchForTriangulation", vba_search_triangulation, P, R)) return -1;
    vMatchedPairs.reserve((size_t)R.n_matches);
    for (int k = 0; k < R.n_matches; k++) vMatchedPairs.emplace_back((size_t)pairs[2 * k], (size_t)pairs[2 * k + 1]);
    return R.n_matches;
}

namespace {
// the search half of both Fuse overloads: one vba_fuse problem.  skip[i] is the caller's test of :980-984 / :1154
struct FuseSearch {
    std::vector<int32_t> best_idx;
    std::vector<uint8_t> state;
    bool run(const char* who, KeyFrame* pKF, const double Rcw[9], const double tcw[3], const double Ow[3], const std::vector<MapPoint*>& pts,
             const std::vector<uint8_t>& skip, double th, bool check_reproj) {
        SearchTarget<KeyFrame> t;
        if (!t.fill(who, "the keyframe", *pKF, pKF->mvpMapPoints.size(), "mnScaleLevels, mvScaleFactors and mvInvLevelSigma2", &pKF->mvInvLevelSigma2))
            return false;
        const std::vector<double> inv_sigma2(pKF->mvInvLevelSigma2.begin(), pKF->mvInvLevelSigma2.end());
        const size_t np = pts.size();
        PointBlock q(np);
        for (size_t i = 0; i < np; i++)
            if (pts[i]) q.point(i, pts[i]);   // every point of the list, the skipped ones included; NULL: zeros
        vba_fuse_problem P{};
        std::memcpy(P.Rcw, Rcw, 72); std::memcpy(P.tcw, tcw, 24); std::memcpy(P.Ow, Ow, 24);
        t.bind(P);
        q.bind_points(P);
        P.normal = q.normal.data(); P.inv_level_sigma2 = inv_sigma2.data();
        P.n_pt = (int32_t)np; P.th_low = ORBmatcher::TH_LOW; P.skip = skip.data();
        P.th = th; P.cos_view = 0.5; P.check_reproj = check_reproj ? 1 : 0; P.chi2_reproj = 5.99;
        best_idx.assign(np, -1); state.assign(np, 1);
        std::vector<uint16_t> best_dist(np);
        std::vector<int8_t> level(np);
        std::vector<double> puv(2 * np);
        vba_fuse_result R{};
        R.best_idx = best_idx.data(); R.best_dist = best_dist.data(); R.level = level.data(); R.uv = puv.data(); R.state = state.data();
        return BackendCall(who, vba_fuse, P, R);
    }
};
}  // namespace

int ORBmatcher::Fuse(KeyFrame* pKF, const std::vector<MapPoint*>& vpMapPoints, const float th) {
    double Rcw[9], tcw[3], Ow[3];
    pKF->GetRotation(Rcw); pKF->GetTranslation(tcw); pKF->GetCameraCenter(Ow);
    const size_t nMPs = vpMapPoints.size();
    std::vector<uint8_t> skip(nMPs);
    for (size_t i = 0; i < nMPs; i++) {
        MapPoint* pMP = vpMapPoints[i];
        skip[i] = !pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF);   // :980-984
    }
    FuseSearch s;
    if (!s.run("ORBmatcher::Fuse", pKF, Rcw, tcw, Ow, vpMapPoints, skip, th, true)) return -1;
    int nFused = 0;
    for (size_t i = 0; i < nMPs; i++) {
        MapPoint* pMP = vpMapPoints[i];
        if (!pMP) continue;
        if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;   // :983 on the live map: a point only moves from searched to skipped
        if (s.state[i] != 0) continue;
        const size_t bestIdx = (size_t)s.best_idx[i];
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);          // :1097-1114
        if (pMPinKF) {
            if (!pMPinKF->isBad()) {
                if (pMPinKF->Observations() > pMP->Observations())
                    pMP->Replace(pMPinKF);
                else
                    pMPinKF->Replace(pMP);
            }
        } else {
            pMP->AddObservation(pKF, bestIdx);
            pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused++;
    }
    return nFused;
}

int ORBmatcher::Fuse(KeyFrame* pKF, const Mat4f& Scw, const std::vector<MapPoint*>& vpPoints, float th, std::vector<MapPoint*>& vpReplacePoint) {
    double Rcw[9], tcw[3], Ow[3];
    DecomposeScw(Scw, Rcw, tcw, Ow);                                  // :1134-1138
    const std::set<MapPoint*> spAlreadyFound = pKF->GetMapPoints();   // :1141
    const size_t nPoints = vpPoints.size();
    std::vector<uint8_t> skip(nPoints);
    for (size_t i = 0; i < nPoints; i++) {
        MapPoint* pMP = vpPoints[i];
        skip[i] = !pMP || pMP->isBad() || spAlreadyFound.count(pMP);   // :1154
    }
    FuseSearch s;
    if (!s.run("ORBmatcher::Fuse (Sim3)", pKF, Rcw, tcw, Ow, vpPoints, skip, th, false)) return -1;
    int nFused = 0;
    for (size_t iMP = 0; iMP < nPoints && iMP < vpReplacePoint.size(); iMP++) {
        MapPoint* pMP = vpPoints[iMP];
        if (!pMP || skip[iMP]) continue;
        if (pMP->isBad()) continue;                               // :1154 on the live map
        if (s.state[iMP] != 0) continue;
        const size_t bestIdx = (size_t)s.best_idx[iMP];
        MapPoint* pMPinKF = pKF->GetMapPoint(bestIdx);           // :1236-1249
        if (pMPinKF) {
            if (!pMPinKF->isBad()) vpReplacePoint[iMP] = pMPinKF;
        } else {
            pMP->AddObservation(pKF, bestIdx);
            pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused++;
    }
    return nFused;
}

namespace {
// one keyframe's side of a vba_search_sim3_problem: the keyframe as a search target and its own map points per keypoint
struct Sim3Side {
    SearchTarget<KeyFrame> t;
    PointBlock q;
    std::vector<uint8_t> has_pt;
    bool fill(const char* who, KeyFrame* pKF, const std::vector<MapPoint*>& pts, const std::vector<uint8_t>& matched, vba_search_sim3_kf& S) {
        if (!t.fill(who, "a keyframe", *pKF, pts.size())) return false;
        q = PointBlock(pts.size(), false); has_pt.assign(pts.size(), 0);
        for (size_t i = 0; i < pts.size(); i++) {
            MapPoint* pMP = pts[i];
            if (!pMP || pMP->isBad()) continue;       // :1314-1318
            has_pt[i] = 1;
            q.point(i, pMP);
        }
        pKF->GetRotation(S.Rcw); pKF->GetTranslation(S.tcw);
        t.bind(S);
        q.bind_points(S);
        S.has_pt = has_pt.data(); S.matched = matched.data();
        return true;
    }
};
}  // namespace

void ORBmatcher::AlreadyMatched(KeyFrame* pKF1, KeyFrame* pKF2, const std::vector<MapPoint*>& vpMatches12, std::vector<uint8_t>& vb1,
                                std::vector<uint8_t>& vb2) {
    const int N1 = (int)pKF1->mvpMapPoints.size(), N2 = (int)pKF2->mvpMapPoints.size();
    vb1.assign((size_t)N1, 0); vb2.assign((size_t)N2, 0);
    for (int i = 0; i < N1 && i < (int)vpMatches12.size(); i++) {   // :1291-1301
        MapPoint* pMP = vpMatches12[(size_t)i];
        if (pMP) {
            vb1[(size_t)i] = 1;
            const int idx2 = pMP->GetIndexInKeyFrame(pKF2);
            if (idx2 >= 0 && idx2 < N2) vb2[(size_t)idx2] = 1;
        }
    }
}

int ORBmatcher::SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12, const float& s12, const Mat3f& R12,
                             const std::array<float, 3>& t12, const float th) {
    const char* who = "ORBmatcher::SearchBySim3";
    const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches(), vpMapPoints2 = pKF2->GetMapPointMatches();
    const size_t N1 = vpMapPoints1.size(), N2 = vpMapPoints2.size();
    if (vpMatches12.size() != N1) {
        std::cerr << who << ": vpMatches12 must have one entry per keypoint of pKF1" << std::endl;
        return -1;
    }
    std::vector<uint8_t> vb1, vb2;
    AlreadyMatched(pKF1, pKF2, vpMatches12, vb1, vb2);
    vba_search_sim3_problem P{};
    Sim3Side s1, s2;
    if (!s1.fill(who, pKF1, vpMapPoints1, vb1, P.kf1) || !s2.fill(who, pKF2, vpMapPoints2, vb2, P.kf2)) return -1;
    P.K[0] = pKF1->fx; P.K[1] = pKF1->fy; P.K[2] = pKF1->cx; P.K[3] = pKF1->cy;   // :1262-1265: pKF1's, in both directions
    P.s12 = s12;
    for (int i = 0; i < 9; i++) P.R12[i] = R12[(size_t)i];
    for (int i = 0; i < 3; i++) P.t12[i] = t12[(size_t)i];
    P.th = th; P.th_high = TH_HIGH;
    std::vector<int32_t> match1(N1), match2(N2), match12(N1);
    std::vector<uint16_t> dist1(N1), dist2(N2);
    std::vector<int8_t> level1(N1), level2(N2);
    std::vector<uint8_t> state1(N1), state2(N2);
    vba_search_sim3_result R{};
    R.match1 = match1.data(); R.match2 = match2.data(); R.best_dist1 = dist1.data(); R.best_dist2 = dist2.data();
    R.level1 = level1.data(); R.level2 = level2.data(); R.state1 = state1.data(); R.state2 = state2.data(); R.match12 = match12.data();
    if (!BackendCall(who, vba_search_by_sim3, P, R)) return -1;
    for (size_t i1 = 0; i1 < N1; i1++)
        if (match12[i1] >= 0) vpMatches12[i1] = vpMapPoints2[(size_t)match12[i1]];   // :1489
    return R.n_found;
}

namespace {
// One vba_search_by_projection problem over a Frame: its keypoints, grid and occupied flags, and the call.  The caller fills the
// query arrays and the mode's fields of P in front of run(); afterwards key_match is applied to F.mvpMapPoints
struct ProjSearch {
    vba_search_proj_problem P{};
    vba_search_proj_result R{};
    SearchTarget<Frame> t;
    std::vector<uint8_t> occupied;
    std::vector<int32_t> key_match, best_idx;
    std::vector<uint16_t> best_dist, best_dist2;
    std::vector<int8_t> level;
    std::vector<double> view_cos, puv;
    std::vector<uint8_t> bin, state;
    bool frame(const char* who, Frame& F) {
        if (!t.fill(who, "the frame", F, F.mvpMapPoints.size())) return false;
        const size_t nk = (size_t)F.N;
        occupied.resize(nk);
        for (size_t i = 0; i < nk; i++) occupied[i] = F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0;   // :113-115, :1596-1598 in front of the call
        t.bind(P);
        P.occupied = occupied.data();
        P.th_high = ORBmatcher::TH_HIGH;
        key_match.assign(nk, -1);
        R.key_match = key_match.data();
        return true;
    }
    bool run(const char* who, size_t nq) {
        P.n_q = (int32_t)nq;
        best_idx.assign(nq, -1); best_dist.assign(nq, 256); best_dist2.assign(nq, 256); level.assign(nq, -128); view_cos.assign(nq, 0.0); puv.assign(2 * nq, 0.0);
        bin.assign(nq, 255); state.assign(nq, 1);
        R.best_idx = best_idx.data(); R.best_dist = best_dist.data(); R.best_dist2 = best_dist2.data(); R.level = level.data(); R.view_cos = view_cos.data();
        R.uv = puv.data(); R.bin = bin.data(); R.state = state.data();
        return BackendCall(who, vba_search_by_projection, P, R);
    }
    // what the function leaves in mvpMapPoints: the last query that wrote a keypoint, NULL where the orientation filter cleared it
    void apply(Frame& F, const std::vector<MapPoint*>& queries) const {
        for (size_t k = 0; k < key_match.size(); k++) {
            if (key_match[k] >= 0) F.mvpMapPoints[k] = queries[(size_t)key_match[k]];
            else if (key_match[k] == -2) F.mvpMapPoints[k] = nullptr;
        }
    }
};

// the per-point arrays both modes read
struct ProjQueries : PointBlock {
    std::vector<uint8_t> skip, blocks;
    explicit ProjQueries(size_t n) : PointBlock(n), skip(n, 1), blocks(n) {}
    void point(size_t i, MapPoint* pMP) {
        PointBlock::point(i, pMP);
        blocks[i] = pMP->Observations() > 0;
    }
    void bind(vba_search_proj_problem& P) const {
        bind_queries(P);
        P.q_skip = skip.data(); P.q_blocks = blocks.data();
    }
};
}  // namespace

int SearchLocalMap(const char* who, Frame& F, const std::vector<MapPoint*>& vpMapPoints, const std::vector<uint8_t>& skip, float th, float nnratio,
                   int* in_view) {
    ProjSearch s;
    if (!s.frame(who, F)) return -1;
    const size_t n = vpMapPoints.size();
    ProjQueries q(n);
    for (size_t i = 0; i < n; i++) {
        q.skip[i] = skip[i];
        if (!skip[i]) q.point(i, vpMapPoints[i]);
    }
    q.bind(s.P);
    s.P.mode = VBA_SEARCH_PROJ_LOCAL_MAP;
    for (int i = 0; i < 9; i++) s.P.Rcw[i] = F.mRcw[i];
    for (int i = 0; i < 3; i++) { s.P.tcw[i] = F.mtcw[i]; s.P.Ow[i] = F.mOw[i]; }
    s.P.th = th; s.P.nn_ratio = nnratio; s.P.cos_view = 0.5;
    if (!s.run(who, n)) return -1;
    int seen = 0;
    for (size_t i = 0; i < n; i++) {
        if (skip[i]) continue;
        MapPoint* pMP = vpMapPoints[i];
        const int st = s.state[i];
        pMP->mbTrackInView = st == 0 || st >= 7;                  // Frame.cpp:494, :541-546
        if (!pMP->mbTrackInView) continue;
        pMP->mTrackProjX = (float)s.puv[2 * i]; pMP->mTrackProjY = (float)s.puv[2 * i + 1];
        pMP->mnTrackScaleLevel = s.level[i]; pMP->mTrackViewCos = (float)s.view_cos[i];
        seen++;
    }
    if (in_view) *in_view = seen;
    s.apply(F, vpMapPoints);
    return s.R.n_matches;
}

int ORBmatcher::SearchByProjection(Frame& F, const std::vector<MapPoint*>& vpMapPoints, const float th) {
    std::vector<uint8_t> skip(vpMapPoints.size());
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
        MapPoint* pMP = vpMapPoints[i];
        skip[i] = !pMP || !pMP->mbTrackInView || pMP->isBad();    // :74-78
    }
    return SearchLocalMap("ORBmatcher::SearchByProjection", F, vpMapPoints, skip, th, mfNNratio, nullptr);
}

int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono) {
    const char* who = "ORBmatcher::SearchByProjection (last frame)";
    if (!bMono) {
        std::cerr << who << ": bMono is false (the backend is monocular)" << std::endl;
        return -1;
    }
    const size_t n = (size_t)LastFrame.N;
    if (LastFrame.mvpMapPoints.size() != n || LastFrame.mvbOutlier.size() != n || LastFrame.mvKeys.size() != n || LastFrame.mvKeysUn.size() != n) {
        std::cerr << who << ": N, mvKeys, mvKeysUn, mvpMapPoints and mvbOutlier of the last frame disagree" << std::endl;
        return -1;
    }
    ProjSearch s;
    if (!s.frame(who, CurrentFrame)) return -1;
    ProjQueries q(n);
    std::vector<uint8_t> q_oct(n);
    std::vector<float> q_angle(n);
    for (size_t i = 0; i < n; i++) {
        MapPoint* pMP = LastFrame.mvpMapPoints[i];
        q.skip[i] = !pMP || LastFrame.mvbOutlier[i];              // :1540-1542
        if (q.skip[i]) continue;
        if (LastFrame.mvKeys[i].octave < 0 || LastFrame.mvKeys[i].octave > 255) {
            std::cerr << who << ": a keypoint's octave is outside 0 .. 255" << std::endl;
            return -1;
        }
        q.point(i, pMP);
        q_oct[i] = (uint8_t)LastFrame.mvKeys[i].octave;           // :1564
        q_angle[i] = LastFrame.mvKeysUn[i].angle;                 // :1628
    }
    q.bind(s.P);
    s.P.q_oct = q_oct.data(); s.P.q_angle = q_angle.data();
    s.P.mode = VBA_SEARCH_PROJ_LAST_FRAME;
    s.P.check_orientation = mbCheckOrientation ? 1 : 0;
    for (int i = 0; i < 3; i++) {                                 // :1521-1522
        for (int j = 0; j < 3; j++) s.P.Rcw[3 * i + j] = CurrentFrame.mTcw[4 * i + j];
        s.P.tcw[i] = CurrentFrame.mTcw[4 * i + 3];
    }
    s.P.th = th;
    if (!s.run(who, n)) return -1;
    s.apply(CurrentFrame, LastFrame.mvpMapPoints);
    return s.R.n_matches;
}

// ---- SearchByProjection for loop closure and relocalisation ----
namespace {
// One vba_search_by_projection_kf problem over a target T (a KeyFrame in loop mode, a Frame in reloc mode): its keypoints and grid,
// the ordered queries, and the call.  The caller fills mode, pose, thresholds and `occupied` in front of run(); key_match comes back
template <class T>
struct KfProjSearch {
    vba_search_proj_kf_problem P{};
    vba_search_proj_kf_result R{};
    SearchTarget<T> t;
    PointBlock q;
    std::vector<double> puv;
    std::vector<uint8_t> occupied, skip, bin, state;
    std::vector<float> q_angle;
    std::vector<int32_t> key_match, best_idx;
    std::vector<uint16_t> best_dist;
    std::vector<int8_t> level;
    bool target(const char* who, const char* noun, T& F) {
        if (!t.fill(who, noun, F, F.mvpMapPoints.size())) return false;
        t.bind(P);
        occupied.assign((size_t)F.N, 0);
        key_match.assign((size_t)F.N, -1);
        return true;
    }
    void queries(size_t n) {
        q = PointBlock(n);
        skip.assign(n, 1); q_angle.assign(n, 0.0f);
    }
    void point(size_t i, MapPoint* pMP) {
        skip[i] = 0;
        q.point(i, pMP);
    }
    bool run(const char* who) {
        const size_t nq = skip.size();
        P.occupied = occupied.data();
        P.n_q = (int32_t)nq;
        q.bind_queries(P);
        P.q_skip = skip.data(); P.q_angle = q_angle.data();
        best_idx.assign(nq, -1); best_dist.assign(nq, 256); level.assign(nq, -128); puv.assign(2 * nq, 0.0); bin.assign(nq, 255); state.assign(nq, 1);
        R.best_idx = best_idx.data(); R.best_dist = best_dist.data(); R.level = level.data(); R.uv = puv.data(); R.bin = bin.data();
        R.state = state.data(); R.key_match = key_match.data();
        return BackendCall(who, vba_search_by_projection_kf, P, R);
    }
};
}  // namespace

int ORBmatcher::SearchByProjection(KeyFrame* pKF, const Mat4f& Scw, const std::vector<MapPoint*>& vpPoints, std::vector<MapPoint*>& vpMatched, int th) {
    const char* who = "ORBmatcher::SearchByProjection (loop)";
    KfProjSearch<KeyFrame> s;
    if (!s.target(who, "the keyframe", *pKF)) return -1;
    if (vpMatched.size() != (size_t)pKF->N) {
        std::cerr << who << ": vpMatched does not have one entry per keypoint of the keyframe" << std::endl;
        return -1;
    }
    s.P.mode = VBA_SEARCH_PROJ_KF_LOOP;
    DecomposeScw(Scw, s.P.Rcw, s.P.tcw, s.P.Ow);                                  // :364-368
    std::set<MapPoint*> spAlreadyFound(vpMatched.begin(), vpMatched.end());        // :372-373, not updated by the matches of the call
    spAlreadyFound.erase(static_cast<MapPoint*>(nullptr));
    for (size_t k = 0; k < vpMatched.size(); k++) s.occupied[k] = vpMatched[k] != nullptr;   // :446
    const size_t n = vpPoints.size();
    s.queries(n);
    for (size_t i = 0; i < n; i++) {
        MapPoint* pMP = vpPoints[i];
        if (!pMP || pMP->isBad() || spAlreadyFound.count(pMP)) continue;           // :385; a NULL entry is skipped
        s.point(i, pMP);
    }
    s.P.th = th; s.P.th_dist = TH_LOW; s.P.cos_view = 0.5;
    if (!s.run(who)) return -1;
    for (size_t k = 0; k < s.key_match.size(); k++)
        if (s.key_match[k] >= 0) vpMatched[k] = vpPoints[(size_t)s.key_match[k]];  // :468
    return s.R.n_matches;
}

int ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const std::set<MapPoint*>& sAlreadyFound, const float th, const int ORBdist) {
    const char* who = "ORBmatcher::SearchByProjection (relocalisation)";
    KfProjSearch<Frame> s;
    if (!s.target(who, "the frame", CurrentFrame)) return -1;
    const std::vector<MapPoint*> vpMPs = pKF->GetMapPointMatches();               // :1682
    const size_t n = vpMPs.size();
    if (pKF->mvKeysUn.size() != n) {
        std::cerr << who << ": mvKeysUn and mvpMapPoints of the keyframe disagree" << std::endl;
        return -1;
    }
    s.P.mode = VBA_SEARCH_PROJ_KF_RELOC;
    s.P.check_orientation = mbCheckOrientation ? 1 : 0;
    PoseParts(CurrentFrame.mTcw, 1.0f, s.P.Rcw, s.P.tcw, s.P.Ow);                 // :1672-1674 in float32 like cv::Mat
    for (size_t k = 0; k < s.occupied.size(); k++) s.occupied[k] = CurrentFrame.mvpMapPoints[k] != nullptr;   // :1738
    s.queries(n);
    for (size_t i = 0; i < n; i++) {
        MapPoint* pMP = vpMPs[i];
        if (!pMP || pMP->isBad() || sAlreadyFound.count(pMP)) continue;            // :1688-1690
        s.point(i, pMP);
        s.q_angle[i] = pKF->mvKeysUn[i].angle;                                    // :1760
    }
    s.P.th = th; s.P.th_dist = ORBdist;
    if (!s.run(who)) return -1;
    for (size_t k = 0; k < s.key_match.size(); k++) {
        if (s.key_match[k] >= 0) CurrentFrame.mvpMapPoints[k] = vpMPs[(size_t)s.key_match[k]];   // :1754
        else if (s.key_match[k] == -2) CurrentFrame.mvpMapPoints[k] = nullptr;                   // :1789
    }
    return s.R.n_matches;
}

// ---- SearchByBoW ----
namespace {
// one side of a vba_search_bow_problem: a KeyFrame (angles of mvKeysUn, :700) or a Frame (angles of mvKeys, :296)
struct BowSide : FeatVecCsr {
    int n = 0;
    const unsigned char* desc = nullptr;
    const std::vector<MapPoint*>* points = nullptr;
    std::vector<uint8_t> good;
    std::vector<float> angle;
    bool ok = false;
    template <class F>
    void fill(const F& f, const std::vector<KeyPoint>& keys) {
        n = f.N;
        ok = keys.size() == (size_t)f.N && f.mDescriptors.size() == 32 * (size_t)f.N && f.mvpMapPoints.size() == (size_t)f.N;
        if (!ok) return;
        desc = f.mDescriptors.data();
        points = &f.mvpMapPoints;
        good.resize((size_t)n); angle.resize((size_t)n);
        for (size_t i = 0; i < (size_t)n; i++) {
            MapPoint* pMP = f.mvpMapPoints[i];
            good[i] = pMP && !pMP->isBad();                       // :243-247, :649-652, :665-671
            angle[i] = keys[i].angle;
        }
        FeatVecCsr::fill(f.mFeatVec);
    }
    explicit BowSide(KeyFrame* kf) { fill(*kf, kf->mvKeysUn); }
    explicit BowSide(const Frame& f) { fill(f, f.mvKeys); }
};

// the result arrays of one pair
struct BowOut {
    std::vector<int32_t> match12, best_idx, match21;
    std::vector<uint16_t> best_dist, best_dist2;
    std::vector<uint8_t> bin, state;
    vba_search_bow_result R{};
    BowOut(size_t n1, size_t n2) : match12(n1), best_idx(n1), match21(n2), best_dist(n1), best_dist2(n1), bin(n1), state(n1) {
        R.match12 = match12.data(); R.best_idx = best_idx.data(); R.best_dist = best_dist.data(); R.best_dist2 = best_dist2.data();
        R.bin = bin.data(); R.state = state.data(); R.match21 = match21.data();
    }
};

// ONE vba_search_by_bow call over the pairs (side1[i], side2[i]) of `mode`
bool RunBow(const char* who, int mode, const std::vector<const BowSide*>& side1, const std::vector<const BowSide*>& side2, float nnratio, bool check_ori,
            std::vector<BowOut>& out) {
    const size_t n = side1.size();
    std::vector<vba_search_bow_problem> P(n);
    std::vector<vba_search_bow_problem*> pp(n);
    std::vector<vba_search_bow_result*> pr(n);
    out.clear();
    out.reserve(n);
    for (size_t i = 0; i < n; i++) {
        const BowSide &a = *side1[i], &b = *side2[i];
        if (!a.ok || !b.ok) {
            std::cerr << who << ": N, the keypoints, mvpMapPoints and mDescriptors of a keyframe or frame disagree" << std::endl;
            return false;
        }
        vba_search_bow_problem& p = P[i];
        p = vba_search_bow_problem{};
        p.mode = mode; p.check_orientation = check_ori ? 1 : 0; p.th_low = ORBmatcher::TH_LOW; p.nn_ratio = nnratio;
        p.n_keys1 = a.n; p.n_keys2 = b.n;
        p.desc1 = a.desc; p.desc2 = b.desc;
        p.good_mp1 = a.good.data(); p.good_mp2 = b.good.data();
        p.angle1 = a.angle.data(); p.angle2 = b.angle.data();
        p.n_nodes1 = (int32_t)a.node_id.size(); p.n_nodes2 = (int32_t)b.node_id.size();
        p.node_id1 = a.node_id.data(); p.node_id2 = b.node_id.data();
        p.node_begin1 = a.node_begin.data(); p.node_begin2 = b.node_begin.data();
        p.node_feat1 = a.node_feat.data(); p.node_feat2 = b.node_feat.data();
        out.emplace_back((size_t)a.n, (size_t)b.n);
        pp[i] = &p;
    }
    for (size_t i = 0; i < n; i++) pr[i] = &out[i].R;            // out does not grow any more
    return BackendCall(who, vba_search_by_bow, (int32_t)n, pp.data(), pr.data());
}

// vpMapPointMatches of :211, :287, :343: the map point of pKF whose match the function leaves at each keypoint of F
void FrameMatches(const BowSide& kf, const BowOut& o, std::vector<MapPoint*>& v) {
    v.assign(o.match21.size(), static_cast<MapPoint*>(nullptr));
    for (size_t k = 0; k < v.size(); k++)
        if (o.match21[k] >= 0) v[k] = (*kf.points)[(size_t)o.match21[k]];
}

// vpMatches12 of :623, :695, :741: the map point of pKF2 matched to each keypoint of pKF1
void KeyFrameMatches(const BowSide& kf2, const BowOut& o, std::vector<MapPoint*>& v) {
    v.assign(o.match12.size(), static_cast<MapPoint*>(nullptr));
    for (size_t i = 0; i < v.size(); i++)
        if (o.match12[i] >= 0) v[i] = (*kf2.points)[(size_t)o.match12[i]];
}
}  // namespace

int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches) {
    const BowSide s1(pKF), s2(F);
    std::vector<BowOut> out;
    if (!RunBow("ORBmatcher::SearchByBoW", VBA_SEARCH_BOW_KF_FRAME, {&s1}, {&s2}, mfNNratio, mbCheckOrientation, out)) return -1;
    FrameMatches(s1, out[0], vpMapPointMatches);
    return out[0].R.n_matches;
}

int ORBmatcher::SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12) {
    const BowSide s1(pKF1), s2(pKF2);
    std::vector<BowOut> out;
    if (!RunBow("ORBmatcher::SearchByBoW", VBA_SEARCH_BOW_KF_KF, {&s1}, {&s2}, mfNNratio, mbCheckOrientation, out)) return -1;
    KeyFrameMatches(s2, out[0], vpMatches12);
    return out[0].R.n_matches;
}

int ORBmatcher::SearchByBoW(const std::vector<KeyFrame*>& vpKFs, Frame& F, std::vector<std::vector<MapPoint*>>& vvpMapPointMatches,
                            std::vector<int>& vnMatches) {
    const BowSide frame(F);
    std::vector<BowSide> kfs;
    kfs.reserve(vpKFs.size());
    for (KeyFrame* kf : vpKFs) kfs.emplace_back(kf);
    std::vector<const BowSide*> s1, s2(vpKFs.size(), &frame);
    for (const BowSide& k : kfs) s1.push_back(&k);
    std::vector<BowOut> out;
    vvpMapPointMatches.assign(vpKFs.size(), std::vector<MapPoint*>());
    vnMatches.assign(vpKFs.size(), 0);
    if (!RunBow("ORBmatcher::SearchByBoW (keyframes against a frame)", VBA_SEARCH_BOW_KF_FRAME, s1, s2, mfNNratio, mbCheckOrientation, out)) return -1;
    for (size_t i = 0; i < out.size(); i++) {
        FrameMatches(kfs[i], out[i], vvpMapPointMatches[i]);
        vnMatches[i] = out[i].R.n_matches;
    }
    return 0;
}

int ORBmatcher::SearchByBoW(KeyFrame* pKF1, const std::vector<KeyFrame*>& vpKFs2, std::vector<std::vector<MapPoint*>>& vvpMatches12,
                            std::vector<int>& vnMatches) {
    const BowSide first(pKF1);
    std::vector<BowSide> kfs;
    kfs.reserve(vpKFs2.size());
    for (KeyFrame* kf : vpKFs2) kfs.emplace_back(kf);
    std::vector<const BowSide*> s1(vpKFs2.size(), &first), s2;
    for (const BowSide& k : kfs) s2.push_back(&k);
    std::vector<BowOut> out;
    vvpMatches12.assign(vpKFs2.size(), std::vector<MapPoint*>());
    vnMatches.assign(vpKFs2.size(), 0);
    if (!RunBow("ORBmatcher::SearchByBoW (a keyframe against keyframes)", VBA_SEARCH_BOW_KF_KF, s1, s2, mfNNratio, mbCheckOrientation, out)) return -1;
    for (size_t i = 0; i < out.size(); i++) {
        KeyFrameMatches(kfs[i], out[i], vvpMatches12[i]);
        vnMatches[i] = out[i].R.n_matches;
    }
    return 0;
}

}  // namespace ORB_SLAM2
