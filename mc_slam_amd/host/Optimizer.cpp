// Optimizer.cpp -- see Optimizer.h.  Line references: src/Optimizer.cpp of mc275/MC_SLAM.
#include "Optimizer.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <chrono>

namespace ORB_SLAM2 {

long unsigned int KeyFrame::nNextId = 0;
long unsigned int MapPoint::nNextId = 0;
int Optimizer::Device = 0;

namespace {

thread_local void* t_handle = nullptr;
thread_local PackedWindow t_last;

void* handle() {
    if (!t_handle && vba_create(Optimizer::Device, &t_handle) != 0) t_handle = nullptr;
    return t_handle;
}

}  // namespace
void* Optimizer::BackendHandle() { return handle(); }
namespace {

Quaterniond MatrixToQuat(const double* m) {  // Eigen::Quaterniond(Matrix3d), then normalised
    Quaterniond q;
    double t = m[0] + m[4] + m[8];
    if (t > 0) {
        t = std::sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (m[7] - m[5]) * t; q[1] = (m[2] - m[6]) * t; q[2] = (m[3] - m[1]) * t;
    } else {
        int i = 0;
        if (m[4] > m[0]) i = 1;
        if (m[8] > m[4 * i]) i = 2;
        const int j = (i + 1) % 3, k = (j + 1) % 3;
        t = std::sqrt(m[4 * i] - m[4 * j] - m[4 * k] + 1.0);
        q[i] = 0.5 * t;
        t = 0.5 / t;
        q[3] = (m[3 * k + j] - m[3 * j + k]) * t;
        q[j] = (m[3 * j + i] + m[3 * i + j]) * t;
        q[k] = (m[3 * k + i] + m[3 * i + k]) * t;
    }
    const double n = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    for (auto& v : q) v /= n;
    return q;
}

// information of EdgeNavStatePRV: swap V/phi rows+cols of the P,V,phi covariance, invert (:273-280)
bool PRVInformation(const std::array<double, 81>& cov, double* info) {
    static const int perm[9] = {0, 1, 2, 6, 7, 8, 3, 4, 5};
    double M[9][18];
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) { M[i][j] = cov[9 * perm[i] + perm[j]]; M[i][9 + j] = (i == j) ? 1.0 : 0.0; }
    for (int c = 0; c < 9; c++) {
        int p = c;
        for (int r = c + 1; r < 9; r++)
            if (std::fabs(M[r][c]) > std::fabs(M[p][c])) p = r;
        if (M[p][c] == 0.0) return false;
        if (p != c)
            for (int j = 0; j < 18; j++) std::swap(M[c][j], M[p][j]);
        const double inv = 1.0 / M[c][c];
        for (int j = 0; j < 18; j++) M[c][j] *= inv;
        for (int r = 0; r < 9; r++) {
            if (r == c || M[r][c] == 0.0) continue;
            const double f = M[r][c];
            for (int j = 0; j < 18; j++) M[r][j] -= f * M[c][j];
        }
    }
    for (int i = 0; i < 9; i++)
        for (int j = 0; j < 9; j++) info[9 * i + j] = M[i][9 + j];
    return true;
}

// KeyFrame* -> row of the window.  Every observation of the window looks its keyframe up (30 000 times for a 50-keyframe window):
// an open-addressing table over a few hundred slots instead of a std::map walk (the reference pays optimizer.vertex(id), a
// tr1::unordered_map look-up, per edge endpoint: Thirdparty/g2o/g2o/core/hyper_graph.cpp:60-66).
struct KfTable {
    std::vector<std::pair<const KeyFrame*, int>> slot;
    size_t mask = 0;
    void reset(size_t n) {
        size_t cap = 64;
        while (cap < 4 * n) cap *= 2;
        slot.assign(cap, {nullptr, -1});
        mask = cap - 1;
    }
    static size_t hash(const KeyFrame* k) { return (size_t)((reinterpret_cast<uintptr_t>(k) >> 4) * 0x9E3779B97F4A7C15ull >> 20); }
    void put(const KeyFrame* k, int row) {
        if (2 * (size_t)(row + 1) > slot.size()) {   // (the fixed keyframes are discovered on the way: grow before the table fills)
            std::vector<std::pair<const KeyFrame*, int>> old;
            old.swap(slot);
            reset(old.size());
            for (auto& e : old) if (e.first) put(e.first, e.second);
        }
        size_t i = hash(k) & mask;
        while (slot[i].first && slot[i].first != k) i = (i + 1) & mask;
        slot[i] = {k, row};
    }
    int get(const KeyFrame* k) const {
        size_t i = hash(k) & mask;
        while (slot[i].first) {
            if (slot[i].first == k) return slot[i].second;
            i = (i + 1) & mask;
        }
        return -1;
    }
};

void FinishProblem(PackedWindow& W) {
    vba_problem& P = W.P;
    P.n_kf = (int32_t)W.vKF.size();
    P.n_pt = (int32_t)W.vMP.size();
    P.n_obs = (int32_t)W.obsKF.size();
    P.n_imu = (int32_t)W.imuI.size();
    P.kf_pose = W.pose.data(); P.kf_vel = W.vel.data(); P.kf_bias = W.bias.data(); P.pt = W.pt.data();
    P.pt_ref_kf = W.ref.data(); P.pt_obs_begin = W.begin.data(); P.obs_kf = W.obsKF.data();
    P.obs_uv = W.uv.data(); P.obs_w = W.w.data();
    P.imu_kf_i = W.imuI.data(); P.imu_kf_j = W.imuJ.data(); P.imu_meas = W.meas.data(); P.imu_info_prv = W.info.data();
    P.inv_bg_rw2 = 1.0 / IMUData::getGyrBiasRW2();   // :246
    P.inv_ba_rw2 = 1.0 / IMUData::getAccBiasRW2();   // :249
    P.huber_vis = (double)(float)std::sqrt(5.991);             // const float thHuberMono, :327
    P.huber_prv = (double)(float)std::sqrt(100 * 21.666);      // :241
    P.huber_bias = (double)(float)std::sqrt(100 * 16.812);     // :242
    P.its_stage1 = 5; P.its_stage2 = 10;                       // :459, :493
    P.chi2_th = 5.991;
    W.outlier.assign(P.n_obs ? P.n_obs : 1, 0);
    W.chi2.assign(P.n_obs ? P.n_obs : 1, 0.0);
    std::memset(&W.R, 0, sizeof W.R);
    W.R.obs_outlier = W.outlier.data();
    W.R.obs_chi2 = W.chi2.data();
}

// g2o's forceStopFlag is a bool* written by the Tracking thread (&LocalMapping::mbAbortBA, src/LocalMapping.cpp:1769-1772): the
// backend reads the caller's flag at its own width (vba_solve_b), so the pointer goes straight through -- the device sees a raised
// flag at its next poll because the host forwards it whenever it enqueues an iteration and while it waits.  (Until round 4 the ABI
// only took an int*: a thread per call mirrored the bool into one.)
static_assert(sizeof(bool) == 1, "vba_solve_b reads the stop flag as one byte");
inline const volatile unsigned char* StopPtr(bool* pbStopFlag) { return reinterpret_cast<const volatile unsigned char*>(pbStopFlag); }

// wall-clock split of the last facade call of this thread (Optimizer::LastTiming): extraction, solve (vba_solve_b: H2D + structure +
// two-stage solve + D2H), erase + write-back under the map lock
thread_local FacadeTiming t_timing;
inline double NowMs() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

const PackedWindow& Optimizer::LastWindow() { return t_last; }
const FacadeTiming& Optimizer::LastTiming() { return t_timing; }
PackedWindow& Optimizer::LastWindowMutable() { return t_last; }

// ------------------------------------------------------------------------------------------------
bool Optimizer::PackLocalBAPRVIDP(KeyFrame* pCurKF, const std::list<KeyFrame*>& lLocalKeyFrames, const Vector3d& gw,
                                  PackedWindow& W) {
    return PackLocalVI(pCurKF, lLocalKeyFrames, gw, true, W);
}
bool Optimizer::PackLocalBundleAdjustmentNavStatePRV(KeyFrame* pCurKF, const std::list<KeyFrame*>& lLocalKeyFrames, const Vector3d& gw,
                                                     PackedWindow& W) {
    return PackLocalVI(pCurKF, lLocalKeyFrames, gw, false, W);
}

// the two visual-inertial local windows share everything but the landmark model: inverse depth in the reference keyframe
// (LocalBAPRVIDP, :32-625) or world XYZ (LocalBundleAdjustmentNavStatePRV, :937-1388)
bool Optimizer::PackLocalVI(KeyFrame* pCurKF, const std::list<KeyFrame*>& lLocalKeyFrames, const Vector3d& gw, bool idp,
                            PackedWindow& W) {
    static const bool ptm = getenv("VBA_FACADE_TIMING") != nullptr;
    double tp[8]; int ti = 0; tp[ti++] = NowMs();
    W = PackedWindow();
    std::memset(&W.P, 0, sizeof W.P);
    if (pCurKF != lLocalKeyFrames.back()) std::cerr << "pCurKF != lLocalKeyFrames.back. check" << std::endl;  // :37-38
    for (KeyFrame* pKFi : lLocalKeyFrames) pKFi->mnBALocalForKF = pCurKF->mnId;                                 // :49-56
    std::list<MapPoint*> lLocalMapPoints;                                                                          // :59-79
    for (KeyFrame* pKFi : lLocalKeyFrames)
        for (MapPoint* pMP : pKFi->GetMapPointMatches())
            if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pCurKF->mnId) {
                lLocalMapPoints.push_back(pMP);
                pMP->mnBALocalForKF = pCurKF->mnId;
            }
    tp[ti++] = NowMs();
    // One copy of every map point's observation list serves both passes that read it -- the search for the fixed cameras (:82-127) and
    // the edges (:337-451); GetObservations() returns the std::map by value (include/MapPoint.h), the reference copies it twice.
    std::vector<MapPoint*> vLocalMP(lLocalMapPoints.begin(), lLocalMapPoints.end());
    std::vector<mapMapPointObs> vObs(vLocalMP.size());
    size_t nObsTotal = 0;
    for (size_t i = 0; i < vLocalMP.size(); i++) { vObs[i] = vLocalMP[i]->GetObservations(); nObsTotal += vObs[i].size(); }
    tp[ti++] = NowMs();
    std::list<KeyFrame*> lFixedCameras;                                                                           // :82-127
    KeyFrame* pKFPrevLocal = lLocalKeyFrames.front()->GetPrevKeyFrame();
    if (pKFPrevLocal) {
        pKFPrevLocal->mnBAFixedForKF = pCurKF->mnId;
        if (!pKFPrevLocal->isBad()) lFixedCameras.push_back(pKFPrevLocal);
    } else
        std::cerr << "pKFPrevLocal is NULL?" << std::endl;
    for (size_t i = 0; i < vLocalMP.size(); i++)
        for (auto& mit : vObs[i]) {
            KeyFrame* pKFi = mit.first;
            if (pKFi->mnBALocalForKF != pCurKF->mnId && pKFi->mnBAFixedForKF != pCurKF->mnId) {
                pKFi->mnBAFixedForKF = pCurKF->mnId;
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    tp[ti++] = NowMs();
    // vertices -> rows: free keyframes (window order = ascending mnId) first, fixed after            (:159-232)
    KfTable kfIdx;
    kfIdx.reset(lLocalKeyFrames.size() + lFixedCameras.size());
    for (KeyFrame* k : lLocalKeyFrames) { kfIdx.put(k, (int)W.vKF.size()); W.vKF.push_back(k); }
    W.P.n_kf_free = (int32_t)W.vKF.size();
    for (KeyFrame* k : lFixedCameras) { kfIdx.put(k, (int)W.vKF.size()); W.vKF.push_back(k); }
    for (KeyFrame* k : W.vKF) {
        const NavState& ns = k->GetNavState();
        const Vector3d P = ns.Get_P(), V = ns.Get_V(), bg = ns.Get_BiasGyr(), ba = ns.Get_BiasAcc(), dbg = ns.Get_dBias_Gyr(), dba = ns.Get_dBias_Acc();
        const Quaterniond q = ns.Get_R();
        W.pose.insert(W.pose.end(), {P[0], P[1], P[2], q[0], q[1], q[2], q[3]});
        W.vel.insert(W.vel.end(), {V[0], V[1], V[2]});
        W.bias.insert(W.bias.end(), {bg[0], bg[1], bg[2], ba[0], ba[1], ba[2], dbg[0], dbg[1], dbg[2], dba[0], dba[1], dba[2]});
    }
    // IMU factors: one EdgeNavStatePRV + one EdgeNavStateBias per local keyframe                     (:251-312)
    for (KeyFrame* pKF1 : lLocalKeyFrames) {
        KeyFrame* pKF0 = pKF1->GetPrevKeyFrame();
        if (!pKF0 || kfIdx.get(pKF0) < 0) { std::cerr << "pKF0 missing" << std::endl; continue; }
        const IMUPreintegrator& M = pKF1->GetIMUPreInt();
        W.imuI.push_back(kfIdx.get(pKF0));
        W.imuJ.push_back(kfIdx.get(pKF1));
        W.meas.push_back(M.getDeltaTime());
        for (double v : M.getDeltaP()) W.meas.push_back(v);
        for (double v : M.getDeltaV()) W.meas.push_back(v);
        for (const Matrix3d* A : {&M.getDeltaR(), &M.getJPBiasg(), &M.getJPBiasa(), &M.getJVBiasg(), &M.getJVBiasa(), &M.getJRBiasg()})
            for (double v : *A) W.meas.push_back(v);
        double info[81];
        if (!PRVInformation(M.getCovPVPhi(), info)) { std::cerr << "singular preintegration covariance" << std::endl; return false; }
        W.info.insert(W.info.end(), info, info + 81);
    }
    tp[ti++] = NowMs();
    W.obsKF.reserve(nObsTotal); W.uv.reserve(2 * nObsTotal); W.w.reserve(nObsTotal);
    W.vEdgeKF.reserve(nObsTotal); W.vEdgeMP.reserve(nObsTotal);
    W.pt.reserve(3 * vLocalMP.size()); W.ref.reserve(vLocalMP.size()); W.refXY.reserve(2 * vLocalMP.size());
    W.vMP.reserve(vLocalMP.size()); W.begin.reserve(vLocalMP.size() + 1);
    W.begin.push_back(0);
    if (!idp) {   // VertexSBAPointXYZ + one EdgeNavStatePRPointXYZ per observation (:1151-1193)
        for (size_t ip = 0; ip < vLocalMP.size(); ip++) {
            MapPoint* pMP = vLocalMP[ip];
            double Pw[3];
            pMP->GetWorldPos(Pw);
            for (auto& mit : vObs[ip]) {
                KeyFrame* pKFi = mit.first;
                if (pKFi->isBad()) continue;
                if (pKFi->mvuRight[mit.second] >= 0) { std::cerr << "Stereo not supported yet" << std::endl; continue; }
                const KeyPoint& kpUn = pKFi->mvKeysUn[mit.second];
                W.obsKF.push_back(kfIdx.get(pKFi));
                W.uv.push_back(kpUn.pt.x); W.uv.push_back(kpUn.pt.y);
                W.w.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
                W.vEdgeKF.push_back(pKFi);
                W.vEdgeMP.push_back(pMP);
                W.P.K[0] = pKFi->fx; W.P.K[1] = pKFi->fy; W.P.K[2] = pKFi->cx; W.P.K[3] = pKFi->cy;
            }
            W.pt.insert(W.pt.end(), {Pw[0], Pw[1], Pw[2]});
            W.ref.push_back(0);
            W.vMP.push_back(pMP);
            W.begin.push_back((int32_t)W.obsKF.size());
        }
    }
    // landmarks and EdgePRIDP edges                                                                   (:337-451)
    for (size_t ip = 0; ip < vLocalMP.size(); ip++) {
        if (!idp) break;
        MapPoint* pMP = vLocalMP[ip];
        double Pw[3];
        pMP->GetWorldPos(Pw);
        KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
        if (!pRefKF || pRefKF->isBad()) continue;                                                                // :349-353
        double Rcw[9], tcw[3];
        pRefKF->GetRotation(Rcw);
        pRefKF->GetTranslation(tcw);
        const double dc = Rcw[6] * Pw[0] + Rcw[7] * Pw[1] + Rcw[8] * Pw[2] + tcw[2];                             // :355-358
        if (dc < 0.01) continue;                                                                                 // :360-365
        const mapMapPointObs& observations = vObs[ip];
        const auto itRef = observations.find(pRefKF);
        if (itRef == observations.end()) { std::cerr << "!observations.count(pRefKF)" << std::endl; continue; }
        const KeyPoint& kpRefUn = pRefKF->mvKeysUn[itRef->second];
        const double normx = (kpRefUn.pt.x - pRefKF->cx) / pRefKF->fx, normy = (kpRefUn.pt.y - pRefKF->cy) / pRefKF->fy;  // :382-385
        const size_t nBefore = W.obsKF.size();
        for (auto& mit : observations) {
            KeyFrame* pKFi = mit.first;
            if (pKFi == pRefKF || pKFi->isBad()) continue;                                                       // :395-400
            if (pKFi->mvuRight[mit.second] >= 0) { std::cerr << "Stereo not supported yet" << std::endl; continue; }
            const KeyPoint& kpUn = pKFi->mvKeysUn[mit.second];
            W.obsKF.push_back(kfIdx.get(pKFi));
            W.uv.push_back(kpUn.pt.x); W.uv.push_back(kpUn.pt.y);
            W.w.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);                                                  // float -> double, :428-429
            W.vEdgeKF.push_back(pKFi);
            W.vEdgeMP.push_back(pMP);
        }
        if (W.obsKF.size() == nBefore) continue;  // no edge -> the vertex is never added (:407-412, 588-589)
        W.pt.insert(W.pt.end(), {1.0 / dc, normx, normy});
        W.ref.push_back(kfIdx.get(pRefKF));
        W.refXY.push_back(normx); W.refXY.push_back(normy);
        W.vMP.push_back(pMP);
        W.begin.push_back((int32_t)W.obsKF.size());
        W.P.K[0] = pRefKF->fx; W.P.K[1] = pRefKF->fy; W.P.K[2] = pRefKF->cx; W.P.K[3] = pRefKF->cy;              // :422
    }
    tp[ti++] = NowMs();
    W.P.variant = idp ? VBA_VARIANT_PRV_IDP : VBA_VARIANT_PRV_XYZ;
    W.P.algo = idp ? VBA_ALGO_GN : VBA_ALGO_LM;                                                                   // :136 / :1028
    Matrix3d Rcb; Vector3d tcb;
    ConfigParam::GetEigT_cb(Rcb, tcb);                                                                            // :41-43
    const Quaterniond qcb = MatrixToQuat(Rcb.data());
    for (int i = 0; i < 3; i++) { W.P.T_cb[i] = tcb[i]; W.P.g_w[i] = gw[i]; }
    for (int i = 0; i < 4; i++) W.P.T_cb[3 + i] = qcb[i];
    W.P.depth_min = idp ? 0.01 : 0.0; W.P.rho_min = 2e-6;                                                         // g2otypes.h:122-127 / :300-303, :484
    if (W.vMP.empty() || W.obsKF.empty()) return false;   // an empty graph: the reference's optimize() changes nothing
    FinishProblem(W);
    tp[ti++] = NowMs();
    if (ptm) { fprintf(stderr, "[facade] pack:"); for (int i = 1; i < ti; i++) fprintf(stderr, " %.3f", tp[i] - tp[i - 1]); fprintf(stderr, " ms (marks+list | obs copies | fixed cams | rows+imu | edges | finish)\n"); }
    return true;
}

void Optimizer::LocalBAPRVIDP(KeyFrame* pCurKF, const std::list<KeyFrame*>& lLocalKeyFrames, bool* pbStopFlag, Map* pMap,
                              const Vector3d& gw, LocalMapping* pLM) {
    PackedWindow& W = t_last;
    t_timing = FacadeTiming();
    const double t0 = NowMs();
    if (!PackLocalBAPRVIDP(pCurKF, lLocalKeyFrames, gw, W)) return;
    t_timing.extract_ms = NowMs() - t0;
    if (pbStopFlag && *pbStopFlag) return;                                                                        // :453-455
    void* h = handle();
    if (!h) { std::cerr << "LocalBAPRVIDP: no HIP device, local BA skipped (the backend has no CPU path)" << std::endl; return; }
    const double t1 = NowMs();
    if (vba_solve_b(h, &W.P, &W.R, StopPtr(pbStopFlag)) != 0) {
        std::cerr << "LocalBAPRVIDP: " << vba_last_error(h) << std::endl;
        return;
    }
    const double t2 = NowMs();
    t_timing.solve_ms = t2 - t1;
    struct WriteBackTimer { double t; ~WriteBackTimer() { t_timing.writeback_ms = NowMs() - t; t_timing.total_ms = t_timing.extract_ms + t_timing.solve_ms + t_timing.writeback_ms; } } wbt{t2};
    if (W.R.status == VBA_ABORTED_BEFORE) return;
    if (W.R.status == VBA_ABORTED_AFTER_STAGE1)
        std::cerr << "Hint: local mapping optimize only 5 iter. Need more computation resource." << std::endl;  // :469-470
    std::vector<std::pair<KeyFrame*, MapPoint*>> vToErase;                                                        // :496-517
    for (size_t i = 0; i < W.vEdgeKF.size(); i++) {
        if (W.vEdgeMP[i]->isBad()) continue;
        if (W.outlier[i]) vToErase.push_back(std::make_pair(W.vEdgeKF[i], W.vEdgeMP[i]));
    }
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                                                     // :520
    for (auto& e : vToErase) { e.first->EraseMapPointMatch(e.second); e.second->EraseObservation(e.first); }      // :523-532
    for (int i = 0; i < W.P.n_kf_free; i++) {                                                                     // :536-570
        KeyFrame* pKFi = W.vKF[i];
        pKFi->SetNavStatePos({{W.pose[7 * i], W.pose[7 * i + 1], W.pose[7 * i + 2]}});
        pKFi->SetNavStateRot({{W.pose[7 * i + 3], W.pose[7 * i + 4], W.pose[7 * i + 5], W.pose[7 * i + 6]}});
        pKFi->SetNavStateVel({{W.vel[3 * i], W.vel[3 * i + 1], W.vel[3 * i + 2]}});
        pKFi->SetNavStateDeltaBg({{W.bias[12 * i + 6], W.bias[12 * i + 7], W.bias[12 * i + 8]}});
        pKFi->SetNavStateDeltaBa({{W.bias[12 * i + 9], W.bias[12 * i + 10], W.bias[12 * i + 11]}});
        pKFi->UpdatePoseFromNS();
    }
    for (size_t p = 0; p < W.vMP.size(); p++) {                                                                   // :573-606
        MapPoint* pMP = W.vMP[p];
        KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
        if (pRefKF->isBad()) continue;
        const double rho = W.pt[3 * p];
        const float Pref[3] = {(float)(W.refXY[2 * p] / rho), (float)(W.refXY[2 * p + 1] / rho), (float)(1.0 / rho)};
        double Rcw[9], twr[3];
        pRefKF->GetRotation(Rcw);       // float32 values of the (updated) reference pose
        pRefKF->GetCameraCenter(twr);
        float Pw[3];
        for (int i = 0; i < 3; i++)     // Rwr * Pref + twr in float32 like cv::Mat
            Pw[i] = (float)Rcw[i] * Pref[0] + (float)Rcw[3 + i] * Pref[1] + (float)Rcw[6 + i] * Pref[2] + (float)twr[i];
        pMP->SetWorldPos(Pw);
        pMP->UpdateNormalAndDepth();
    }
    if (pLM) pLM->SetMapUpdateFlagInTracking(true);                                                               // :620-623
}

void Optimizer::LocalBundleAdjustmentNavStatePRV(KeyFrame* pCurKF, const std::list<KeyFrame*>& lLocalKeyFrames, bool* pbStopFlag,
                                                 Map* pMap, const Vector3d& gw, LocalMapping* pLM) {             // :937-1388
    PackedWindow& W = t_last;
    if (!PackLocalBundleAdjustmentNavStatePRV(pCurKF, lLocalKeyFrames, gw, W)) return;
    if (pbStopFlag && *pbStopFlag) return;                                                                        // :1196-1198
    void* h = handle();
    if (!h) { std::cerr << "LocalBundleAdjustmentNavStatePRV: no HIP device, local BA skipped (the backend has no CPU path)" << std::endl; return; }
    {
        if (vba_solve_b(h, &W.P, &W.R, StopPtr(pbStopFlag)) != 0) {
            std::cerr << "LocalBundleAdjustmentNavStatePRV: " << vba_last_error(h) << std::endl;
            return;
        }
    }
    if (W.R.status == VBA_ABORTED_BEFORE) return;
    std::vector<std::pair<KeyFrame*, MapPoint*>> vToErase;                                                        // :1222-1238
    for (size_t i = 0; i < W.vEdgeKF.size(); i++) {
        if (W.vEdgeMP[i]->isBad()) continue;
        if (W.outlier[i]) vToErase.push_back(std::make_pair(W.vEdgeKF[i], W.vEdgeMP[i]));
    }
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (auto& e : vToErase) { e.first->EraseMapPointMatch(e.second); e.second->EraseObservation(e.first); }
    for (int i = 0; i < W.P.n_kf_free; i++) {                                                                     // :1250-1270
        KeyFrame* pKFi = W.vKF[i];
        pKFi->SetNavStatePos({{W.pose[7 * i], W.pose[7 * i + 1], W.pose[7 * i + 2]}});
        pKFi->SetNavStateRot({{W.pose[7 * i + 3], W.pose[7 * i + 4], W.pose[7 * i + 5], W.pose[7 * i + 6]}});
        pKFi->SetNavStateVel({{W.vel[3 * i], W.vel[3 * i + 1], W.vel[3 * i + 2]}});
        pKFi->SetNavStateDeltaBg({{W.bias[12 * i + 6], W.bias[12 * i + 7], W.bias[12 * i + 8]}});
        pKFi->SetNavStateDeltaBa({{W.bias[12 * i + 9], W.bias[12 * i + 10], W.bias[12 * i + 11]}});
        pKFi->UpdatePoseFromNS();
    }
    for (size_t p = 0; p < W.vMP.size(); p++) {                                                                   // :1275-1283
        const float Pw[3] = {(float)W.pt[3 * p], (float)W.pt[3 * p + 1], (float)W.pt[3 * p + 2]};
        W.vMP[p]->SetWorldPos(Pw);
        W.vMP[p]->UpdateNormalAndDepth();
    }
    if (pLM) pLM->SetMapUpdateFlagInTracking(true);
}

// ------------------------------------------------------------------------------------------------
bool Optimizer::PackLocalBundleAdjustment(KeyFrame* pKF, PackedWindow& W) { return PackLocalBundleAdjustment(pKF, nullptr, W); }

bool Optimizer::PackLocalBundleAdjustment(KeyFrame* pKF, const std::list<KeyFrame*>* pList, PackedWindow& W) {
    W = PackedWindow();
    std::memset(&W.P, 0, sizeof W.P);
    std::list<KeyFrame*> lLocalKeyFrames;
    if (pList) {                                                                                                  // :2981-2986
        lLocalKeyFrames = *pList;
        for (KeyFrame* pKFi : lLocalKeyFrames) pKFi->mnBALocalForKF = pKF->mnId;
    } else {                                                                                                      // :3861-3875
        lLocalKeyFrames.push_back(pKF);
        pKF->mnBALocalForKF = pKF->mnId;
        for (KeyFrame* pKFi : pKF->GetVectorCovisibleKeyFrames()) {
            pKFi->mnBALocalForKF = pKF->mnId;
            if (!pKFi->isBad()) lLocalKeyFrames.push_back(pKFi);
        }
    }
    std::list<MapPoint*> lLocalMapPoints;                                                                         // :3878-3895
    for (KeyFrame* pKFi : lLocalKeyFrames)
        for (MapPoint* pMP : pKFi->GetMapPointMatches())
            if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
                lLocalMapPoints.push_back(pMP);
                pMP->mnBALocalForKF = pKF->mnId;
            }
    std::list<KeyFrame*> lFixedCameras;                                                                           // :3898-3915
    if (pList) {   // the keyframe before the window is fixed first (:3005-3023)
        KeyFrame* pKFPrevLocal = lLocalKeyFrames.front()->GetPrevKeyFrame();
        if (pKFPrevLocal) {
            pKFPrevLocal->mnBAFixedForKF = pKF->mnId;
            if (!pKFPrevLocal->isBad()) lFixedCameras.push_back(pKFPrevLocal);
        }
    }
    for (MapPoint* pMP : lLocalMapPoints)
        for (auto& mit : pMP->GetObservations()) {
            KeyFrame* pKFi = mit.first;
            if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
                pKFi->mnBAFixedForKF = pKF->mnId;
                if (!pKFi->isBad()) lFixedCameras.push_back(pKFi);
            }
        }
    std::map<KeyFrame*, int> kfIdx;
    std::vector<KeyFrame*> fixedLocal;
    for (KeyFrame* k : lLocalKeyFrames) {
        if (k->mnId == 0) { fixedLocal.push_back(k); continue; }   // vSE3->setFixed(pKFi->mnId == 0), :3944
        kfIdx[k] = (int)W.vKF.size();
        W.vKF.push_back(k);
    }
    W.P.n_kf_free = (int32_t)W.vKF.size();
    for (KeyFrame* k : fixedLocal) { kfIdx[k] = (int)W.vKF.size(); W.vKF.push_back(k); }
    for (KeyFrame* k : lFixedCameras) { kfIdx[k] = (int)W.vKF.size(); W.vKF.push_back(k); }
    if (W.P.n_kf_free == 0) return false;
    for (KeyFrame* k : W.vKF) {  // Converter::toSE3Quat(pKFi->GetPose()): float32 -> double, Quaterniond(R), normalizeRotation
        double R[9], t[3];
        k->GetRotation(R);
        k->GetTranslation(t);
        Quaterniond q = MatrixToQuat(R);
        if (q[3] < 0) for (auto& v : q) v = -v;
        W.pose.insert(W.pose.end(), {t[0], t[1], t[2], q[0], q[1], q[2], q[3]});
        W.vel.insert(W.vel.end(), {0, 0, 0});
        W.bias.insert(W.bias.end(), 12, 0.0);
    }
    W.begin.push_back(0);
    for (MapPoint* pMP : lLocalMapPoints) {                                                                       // :3992-4085
        double Pw[3];
        pMP->GetWorldPos(Pw);
        for (auto& mit : pMP->GetObservations()) {
            KeyFrame* pKFi = mit.first;
            if (pKFi->isBad() || pKFi->mvuRight[mit.second] >= 0) continue;  // stereo branch never taken for mono
            const KeyPoint& kpUn = pKFi->mvKeysUn[mit.second];
            W.obsKF.push_back(kfIdx[pKFi]);
            W.uv.push_back(kpUn.pt.x); W.uv.push_back(kpUn.pt.y);
            W.w.push_back(pKFi->mvInvLevelSigma2[kpUn.octave]);
            W.vEdgeKF.push_back(pKFi);
            W.vEdgeMP.push_back(pMP);
            W.P.K[0] = pKFi->fx; W.P.K[1] = pKFi->fy; W.P.K[2] = pKFi->cx; W.P.K[3] = pKFi->cy;
        }
        W.pt.insert(W.pt.end(), {Pw[0], Pw[1], Pw[2]});
        W.ref.push_back(0);
        W.vMP.push_back(pMP);
        W.begin.push_back((int32_t)W.obsKF.size());
    }
    if (W.vMP.empty() || W.obsKF.empty()) return false;   // nothing to optimise: g2o would run on an empty graph and change nothing
    W.P.variant = VBA_VARIANT_SE3_XYZ;
    W.P.algo = VBA_ALGO_LM;                                                                                       // :3928
    W.P.T_cb[6] = 1.0;
    W.P.depth_min = 0.0;
    if (W.vMP.empty() || W.obsKF.empty()) return false;   // an empty graph: the reference's optimize() changes nothing
    FinishProblem(W);
    return true;
}

void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, const std::list<KeyFrame*>& lLocalKeyFrames, bool* pbStopFlag, Map* pMap,
                                      LocalMapping* pLM) {
    if (pKF != lLocalKeyFrames.back()) std::cerr << "pKF != lLocalKeyFrames.back. check" << std::endl;                // :2978-2979
    LocalBundleAdjustmentImpl(pKF, &lLocalKeyFrames, pbStopFlag, pMap, pLM);
}

void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, LocalMapping* pLM) {
    LocalBundleAdjustmentImpl(pKF, nullptr, pbStopFlag, pMap, pLM);
}

void Optimizer::LocalBundleAdjustmentImpl(KeyFrame* pKF, const std::list<KeyFrame*>* pList, bool* pbStopFlag, Map* pMap, LocalMapping* pLM) {
    PackedWindow& W = t_last;
    if (!PackLocalBundleAdjustment(pKF, pList, W)) return;
    if (pbStopFlag && *pbStopFlag) return;                                                                        // :4088-4090
    void* h = handle();
    if (!h) { std::cerr << "LocalBundleAdjustment: no HIP device, local BA skipped (the backend has no CPU path)" << std::endl; return; }
    {
        if (vba_solve_b(h, &W.P, &W.R, StopPtr(pbStopFlag)) != 0) {
            std::cerr << "LocalBundleAdjustment: " << vba_last_error(h) << std::endl;
            return;
        }
    }
    if (W.R.status == VBA_ABORTED_BEFORE) return;
    std::vector<std::pair<KeyFrame*, MapPoint*>> vToErase;                                                        // :4146-4163
    for (size_t i = 0; i < W.vEdgeKF.size(); i++) {
        if (W.vEdgeMP[i]->isBad()) continue;
        if (W.outlier[i]) vToErase.push_back(std::make_pair(W.vEdgeKF[i], W.vEdgeMP[i]));
    }
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                                                     // :4181
    for (auto& e : vToErase) { e.first->EraseMapPointMatch(e.second); e.second->EraseObservation(e.first); }
    for (int i = 0; i < W.P.n_kf_free; i++) {                                                                     // :4198-4204, Converter::toCvMat(SE3Quat)
        const Matrix3d R = QuatToMatrix({{W.pose[7 * i + 3], W.pose[7 * i + 4], W.pose[7 * i + 5], W.pose[7 * i + 6]}});
        Mat4f T{};
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
            T[4 * r + 3] = (float)W.pose[7 * i + r];
        }
        T[15] = 1.0f;
        W.vKF[i]->SetPose(T);
    }
    for (size_t p = 0; p < W.vMP.size(); p++) {                                                                   // :4207-4214
        const float Pw[3] = {(float)W.pt[3 * p], (float)W.pt[3 * p + 1], (float)W.pt[3 * p + 2]};
        W.vMP[p]->SetWorldPos(Pw);
        W.vMP[p]->UpdateNormalAndDepth();
    }
    if (pLM) pLM->SetMapUpdateFlagInTracking(true);
}


// ------------------------------------------------------------------------------------------------
// Global bundle adjustment.  Same factors as the local windows at map scale, one optimize(nIterations) with
// Levenberg-Marquardt, no outlier pass (VBA_PROTO_SINGLE).
// ------------------------------------------------------------------------------------------------
namespace {
// landmarks + monocular reprojection edges of a whole map (src/Optimizer.cpp:776-833 / :3417-3513)
void PackMapPoints(const std::vector<MapPoint*>& vpMP, std::map<KeyFrame*, int>& kfIdx, PackedWindow& W) {
    W.begin.push_back(0);
    for (MapPoint* pMP : vpMP) {
        if (pMP->isBad()) continue;
        const size_t e0 = W.obsKF.size();
        for (auto& mit : pMP->GetObservations()) {
            KeyFrame* pKF = mit.first;
            if (pKF->isBad() || !kfIdx.count(pKF)) continue;       // "|| pKF->mnId > maxKFid"
            if (pKF->mvuRight[mit.second] >= 0) continue;          // stereo: not supported here
            const KeyPoint& kpUn = pKF->mvKeysUn[mit.second];
            W.obsKF.push_back(kfIdx[pKF]);
            W.uv.push_back(kpUn.pt.x); W.uv.push_back(kpUn.pt.y);
            W.w.push_back(pKF->mvInvLevelSigma2[kpUn.octave]);
            W.vEdgeKF.push_back(pKF);
            W.vEdgeMP.push_back(pMP);
            W.P.K[0] = pKF->fx; W.P.K[1] = pKF->fy; W.P.K[2] = pKF->cx; W.P.K[3] = pKF->cy;
        }
        if (W.obsKF.size() == e0) continue;                        // nEdges == 0: vbNotIncludedMP, vertex removed
        double Pw[3];
        pMP->GetWorldPos(Pw);
        W.pt.insert(W.pt.end(), {Pw[0], Pw[1], Pw[2]});
        W.ref.push_back(0);
        W.vMP.push_back(pMP);
        W.begin.push_back((int32_t)W.obsKF.size());
    }
}

bool RunGlobal(PackedWindow& W, bool* pbStopFlag, const char* who) {
    void* h = handle();
    if (!h) { std::cerr << who << ": no HIP device, global BA skipped (the backend has no CPU path)" << std::endl; return false; }
    if (vba_solve_b(h, &W.P, &W.R, StopPtr(pbStopFlag)) != 0) {
        std::cerr << who << ": " << vba_last_error(h) << std::endl;
        return false;
    }
    return true;  // a raised stop flag leaves the estimates untouched; the reference still writes them back
}

void WriteBackMapPoints(PackedWindow& W, const unsigned long nLoopKF) {   // :915-931 / :3583-3604
    for (size_t p = 0; p < W.vMP.size(); p++) {
        const float Pw[3] = {(float)W.pt[3 * p], (float)W.pt[3 * p + 1], (float)W.pt[3 * p + 2]};
        if (nLoopKF == 0) {
            W.vMP[p]->SetWorldPos(Pw);
            W.vMP[p]->UpdateNormalAndDepth();
        } else {
            for (int i = 0; i < 3; i++) W.vMP[p]->mPosGBA[i] = Pw[i];
            W.vMP[p]->mnBAGlobalForKF = nLoopKF;
        }
    }
}
}  // namespace

bool Optimizer::PackGlobalBundleAdjustmentNavStatePRV(Map* pMap, const Vector3d& gw, int nIterations, bool bRobust, PackedWindow& W) {
    W = PackedWindow();
    std::memset(&W.P, 0, sizeof W.P);
    std::map<KeyFrame*, int> kfIdx;
    for (KeyFrame* pKF : pMap->GetAllKeyFrames()) {                                                               // :661-690
        if (pKF->isBad()) continue;
        kfIdx[pKF] = (int)W.vKF.size();
        W.vKF.push_back(pKF);
        const NavState& ns = pKF->GetNavState();
        const Vector3d P = ns.Get_P(), V = ns.Get_V(), bg = ns.Get_BiasGyr(), ba = ns.Get_BiasAcc(), dbg = ns.Get_dBias_Gyr(), dba = ns.Get_dBias_Acc();
        const Quaterniond q = ns.Get_R();
        W.pose.insert(W.pose.end(), {P[0], P[1], P[2], q[0], q[1], q[2], q[3]});
        W.vel.insert(W.vel.end(), {V[0], V[1], V[2]});
        W.bias.insert(W.bias.end(), {bg[0], bg[1], bg[2], ba[0], ba[1], ba[2], dbg[0], dbg[1], dbg[2], dba[0], dba[1], dba[2]});
        W.kfFix.push_back(pKF->mnId == 0 ? 0x5 : 0x0);   // PR and Bias of keyframe 0 fixed, its V free (:667-685)
    }
    if (W.vKF.empty()) return false;
    W.P.n_kf_free = (int32_t)W.vKF.size();
    for (KeyFrame* pKF1 : W.vKF) {                                                                                // :700-770
        KeyFrame* pKF0 = pKF1->GetPrevKeyFrame();
        if (!pKF0 || !kfIdx.count(pKF0)) continue;
        const IMUPreintegrator& pre = pKF1->GetIMUPreInt();
        double info[81];
        if (!PRVInformation(pre.getCovPVPhi(), info)) continue;
        W.imuI.push_back(kfIdx[pKF0]);
        W.imuJ.push_back(kfIdx[pKF1]);
        W.meas.push_back(pre.getDeltaTime());
        for (double v : pre.getDeltaP()) W.meas.push_back(v);
        for (double v : pre.getDeltaV()) W.meas.push_back(v);
        for (double v : pre.getDeltaR()) W.meas.push_back(v);
        for (double v : pre.getJPBiasg()) W.meas.push_back(v);
        for (double v : pre.getJPBiasa()) W.meas.push_back(v);
        for (double v : pre.getJVBiasg()) W.meas.push_back(v);
        for (double v : pre.getJVBiasa()) W.meas.push_back(v);
        for (double v : pre.getJRBiasg()) W.meas.push_back(v);
        W.info.insert(W.info.end(), info, info + 81);
    }
    PackMapPoints(pMap->GetAllMapPoints(), kfIdx, W);
    W.P.variant = VBA_VARIANT_PRV_XYZ;
    W.P.algo = VBA_ALGO_LM;                                                                                       // :652
    Matrix3d Rcb; Vector3d tcb;
    ConfigParam::GetEigT_cb(Rcb, tcb);
    const Quaterniond qcb = MatrixToQuat(Rcb.data());
    for (int i = 0; i < 3; i++) { W.P.T_cb[i] = tcb[i]; W.P.g_w[i] = gw[i]; }
    for (int i = 0; i < 4; i++) W.P.T_cb[3 + i] = qcb[i];
    W.P.depth_min = 0.0;
    if (W.vMP.empty() || W.obsKF.empty()) return false;   // an empty graph: the reference's optimize() changes nothing
    FinishProblem(W);
    W.P.protocol = VBA_PROTO_SINGLE;
    W.P.robust = bRobust ? 1 : 0;
    W.P.its_stage1 = nIterations; W.P.its_stage2 = 0;                                                             // :836
    W.P.huber_vis = (double)(float)std::sqrt(5.99);                                                               // thHuber2D, :773
    W.P.kf_fix = W.kfFix.data();
    return true;
}

void Optimizer::GlobalBundleAdjustmentNavStatePRV(Map* pMap, const Vector3d& gw, int nIterations, bool* pbStopFlag,
                                                  const unsigned long nLoopKF, const bool bRobust) {
    PackedWindow& W = t_last;
    if (!PackGlobalBundleAdjustmentNavStatePRV(pMap, gw, nIterations, bRobust, W)) return;
    if (!RunGlobal(W, pbStopFlag, "GlobalBundleAdjustmentNavStatePRV")) return;
    for (size_t i = 0; i < W.vKF.size(); i++) {                                                                   // :842-893
        KeyFrame* pKF = W.vKF[i];
        NavState ns = pKF->GetNavState();
        ns.Set_Pos({{W.pose[7 * i], W.pose[7 * i + 1], W.pose[7 * i + 2]}});
        ns.Set_Rot({{W.pose[7 * i + 3], W.pose[7 * i + 4], W.pose[7 * i + 5], W.pose[7 * i + 6]}});
        ns.Set_Vel({{W.vel[3 * i], W.vel[3 * i + 1], W.vel[3 * i + 2]}});
        ns.Set_DeltaBiasGyr({{W.bias[12 * i + 6], W.bias[12 * i + 7], W.bias[12 * i + 8]}});
        ns.Set_DeltaBiasAcc({{W.bias[12 * i + 9], W.bias[12 * i + 10], W.bias[12 * i + 11]}});
        if (nLoopKF == 0) {
            pKF->SetNavState(ns);
            pKF->UpdatePoseFromNS();
        } else {   // the map kept growing meanwhile: results parked for LoopClosing to propagate (:873-891)
            KeyFrame tmp;
            tmp.SetNavState(ns);
            tmp.UpdatePoseFromNS();          // same float32 chain: Twb * Tbc, inverted
            pKF->mNavStateGBA = ns;
            pKF->mTcwGBA = tmp.GetPose();
            pKF->mnBAGlobalForKF = nLoopKF;
        }
    }
    WriteBackMapPoints(W, nLoopKF);
}

bool Optimizer::PackBundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations,
                                     bool bRobust, PackedWindow& W) {
    W = PackedWindow();
    std::memset(&W.P, 0, sizeof W.P);
    std::map<KeyFrame*, int> kfIdx;
    std::vector<KeyFrame*> fixed;
    for (KeyFrame* pKF : vpKFs) {                                                                                 // :3400-3412
        if (pKF->isBad()) continue;
        if (pKF->mnId == 0) { fixed.push_back(pKF); continue; }   // vSE3->setFixed(pKF->mnId == 0)
        kfIdx[pKF] = (int)W.vKF.size();
        W.vKF.push_back(pKF);
    }
    W.P.n_kf_free = (int32_t)W.vKF.size();
    for (KeyFrame* k : fixed) { kfIdx[k] = (int)W.vKF.size(); W.vKF.push_back(k); }
    if (W.P.n_kf_free == 0) return false;
    for (KeyFrame* k : W.vKF) {  // Converter::toSE3Quat(pKF->GetPose())
        double R[9], t[3];
        k->GetRotation(R);
        k->GetTranslation(t);
        Quaterniond q = MatrixToQuat(R);
        if (q[3] < 0) for (auto& v : q) v = -v;
        W.pose.insert(W.pose.end(), {t[0], t[1], t[2], q[0], q[1], q[2], q[3]});
        W.vel.insert(W.vel.end(), {0, 0, 0});
        W.bias.insert(W.bias.end(), 12, 0.0);
    }
    PackMapPoints(vpMP, kfIdx, W);
    W.P.variant = VBA_VARIANT_SE3_XYZ;
    W.P.algo = VBA_ALGO_LM;                                                                                       // :3393
    W.P.T_cb[6] = 1.0;
    W.P.depth_min = 0.0;
    if (W.vMP.empty() || W.obsKF.empty()) return false;   // an empty graph: the reference's optimize() changes nothing
    FinishProblem(W);
    W.P.protocol = VBA_PROTO_SINGLE;
    W.P.robust = bRobust ? 1 : 0;
    W.P.its_stage1 = nIterations; W.P.its_stage2 = 0;                                                             // :3518
    W.P.huber_vis = (double)(float)std::sqrt(5.99);                                                               // thHuber2D, :3414
    return true;
}

void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>& vpKFs, const std::vector<MapPoint*>& vpMP, int nIterations,
                                 bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
    PackedWindow& W = t_last;
    if (!PackBundleAdjustment(vpKFs, vpMP, nIterations, bRobust, W)) return;
    if (!RunGlobal(W, pbStopFlag, "BundleAdjustment")) return;
    for (int i = 0; i < W.P.n_kf_free; i++) {                                                                     // :3521-3541, Converter::toCvMat(SE3Quat)
        const Matrix3d R = QuatToMatrix({{W.pose[7 * i + 3], W.pose[7 * i + 4], W.pose[7 * i + 5], W.pose[7 * i + 6]}});
        Mat4f T{};
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
            T[4 * r + 3] = (float)W.pose[7 * i + r];
        }
        T[15] = 1.0f;
        if (nLoopKF == 0) W.vKF[i]->SetPose(T);
        else { W.vKF[i]->mTcwGBA = T; W.vKF[i]->mnBAGlobalForKF = nLoopKF; }
    }
    // the fixed keyframe is written back too in the reference (its estimate did not move): a float32 round trip
    WriteBackMapPoints(W, nLoopKF);
}

// ------------------------------------------------------------------------------------------------
// Per-frame pose optimisation (src/Optimizer.cpp:3610-3835, 2046-2317, 1671-2044): set-up and write-back here, the four
// optimize(10) rounds + reclassification + marginals behind vba_pose_optimize.
// ------------------------------------------------------------------------------------------------
namespace {
void NavToArray(const NavState& ns, double* v) {
    const Vector3d P = ns.Get_P(), V = ns.Get_V(), bg = ns.Get_BiasGyr(), ba = ns.Get_BiasAcc(), dbg = ns.Get_dBias_Gyr(), dba = ns.Get_dBias_Acc();
    const Quaterniond q = ns.Get_R();
    const double a[22] = {P[0], P[1], P[2], q[0], q[1], q[2], q[3], V[0], V[1], V[2], bg[0], bg[1], bg[2], ba[0], ba[1], ba[2],
                          dbg[0], dbg[1], dbg[2], dba[0], dba[1], dba[2]};
    std::memcpy(v, a, sizeof a);
}
struct FrameObs {
    std::vector<double> pw, uv, w;
    std::vector<size_t> idx;
    std::vector<uint8_t> outl;
};
// monocular correspondences of a frame (:2137-2172); resets mvbOutlier like the reference does
void GatherFrame(Frame* f, FrameObs& o) {
    for (int i = 0; i < f->N; i++) {
        MapPoint* pMP = f->mvpMapPoints[i];
        if (!pMP || f->mvuRight[i] >= 0) continue;   // stereo: "stereo shouldn't in poseoptimization"
        f->mvbOutlier[i] = false;
        double P[3];
        pMP->GetWorldPos(P);
        const KeyPoint& kp = f->mvKeysUn[i];
        o.pw.insert(o.pw.end(), {P[0], P[1], P[2]});
        o.uv.push_back(kp.pt.x); o.uv.push_back(kp.pt.y);
        o.w.push_back(f->mvInvLevelSigma2[kp.octave]);
        o.idx.push_back((size_t)i);
    }
    o.outl.assign(o.idx.size() + 1, 0);
}
void FillCommon(vba_frame_problem& F, Frame* f, const FrameObs& o) {
    F.n_obs = (int32_t)o.idx.size();
    F.obs_pw = o.pw.data(); F.obs_uv = o.uv.data(); F.obs_w = o.w.data();
    F.K[0] = f->fx; F.K[1] = f->fy; F.K[2] = f->cx; F.K[3] = f->cy;
}
void FillImu(vba_frame_problem& F, const IMUPreintegrator& pre, const Vector3d& gw) {
    Matrix3d Rcb; Vector3d tcb;
    ConfigParam::GetEigT_cb(Rcb, tcb);
    const Quaterniond qcb = MatrixToQuat(Rcb.data());
    for (int i = 0; i < 3; i++) { F.T_cb[i] = tcb[i]; F.g_w[i] = gw[i]; }
    for (int i = 0; i < 4; i++) F.T_cb[3 + i] = qcb[i];
    double* m = F.imu_meas;
    m[0] = pre.getDeltaTime();
    std::memcpy(m + 1, pre.getDeltaP().data(), 24); std::memcpy(m + 4, pre.getDeltaV().data(), 24);
    std::memcpy(m + 7, pre.getDeltaR().data(), 72);
    std::memcpy(m + 16, pre.getJPBiasg().data(), 72); std::memcpy(m + 25, pre.getJPBiasa().data(), 72);
    std::memcpy(m + 34, pre.getJVBiasg().data(), 72); std::memcpy(m + 43, pre.getJVBiasa().data(), 72);
    std::memcpy(m + 52, pre.getJRBiasg().data(), 72);
    std::memcpy(F.imu_cov_pvphi, pre.getCovPVPhi().data(), sizeof F.imu_cov_pvphi);
    F.inv_bg_rw2 = 1.0 / IMUData::getGyrBiasRW2();
    F.inv_ba_rw2 = 1.0 / IMUData::getAccBiasRW2();
}
int RunFrame(vba_frame_problem& F, vba_frame_result& R, const char* who) {
    void* h = handle();
    if (!h) { std::cerr << who << ": no HIP device, pose optimisation skipped (the backend has no CPU path)" << std::endl; return -1; }
    vba_frame_problem* pf = &F;
    vba_frame_result* pr = &R;
    if (vba_pose_optimize(h, 1, &pf, &pr) != 0) { std::cerr << who << ": " << vba_last_error(h) << std::endl; return -1; }
    return 0;
}
NavState ArrayToNav(const NavState& base, const double* v) {   // ns_recov: PVR from the PVR vertex, delta biases from the bias vertex
    NavState ns = base;
    ns.Set_Pos({{v[0], v[1], v[2]}});
    ns.Set_Rot({{v[3], v[4], v[5], v[6]}});
    ns.Set_Vel({{v[7], v[8], v[9]}});
    ns.Set_DeltaBiasGyr({{v[16], v[17], v[18]}});
    ns.Set_DeltaBiasAcc({{v[19], v[20], v[21]}});
    return ns;
}
}  // namespace

int Optimizer::PoseOptimization(Frame* pFrame) {                                                                   // :3610-3835
    FrameObs o;
    GatherFrame(pFrame, o);
    if (o.idx.size() < 3) return 0;                                                                               // :3726-3727
    vba_frame_problem F;
    std::memset(&F, 0, sizeof F);
    vba_frame_result R;
    std::memset(&R, 0, sizeof R);
    F.last_is_frame = VBA_FRAME_VISION;
    FillCommon(F, pFrame, o);
    {   // Converter::toSE3Quat(pFrame->mTcw)
        double Rm[9];
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rm[3 * i + j] = pFrame->mTcw[4 * i + j];
        Quaterniond q = MatrixToQuat(Rm);
        if (q[3] < 0) for (auto& v : q) v = -v;
        for (int i = 0; i < 3; i++) F.nav[i] = pFrame->mTcw[4 * i + 3];
        for (int i = 0; i < 4; i++) F.nav[3 + i] = q[i];
    }
    F.T_cb[6] = 1.0;
    R.outlier = o.outl.data();
    if (RunFrame(F, R, "PoseOptimization") != 0) return 0;
    for (size_t k = 0; k < o.idx.size(); k++) pFrame->mvbOutlier[o.idx[k]] = o.outl[k] != 0;
    const Matrix3d Rr = QuatToMatrix({{F.nav[3], F.nav[4], F.nav[5], F.nav[6]}});                                  // Converter::toCvMat(SE3quat_recov)
    Mat4f T{};
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) T[4 * r + c] = (float)Rr[3 * r + c];
        T[4 * r + 3] = (float)F.nav[r];
    }
    T[15] = 1.0f;
    pFrame->SetPose(T);
    return R.n_inliers;
}

int Optimizer::PoseOptimization(Frame* pFrame, KeyFrame* pLastKF, const IMUPreintegrator& imupreint, const Vector3d& gw,
                                const bool& bComputeMarg) {                                                       // :2046-2317
    FrameObs o;
    GatherFrame(pFrame, o);
    if (o.idx.size() < 3) return 0;
    vba_frame_problem F;
    std::memset(&F, 0, sizeof F);
    vba_frame_result R;
    std::memset(&R, 0, sizeof R);
    F.last_is_frame = VBA_FRAME_KF;
    F.compute_marg = bComputeMarg ? 1 : 0;
    FillCommon(F, pFrame, o);
    FillImu(F, imupreint, gw);
    NavToArray(pFrame->GetNavState(), F.nav);
    NavToArray(pLastKF->GetNavState(), F.nav_last);
    R.outlier = o.outl.data();
    if (RunFrame(F, R, "PoseOptimization") != 0) return 0;
    for (size_t k = 0; k < o.idx.size(); k++) pFrame->mvbOutlier[o.idx[k]] = o.outl[k] != 0;
    const NavState ns = ArrayToNav(pFrame->GetNavState(), F.nav);
    pFrame->SetNavState(ns);
    pFrame->UpdatePoseFromNS();
    if (bComputeMarg) {
        std::memcpy(pFrame->mMargCovInv.data(), R.marg_cov_inv, sizeof R.marg_cov_inv);
        pFrame->mNavStatePrior = ns;
    }
    return R.n_inliers;
}

int Optimizer::PoseOptimization(Frame* pFrame, Frame* pLastFrame, const IMUPreintegrator& imupreint, const Vector3d& gw,
                                const bool& bComputeMarg) {                                                       // :1671-2044
    FrameObs o, ol;
    GatherFrame(pFrame, o);
    GatherFrame(pLastFrame, ol);
    if (o.idx.size() < 3) return 0;
    vba_frame_problem F;
    std::memset(&F, 0, sizeof F);
    vba_frame_result R;
    std::memset(&R, 0, sizeof R);
    F.last_is_frame = VBA_FRAME_FRAME;
    F.compute_marg = bComputeMarg ? 1 : 0;
    FillCommon(F, pFrame, o);
    F.n_obs_last = (int32_t)ol.idx.size();
    F.last_pw = ol.pw.data(); F.last_uv = ol.uv.data(); F.last_w = ol.w.data();
    FillImu(F, imupreint, gw);
    NavToArray(pFrame->GetNavState(), F.nav);
    NavToArray(pLastFrame->GetNavState(), F.nav_last);
    NavToArray(pLastFrame->mNavStatePrior, F.prior_nav);
    std::memcpy(F.prior_info, pLastFrame->mMargCovInv.data(), sizeof F.prior_info);
    R.outlier = o.outl.data();
    R.outlier_last = ol.outl.data();
    if (RunFrame(F, R, "PoseOptimization") != 0) return 0;
    for (size_t k = 0; k < o.idx.size(); k++) pFrame->mvbOutlier[o.idx[k]] = o.outl[k] != 0;
    for (size_t k = 0; k < ol.idx.size(); k++) pLastFrame->mvbOutlier[ol.idx[k]] = ol.outl[k] != 0;
    const NavState ns = ArrayToNav(pFrame->GetNavState(), F.nav);
    pFrame->SetNavState(ns);
    pFrame->UpdatePoseFromNS();
    if (bComputeMarg) {
        std::memcpy(pFrame->mMargCovInv.data(), R.marg_cov_inv, sizeof R.marg_cov_inv);
        pFrame->mNavStatePrior = ns;
    }
    return R.n_inliers;
}

int Optimizer::OptimizeSim3(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches1, g2o::Sim3& g2oS12, const float th2,
                            const bool bFixScale) {                                                               // :4579-4785
    const Mat4f& T1 = pKF1->GetPose();
    const Mat4f& T2 = pKF2->GetPose();
    // cv::Mat P3Dc = Rcw * P3Dw + tcw (:4659-4669): CV_32F arithmetic, widened by Converter::toVector3d
    auto toCamera = [](const Mat4f& T, const float* Pw, double* Pc) {
        for (int i = 0; i < 3; i++) {
            float a = T[4 * i] * Pw[0];
            a += T[4 * i + 1] * Pw[1];
            a += T[4 * i + 2] * Pw[2];
            a += T[4 * i + 3];
            Pc[i] = (double)a;
        }
    };
    const int N = (int)vpMatches1.size();
    const std::vector<MapPoint*> vpMapPoints1 = pKF1->GetMapPointMatches();
    std::vector<double> p1c, p2c, uv1, uv2, w1, w2;
    std::vector<size_t> vnIndexEdge;
    vnIndexEdge.reserve(N);
    for (int i = 0; i < N; i++) {
        if (!vpMatches1[i]) continue;                                                                             // :4640
        MapPoint* pMP1 = vpMapPoints1[i];
        MapPoint* pMP2 = vpMatches1[i];
        const int i2 = pMP2->GetIndexInKeyFrame(pKF2);
        if (!pMP1 || !pMP2) continue;                                                                             // :4653, :4677
        if (pMP1->isBad() || pMP2->isBad() || i2 < 0) continue;                                                   // :4655, :4674
        double P[3];
        toCamera(T1, pMP1->mWorldPos, P);
        p1c.insert(p1c.end(), P, P + 3);
        toCamera(T2, pMP2->mWorldPos, P);
        p2c.insert(p2c.end(), P, P + 3);
        const KeyPoint& kpUn1 = pKF1->mvKeysUn[i];                                                                // :4683-4693
        uv1.push_back(kpUn1.pt.x); uv1.push_back(kpUn1.pt.y);
        w1.push_back(pKF1->mvInvLevelSigma2[kpUn1.octave]);
        const KeyPoint& kpUn2 = pKF2->mvKeysUn[i2];                                                               // :4701-4710
        uv2.push_back(kpUn2.pt.x); uv2.push_back(kpUn2.pt.y);
        w2.push_back(pKF2->mvInvLevelSigma2[kpUn2.octave]);
        vnIndexEdge.push_back(i);
    }
    const int nCorrespondences = (int)vnIndexEdge.size();
    vba_sim3_problem P;
    std::memset(&P, 0, sizeof P);
    vba_sim3_result R;
    std::memset(&R, 0, sizeof R);
    std::vector<uint8_t> outl((size_t)nCorrespondences + 1, 0);
    P.n_pairs = nCorrespondences;
    P.fix_scale = bFixScale ? 1 : 0;
    for (int k = 0; k < 3; k++) P.S12[k] = g2oS12.translation()[k];
    for (int k = 0; k < 4; k++) P.S12[3 + k] = g2oS12.rotation()[k];
    P.S12[7] = g2oS12.scale();
    P.p1c = p1c.data(); P.p2c = p2c.data(); P.uv1 = uv1.data(); P.uv2 = uv2.data(); P.w1 = w1.data(); P.w2 = w2.data();
    P.K1[0] = pKF1->fx; P.K1[1] = pKF1->fy; P.K1[2] = pKF1->cx; P.K1[3] = pKF1->cy;                               // :4612-4619
    P.K2[0] = pKF2->fx; P.K2[1] = pKF2->fy; P.K2[2] = pKF2->cx; P.K2[3] = pKF2->cy;
    P.th2 = th2;
    P.huber = (double)std::sqrt(th2);                                                                             // const float deltaHuber = sqrt(th2), :4634
    P.its_stage1 = 5; P.its_stage2_bad = 10; P.its_stage2_clean = 5; P.min_inliers = 10;                          // :4724, :4749-4755
    R.outlier = outl.data();
    void* h = handle();
    if (!h) { std::cerr << "OptimizeSim3: no HIP device, Sim3 refinement skipped (the backend has no CPU path)" << std::endl; return 0; }
    vba_sim3_problem* pp = &P;
    vba_sim3_result* pr = &R;
    if (vba_sim3_optimize(h, 1, &pp, &pr) != 0) { std::cerr << "OptimizeSim3: " << vba_last_error(h) << std::endl; return 0; }
    for (int k = 0; k < nCorrespondences; k++)
        if (outl[k]) vpMatches1[vnIndexEdge[k]] = static_cast<MapPoint*>(NULL);                                   // :4738-4739, :4773-4774
    if (nCorrespondences - R.n_bad_stage1 < 10) return 0;                                                         // :4755-4756: g2oS12 untouched
    g2oS12 = g2o::Sim3({{P.S12[3], P.S12[4], P.S12[5], P.S12[6]}}, {{P.S12[0], P.S12[1], P.S12[2]}}, P.S12[7]);   // :4781-4782
    return R.n_inliers;
}

namespace {
thread_local PackedPoseGraph t_last_pg;
void put_sim3(const g2o::Sim3& S, std::vector<double>& v) {
    for (int k = 0; k < 3; k++) v.push_back(S.translation()[k]);
    for (int k = 0; k < 4; k++) v.push_back(S.rotation()[k]);
    v.push_back(S.scale());
}
}  // namespace
PackedPoseGraph& Optimizer::LastPoseGraph() { return t_last_pg; }

bool Optimizer::PackEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                   const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                   const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections, bool bFixScale, PackedPoseGraph& G) {
    G = PackedPoseGraph();
    const std::vector<KeyFrame*> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MapPoint*> vpMPs = pMap->GetAllMapPoints();
    const unsigned int nMaxKFid = pMap->GetMaxKFid();
    std::vector<g2o::Sim3> vScw(nMaxKFid + 1);
    std::vector<int> vVertex(nMaxKFid + 1, -1);       // optimizer.vertex(id): -1 where the reference has none (bad keyframes)
    const int minFeat = 100;
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {                                                      // :4284-4325
        KeyFrame* pKF = vpKFs[i];
        if (pKF->isBad()) continue;
        const int nIDi = pKF->mnId;
        LoopClosing::KeyFrameAndPose::const_iterator it = CorrectedSim3.find(pKF);
        if (it != CorrectedSim3.end()) {
            vScw[nIDi] = it->second;
        } else {
            double R[9], t[3];
            pKF->GetRotation(R);
            pKF->GetTranslation(t);
            Matrix3d Rcw;
            for (int k = 0; k < 9; k++) Rcw[k] = R[k];
            vScw[nIDi] = g2o::Sim3(MatrixToQuat(Rcw), {{t[0], t[1], t[2]}}, 1.0);                                 // Sim3(Matrix3d, ...): Quaterniond(R)
        }
        vVertex[nIDi] = (int)G.vKF.size();
        G.vKF.push_back(pKF);
        put_sim3(vScw[nIDi], G.S);
        G.fixed.push_back(pKF == pLoopKF ? 1 : 0);                                                                // :4314-4315
    }
    // an edge of the reference whose vertex does not exist is refused by addEdge; one between two fixed vertices cannot occur
    // (there is one fixed vertex)
    auto addEdge = [&](long unsigned int nIDi, long unsigned int nIDj, const g2o::Sim3& Sji) {
        if (nIDi > nMaxKFid || nIDj > nMaxKFid || vVertex[nIDi] < 0 || vVertex[nIDj] < 0 || nIDi == nIDj) return;
        G.ei.push_back(vVertex[nIDi]);
        G.ej.push_back(vVertex[nIDj]);
        put_sim3(Sji, G.edgeS);
    };
    std::set<std::pair<long unsigned int, long unsigned int>> sInsertedEdges;
    for (std::map<KeyFrame*, std::set<KeyFrame*>>::const_iterator mit = LoopConnections.begin(), mend = LoopConnections.end(); mit != mend; mit++) {
        KeyFrame* pKF = mit->first;                                                                               // :4331-4365
        const long unsigned int nIDi = pKF->mnId;
        const std::set<KeyFrame*>& spConnections = mit->second;
        const g2o::Sim3 Siw = vScw[nIDi];
        const g2o::Sim3 Swi = Siw.inverse();
        for (std::set<KeyFrame*>::const_iterator sit = spConnections.begin(), send = spConnections.end(); sit != send; sit++) {
            const long unsigned int nIDj = (*sit)->mnId;
            if ((nIDi != pCurKF->mnId || nIDj != pLoopKF->mnId) && pKF->GetWeight(*sit) < minFeat) continue;
            const g2o::Sim3 Sjw = vScw[nIDj];
            addEdge(nIDi, nIDj, Sjw * Swi);
            sInsertedEdges.insert(std::make_pair(std::min(nIDi, nIDj), std::max(nIDi, nIDj)));
        }
    }
    for (size_t i = 0, iend = vpKFs.size(); i < iend; i++) {                                                      // :4368-4478
        KeyFrame* pKF = vpKFs[i];
        const int nIDi = pKF->mnId;
        g2o::Sim3 Swi;
        LoopClosing::KeyFrameAndPose::const_iterator iti = NonCorrectedSim3.find(pKF);
        if (iti != NonCorrectedSim3.end()) Swi = (iti->second).inverse();
        else Swi = vScw[nIDi].inverse();
        KeyFrame* pParentKF = pKF->GetParent();
        if (pParentKF) {                                                                                          // spanning tree
            const int nIDj = pParentKF->mnId;
            g2o::Sim3 Sjw;
            LoopClosing::KeyFrameAndPose::const_iterator itj = NonCorrectedSim3.find(pParentKF);
            if (itj != NonCorrectedSim3.end()) Sjw = itj->second;
            else Sjw = vScw[nIDj];
            addEdge(nIDi, nIDj, Sjw * Swi);
        }
        const std::set<KeyFrame*> sLoopEdges = pKF->GetLoopEdges();                                               // loop edges
        for (std::set<KeyFrame*>::const_iterator sit = sLoopEdges.begin(), send = sLoopEdges.end(); sit != send; sit++) {
            KeyFrame* pLKF = *sit;
            if (pLKF->mnId < pKF->mnId) {
                g2o::Sim3 Slw;
                LoopClosing::KeyFrameAndPose::const_iterator itl = NonCorrectedSim3.find(pLKF);
                if (itl != NonCorrectedSim3.end()) Slw = itl->second;
                else Slw = vScw[pLKF->mnId];
                addEdge(nIDi, pLKF->mnId, Slw * Swi);
            }
        }
        const std::vector<KeyFrame*> vpConnectedKFs = pKF->GetCovisiblesByWeight(minFeat);                        // covisibility
        for (std::vector<KeyFrame*>::const_iterator vit = vpConnectedKFs.begin(); vit != vpConnectedKFs.end(); vit++) {
            KeyFrame* pKFn = *vit;
            if (pKFn && pKFn != pParentKF && !pKF->hasChild(pKFn) && !sLoopEdges.count(pKFn)) {
                if (!pKFn->isBad() && pKFn->mnId < pKF->mnId) {
                    if (sInsertedEdges.count(std::make_pair(std::min(pKF->mnId, pKFn->mnId), std::max(pKF->mnId, pKFn->mnId)))) continue;
                    g2o::Sim3 Snw;
                    LoopClosing::KeyFrameAndPose::const_iterator itn = NonCorrectedSim3.find(pKFn);
                    if (itn != NonCorrectedSim3.end()) Snw = itn->second;
                    else Snw = vScw[pKFn->mnId];
                    addEdge(nIDi, pKFn->mnId, Snw * Swi);
                }
            }
        }
    }
    for (size_t i = 0, iend = vpMPs.size(); i < iend; i++) {                                                      // :4511-4530
        MapPoint* pMP = vpMPs[i];
        if (pMP->isBad()) continue;
        long unsigned int nIDr;
        if (pMP->mnCorrectedByKF == pCurKF->mnId) nIDr = pMP->mnCorrectedReference;
        else nIDr = pMP->GetReferenceKeyFrame()->mnId;
        if (nIDr > nMaxKFid || vVertex[nIDr] < 0) continue;   // no vertex: vScw and vCorrectedSwc are both the identity there, the point stays
        double P[3];
        pMP->GetWorldPos(P);
        G.pt.insert(G.pt.end(), P, P + 3);
        G.ptRef.push_back(vVertex[nIDr]);
        G.vMP.push_back(pMP);
    }
    std::memset(&G.P, 0, sizeof G.P);
    std::memset(&G.R, 0, sizeof G.R);
    G.P.n_vertices = (int32_t)G.vKF.size(); G.P.n_edges = (int32_t)G.ei.size();
    G.P.fix_scale = bFixScale ? 1 : 0;
    G.P.its = 20;                                                                                                 // :4482
    G.P.lambda_init = 1e-16;                                                                                      // :4265
    G.P.S = G.S.data(); G.P.fixed = G.fixed.data(); G.P.edge_i = G.ei.data(); G.P.edge_j = G.ej.data(); G.P.edge_S = G.edgeS.data();
    G.P.n_pt = (int32_t)G.vMP.size(); G.P.pt = G.pt.data(); G.P.pt_ref = G.ptRef.data();
    return !G.vKF.empty();
}

void Optimizer::OptimizeEssentialGraph(Map* pMap, KeyFrame* pLoopKF, KeyFrame* pCurKF, const LoopClosing::KeyFrameAndPose& NonCorrectedSim3,
                                       const LoopClosing::KeyFrameAndPose& CorrectedSim3,
                                       const std::map<KeyFrame*, std::set<KeyFrame*>>& LoopConnections, const bool& bFixScale,
                                       LoopClosing* pLC) {                                                        // :4243-4552
    PackedPoseGraph& G = t_last_pg;
    if (!PackEssentialGraph(pMap, pLoopKF, pCurKF, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale, G)) return;
    void* h = handle();
    if (!h) { std::cerr << "OptimizeEssentialGraph: no HIP device, pose graph skipped (the backend has no CPU path)" << std::endl; return; }
    vba_posegraph_problem* pp = &G.P;
    vba_posegraph_result* pr = &G.R;
    if (vba_posegraph_optimize(h, 1, &pp, &pr) != 0) { std::cerr << "OptimizeEssentialGraph: " << vba_last_error(h) << std::endl; return; }
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);
    for (size_t i = 0; i < G.vKF.size(); i++) {                                                                   // :4488-4508: Sim3 [sR t; 0 1] -> SE3 [R t/s; 0 1]
        const double* Si = &G.S[8 * i];
        const Matrix3d eigR = QuatToMatrix({{Si[3], Si[4], Si[5], Si[6]}});
        const double s = Si[7];
        Mat4f Tiw{};
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) Tiw[4 * r + c] = (float)eigR[3 * r + c];
            Tiw[4 * r + 3] = (float)(Si[r] * (1.0 / s));
        }
        Tiw[15] = 1.0f;
        G.vKF[i]->SetPose(Tiw);
        G.vKF[i]->UpdateNavStatePVRFromTcw(Tiw, ConfigParam::Rbc(), ConfigParam::Pbc());
    }
    for (size_t i = 0; i < G.vMP.size(); i++) {                                                                   // :4537-4545
        const float P[3] = {(float)G.pt[3 * i], (float)G.pt[3 * i + 1], (float)G.pt[3 * i + 2]};
        G.vMP[i]->SetWorldPos(P);
        G.vMP[i]->UpdateNormalAndDepth();
    }
    if (pLC) pLC->SetMapUpdateFlagInTracking(true);                                                               // :4548-4551
}

void Optimizer::GlobalBundleAdjustment(Map* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust) {
    BundleAdjustment(pMap->GetAllKeyFrames(), pMap->GetAllMapPoints(), nIterations, pbStopFlag, nLoopKF, bRobust);   // :3346-3354
}

}  // namespace ORB_SLAM2
