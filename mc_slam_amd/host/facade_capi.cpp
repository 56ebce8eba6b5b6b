// facade_capi.cpp -- C entry points that let the test-suite build a KeyFrame / MapPoint map from flat arrays,
// call the C++ facade (Optimizer.h) and read the map back.  Test harness of the facade, not part of the
// product ABI (that is include/vislam_ba.h).
#include <algorithm>
#include <cstring>
#include <map>
#include <memory>

#include "Optimizer.h"
#include "Sim3Solver.h"
#include "Initializer.h"
#include "ORBmatcher.h"
#include "Tracking.h"
#include "LoopClosing.h"

using namespace ORB_SLAM2;

struct FcMap {
    Map map;
    LocalMapping lm;
    LoopClosing lc;
    std::map<long, std::unique_ptr<KeyFrame>> kfs;
    std::map<long, std::unique_ptr<MapPoint>> mps;
    std::map<long, std::unique_ptr<Frame>> frames;
};

extern "C" {

void* fc_create() { return new FcMap(); }
void fc_destroy(void* m) { delete reinterpret_cast<FcMap*>(m); }
void fc_set_device(int dev) { Optimizer::Device = dev; }
void fc_set_tbc(const double* R9, const double* p3) {
    Matrix3d R; Vector3d p;
    std::memcpy(R.data(), R9, 72); std::memcpy(p.data(), p3, 24);
    ConfigParam::SetTbc(R, p);
}
// nav: P(3) q(4) V(3) bg(3) ba(3) dbg(3) dba(3)
int fc_add_keyframe(void* m, long id, const double* nav, const double* K, long prev_id, int bad) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::unique_ptr<KeyFrame> k(new KeyFrame());
    k->mnId = id;
    if ((long unsigned)id + 1 > KeyFrame::nNextId) KeyFrame::nNextId = id + 1;
    k->fx = (float)K[0]; k->fy = (float)K[1]; k->cx = (float)K[2]; k->cy = (float)K[3];
    k->mNavState.Set_Pos({{nav[0], nav[1], nav[2]}});
    k->mNavState.Set_Rot({{nav[3], nav[4], nav[5], nav[6]}});
    k->mNavState.Set_Vel({{nav[7], nav[8], nav[9]}});
    k->mNavState.Set_BiasGyr({{nav[10], nav[11], nav[12]}});
    k->mNavState.Set_BiasAcc({{nav[13], nav[14], nav[15]}});
    k->mNavState.Set_DeltaBiasGyr({{nav[16], nav[17], nav[18]}});
    k->mNavState.Set_DeltaBiasAcc({{nav[19], nav[20], nav[21]}});
    k->mvInvLevelSigma2.resize(8);
    k->mvLevelSigma2.resize(8);
    for (int l = 0; l < 8; l++) k->mvLevelSigma2[l] = (float)std::pow(1.2, 2 * l);
    k->mvScaleFactors.resize(8);
    for (int l = 0; l < 8; l++) k->mvScaleFactors[l] = (float)std::pow(1.2, l);
    for (int l = 0; l < 8; l++) k->mvInvLevelSigma2[l] = 1.0f / (float)std::pow(1.2, 2 * l);  // ORBextractor.cpp:427-441
    k->mbBad = bad != 0;
    if (prev_id >= 0 && M->kfs.count(prev_id)) k->mpPrevKeyFrame = M->kfs[prev_id].get();
    k->UpdatePoseFromNS();
    M->kfs[id] = std::move(k);
    return 0;
}
int fc_set_pose_tcw(void* m, long id, const float* T16) {  // vision-only path: float32 T_cw given directly
    FcMap* M = reinterpret_cast<FcMap*>(m);
    Mat4f T; std::memcpy(T.data(), T16, 64);
    M->kfs.at(id)->SetPose(T);
    return 0;
}
int fc_set_covisible(void* m, long id, const long* ids, int n) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    for (int i = 0; i < n; i++) M->kfs.at(id)->mvpOrderedConnectedKeyFrames.push_back(M->kfs.at(ids[i]).get());
    return 0;
}
int fc_set_preint(void* m, long id, const double* meas61, const double* cov81) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    IMUPreintegrator& P = M->kfs.at(id)->mIMUPreInt;
    P._delta_time = meas61[0];
    std::memcpy(P._delta_P.data(), meas61 + 1, 24); std::memcpy(P._delta_V.data(), meas61 + 4, 24);
    std::memcpy(P._delta_R.data(), meas61 + 7, 72);
    std::memcpy(P._J_P_Biasg.data(), meas61 + 16, 72); std::memcpy(P._J_P_Biasa.data(), meas61 + 25, 72);
    std::memcpy(P._J_V_Biasg.data(), meas61 + 34, 72); std::memcpy(P._J_V_Biasa.data(), meas61 + 43, 72);
    std::memcpy(P._J_R_Biasg.data(), meas61 + 52, 72);
    std::memcpy(P._cov_P_V_Phi.data(), cov81, 648);
    return 0;
}
int fc_add_mappoint(void* m, long id, const float* Pw, long ref_kf) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::unique_ptr<MapPoint> p(new MapPoint());
    p->mnId = id;
    if ((long unsigned)id + 1 > MapPoint::nNextId) MapPoint::nNextId = id + 1;
    p->SetWorldPos(Pw);
    p->mpRefKF = M->kfs.at(ref_kf).get();
    M->mps[id] = std::move(p);
    return 0;
}
int fc_add_observation(void* m, long mp, long kf, float u, float v, int octave) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    KeyFrame* k = M->kfs.at(kf).get();
    MapPoint* p = M->mps.at(mp).get();
    KeyPoint kp; kp.pt.x = u; kp.pt.y = v; kp.octave = octave;
    k->mvKeysUn.push_back(kp);
    k->mvuRight.push_back(-1.0f);
    k->mvpMapPoints.push_back(p);
    p->mObservations[k] = k->mvKeysUn.size() - 1;
    return 0;
}
static std::list<KeyFrame*> window(FcMap* M, const long* ids, int n) {
    std::list<KeyFrame*> l;
    for (int i = 0; i < n; i++) l.push_back(M->kfs.at(ids[i]).get());
    return l;
}
// LocalBAPRVIDP with the CALLER'S flag: `stop` is a bool (one byte) that another thread may raise while the call runs, exactly as
// LocalMapping::InterruptBA does with mbAbortBA (src/LocalMapping.cpp:1769-1772)
int fc_local_ba_prvidp_flag(void* m, const long* ids, int n, const double* gw, bool* stop) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::list<KeyFrame*> l = window(M, ids, n);
    const Vector3d g{{gw[0], gw[1], gw[2]}};
    Optimizer::LocalBAPRVIDP(l.back(), l, stop, &M->map, g, &M->lm);
    return 0;
}
// wall-clock split of this thread's last LocalBAPRVIDP: extraction, solve, erase + write-back, total (ms)
void fc_last_timing(double* out4) {
    const FacadeTiming& t = Optimizer::LastTiming();
    out4[0] = t.extract_ms; out4[1] = t.solve_ms; out4[2] = t.writeback_ms; out4[3] = t.total_ms;
}
// mode 0: full LocalBAPRVIDP; 1: extraction only (no GPU needed)
int fc_local_ba_prvidp(void* m, const long* ids, int n, const double* gw, int stop, int mode) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::list<KeyFrame*> l = window(M, ids, n);
    bool bstop = stop != 0;
    const Vector3d g{{gw[0], gw[1], gw[2]}};
    if (mode == 1) {
        return Optimizer::PackLocalBAPRVIDP(l.back(), l, g, Optimizer::LastWindowMutable()) ? 0 : -1;
    }
    Optimizer::LocalBAPRVIDP(l.back(), l, &bstop, &M->map, g, &M->lm);
    return 0;
}
// LocalBundleAdjustmentNavStatePRV (VI window, XYZ landmarks, LM); mode 1: extraction only
int fc_local_ba_prv_xyz(void* m, const long* ids, int n, const double* gw, int stop, int mode) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::list<KeyFrame*> l = window(M, ids, n);
    bool bstop = stop != 0;
    const Vector3d g{{gw[0], gw[1], gw[2]}};
    if (mode == 1) return Optimizer::PackLocalBundleAdjustmentNavStatePRV(l.back(), l, g, Optimizer::LastWindowMutable()) ? 0 : -1;
    Optimizer::LocalBundleAdjustmentNavStatePRV(l.back(), l, &bstop, &M->map, g, &M->lm);
    return 0;
}
// LocalBundleAdjustment over an explicit keyframe list (include/Optimizer.h:57-59); mode 1: extraction only
int fc_local_ba_vision_list(void* m, const long* ids, int n, int stop, int mode) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::list<KeyFrame*> l = window(M, ids, n);
    bool bstop = stop != 0;
    if (mode == 1) return Optimizer::PackLocalBundleAdjustment(l.back(), &l, Optimizer::LastWindowMutable()) ? 0 : -1;
    Optimizer::LocalBundleAdjustment(l.back(), l, &bstop, &M->map, &M->lm);
    return 0;
}
int fc_local_ba_vision(void* m, long cur, int stop) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    bool bstop = stop != 0;
    Optimizer::LocalBundleAdjustment(M->kfs.at(cur).get(), &bstop, &M->map, &M->lm);
    return 0;
}
static void fill_map(FcMap* M) {
    M->map.mspKeyFrames.clear(); M->map.mspMapPoints.clear();
    for (auto& k : M->kfs) M->map.mspKeyFrames.push_back(k.second.get());
    for (auto& p : M->mps) M->map.mspMapPoints.push_back(p.second.get());
}
// mode 0: run; 1: extraction only (no GPU needed)
int fc_global_ba_prv(void* m, const double* gw, int nIterations, long nLoopKF, int bRobust, int stop, int mode) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    fill_map(M);
    bool bstop = stop != 0;
    const Vector3d g{{gw[0], gw[1], gw[2]}};
    if (mode == 1) return Optimizer::PackGlobalBundleAdjustmentNavStatePRV(&M->map, g, nIterations, bRobust != 0, Optimizer::LastWindowMutable()) ? 0 : -1;
    Optimizer::GlobalBundleAdjustmentNavStatePRV(&M->map, g, nIterations, &bstop, (unsigned long)nLoopKF, bRobust != 0);
    return 0;
}
int fc_global_ba_vision(void* m, int nIterations, long nLoopKF, int bRobust, int stop, int mode) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    fill_map(M);
    bool bstop = stop != 0;
    if (mode == 1) return Optimizer::PackBundleAdjustment(M->map.GetAllKeyFrames(), M->map.GetAllMapPoints(), nIterations, bRobust != 0, Optimizer::LastWindowMutable()) ? 0 : -1;
    Optimizer::GlobalBundleAdjustment(&M->map, nIterations, &bstop, (unsigned long)nLoopKF, bRobust != 0);
    return 0;
}
int fc_get_gba(void* m, long id, double* nav22, float* T16, long* nLoop) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    KeyFrame* k = M->kfs.at(id).get();
    const NavState& ns = k->mNavStateGBA;
    const Vector3d P = ns.Get_P(), V = ns.Get_V(), bg = ns.Get_BiasGyr(), ba = ns.Get_BiasAcc(), dbg = ns.Get_dBias_Gyr(), dba = ns.Get_dBias_Acc();
    const Quaterniond q = ns.Get_R();
    const double v[22] = {P[0], P[1], P[2], q[0], q[1], q[2], q[3], V[0], V[1], V[2], bg[0], bg[1], bg[2], ba[0], ba[1], ba[2],
                          dbg[0], dbg[1], dbg[2], dba[0], dba[1], dba[2]};
    std::memcpy(nav22, v, sizeof v);
    std::memcpy(T16, k->mTcwGBA.data(), 64);
    *nLoop = (long)k->mnBAGlobalForKF;
    return 0;
}
int fc_get_mappoint_gba(void* m, long id, float* Pw, long* nLoop) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    MapPoint* p = M->mps.at(id).get();
    std::memcpy(Pw, p->mPosGBA, 12);
    *nLoop = (long)p->mnBAGlobalForKF;
    return 0;
}
// ---- frames (per-frame pose optimisation) ----
static void set_nav(NavState& ns, const double* nav) {
    ns.Set_Pos({{nav[0], nav[1], nav[2]}});
    ns.Set_Rot({{nav[3], nav[4], nav[5], nav[6]}});
    ns.Set_Vel({{nav[7], nav[8], nav[9]}});
    ns.Set_BiasGyr({{nav[10], nav[11], nav[12]}});
    ns.Set_BiasAcc({{nav[13], nav[14], nav[15]}});
    ns.Set_DeltaBiasGyr({{nav[16], nav[17], nav[18]}});
    ns.Set_DeltaBiasAcc({{nav[19], nav[20], nav[21]}});
}
static void get_nav(const NavState& ns, double* nav22) {
    const Vector3d P = ns.Get_P(), V = ns.Get_V(), bg = ns.Get_BiasGyr(), ba = ns.Get_BiasAcc(), dbg = ns.Get_dBias_Gyr(), dba = ns.Get_dBias_Acc();
    const Quaterniond q = ns.Get_R();
    const double v[22] = {P[0], P[1], P[2], q[0], q[1], q[2], q[3], V[0], V[1], V[2], bg[0], bg[1], bg[2], ba[0], ba[1], ba[2],
                          dbg[0], dbg[1], dbg[2], dba[0], dba[1], dba[2]};
    std::memcpy(nav22, v, sizeof v);
}
int fc_add_frame(void* m, long id, const double* nav22, const double* K) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::unique_ptr<Frame> f(new Frame());
    f->fx = (float)K[0]; f->fy = (float)K[1]; f->cx = (float)K[2]; f->cy = (float)K[3];
    f->mvInvLevelSigma2.resize(8);
    for (int l = 0; l < 8; l++) f->mvInvLevelSigma2[l] = 1.0f / (float)std::pow(1.2, 2 * l);
    set_nav(f->mNavState, nav22);
    f->UpdatePoseFromNS();
    M->frames[id] = std::move(f);
    return 0;
}
int fc_frame_set_tcw(void* m, long id, const float* T16) {
    Mat4f T; std::memcpy(T.data(), T16, 64);
    reinterpret_cast<FcMap*>(m)->frames.at(id)->SetPose(T);
    return 0;
}
int fc_frame_add_obs(void* m, long frame, long mp, float u, float v, int octave) {   // mp < 0: an unmatched keypoint
    FcMap* M = reinterpret_cast<FcMap*>(m);
    Frame* f = M->frames.at(frame).get();
    KeyPoint kp; kp.pt.x = u; kp.pt.y = v; kp.octave = octave;
    f->mvKeysUn.push_back(kp);
    f->mvuRight.push_back(-1.0f);
    f->mvpMapPoints.push_back(mp >= 0 ? M->mps.at(mp).get() : nullptr);
    f->mvbOutlier.push_back(true);   // whatever the tracker left there: the optimiser resets matched ones
    f->N = (int)f->mvKeysUn.size();
    return 0;
}
int fc_frame_set_prior(void* m, long id, const double* prior_nav22, const double* info225) {
    Frame* f = reinterpret_cast<FcMap*>(m)->frames.at(id).get();
    set_nav(f->mNavStatePrior, prior_nav22);
    std::memcpy(f->mMargCovInv.data(), info225, 225 * 8);
    return 0;
}
static IMUPreintegrator make_preint(const double* meas61, const double* cov81) {
    IMUPreintegrator P;
    P._delta_time = meas61[0];
    std::memcpy(P._delta_P.data(), meas61 + 1, 24); std::memcpy(P._delta_V.data(), meas61 + 4, 24);
    std::memcpy(P._delta_R.data(), meas61 + 7, 72);
    std::memcpy(P._J_P_Biasg.data(), meas61 + 16, 72); std::memcpy(P._J_P_Biasa.data(), meas61 + 25, 72);
    std::memcpy(P._J_V_Biasg.data(), meas61 + 34, 72); std::memcpy(P._J_V_Biasa.data(), meas61 + 43, 72);
    std::memcpy(P._J_R_Biasg.data(), meas61 + 52, 72);
    std::memcpy(P._cov_P_V_Phi.data(), cov81, 648);
    return P;
}
// kind 2: PoseOptimization(Frame*); 0: (Frame*, KeyFrame* last, ...); 1: (Frame*, Frame* last, ...).  Returns the inlier count.
int fc_pose_optimization(void* m, int kind, long frame, long last, const double* meas61, const double* cov81, const double* gw, int marg) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    Frame* f = M->frames.at(frame).get();
    if (kind == 2) return Optimizer::PoseOptimization(f);
    const IMUPreintegrator pre = make_preint(meas61, cov81);
    const Vector3d g{{gw[0], gw[1], gw[2]}};
    if (kind == 0) return Optimizer::PoseOptimization(f, M->kfs.at(last).get(), pre, g, marg != 0);
    return Optimizer::PoseOptimization(f, M->frames.at(last).get(), pre, g, marg != 0);
}
int fc_frame_get(void* m, long id, double* nav22, float* T16, double* marg225, double* prior22, unsigned char* outlier, int cap) {
    Frame* f = reinterpret_cast<FcMap*>(m)->frames.at(id).get();
    get_nav(f->GetNavState(), nav22);
    std::memcpy(T16, f->mTcw.data(), 64);
    std::memcpy(marg225, f->mMargCovInv.data(), 225 * 8);
    get_nav(f->mNavStatePrior, prior22);
    for (int i = 0; i < f->N && i < cap; i++) outlier[i] = f->mvbOutlier[i] ? 1 : 0;
    return f->N;
}
int fc_get_nav(void* m, long id, double* nav22, float* T16) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    KeyFrame* k = M->kfs.at(id).get();
    const NavState& ns = k->GetNavState();
    const Vector3d P = ns.Get_P(), V = ns.Get_V(), bg = ns.Get_BiasGyr(), ba = ns.Get_BiasAcc(), dbg = ns.Get_dBias_Gyr(), dba = ns.Get_dBias_Acc();
    const Quaterniond q = ns.Get_R();
    const double v[22] = {P[0], P[1], P[2], q[0], q[1], q[2], q[3], V[0], V[1], V[2], bg[0], bg[1], bg[2], ba[0], ba[1], ba[2],
                          dbg[0], dbg[1], dbg[2], dba[0], dba[1], dba[2]};
    std::memcpy(nav22, v, sizeof v);
    std::memcpy(T16, k->GetPose().data(), 64);
    return 0;
}
int fc_get_mappoint(void* m, long id, float* Pw, int* n_obs, int* n_updates) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    MapPoint* p = M->mps.at(id).get();
    std::memcpy(Pw, p->mWorldPos, 12);
    *n_obs = (int)p->mObservations.size();
    *n_updates = p->nNormalUpdates;
    return 0;
}
// ---- loop-closure Sim3 refinement ----
// one keypoint of a keyframe, with or without a map point (mp < 0: mvpMapPoints[i] = NULL); observe = 0 leaves the point's
// observation map without the keyframe (GetIndexInKeyFrame < 0)
int fc_kf_add_keypoint(void* m, long kf, long mp, float u, float v, int octave, int observe) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    KeyFrame* k = M->kfs.at(kf).get();
    MapPoint* p = mp >= 0 ? M->mps.at(mp).get() : nullptr;
    KeyPoint kp; kp.pt.x = u; kp.pt.y = v; kp.octave = octave;
    k->mvKeysUn.push_back(kp);
    k->mvuRight.push_back(-1.0f);
    k->mvpMapPoints.push_back(p);
    if (p && observe) p->mObservations[k] = k->mvKeysUn.size() - 1;
    return (int)k->mvKeysUn.size() - 1;
}
int fc_set_mappoint_bad(void* m, long mp, int bad) {
    reinterpret_cast<FcMap*>(m)->mps.at(mp)->mbBad = bad != 0;
    return 0;
}
// Optimizer::OptimizeSim3(kf1, kf2, vpMatches1, g2oS12, th2, bFixScale): matches[i] = id of the map point matched to keypoint i
// of kf1 (-1: NULL), rewritten in place (-1 where the call nulled the entry); S12 = t(3) q(4, xyzw) s in / out.  Returns the count.
int fc_optimize_sim3(void* m, long kf1, long kf2, long* matches, int n, double* S12, float th2, int fix_scale) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::vector<MapPoint*> vpMatches1((size_t)n, nullptr);
    for (int i = 0; i < n; i++)
        if (matches[i] >= 0) vpMatches1[i] = M->mps.at(matches[i]).get();
    g2o::Sim3 S({{S12[3], S12[4], S12[5], S12[6]}}, {{S12[0], S12[1], S12[2]}}, S12[7]);
    const int nIn = Optimizer::OptimizeSim3(M->kfs.at(kf1).get(), M->kfs.at(kf2).get(), vpMatches1, S, th2, fix_scale != 0);
    for (int i = 0; i < n; i++) matches[i] = vpMatches1[i] ? (long)vpMatches1[i]->mnId : -1;
    for (int k = 0; k < 3; k++) S12[k] = S.translation()[k];
    for (int k = 0; k < 4; k++) S12[3 + k] = S.rotation()[k];
    S12[7] = S.scale();
    return nIn;
}
// g2o::Sim3 members: out[0..2] = a.map(x), out[3..10] = a.inverse(), out[11..18] = a * b   (t, q, s each)
void fc_sim3_ops(const double* a8, const double* b8, const double* x3, double* out19) {
    const g2o::Sim3 A({{a8[3], a8[4], a8[5], a8[6]}}, {{a8[0], a8[1], a8[2]}}, a8[7]), B({{b8[3], b8[4], b8[5], b8[6]}}, {{b8[0], b8[1], b8[2]}}, b8[7]);
    const Vector3d y = A.map({{x3[0], x3[1], x3[2]}});
    auto put = [](const g2o::Sim3& S, double* o) {
        for (int k = 0; k < 3; k++) o[k] = S.translation()[k];
        for (int k = 0; k < 4; k++) o[3 + k] = S.rotation()[k];
        o[7] = S.scale();
    };
    for (int k = 0; k < 3; k++) out19[k] = y[k];
    put(A.inverse(), out19 + 3);
    put(A * B, out19 + 11);
}
// ---- loop-candidate Sim3 RANSAC (Sim3Solver.h) ----
// Sim3Solver(kf1, kf2, vpMatched12, bFixScale): matches[i] = id of the map point matched to keypoint i of kf1 (-1: NULL)
void* fc_sim3solver_create(void* m, long kf1, long kf2, const long* matches, int n, int fix_scale) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::vector<MapPoint*> v((size_t)n, nullptr);
    for (int i = 0; i < n; i++)
        if (matches[i] >= 0) v[i] = M->mps.at(matches[i]).get();
    return new Sim3Solver(M->kfs.at(kf1).get(), M->kfs.at(kf2).get(), v, fix_scale != 0);
}
void fc_sim3solver_destroy(void* s) { delete reinterpret_cast<Sim3Solver*>(s); }
void fc_sim3solver_set_ransac(void* s, double probability, int min_inliers, int max_iterations) {
    reinterpret_cast<Sim3Solver*>(s)->SetRansacParameters(probability, min_inliers, max_iterations);
}
// out: N, mN1, mRansacMaxIts, mnIterations, mnBestInliers, mRansacMinInliers
void fc_sim3solver_info(void* s, int* out6) {
    const Sim3Solver* S = reinterpret_cast<Sim3Solver*>(s);
    out6[0] = S->N; out6[1] = S->mN1; out6[2] = S->mRansacMaxIts; out6[3] = S->mnIterations; out6[4] = S->mnBestInliers; out6[5] = S->mRansacMinInliers;
}
// the constructor's products: mvnIndices1 [N], the gates [N] each, mvX3Dc1 / mvX3Dc2 [N][3], K1 / K2 [4]
void fc_sim3solver_arrays(void* s, long* indices1, double* gate1, double* gate2, double* p1c, double* p2c, double* K1, double* K2) {
    const Sim3Solver* S = reinterpret_cast<Sim3Solver*>(s);
    for (size_t i = 0; i < S->mvnIndices1.size(); i++) {
        indices1[i] = (long)S->mvnIndices1[i];
        gate1[i] = (double)S->mvnMaxError1[i];
        gate2[i] = (double)S->mvnMaxError2[i];
    }
    if (!S->mvX3Dc1.empty()) {
        std::memcpy(p1c, S->mvX3Dc1.data(), 8 * S->mvX3Dc1.size());
        std::memcpy(p2c, S->mvX3Dc2.data(), 8 * S->mvX3Dc2.size());
    }
    std::memcpy(K1, S->mK1, 32);
    std::memcpy(K2, S->mK2, 32);
}
void fc_srand(unsigned seed) { srand(seed); }
// the draw alone (no backend call): n hypotheses, triples [n][3]
void fc_sim3solver_draw(void* s, int n, int32_t* triples) {
    std::vector<int32_t> t;
    reinterpret_cast<Sim3Solver*>(s)->DrawTriples(n, t);
    if (!t.empty()) std::memcpy(triples, t.data(), 4 * t.size());
}
// iterate(nIterations, ...) (find when nIterations < 0): returns 1 with T12 on a hit; inliers [mN1]; triples: the draws of the
// call [up to max_hyp][3], *n_hyp how many hypotheses were drawn
int fc_sim3solver_iterate(void* s, int nIterations, int* no_more, uint8_t* inliers, int* n_inliers, float* T16, int32_t* triples, int max_hyp,
                          int* n_hyp) {
    Sim3Solver* S = reinterpret_cast<Sim3Solver*>(s);
    std::vector<bool> vb;
    bool bNoMore = false;
    Mat4f T{};
    const bool found = nIterations < 0 ? S->find(vb, *n_inliers, T) : S->iterate(nIterations, bNoMore, vb, *n_inliers, T);
    *no_more = bNoMore ? 1 : 0;
    for (size_t i = 0; i < vb.size(); i++) inliers[i] = vb[i] ? 1 : 0;
    std::memcpy(T16, T.data(), 64);
    *n_hyp = (int)S->mvLastTriples.size() / 3;
    if (*n_hyp > 0) std::memcpy(triples, S->mvLastTriples.data(), 12 * (size_t)std::min(*n_hyp, max_hyp));
    return found ? 1 : 0;
}
// GetEstimatedRotation [9] / Translation [3] / Scale
void fc_sim3solver_estimate(void* s, float* R9, float* t3, float* scale) {
    Sim3Solver* S = reinterpret_cast<Sim3Solver*>(s);
    const std::array<float, 9> R = S->GetEstimatedRotation();
    const std::array<float, 3> t = S->GetEstimatedTranslation();
    std::memcpy(R9, R.data(), 36);
    std::memcpy(t3, t.data(), 12);
    *scale = S->GetEstimatedScale();
}
// ---- monocular map initialisation (Initializer.h) ----
// Initializer(ReferenceFrame, sigma, iterations) over a Frame made of K (fx fy cx cy) and n keypoints uv [n][2]
void* fc_initializer_create(const float* K, const float* uv, int n, float sigma, int iterations) {
    Frame F;
    F.fx = K[0]; F.fy = K[1]; F.cx = K[2]; F.cy = K[3];
    F.N = n;
    F.mvKeysUn.resize((size_t)n);
    for (int i = 0; i < n; i++) { F.mvKeysUn[i].pt.x = uv[2 * i]; F.mvKeysUn[i].pt.y = uv[2 * i + 1]; }
    return new Initializer(F, sigma, iterations);
}
void fc_initializer_destroy(void* s) { delete reinterpret_cast<Initializer*>(s); }
// Initialize(CurrentFrame, vMatches12 [n keypoints of the reference frame], ...): returns its return value; R21 [9], t21 [3],
// vP3D [n1][3] and vbTriangulated [n1] are written on success only; sets [iterations][8]: mvSets of the call; info [10]: ok model
// reason best_hyp_h best_hyp_f n_inliers_h n_inliers_f n_rt best_rt n_matches of the backend call
int fc_initializer_initialize(void* s, const float* uv2, int n2, const int* vMatches12, int n1, float* R21, float* t21, float* vP3D,
                              uint8_t* vbTriangulated, int32_t* sets, int32_t* info) {
    Initializer* I = reinterpret_cast<Initializer*>(s);
    Frame F;
    F.N = n2;
    F.mvKeysUn.resize((size_t)n2);
    for (int i = 0; i < n2; i++) { F.mvKeysUn[i].pt.x = uv2[2 * i]; F.mvKeysUn[i].pt.y = uv2[2 * i + 1]; }
    std::array<float, 9> R{};
    std::array<float, 3> t{};
    std::vector<Point3f> P3D;
    std::vector<bool> tri;
    const bool ok = I->Initialize(F, std::vector<int>(vMatches12, vMatches12 + n1), R, t, P3D, tri);
    if (ok) {
        std::memcpy(R21, R.data(), 36);
        std::memcpy(t21, t.data(), 12);
        for (size_t i = 0; i < P3D.size(); i++) { vP3D[3 * i] = P3D[i].x; vP3D[3 * i + 1] = P3D[i].y; vP3D[3 * i + 2] = P3D[i].z; vbTriangulated[i] = tri[i] ? 1 : 0; }
    }
    for (size_t it = 0; it < I->mvSets.size(); it++)
        for (int j = 0; j < 8; j++) sets[8 * it + j] = (int32_t)I->mvSets[it][j];
    const vba_two_view_result& L = I->mLast;
    const int32_t v[10] = {L.ok, L.model, L.reason, L.best_hyp_h, L.best_hyp_f, L.n_inliers_h, L.n_inliers_f, L.n_rt, L.best_rt, (int32_t)I->mvMatches12.size()};
    std::memcpy(info, v, sizeof v);
    return ok ? 1 : 0;
}
// ---- the matcher of the monocular initialisation (ORBmatcher::SearchForInitialization, the Tracking slice) ----
// a Frame of n keypoints as the matcher reads it: uv [n][2], octaves, angles, N x 32 descriptor bytes, K (fx fy cx cy), the image
// bounds (min_x max_x min_y max_y) and the grid, which is assigned here; mvKeys = mvKeysUn, every keypoint monocular
void* fc_init_frame_create(int n, const float* uv, const int* octave, const float* angle, const unsigned char* desc, const float* K, const float* bounds,
                           int cols, int rows) {
    Frame* F = new Frame();
    F->fx = K[0]; F->fy = K[1]; F->cx = K[2]; F->cy = K[3];
    F->N = n;
    F->mvKeysUn.resize((size_t)n);
    for (int i = 0; i < n; i++) {
        KeyPoint& kp = F->mvKeysUn[(size_t)i];
        kp.pt.x = uv[2 * i]; kp.pt.y = uv[2 * i + 1]; kp.octave = octave[i]; kp.angle = angle[i];
    }
    F->mvKeys = F->mvKeysUn;
    F->mvuRight.assign((size_t)n, -1.0f);
    F->mvpMapPoints.assign((size_t)n, nullptr);
    F->mDescriptors.assign(desc, desc + 32 * (size_t)n);
    F->mnScaleLevels = 8;
    F->mvScaleFactors.resize(8);
    for (int l = 0; l < 8; l++) F->mvScaleFactors[(size_t)l] = (float)std::pow(1.2, l);
    F->mnMinX = bounds[0]; F->mnMaxX = bounds[1]; F->mnMinY = bounds[2]; F->mnMaxY = bounds[3];
    F->mnGridCols = cols; F->mnGridRows = rows;
    F->AssignFeaturesToGrid();
    return F;
}
void fc_init_frame_destroy(void* f) { delete reinterpret_cast<Frame*>(f); }
void fc_init_frame_set_uright(void* f, int idx, float ur) { reinterpret_cast<Frame*>(f)->mvuRight.at((size_t)idx) = ur; }
// ORBmatcher(nnratio, check_ori).SearchForInitialization(F1, F2, vbPrevMatched [n_prev][2] in and out, vnMatches12, windowSize); matches
// [cap] receives vnMatches12 as the call leaves it (n_out: its size).  Returns the return value
int fc_search_for_initialization(void* f1, void* f2, float* prev, int n_prev, int* matches, int cap, int* n_out, float nnratio, int check_ori, int window) {
    std::vector<Point2f> vbPrevMatched((size_t)n_prev);
    for (int i = 0; i < n_prev; i++) { vbPrevMatched[(size_t)i].x = prev[2 * i]; vbPrevMatched[(size_t)i].y = prev[2 * i + 1]; }
    std::vector<int> vnMatches12;
    ORBmatcher matcher(nnratio, check_ori != 0);
    const int r = matcher.SearchForInitialization(*reinterpret_cast<Frame*>(f1), *reinterpret_cast<Frame*>(f2), vbPrevMatched, vnMatches12, window);
    for (int i = 0; i < n_prev; i++) { prev[2 * i] = vbPrevMatched[(size_t)i].x; prev[2 * i + 1] = vbPrevMatched[(size_t)i].y; }
    *n_out = (int)vnMatches12.size();
    for (size_t i = 0; i < vnMatches12.size() && (int)i < cap; i++) matches[i] = vnMatches12[i];
    return r;
}
// Tracking::MonocularInitializationMatches with mInitialFrame = f_init, mCurrentFrame = f_cur, mvbPrevMatched = prev [n1][2] (in and
// out), mvIniMatches = matches [n1] (in and out) and an Initializer(mInitialFrame, 1.0, 200).  alive: whether the initializer
// survived.  With do_initialize and a live initializer the slice's matches go on into Initialize (src/Tracking.cpp:1388), whose
// outputs are those of fc_initializer_initialize and whose return value lands in init_ret (-1: not called).  Returns the slice's
// return value
int fc_monocular_initialization(void* f_init, void* f_cur, float* prev, int* matches, int n1, int do_initialize, int* alive, int* init_ret, float* R21,
                                float* t21, float* vP3D, uint8_t* vbTriangulated, int32_t* sets, int32_t* info) {
    Tracking t;
    t.mInitialFrame = *reinterpret_cast<Frame*>(f_init);
    t.mCurrentFrame = *reinterpret_cast<Frame*>(f_cur);
    t.mvbPrevMatched.resize((size_t)n1);
    for (int i = 0; i < n1; i++) { t.mvbPrevMatched[(size_t)i].x = prev[2 * i]; t.mvbPrevMatched[(size_t)i].y = prev[2 * i + 1]; }
    t.mvIniMatches.assign(matches, matches + n1);
    t.mpInitializer.reset(new Initializer(t.mInitialFrame, 1.0, 200));
    const int r = t.MonocularInitializationMatches();
    for (int i = 0; i < n1; i++) { prev[2 * i] = t.mvbPrevMatched[(size_t)i].x; prev[2 * i + 1] = t.mvbPrevMatched[(size_t)i].y; }
    for (int i = 0; i < n1 && (size_t)i < t.mvIniMatches.size(); i++) matches[i] = t.mvIniMatches[(size_t)i];
    *alive = t.mpInitializer ? 1 : 0;
    *init_ret = -1;
    if (!t.mpInitializer || !do_initialize) return r;
    Initializer* I = t.mpInitializer.get();
    std::array<float, 9> R{};
    std::array<float, 3> tt{};
    std::vector<Point3f> P3D;
    std::vector<bool> tri;
    const bool ok = I->Initialize(t.mCurrentFrame, t.mvIniMatches, R, tt, P3D, tri);
    if (ok) {
        std::memcpy(R21, R.data(), 36);
        std::memcpy(t21, tt.data(), 12);
        for (size_t i = 0; i < P3D.size(); i++) { vP3D[3 * i] = P3D[i].x; vP3D[3 * i + 1] = P3D[i].y; vP3D[3 * i + 2] = P3D[i].z; vbTriangulated[i] = tri[i] ? 1 : 0; }
    }
    for (size_t it = 0; it < I->mvSets.size(); it++)
        for (int j = 0; j < 8; j++) sets[8 * it + j] = (int32_t)I->mvSets[it][j];
    const vba_two_view_result& L = I->mLast;
    const int32_t v[10] = {L.ok, L.model, L.reason, L.best_hyp_h, L.best_hyp_f, L.n_inliers_h, L.n_inliers_f, L.n_rt, L.best_rt, (int32_t)I->mvMatches12.size()};
    std::memcpy(info, v, sizeof v);
    *init_ret = ok ? 1 : 0;
    return r;
}
// ---- new map points (LocalMapping::CreateNewMapPoints, LocalMapping.cpp) ----
// The matcher is a table: neighbour i of `neigh` gets matches [begin[i], begin[i + 1]) of `matches` ([..][2] keypoint indices in kf /
// in the neighbour).  seen[i]: how many keypoints of kf had a map point when the matcher was called for neighbour i, -1 where it was
// not called (the neighbour failed the baseline gate).  The created points move into the map under their mnId; new_ids lists them
// in the order of the recent list.  Returns nnew (-1: the backend failed)
int fc_create_new_map_points(void* m, long kf, const long* neigh, int n_neigh, const int* begin, const long* matches, int* seen, long* new_ids, int cap) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    KeyFrame* pKF = M->kfs.at(kf).get();
    std::vector<KeyFrame*> vpNeighKFs;
    for (int i = 0; i < n_neigh; i++) { vpNeighKFs.push_back(M->kfs.at(neigh[i]).get()); seen[i] = -1; }
    const TriangulationMatcher matcher = [&](KeyFrame* k1, KeyFrame* k2, std::vector<std::pair<size_t, size_t>>& out) {
        const int i = (int)(std::find(vpNeighKFs.begin(), vpNeighKFs.end(), k2) - vpNeighKFs.begin());
        seen[i] = (int)std::count_if(k1->mvpMapPoints.begin(), k1->mvpMapPoints.end(), [](MapPoint* p) { return p != nullptr; });
        for (int j = begin[i]; j < begin[i + 1]; j++) out.emplace_back((size_t)matches[2 * j], (size_t)matches[2 * j + 1]);
    };
    std::list<MapPoint*> recent;
    const int nnew = M->lm.CreateNewMapPoints(pKF, vpNeighKFs, matcher, &M->map, recent);
    int k = 0;
    for (MapPoint* p : recent) {
        if (k < cap) new_ids[k] = (long)p->mnId;
        k++;
        M->mps[(long)p->mnId].reset(p);
    }
    return nnew;
}
// one map point in full: position, reference keyframe, nObs, and its observations as (keyframe id, keypoint index) in keyframe order
int fc_get_mappoint_obs(void* m, long id, float* Pw, long* ref_kf, int* n_obs_counter, long* obs, int cap) {
    MapPoint* p = reinterpret_cast<FcMap*>(m)->mps.at(id).get();
    std::memcpy(Pw, p->mWorldPos, 12);
    *ref_kf = p->mpRefKF ? (long)p->mpRefKF->mnId : -1;
    *n_obs_counter = p->nObs;
    int k = 0;
    for (const auto& o : p->mObservations) {
        if (k < cap) { obs[2 * k] = (long)o.first->mnId; obs[2 * k + 1] = (long)o.second; }
        k++;
    }
    return k;
}
// the map point id behind keypoint idx of a keyframe (-1: NULL), and how many points the map lists
long fc_kf_mappoint_at(void* m, long kf, int idx) {
    MapPoint* p = reinterpret_cast<FcMap*>(m)->kfs.at(kf)->mvpMapPoints.at(idx);
    return p ? (long)p->mnId : -1;
}
int fc_map_n_points(void* m) { return (int)reinterpret_cast<FcMap*>(m)->map.mspMapPoints.size(); }
float fc_kf_median_depth(void* m, long kf, int q) { return reinterpret_cast<FcMap*>(m)->kfs.at(kf)->ComputeSceneMedianDepth(q); }
// ---- the matcher (ORBmatcher::SearchForTriangulation, ORBmatcher.cpp) ----
// what the matcher reads beside the keypoints: N x 32 descriptor bytes, one angle per keypoint, the feature vector in CSR form
// (node ids ascending); N becomes the number of keypoints the keyframe holds
int fc_kf_set_matcher_data(void* m, long kf, const unsigned char* desc, const float* angle, int n_nodes, const unsigned int* node_id, const int* node_begin,
                           const int* node_feat) {
    KeyFrame* k = reinterpret_cast<FcMap*>(m)->kfs.at(kf).get();
    k->N = (int)k->mvKeysUn.size();
    k->mDescriptors.assign(desc, desc + 32 * (size_t)k->N);
    for (int i = 0; i < k->N; i++) k->mvKeysUn[i].angle = angle[i];
    k->mFeatVec.clear();
    for (int j = 0; j < n_nodes; j++) {
        std::vector<unsigned int>& v = k->mFeatVec[node_id[j]];
        for (int i = node_begin[j]; i < node_begin[j + 1]; i++) v.push_back((unsigned int)node_feat[i]);
    }
    return k->N;
}
void fc_compute_f12(void* m, long kf1, long kf2, float* F9, float* epipole2) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    const Mat3f F = LocalMapping::ComputeF12(M->kfs.at(kf1).get(), M->kfs.at(kf2).get());
    std::memcpy(F9, F.data(), 36);
    ORBmatcher::Epipole(M->kfs.at(kf1).get(), M->kfs.at(kf2).get(), epipole2[0], epipole2[1]);
}
// ORBmatcher(0.6, check_ori)::SearchForTriangulation with ComputeF12's matrix: the return value, pairs [cap][2] filled up to cap
int fc_search_for_triangulation(void* m, long kf1, long kf2, int check_ori, int only_stereo, long* pairs, int cap) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    KeyFrame *k1 = M->kfs.at(kf1).get(), *k2 = M->kfs.at(kf2).get();
    ORBmatcher matcher(0.6, check_ori != 0);
    std::vector<std::pair<size_t, size_t>> v;
    const int n = matcher.SearchForTriangulation(k1, k2, LocalMapping::ComputeF12(k1, k2), v, only_stereo != 0);
    for (size_t i = 0; i < v.size() && (int)i < cap; i++) { pairs[2 * i] = (long)v[i].first; pairs[2 * i + 1] = (long)v[i].second; }
    return n;
}
// CreateNewMapPoints without a matcher table (the overload that calls the matcher itself); new_ids as fc_create_new_map_points
int fc_create_new_map_points_matched(void* m, long kf, const long* neigh, int n_neigh, long* new_ids, int cap) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::vector<KeyFrame*> vpNeighKFs;
    for (int i = 0; i < n_neigh; i++) vpNeighKFs.push_back(M->kfs.at(neigh[i]).get());
    std::list<MapPoint*> recent;
    const int nnew = M->lm.CreateNewMapPoints(M->kfs.at(kf).get(), vpNeighKFs, &M->map, recent);
    int k = 0;
    for (MapPoint* p : recent) {
        if (k < cap) new_ids[k] = (long)p->mnId;
        k++;
        M->mps[(long)p->mnId].reset(p);
    }
    return nnew;
}
// ---- map-point fusion (ORBmatcher::Fuse, LocalMapping::SearchInNeighbors) ----
// what Fuse reads of a keyframe beside the keypoints: N x 32 descriptor bytes, the image bounds and the grid, which is assigned here
// as Frame::AssignFeaturesToGrid does; N becomes the number of keypoints the keyframe holds
int fc_kf_set_fuse_data(void* m, long kf, const unsigned char* desc, int min_x, int max_x, int min_y, int max_y, int cols, int rows) {
    KeyFrame* k = reinterpret_cast<FcMap*>(m)->kfs.at(kf).get();
    k->N = (int)k->mvKeysUn.size();
    k->mDescriptors.assign(desc, desc + 32 * (size_t)k->N);
    k->mnMinX = min_x; k->mnMaxX = max_x; k->mnMinY = min_y; k->mnMaxY = max_y;
    k->mnGridCols = cols; k->mnGridRows = rows;
    k->AssignFeaturesToGrid();
    return k->N;
}
// the grid in CSR form: cell (ix, iy) at ix * rows + iy; returns the number of listed keypoints
int fc_kf_grid(void* m, long kf, int* cell_begin, int* cell_feat, float* inv_wh) {
    KeyFrame* k = reinterpret_cast<FcMap*>(m)->kfs.at(kf).get();
    int n = 0, c = 0;
    cell_begin[0] = 0;
    for (int ix = 0; ix < k->mnGridCols; ix++)
        for (int iy = 0; iy < k->mnGridRows; iy++) {
            for (size_t idx : k->mGrid[(size_t)ix][(size_t)iy]) cell_feat[n++] = (int)idx;
            cell_begin[++c] = n;
        }
    inv_wh[0] = k->mfGridElementWidthInv; inv_wh[1] = k->mfGridElementHeightInv;
    return n;
}
int fc_kf_set_uright(void* m, long kf, int idx, float ur) {
    reinterpret_cast<FcMap*>(m)->kfs.at(kf)->mvuRight.at(idx) = ur;
    return 0;
}
// what Fuse reads of a map point beside its position; nObs becomes the number of its observations, and the point joins the map
int fc_mp_set_fuse_data(void* m, long mp, const float* normal, float min_distance, float max_distance, const unsigned char* desc) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    MapPoint* p = M->mps.at(mp).get();
    std::memcpy(p->mNormalVector, normal, 12);
    p->mfMinDistance = min_distance; p->mfMaxDistance = max_distance;
    std::memcpy(p->mDescriptor, desc, 32);
    p->nObs = (int)p->mObservations.size();
    p->mpMap = &M->map;
    M->map.AddMapPoint(p);
    return 0;
}
static std::vector<MapPoint*> point_list(FcMap* M, const long* ids, int n) {
    std::vector<MapPoint*> v;
    for (int i = 0; i < n; i++) v.push_back(ids[i] >= 0 ? M->mps.at(ids[i]).get() : nullptr);
    return v;
}
// ORBmatcher::Fuse(pKF, vpMapPoints, th); an id of -1 is a NULL entry
int fc_fuse(void* m, long kf, const long* mp_ids, int n, float th) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    ORBmatcher matcher;
    return matcher.Fuse(M->kfs.at(kf).get(), point_list(M, mp_ids, n), th);
}
// ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint): replace_ids [n] comes back with the ids of vpReplacePoint (-1: NULL)
int fc_fuse_sim3(void* m, long kf, const float* Scw16, const long* mp_ids, int n, float th, long* replace_ids) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    Mat4f S; std::memcpy(S.data(), Scw16, 64);
    std::vector<MapPoint*> rep((size_t)n, nullptr);
    ORBmatcher matcher;
    const int r = matcher.Fuse(M->kfs.at(kf).get(), S, point_list(M, mp_ids, n), th, rep);
    for (int i = 0; i < n; i++) replace_ids[i] = rep[(size_t)i] ? (long)rep[(size_t)i]->mnId : -1;
    return r;
}
int fc_search_in_neighbors(void* m, long kf, const long* targets, int n) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::vector<KeyFrame*> v;
    for (int i = 0; i < n; i++) v.push_back(M->kfs.at(targets[i]).get());
    return M->lm.SearchInNeighbors(M->kfs.at(kf).get(), v);
}
// out5: bad, the id of mpReplaced (-1: NULL), nObs, the ComputeDistinctiveDescriptors counter, 1 if the map still lists the point
int fc_mp_fuse_state(void* m, long mp, long* out5) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    MapPoint* p = M->mps.at(mp).get();
    out5[0] = p->mbBad ? 1 : 0;
    out5[1] = p->mpReplaced ? (long)p->mpReplaced->mnId : -1;
    out5[2] = p->nObs;
    out5[3] = p->nDescriptorUpdates;
    out5[4] = (long)std::count(M->map.mspMapPoints.begin(), M->map.mspMapPoints.end(), p);
    return 0;
}
// ---- map-point refresh (UpdateMapPoints, the two LocalMapping loops; MapPointUpdate.cpp) ----
// UpdateMapPoints(the points `ids`, what); an id of -1 is a NULL entry
int fc_update_map_points(void* m, const long* mp_ids, int n, int what) { return UpdateMapPoints(point_list(reinterpret_cast<FcMap*>(m), mp_ids, n), what); }
// LocalMapping::ProcessNewKeyFramePoints(kf, list): recent [cap] receives the ids the call appended to an empty mlpRecentAddedMapPoints,
// in order (n_recent: how many)
int fc_process_new_keyframe_points(void* m, long kf, long* recent, int cap, int* n_recent) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::list<MapPoint*> l;
    const int r = M->lm.ProcessNewKeyFramePoints(M->kfs.at(kf).get(), l);
    *n_recent = (int)l.size();
    int k = 0;
    for (MapPoint* p : l)
        if (k < cap) recent[k++] = (long)p->mnId;
    return r;
}
int fc_update_current_keyframe_points(void* m, long kf) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    return M->lm.UpdateCurrentKeyFramePoints(M->kfs.at(kf).get());
}
// what the refresh writes and what it must leave alone: mNormalVector, (mfMinDistance, mfMaxDistance), mDescriptor; counters: the
// UpdateNormalAndDepth stub's, the ComputeDistinctiveDescriptors stub's, the size of mObservations, nObs
int fc_mp_attributes(void* m, long mp, float* normal3, float* minmax2, unsigned char* desc32, int* counters4) {
    MapPoint* p = reinterpret_cast<FcMap*>(m)->mps.at(mp).get();
    std::memcpy(normal3, p->mNormalVector, 12);
    minmax2[0] = p->mfMinDistance; minmax2[1] = p->mfMaxDistance;
    std::memcpy(desc32, p->mDescriptor, 32);
    counters4[0] = p->nNormalUpdates; counters4[1] = p->nDescriptorUpdates; counters4[2] = (int)p->mObservations.size(); counters4[3] = p->nObs;
    return 0;
}
// ---- projection matching for tracking (both ORBmatcher::SearchByProjection overloads, the Tracking slice) ----
// what the tracking matchers read of a frame beside the keypoints fc_frame_add_obs gave it: the id, N x 32 descriptor bytes, the
// keypoint angles, the image bounds and the grid, which is assigned here; eight levels of factor 1.2; mvKeys = mvKeysUn; the pose
// parts of UpdatePoseMatrices.  N becomes the number of keypoints the frame holds
int fc_frame_set_tracking_data(void* m, long frame, long id, const unsigned char* desc, const float* angle, float min_x, float max_x, float min_y,
                               float max_y, int cols, int rows) {
    Frame* f = reinterpret_cast<FcMap*>(m)->frames.at(frame).get();
    f->mnId = (long unsigned)id;
    f->N = (int)f->mvKeysUn.size();
    for (int i = 0; i < f->N; i++) f->mvKeysUn[(size_t)i].angle = angle[i];
    f->mvKeys = f->mvKeysUn;
    f->mDescriptors.assign(desc, desc + 32 * (size_t)f->N);
    f->mnScaleLevels = 8;
    f->mvScaleFactors.resize(8);
    for (int l = 0; l < 8; l++) f->mvScaleFactors[(size_t)l] = (float)std::pow(1.2, l);
    f->mnMinX = min_x; f->mnMaxX = max_x; f->mnMinY = min_y; f->mnMaxY = max_y;
    f->mnGridCols = cols; f->mnGridRows = rows;
    f->AssignFeaturesToGrid();
    f->UpdatePoseMatrices();
    return f->N;
}
int fc_frame_set_outlier(void* m, long frame, int idx, int outlier) {
    reinterpret_cast<FcMap*>(m)->frames.at(frame)->mvbOutlier.at((size_t)idx) = outlier != 0;
    return 0;
}
int fc_frame_set_uright(void* m, long frame, int idx, float ur) {
    reinterpret_cast<FcMap*>(m)->frames.at(frame)->mvuRight.at((size_t)idx) = ur;
    return 0;
}
// the ids behind mvpMapPoints (-1: NULL); returns N
int fc_frame_points(void* m, long frame, long* ids, int cap) {
    Frame* f = reinterpret_cast<FcMap*>(m)->frames.at(frame).get();
    for (int i = 0; i < f->N && i < cap; i++) ids[i] = f->mvpMapPoints[(size_t)i] ? (long)f->mvpMapPoints[(size_t)i]->mnId : -1;
    return f->N;
}
// nObs as the test wants it (Observations() > 0 decides whether a point blocks its keypoint), mbTrackInView, mnLastFrameSeen
int fc_mp_set_track(void* m, long mp, int n_obs, int in_view, long last_frame_seen) {
    MapPoint* p = reinterpret_cast<FcMap*>(m)->mps.at(mp).get();
    p->nObs = n_obs; p->mbTrackInView = in_view != 0; p->mnLastFrameSeen = (long unsigned)last_frame_seen;
    return 0;
}
// out7: mbTrackInView, mTrackProjX, mTrackProjY, mnTrackScaleLevel, mTrackViewCos, mnVisible, mnLastFrameSeen
int fc_mp_track_state(void* m, long mp, double* out7) {
    MapPoint* p = reinterpret_cast<FcMap*>(m)->mps.at(mp).get();
    out7[0] = p->mbTrackInView ? 1 : 0; out7[1] = p->mTrackProjX; out7[2] = p->mTrackProjY; out7[3] = p->mnTrackScaleLevel;
    out7[4] = p->mTrackViewCos; out7[5] = p->mnVisible; out7[6] = (double)p->mnLastFrameSeen;
    return 0;
}
// ORBmatcher(0.9, check_ori).SearchByProjection(CurrentFrame, LastFrame, th, bMono)
int fc_search_by_projection_last(void* m, long cur, long last, float th, int mono, int check_ori) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    ORBmatcher matcher(0.9, check_ori != 0);
    return matcher.SearchByProjection(*M->frames.at(cur), *M->frames.at(last), th, mono != 0);
}
// ORBmatcher(nnratio).SearchByProjection(F, vpMapPoints, th); an id of -1 is a NULL entry
int fc_search_by_projection_map(void* m, long frame, const long* mp_ids, int n, float th, float nnratio) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    ORBmatcher matcher(nnratio);
    return matcher.SearchByProjection(*M->frames.at(frame), point_list(M, mp_ids, n), th);
}
// Tracking::SearchLocalPoints with mCurrentFrame = the frame (copied in and back out) and mvpLocalMapPoints = the list
int fc_search_local_points(void* m, long frame, const long* mp_ids, int n, long last_reloc_frame_id) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    Tracking t;
    t.mCurrentFrame = *M->frames.at(frame);
    t.mvpLocalMapPoints = point_list(M, mp_ids, n);
    t.mnLastRelocFrameId = (long unsigned)last_reloc_frame_id;
    const int r = t.SearchLocalPoints();
    *M->frames.at(frame) = t.mCurrentFrame;
    return r;
}
// the matching half of Tracking::TrackWithMotionModel
int fc_track_motion_model_matches(void* m, long cur, long last) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    Tracking t;
    t.mCurrentFrame = *M->frames.at(cur);
    t.mLastFrame = *M->frames.at(last);
    const int r = t.TrackWithMotionModelMatches();
    *M->frames.at(cur) = t.mCurrentFrame;
    return r;
}
// ---- bag-of-words matching (both ORBmatcher::SearchByBoW overloads, their batch forms, the Tracking slice) ----
// what SearchByBoW reads of a frame beside the keypoints fc_frame_add_obs gave it: N x 32 descriptor bytes, one angle per keypoint
// (mvKeys = mvKeysUn), the feature vector in CSR form (node ids ascending); N becomes the number of keypoints the frame holds
int fc_frame_set_bow_data(void* m, long frame, const unsigned char* desc, const float* angle, int n_nodes, const unsigned int* node_id, const int* node_begin,
                          const int* node_feat) {
    Frame* f = reinterpret_cast<FcMap*>(m)->frames.at(frame).get();
    f->N = (int)f->mvKeysUn.size();
    f->mDescriptors.assign(desc, desc + 32 * (size_t)f->N);
    for (int i = 0; i < f->N; i++) f->mvKeysUn[(size_t)i].angle = angle[i];
    f->mvKeys = f->mvKeysUn;
    f->mFeatVec.clear();
    for (int j = 0; j < n_nodes; j++) {
        std::vector<unsigned int>& v = f->mFeatVec[node_id[j]];
        for (int i = node_begin[j]; i < node_begin[j + 1]; i++) v.push_back((unsigned int)node_feat[i]);
    }
    return f->N;
}
int fc_mp_set_bad(void* m, long mp, int bad) {
    reinterpret_cast<FcMap*>(m)->mps.at(mp)->mbBad = bad != 0;
    return 0;
}
static void ids_of(const std::vector<MapPoint*>& v, long* ids, int cap) {
    for (size_t i = 0; i < v.size() && (int)i < cap; i++) ids[i] = v[i] ? (long)v[i]->mnId : -1;
}
// ORBmatcher(nnratio, check_ori).SearchByBoW(pKF, F, vpMapPointMatches): match_ids [cap] comes back with the ids (-1: NULL)
int fc_search_by_bow_frame(void* m, long kf, long frame, float nnratio, int check_ori, long* match_ids, int cap) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    ORBmatcher matcher(nnratio, check_ori != 0);
    std::vector<MapPoint*> v;
    const int r = matcher.SearchByBoW(M->kfs.at(kf).get(), *M->frames.at(frame), v);
    ids_of(v, match_ids, cap);
    return r;
}
// ORBmatcher(nnratio, check_ori).SearchByBoW(pKF1, pKF2, vpMatches12)
int fc_search_by_bow_kf(void* m, long kf1, long kf2, float nnratio, int check_ori, long* match_ids, int cap) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    ORBmatcher matcher(nnratio, check_ori != 0);
    std::vector<MapPoint*> v;
    const int r = matcher.SearchByBoW(M->kfs.at(kf1).get(), M->kfs.at(kf2).get(), v);
    ids_of(v, match_ids, cap);
    return r;
}
// the batch forms: n keyframes against one frame (frame >= 0) or keyframe kf1 against n keyframes; match_ids [n][stride], n_matches [n]
int fc_search_by_bow_batch(void* m, long kf1, long frame, const long* kfs, int n, float nnratio, int check_ori, long* match_ids, int stride, int* n_matches) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    ORBmatcher matcher(nnratio, check_ori != 0);
    std::vector<KeyFrame*> v;
    for (int i = 0; i < n; i++) v.push_back(M->kfs.at(kfs[i]).get());
    std::vector<std::vector<MapPoint*>> vv;
    std::vector<int> vn;
    const int r = frame >= 0 ? matcher.SearchByBoW(v, *M->frames.at(frame), vv, vn) : matcher.SearchByBoW(M->kfs.at(kf1).get(), v, vv, vn);
    for (size_t i = 0; i < vv.size(); i++) {
        ids_of(vv[i], match_ids + i * (size_t)stride, stride);
        n_matches[i] = vn[i];
    }
    return r;
}
// the matching half of Tracking::TrackReferenceKeyFrame with mpReferenceKF = kf, mCurrentFrame = cur (copied in and back out) and
// mLastFrame = last
int fc_track_reference_kf_matches(void* m, long kf, long cur, long last) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    Tracking t;
    t.mpReferenceKF = M->kfs.at(kf).get();
    t.mCurrentFrame = *M->frames.at(cur);
    t.mLastFrame = *M->frames.at(last);
    const int r = t.TrackReferenceKeyFrameMatches();
    *M->frames.at(cur) = t.mCurrentFrame;
    return r;
}
// ---- Sim3 projection matching (ORBmatcher::SearchBySim3) ----
// ORBmatcher::SearchBySim3(pKF1, pKF2, vpMatches12, s12, R12, t12, th): match_ids [n] holds the ids of vpMatches12 (-1: NULL) and
// comes back with those after the call
int fc_search_by_sim3(void* m, long kf1, long kf2, long* match_ids, int n, float s12, const float* R9, const float* t3, float th) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::vector<MapPoint*> v = point_list(M, match_ids, n);
    Mat3f R; std::memcpy(R.data(), R9, 36);
    const std::array<float, 3> t = {{t3[0], t3[1], t3[2]}};
    ORBmatcher matcher;
    const int r = matcher.SearchBySim3(M->kfs.at(kf1).get(), M->kfs.at(kf2).get(), v, s12, R, t, th);
    for (int i = 0; i < n; i++) match_ids[i] = v[(size_t)i] ? (long)v[(size_t)i]->mnId : -1;
    return r;
}
// the vbAlreadyMatched flags of src/ORBmatcher.cpp:1287-1301 (no GPU needed): flags1 [N1], flags2 [N2]
int fc_search_by_sim3_flags(void* m, long kf1, long kf2, const long* match_ids, int n, unsigned char* flags1, unsigned char* flags2) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    std::vector<uint8_t> vb1, vb2;
    ORBmatcher::AlreadyMatched(M->kfs.at(kf1).get(), M->kfs.at(kf2).get(), point_list(M, match_ids, n), vb1, vb2);
    std::memcpy(flags1, vb1.data(), vb1.size());
    std::memcpy(flags2, vb2.data(), vb2.size());
    return (int)vb1.size();
}
// ---- essential graph ----
// spanning tree, loop edges and the ordered covisibility list (descending weights) of one keyframe
int fc_kf_set_graph(void* m, long kf, long parent, const long* children, int n_children, const long* loop_edges, int n_loop,
                    const long* cov_ids, const int* cov_w, int n_cov) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    KeyFrame* k = M->kfs.at(kf).get();
    k->mpParent = parent >= 0 ? M->kfs.at(parent).get() : nullptr;
    k->mspChildrens.clear(); k->mspLoopEdges.clear();
    k->mvpOrderedConnectedKeyFrames.clear(); k->mvOrderedWeights.clear(); k->mConnectedKeyFrameWeights.clear();
    for (int i = 0; i < n_children; i++) k->mspChildrens.insert(M->kfs.at(children[i]).get());
    for (int i = 0; i < n_loop; i++) k->mspLoopEdges.insert(M->kfs.at(loop_edges[i]).get());
    for (int i = 0; i < n_cov; i++) {
        KeyFrame* o = M->kfs.at(cov_ids[i]).get();
        k->mvpOrderedConnectedKeyFrames.push_back(o);
        k->mvOrderedWeights.push_back(cov_w[i]);
        k->mConnectedKeyFrameWeights[o] = cov_w[i];
    }
    return 0;
}
int fc_set_kf_bad(void* m, long kf, int bad) {
    reinterpret_cast<FcMap*>(m)->kfs.at(kf)->mbBad = bad != 0;
    return 0;
}
int fc_mappoint_set_corrected(void* m, long mp, long by_kf, long reference) {
    MapPoint* p = reinterpret_cast<FcMap*>(m)->mps.at(mp).get();
    p->mnCorrectedByKF = (long unsigned)by_kf;
    p->mnCorrectedReference = (long unsigned)reference;
    return 0;
}
// Optimizer::OptimizeEssentialGraph(map, loop_kf, cur_kf, NonCorrectedSim3, CorrectedSim3, LoopConnections, bFixScale, &lc).
// nonc / corr: keyframe ids with their Sim3 (t, q xyzw, s each); conn: pairs (keyframe, connected keyframe).  mode 1: extraction
// only (no GPU needed).  Returns the number of vertices packed.
int fc_optimize_essential_graph(void* m, long loop_kf, long cur_kf, const long* nonc_ids, const double* nonc_S, int n_nonc,
                                const long* corr_ids, const double* corr_S, int n_corr, const long* conn, int n_conn, int fix_scale, int mode) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    fill_map(M);
    M->map.mnMaxKFid = 0;
    for (auto& k : M->kfs) M->map.mnMaxKFid = std::max(M->map.mnMaxKFid, k.second->mnId);
    auto sim3 = [](const double* a) { return g2o::Sim3({{a[3], a[4], a[5], a[6]}}, {{a[0], a[1], a[2]}}, a[7]); };
    LoopClosing::KeyFrameAndPose NonCorrected, Corrected;
    for (int i = 0; i < n_nonc; i++) NonCorrected[M->kfs.at(nonc_ids[i]).get()] = sim3(nonc_S + 8 * i);
    for (int i = 0; i < n_corr; i++) Corrected[M->kfs.at(corr_ids[i]).get()] = sim3(corr_S + 8 * i);
    std::map<KeyFrame*, std::set<KeyFrame*>> LoopConnections;
    for (int i = 0; i < n_conn; i++) LoopConnections[M->kfs.at(conn[2 * i]).get()].insert(M->kfs.at(conn[2 * i + 1]).get());
    KeyFrame *pLoop = M->kfs.at(loop_kf).get(), *pCur = M->kfs.at(cur_kf).get();
    if (mode == 1) Optimizer::PackEssentialGraph(&M->map, pLoop, pCur, NonCorrected, Corrected, LoopConnections, fix_scale != 0, Optimizer::LastPoseGraph());
    else Optimizer::OptimizeEssentialGraph(&M->map, pLoop, pCur, NonCorrected, Corrected, LoopConnections, fix_scale != 0, &M->lc);
    return (int)Optimizer::LastPoseGraph().vKF.size();
}
const vba_posegraph_problem* fc_last_posegraph() { return &Optimizer::LastPoseGraph().P; }
const vba_posegraph_result* fc_last_posegraph_result() { return &Optimizer::LastPoseGraph().R; }
int fc_last_posegraph_ids(long* kf_ids, int cap_kf, long* mp_ids, int cap_mp) {   // mnId behind every vertex and every point row
    const PackedPoseGraph& G = Optimizer::LastPoseGraph();
    for (size_t i = 0; i < G.vKF.size() && (int)i < cap_kf; i++) kf_ids[i] = (long)G.vKF[i]->mnId;
    for (size_t i = 0; i < G.vMP.size() && (int)i < cap_mp; i++) mp_ids[i] = (long)G.vMP[i]->mnId;
    return (int)G.vMP.size();
}
// ---- projection matching for loop closure and relocalisation (the two other ORBmatcher::SearchByProjection overloads, LoopClosing) ----
// ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th): matched_ids [n_matched] holds the ids of vpMatched going in and
// coming back (-1: NULL)
int fc_search_by_projection_loop(void* m, long kf, const float* Scw16, const long* mp_ids, int n, long* matched_ids, int n_matched, int th) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    Mat4f S; std::memcpy(S.data(), Scw16, 64);
    std::vector<MapPoint*> matched = point_list(M, matched_ids, n_matched);
    ORBmatcher matcher(0.75, true);
    const int r = matcher.SearchByProjection(M->kfs.at(kf).get(), S, point_list(M, mp_ids, n), matched, th);
    ids_of(matched, matched_ids, n_matched);
    return r;
}
// ORBmatcher(0.9, check_ori).SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist); the frame's points: fc_frame_points
int fc_search_by_projection_reloc(void* m, long frame, long kf, const long* found_ids, int n_found, float th, int orb_dist, int check_ori) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    const std::vector<MapPoint*> found = point_list(M, found_ids, n_found);
    ORBmatcher matcher(0.9, check_ori != 0);
    return matcher.SearchByProjection(*M->frames.at(frame), M->kfs.at(kf).get(), std::set<MapPoint*>(found.begin(), found.end()), th, orb_dist);
}
// the keypoint angles of a keyframe (what the relocalisation overload reads of pKF beside its map points)
int fc_kf_set_angles(void* m, long kf, const float* angle, int n) {
    KeyFrame* k = reinterpret_cast<FcMap*>(m)->kfs.at(kf).get();
    for (int i = 0; i < n && i < (int)k->mvKeysUn.size(); i++) k->mvKeysUn[(size_t)i].angle = angle[i];
    return (int)k->mvKeysUn.size();
}
// LoopClosing::MatchLoopMapPoints with mpCurrentKF, mpMatchedKF, mScw and mvpCurrentMatchedPoints (ids, -1: NULL) as given; matched_ids
// comes back as the call left mvpCurrentMatchedPoints, loop_ids [cap] with the ids of mvpLoopMapPoints.  out3: the decision,
// nTotalMatches, the size of mvpLoopMapPoints
int fc_match_loop_map_points(void* m, long cur, long matched_kf, const float* Scw16, long* matched_ids, int n_matched, long* loop_ids, int cap, int* out3) {
    FcMap* M = reinterpret_cast<FcMap*>(m);
    LoopClosing& lc = M->lc;
    lc.mpCurrentKF = M->kfs.at(cur).get();
    lc.mpMatchedKF = M->kfs.at(matched_kf).get();
    std::memcpy(lc.mScw.data(), Scw16, 64);
    lc.mvpCurrentMatchedPoints = point_list(M, matched_ids, n_matched);
    out3[0] = lc.MatchLoopMapPoints() ? 1 : 0;
    out3[1] = lc.mnLoopTotalMatches;
    out3[2] = (int)lc.mvpLoopMapPoints.size();
    ids_of(lc.mvpCurrentMatchedPoints, matched_ids, n_matched);
    ids_of(lc.mvpLoopMapPoints, loop_ids, cap);
    return 0;
}
int fc_loop_map_updated(void* m) { return reinterpret_cast<FcMap*>(m)->lc.mbMapUpdateFlagForTracking ? 1 : 0; }
int fc_map_updated(void* m) { return reinterpret_cast<FcMap*>(m)->lm.mbMapUpdateFlagForTracking ? 1 : 0; }
// last packed window (what the facade handed / would hand to vba_solve)
const vba_problem* fc_last_problem() { return &Optimizer::LastWindow().P; }
int fc_last_mp_ids(long* out, int cap) {  // mnId of the MapPoint behind every landmark row of the last window
    const PackedWindow& W = Optimizer::LastWindow();
    const int n = (int)W.vMP.size();
    for (int i = 0; i < n && i < cap; i++) out[i] = (long)W.vMP[i]->mnId;
    return n;
}
int fc_last_kf_ids(long* out, int cap) {
    const PackedWindow& W = Optimizer::LastWindow();
    const int n = (int)W.vKF.size();
    for (int i = 0; i < n && i < cap; i++) out[i] = (long)W.vKF[i]->mnId;
    return n;
}
const vba_result* fc_last_result() { return &Optimizer::LastWindow().R; }

}  // extern "C"
