// orbslam_min.h -- the slice of the reference's host data model that Optimizer::LocalBAPRVIDP /
// LocalBundleAdjustment read and write (SURVEY.md section 8b lists the surface).  Same class, member and
// method names as mc275/MC_SLAM (include/KeyFrame.h, include/MapPoint.h, src/IMU/NavState.h,
// src/IMU/IMUPreintegrator.h, src/IMU/configparam.h, src/IMU/imudata.h), minus OpenCV / Eigen (absent from
// this image): cv::Mat poses become float[16] row-major (they ARE float32 in the reference, CV_32F),
// Eigen vectors become small POD arrays.  It exists so that the facade in Optimizer.cpp compiles against the
// interface it is meant to drop into, and so that tests can drive it; it is not a SLAM system.
#pragma once
#include <array>
#include <cmath>
#include <algorithm>
#include <cstddef>
#include <functional>
#include <list>
#include <map>
#include <mutex>
#include <set>
#include <utility>
#include <vector>

namespace ORB_SLAM2 {

typedef std::array<double, 3> Vector3d;
typedef std::array<double, 4> Quaterniond;  // x y z w (Eigen coefficient order)
typedef std::array<double, 9> Matrix3d;     // row-major
typedef std::array<float, 16> Mat4f;        // cv::Mat CV_32F 4x4, row-major
typedef std::array<float, 9> Mat3f;         // cv::Mat CV_32F 3x3, row-major

inline Matrix3d QuatToMatrix(const Quaterniond& q) {  // Eigen::Quaterniond::toRotationMatrix
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    return {1 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1 - (txx + tzz), tyz - twx, txz - twy, tyz + twx, 1 - (txx + tyy)};
}

// src/IMU/NavState.h:124-138
class NavState {
public:
    Vector3d Get_P() const { return _P; }
    Vector3d Get_V() const { return _V; }
    Quaterniond Get_R() const { return _R; }  // Sophus::SO3 (unit quaternion storage)
    Matrix3d Get_RotMatrix() const { return QuatToMatrix(_R); }
    Vector3d Get_BiasGyr() const { return _BiasGyr; }
    Vector3d Get_BiasAcc() const { return _BiasAcc; }
    Vector3d Get_dBias_Gyr() const { return _dBias_g; }
    Vector3d Get_dBias_Acc() const { return _dBias_a; }
    void Set_Pos(const Vector3d& v) { _P = v; }
    void Set_Vel(const Vector3d& v) { _V = v; }
    void Set_Rot(const Quaterniond& q) { _R = q; }
    void Set_BiasGyr(const Vector3d& v) { _BiasGyr = v; }
    void Set_BiasAcc(const Vector3d& v) { _BiasAcc = v; }
    void Set_DeltaBiasGyr(const Vector3d& v) { _dBias_g = v; }
    void Set_DeltaBiasAcc(const Vector3d& v) { _dBias_a = v; }

private:
    Vector3d _P{{0, 0, 0}}, _V{{0, 0, 0}};
    Quaterniond _R{{0, 0, 0, 1}};
    Vector3d _BiasGyr{{0, 0, 0}}, _BiasAcc{{0, 0, 0}}, _dBias_g{{0, 0, 0}}, _dBias_a{{0, 0, 0}};
};

// src/IMU/IMUPreintegrator.h:179-195
class IMUPreintegrator {
public:
    double getDeltaTime() const { return _delta_time; }
    const Vector3d& getDeltaP() const { return _delta_P; }
    const Vector3d& getDeltaV() const { return _delta_V; }
    const Matrix3d& getDeltaR() const { return _delta_R; }
    const Matrix3d& getJPBiasg() const { return _J_P_Biasg; }
    const Matrix3d& getJPBiasa() const { return _J_P_Biasa; }
    const Matrix3d& getJVBiasg() const { return _J_V_Biasg; }
    const Matrix3d& getJVBiasa() const { return _J_V_Biasa; }
    const Matrix3d& getJRBiasg() const { return _J_R_Biasg; }
    const std::array<double, 81>& getCovPVPhi() const { return _cov_P_V_Phi; }
    double _delta_time = 0;
    Vector3d _delta_P{{0, 0, 0}}, _delta_V{{0, 0, 0}};
    Matrix3d _delta_R{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
    Matrix3d _J_P_Biasg{}, _J_P_Biasa{}, _J_V_Biasg{}, _J_V_Biasa{}, _J_R_Biasg{};
    std::array<double, 81> _cov_P_V_Phi{};
};

// src/IMU/imudata.cpp:25-26
struct IMUData {
    static double getGyrBiasRW2() { return 2.0e-5 * 2.0e-5; }
    static double getAccBiasRW2() { return 5.0e-3 * 5.0e-3; }
};

// src/IMU/configparam.cpp:55-71 (T_bc from the settings file, rotation re-normalised; T_cb = T_bc^-1)
struct ConfigParam {
    static Matrix3d& Rbc() { static Matrix3d R{{1, 0, 0, 0, 1, 0, 0, 0, 1}}; return R; }
    static Vector3d& Pbc() { static Vector3d p{{0, 0, 0}}; return p; }
    static void SetTbc(const Matrix3d& R, const Vector3d& p) { Rbc() = R; Pbc() = p; }
    static void GetEigT_cb(Matrix3d& Rcb, Vector3d& tcb) {
        const Matrix3d& R = Rbc();
        const Vector3d& p = Pbc();
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) Rcb[3 * i + j] = R[3 * j + i];
        for (int i = 0; i < 3; i++) tcb[i] = -(Rcb[3 * i] * p[0] + Rcb[3 * i + 1] * p[1] + Rcb[3 * i + 2] * p[2]);
    }
};

struct KeyPoint {  // cv::KeyPoint: pt.x, pt.y are float, octave int, angle float (degrees in [0, 360))
    struct { float x, y; } pt;
    int octave;
    float angle = 0.0f;   // what ORBmatcher::SearchForTriangulation reads (src/ORBmatcher.cpp:898)
};

class KeyFrame;
class MapPoint;

// src/MapPoint.cpp:19-22
struct cmpKeyFrameId {
    bool operator()(const KeyFrame* a, const KeyFrame* b) const;
};
typedef std::map<KeyFrame*, size_t, cmpKeyFrameId> mapMapPointObs;

class Map {
public:
    std::mutex mMutexMapUpdate;  // include/Map.h:72
    std::vector<KeyFrame*> GetAllKeyFrames() { return mspKeyFrames; }    // include/Map.h:44 (a std::set there: id order)
    std::vector<MapPoint*> GetAllMapPoints() { return mspMapPoints; }    // include/Map.h:45
    long unsigned int GetMaxKFid() { return mnMaxKFid; }                 // include/Map.h:50
    void AddMapPoint(MapPoint* pMP) { mspMapPoints.push_back(pMP); }     // src/Map.cpp (a std::set there)
    void EraseMapPoint(MapPoint* pMP) {                                  // src/Map.cpp: the point leaves the set, it is not deleted
        mspMapPoints.erase(std::remove(mspMapPoints.begin(), mspMapPoints.end(), pMP), mspMapPoints.end());
    }
    long unsigned int mnMaxKFid = 0;
    std::vector<KeyFrame*> mspKeyFrames;
    std::vector<MapPoint*> mspMapPoints;
};

// ORBmatcher::SearchForTriangulation stays matcher code: CreateNewMapPoints calls it per neighbour, in order, through this function
// object (keyframe 1, keyframe 2, the matched keypoint indices to fill)
typedef std::function<void(KeyFrame*, KeyFrame*, std::vector<std::pair<size_t, size_t>>&)> TriangulationMatcher;

class LocalMapping {
public:
    void SetMapUpdateFlagInTracking(bool b) { mbMapUpdateFlagForTracking = b; }
    bool mbMapUpdateFlagForTracking = false;
    // src/LocalMapping.cpp:1237-1546 for a monocular pKF (= mpCurrentKeyFrame) and the neighbours the caller chose (:1243-1251): the
    // baseline / median-depth gate, the matcher and one vba_triangulate call per neighbour, then the map-point construction of
    // :1520-1542 for every accepted match (LocalMapping.cpp).  Returns nnew, -1 when the backend failed
    int CreateNewMapPoints(KeyFrame* pKF, const std::vector<KeyFrame*>& vpNeighKFs, const TriangulationMatcher& matcher, Map* pMap,
                           std::list<MapPoint*>& lpRecentAddedMapPoints);
    // the same with the reference's own matcher call (:1314-1318): ComputeF12, then ORBmatcher(0.6, false)::SearchForTriangulation
    // over vba_search_triangulation (ORBmatcher.cpp), so the function runs on its own.  A matcher or backend failure ends the walk at
    // that neighbour with -1; the points made from the neighbours in front of it stay in the map
    int CreateNewMapPoints(KeyFrame* pKF, const std::vector<KeyFrame*>& vpNeighKFs, Map* pMap, std::list<MapPoint*>& lpRecentAddedMapPoints);
    // src/LocalMapping.cpp:1659-1680: K1^-T [t12]x R12 K2^-1 with analytic K inverses, FP64 products, the result held as float32
    static Mat3f ComputeF12(KeyFrame* pKF1, KeyFrame* pKF2);
    // src/LocalMapping.cpp:1588-1632, steps 2 and 3 of SearchInNeighbors for pKF (= mpCurrentKeyFrame) and the target keyframes the
    // caller chose (step 1, :1554-1582): ORBmatcher::Fuse of pKF's map points into every target, then of the targets' map points
    // into pKF, one vba_fuse call per Fuse call, in order (LocalMapping.cpp).  Returns the fused points of all calls, -1 when the
    // backend failed (the Fuse calls in front of the failing one stay applied)
    int SearchInNeighbors(KeyFrame* pKF, const std::vector<KeyFrame*>& vpTargetKFs);
    // src/LocalMapping.cpp:1144-1171, the map-point loop of ProcessNewKeyFrame for pKF (= mpCurrentKeyFrame): a good point that pKF does
    // not observe yet gets its AddObservation, in keypoint order, a point already in the keyframe goes to the recent list; then the
    // UpdateNormalAndDepth / ComputeDistinctiveDescriptors pairs of the new observers as ONE vba_mappoint_update call
    // (MapPointUpdate.cpp).  Returns the points refreshed, -1 when the backend failed (the observations stay added)
    int ProcessNewKeyFramePoints(KeyFrame* pKF, std::list<MapPoint*>& lpRecentAddedMapPoints);
    // src/LocalMapping.cpp:1635-1650, the end of SearchInNeighbors: both refreshes for every good map point of pKF, ONE call.  Returns
    // the points refreshed, -1 when the backend failed
    int UpdateCurrentKeyFramePoints(KeyFrame* pKF);
};

class KeyFrame {
public:
    long unsigned int mnId = 0;
    static long unsigned int nNextId;
    long unsigned int mnBALocalForKF = (long unsigned int)-1, mnBAFixedForKF = (long unsigned int)-1;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;          // negative for monocular points
    std::vector<float> mvInvLevelSigma2;
    std::vector<float> mvLevelSigma2;     // include/KeyFrame.h: what Sim3Solver reads (src/Sim3Solver.cpp:75-76)
    std::vector<float> mvScaleFactors;    // include/KeyFrame.h: what CreateNewMapPoints reads (src/LocalMapping.cpp:1513)
    // what ORBmatcher::SearchForTriangulation reads (src/ORBmatcher.cpp:763-764, :831): N keypoints, N x 32 descriptor bytes (the
    // rows of the cv::Mat), the DBoW2::FeatureVector as node id -> keypoint indices
    int N = 0;
    std::vector<unsigned char> mDescriptors;
    std::map<unsigned int, std::vector<unsigned int>> mFeatVec;
    float mfScaleFactor = 1.2f;           // src/LocalMapping.cpp:1272

    std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
    KeyFrame* GetPrevKeyFrame() { return mpPrevKeyFrame; }
    const NavState& GetNavState() { return mNavState; }
    void SetNavState(const NavState& ns) { mNavState = ns; }
    const IMUPreintegrator& GetIMUPreInt() { return mIMUPreInt; }
    bool isBad() { return mbBad; }
    // float32 camera pose T_cw, kept in sync by UpdatePoseFromNS / SetPose (src/KeyFrame.cpp:96-114)
    const Mat4f& GetPose() const { return Tcw; }
    void SetPose(const Mat4f& T) { Tcw = T; }
    void GetRotation(double R[9]) const { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R[3 * i + j] = Tcw[4 * i + j]; }
    void GetTranslation(double t[3]) const { for (int i = 0; i < 3; i++) t[i] = Tcw[4 * i + 3]; }
    void GetCameraCenter(double c[3]) const {  // -R^T t in float32 arithmetic like cv::Mat (KeyFrame::SetPose)
        for (int i = 0; i < 3; i++) {
            float s = 0;
            for (int k = 0; k < 3; k++) s += Tcw[4 * k + i] * Tcw[4 * k + 3];
            c[i] = -s;
        }
    }
    void SetNavStatePos(const Vector3d& v) { mNavState.Set_Pos(v); }
    void SetNavStateRot(const Quaterniond& q) { mNavState.Set_Rot(q); }
    void SetNavStateVel(const Vector3d& v) { mNavState.Set_Vel(v); }
    void SetNavStateDeltaBg(const Vector3d& v) { mNavState.Set_DeltaBiasGyr(v); }
    void SetNavStateDeltaBa(const Vector3d& v) { mNavState.Set_DeltaBiasAcc(v); }
    void UpdatePoseFromNS() {  // src/KeyFrame.cpp:96-114 with ConfigParam::GetMatTbc(), float32 like cv::Mat
        const Matrix3d Rwb = mNavState.Get_RotMatrix();
        const Vector3d Pwb = mNavState.Get_P();
        float Rwbf[9], Rbcf[9], Pbcf[3], Pwbf[3];
        for (int i = 0; i < 9; i++) { Rwbf[i] = (float)Rwb[i]; Rbcf[i] = (float)ConfigParam::Rbc()[i]; }
        for (int i = 0; i < 3; i++) { Pbcf[i] = (float)ConfigParam::Pbc()[i]; Pwbf[i] = (float)Pwb[i]; }
        float Rwc[9], Pwc[3];
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) {
                float s = 0;
                for (int k = 0; k < 3; k++) s += Rwbf[3 * i + k] * Rbcf[3 * k + j];
                Rwc[3 * i + j] = s;
            }
            float s = 0;
            for (int k = 0; k < 3; k++) s += Rwbf[3 * i + k] * Pbcf[k];
            Pwc[i] = s + Pwbf[i];
        }
        Mat4f T{};
        for (int i = 0; i < 3; i++) {
            float s = 0;
            for (int j = 0; j < 3; j++) { T[4 * i + j] = Rwc[3 * j + i]; s += Rwc[3 * j + i] * Pwc[j]; }
            T[4 * i + 3] = -s;
        }
        T[15] = 1.0f;
        SetPose(T);
    }
    void AddMapPoint(MapPoint* pMP, const size_t& idx) { mvpMapPoints[idx] = pMP; }   // src/KeyFrame.cpp
    // what ORBmatcher::Fuse reads and writes (include/KeyFrame.h:240-245, :289-300, :322; src/KeyFrame.cpp:560-610, :1119-1122)
    int mnGridCols = 64, mnGridRows = 48;                                 // FRAME_GRID_COLS, FRAME_GRID_ROWS
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    int mnMinX = 0, mnMinY = 0, mnMaxX = 0, mnMaxY = 0;
    int mnScaleLevels = 8;
    float mfLogScaleFactor = std::log(1.2f);
    std::vector<std::vector<std::vector<size_t>>> mGrid;                  // [col][row] keypoint indices
    long unsigned int mnFuseTargetForKF = 0;
    bool IsInImage(const float& x, const float& y) const { return (x >= mnMinX && x < mnMaxX && y >= mnMinY && y < mnMaxY); }
    MapPoint* GetMapPoint(const size_t& idx) { return mvpMapPoints[idx]; }
    void ReplaceMapPointMatch(const size_t& idx, MapPoint* pMP) { mvpMapPoints[idx] = pMP; }
    void EraseMapPointMatch(const size_t& idx) { mvpMapPoints[idx] = nullptr; }
    std::set<MapPoint*> GetMapPoints();   // the points that are neither NULL nor bad (below MapPoint)
    // Frame::AssignFeaturesToGrid with PosInGrid (src/Frame.cpp): round() of the float32 cell coordinate, a keypoint outside the grid
    // is in no cell
    void AssignFeaturesToGrid() {
        mfGridElementWidthInv = (float)mnGridCols / (float)(mnMaxX - mnMinX);
        mfGridElementHeightInv = (float)mnGridRows / (float)(mnMaxY - mnMinY);
        mGrid.assign((size_t)mnGridCols, std::vector<std::vector<size_t>>((size_t)mnGridRows));
        for (size_t i = 0; i < mvKeysUn.size(); i++) {
            const int posX = (int)std::round((mvKeysUn[i].pt.x - mnMinX) * mfGridElementWidthInv);
            const int posY = (int)std::round((mvKeysUn[i].pt.y - mnMinY) * mfGridElementHeightInv);
            if (posX < 0 || posX >= mnGridCols || posY < 0 || posY >= mnGridRows) continue;
            mGrid[(size_t)posX][(size_t)posY].push_back(i);
        }
    }
    // src/KeyFrame.cpp:1163-1195 in float32 like cv::Mat (below MapPoint).  Without a single map point the reference indexes an empty
    // vector; here that case returns -1 (every baseline ratio is then below the gate of CreateNewMapPoints)
    float ComputeSceneMedianDepth(const int q);
    void EraseMapPointMatch(MapPoint* pMP);   // src/KeyFrame.cpp:573-579: through pMP->GetIndexInKeyFrame(this) (below MapPoint)
    std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() { return mvpOrderedConnectedKeyFrames; }
    // spanning tree, loop edges and covisibility weights: what OptimizeEssentialGraph reads (include/KeyFrame.h:104-128)
    KeyFrame* GetParent() { return mpParent; }
    bool hasChild(KeyFrame* pKF) { return mspChildrens.count(pKF) != 0; }
    std::set<KeyFrame*> GetLoopEdges() { return mspLoopEdges; }
    int GetWeight(KeyFrame* pKF) {                                        // src/KeyFrame.cpp:548-555
        const auto it = mConnectedKeyFrameWeights.find(pKF);
        return it == mConnectedKeyFrameWeights.end() ? 0 : it->second;
    }
    // src/KeyFrame.cpp:525-544 as it stands: upper_bound over the descending weights; when EVERY connected keyframe has at least
    // weight w the iterator is end() and the reference returns an empty vector
    std::vector<KeyFrame*> GetCovisiblesByWeight(const int& w) {
        if (mvpOrderedConnectedKeyFrames.empty()) return std::vector<KeyFrame*>();
        size_t n = 0;
        while (n < mvOrderedWeights.size() && !(w > mvOrderedWeights[n])) n++;
        if (n == mvOrderedWeights.size()) return std::vector<KeyFrame*>();
        return std::vector<KeyFrame*>(mvpOrderedConnectedKeyFrames.begin(), mvpOrderedConnectedKeyFrames.begin() + n);
    }
    // src/KeyFrame.cpp:19-36: P, R and V of the NavState from a new T_cw (float32 matrices like cv::Mat; bV1 = bV2)
    void UpdateNavStatePVRFromTcw(const Mat4f& Tcw_, const Matrix3d& Rbc, const Vector3d& Pbc);

    // state (public here: the test harness fills it)
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<KeyFrame*> mvpOrderedConnectedKeyFrames;
    std::vector<int> mvOrderedWeights;                       // weights of mvpOrderedConnectedKeyFrames, descending
    std::map<KeyFrame*, int> mConnectedKeyFrameWeights;
    KeyFrame* mpParent = nullptr;
    std::set<KeyFrame*> mspChildrens, mspLoopEdges;
    KeyFrame* mpPrevKeyFrame = nullptr;
    NavState mNavState;
    IMUPreintegrator mIMUPreInt;
    bool mbBad = false;
    Mat4f Tcw{};
    // results of a global BA that runs while the map keeps growing (include/KeyFrame.h:180-186)
    NavState mNavStateGBA;
    Mat4f mTcwGBA{};
    long unsigned int mnBAGlobalForKF = 0;
};

class MapPoint {
public:
    MapPoint() {}
    // MapPoint(const cv::Mat& Pos, KeyFrame* pRefKF, Map* pMap) (src/MapPoint.cpp): the position, the reference keyframe, the next id
    MapPoint(const float Pos[3], KeyFrame* pRefKF) : mnId(nNextId++), mpRefKF(pRefKF) { SetWorldPos(Pos); }
    long unsigned int mnId = 0;
    static long unsigned int nNextId;
    long unsigned int mnBALocalForKF = (long unsigned int)-1;
    long unsigned int mnCorrectedByKF = 0, mnCorrectedReference = 0;      // include/MapPoint.h:86-87 (LoopClosing::CorrectLoop)
    bool isBad() { return mbBad; }
    void GetWorldPos(double P[3]) const { for (int i = 0; i < 3; i++) P[i] = mWorldPos[i]; }  // float32 -> double (Converter::toVector3d)
    void SetWorldPos(const float P[3]) { for (int i = 0; i < 3; i++) mWorldPos[i] = P[i]; }
    mapMapPointObs GetObservations() { return mObservations; }
    KeyFrame* GetReferenceKeyFrame() { return mpRefKF; }
    void EraseObservation(KeyFrame* pKF) { mObservations.erase(pKF); }
    void AddObservation(KeyFrame* pKF, size_t idx) {   // src/MapPoint.cpp (monocular: nObs grows by one)
        if (mObservations.count(pKF)) return;
        mObservations[pKF] = idx;
        nObs++;
    }
    int GetIndexInKeyFrame(KeyFrame* pKF) {   // src/MapPoint.cpp: the keypoint index of this point in pKF, -1 if pKF does not observe it
        const auto it = mObservations.find(pKF);
        return it == mObservations.end() ? -1 : (int)it->second;
    }
    void UpdateNormalAndDepth() { ++nNormalUpdates; }  // bookkeeping of the map, out of scope
    // what ORBmatcher::Fuse reads and writes (src/MapPoint.cpp)
    void GetNormal(double n[3]) const { for (int i = 0; i < 3; i++) n[i] = mNormalVector[i]; }
    float GetMinDistanceInvariance() const { return 0.8f * mfMinDistance; }
    float GetMaxDistanceInvariance() const { return 1.2f * mfMaxDistance; }
    const unsigned char* GetDescriptor() const { return mDescriptor; }
    bool IsInKeyFrame(KeyFrame* pKF) { return mObservations.count(pKF) != 0; }
    int Observations() { return nObs; }
    MapPoint* GetReplaced() { return mpReplaced; }
    void IncreaseVisible(int n = 1) { mnVisible += n; }
    void IncreaseFound(int n = 1) { mnFound += n; }
    void ComputeDistinctiveDescriptors() { ++nDescriptorUpdates; }   // a counter, like UpdateNormalAndDepth
    void Replace(MapPoint* pMP);                                      // src/MapPoint.cpp:245-292 (below)

    mapMapPointObs mObservations;
    KeyFrame* mpRefKF = nullptr;
    float mWorldPos[3] = {0, 0, 0};
    bool mbBad = false;
    int nNormalUpdates = 0;
    int nObs = 0;
    float mNormalVector[3] = {0, 0, 0};
    float mfMinDistance = 0, mfMaxDistance = 0;
    unsigned char mDescriptor[32] = {0};
    int mnVisible = 1, mnFound = 1;
    int nDescriptorUpdates = 0;
    long unsigned int mnFuseCandidateForKF = 0;   // include/MapPoint.h:149
    // what Frame::isInFrustum writes and ORBmatcher::SearchByProjection(F, vpMapPoints, th) reads (include/MapPoint.h:68-76), and the
    // mark of Tracking::SearchLocalPoints
    bool mbTrackInView = false;
    float mTrackProjX = 0, mTrackProjY = 0, mTrackViewCos = 0;
    int mnTrackScaleLevel = 0;
    long unsigned int mnLastFrameSeen = 0;
    MapPoint* mpReplaced = nullptr;
    Map* mpMap = nullptr;
    float mPosGBA[3] = {0, 0, 0};          // include/MapPoint.h:90-91
    long unsigned int mnBAGlobalForKF = 0;
    long unsigned int mnLoopPointForKF = 0;   // include/MapPoint.h:85: the mark of LoopClosing::ComputeSim3 (src/LoopClosing.cpp:455-459)
};

// include/Frame.h: the slice PoseOptimization reads and writes (:48-67, :104, :214, :230)
class Frame {
public:
    int N = 0;
    float fx = 0, fy = 0, cx = 0, cy = 0;
    std::vector<KeyPoint> mvKeysUn;
    std::vector<float> mvuRight;
    std::vector<float> mvInvLevelSigma2;
    std::vector<MapPoint*> mvpMapPoints;
    std::vector<bool> mvbOutlier;
    Mat4f mTcw{};
    std::array<double, 225> mMargCovInv{};   // Matrix<double,15,15>, row-major here
    NavState mNavStatePrior;
    const NavState& GetNavState() const { return mNavState; }
    void SetNavState(const NavState& ns) { mNavState = ns; }
    void SetPose(const Mat4f& T) { mTcw = T; }
    void UpdatePoseFromNS() {  // Frame::UpdatePoseFromNS(ConfigParam::GetMatTbc()): the same float32 chain as KeyFrame's
        KeyFrame k;
        k.SetNavState(mNavState);
        k.UpdatePoseFromNS();
        mTcw = k.GetPose();
    }
    NavState mNavState;
    // what the two tracking matchers, ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, ...) and (F, vpMapPoints, th), read
    // (include/Frame.h; src/Frame.cpp:440-470, :562-620): the id, the raw keypoints, the descriptor rows, the scale table, the image
    // bounds (static floats there), the grid and the pose parts of UpdatePoseMatrices
    long unsigned int mnId = 0;
    std::vector<KeyPoint> mvKeys;
    std::vector<unsigned char> mDescriptors;              // N x 32
    std::map<unsigned int, std::vector<unsigned int>> mFeatVec;   // what ComputeBoW leaves (SearchByBoW): node id -> keypoint indices
    std::vector<float> mvScaleFactors;
    int mnScaleLevels = 8;
    float mfLogScaleFactor = std::log(1.2f);
    float mnMinX = 0, mnMaxX = 0, mnMinY = 0, mnMaxY = 0;
    int mnGridCols = 64, mnGridRows = 48;                 // FRAME_GRID_COLS, FRAME_GRID_ROWS
    float mfGridElementWidthInv = 0, mfGridElementHeightInv = 0;
    std::vector<std::vector<std::vector<size_t>>> mGrid;  // [col][row] keypoint indices
    float mRcw[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, mtcw[3] = {0, 0, 0}, mOw[3] = {0, 0, 0};
    void UpdatePoseMatrices() {   // src/Frame.cpp:457-463: mRcw, mtcw, mOw = -mRcw^T mtcw in float32 like cv::Mat
        for (int i = 0; i < 3; i++) {
            for (int j = 0; j < 3; j++) mRcw[3 * i + j] = mTcw[4 * i + j];
            mtcw[i] = mTcw[4 * i + 3];
        }
        for (int i = 0; i < 3; i++) {
            float s = 0;
            for (int k = 0; k < 3; k++) s += mRcw[3 * k + i] * mtcw[k];
            mOw[i] = -s;
        }
    }
    void AssignFeaturesToGrid() {   // src/Frame.cpp:430-450 with PosInGrid: round() of the float32 cell coordinate
        mfGridElementWidthInv = (float)mnGridCols / (mnMaxX - mnMinX);
        mfGridElementHeightInv = (float)mnGridRows / (mnMaxY - mnMinY);
        mGrid.assign((size_t)mnGridCols, std::vector<std::vector<size_t>>((size_t)mnGridRows));
        for (size_t i = 0; i < mvKeysUn.size(); i++) {
            const int posX = (int)std::round((mvKeysUn[i].pt.x - mnMinX) * mfGridElementWidthInv);
            const int posY = (int)std::round((mvKeysUn[i].pt.y - mnMinY) * mfGridElementHeightInv);
            if (posX < 0 || posX >= mnGridCols || posY < 0 || posY >= mnGridRows) continue;
            mGrid[(size_t)posX][(size_t)posY].push_back(i);
        }
    }
};

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:336-413; bit VBA_MAPPOINT_DESC = 1 of `what`) and / or
// MapPoint::UpdateNormalAndDepth (:450-501; bit VBA_MAPPOINT_NORMAL = 2) for every point of the list that is neither NULL nor bad
// (:344, :458), as ONE vba_mappoint_update call (MapPointUpdate.cpp): mDescriptor, mNormalVector, mfMaxDistance and mfMinDistance are
// written as float32 where the reference writes them.  The counters of the per-point stubs above are not touched.  Returns the points
// handed to the backend, -1 when the backend failed or an input cannot be gathered (a message on std::cerr; nothing is written)
int UpdateMapPoints(const std::vector<MapPoint*>& vpMPs, int what);

inline bool cmpKeyFrameId::operator()(const KeyFrame* a, const KeyFrame* b) const { return a->mnId < b->mnId; }
inline Quaterniond MatrixToQuat(const Matrix3d& m) {   // Eigen::Quaterniond(Matrix3d)
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
    return q;
}
inline void KeyFrame::UpdateNavStatePVRFromTcw(const Mat4f& Tcw_, const Matrix3d& Rbc, const Vector3d& Pbc) {
    // Tbc * Tcw in float32, then Converter::toCvMatInverse: Rwb = (Rbc Rcw)^T, Pwb = -Rwb (Rbc tcw + Pbc)
    float Rbw[9], tbw[3];
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) {
            float a = 0;
            for (int k = 0; k < 3; k++) a += (float)Rbc[3 * i + k] * Tcw_[4 * k + j];
            Rbw[3 * i + j] = a;
        }
        float a = 0;
        for (int k = 0; k < 3; k++) a += (float)Rbc[3 * i + k] * Tcw_[4 * k + 3];
        tbw[i] = a + (float)Pbc[i];
    }
    Matrix3d Rwb;
    Vector3d Pwb;
    for (int i = 0; i < 3; i++) {
        float a = 0;
        for (int k = 0; k < 3; k++) { Rwb[3 * i + k] = (double)Rbw[3 * k + i]; a += Rbw[3 * k + i] * tbw[k]; }
        Pwb[i] = (double)(-a);
    }
    const Matrix3d Rw1 = mNavState.Get_RotMatrix();
    const Vector3d Vw1 = mNavState.Get_V();
    Vector3d b{{0, 0, 0}}, Vw2{{0, 0, 0}};
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) b[i] += Rw1[3 * k + i] * Vw1[k];          // Rw1^T Vw1
    for (int i = 0; i < 3; i++)
        for (int k = 0; k < 3; k++) Vw2[i] += Rwb[3 * i + k] * b[k];
    mNavState.Set_Pos(Pwb);
    mNavState.Set_Rot(MatrixToQuat(Rwb));
    mNavState.Set_Vel(Vw2);
}
inline float KeyFrame::ComputeSceneMedianDepth(const int q) {
    std::vector<float> vDepths;
    vDepths.reserve(mvpMapPoints.size());
    for (MapPoint* pMP : mvpMapPoints)
        if (pMP) {
            const float* P = pMP->mWorldPos;
            vDepths.push_back((Tcw[8] * P[0] + Tcw[9] * P[1] + Tcw[10] * P[2]) + Tcw[11]);
        }
    if (vDepths.empty()) return -1.0f;
    std::sort(vDepths.begin(), vDepths.end());
    return vDepths[(vDepths.size() - 1) / q];
}
inline void KeyFrame::EraseMapPointMatch(MapPoint* pMP) {
    const int idx = pMP->GetIndexInKeyFrame(this);
    if (idx >= 0) mvpMapPoints[idx] = nullptr;
}
inline std::set<MapPoint*> KeyFrame::GetMapPoints() {   // src/KeyFrame.cpp:590-605
    std::set<MapPoint*> s;
    for (MapPoint* pMP : mvpMapPoints)
        if (pMP && !pMP->isBad()) s.insert(pMP);
    return s;
}
inline void MapPoint::Replace(MapPoint* pMP) {
    if (pMP->mnId == this->mnId) return;
    const mapMapPointObs obs = mObservations;
    mObservations.clear();
    mbBad = true;
    const int nvisible = mnVisible, nfound = mnFound;
    mpReplaced = pMP;
    for (mapMapPointObs::const_iterator mit = obs.begin(), mend = obs.end(); mit != mend; mit++) {
        KeyFrame* pKF = mit->first;
        if (!pMP->IsInKeyFrame(pKF)) {
            pKF->ReplaceMapPointMatch(mit->second, pMP);
            pMP->AddObservation(pKF, mit->second);
        } else {
            pKF->EraseMapPointMatch(mit->second);
        }
    }
    pMP->IncreaseFound(nfound);
    pMP->IncreaseVisible(nvisible);
    pMP->ComputeDistinctiveDescriptors();
    if (mpMap) mpMap->EraseMapPoint(this);
}

}  // namespace ORB_SLAM2

// Thirdparty/g2o/g2o/types/sim3.h:41-292: the members LoopClosing uses (quaternion, translation, scale; map, inverse, operator*)
namespace g2o {
class Sim3 {
public:
    typedef ORB_SLAM2::Quaterniond Quaterniond;
    typedef ORB_SLAM2::Vector3d Vector3d;
    Sim3() {}
    Sim3(const Quaterniond& r_, const Vector3d& t_, double s_) : r(r_), t(t_), s(s_) {}
    const Quaterniond& rotation() const { return r; }
    Quaterniond& rotation() { return r; }
    const Vector3d& translation() const { return t; }
    Vector3d& translation() { return t; }
    const double& scale() const { return s; }
    double& scale() { return s; }
    Vector3d map(const Vector3d& xyz) const {   // s * (r * xyz) + t
        const Vector3d v = rot(r, xyz);
        return {{s * v[0] + t[0], s * v[1] + t[1], s * v[2] + t[2]}};
    }
    Sim3 inverse() const {                      // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
        const Quaterniond rc{{-r[0], -r[1], -r[2], r[3]}};
        return Sim3(rc, rot(rc, {{(-1. / s) * t[0], (-1. / s) * t[1], (-1. / s) * t[2]}}), 1. / s);
    }
    Sim3 operator*(const Sim3& o) const {       // ret.r = r * o.r; ret.t = s * (r * o.t) + t; ret.s = s * o.s
        Sim3 ret;
        ret.r = {{r[3] * o.r[0] + r[0] * o.r[3] + r[1] * o.r[2] - r[2] * o.r[1], r[3] * o.r[1] + r[1] * o.r[3] + r[2] * o.r[0] - r[0] * o.r[2],
                  r[3] * o.r[2] + r[2] * o.r[3] + r[0] * o.r[1] - r[1] * o.r[0], r[3] * o.r[3] - r[0] * o.r[0] - r[1] * o.r[1] - r[2] * o.r[2]}};
        ret.t = map(o.t);
        ret.s = s * o.s;
        return ret;
    }

private:
    static Vector3d rot(const Quaterniond& q, const Vector3d& v) {   // Eigen::Quaterniond * Vector3d
        const ORB_SLAM2::Matrix3d R = ORB_SLAM2::QuatToMatrix(q);
        return {{R[0] * v[0] + R[1] * v[1] + R[2] * v[2], R[3] * v[0] + R[4] * v[1] + R[5] * v[2], R[6] * v[0] + R[7] * v[1] + R[8] * v[2]}};
    }
    Quaterniond r{{0, 0, 0, 1}};
    Vector3d t{{0, 0, 0}};
    double s = 1.;
};
}  // namespace g2o

namespace ORB_SLAM2 {
// include/LoopClosing.h:28-34, :60: what Optimizer::OptimizeEssentialGraph takes from it
class LoopClosing {
public:
    typedef std::map<KeyFrame*, g2o::Sim3, std::less<KeyFrame*>> KeyFrameAndPose;
    void SetMapUpdateFlagInTracking(bool b) { mbMapUpdateFlagForTracking = b; }
    bool mbMapUpdateFlagForTracking = false;
    // what steps 6-9 of ComputeSim3 read and write (include/LoopClosing.h:117-126; LoopClosing.h has the function)
    KeyFrame* mpCurrentKF = nullptr;
    KeyFrame* mpMatchedKF = nullptr;
    Mat4f mScw{};
    std::vector<MapPoint*> mvpCurrentMatchedPoints, mvpLoopMapPoints;
    int mnLoopTotalMatches = 0;            // nTotalMatches of the last MatchLoopMapPoints (src/LoopClosing.cpp:473-478), -1 when it failed
    bool MatchLoopMapPoints();             // LoopClosing.cpp
};
}  // namespace ORB_SLAM2
