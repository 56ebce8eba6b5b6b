// MapPointUpdate.cpp -- MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (src/MapPoint.cpp:336-413, :450-501)
// for a list of map points over vba_mappoint_update: the skips of bad points, the gather of every point's observations in the order
// of mObservations (keyframe table, centres, bad flags, descriptor rows), the observations[pRefKF] lookup as it stands, ONE call,
// then the float32 write-back of mDescriptor, mNormalVector, mfMaxDistance and mfMinDistance.  And the two loops of LocalMapping that
// call the pair for every map point of the current keyframe: ProcessNewKeyFrame (src/LocalMapping.cpp:1144-1171) and the end of
// SearchInNeighbors (:1635-1650).  A point's update reads only its own observations and the keyframes' centres and descriptor rows,
// so the points of a keyframe share a call without changing an answer.  The per-point stubs of orbslam_min.h and their counters are
// not touched.  A source of its own: nothing here needs the matchers, and the matchers' CPU harness does not need this symbol.
#include <cstdint>
#include <cstring>
#include <iostream>
#include <map>
#include <string>
#include <vector>

#include "../../include/vislam_ba.h"
#include "BackendCall.h"
#include "orbslam_min.h"

namespace ORB_SLAM2 {

int UpdateMapPoints(const std::vector<MapPoint*>& vpMPs, int what) {
    const char* who = "UpdateMapPoints";
    const auto refuse = [&](const std::string& why) { std::cerr << who << ": " << why << std::endl; return -1; };
    if (what & ~(VBA_MAPPOINT_DESC | VBA_MAPPOINT_NORMAL)) return refuse("what has a bit outside VBA_MAPPOINT_DESC | VBA_MAPPOINT_NORMAL");
    const bool want_desc = what & VBA_MAPPOINT_DESC, want_normal = what & VBA_MAPPOINT_NORMAL;
    std::vector<MapPoint*> pts;
    for (MapPoint* pMP : vpMPs)
        if (pMP && !pMP->isBad()) pts.push_back(pMP);                            // :344, :458
    if (pts.empty() || what == 0) return 0;
    // the keyframe table: every observer and every reference keyframe once
    std::map<KeyFrame*, int32_t> row;
    std::vector<KeyFrame*> kfs;
    const auto row_of = [&](KeyFrame* pKF) {
        const auto it = row.find(pKF);
        if (it != row.end()) return it->second;
        kfs.push_back(pKF);
        return row[pKF] = (int32_t)kfs.size() - 1;
    };
    const size_t n = pts.size();
    std::vector<uint8_t> w(n, (uint8_t)what), obs_desc;
    std::vector<double> pos(3 * n, 0.0), ref_scale(n, 1.0), ref_top_scale(n, 1.0);
    std::vector<int32_t> ref_kf(n, 0), obs_begin(1, 0), obs_kf;
    for (size_t i = 0; i < n; i++) {
        MapPoint* pMP = pts[i];
        const mapMapPointObs observations = pMP->GetObservations();               // :346, :462
        if (observations.size() > VBA_MAPPOINT_MAX_OBS) return refuse("a point has more than 1024 observations");
        for (const auto& ob : observations) {
            KeyFrame* pKF = ob.first;
            obs_kf.push_back(row_of(pKF));
            if (!want_desc) continue;
            if (pKF->mDescriptors.size() < 32 * (ob.second + 1)) return refuse("an observing keyframe has no descriptor row for its keypoint");
            obs_desc.insert(obs_desc.end(), pKF->mDescriptors.begin() + 32 * ob.second, pKF->mDescriptors.begin() + 32 * (ob.second + 1));   // :361
        }
        obs_begin.push_back((int32_t)obs_kf.size());
        if (!want_normal || observations.empty()) continue;                      // :467
        KeyFrame* pRefKF = pMP->GetReferenceKeyFrame();
        if (!pRefKF) return refuse("a point has no reference keyframe");
        pMP->GetWorldPos(&pos[3 * i]);
        ref_kf[i] = row_of(pRefKF);
        // :486 `observations[pRefKF]` on the local map: a reference keyframe that is no observer gets the index 0
        const auto it = observations.find(pRefKF);
        const size_t idx = it == observations.end() ? 0 : it->second;
        if (idx >= pRefKF->mvKeysUn.size()) return refuse("the reference keyframe has no keypoint at the point's index");
        const int level = pRefKF->mvKeysUn[idx].octave, nLevels = pRefKF->mnScaleLevels;
        if (level < 0 || (size_t)level >= pRefKF->mvScaleFactors.size() || nLevels < 1 || (size_t)nLevels > pRefKF->mvScaleFactors.size())
            return refuse("the reference keyframe's scale table does not hold the keypoint's level");
        ref_scale[i] = pRefKF->mvScaleFactors[(size_t)level];                     // :487
        ref_top_scale[i] = pRefKF->mvScaleFactors[(size_t)nLevels - 1];           // :496
    }
    std::vector<double> kf_center(3 * kfs.size() + 3, 0.0);
    std::vector<uint8_t> kf_bad(kfs.size() + 1, 0);
    for (size_t k = 0; k < kfs.size(); k++) {
        kfs[k]->GetCameraCenter(&kf_center[3 * k]);                               // :476, :484
        kf_bad[k] = kfs[k]->isBad() ? 1 : 0;                                      // :360
    }
    obs_kf.push_back(0); obs_desc.resize(obs_desc.size() + 32);                   // never empty: .data() is no NULL
    vba_mappoint_problem P{};
    P.n_kf = (int32_t)kfs.size(); P.kf_center = kf_center.data(); P.kf_bad = kf_bad.data();
    P.n_pt = (int32_t)n; P.what = w.data(); P.pos = pos.data(); P.ref_kf = ref_kf.data(); P.ref_scale = ref_scale.data(); P.ref_top_scale = ref_top_scale.data();
    P.obs_begin = obs_begin.data(); P.obs_kf = obs_kf.data(); P.obs_desc = obs_desc.data();
    std::vector<int32_t> best_obs(n), best_median(n), n_desc(n);
    std::vector<uint8_t> desc(32 * n), desc_state(n), normal_state(n);
    std::vector<double> normal(3 * n), dist_max(n), dist_min(n);
    vba_mappoint_result R{};
    R.best_obs = best_obs.data(); R.best_median = best_median.data(); R.n_desc = n_desc.data(); R.desc = desc.data(); R.normal = normal.data();
    R.dist_max = dist_max.data(); R.dist_min = dist_min.data(); R.desc_state = desc_state.data(); R.normal_state = normal_state.data();
    if (!BackendCall(who, vba_mappoint_update, P, R)) return -1;
    for (size_t i = 0; i < n; i++) {
        MapPoint* pMP = pts[i];
        if (desc_state[i] == 0) std::memcpy(pMP->mDescriptor, &desc[32 * i], 32);   // :410
        if (normal_state[i] == 0) {                                              // :494-498, narrowed to the float32 the map holds
            pMP->mfMaxDistance = (float)dist_max[i];
            pMP->mfMinDistance = (float)dist_min[i];
            for (int k = 0; k < 3; k++) pMP->mNormalVector[k] = (float)normal[3 * i + (size_t)k];
        }
    }
    return (int)n;
}

int LocalMapping::ProcessNewKeyFramePoints(KeyFrame* pKF, std::list<MapPoint*>& lpRecentAddedMapPoints) {
    const std::vector<MapPoint*> vpMapPointMatches = pKF->GetMapPointMatches();   // :1144
    std::vector<MapPoint*> vpUpdate;
    for (size_t i = 0; i < vpMapPointMatches.size(); i++) {
        MapPoint* pMP = vpMapPointMatches[i];
        if (!pMP || pMP->isBad()) continue;
        if (!pMP->IsInKeyFrame(pKF)) {
            pMP->AddObservation(pKF, i);                                          // :1157
            vpUpdate.push_back(pMP);                                              // :1159-1161, batched below
        } else {
            lpRecentAddedMapPoints.push_back(pMP);                                // :1167
        }
    }
    return UpdateMapPoints(vpUpdate, VBA_MAPPOINT_DESC | VBA_MAPPOINT_NORMAL);
}

int LocalMapping::UpdateCurrentKeyFramePoints(KeyFrame* pKF) {
    return UpdateMapPoints(pKF->GetMapPointMatches(), VBA_MAPPOINT_DESC | VBA_MAPPOINT_NORMAL);   // :1635-1650; NULL and bad points are skipped there
}

}  // namespace ORB_SLAM2
