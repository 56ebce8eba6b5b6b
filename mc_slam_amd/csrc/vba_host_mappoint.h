// vba_host_mappoint.h -- host half of vba_mappoint_update (plain C++17, no HIP): which problems are refused, the exits of both parts
// that need no arithmetic (not asked, no observation (src/MapPoint.cpp:349, :467), no good keyframe (:364)), the item table of a call
// -- every point with device work, sorted by its observation count, the workgroup items (more than VBA_MP_WAVE_OBS observations) in
// front of the wave items, which then share a workgroup with three neighbours of similar size --, the arena, the packing (the
// keyframes' centres, per point with a normal part its observers as rows of the centre region, per point with a descriptor part the
// descriptors of its good keyframes, compacted) and the write-back, which maps the winning row back to an index into the point's
// observation list and copies that descriptor.  Included by vislam_ba.hip (vba_host_small.h) and by the sanitizer harness
// tests/host_mappoint_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_mappoint.py).
#pragma once
#include "../../include/vislam_ba.h"
#include "vba_host_arena.h"
#include "vba_layout.h"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

namespace vba_host {

// totals of a call: points, keyframes, items (big: the workgroup items), observer entries of the normal parts, descriptors of the
// descriptor parts
struct MapPointTotals {
    size_t pts = 0, kf = 0, items = 0, big = 0, obs = 0, desc = 0;
};

// what check_mappoint leaves for the later steps: per problem the offsets of its points and keyframes in the call, per point of the
// call N (descriptors of good keyframes; 0 without a descriptor part) and its item (-1: no device work)
struct MapPointIndex {
    std::vector<size_t> pt0, kf0;
    std::vector<int32_t> n_desc, item_of;
};

inline bool mp_finite3(const double* v) { return std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

// 0: every problem is usable; otherwise err says which is not and why
inline int check_mappoint(int n, const vba_mappoint_problem* const* in, const vba_mappoint_result* const* out, MapPointTotals& T, MapPointIndex& X,
                          std::string& err) {
    T = MapPointTotals();
    X = MapPointIndex();
    for (int f = 0; f < n; f++) {
        const vba_mappoint_problem* P = in[f];
        const vba_mappoint_result* R = out[f];
        auto fail = [&err, f](const std::string& m) { err = "problem " + std::to_string(f) + ": " + m; return 1; };
        if (!P || !R) return fail("NULL problem or result");
        if (P->n_kf < 0) return fail("negative n_kf");
        if (P->n_pt < 0) return fail("negative n_pt");
        X.pt0.push_back(T.pts); X.kf0.push_back(T.kf);
        const size_t np = (size_t)P->n_pt;
        if (np == 0) { T.kf += (size_t)P->n_kf; continue; }
        if (!P->what || !P->obs_begin || !R->best_obs || !R->best_median || !R->n_desc || !R->desc || !R->normal || !R->dist_max || !R->dist_min ||
            !R->desc_state || !R->normal_state)
            return fail("NULL array with n_pt > 0");
        if (P->obs_begin[0] != 0) return fail("obs_begin does not start at 0");
        bool any_desc = false, any_normal = false, reads_obs = false;
        for (size_t i = 0; i < np; i++) {
            const long long c = (long long)P->obs_begin[i + 1] - (long long)P->obs_begin[i];
            if (c < 0) return fail("obs_begin decreases at point " + std::to_string(i));
            if (c > VBA_MP_MAX_OBS) return fail("point " + std::to_string(i) + ": more than 1024 observations: a point's descriptors live in LDS");
            if (P->what[i] & ~(VBA_MAPPOINT_DESC | VBA_MAPPOINT_NORMAL)) return fail("point " + std::to_string(i) + ": what has a bit outside the two parts");
            any_desc = any_desc || (P->what[i] & VBA_MAPPOINT_DESC);
            any_normal = any_normal || (P->what[i] & VBA_MAPPOINT_NORMAL);
            reads_obs = reads_obs || (P->what[i] && c > 0);
        }
        if (reads_obs && !P->obs_kf) return fail("NULL obs_kf");
        if (any_desc && (!P->kf_bad || !P->obs_desc)) return fail("NULL array that the descriptor part needs");
        if (any_normal && (!P->kf_center || !P->pos || !P->ref_kf || !P->ref_scale || !P->ref_top_scale)) return fail("NULL array that the normal part needs");
        if (any_normal)
            for (size_t k = 0, e = (size_t)P->n_kf; k < e; k++)
                if (!mp_finite3(P->kf_center + 3 * k)) return fail("keyframe " + std::to_string(k) + ": centre is not finite");
        for (size_t i = 0; i < np; i++) {
            const size_t b = (size_t)P->obs_begin[i], e = (size_t)P->obs_begin[i + 1];
            const bool desc = P->what[i] & VBA_MAPPOINT_DESC, normal = P->what[i] & VBA_MAPPOINT_NORMAL;
            auto pfail = [&](const std::string& m) { return fail("point " + std::to_string(i) + ": " + m); };
            int32_t nd = 0;
            if (desc || normal)
                for (size_t j = b; j < e; j++) {
                    if (P->obs_kf[j] < 0 || P->obs_kf[j] >= P->n_kf) return pfail("observation " + std::to_string(j - b) + ": obs_kf out of range");
                    if (desc) nd += P->kf_bad[P->obs_kf[j]] ? 0 : 1;
                }
            if (normal && e > b) {
                if (!mp_finite3(P->pos + 3 * i)) return pfail("position is not finite");
                if (!std::isfinite(P->ref_scale[i]) || !std::isfinite(P->ref_top_scale[i])) return pfail("a scale is not finite");
                if (!(P->ref_scale[i] > 0.0) || !(P->ref_top_scale[i] > 0.0)) return pfail("a scale is <= 0");
                if (P->ref_kf[i] < 0 || P->ref_kf[i] >= P->n_kf) return pfail("ref_kf out of range");
            }
            X.n_desc.push_back(nd);
            const bool work = nd > 0 || (normal && e > b);
            X.item_of.push_back(work ? 0 : -1);   // the item table gives the index
            if (!work) continue;
            T.items++; T.big += (e - b > VBA_MP_WAVE_OBS);
            T.desc += (size_t)nd; T.obs += normal ? e - b : 0;
        }
        T.pts += np; T.kf += (size_t)P->n_kf;
    }
    return 0;
}

// [item | center | obs | desc] go up in one copy, [best | nrm | nstate] come back in one copy
struct MapPointArena {
    ArenaLayout L;
    size_t item, center, obs, desc, best, nrm, nstate;
    MapPointArena(const MapPointTotals& T) {
        item = L.take(sizeof(MpItem) * (T.items + 1)); center = L.take(24 * (T.kf + 1)); obs = L.take(4 * (T.obs + 1)); desc = L.take(32 * (T.desc + 1));
        L.end_upload();
        best = L.take(4 * (T.items + 1)); nrm = L.take(40 * (T.items + 1)); nstate = L.take(T.items + 1);
        L.end_back();
    }
};

// The item table: the points with device work by descending observation count (a counting sort, stable: equal counts keep the order
// of the call), so the first T.big items are the workgroup items.  An item's rows in the descriptor and observer regions follow the
// item order.  Everything of an item but those two regions' contents is written here
inline void describe_mappoint(int n, const vba_mappoint_problem* const* in, const MapPointTotals& T, MapPointIndex& X, MpItem* item) {
    std::vector<size_t> first(VBA_MP_MAX_OBS + 2, 0);   // first[c]: the first item of count c; counts descend
    for (int f = 0; f < n; f++)
        for (size_t i = 0, np = (size_t)in[f]->n_pt; i < np; i++)
            if (X.item_of[X.pt0[(size_t)f] + i] >= 0) first[(size_t)(in[f]->obs_begin[i + 1] - in[f]->obs_begin[i])]++;
    size_t at_ = 0;
    for (size_t c = VBA_MP_MAX_OBS + 1; c-- > 0;) { const size_t k = first[c]; first[c] = at_; at_ += k; }
    for (int f = 0; f < n; f++) {
        const vba_mappoint_problem* P = in[f];
        for (size_t i = 0, np = (size_t)P->n_pt; i < np; i++) {
            const size_t g = X.pt0[(size_t)f] + i;
            if (X.item_of[g] < 0) continue;
            const size_t c = (size_t)(P->obs_begin[i + 1] - P->obs_begin[i]), k = first[c]++;
            X.item_of[g] = (int32_t)k;
            MpItem& I = item[k];
            std::memset(&I, 0, sizeof I);
            I.n_desc = X.n_desc[g];
            if (P->what[i] & VBA_MAPPOINT_NORMAL) {   // work implies observations here or a descriptor part
                I.n_obs = (int)c;
                if (c > 0) {
                    I.ref = (int)(X.kf0[(size_t)f] + (size_t)P->ref_kf[i]);
                    std::memcpy(I.pos, P->pos + 3 * i, 24);
                    I.ref_scale = P->ref_scale[i]; I.ref_top_scale = P->ref_top_scale[i];
                }
            }
        }
    }
    long long d0 = 0, o0 = 0;
    for (size_t k = 0; k < T.items; k++) {
        item[k].desc0 = d0; item[k].obs0 = o0;
        d0 += item[k].n_desc; o0 += item[k].n_obs;
    }
}

// one problem into the staging block: its keyframes' centres (zeros where no point reads them), and per item of the problem the
// observers as rows of the centre region and the descriptors of the good keyframes, in observation order
inline void pack_mappoint(int f, const vba_mappoint_problem* P, const MapPointIndex& X, const MapPointArena& A, void* hin) {
    const size_t kf0 = X.kf0[(size_t)f], pt0 = X.pt0[(size_t)f], np = (size_t)P->n_pt;
    double* center = at<double>(hin, A.center) + 3 * kf0;
    bool any_normal = false;
    for (size_t i = 0; i < np; i++) any_normal = any_normal || (P->what[i] & VBA_MAPPOINT_NORMAL);
    if (any_normal) std::memcpy(center, P->kf_center, 24 * (size_t)P->n_kf);
    else std::memset(center, 0, 24 * (size_t)P->n_kf);
    const MpItem* item = at<MpItem>(hin, A.item);
    for (size_t i = 0; i < np; i++) {
        if (X.item_of[pt0 + i] < 0) continue;
        const MpItem& I = item[X.item_of[pt0 + i]];
        const size_t b = (size_t)P->obs_begin[i], e = (size_t)P->obs_begin[i + 1];
        if (I.n_obs > 0) {
            int32_t* o = at<int32_t>(hin, A.obs) + (size_t)I.obs0;
            for (size_t j = b; j < e; j++) o[j - b] = (int32_t)(kf0 + (size_t)P->obs_kf[j]);
        }
        if (I.n_desc > 0) {
            unsigned char* d = at<unsigned char>(hin, A.desc) + 32 * (size_t)I.desc0;
            for (size_t j = b; j < e; j++)
                if (!P->kf_bad[P->obs_kf[j]]) { std::memcpy(d, P->obs_desc + 32 * j, 32); d += 32; }
        }
    }
}

// The write-back of one problem: the states of both parts, the winner as (median, index into the point's observation list) with its
// descriptor copied from the caller's obs_desc, the normal and the two distances; the neutral values where a part did not run to its
// end; the counts
inline void unpack_mappoint(int f, const vba_mappoint_problem* P, vba_mappoint_result* R, const MapPointIndex& X, const int32_t* best, const double* nrm,
                            const unsigned char* nstate) {
    const size_t pt0 = X.pt0[(size_t)f], np = (size_t)P->n_pt;
    int nd = 0, nn = 0;
    for (size_t i = 0; i < np; i++) {
        const size_t b = (size_t)P->obs_begin[i], e = (size_t)P->obs_begin[i + 1];
        const int32_t it = X.item_of[pt0 + i], N = X.n_desc[pt0 + i];
        R->best_obs[i] = -1; R->best_median[i] = -1; R->n_desc[i] = N;
        std::memset(R->desc + 32 * i, 0, 32);
        R->normal[3 * i] = R->normal[3 * i + 1] = R->normal[3 * i + 2] = 0.0;
        R->dist_max[i] = R->dist_min[i] = 0.0;
        if (!(P->what[i] & VBA_MAPPOINT_DESC)) R->desc_state[i] = 1;
        else if (e == b) R->desc_state[i] = 2;                                   // :349
        else if (N == 0) R->desc_state[i] = 3;                                   // :364
        else {
            const int32_t key = best[it];
            int32_t row = key & 0xffff;
            size_t j = b;
            for (; j < e; j++)                                                   // the row among the good keyframes' observations
                if (!P->kf_bad[P->obs_kf[j]] && row-- == 0) break;
            if (j < e) {                                                         // a row below N always is
                R->best_obs[i] = (int32_t)(j - b); R->best_median[i] = key >> 16;
                std::memcpy(R->desc + 32 * i, P->obs_desc + 32 * j, 32);         // :410
            }
            R->desc_state[i] = 0;
            nd++;
        }
        if (!(P->what[i] & VBA_MAPPOINT_NORMAL)) R->normal_state[i] = 1;
        else if (e == b) R->normal_state[i] = 2;                                 // :467
        else if (nstate[it] != 0) R->normal_state[i] = 3;                        // the point lies in an observer's centre
        else {
            const double* v = nrm + 5 * (size_t)it;
            R->normal[3 * i] = v[0]; R->normal[3 * i + 1] = v[1]; R->normal[3 * i + 2] = v[2];
            R->dist_max[i] = v[3]; R->dist_min[i] = v[4];
            R->normal_state[i] = 0;
            nn++;
        }
    }
    R->status = VBA_OK;
    R->n_desc_done = nd;
    R->n_normal_done = nn;
}

// One call (a fresh object each): what the driver (run_small, vba_host_small.h) and the sanitizer harness (run_call,
// tests/host_check.h) run.  bind is the only place that maps the arena's regions to the kernel's pointers
struct MapPointCall {
    int n = 0;
    MapPointTotals T;
    MapPointIndex X;
    MapPointArena A = MapPointArena(MapPointTotals());
    int prepare(int n_problems, const vba_mappoint_problem* const* in, const vba_mappoint_result* const* out, std::string& err) {
        n = n_problems;
        if (check_mappoint(n, in, out, T, X, err)) return 1;
        A = MapPointArena(T);
        return 0;
    }
    const ArenaLayout& layout() const { return A.L; }
    size_t download_bytes() const { return A.L.back_bytes(); }
    size_t grid() const { return T.big + (T.items - T.big + 3) / 4; }   // k_mappoint_update: a workgroup item each, then four wave items each
    void describe(const vba_mappoint_problem* const* in, void* hin) { describe_mappoint(n, in, T, X, at<MpItem>(hin, A.item)); }
    const char* pack(int f, const vba_mappoint_problem* P, void* hin) const {
        pack_mappoint(f, P, X, A, hin);
        return nullptr;
    }
    MpBatch bind(void* base) const {
        MpBatch B;
        B.item = at<MpItem>(base, A.item); B.center = at<double>(base, A.center); B.obs = at<int>(base, A.obs); B.desc = at<unsigned int>(base, A.desc);
        B.n_items = (int)T.items; B.n_big = (int)T.big;
        B.best = at<int>(base, A.best); B.nrm = at<double>(base, A.nrm); B.nstate = at<unsigned char>(base, A.nstate);
        return B;
    }
    void unpack(int f, vba_mappoint_problem* P, vba_mappoint_result* R, void*, void* hout) const {
        auto back = [&](size_t off) { return A.L.in_back(off); };
        unpack_mappoint(f, P, R, X, at<int32_t>(hout, back(A.best)), at<double>(hout, back(A.nrm)), at<unsigned char>(hout, back(A.nstate)));
    }
};

}  // namespace vba_host
