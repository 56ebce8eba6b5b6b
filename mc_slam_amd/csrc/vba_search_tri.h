// vba_search_tri.h -- batched matching for triangulation on the GPU.
// Replaces, for a batch of keyframe pairs, ORBmatcher::SearchForTriangulation (src/ORBmatcher.cpp:760-955, monocular) behind the
// node join, which the host does (vba_host_search_tri.h): the candidate loop of every keypoint of keyframe 1 (:833-884) with
// CheckDistEpipolarLine (:167-192), the rotation histogram (:896-906), ComputeThreeMaxima (:1800-1841) and the filter (:931-940).
// The state codes are those of include/vislam_ba.h.
//
// One 256-lane workgroup per pair, ONE launch.  Lanes stride over the query list the host laid out in the order of the reference's
// walk, so neighbouring lanes sit in the same node and run through the same candidates.  A query's descriptor lives in 8 VGPRs; a
// candidate is one 64-byte StKey record: two 16-byte loads bring its descriptor, and only a candidate whose distance passes :863
// has its other two quarters loaded.  vbMatched2 is never set in the reference (:782, :848), so a query reads nothing another
// query writes: the sequential update of :863-882 runs inside one lane, in list order, as written.  F12, the epipole, the two
// thresholds, the level tables and the histogram live in LDS.  Four phases separated by workgroup barriers only: (0) staging, and
// the outputs of every keypoint that is no query; (1) the queries, bins counted with integer LDS atomics (counts do not depend on
// order); (2) the three maxima, by every lane from LDS; (3) the filter, each lane over the queries it matched itself.  No atomics on
// memory, no floating-point atomics, nothing waits on another workgroup; every loop is bounded by the pair's sizes; every output
// address is written by exactly one lane per phase, and a lane reads back only what it wrote itself.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_search_area.h"   // sa_load_desc, sa_hamming

#define ST_NT VBA_ST_NT
// offsets in StDesc::c (and in the LDS copy)
#define ST_F 0
#define ST_EX 9
#define ST_EY 10
#define ST_CHI2 11
#define ST_R2 12

// :898-901 in float32, these three operations and C round (half away from zero)
DEVI int st_bin(float angle1, float angle2) {
    float rot = angle1 - angle2;
    if (rot < 0.0f) rot += 360.0f;
    const float factor = 1.0f / VBA_ST_HISTO;
    int bin = (int)roundf(rot * factor);
    if (bin == VBA_ST_HISTO) bin = 0;   // :902 (cannot occur with this factor; kept)
    return bin;
}

// ComputeThreeMaxima (:1800-1841) over bin counts
DEVI void st_three_maxima(const int* histo, int& ind1, int& ind2, int& ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    int i1 = -1, i2 = -1, i3 = -1;
    for (int i = 0; i < VBA_ST_HISTO; i++) {
        const int s = histo[i];
        const bool g1 = s > max1, g2 = s > max2, g3 = s > max3;   // max1 >= max2 >= max3, so g1 implies g2 implies g3
        max3 = g2 ? max2 : (g3 ? s : max3);
        i3 = g2 ? i2 : (g3 ? i : i3);
        max2 = g1 ? max1 : (g2 ? s : max2);
        i2 = g1 ? i1 : (g2 ? i : i2);
        max1 = g1 ? s : max1;
        i1 = g1 ? i : i1;
    }
    const float lim = 0.1f * (float)max1;
    const bool cut2 = (float)max2 < lim, cut3 = (float)max3 < lim;
    ind1 = i1;
    ind2 = cut2 ? -1 : i2;
    ind3 = (cut2 || cut3) ? -1 : i3;
}

__global__ void __launch_bounds__(ST_NT) k_search_tri(StBatch B) {
    __shared__ double sc[VBA_ST_CONST];
    __shared__ double slev[2 * VBA_TRI_LEVELS];
    __shared__ int shist[VBA_ST_HISTO];
    __shared__ int scount[2];            // matches in front of the filter, matches the filter dropped
    const StDesc& d = B.desc[blockIdx.x];
    const int tid = threadIdx.x;
    const int n1 = d.n_keys1, nq = d.n_q, nl = d.n_levels2;   // nl: 1 .. VBA_TRI_LEVELS (checked on the host)
    const int th_low = d.th_low;
    const bool check_ori = d.check_orientation != 0;
    const StKey* key1 = B.key1 + (size_t)d.key1_0;
    const StKey* key2 = B.key2 + (size_t)d.key2_0;
    const StQuery* query = B.query + (size_t)d.key1_0;
    const int* feat = B.feat + (size_t)d.feat0;
    int* match12 = B.match12 + (size_t)d.key1_0;
    unsigned char* best_dist = B.best_dist + (size_t)d.key1_0;
    unsigned char* state = B.state + (size_t)d.key1_0;

    // ---- phase 0: staging; every keypoint of keyframe 1 that is no query leaves with the state the host found
    if (tid < VBA_ST_CONST) sc[tid] = d.c[tid];
    if (tid < 2 * nl) slev[tid] = B.lev[(size_t)d.lev0 + tid];
    if (tid < VBA_ST_HISTO) shist[tid] = 0;
    if (tid < 2) scount[tid] = 0;
    for (int i = tid; i < n1; i += ST_NT) {
        const unsigned char role = key1[i].role;
        if (role != 0) { match12[i] = -1; best_dist[i] = 255; state[i] = role; }
    }
    __syncthreads();
    const double* sg2 = slev;
    const double* sc2 = slev + nl;

    // ---- phase 1: the queries (:810-907)
    int n_mine = 0;
    for (int q = tid; q < nq; q += ST_NT) {
        const StQuery qr = query[q];
        const StKey& k1 = key1[qr.idx1];
        unsigned int a[8];
        sa_load_desc(a, k1.d);
        const double u1 = k1.u, v1 = k1.v;
        const float angle1 = k1.angle;
        // the epipolar line of kp1 in keyframe 2: l = x1' F12 = [a b c] (:172-174)
        const double la = (u1 * sc[ST_F + 0] + v1 * sc[ST_F + 3]) + sc[ST_F + 6];
        const double lb = (u1 * sc[ST_F + 1] + v1 * sc[ST_F + 4]) + sc[ST_F + 7];
        const double lc = (u1 * sc[ST_F + 2] + v1 * sc[ST_F + 5]) + sc[ST_F + 8];
        const double den = la * la + lb * lb;
        int bestDist = th_low, bestIdx2 = -1;
        float bestAngle = 0.0f;
        for (int c = qr.c_begin; c < qr.c_end; c++) {
            const int idx2 = feat[c];
            const StKey& k2 = key2[idx2];
            const int dist = sa_hamming(a, k2.d);
            // the reference tests the map point (:848) in front of the distance (:863); both are plain `continue`s, so the order
            // is free, and this one reads the second half of the record only for a candidate whose distance passes
            if (dist > th_low || dist > bestDist) continue;                       // :863
            if (k2.role != 0) continue;                                           // :848 pMP2
            const double u2 = k2.u, v2 = k2.v;
            const int oct = k2.oct;
            const double dx = sc[ST_EX] - u2, dy = sc[ST_EY] - v2;
            if (dx * dx + dy * dy < sc[ST_R2] * sc2[oct]) continue;               // :874
            const double num = (la * u2 + lb * v2) + lc;                          // :180
            if (den == 0.0) continue;                                             // :184
            if (!(num * num / den < sc[ST_CHI2] * sg2[oct])) continue;            // :191
            bestIdx2 = idx2;                                                      // :881-882
            bestDist = dist;
            bestAngle = k2.angle;
        }
        match12[qr.idx1] = bestIdx2;
        best_dist[qr.idx1] = (bestIdx2 >= 0) ? (unsigned char)bestDist : (unsigned char)255;
        state[qr.idx1] = (bestIdx2 >= 0) ? 0 : 3;
        if (bestIdx2 >= 0) {
            n_mine++;
            if (check_ori) atomicAdd(&shist[st_bin(angle1, bestAngle)], 1);
        }
    }
    if (n_mine) atomicAdd(&scount[0], n_mine);
    __syncthreads();

    // ---- phase 2: the three maxima (:929), by every lane from the same LDS words
    int ind1 = -1, ind2 = -1, ind3 = -1;
    if (check_ori) st_three_maxima(shist, ind1, ind2, ind3);

    // ---- phase 3: the filter (:931-940); a lane walks the queries it ran itself and reads back its own match12
    if (check_ori) {
        int n_drop = 0;
        for (int q = tid; q < nq; q += ST_NT) {
            const int idx1 = query[q].idx1;
            const int idx2 = match12[idx1];
            if (idx2 < 0) continue;
            const int bin = st_bin(key1[idx1].angle, key2[idx2].angle);
            if (bin == ind1 || bin == ind2 || bin == ind3) continue;
            match12[idx1] = -1;
            state[idx1] = 4;
            n_drop++;
        }
        if (n_drop) atomicAdd(&scount[1], n_drop);
    }
    __syncthreads();
    StOut& o = B.out[blockIdx.x];
    if (tid < VBA_ST_HISTO) o.hist[tid] = shist[tid];
    if (tid == 0) {
        o.status = VBA_OK;
        o.n_before_filter = scount[0];
        o.n_matches = scount[0] - scount[1];
        o.ind[0] = ind1; o.ind[1] = ind2; o.ind[2] = ind3;
    }
}
