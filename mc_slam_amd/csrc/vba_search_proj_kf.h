// vba_search_proj_kf.h -- batched projection matching for loop closure and relocalisation on the GPU.
// Replaces, for a batch of (target, ordered query list) problems, ORBmatcher::SearchByProjection(KeyFrame* pKF, cv::Mat Scw, vpPoints,
// vpMatched, th) (src/ORBmatcher.cpp:354-475, over KeyFrame::GetFeaturesInArea src/KeyFrame.cpp:1071-1115; mode 0, "loop") and
// ORBmatcher::SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (:1667-1797, over
// Frame::GetFeaturesInArea src/Frame.cpp:562-620; mode 1, "reloc"), monocular.  The state codes are those of include/vislam_ba.h; the
// rotation histogram, ComputeThreeMaxima, the drop and the writes into vpMatched / mvpMapPoints are replayed on the host
// (vba_host_search_proj_kf.h).
//
// The queries of a problem are NOT independent: a match takes its keypoint away from every later query (:446 and :468; :1738 and
// :1754).  The layout is that of k_search_proj (vba_search_proj.h), with every query blocking: one 256-lane workgroup owns a problem
// and its lanes stride over the queries.  Phase 1 evaluates the mode's gates and the projection once per query.  Then the conflict
// pass of vba_search_claim.h runs (the protocol, its proof and the bound of n_q + 1 rounds are there): every match claims its
// keypoint, a keypoint occupied before the call is statically taken, and the visitor skips a query that never reaches the area.  The
// claim table is n_keys int32 of dynamic LDS (n_keys <= VBA_SP_MAX_KEYS, checked on the host).  The kernel takes k_search_proj's
// argument and leaves best_dist2 and view_cos alone (the host binds them as null).  Every output address is written by one lane
// only.  Plain log, floor, ceil and sqrt in FP64, contraction off so that the operations are the ones the header names.
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_search_area.h"
#include "vba_search_claim.h"

#define SK_NT VBA_SP_NT   // SpDesc::c is the camera block (SA_*, vba_search_area.h)

__global__ void __launch_bounds__(SK_NT) k_search_proj_kf(SpBatch B) {
#pragma clang fp contract(off)
    extern __shared__ int sk_claim[];   // [n_keys of the call's largest target]
    __shared__ double sc[VBA_SP_CONST];
    const SpDesc& d = B.desc[blockIdx.x];
    const int tid = threadIdx.x;
    const int nk = d.n_keys, nq = d.n_q, nl = d.n_levels;   // nk <= VBA_SP_MAX_KEYS, nl: 1 .. VBA_TRI_LEVELS (checked on the host)
    const bool reloc = d.mode != 0;
    if (tid < VBA_SP_CONST) sc[tid] = d.c[tid];
    const double* tb = sc + SA_TB;
    const SaGrid grid = {B.key + (size_t)d.key0, B.cell_begin + (size_t)d.cell0, B.cell_feat + (size_t)d.feat0, d.cols, d.rows};
    const unsigned char* occupied = B.occupied + (size_t)d.key0;
    const double* scale = B.lev + (size_t)d.lev0;
    const SpQuery* query = B.query + (size_t)d.q0;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    const auto taken = [&](int k) { return occupied[k] != 0; };
    claim_reset<SK_NT>(sk_claim, nk, taken);

    // phase 1: the gates and the projection, once per query.  255: the query reaches the area
    const int st_level = reloc ? 4 : 6;
    for (int q = tid; q < nq; q += SK_NT) {
        const size_t o = (size_t)d.q0 + (size_t)q;
        const SpQuery& Q = query[q];
        int state = 255, level = -128;
        double u = qnan, v = qnan, r = 0.0;
        do {
            if (Q.skip) { state = 1; break; }                                            // :385, :1688-1690
            const double px = Q.pos[0], py = Q.pos[1], pz = Q.pos[2];
            double xc, yc, zc;
            sa_rigid(sc + SA_R, sc + SA_T, px, py, pz, xc, yc, zc);
            if (!reloc) {
                if (zc < 0.0) { state = 2; break; }                                      // :395
                const double invz = 1.0 / zc;
                u = sc[SA_K + 0] * (xc * invz) + sc[SA_K + 2];                           // :399-404
                v = sc[SA_K + 1] * (yc * invz) + sc[SA_K + 3];
                if (!(u >= tb[SA_B + 0] && u < tb[SA_B + 1] && v >= tb[SA_B + 2] && v < tb[SA_B + 3])) { state = 3; break; }   // :407
            } else {
                const double invz = 1.0 / zc;                                            // :1698, no depth test
                u = (sc[SA_K + 0] * xc) * invz + sc[SA_K + 2];                           // :1700-1701
                v = (sc[SA_K + 1] * yc) * invz + sc[SA_K + 3];
                // :1703-1706; a NaN passes the reference's tests and leaves here (a deviation)
                if (!(isfinite(u) && isfinite(v)) || u < tb[SA_B + 0] || u > tb[SA_B + 1] || v < tb[SA_B + 2] || v > tb[SA_B + 3]) { state = 2; break; }
            }
            const double ox = px - sc[SA_OW + 0], oy = py - sc[SA_OW + 1], oz = pz - sc[SA_OW + 2];
            const double dist = sqrt((ox * ox + oy * oy) + oz * oz);
            if (dist < Q.dist_min || dist > Q.dist_max) { state = reloc ? 3 : 4; break; }   // :417, :1716
            if (!reloc) {
                const double dot = (ox * Q.normal[0] + oy * Q.normal[1]) + oz * Q.normal[2];
                if (dot < sc[SA_COS] * dist) { state = 5; break; }                       // :423
            }
            if (!sa_predict_level(Q.pred_max, dist, tb[SA_LOGSF], nl, level)) { state = st_level; break; }   // :426, :1719 with the range check
            r = tb[SA_TH] * scale[level];                                                // :430, :1722
        } while (false);
        B.best_idx[o] = -1;
        B.best_dist[o] = 256;
        B.level[o] = (signed char)level;
        const bool has_uv = state == 255 || state >= (reloc ? 2 : 3);
        B.uv[2 * o] = has_uv ? u : qnan;
        B.uv[2 * o + 1] = has_uv ? v : qnan;
        B.state[o] = (unsigned char)state;
        B.rad[o] = r;
        B.prev[o] = (state == 255) ? -1 : -2;
    }

    // the conflict pass: at most n_q + 1 rounds.  The visitor walks one query against the table of the round before
    const int th_dist = d.th_high;
    const auto claim_of = [&](int q) { return B.prev[(size_t)d.q0 + (size_t)q]; };
    const int n_rounds = claim_rounds<SK_NT>(sk_claim, nk, nq, nq, taken, claim_of, [&](int q, int round) {
        const size_t o = (size_t)d.q0 + (size_t)q;
        const int before = B.prev[o];
        if (q < round || before == -2) return false;   // final since round q; never reaches the area
        const SpQuery& Q = query[q];
        const double u = B.uv[2 * o], v = B.uv[2 * o + 1], r = B.rad[o];
        const int L = (int)B.level[o];
        int bestDist = 256, bestIdx = -1;
        bool any = false;
        unsigned int a[8];
        sa_load_desc(a, Q.d);
        sa_walk(grid, tb, u, v, r, [&](int idx, const FuKey& k) {
            const int kl = k.oct;
            if (reloc && (kl < L - 1 || kl > L + 1)) return;                         // Frame.cpp:600-607 with (L - 1, L + 1): maxLevel >= 0
            if (!(fabs(k.u - u) < r && fabs(k.v - v) < r)) return;                   // KeyFrame.cpp:1107, Frame.cpp:612
            any = true;                                                              // :434, :1727
            if (sk_claim[idx] < q) return;                                           // :446, :1738
            if (!reloc && (kl < L - 1 || kl > L)) return;                            // :451
            const int dist = sa_hamming(a, k.d);
            if (dist < bestDist) { bestDist = dist; bestIdx = idx; }                 // :458, :1745
        });
        int state;
        if (!any) state = reloc ? 5 : 7;
        else if (!(bestDist <= th_dist && bestIdx >= 0)) state = reloc ? 6 : 8;      // :466, :1752
        else state = 0;
        const int now = (state == 0) ? bestIdx : -1;
        B.prev[o] = now;
        B.best_idx[o] = bestIdx;
        B.best_dist[o] = (unsigned short)bestDist;
        B.state[o] = (unsigned char)state;
        return now != before;
    });
    if (tid == 0) B.rounds[blockIdx.x] = n_rounds;
}
