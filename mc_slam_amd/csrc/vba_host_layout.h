// vba_host_layout.h -- the description half of an upload (plain C++17, no HIP, no handle): which windows are refused and why, the
// descriptor of a window (offsets into the concatenated arrays, position of its variables in the reduced system), the small
// host-built tables of the batch and its launch geometry.  Included by vislam_ba.hip (vba_host_upload.h) and by the sanitizer
// harness tests/host_layout_check.cpp (g++ -fsanitize=address,undefined, tests/test_host_layout.py).
#pragma once
#include "vba_layout.h"
#include "vba_host_structure.h"

#include <cstddef>

namespace vba_host {

inline void quat_to_R_host(const double* q, double* R) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w;
    const double txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
    R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// row of S of dof r of free keyframe a, as the kernels read it from the descriptor (the other encoding of vpos_host: the tests
// compare the two for every order)
inline int vpos(const WinDesc& d, int a, int r) {
    return r < 6 ? d.vp_pr0 + d.vp_prs * a + r : (a < d.vp_h ? d.vp_vb0 + d.vp_vbs * a : d.vp_vb1 - 9 * a) + (r - 6);
}

// the sizes build_structure and the pre-sizing of the staging rely on; a window that fails this is refused by check_window
inline bool window_sizes_ok(const vba_problem* P) {
    if (P->variant < 0 || P->variant > 2 || P->n_kf_free <= 0 || P->n_kf_free > P->n_kf || P->n_pt <= 0 || P->n_obs <= 0 || P->n_imu < 0) return false;
    return !(P->variant != VBA_VARIANT_SE3_XYZ && P->n_imu > 0 && (!P->imu_kf_i || !P->imu_kf_j));
}

// why a window cannot be part of the batch whose first window is `first` (nullptr: it can)
inline const char* check_window(const vba_problem* P, const vba_problem* first) {
    if (P->variant < 0 || P->variant > 2 || (P->algo != VBA_ALGO_GN && P->algo != VBA_ALGO_LM)) return "bad variant / algo";
    if (P->variant == VBA_VARIANT_PRV_IDP && P->algo != VBA_ALGO_GN)
        return "inverse-depth landmarks are solved with Gauss-Newton only (as the reference does, src/Optimizer.cpp:136)";
    if (P->variant != VBA_VARIANT_PRV_IDP && P->algo != VBA_ALGO_LM)
        return "XYZ landmarks are solved with Levenberg-Marquardt only (as the reference does, src/Optimizer.cpp:1028,3928)";
    if (P->n_kf_free <= 0 || P->n_kf_free > P->n_kf || P->n_pt < 0 || P->n_obs < 0 || P->n_imu < 0) return "bad sizes";
    if (P->variant != VBA_VARIANT_SE3_XYZ && P->n_imu > 0 && (!P->imu_kf_i || !P->imu_kf_j || !P->imu_meas || !P->imu_info_prv))
        return "n_imu > 0 but an IMU array is NULL";
    if (P->n_pt == 0 || P->n_obs == 0) return "a window without landmarks or observations has nothing to optimise";
    if (P != first && (P->variant != first->variant || P->algo != first->algo || P->solver != first->solver)) return "mixed batch";
    if (P->solver != VBA_SOLVER_LDLT && P->solver != VBA_SOLVER_PCG) return "unknown solver";
    if (P->its_stage1 > 30 || P->its_stage2 > 30 || P->its_stage1 < 0 || P->its_stage2 < 0) return "its out of range";
    if (P->protocol != VBA_PROTO_LOCAL && P->protocol != VBA_PROTO_SINGLE) return "unknown protocol";
    // the diagonal Schur walk reaches a window's slot records through a 32-bit byte offset from the window's first one
    if (P->variant == VBA_VARIANT_PRV_IDP && ((long long)P->n_obs + P->n_pt) * (VBA_SLOT * 8) >= (1ll << 32))
        return "inverse-depth window with more than 2^32 bytes of slot records";
    return nullptr;
}

// running offsets of the windows described so far into the concatenated arrays of the batch
struct BatchCursor {
    int win = 0;   // windows described so far
    int kf0 = 0, pt0 = 0, obs0 = 0, imu0 = 0, pair0 = 0, pimu0 = 0, vec0 = 0, part0 = 0;
    long long item0 = 0, mask0 = 0;
    size_t S_tot = 0;
};

// launch geometry: maxima over the windows of the batch (a fresh one per upload: the initialisers are the reset)
struct LaunchGeom {
    int max_pt_blk = 0, max_imu = 0, max_pairs = 0, max_nb = 0, max_obs_blk = 0, max_kf_blk = 0, max_ns_blk = 0;
    int max_nS = 0, max_its[2] = {0, 0}, max_free = 0, max_lin_blk = 0, max_quads = 1, max_offp = 1, max_pan = 0;
    int max_kf = 0, max_mwords = 1;   // keyframes (free and fixed) and 64-bit mask words of the largest window: the structure build
    size_t chain_lds = 0;   // dynamic LDS of k_chol_chain (its per-column tile tables)
    int min_nc = 1 << 30, max_nc = 0, max_cu = 0, max_chain_rows = 0, max_split = 0;   // chain columns of the batch's windows (k_chol_chain); tiles of its update launch
    std::vector<int> step_grid;  // workgroups per factorisation step (max over the batch)
    std::vector<int> pan_grid;   // panel tiles per step (max over the batch)
    double tile_updates = 0;     // tile-pair updates per factorisation, summed over the batch
    bool any_lin_fallback = false;  // an XYZ window of the batch has a landmark with > 256 observations: k_lin_xyz also runs
};

// the small host-built lists of the batch, window after window
struct BatchTables {
    std::vector<int> tlstep, tlpair, tlpanb, tlpan, linblk, tlkb, tlk, adjbeg, adj, prun0, prefbeg, preflist, culist, chaintab;
};

struct DescribeOpts {
    bool pcg = false;       // the batch is solved with PCG: adjacency lists, p'Sp partials
    bool chain_on = false;  // chain columns in one launch (vba_chain.h)
    int pcg_rows = 64;      // rows per workgroup of the PCG matvec (PCG_ROWS)
};

// Descriptor of the next window of the batch: fills d, appends the window's rows to the tables, advances the cursor and folds
// the window into the launch geometry.  Returns the refusal message, or nullptr.
inline const char* describe_window(const vba_problem* P, const Structure& st, const DescribeOpts& opts, BatchCursor& c, LaunchGeom& g,
                                   BatchTables& t, WinDesc& d) {
    const int w = c.win;
    d.variant = P->variant; d.algo = P->algo;
    d.protocol = P->protocol; d.robust = P->robust;
    d.win = w;
    d.n_kf = P->n_kf; d.n_free = P->n_kf_free; d.n_pt = P->n_pt; d.n_obs = P->n_obs;
    d.n_imu = (P->variant == VBA_VARIANT_SE3_XYZ) ? 0 : P->n_imu;
    d.pdim = (P->variant == VBA_VARIANT_SE3_XYZ) ? 6 : 15;
    d.np = d.pdim * d.n_free;
    d.nS = st.nS;           // (the order decides: the two-sided order pads each of its parts to a tile boundary)
    d.nb = d.nS / VBA_NB;
    d.its[0] = P->its_stage1; d.its[1] = P->its_stage2;
    d.kf0 = c.kf0; d.pt0 = c.pt0; d.obs0 = c.obs0; d.imu0 = c.imu0;
    d.pair0 = c.pair0; d.n_pairs = d.n_free * (d.n_free + 1) / 2;
    d.item0 = (int)c.item0; d.pimu0 = c.pimu0; d.vec0 = c.vec0; d.part0 = c.part0;
    d.mask0 = c.mask0; d.mwords = st.mwords;
    d.adj0 = (int)t.adj.size();
    if (opts.pcg) {
        t.adjbeg.resize((size_t)c.kf0 + w, 0);   // rows of adj_begin start at kf0 + win, like the keyframe segments
        t.adjbeg.insert(t.adjbeg.end(), st.adj_begin.begin(), st.adj_begin.end());
        t.adj.insert(t.adj.end(), st.adj.begin(), st.adj.end());
    }
    d.n_part_pt = (d.n_pt + 63) / 64;
    d.n_part_lin = d.n_part_pt;
    d.lin_runs = 0;
    if (!st.linblk.empty()) {   // the work split of the edge-parallel linearisation
        d.lb0 = (int)(t.linblk.size() / 4);
        t.linblk.insert(t.linblk.end(), st.linblk.begin(), st.linblk.end());
        d.n_part_lin = (int)(st.linblk.size() / 4);
        d.lin_runs = 1;
        if (!st.prun0.empty()) {   // inverse depth: the run records of the reference-keyframe terms (ids window-local)
            t.prun0.resize((size_t)d.lb0, 0);
            t.prun0.insert(t.prun0.end(), st.prun0.begin(), st.prun0.end() - 1);
            t.prefbeg.resize((size_t)c.kf0 + w, 0);   // rows start at kf0 + win, like the keyframe segments
            t.prefbeg.insert(t.prefbeg.end(), st.pref_begin.begin(), st.pref_begin.end());
            t.preflist.resize((size_t)c.pt0, 0);      // a window has at most n_pt run records: its list starts at pt0
            t.preflist.insert(t.preflist.end(), st.pref_list.begin(), st.pref_list.end());
        }
    } else
        g.any_lin_fallback = true;
    d.S0 = (long long)c.S_tot;
    for (int i = 0; i < 4; i++) d.K[i] = P->K[i];
    quat_to_R_host(P->T_cb + 3, d.Rcb);
    for (int i = 0; i < 3; i++) { d.tcb[i] = P->T_cb[i]; d.g[i] = P->g_w[i]; }
    d.inv_bg = P->inv_bg_rw2; d.inv_ba = P->inv_ba_rw2;
    d.hub_vis = P->huber_vis; d.hub_prv = P->huber_prv; d.hub_bias = P->huber_bias;
    d.chi2_th = P->chi2_th; d.depth_min = P->depth_min; d.rho_min = P->rho_min;
    d.tl_step0 = (int)t.tlstep.size(); d.tl_pair0 = (int)t.tlpair.size(); d.tl_pan0 = (int)t.tlpan.size();
    t.tlstep.insert(t.tlstep.end(), st.step_begin.begin(), st.step_begin.end());
    t.tlpanb.insert(t.tlpanb.end(), st.pan_begin.begin(), st.pan_begin.end());
    t.tlpair.insert(t.tlpair.end(), st.tpairs.begin(), st.tpairs.end());
    t.tlpan.insert(t.tlpan.end(), st.pan.begin(), st.pan.end());
    d.order = st.order;
    d.vp_h = 2147483647; d.vp_vb1 = 0;
    for (int q = 0; q < 3; q++) { d.pad0[q] = 0; d.padn[q] = 0; }
    d.pad0[0] = d.np; d.padn[0] = d.nS - d.np;
    if (d.pdim != 15) { d.vp_pr0 = 0; d.vp_prs = 6; d.vp_vb0 = 0; d.vp_vbs = 0; }
    else if (d.order == 2) {
        int hh, baseB, pr0;
        two_sided_layout(d.n_free, hh, baseB, pr0);
        d.vp_pr0 = pr0; d.vp_prs = 6; d.vp_vb0 = 0; d.vp_vbs = 9; d.vp_h = hh; d.vp_vb1 = baseB + 9 * (d.n_free - 1);
        d.pad0[0] = 9 * hh; d.padn[0] = baseB - 9 * hh;
        d.pad0[1] = baseB + 9 * (d.n_free - hh); d.padn[1] = pr0 - d.pad0[1];
        d.pad0[2] = pr0 + 6 * d.n_free; d.padn[2] = d.nS - d.pad0[2];
    }
    else if (d.order) { d.vp_pr0 = 0; d.vp_prs = 15; d.vp_vb0 = 6; d.vp_vbs = 15; }
    else { d.vp_pr0 = 9 * d.n_free; d.vp_prs = 6; d.vp_vb0 = 0; d.vp_vbs = 9; }
    d.nc_split = (opts.chain_on && st.nc > 0) ? st.nc_split : 0;
    g.max_split = std::max(g.max_split, d.nc_split);
    d.tl_kb0 = (int)t.tlkb.size(); d.tl_k0 = (int)t.tlk.size();
    t.tlkb.insert(t.tlkb.end(), st.kl_begin.begin(), st.kl_begin.end());
    t.tlk.insert(t.tlk.end(), st.klist.begin(), st.klist.end());
    d.nc = opts.chain_on ? st.nc : 0;
    d.cu0 = (int)(t.culist.size() / 4); d.n_cu = d.nc > 0 ? (int)(st.cu.size() / 4) : 0;
    if (d.nc > 0) t.culist.insert(t.culist.end(), st.cu.begin(), st.cu.end());
    d.ct0 = (int)(t.chaintab.size() / 4);
    if (d.nc > 0) t.chaintab.insert(t.chaintab.end(), st.chain_tab.begin(), st.chain_tab.end());
    g.min_nc = std::min(g.min_nc, d.nc); g.max_nc = std::max(g.max_nc, d.nc); g.max_cu = std::max(g.max_cu, d.n_cu);
    g.max_chain_rows = std::max(g.max_chain_rows, d.nc > 0 ? d.nb - d.nc : 0);
    g.chain_lds = std::max(g.chain_lds, ((size_t)d.nc * (d.nb - d.nc) + 2 * (size_t)d.nc + 8) * sizeof(short));   // chain_tab_bytes
    if ((int)g.step_grid.size() < d.nb) { g.step_grid.resize(d.nb, 1); g.pan_grid.resize(d.nb, 0); }
    for (int k = 0; k < d.nb; k++) {
        g.step_grid[k] = std::max(g.step_grid[k], std::max(1, st.step_npairs[k]));
        g.pan_grid[k] = std::max(g.pan_grid[k], st.pan_begin[k + 1] - st.pan_begin[k]);
    }
    g.tile_updates += (double)st.tpairs.size();
    if ((int)st.pair_a.size() != d.n_pairs || (int)st.off_pair.size() != d.n_pairs || (int)st.pair_mask.size() != d.n_pairs ||
        (int)st.pimu_begin.size() != d.n_pairs + 1 || st.lmask.size() != (size_t)d.n_pt * st.mwords)
        return "internal: structure sizes";
    {   // the per-window offsets are 32-bit: refuse a batch that would overflow them instead of wrapping
        const long long lim = 2147483647LL - 64;
        if ((long long)c.obs0 + d.n_obs > lim || c.item0 + st.item_cap > lim ||
            (long long)t.tlpair.size() > lim || (long long)t.tlk.size() > lim || (long long)c.vec0 + d.nS > lim)
            return "batch too large for 32-bit offsets: split it into several calls";
    }
    c.win++;
    c.kf0 += d.n_kf; c.pt0 += d.n_pt; c.obs0 += d.n_obs; c.imu0 += d.n_imu;
    c.pair0 += d.n_pairs; c.item0 += st.item_cap; c.pimu0 += (int)(st.pimu.size() / 2);
    c.mask0 += (long long)d.n_pt * st.mwords;
    c.vec0 += d.nS;
    const int obs_blk = (d.n_obs + 63) / 64;
    // chi2 / computeScale / max-diagonal partials of the linearisation and update kernels, the per-block sums of the final edge
    // pass -- and, with PCG, one p'Sp partial per PCG_ROWS rows of the reduced system (k_pcg_matvec), which grows with the
    // KEYFRAMES of the window, not with its landmarks
    c.part0 += std::max(std::max(3 * std::max(d.n_part_lin, (d.n_pt + 63) / 64), 2 * obs_blk), opts.pcg ? (d.np + opts.pcg_rows - 1) / opts.pcg_rows : 0) + 2;
    c.S_tot += (size_t)d.nS * d.nS;
    g.max_kf = std::max(g.max_kf, d.n_kf);
    g.max_mwords = std::max(g.max_mwords, d.mwords);
    g.max_pt_blk = std::max(g.max_pt_blk, (d.n_pt + 63) / 64);
    g.max_lin_blk = std::max(g.max_lin_blk, d.n_part_lin);
    g.max_imu = std::max(g.max_imu, d.n_imu);
    g.max_pairs = std::max(g.max_pairs, d.n_pairs);
    g.max_free = std::max(g.max_free, d.n_free);
    g.max_quads = std::max(g.max_quads, (d.n_pairs - d.n_free + 3) / 4);
    g.max_pan = std::max(g.max_pan, (int)st.pan.size());
    g.max_offp = std::max(g.max_offp, d.n_pairs - d.n_free);
    g.max_nb = std::max(g.max_nb, d.nb);
    g.max_obs_blk = std::max(g.max_obs_blk, obs_blk);
    g.max_kf_blk = std::max(g.max_kf_blk, (d.n_kf + 63) / 64);
    g.max_ns_blk = std::max(g.max_ns_blk, (d.nS + 63) / 64);
    g.max_nS = std::max(g.max_nS, d.nS);
    g.max_its[0] = std::max(g.max_its[0], d.its[0]);
    g.max_its[1] = std::max(g.max_its[1], d.its[1]);
    return nullptr;
}

}  // namespace vba_host
