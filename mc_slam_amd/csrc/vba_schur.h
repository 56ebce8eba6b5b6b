// vba_schur.h -- the reduced system: S, its right-hand side, b_p and the H_pp diagonal, one workgroup per keyframe pair.
// Reads the records of the linearisation (slot, erec, prec, lm_sd, obs_uvk, imuH), kfR, pt, var_act and the pair / item lists of the
// structure build; writes S (lower triangle), vec, bpose and, for XYZ landmarks, kf_dir.  The walk over a pair's items is
// separate per landmark type (inverse depth, Gauss-Newton; XYZ, Levenberg-Marquardt): schur_off_walk_idp / _xyz for the
// off-diagonal pairs, the two branches of schur_diag_body for the diagonal ones; what surrounds a walk is shared.
// Needs vba_batch.h and vba_lin.h (idp_point_world, idp_edge_wres).
#pragma once
#include "vba_batch.h"
#include "vba_lin.h"

// ------------------------------------------------------------------------------------------------
// K_schur: one workgroup per keyframe block pair (a <= b).  Gathers, in a fixed order, every landmark
// observed from both keyframes: S_ab = H_ab - sum_l W_al Dinv_l W_bl^T (block_solver.hpp:373-430), adds the
// IMU blocks, writes the pdim x pdim block (and its mirror) exactly once.  Diagonal pairs also produce the
// reduced right-hand side (:436-439), the unreduced b_p and the H_pp diagonal (for LM's lambda init).
// ------------------------------------------------------------------------------------------------
DEVI double wave_sum(double v) {   // (the 64-lane sums of the diagonal pass stay on the crossbar: with the DPP form k_schur_all needs two registers more and spills)
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// window / pair of a workgroup.  With >= 8 windows the mapping is XCD-aware: the dispatcher deals consecutive
// workgroups round-robin over the 8 XCDs, so all workgroups of one window share (id % 8) and the window's slot
// records stay in one XCD's L2.  (Speed only; results do not depend on placement.)
DEVI bool schur_map(const Batch& B, int per_win, int& w, int& idx) {
    const int lid = blockIdx.x;
    if (B.n_win >= 8) {
        w = (lid & 7) + 8 * ((lid >> 3) / per_win);
        idx = (lid >> 3) % per_win;
    } else {
        w = lid / per_win;
        idx = lid % per_win;
    }
    return w < B.n_win;
}

// The IMU factors and the sub-block mask of one keyframe pair, fetched ONCE per wave: in the many-window kernel right behind the
// walk, so that the reductions hide the two dependent round trips (not held across the walk: the Schur kernels have no register
// to spare there); in the few-window kernels where the block is written.  The structure build (vba_host_structure.h) lists every
// IMU edge of the problem under its pairs, so a list has no bound in general; a keyframe chain gives one factor per neighbour
// pair and one or two per diagonal pair.  The first two are resolved here; a longer list goes through the loops that read pimu
// per factor.
struct PairImu {
    int qb, n;               // first entry of the pair's (edge, role) list, number of entries
    int mask;                // pair_mask: the sub-blocks some tile of the factor reads (schur_write_block)
    const double *H0, *H1;   // information blocks of the first two factors (valid pointers whatever n is)
    int ro0, co0, ro1, co1;  // their row / column offsets: role bit0: a is keyframe j of the edge, bit1: b is keyframe j
};
DEVI PairImu pair_imu(const Batch& B, const WinDesc& d, int pr) {
    PairImu f;
    const int* pb = B.pimu_begin + d.pair0 + d.win + pr;
    f.qb = pb[0];
    f.n = pb[1] - f.qb;
    f.mask = B.pair_mask[d.pair0 + pr];
    f.H0 = f.H1 = B.imuH;
    f.ro0 = f.co0 = f.ro1 = f.co1 = 0;
    if (f.n > 0) {
        const int* e0 = B.pimu + 2 * (size_t)(d.pimu0 + f.qb);
        const int* e1 = e0 + ((f.n > 1) ? 2 : 0);   // (both entries requested together)
        const int k0 = e0[0], role0 = e0[1], k1 = e1[0], role1 = e1[1];
        f.H0 = B.imuH + VBA_IMUH * (size_t)(d.imu0 + k0);
        f.H1 = B.imuH + VBA_IMUH * (size_t)(d.imu0 + k1);
        f.ro0 = (role0 & 1) ? 15 : 0; f.co0 = (role0 & 2) ? 15 : 0;
        f.ro1 = (role1 & 1) ? 15 : 0; f.co1 = (role1 & 2) ? 15 : 0;
    }
    return f;
}

// A block with IMU terms or a diagonal block, at most two factors: PP = pdim and NT = lanes per pair are compile-time, so the
// entries of a lane are enumerated without a division, and every load an entry needs (the block value from LDS, H of both
// factors, var_act of its row and column) is requested before the first entry is formed -- one round trip for up to CH entries
// instead of one per load.  Each entry is formed exactly as the loop below forms it: blk or 0.0, + H in list order, the
// diagonal rule, the same store side.
template <int PP, int NT, bool DIAG>
DEVI void schur_write_block_imu(const Batch& B, const WinDesc& d, double lambda, int mask, const PairImu& f, int a, int b,
                                const double* blk, int t, int bstride) {
    constexpr int NE = PP * PP, TR = (NE + NT - 1) / NT, CH = (TR < 8) ? TR : 8;
    constexpr bool diag = DIAG;
    const int n = d.nS;
    const int* va = B.var_act + d.vec0;
    double* S = B.S + d.S0;
    // vpos(d, x, r) = (r < 6 ? pr_x : vb_x) + r
    const int pr_a = d.vp_pr0 + d.vp_prs * a, pr_b = d.vp_pr0 + d.vp_prs * b;
    const int vb_a = ((a < d.vp_h) ? d.vp_vb0 + d.vp_vbs * a : d.vp_vb1 - 9 * a) - 6;
    const int vb_b = ((b < d.vp_h) ? d.vp_vb0 + d.vp_vbs * b : d.vp_vb1 - 9 * b) - 6;
#pragma unroll
    for (int c0 = 0; c0 < TR; c0 += CH) {
        double bl[CH], h0[CH], h1[CH];
        int gr[CH], gc[CH], ar[CH], ac[CH], hi[CH];
#pragma unroll
        for (int i = 0; i < CH; i++) {
            bl[i] = h0[i] = h1[i] = 0.0;
            gr[i] = gc[i] = hi[i] = 0;
            ar[i] = ac[i] = 1;
            if (c0 + i >= TR) break;
            const int q0 = t + (c0 + i) * NT;
            const int q = (q0 < NE) ? q0 : 0;   // (a lane past the block's end requests entry 0 and stores nothing)
            const int r = q / PP, col = q % PP;
            gr[i] = ((r < 6) ? pr_a : vb_a) + r;
            gc[i] = ((col < 6) ? pr_b : vb_b) + col;
            hi[i] = r * 30 + col;
            bl[i] = blk[(r < 6 && col < 6) ? r * bstride + col : 0];
        }
        if (f.n > 0) {
            const double* H = f.H0 + f.ro0 * 30 + f.co0;
#pragma unroll
            for (int i = 0; i < CH; i++) if (c0 + i < TR) h0[i] = H[hi[i]];
        }
        if (f.n > 1) {
            const double* H = f.H1 + f.ro1 * 30 + f.co1;
#pragma unroll
            for (int i = 0; i < CH; i++) if (c0 + i < TR) h1[i] = H[hi[i]];
        }
        if (diag) {
#pragma unroll
            for (int i = 0; i < CH; i++) if (c0 + i < TR) { ar[i] = va[gr[i]]; ac[i] = va[gc[i]]; }
        }
#pragma unroll
        for (int i = 0; i < CH; i++) {
            if (c0 + i >= TR) break;
            const int q = t + (c0 + i) * NT;
            if (q >= NE) continue;
            const int r = q / PP, col = q % PP;
            if (!((mask >> ((r >= 6 ? 2 : 0) + (col >= 6 ? 1 : 0))) & 1)) continue;
            double s = (r < 6 && col < 6) ? bl[i] : 0.0;
            if (f.n > 0) s += h0[i];
            if (f.n > 1) s += h1[i];
            if (diag) {
                if (!ar[i] || !ac[i]) s = (r == col) ? 1.0 : 0.0;  // vertex outside the index mapping
                else if (r == col) s += lambda;                     // setLambda, block_solver.hpp:564-589
            }
            if (gr[i] >= gc[i]) S[(size_t)gr[i] * n + gc[i]] = s;
            else if (!diag) S[(size_t)gc[i] * n + gr[i]] = s;
        }
    }
}

// adds the IMU blocks, applies the active-set / damping rules and writes one pdim x pdim block of S (lower
// triangle only: the factorisation never reads above the diagonal)
// LD = landmark dimension of the caller (inverse-depth windows have pdim 15), NT = lanes per pair (64 or 16), DIAG: a == b
template <int LD, int NT, bool DIAG>
DEVI void schur_write_block(const Batch& B, const WinDesc& d, const WinCtrl& c, const PairImu& f, int pr, int a, int b,
                            const double* blk, int t, int bstride) {
    const int P = d.pdim, n = d.nS;
    constexpr bool diag = DIAG;
    const double lambda = (d.algo == 1) ? c.lambda : 0.0;
    const int qb = f.qb, qe = f.qb + f.n;
    const int* va = B.var_act + d.vec0;
    double* S = B.S + d.S0;
    // sub-blocks that no tile of the factor ever reads (structurally zero in L under the V/Bias-first order) are
    // not written at all: bit0 PRxPR, bit1 PRxVB, bit2 VBxPR, bit3 VBxVB (mask built with the tile lists at upload)
    const int mask = f.mask;
    if (mask == 0) return;   // nothing of this block is ever read (or it keeps the zero of the upload)
    if (mask == 1 && !diag && qb == qe) {  // only the 6x6 PR x PR sub-block lands in a tile the factor reads, no IMU term
        for (int q = t; q < 36; q += NT) {
            const int r = q / 6, col = q % 6;
            const int gr = vpos(d, a, r), gc = vpos(d, b, col);
            const double s = blk[r * bstride + col];
            if (gr >= gc) S[(size_t)gr * n + gc] = s;
            else S[(size_t)gc * n + gr] = s;
        }
        return;
    }
    if (f.n <= 2) {
        if (P == 15) { schur_write_block_imu<15, NT, DIAG>(B, d, lambda, mask, f, a, b, blk, t, bstride); return; }
        if (LD == 3 && P == 6) { schur_write_block_imu<6, NT, DIAG>(B, d, lambda, mask, f, a, b, blk, t, bstride); return; }
    }
    for (int q = t; q < P * P; q += NT) {   // more than two factors on the pair
        const int r = q / P, col = q % P;
        if (!((mask >> ((r >= 6 ? 2 : 0) + (col >= 6 ? 1 : 0))) & 1)) continue;
        double s = (r < 6 && col < 6) ? blk[r * bstride + col] : 0.0;
        for (int m = qb; m < qe; m++) {
            const int k = B.pimu[2 * (size_t)(d.pimu0 + m)], role = B.pimu[2 * (size_t)(d.pimu0 + m) + 1];
            const double* H = B.imuH + VBA_IMUH * (size_t)(d.imu0 + k);
            const int ro = (role & 1) ? 15 : 0, co = (role & 2) ? 15 : 0;  // bit0: a is j ; bit1: b is j
            s += H[(ro + r) * 30 + co + col];
        }
        const int gr = vpos(d, a, r), gc = vpos(d, b, col);
        if (diag) {
            if (!va[gr] || !va[gc]) s = (r == col) ? 1.0 : 0.0;  // vertex outside the index mapping
            else if (r == col) s += lambda;                       // setLambda, block_solver.hpp:564-589
        }
        if (gr >= gc) S[(size_t)gr * n + gc] = s;
        else if (!diag) S[(size_t)gc * n + gr] = s;
    }
}

// off-diagonal keyframe pairs (a < b).  A pair has ~90 items on average, far too few for a whole wave: four
// pairs share one wave, 16 lanes each (the 36-value reduction then costs 4 butterfly steps per FOUR pairs
// instead of 6 per pair, and every lane sees ~6 items instead of ~1.4).
// LD = landmark dimension (1: inverse depth, slot record 6 doubles; 3: XYZ, slot record 24 doubles)
// LP = lanes per pair: 64 (one pair per wave: small batches, latency) or 16 (four pairs per wave: throughput)
// Bi = [A | B_rot] of an EdgePRIDP from its 32-B record (P_c, s = sqrt(rho' w)) and the observer's rotation R_a:
// J_c = J_pi(P_c) R_cb, A = s J_c R_a^T, B_rot = -s J_c x t_a with t_a = R_cb^T (P_c - t_cb)   (k_lin2 phase B, g2otypes.cpp:139-145).
// All the reference items of the off-diagonal pairs need; the diagonal walk adds the weighted residual (rebuild_edge_res).
DEVI void rebuild_edge(const WinDesc& d, const double* Ra, const double (&rec)[VBA_EREC1], double* b0, double* b1) {
    const double Pc[3] = {rec[0], rec[1], rec[2]}, sc = rec[3];
    const double fx = d.K[0], fy = d.K[1];
    const double iz = 1.0 / Pc[2];
    const double Jp[6] = {fx * iz, 0.0, -Pc[0] * iz * fx * iz, 0.0, fy * iz, -Pc[1] * iz * fy * iz};
    double Jc[6];
#pragma unroll
    for (int rr = 0; rr < 2; rr++)
#pragma unroll
        for (int k = 0; k < 3; k++)
            Jc[3 * rr + k] = Jp[3 * rr] * d.Rcb[k] + Jp[3 * rr + 1] * d.Rcb[3 + k] + Jp[3 * rr + 2] * d.Rcb[6 + k];
    const double pm[3] = {Pc[0] - d.tcb[0], Pc[1] - d.tcb[1], Pc[2] - d.tcb[2]};
    double ta[3];
    mtv3(d.Rcb, pm, ta);
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
        double* bb = rr ? b1 : b0;
#pragma unroll
        for (int k = 0; k < 3; k++)
            bb[k] = sc * (Jc[3 * rr] * Ra[3 * k] + Jc[3 * rr + 1] * Ra[3 * k + 1] + Jc[3 * rr + 2] * Ra[3 * k + 2]);
        const double j0 = Jc[3 * rr], j1 = Jc[3 * rr + 1], j2 = Jc[3 * rr + 2];
        bb[3] = -sc * (j1 * ta[2] - j2 * ta[1]);
        bb[4] = -sc * (j2 * ta[0] - j0 * ta[2]);
        bb[5] = -sc * (j0 * ta[1] - j1 * ta[0]);
    }
}
// The weighted residual s r the linearisation formed for this record (idp_edge_wres, the same function), from the record and the
// pixel of its observation.  The record used to carry it; what it held where s = 0 was
//   an outlier edge (level != 0):  r = 0.  The select gives 0 again.
//   a fixed observer:              s r of the edge, not 0.  But there Bi = s (...) is +-0 in every entry, so its term of
//                                  b_p = -(b0 r0 + b1 r1) was +-0 with that r and is +-0 with r = 0, and a sum that starts at +0
//                                  is left unchanged, bit for bit, by adding either zero.
// A select, not a product with s: where s = 0 nothing vouches for P_c (an outlier behind the camera, z = 0), and 0 * inf is a NaN.
DEVI void rebuild_edge_res(const WinDesc& d, const double (&rec)[VBA_EREC1], double u, double v, double& r0, double& r1) {
    const double Pc[3] = {rec[0], rec[1], rec[2]}, sc = rec[3];
    double w0, w1;
    idp_edge_wres(d, Pc, u, v, sc, w0, w1);
    r0 = (sc != 0.0) ? w0 : 0.0;
    r1 = (sc != 0.0) ? w1 : 0.0;
}

// The walk of an off-diagonal pair over its items [ib, ie), lane l16 of the pair's LP lanes: the lane's sums, 6x6 row-major.  Every
// item is the Schur term of one landmark seen from both keyframes -- -U_a U_b^T (inverse depth: U = W sqrt(D^-1), 6x1) or
// -W_a Sigma W_b^T (XYZ: W 6x3 from the slot records, Sigma = (H_ll + lambda I)^-1 from the landmark's record).
// (A walk sums in an array of its own, declared first, and hands it over at its end.  Summing through the reference the compiler
// promotes the sums to registers only once the walk is inlined, behind its other loop variables, and the kernel comes out in
// another instruction order.)
// Inverse depth (Gauss-Newton): the items [im, ie) involve the landmark's reference keyframe and are walked a second time.
template <int LP>
DEVI void schur_off_walk_idp(const Batch& B, const WinDesc& d, int a, int b, int ib, int im, int ie, int l16, double (&out)[36]) {
    double acc[36];
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = 0;
    constexpr int SS = VBA_SLOT;
    const double* slots = B.slot + SS * (size_t)(d.obs0 + d.pt0);
    const int2* items = reinterpret_cast<const int2*>(B.items) + d.item0;
    // two items per lane and trip, their four records requested together: the gather is bound by the latency of its dependent
    // fetches (occupancy experiment: 3 / 2 / 1 waves per SIMD = 107 / 128 / 179 ms), so a wave keeps twice as many in flight.
    // Every lane still takes its items in the same order: the same sums.
    int2 n0 = make_int2(0, 0), n1 = make_int2(0, 0);
    if (ib + l16 < ie) n0 = items[ib + l16];
    if (ib + l16 + LP < ie) n1 = items[ib + l16 + LP];
    for (int it = ib + l16; it < ie; it += 2 * LP) {
        const int2 i0 = n0;
        const bool two = it + LP < ie;
        const int2 i1 = two ? n1 : n0;
        if (it + 2 * LP < ie) n0 = items[it + 2 * LP];
        if (it + 3 * LP < ie) n1 = items[it + 3 * LP];
        const double *qa0 = slots + SS * (size_t)i0.x, *qb0 = slots + SS * (size_t)i0.y;
        const double *qa1 = slots + SS * (size_t)i1.x, *qb1 = slots + SS * (size_t)i1.y;
        double UA0[6], UB0[6], UA1[6], UB1[6];
#pragma unroll
        for (int i = 0; i < 6; i++) { UA0[i] = qa0[i]; UB0[i] = qb0[i]; UA1[i] = qa1[i]; UB1[i] = qb1[i]; }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++) acc[6 * i + j] -= UA0[i] * UB0[j];
        if (two) {
#pragma unroll
            for (int i = 0; i < 6; i++)
#pragma unroll
                for (int j = 0; j < 6; j++) acc[6 * i + j] -= UA1[i] * UB1[j];
        }
    }
    // the items [im, ie) involve the landmark's reference keyframe and also carry a direct H_pp term: the edge of the
    // other keyframe adds Br^T Bi (a = ref) or Bi^T Br (b = ref), with Br = [-A | A N0] rebuilt from the record's
    // A = Bi[:, 0:3].  Their own loop: the walk above stays free of this branch and of its loads.
    // (indices one trip ahead, as above: item -> landmark of its reference record -> landmark is two dependent fetches otherwise)
    int2 rnx = make_int2(0, 0);
    int rnx_lm = 0;
    if (im + l16 < ie) {
        rnx = items[im + l16];
        rnx_lm = B.rec_lm[d.pt0 + ((rnx.x >= d.n_obs) ? rnx.x : rnx.y) - d.n_obs];
    }
    for (int it = im + l16; it < ie; it += LP) {
        const int2 itm = rnx;
        const size_t gp = d.pt0 + rnx_lm;   // the landmark of the reference record
        if (it + LP < ie) {
            rnx = items[it + LP];
            rnx_lm = B.rec_lm[d.pt0 + ((rnx.x >= d.n_obs) ? rnx.x : rnx.y) - d.n_obs];
        }
        const int sa = itm.x, sb = itm.y;
        const bool a_ref = sa >= d.n_obs;
        const double* re = B.erec + VBA_EREC1 * (size_t)(d.obs0 + (a_ref ? sb : sa));
        const double rho = B.pt[3 * gp], xb = B.pt[3 * gp + 1], yb = B.pt[3 * gp + 2];
        const double* Ro = B.kfR + 12 * (size_t)(d.kf0 + (a_ref ? b : a));  // the observer's rotation
        double rec[VBA_EREC1], bi0[6], bi1[6], br0[6], br1[6];
#pragma unroll
        for (int i = 0; i < VBA_EREC1; i++) rec[i] = re[i];   // (one aligned 32-byte record)
        rebuild_edge(d, Ro, rec, bi0, bi1);   // (the rotation is read where it is used: nine registers fewer in flight)
        {   // N0 = R0 hat(b0) of the landmark in its reference keyframe, as the linearisation forms it (lin2_body, phase A): the
            // landmark has not moved since (the update comes after the solve).  Br = [-A | A N0], both rows, then N0 is dead.
            const double* C0 = B.kfR + 12 * (size_t)(d.kf0 + (a_ref ? a : b));
            double dd, c0[3], b0[3], Xw[3], Hb[9], N0[9];
            idp_point_world(d, C0, rho, xb, yb, dd, c0, b0, Xw);
            hat3(b0, Hb);
            mm3(C0, Hb, N0);
#pragma unroll
            for (int k = 0; k < 3; k++) {
                br0[k] = -bi0[k]; br1[k] = -bi1[k];
                br0[3 + k] = bi0[0] * N0[k] + bi0[1] * N0[3 + k] + bi0[2] * N0[6 + k];
                br1[3 + k] = bi1[0] * N0[k] + bi1[1] * N0[3 + k] + bi1[2] * N0[6 + k];
            }
        }
#pragma unroll
        for (int h = 0; h < 2; h++) {
            const double* bi = h ? bi1 : bi0;
            const double* br = h ? br1 : br0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double x = a_ref ? br[i] : bi[i];
#pragma unroll
                for (int j = 0; j < 6; j++) acc[6 * i + j] += x * (a_ref ? bi[j] : br[j]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 36; i++) out[i] = acc[i];
}
// XYZ (Levenberg-Marquardt): one item per lane and trip, Sigma fetched through the landmark of the item's first slot
template <int LP>
DEVI void schur_off_walk_xyz(const Batch& B, const WinDesc& d, int ib, int ie, int l16, double (&out)[36]) {
    double acc[36];
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = 0;
    constexpr int SS = VBA_SLOT3;
    const double* slots = B.slot + SS * (size_t)(d.obs0 + d.pt0);
    const int2* items = reinterpret_cast<const int2*>(B.items) + d.item0;
    int2 nxt = make_int2(0, 0);
    int nxt_lm = 0;
    if (ib + l16 < ie) {
        nxt = items[ib + l16];
        nxt_lm = B.slot_lm[d.obs0 + nxt.x];
    }
    for (int it = ib + l16; it < ie; it += LP) {
        const int2 itm = nxt;  // indices were fetched one trip ahead: one dependent round trip per item, not two
        const int lm = nxt_lm;
        if (it + LP < ie) {
            nxt = items[it + LP];
            nxt_lm = B.slot_lm[d.obs0 + nxt.x];
        }
        const double* qa = slots + SS * (size_t)itm.x;
        const double* qb = slots + SS * (size_t)itm.y;
        double UA[18], UB[18];
#pragma unroll
        for (int i = 0; i < 18; i++) { UA[i] = qa[i]; UB[i] = qb[i]; }
        const double* sg = B.prec + VBA_PREC * (size_t)(d.pt0 + lm) + 10;
        const double s00 = sg[0], s01 = sg[1], s02 = sg[2], s11 = sg[3], s12 = sg[4], s22 = sg[5];
#pragma unroll
        for (int i = 0; i < 6; i++) {   // UA <- W_a Sigma
            const double w0 = UA[3 * i], w1 = UA[3 * i + 1], w2 = UA[3 * i + 2];
            UA[3 * i] = w0 * s00 + w1 * s01 + w2 * s02;
            UA[3 * i + 1] = w0 * s01 + w1 * s11 + w2 * s12;
            UA[3 * i + 2] = w0 * s02 + w1 * s12 + w2 * s22;
        }
#pragma unroll
        for (int i = 0; i < 6; i++)
#pragma unroll
            for (int j = 0; j < 6; j++)
#pragma unroll
                for (int l = 0; l < 3; l++) acc[6 * i + j] -= UA[3 * i + l] * UB[3 * j + l];
    }
#pragma unroll
    for (int i = 0; i < 36; i++) out[i] = acc[i];
}

// One off-diagonal pair per LP lanes: the pair and its item range, the walk of its landmark type, then the sums and the block
template <int LD, int LP>
DEVI void schur_off_body(const Batch& B, int max_quads, double* blk4, int w_in = -1, int quad_in = 0) {
    int w = w_in, quad = quad_in;
    if (w_in < 0 && !schur_map(B, max_quads, w, quad)) return;
    const WinDesc& d = B.desc[w];
    const WinCtrl& c = B.ctrl[w];
    if (!win_on(d, c)) return;
    constexpr int NG = 64 / LP;  // pairs per wave
    const int t = threadIdx.x, g = t / LP, l16 = t % LP;
    // off-diagonal pairs only: enumerate them through the host-built list of their pair indices
    const int n_off = d.n_pairs - d.n_free;
    const int oi = quad * NG + g;
    const bool have = oi < n_off;
    int pr = 0, a = 0, b = 0, ib = 0, im = 0, ie = 0;
    if (have) {
        pr = B.off_pair[d.pair0 + oi];
        a = B.pair_a[d.pair0 + pr];
        b = B.pair_b[d.pair0 + pr];
        ib = B.item_begin[d.pair0 + d.win + pr];
        ie = B.item_begin[d.pair0 + d.win + pr + 1];
        im = (LD == 1) ? B.item_mid[d.pair0 + d.win + pr] : ie;
    }
    double acc[36];
    if constexpr (LD == 1) schur_off_walk_idp<LP>(B, d, a, b, ib, im, ie, l16, acc);
    else schur_off_walk_xyz<LP>(B, d, ib, ie, l16, acc);
    PairImu f = {};
    if (LP == 16 && have) f = pair_imu(B, d, pr);   // (one pair per wave, the few-window kernels: at the write -- the registers would cost a wave per SIMD)
    // fixed-order sums inside each LP-lane group (skipped when no pair of the wave has an item: most keyframe pairs of a window
    // share no landmark, and in distance order they fill whole waves)
    if (__ballot(ib < ie) != 0ull) {
#pragma unroll
        for (int i = 0; i < 36; i++) acc[i] = (LP == 16) ? row16_sum(acc[i]) : wave64_sum(acc[i]);
    }
    double* blk = blk4 + g * 36;
    if (l16 == 0) {
#pragma unroll
        for (int i = 0; i < 36; i++) blk[i] = acc[i];
    }
    __syncthreads();
    if (LP != 16 && have) f = pair_imu(B, d, pr);
    if (have) schur_write_block<LD, LP, false>(B, d, c, f, pr, a, b, blk, l16, 6);
}
__global__ void __launch_bounds__(64, 2) k_schur_off(Batch B, int max_quads) {   // (the split form, VBA_SCHUR_SPLIT: not the default path)
    __shared__ double blk4[4 * 36];
    schur_off_body<1, 16>(B, max_quads, blk4);
}
__global__ void __launch_bounds__(64) k_schur_off_w(Batch B, int max_quads) {  // one pair per wave
    __shared__ double blk4[4 * 36];
    schur_off_body<1, 64>(B, max_quads, blk4);
}
__global__ void __launch_bounds__(64) k_schur_off3(Batch B, int max_quads) {
    __shared__ double blk4[4 * 36];
    schur_off_body<3, 16>(B, max_quads, blk4);
}
__global__ void __launch_bounds__(64) k_schur_off3_w(Batch B, int max_quads) {
    __shared__ double blk4[4 * 36];
    schur_off_body<3, 64>(B, max_quads, blk4);
}

// diagonal pairs (a,a): every slot of keyframe a; also the reduced rhs (block_solver.hpp:436-439), the
// unreduced b_p and the H_pp diagonal (LM's lambda init)
// EARLY: the pair's IMU list is fetched ahead of the reductions (the many-window kernel; in the few-window kernels the registers
// this holds cost a wave per SIMD)
template <int LD, bool EARLY = false>
DEVI void schur_diag_body(const Batch& B, int max_free, int hd_pass, double* blk, double* sh_r, double* sh_b, double* sh_h,
                          int w_in = -1, int a_in = 0) {
    int w = w_in, a = a_in;
    if (w_in < 0 && !schur_map(B, max_free, w, a)) return;
    const WinDesc& d = B.desc[w];
    const WinCtrl& c = B.ctrl[w];
    // hd_pass: LM's pre-trial pass for computeLambdaInit -- part of the "outer" slot, which a window that still owes a trial skips
    if (hd_pass ? (!c.active || c.lm_need_trial) : !win_on(d, c)) return;
    if (a >= d.n_free) return;
    const int t = threadIdx.x;
    const int pr = a * d.n_free - a * (a - 1) / 2;  // index of pair (a,a)
    double acc[21], rhs[6], bp[6], hd[6];  // the block is symmetric: upper triangle only, row-major (i <= j)
#pragma unroll
    for (int i = 0; i < 21; i++) acc[i] = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) rhs[i] = bp[i] = hd[i] = 0;
    // The walk: each lane's sums over the items of the pair, separate per landmark type.  (The two walks are branches here and not
    // functions of their own, as the off-diagonal ones are: compiled on their own ahead of inlining they come out differently --
    // another schedule in k_schur_diag and the fused kernels, another operand order of the Sigma products in k_schur_diag3.)
    if constexpr (LD == 1) {
        // ---- inverse depth (Gauss-Newton): three index ranges, run records, lm_sd, edge records rebuilt by their reader
        constexpr int SS = VBA_SLOT;
        // the items of the diagonal pair are the records of keyframe a: its slot records (observer) and, for inverse-depth
        // landmarks, the landmark records it is the reference keyframe of -- two index ranges, no list
        const int* kseg = B.kf_seg + d.kf0 + d.win;
        const int s0 = kseg[a], n_o = kseg[a + 1] - s0;
        const int r0s = B.ref_seg[d.kf0 + d.win + a], n_r = B.ref_seg[d.kf0 + d.win + a + 1] - r0s;
        const double* slots = B.slot + SS * (size_t)(d.obs0 + d.pt0);
        double Ra[9];  // rotation of keyframe a (the observer of every non-reference item of its diagonal pair)
        {
            const double* Ca = B.kfR + 12 * (size_t)(d.kf0 + a);
#pragma unroll
            for (int i = 0; i < 9; i++) Ra[i] = Ca[i];
        }
        // inverse depth: a third range of items -- the run records of this keyframe's reference terms (G0: 21, g0: 6 summed over runs of
        // landmarks by k_lin2, phase E).
        const int* pfb = B.pref_begin + d.kf0 + d.win;
        const int m0 = pfb[a];
        const int n_run = pfb[a + 1] - m0;
        const int* run_list = B.pref_list + d.pt0 + m0;
        // inverse depth: every item of the walk reaches a record through one index -- a slot or reference record the (sqrt(Dinv), beta) of
        // its landmark (lm_sd: beta lives with the landmark, not in the slot record), a run item its run record.  A lane holds the index of
        // its NEXT item, fetched one trip ahead (all three index reads are contiguous across the wave): inside a trip beta and the run
        // record are single dependent fetches, beside the slot and the edge record, and not two in sequence.
        const int n_items = n_o + n_r + n_run;
        // (the offsets of the three index ranges as scalars, the element indices unsigned: scalar base + 32-bit lane offset addressing.
        // As 64-bit lane addresses they cost the fused kernels their register budget: k_schur_all 12 B of scratch, k_schur_all_w a wave)
        const int o_s = __builtin_amdgcn_readfirstlane(d.obs0 + s0), o_r = __builtin_amdgcn_readfirstlane(d.pt0 + r0s - n_o);
        const int o_n = __builtin_amdgcn_readfirstlane(n_o + n_r), o_p = __builtin_amdgcn_readfirstlane(d.pt0);
        auto item_index = [&](int it) {
            return (it < n_o) ? B.slot_lm[(unsigned)(o_s + it)] : (it < o_n) ? B.rec_lm[(unsigned)(o_r + it)] : run_list[(unsigned)(it - o_n)];
        };
        // likewise the records (inverse depth): the slot records from the window's first one, the keyframe's edge records and the pixels
        // beside them (item `it` < n_o sits at record o_s + it) from the start of the keyframe's segment -- a scalar base + the lane's BYTE
        // offset, formed in 32 bits (check_window refuses a window whose slot records pass 2^32 bytes; the other two are smaller).  With
        // 64-bit lane addresses for the three the walk does not fit the register budget of the fused kernels
        const char* e_base = reinterpret_cast<const char*>(B.erec + VBA_EREC1 * (size_t)o_s);
        const char* u_base = reinterpret_cast<const char*>(B.obs_uvk + 2 * (size_t)o_s);
        int nxt_idx = 0;
        if (t < n_items) nxt_idx = item_index(t);
        for (int it = t; it < n_items; it += 64) {
            const int idx = nxt_idx;
            if (it + 64 < n_items) nxt_idx = item_index(it + 64);
            if (it >= n_o + n_r) {   // a run record: direct terms only
                const double* pr_ = B.prec + VBA_PREC * (size_t)(d.pt0 + idx);
#pragma unroll
                for (int g = 0; g < 21; g++) acc[g] += pr_[g];
                // (no H_pp diagonal here: it feeds Levenberg-Marquardt's lambda init, and inverse-depth windows run Gauss-Newton)
#pragma unroll
                for (int i = 0; i < 6; i++) bp[i] += pr_[21 + i];
                continue;
            }
            const int sa = (it < n_o) ? s0 + it : d.n_obs + r0s + (it - n_o);
            const double* qa = reinterpret_cast<const double*>(reinterpret_cast<const char*>(slots) + (unsigned)sa * (unsigned)(SS * 8));
            double U[6], beta[1];   // U = W_a sqrt(D^-1) from the record, beta of its landmark
#pragma unroll
            for (int i = 0; i < 6; i++) U[i] = qa[i];
            beta[0] = B.lm_sd[(unsigned)(o_p + idx)].y;
            if (sa >= d.n_obs) {
                // (a landmark record of this keyframe: its direct terms come summed over runs of landmarks, below)
            } else {
                const double* ra = reinterpret_cast<const double*>(e_base + (unsigned)it * (unsigned)(VBA_EREC1 * 8));
                double r0 = 0.0, r1 = 0.0;
                double b0[6], b1[6];
                // slot record, 32-B edge record and pixel all sit at record position sa = s0 + it: three contiguous reads across the wave
                double rec[VBA_EREC1];
#pragma unroll
                for (int i = 0; i < VBA_EREC1; i++) rec[i] = ra[i];
                const double2 uv = *reinterpret_cast<const double2*>(u_base + (unsigned)it * 16u);
                rebuild_edge_res(d, rec, uv.x, uv.y, r0, r1);
                rebuild_edge(d, Ra, rec, b0, b1);
                int gi = 0;
#pragma unroll
                for (int i = 0; i < 6; i++) {
#pragma unroll
                    for (int j = i; j < 6; j++) acc[gi++] += b0[i] * b0[j] + b1[i] * b1[j];
                    bp[i] += -(b0[i] * r0 + b1[i] * r1);
                }
            }
            // (the one-trip loops over the landmark's single dimension stay: written flat, the last row's two products swap places
            // in the compiled walk)
            int gi = 0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
                for (int l = 0; l < 1; l++) rhs[i] -= U[i + l] * beta[l];   // U beta
#pragma unroll
                for (int j = i; j < 6; j++) {
#pragma unroll
                    for (int l = 0; l < 1; l++) acc[gi] -= U[i + l] * U[j + l];
                    gi++;
                }
            }
        }
    } else {
        // ---- XYZ (Levenberg-Marquardt): the slot records of keyframe a, one index range.  The direct terms sum Bi^T Bi and b_p do
        // not depend on the damping, so the pass that opens an outer iteration (hd_pass) takes them from the edge records ONCE and
        // parks them per keyframe (kf_dir); the trials then read the slot records U(lambda) only -- 192 B instead of 384 B per
        // record and trial
        constexpr int SS = VBA_SLOT3;
        const int* kseg = B.kf_seg + d.kf0 + d.win;
        const int s0 = kseg[a], n_o = kseg[a + 1] - s0;
        const double* slots = B.slot + SS * (size_t)(d.obs0 + d.pt0);
        const bool want_u = !hd_pass, want_dir = hd_pass;
        for (int it = t; it < n_o; it += 64) {
            const int sa = s0 + it;
            const double* qa = slots + SS * (size_t)sa;
            double UA[18], UB[18], beta[3];   // UA = W_a Sigma, UB = W_a, beta = t = Sigma b_l
#pragma unroll
            for (int i = 0; i < 18; i++) UB[i] = want_u ? qa[i] : 0.0;
            // (the pass that opens an outer iteration reads no Sigma at all: the record may hold anything there -- after a failed
            // solve of the window that occupied this place before, a NaN, and 0 * NaN would poison the whole keyframe block)
            const double* sg = B.prec + VBA_PREC * (size_t)(d.pt0 + (want_u ? B.slot_lm[d.obs0 + sa] : 0)) + 10;
            double s00 = 0.0, s01 = 0.0, s02 = 0.0, s11 = 0.0, s12 = 0.0, s22 = 0.0;
            if (want_u) { s00 = sg[0]; s01 = sg[1]; s02 = sg[2]; s11 = sg[3]; s12 = sg[4]; s22 = sg[5]; }
#pragma unroll
            for (int l = 0; l < 3; l++) beta[l] = want_u ? sg[6 + l] : 0.0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                const double w0 = UB[3 * i], w1 = UB[3 * i + 1], w2 = UB[3 * i + 2];
                UA[3 * i] = w0 * s00 + w1 * s01 + w2 * s02;
                UA[3 * i + 1] = w0 * s01 + w1 * s11 + w2 * s12;
                UA[3 * i + 2] = w0 * s02 + w1 * s12 + w2 * s22;
            }
            if (want_dir) {
                const double* ra = B.erec + VBA_EREC * (size_t)(d.obs0 + sa);
                double b0[6], b1[6];
#pragma unroll
                for (int i = 0; i < 6; i++) { b0[i] = ra[i]; b1[i] = ra[6 + i]; }   // XYZ edge record: Bi (12), g (6)
                int gi = 0;
#pragma unroll
                for (int i = 0; i < 6; i++) {
#pragma unroll
                    for (int j = i; j < 6; j++) acc[gi++] += b0[i] * b0[j] + b1[i] * b1[j];
                    bp[i] += ra[12 + i];
                }
            }
            int gi = 0;
#pragma unroll
            for (int i = 0; i < 6; i++) {
#pragma unroll
                for (int l = 0; l < 3; l++) rhs[i] -= UB[3 * i + l] * beta[l];   // W_a t
#pragma unroll
                for (int j = i; j < 6; j++) {
#pragma unroll
                    for (int l = 0; l < 3; l++) acc[gi] -= UA[3 * i + l] * UB[3 * j + l];
                    gi++;
                }
            }
        }
    }
    PairImu f = {};
    if (EARLY) f = pair_imu(B, d, pr);
#pragma unroll
    for (int i = 0; i < 21; i++) acc[i] = wave_sum(acc[i]);
#pragma unroll
    for (int i = 0; i < 6; i++) { rhs[i] = wave_sum(rhs[i]); bp[i] = wave_sum(bp[i]); }
    if (LD != 1) {
        double* kd = B.kf_dir + 32 * (size_t)(d.kf0 + a);
        if (hd_pass) {
            if (t == 0) {
#pragma unroll
                for (int g = 0; g < 21; g++) kd[g] = acc[g];
#pragma unroll
                for (int i = 0; i < 6; i++) kd[21 + i] = bp[i];
            }
            hd[0] = acc[0]; hd[1] = acc[6]; hd[2] = acc[11]; hd[3] = acc[15]; hd[4] = acc[18]; hd[5] = acc[20];
        } else {
#pragma unroll
            for (int g = 0; g < 21; g++) acc[g] += kd[g];
#pragma unroll
            for (int i = 0; i < 6; i++) bp[i] = kd[21 + i];
        }
    }
    const int P = d.pdim;
    for (int q = t; q < P * P; q += 64) blk[q] = 0.0;
    __syncthreads();
    if (t == 0) {
        int gi = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
#pragma unroll
            for (int j = i; j < 6; j++) { blk[i * P + j] = acc[gi]; blk[j * P + i] = acc[gi]; gi++; }
            sh_r[i] = rhs[i]; sh_b[i] = bp[i]; sh_h[i] = hd[i];
        }
    }
    __syncthreads();
    if (!EARLY) f = pair_imu(B, d, pr);
    // the rows of the right-hand side: their IMU terms and var_act are requested here, ahead of the block's loads and stores
    double hb0 = 0.0, hh0 = 0.0, hb1 = 0.0, hh1 = 0.0;
    int gr = 0, act_i = 0;
    if (t < P) {
        gr = vpos(d, a, t);
        act_i = B.var_act[d.vec0 + gr];
        if (f.n > 0) { hb0 = f.H0[900 + f.ro0 + t]; hh0 = f.H0[(f.ro0 + t) * 30 + f.ro0 + t]; }
        if (f.n > 1) { hb1 = f.H1[900 + f.ro1 + t]; hh1 = f.H1[(f.ro1 + t) * 30 + f.ro1 + t]; }
    }
    if (!hd_pass) schur_write_block<LD, 64, true>(B, d, c, f, pr, a, a, blk, t, P);   // (the hd pass only feeds lambda init and b_p)
    if (t < P) {
        double s = 0.0, sb = 0.0, h = 0.0;
        if (t < 6) { s = sh_r[t]; sb = sh_b[t]; h = sh_h[t]; }
        if (f.n > 0) { sb += hb0; h += hh0; }
        if (f.n > 1) { sb += hb1; h += hh1; }
        for (int m = f.qb + 2; m < f.qb + f.n; m++) {   // more than two factors on the keyframe
            const int k = B.pimu[2 * (size_t)(d.pimu0 + m)], role = B.pimu[2 * (size_t)(d.pimu0 + m) + 1];
            const double* H = B.imuH + VBA_IMUH * (size_t)(d.imu0 + k);
            const int ro = (role & 1) ? 15 : 0;
            sb += H[900 + ro + t];
            h += H[(ro + t) * 30 + ro + t];
        }
        const bool act = act_i != 0;
        (B.vec + d.vec0)[gr] = act ? (sb + s) : 0.0;            // reduced rhs = b_p - sum W Dinv b_l
        (B.bpose + 2 * (size_t)d.vec0)[gr] = act ? sb : 0.0;        // unreduced b_p (LM computeScale)
        if (LD == 1 || hd_pass) (B.bpose + 2 * (size_t)d.vec0)[d.nS + gr] = act ? h : 0.0;  // H_pp diagonal (LM computeLambdaInit)
    }
}
__global__ void __launch_bounds__(64) k_schur_diag(Batch B, int max_free) {
    __shared__ double blk[15 * 15 + 16];
    __shared__ double sh_r[6], sh_b[6], sh_h[6];
    schur_diag_body<1>(B, max_free, 0, blk, sh_r, sh_b, sh_h);
}
// Both Schur kernels of the inverse-depth variant in ONE launch, a window's diagonal pairs right before its off-diagonal
// ones: they read the same slot and edge records, which are then still in the XCD's L2 for the second reader.
__global__ void __launch_bounds__(64, 3) k_schur_all(Batch B, int max_free, int max_quads) {
    __shared__ double blk[15 * 15 + 16];
    __shared__ double sh_r[6], sh_b[6], sh_h[6];
    int w, idx;
    if (!schur_map(B, max_free + max_quads, w, idx)) return;
    w = __builtin_amdgcn_readfirstlane(w); idx = __builtin_amdgcn_readfirstlane(idx);
    if (idx < max_free) schur_diag_body<1, true>(B, max_free, 0, blk, sh_r, sh_b, sh_h, w, idx);
    else schur_off_body<1, 16>(B, max_quads, blk, w, idx - max_free);
}
// the same for fewer than 8 windows: one off-diagonal pair per wave (latency), still one launch
__global__ void __launch_bounds__(64) k_schur_all_w(Batch B, int max_free, int max_offp) {
    __shared__ double blk[15 * 15 + 16];
    __shared__ double sh_r[6], sh_b[6], sh_h[6];
    int w, idx;
    if (!schur_map(B, max_free + max_offp, w, idx)) return;
    if (idx < max_free) schur_diag_body<1>(B, max_free, 0, blk, sh_r, sh_b, sh_h, w, idx);
    else schur_off_body<1, 64>(B, max_offp, blk, w, idx - max_free);
}
__global__ void __launch_bounds__(64) k_schur_diag3(Batch B, int max_free, int hd_pass) {
    __shared__ double blk[15 * 15 + 16];
    __shared__ double sh_r[6], sh_b[6], sh_h[6];
    schur_diag_body<3>(B, max_free, hd_pass, blk, sh_r, sh_b, sh_h);
}
