// vba_factor.h -- factorisation of the reduced system on 32x32 tiles, with the forward substitution riding along: the
// right-looking step (k_chol_step), its few-window form (k_chol_step4) and the left-looking form for large batches (k_chol_*_ll*).
// Reads S, vec and the tile lists of the symbolic factorisation (tl_*); writes Lf, yv, dvec, winv and WinCtrl::chol_fail.
// Needs vba_batch.h.
#pragma once
#include "vba_batch.h"

// ------------------------------------------------------------------------------------------------
// Reduced-system factorisation S = L L^T on 32x32 tiles, right-looking, ONE launch per block column:
// every workgroup (one wave) of step k owns one tile pair (I,J) of the trailing update and redoes, on its
// own, the little work it depends on -- POTRF of the diagonal tile (registers + v_readlane broadcasts, no
// LDS round trips on the critical path) and the triangular solves of the two panel tiles L_Ik, L_Jk -- then
// applies C_IJ -= L_Ik L_Jk^T with v_mfma_f64_16x16x4_f64.  No inter-workgroup dependency inside a launch.
// The right-hand side rides along as one more row of the panel solve (forward substitution for free).
// Tiles that are structurally zero in L (V/Bias-first ordering) are not in the lists and never touched.
// Restates LinearSolverEigen::solve (linear_solver_eigen.h:94-124) on the dense reduced system.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) k_chol_step(Batch B, int k) {
    __shared__ double XI[32 * 34];   // first holds L_kk (stride 33) for the panel solves, then X_I (stride 34)
    __shared__ double XJ[32 * 34];
    __shared__ double rd[32];
    double* Lk = XI;
    const int w = blockIdx.y;
    const WinDesc& d = B.desc[w];
    WinCtrl& c = B.ctrl[w];
    if (!win_on(d, c)) return;
    if (k >= d.nb || k < d.nc) return;   // (columns [0, nc): k_chol_chain)
    const int* sb = B.tl_step_begin + d.tl_step0;
    const int npair = sb[k + 1] - sb[k];
    const int bx = blockIdx.x;
    if (bx >= (npair > 0 ? npair : 1)) return;
    const bool has_pair = bx < npair;
    int I = 0, J = 0;
    if (has_pair) {
        const int v = B.tl_pairs[d.tl_pair0 + sb[k] + bx];
        I = v >> 16;
        J = v & 0xffff;
    }
    const int lane = threadIdx.x, r = lane & 31, hi = lane >> 5;
    const int n = d.nS;
    double* S = B.S + d.S0;
    double* Lf = B.Lf + d.S0;
    double* vec = B.vec + d.vec0;
    double* yv = B.yv + d.vec0;
    const size_t dk = (size_t)k * 32;
    const bool diagp = has_pair && (I == J);
    const bool rhs_lane = (!has_pair || diagp) && lane == 32;
    const bool row_act = has_pair && (hi == 0 || !diagp);
    // panel rows first: their loads are in flight while the diagonal tile is factored
    double x[32];
    {
        const double* src = row_act ? (S + ((size_t)(hi ? J : I) * 32 + r) * n + dk) : (vec + dk);
        const bool ld = row_act || rhs_lane;
#pragma unroll
        for (int q = 0; q < 32; q++) x[q] = ld ? src[q] : 0.0;
    }
    double a[32];
    const double* arow = S + (dk + r) * n + dk;
#pragma unroll
    for (int q = 0; q < 32; q++) a[q] = (q <= r) ? arow[q] : 0.0;
    // the trailing tile C_IJ is requested now as well: it arrives while the diagonal tile is factored and the panels solved
    const int l15 = lane & 15, l4 = lane >> 4;
    d4_t cacc[2][2];
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++) {
            const double* C = S + ((size_t)I * 32 + 16 * ti) * n + (size_t)J * 32 + 16 * tj;
#pragma unroll
            for (int i = 0; i < 4; i++) cacc[ti][tj][i] = has_pair ? C[(size_t)(l4 + 4 * i) * n + l15] : 0.0;
        }
    // L D L^T of the diagonal tile (unit lower L, D on the diagonal), as Eigen's SimplicialLDLT does: negative
    // pivots are fine, only an exactly zero / non-finite pivot fails (linear_solver_eigen.h:105-111)
    bool bad = false;
    double rdiag = 1.0;  // 1 / d_r of this lane's row
#pragma unroll
    for (int cc = 0; cc < 32; cc++) {
        const double piv = rl64(a[cc], cc);
        bad = bad || (piv == 0.0) || !isfinite(piv);
        double y = __builtin_amdgcn_rcp(piv);  // v_rcp_f64 + two Newton steps: full double accuracy
        y = y * (2.0 - piv * y);
        y = y * (2.0 - piv * y);
        const double u = a[cc];                 // a_{r,cc} before the division = l_{r,cc} d_cc
        const double l = u * y;
        rdiag = (r == cc) ? y : rdiag;
        a[cc] = (r == cc) ? piv : l;
#pragma unroll
        for (int c2 = cc + 1; c2 < 32; c2++) a[c2] -= l * rl64(u, c2);
    }
    if (hi == 0) {
#pragma unroll
        for (int q = 0; q < 32; q++) Lk[r * 33 + q] = (q <= r) ? a[q] : 0.0;
        rd[r] = rdiag;
        if (bx == 0) {
            double* lrow = Lf + (dk + r) * n + dk;
#pragma unroll
            for (int q = 0; q < 32; q++)
                if (q <= r) lrow[q] = a[q];
        }
    }
    if (bx == 0 && lane == 0 && bad) c.chol_fail = 1;
    __syncthreads();
    // X' L_kk^T = A with unit-diagonal L (row per lane, column-oriented so the 31-q updates of a step are
    // independent); the panel factor is L_Ik = X' D^-1, the forward-substituted rhs z_k = L_kk^-1 r_k
#pragma unroll
    for (int q = 0; q < 32; q++) {
        const double xq = x[q];
#pragma unroll
        for (int c2 = q + 1; c2 < 32; c2++) x[c2] -= xq * Lk[c2 * 33 + q];
    }
    if (bx == 0 && lane == 32) {
#pragma unroll
        for (int q = 0; q < 32; q++) yv[dk + q] = x[q];  // z_k
    }
    if (!has_pair) return;
    double xs[32];   // row of L_Ik = X' D^-1
#pragma unroll
    for (int q = 0; q < 32; q++) xs[q] = x[q] * rd[q];
    double sy = 0.0;  // L_Ik row . z_k ; z_k sits in lane 32 of a diagonal pair (wave-uniform control flow here)
#pragma unroll
    for (int q = 0; q < 32; q++) sy += xs[q] * rl64(x[q], 32);
    if (diagp && hi == 0) {
        double* dst = Lf + ((size_t)I * 32 + r) * n + dk;
#pragma unroll
        for (int q = 0; q < 32; q++) dst[q] = xs[q];  // L_Ik
        vec[(size_t)I * 32 + r] -= sy;
    }
    __syncthreads();  // every lane is done reading L_kk before X_I overwrites it
    // C_IJ -= L_Ik D L_Jk^T = (X'_I D^-1) X'_J^T : XI holds the scaled rows of tile I, XJ the unscaled rows of tile J
    if (hi == 0) {
#pragma unroll
        for (int q = 0; q < 32; q++) XI[r * 34 + q] = xs[q];
        if (diagp) {
#pragma unroll
            for (int q = 0; q < 32; q++) XJ[r * 34 + q] = x[q];
        }
    } else if (!diagp) {
#pragma unroll
        for (int q = 0; q < 32; q++) XJ[r * 34 + q] = x[q];
    }
    __syncthreads();
    const double* XJp = XJ;
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++) {
            if (diagp && tj > ti) continue;
            double* C = S + ((size_t)I * 32 + 16 * ti) * n + (size_t)J * 32 + 16 * tj;
            d4_t acc = cacc[ti][tj];
#pragma unroll
            for (int ks = 0; ks < 8; ks++) {
                const double av = -XI[(16 * ti + l15) * 34 + 4 * ks + l4];
                const double bv = XJp[(16 * tj + l15) * 34 + 4 * ks + l4];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc, 0, 0, 0);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) C[(size_t)(l4 + 4 * i) * n + l15] = acc[i];
        }
}

// ------------------------------------------------------------------------------------------------
// The same step for FEW windows (latency is everything: one window = a chain of nb dependent launches), built around
// `v_fmac_f64_dpp ... row_newbcast:n` (gfx90a+: the only DPP control the FP64 pipe takes -- lane n of every 16-lane row is
// broadcast to the row).  In the form above every element of a rank-1 update costs three instructions: two v_readlane_b32 to bring
// u_{c2} (held by lane c2) into a scalar pair, one FMA; the 32 x 32 elimination is ~1 500 of them per row set and a lone wave
// issues one every four to six cycles.  With the broadcast inside the FMA an element costs ONE instruction.  Layout:
//   lanes 0..31 of a wave hold the 32 rows of the diagonal tile, lanes 32..63 the rows of ONE panel tile, in the same 32 registers
//   t[] (t[c] = column c of the lane's row); wave 0 of the workgroup takes tile (I,k), wave 1 tile (J,k) -- both eliminate the
//   diagonal tile (the same instructions, hence the same bits) on their own SIMD, so a pivot costs 31 - cc FMACs for diagonal and
//   panel rows together (round 3's first DPP form, k_chol_step3, kept the panel rows of both tiles in a second array in one wave:
//   2 (31 - cc) FMACs per pivot, ~66 instructions; 9.8 k cycles per elimination against 7.0 k here);
//   at pivot cc, u = t[cc] of lanes 0..31 is u_0..u_31; the broadcast operand must sit in every 16-lane row, so u_0..15 / u_16..31
//   are replicated with ds_bpermute (crossbar only, no LDS memory) into uLow / uHigh and
//   t[c2] -= l * u_{c2}  is  v_fmac_f64_dpp t[c2], -(c2 < 16 ? uLow : uHigh), l  row_newbcast:(c2 & 15)
//   (the sign rides in the DPP word's source modifier: no negated copy of l).
// The hand-written instruction reads its broadcast operand through DPP: the two wait states a DPP read needs after a VALU write of
// that register (the compiler does not look into inline assembly) are the s_nop in front of each pivot's first FMAC.
// Zero / non-finite pivots are looked for once, in the d vector, after the elimination.
// Same arithmetic as k_chol_step up to the association of l = a / d: results agree to rounding (and bit for bit with k_chol_step3,
// checked before that kernel was removed: scripts/step_forms.py).
// ------------------------------------------------------------------------------------------------
template <int LANE>
DEVI double wl64(double old, double v) {  // old with lane LANE replaced by the wave-uniform value v (two v_writelane_b32)
    int lo = __double2loint(old), hi = __double2hiint(old);
    const int vlo = __builtin_amdgcn_readfirstlane(__double2loint(v)), vhi = __builtin_amdgcn_readfirstlane(__double2hiint(v));
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(lo) : "s"(vlo), "n"(LANE));
    asm volatile("v_writelane_b32 %0, %1, %2" : "+v"(hi) : "s"(vhi), "n"(LANE));
    return __hiloint2double(hi, lo);
}
template <int N, bool NOP>
DEVI void fnmac_bcast(double& acc, double urep, double s) {   // acc -= urep[lane N of this lane's row] * s
    if (NOP) asm volatile("s_nop 1\n\tv_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(urep), "v"(s), "n"(N));
    else asm volatile("v_fmac_f64_dpp %0, -%1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(urep), "v"(s), "n"(N));
}
DEVI double bperm64(double v, int byte_addr) {   // the value of lane byte_addr / 4
    const int lo = __builtin_amdgcn_ds_bpermute(byte_addr, __double2loint(v));
    const int hi = __builtin_amdgcn_ds_bpermute(byte_addr, __double2hiint(v));
    return __hiloint2double(hi, lo);
}
template <int C2, int CC>
struct ElimUpd {   // columns C2..31 of pivot CC
    static DEVI void run(double (&t)[32], double uLow, double uHigh, double l) {
        if constexpr (C2 < 32) {
            fnmac_bcast<(C2 & 15), false>(t[C2], (C2 < 16) ? uLow : uHigh, l);
            ElimUpd<C2 + 1, CC>::run(t, uLow, uHigh, l);
        }
    }
};
// One pivot.  No per-lane masks anywhere: the entries of a diagonal row above the diagonal are never read by another lane (u_{c2}
// comes from lane c2 > CC, the pivot from lane CC) nor stored where anybody uses them, so they may hold anything -- lane CC's own
// update with l = 1 and the lanes r < CC run through the same instructions; what a lane must KEEP from pivot CC (d_CC, z_CC) is
// captured with v_writelane into lane CC of dout / zout before the unguarded updates overwrite it.
// uLow / uHigh are column CC replicated into every 16-lane row; those of the NEXT pivot are requested as soon as its column is
// final (after the first FMAC) so that the crossbar round trip hides behind the remaining FMACs of this one.  (A fully hand-
// scheduled variant -- the reciprocal, l, z and the captures of the next pivot slotted between the FMACs -- measured the same.)
// WRITE_X: 0 nothing; 1 Xrow[CC] = l; 2 (vba_chain.h) Xrow[pc] = l and Xrow[pc + ELIM_U_OFF] = u = l d with pc = (CC & 3) * 8 + (CC >> 2): the
// eight k-steps a lane needs as an MFMA operand lie side by side, and the second operand (rows times D) needs no multiplication
#define ELIM_U_OFF (32 * 34)
template <int CC, int WRITE_X>
struct ElimStep {
    static DEVI void run(double (&t)[32], double& rr, double& dout, double& zout, double uLow, double uHigh, int aLow, int aHigh, double* Xrow) {
        if constexpr (CC < 32) {
            const double u = t[CC];                      // column CC before the division: l d
            const double piv = rl64(u, CC);              // d_CC (lane CC holds row CC of the diagonal tile)
            double y = __builtin_amdgcn_rcp(piv);        // v_rcp_f64 + two Newton steps: full double accuracy
            y = y * (2.0 - piv * y);
            y = y * (2.0 - piv * y);
            const double l = u * y;
            const double zc = rl64(rr, CC);              // z_CC is final here
            dout = wl64<CC>(dout, piv);
            zout = wl64<CC>(zout, zc);
            rr -= l * zc;
            if constexpr (WRITE_X == 1) Xrow[CC] = l;    // lanes 32..63: row r of L_Tk for the MFMA update (lanes 0..31: a scratch row)
            if constexpr (WRITE_X == 2) { Xrow[(CC & 3) * 8 + (CC >> 2)] = l; Xrow[(CC & 3) * 8 + (CC >> 2) + ELIM_U_OFF] = u; }
            t[CC] = l;
            double nLow = 0.0, nHigh = 0.0;
            if constexpr (CC < 31) {
                fnmac_bcast<((CC + 1) & 15), true>(t[CC + 1], (CC + 1 < 16) ? uLow : uHigh, l);
                if constexpr (CC + 1 < 15) nLow = bperm64(t[CC + 1], aLow);
                if constexpr (CC + 1 < 31) nHigh = bperm64(t[CC + 1], aHigh);
                __builtin_amdgcn_sched_barrier(0);       // (the requests stay in front of the remaining FMACs)
                ElimUpd<CC + 2, CC>::run(t, uLow, uHigh, l);
            }
            ElimStep<CC + 1, WRITE_X>::run(t, rr, dout, zout, nLow, nHigh, aLow, aHigh, Xrow);
        }
    }
};
template <int WRITE_X>
DEVI void elim_tile(double (&t)[32], double& rr, double& dout, double& zout, int aLow, int aHigh, double* Xrow) {
    ElimStep<0, WRITE_X>::run(t, rr, dout, zout, bperm64(t[0], aLow), bperm64(t[0], aHigh), aLow, aHigh, Xrow);
}

// ONE = a single window: what the kernel would fetch from the window descriptor and the step table (descriptor -> step table ->
// pair list -> tile rows: four dependent loads, ~600 cycles each, in front of the elimination) comes in the kernel arguments, and
// the chain is pair list -> tile rows.
struct StepOne { int algo, nS, nb, vec0, pair_off, npair; long long S0; };
template <bool ONE>
__global__ void __launch_bounds__(128) k_chol_step4(Batch B, int k, StepOne so) {
    __shared__ double XI[32 * 34];   // rows of L_Ik            (A operand: -L_Ik)
    __shared__ double XJ[32 * 34];   // rows of L_Jk            (B operand: L_Jk D_k, scaled when it is read)
    __shared__ double XD[32 * 34];   // where the diagonal lanes' Xrow stores go (never read)
    __shared__ double dg[32];
    const int w = blockIdx.y;
    WinCtrl& c = B.ctrl[w];
    int n, npair, pair_off;
    long long S0;
    int vec0;
    if constexpr (ONE) {
        if (!(c.active && (so.algo == 0 || c.lm_need_trial))) return;   // win_on
        if (k >= so.nb) return;
        n = so.nS; npair = so.npair; pair_off = so.pair_off; S0 = so.S0; vec0 = so.vec0;
    } else {
        const WinDesc& d = B.desc[w];
        if (!win_on(d, c)) return;
        if (k >= d.nb || k < d.nc) return;
        const int* sb = B.tl_step_begin + d.tl_step0;
        npair = sb[k + 1] - sb[k];
        pair_off = d.tl_pair0 + sb[k];
        n = d.nS; S0 = d.S0; vec0 = d.vec0;
    }
    const int bx = blockIdx.x;
    if (bx >= (npair > 0 ? npair : 1)) return;
    const bool has_pair = bx < npair;
    int I = 0, J = 0;
    if (has_pair) {
        const int v = B.tl_pairs[pair_off + bx];
        I = v >> 16;
        J = v & 0xffff;
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hi = lane >> 5;
    double* S = B.S + S0;
    double* Lf = B.Lf + S0;
    double* vec = B.vec + vec0;
    double* yv = B.yv + vec0;
    const size_t dk = (size_t)k * 32;
    const bool diagp = has_pair && (I == J);
#ifdef VBA_STAMPS   // diagnostic build only (scripts/stamps.sh): shader-clock stamps of wave 0 of workgroup 1 of column 5 into B.dbg
    unsigned long long st_[8];
#define STAMP(i) { if (k == 5 && bx == 1 && wave == 0) { st_[i] = __builtin_amdgcn_s_memtime(); } }
    STAMP(0)
#else
#define STAMP(i)
#endif
    const int l15 = lane & 15, l4 = lane >> 4;
    const bool elim = wave == 0 || (has_pair && !diagp);
    const int T = wave ? J : I;                      // this wave's panel tile
    double t[32], rr = 0.0;
    if (elim) {
        {   // whole rows, 32-byte pieces (rows start on 256-byte boundaries: nS is a multiple of 32)
            const double4* row = reinterpret_cast<const double4*>(S + (hi ? (size_t)T * 32 + r : dk + r) * n + dk);
            if (!hi || has_pair) {
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    const double4 v = row[q];
                    t[4 * q] = v.x; t[4 * q + 1] = v.y; t[4 * q + 2] = v.z; t[4 * q + 3] = v.w;
                }
            } else {
#pragma unroll
                for (int q = 0; q < 32; q++) t[q] = 0.0;
            }
        }
        // right-hand side: one more column.  The rhs rows of a panel tile are updated by ONE workgroup, the one of its diagonal pair
        rr = hi ? ((diagp && wave == 0) ? vec[(size_t)I * 32 + r] : 0.0) : vec[dk + r];
    }
    // this wave's half of the trailing tile C_IJ (rows 16 wave .. 16 wave + 15), requested behind the rows the elimination waits
    // for: it arrives while the elimination runs
    d4_t cacc[2];
#pragma unroll
    for (int tj = 0; tj < 2; tj++) {
        const double* C = S + ((size_t)I * 32 + 16 * wave) * n + (size_t)J * 32 + 16 * tj;
#pragma unroll
        for (int i = 0; i < 4; i++) cacc[tj][i] = has_pair ? C[(size_t)(l4 + 4 * i) * n + l15] : 0.0;
    }
    if (elim) {
        double dout = 1.0, zout = 0.0;               // lane r < 32 ends up with d_r and z_r
#ifdef VBA_STAMPS
        { double sink = t[0] + t[31] + rr; asm volatile("" :: "v"(sink)); }   // the loads have landed
#endif
        STAMP(1)
        elim_tile<1>(t, rr, dout, zout, 4 * l15, 4 * (16 + l15), (hi ? (wave ? XJ : XI) : XD) + r * 34);
        STAMP(2)
        if (wave == 0) {
            if (bx == 0 && !hi) {                    // the factor's diagonal tile (unit L below the diagonal, D on it) and z_k = L_kk^-1 r_k
                double4* lrow = reinterpret_cast<double4*>(Lf + (dk + r) * n + dk);
#pragma unroll
                for (int q = 0; q < 8; q++) {
                    double4 v;
                    // (what the elimination leaves above the diagonal is arbitrary: zeros go into the factor)
                    v.x = (4 * q == r) ? dout : ((4 * q < r) ? t[4 * q] : 0.0);
                    v.y = (4 * q + 1 == r) ? dout : ((4 * q + 1 < r) ? t[4 * q + 1] : 0.0);
                    v.z = (4 * q + 2 == r) ? dout : ((4 * q + 2 < r) ? t[4 * q + 2] : 0.0);
                    v.w = (4 * q + 3 == r) ? dout : ((4 * q + 3 < r) ? t[4 * q + 3] : 0.0);
                    lrow[q] = v;
                }
                yv[dk + r] = zout;
            }
            if (bx == 0) {
                const bool badl = !hi && (dout == 0.0 || !isfinite(dout));
                if (__ballot(badl) != 0ull && lane == 0) c.chol_fail = 1;
            }
            if (diagp && hi) {                       // tile (I,k) of the factor and the rhs rows it has updated
                double4* dst = reinterpret_cast<double4*>(Lf + ((size_t)I * 32 + r) * n + dk);
#pragma unroll
                for (int q = 0; q < 8; q++) dst[q] = make_double4(t[4 * q], t[4 * q + 1], t[4 * q + 2], t[4 * q + 3]);
                vec[(size_t)I * 32 + r] = rr;
            }
            if (!hi) dg[r] = dout;
        }
        STAMP(3)
    }
    if (!has_pair) return;                           // (the same for every thread of the workgroup)
    // C_IJ -= L_Ik D_k L_Jk^T: XI / XJ hold the rows of L_Ik / L_Jk (written pivot by pivot above), D_k is dg; 16 rows per wave.
    // (LDS-only barrier: the stores of the factor tiles above drain while the MFMAs run)
    lds_barrier();
    const double* XJp = diagp ? XI : XJ;
#pragma unroll
    for (int ks = 0; ks < 8; ks++) {    // (the wave's two products side by side: independent accumulators)
        const double av = -XI[(16 * wave + l15) * 34 + 4 * ks + l4];
        const double dvk = dg[4 * ks + l4];
#pragma unroll
        for (int tj = 0; tj < 2; tj++) {
            const double bv = XJp[(16 * tj + l15) * 34 + 4 * ks + l4] * dvk;
            cacc[tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, cacc[tj], 0, 0, 0);
        }
    }
#pragma unroll
    for (int tj = 0; tj < 2; tj++) {
        if (diagp && tj > wave) continue;
        double* C = S + ((size_t)I * 32 + 16 * wave) * n + (size_t)J * 32 + 16 * tj;
#pragma unroll
        for (int i = 0; i < 4; i++) C[(size_t)(l4 + 4 * i) * n + l15] = cacc[tj][i];
    }
#ifdef VBA_STAMPS
    STAMP(4)
    if (wave == 0) { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); STAMP(5) }
    if (k == 5 && bx == 1 && threadIdx.x == 0)
        for (int i = 0; i < 6; i++) B.dbg[i] = (double)st_[i];
#endif
#undef STAMP
}

// ------------------------------------------------------------------------------------------------
// Left-looking form of the tile factorisation for LARGE batches.  The right-looking kernels above re-read and
// re-write every trailing tile once per step (~19 MB of HBM traffic per C3 factorisation); here a tile is read from S
// once, accumulates ALL its updates C_IJ = S_IJ - sum_k L_Ik D_k L_Jk^T in MFMA registers (same k order, hence the same
// rounding as the right-looking sweep), and is written once.  S itself is never modified.  Per block column J:
//   diagonal tile : C_JJ, its L D L^T, the forward-substituted rhs y_J, and W_J = L_JJ^-T D_J^-1 (so that the panel
//                   needs no serial triangular solve)
//   panel tile    : C_IJ, then L_IJ = C_IJ W_J as one more MFMA product.
// ------------------------------------------------------------------------------------------------
// In this mode the factor is stored TILE BY TILE -- tile (I,J) at 1024 (I nb + J) doubles -- in the order the MFMA operand
// registers want it: element (r, c) of a tile belongs to lane (c & 3) * 16 + (r & 15), the lane's 16 elements being the two row
// halves x eight k-steps of v_mfma_f64_16x16x4 (operand A[row][k]: row = lane & 15, k = 4 ks + (lane >> 4)), two k-steps per 16-byte
// piece.  A panel wave then loads both operand tiles of a product with 8 + 8 fully coalesced global_load_dwordx4 straight into
// the registers the MFMAs read: no LDS, no barrier, and the occupancy is set by the registers alone.
DEVI int ll_pk(int r, int c) { return (((((r >> 4) * 4 + (c >> 3)) * 64) + ((c & 3) * 16 + (r & 15))) * 2) + ((c >> 2) & 1); }
DEVI size_t ll_tile(const WinDesc& d, int I, int J) { return 1024 * ((size_t)I * d.nb + J); }

// diagonal tile of block column J: C_JJ = S_JJ - sum_k L_Jk D_k L_Jk^T and the dot products L_Jk y_k for the forward substitution.
// Both MFMA operands are the one packed tile L_Jk (A = -L_Jk, B = L_Jk D_k), loaded straight into registers.
DEVI void ll_diag_accumulate(const Batch& B, const WinDesc& d, int J, int kb, int ke, d4_t (&acc)[2][2], double& sdot_out) {
    const int lane = threadIdx.x, n = d.nS;
    const double* S = B.S + d.S0;
    const double* Lf = B.Lf + d.S0;
    const int l15 = lane & 15, l4 = lane >> 4;
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++) {
            const double* C = S + ((size_t)J * 32 + 16 * ti) * n + (size_t)J * 32 + 16 * tj;
#pragma unroll
            for (int i = 0; i < 4; i++) acc[ti][tj][i] = C[(size_t)(l4 + 4 * i) * n + l15];
        }
    const int* kl = B.tl_kl + d.tl_k0;
    double p0 = 0.0, p1 = 0.0;   // this lane's share of (L_Jk y_k) for rows l15 and 16 + l15: columns 4 ks + l4
    // one wave per window, a chain of dependent products: the tile of step e+1 is in flight (registers) while the MFMAs of step e run
    double2 nx[8];
    double ndv[8], nyk[8];
    auto fetch = [&](int k) {
        const double2* t = reinterpret_cast<const double2*>(Lf + ll_tile(d, J, k)) + lane;
        const double* sd = B.dvec + d.vec0 + (size_t)k * 32 + l4;
        const double* sy = B.yv + d.vec0 + (size_t)k * 32 + l4;
#pragma unroll
        for (int q = 0; q < 8; q++) { nx[q] = t[64 * q]; ndv[q] = sd[4 * q]; nyk[q] = sy[4 * q]; }
    };
    if (kb < ke) fetch(kl[kb]);
    for (int e = kb; e < ke; e++) {
        double2 x[8];
        double dv[8], yk[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { x[q] = nx[q]; dv[q] = ndv[q]; yk[q] = nyk[q]; }
        if (e + 1 < ke) fetch(kl[e + 1]);
#pragma unroll
        for (int ks = 0; ks < 8; ks++) {
            const double2 a0 = x[ks >> 1], a1 = x[4 + (ks >> 1)];
            p0 += ((ks & 1) ? a0.y : a0.x) * yk[ks];
            p1 += ((ks & 1) ? a1.y : a1.x) * yk[ks];
        }
        // (k-step outermost: four independent accumulators back to back -- a chain of dependent FP64 MFMAs issues at about two
        // thirds of the rate; every accumulator still sums its k-steps in ascending order)
#pragma unroll
        for (int ks = 0; ks < 8; ks++)
#pragma unroll
            for (int ti = 0; ti < 2; ti++)
#pragma unroll
                for (int tj = 0; tj < 2; tj++) {
                    const double2 pi = x[ti * 4 + (ks >> 1)], pj = x[tj * 4 + (ks >> 1)];
                    const double av = -((ks & 1) ? pi.y : pi.x);
                    const double bv = ((ks & 1) ? pj.y : pj.x) * dv[ks];
                    acc[ti][tj] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, acc[ti][tj], 0, 0, 0);
                }
    }
    p0 += __shfl_xor(p0, 16, 64); p0 += __shfl_xor(p0, 32, 64);
    p1 += __shfl_xor(p1, 16, 64); p1 += __shfl_xor(p1, 32, 64);
    sdot_out = (lane & 16) ? p1 : p0;   // lane r < 32 holds the sum of row r (lanes 32..63 mirror them)
}

// Diagonal tile of block column J: C_JJ, its L D L^T, y_J, D_J and W_J = (L_JJ^-T D_J^-1)^T (packed like a factor tile), with the
// elimination of k_chol_step4 (v_fmac_f64_dpp row_newbcast: one instruction per element of a rank-1 update instead of two
// v_readlane + one FMA: the first form of this kernel, 6 054 instructions; diagonal rows in lanes 0..31 and the rows that ride
// along in lanes 32..63 of ONE register array).  The rows that ride along with the diagonal tile are the rows of the IDENTITY: a row P of a
// panel comes out of the elimination as P L^-T D^-1, so the identity comes out as L_JJ^-T D_J^-1 -- W_J itself, for the price of the
// ride (496 FMACs) instead of a 32-column forward substitution against L_JJ in LDS (in-kernel stamps of ll_diag: 12-18 k cycles
// LDL^T + 5 k y_J + 13 k W_J per column; here ~10 k for all three).  The right-hand side rides along as one more column (y_J).
// Both tiles leave through LDS in 16-byte pieces of the packed order (ll_diag: 64 scattered 8-byte stores per lane).
DEVI void ll_diag2(const Batch& B, const WinDesc& d, WinCtrl& c, int w, int J, double* CT, double* WT) {
    const int* pb = B.tl_pan_begin + d.tl_step0;
    const int* klb = B.tl_kl_begin + d.tl_kb0;
    const int ent = pb[J] + J;  // column entry of (J,J)
    const int lane = threadIdx.x, r = lane & 31, hi = lane >> 5;
    const int l15 = lane & 15, l4 = lane >> 4;
    d4_t acc[2][2];
    double sdot = 0.0;
    ll_diag_accumulate(B, d, J, klb[ent], klb[ent + 1], acc, sdot);
    // C_JJ through LDS into one row per lane of the lower half of the wave (what lies above the diagonal is never used); the upper
    // half holds the rows of the identity
#pragma unroll
    for (int ti = 0; ti < 2; ti++)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int i = 0; i < 4; i++) CT[(16 * ti + l4 + 4 * i) * 34 + 16 * tj + l15] = acc[ti][tj][i];
    lds_barrier();
    double t[32];
#pragma unroll
    for (int q = 0; q < 32; q++) {
        const double cv = CT[r * 34 + q];
        t[q] = hi ? ((q == r) ? 1.0 : 0.0) : cv;
    }
    const size_t dk = (size_t)J * 32;
    const double rh = (B.vec + d.vec0)[dk + r] - __shfl(sdot, r, 64);   // b_J - sum_k L_Jk y_k
    double rr = hi ? 0.0 : rh, dout = 1.0, zout = 0.0;
    lds_barrier();                                    // every lane has its row: CT is free
    elim_tile<0>(t, rr, dout, zout, 4 * l15, 4 * (16 + l15), nullptr);
    {
        const bool badl = !hi && (dout == 0.0 || !isfinite(dout));
        if (__ballot(badl) != 0ull && lane == 0) c.chol_fail = 1;
    }
    if (!hi) {
        B.dvec[d.vec0 + dk + r] = dout;
        (B.yv + d.vec0)[dk + r] = zout;
    }
    // rows of L_JJ (unit lower, D on the diagonal, zeros above) into CT and the identity rows -- row r of L^-T D^-1 = column r of W_J^T --
    // into WT, one row per lane, no divergence: CT[r][c] = L[r][c], WT[r][c] = W^T[c][r]
    double* rowp = (hi ? WT : CT) + r * 34;
#pragma unroll
    for (int q = 0; q < 32; q++) rowp[q] = (hi || q < r) ? t[q] : ((q == r) ? dout : 0.0);
    lds_barrier();
    // packed order (ll_pk): piece (q, lane) = { M[row][c0], M[row][c0 + 4] }, row = 16 (q >> 2) + (lane & 15), c0 = 8 (q & 3) + (lane >> 4)
    double2* Ljj = reinterpret_cast<double2*>(B.Lf + d.S0 + ll_tile(d, J, J)) + lane;
    double2* Wd = reinterpret_cast<double2*>(B.winv + 1024 * (size_t)d.win) + lane;   // d.win: the batch-wide window index
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const int row = 16 * (q >> 2) + l15, c0 = 8 * (q & 3) + l4;
        Ljj[64 * q] = make_double2(CT[row * 34 + c0], CT[row * 34 + c0 + 4]);
        Wd[64 * q] = make_double2(WT[c0 * 34 + row], WT[(c0 + 4) * 34 + row]);
    }
}

// (A fused variant -- the wave that owns tile (J+1,J) going on to factor diagonal tile J+1 -- was measured: no gain at 512
// windows)
__global__ void __launch_bounds__(64) k_chol_diag_ll2(Batch B, int J) {
    __shared__ double CT[32 * 34];
    __shared__ double WT[32 * 34];
    const int w = blockIdx.x;
    if (w >= B.n_win) return;
    const WinDesc& d = B.desc[w];
    WinCtrl& c = B.ctrl[w];
    if (!win_on(d, c)) return;
    if (J >= d.nb || J < d.nc) return;
    ll_diag2(B, d, c, w, J, CT, WT);
}

// panel tile (I,J): C_IJ = S_IJ - sum_k L_Ik D_k L_Jk^T, then L_IJ = C_IJ W_J.  The wave accumulates the TRANSPOSED tile
// (A operand = L_Jk D_k, B operand = -L_Ik: the same products in the same order as the row-major form, so the same bits): the
// accumulator registers of C^T are then exactly the B operand of L_IJ^T = W_J^T C_IJ^T, and that product's result registers are
// exactly the packed order of tile (I,J) -- nothing passes through LDS.
DEVI void ll_panel_init(const double* S, int n, int I, int J, int l15, int l4, d4_t (&acc)[2][2]) {
#pragma unroll
    for (int tj = 0; tj < 2; tj++)
#pragma unroll
        for (int ti = 0; ti < 2; ti++) {
            const double* C = S + ((size_t)I * 32 + 16 * ti + l15) * n + (size_t)J * 32 + 16 * tj + l4;
#pragma unroll
            for (int i = 0; i < 4; i++) acc[tj][ti][i] = C[4 * i];   // acc[tj][ti][i] = C[32 I + 16 ti + l15][32 J + 16 tj + 4 i + l4]
        }
}
DEVI void ll_panel_mfma(const double (&av)[2][8], const double2 (&xi)[8], d4_t (&acc)[2][2]) {
#pragma unroll
    for (int ks = 0; ks < 8; ks++)      // (k-step outermost: the four accumulators are independent of one another)
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int ti = 0; ti < 2; ti++) {
                const double2 pi = xi[ti * 4 + (ks >> 1)];
                const double bv = -((ks & 1) ? pi.y : pi.x);
                acc[tj][ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(av[tj][ks], bv, acc[tj][ti], 0, 0, 0);
            }
}
// L_IJ^T = W_J^T C_IJ^T: A operand = the packed W tile, B operand = the accumulators; the result registers are the packed tile
DEVI void ll_panel_finish_keep(const double2 (&xw)[8], const d4_t (&acc)[2][2], double2* out, double2 (&xo)[8]);
DEVI void ll_panel_finish(const double2 (&xw)[8], const d4_t (&acc)[2][2], double2* out) {
    double2 xo[8];
    ll_panel_finish_keep(xw, acc, out, xo);
}

// the same, also handing the tile back as the operand pieces of a later product (k_chol_chain_panel)
DEVI void ll_panel_finish_keep(const double2 (&xw)[8], const d4_t (&acc)[2][2], double2* out, double2 (&xo)[8]) {
    d4_t o[2][2];
#pragma unroll
    for (int tk = 0; tk < 2; tk++)
#pragma unroll
        for (int ti = 0; ti < 2; ti++) o[tk][ti] = d4_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 8; ks++)      // (k-step outermost: four independent accumulators)
#pragma unroll
        for (int tk = 0; tk < 2; tk++)
#pragma unroll
            for (int ti = 0; ti < 2; ti++) {
                const double2 pw = xw[tk * 4 + (ks >> 1)];
                const double av = (ks & 1) ? pw.y : pw.x;
                const double bv = acc[ks >> 2][ti][ks & 3];
                o[tk][ti] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, bv, o[tk][ti], 0, 0, 0);
            }
#pragma unroll
    for (int tk = 0; tk < 2; tk++)
#pragma unroll
        for (int ti = 0; ti < 2; ti++) {
            // o[i] = L[16 ti + l15][16 tk + 4 i + l4]: k-steps 4 tk + i of row half ti
            xo[ti * 4 + 2 * tk] = make_double2(o[tk][ti][0], o[tk][ti][1]);
            xo[ti * 4 + 2 * tk + 1] = make_double2(o[tk][ti][2], o[tk][ti][3]);
            out[64 * (ti * 4 + 2 * tk)] = xo[ti * 4 + 2 * tk];
            out[64 * (ti * 4 + 2 * tk + 1)] = xo[ti * 4 + 2 * tk + 1];
        }
}

// One wave per tile.  (Measured and not kept, all within +-3 % of this form at 4096 windows: two tiles of the column per wave sharing
// L_Jk D_k and W_J -- a quarter less traffic; one 32-byte record per tile instead of the chain column row -> panel entry -> list
// bounds -> list; a register double buffer for the next product's tiles; 2, 3 or 4 waves per SIMD.  See DESIGN.md section 6.)
__global__ void __launch_bounds__(64) k_chol_panel_ll(Batch B, int J, int per_win) {
    // the waves of one window sit on one XCD (schur_map)
    int w, bx;
    if (!schur_map(B, per_win, w, bx)) return;
    const WinDesc& d = B.desc[w];
    if (!win_on(d, B.ctrl[w])) return;
    if (J >= d.nb || J < d.nc) return;
    const int* pb = B.tl_pan_begin + d.tl_step0;
    const int* pan = B.tl_pan + d.tl_pan0;
    const int npan = pb[J + 1] - pb[J];
    if (bx >= npan) return;
    const int I = pan[pb[J] + bx];
    const int* klb = B.tl_kl_begin + d.tl_kb0;
    const int ent = pb[J] + J + 1 + bx;
    const int lane = threadIdx.x, n = d.nS;
    const int l15 = lane & 15, l4 = lane >> 4;
    const double* S = B.S + d.S0;
    double* Lf = B.Lf + d.S0;
    d4_t acc[2][2];
    ll_panel_init(S, n, I, J, l15, l4, acc);
    const int* kl = B.tl_kl + d.tl_k0;
    const int kb = klb[ent], ke = klb[ent + 1];
    for (int e = kb; e < ke; e++) {
        const int k = kl[e];
        const double2* tj_ = reinterpret_cast<const double2*>(Lf + ll_tile(d, J, k)) + lane;
        const double2* ti_ = reinterpret_cast<const double2*>(Lf + ll_tile(d, I, k)) + lane;
        const double* sd = B.dvec + d.vec0 + (size_t)k * 32 + l4;
        double2 xj[8], xi[8];
        double dv[8];
#pragma unroll
        for (int q = 0; q < 8; q++) { xj[q] = tj_[64 * q]; xi[q] = ti_[64 * q]; dv[q] = sd[4 * q]; }
        double av[2][8];
#pragma unroll
        for (int tj = 0; tj < 2; tj++)
#pragma unroll
            for (int ks = 0; ks < 8; ks++) {
                const double2 pj = xj[tj * 4 + (ks >> 1)];
                av[tj][ks] = ((ks & 1) ? pj.y : pj.x) * dv[ks];
            }
        ll_panel_mfma(av, xi, acc);
    }
    const double2* tw = reinterpret_cast<const double2*>(B.winv + 1024 * (size_t)d.win) + lane;
    double2 xw[8];
#pragma unroll
    for (int q = 0; q < 8; q++) xw[q] = tw[64 * q];
    ll_panel_finish(xw, acc, reinterpret_cast<double2*>(Lf + ll_tile(d, I, J)) + lane);
}
