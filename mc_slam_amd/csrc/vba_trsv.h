// vba_trsv.h -- back-substitution L^T x = y, one workgroup per window: k_trsv (row-major factor) and k_trsv_p (packed factor
// of the left-looking kernels).  Reads Lf, yv, dvec and the tile lists; writes the pose step into vec.  Needs vba_batch.h and
// vba_factor.h (ll_tile).
#pragma once
#include "vba_batch.h"
#include "vba_factor.h"

// K_trsv: L^T x = y.  One 256-thread workgroup per window walks the block columns from the bottom: the
// column's nonzero tiles are gathered by the four waves (one tile per wave and trip), the 32x32 triangular solve runs in wave 0 on
// registers (column of L per lane, v_readlane broadcasts).
__global__ void __launch_bounds__(256) k_trsv(Batch B) {
    extern __shared__ double xs[];  // nS doubles + 8*32 partials + 32*33 diagonal tile
    const int w = blockIdx.x;
    const WinDesc& d = B.desc[w];
    if (!win_on(d, B.ctrl[w])) return;
    const int n = d.nS, t = threadIdx.x;
    double* part = xs + n;
    double* Lt = part + 256;
    const double* S = B.Lf + d.S0;
    const bool pk = B.l_packed;   // left-looking mode: the factor is stored tile by tile (ll_pk)
    double* vec = B.vec + d.vec0;
    const double* yv = B.yv + d.vec0;
    const int* pb = B.tl_pan_begin + d.tl_step0;
    const int* pan = B.tl_pan + d.tl_pan0;
    for (int q = t; q < n; q += 256) xs[q] = yv[q];
    for (int q = t; q < 256; q += 256) part[q] = 0.0;
    __syncthreads();
    // the column's panel tiles are dealt to the four waves; a lane takes 16 elements of a tile, so its loads are in flight
    // together and a column with m tiles costs ceil(m / 4) memory round trips, not m
    const int cc = t & 31, rl = t >> 5, wave = t >> 6, half = (t >> 5) & 1;
    const int lane = t & 63, l15 = lane & 15, l4 = lane >> 4;
    // the diagonal tile of the next block column is fetched while this one is solved; element u of a thread sits at (dr[u], dc[u])
    double nx[4];
    int dpos[4];
#pragma unroll
    for (int u = 0; u < 4; u++) {
        const int q = t + 256 * u;   // row-major: element (q >> 5, q & 31); packed: piece q >> 1 of lane (q >> 1) & 63, half q & 1
        const int pr = 16 * (q >> 9) + ((q >> 1) & 15), pc = 8 * ((q >> 7) & 3) + 4 * (q & 1) + ((q >> 5) & 3);
        dpos[u] = pk ? pr * 33 + pc : (q >> 5) * 33 + (q & 31);
    }
    auto diag_fetch = [&](int k) {
        if (pk) {
            const double* tdk = S + ll_tile(d, k, k);
#pragma unroll
            for (int u = 0; u < 4; u++) nx[u] = tdk[t + 256 * u];
        } else {
            const size_t dk = (size_t)k * 32;
#pragma unroll
            for (int u = 0; u < 4; u++) { const int q = t + 256 * u; nx[u] = S[(dk + (q >> 5)) * n + dk + (q & 31)]; }
        }
    };
    diag_fetch(d.nb - 1);
#ifdef VBA_STAMPS
    unsigned long long st_[8];
#define TSTAMP(i) { if (k == 10) st_[i] = __builtin_amdgcn_s_memtime(); }
#else
#define TSTAMP(i)
#endif
    for (int k = d.nb - 1; k >= 0; k--) {
        const size_t dk = (size_t)k * 32;
        const int i0 = pb[k], m = pb[k + 1] - i0;
        TSTAMP(0)
        if (pk) {
            // a wave per tile: 8 coalesced 16-byte loads per lane; the lane's 16 elements are rows l15 and 16 + l15 of the
            // columns 4 ks + l4 -- eight column sums per lane, reduced over the 16 lanes of a DPP row at the end
            double cs[8];
#pragma unroll
            for (int q = 0; q < 8; q++) cs[q] = 0.0;
            for (int i = wave; i < m; i += 4) {
                const int I = pan[i0 + i];
                const double2* tp = reinterpret_cast<const double2*>(S + ll_tile(d, I, k)) + lane;
                double2 lv[8];
#pragma unroll
                for (int q = 0; q < 8; q++) lv[q] = tp[64 * q];
                const double x0 = xs[I * 32 + l15], x1 = xs[I * 32 + 16 + l15];
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    cs[2 * j] += lv[j].x * x0;
                    cs[2 * j + 1] += lv[j].y * x0;
                    cs[2 * j] += lv[4 + j].x * x1;
                    cs[2 * j + 1] += lv[4 + j].y * x1;
                }
            }
#pragma unroll
            for (int q = 0; q < 8; q++) {
                const double v = row16_sum(cs[q]);
                if (l15 == 0) part[wave * 32 + 4 * q + l4] = v;
            }
        } else {
            double s = 0.0;
            for (int i = wave; i < m; i += 4) {
                const int I = pan[i0 + i];
                const int r0 = I * 32 + half * 16;
                double lv[16];
#pragma unroll
                for (int rr = 0; rr < 16; rr++) lv[rr] = S[(size_t)(r0 + rr) * n + dk + cc];
#pragma unroll
                for (int rr = 0; rr < 16; rr++) s += lv[rr] * xs[r0 + rr];
            }
            part[rl * 32 + cc] = s;
        }
#pragma unroll
        for (int u = 0; u < 4; u++) Lt[dpos[u]] = nx[u];
        TSTAMP(1)
        if (k > 0) diag_fetch(k - 1);
        __syncthreads();
        TSTAMP(2)
        if (t < 64) {
            const int c = t & 31;
            double v;
            double col[32];
#pragma unroll
            for (int j = 0; j < 32; j++) col[j] = Lt[j * 33 + c];  // column c of L_kk (rows j >= c are the factor)
            double dgc = 1.0;
#pragma unroll
            for (int j = 0; j < 32; j++) dgc = (j == c) ? col[j] : dgc;  // d_c sits on the diagonal of the tile
            v = xs[dk + c] / dgc;                                         // D^-1 z
#pragma unroll
            for (int q = 0; q < 8; q++) v -= part[q * 32 + c];
#ifdef VBA_STAMPS
            asm volatile("" :: "v"(v));
#endif
            TSTAMP(3)
#pragma unroll
            for (int j = 31; j >= 0; j--) {                               // unit-diagonal L_kk^T x_k = v
                const double xj = rl64(v, j);
                v = (c < j) ? v - col[j] * xj : v;
            }
            if (t < 32) xs[dk + c] = v;
            TSTAMP(4)
        }
        __syncthreads();
        TSTAMP(5)
#ifdef VBA_STAMPS
        if (k == 10 && t == 0) for (int i = 0; i < 6; i++) B.dbg[16 + i] = (double)st_[i];
#endif
    }
#undef TSTAMP
    for (int q = t; q < n; q += 256) vec[q] = xs[q];
}

// The back-substitution for the row-major factor of the few-window kernels, where its latency counts (one window: 8-10 calls per
// solve, 23 block columns each), as a two-stage pipeline (8 waves).  In k_trsv a block column is a chain  products of ALL its tiles
// with x -> barrier -> 32-step triangular solve -> barrier  (2.3 us per column at C3 size even with the tile lists in LDS and the
// tiles prefetched: round 3's k_trsv_w, 52 us per call), although only ONE of those tiles, (k+1, k), needs the x_{k+1} that the
// previous column has just produced.  Here
//   * wave 0 only solves: column K in 32 steps of  x_j = readlane(acc, j); acc -= reg[j] * x_j.  Lanes 0..31 hold column c of the
//     (strictly lower) diagonal tile in reg[] and the running right-hand side in acc; lanes 32..63 hold column c of tile (K, K-1)
//     and accumulate -sum_j L[32K + j][32(K-1) + c] x_j with the SAME instruction: the one product that needs x_K is finished when x_K
//     is, and seeds column K - 1;
//   * waves 1..7 work one column ahead: the products of column K - 1 with the tiles I >= K + 1 (x_I is final), summed to one partial
//     row per wave; they also bring the diagonal tile and tile (K-1, K-2) of the next solve into LDS (zeros above the diagonal, so the
//     solve needs no mask) and divide z by d (the solve starts from D^-1 z); their tiles are requested one phase earlier still
//     (registers: eight 16-byte loads per tile from one wave-uniform base + 32-bit lane offsets), so no load waits inside a phase.
// One LDS-only barrier per column; the chain per column is wave 0's ~10 LDS reads + 32 x 3 instructions.  Fixed summation order.
// Measured at C3 size: 37 -> 30 us per call (k_trsv_w: 52).
#define TRSV_P_PF 4
#define TRSV_P_DW 7
__global__ void __launch_bounds__(512) k_trsv_p(Batch B) {
    extern __shared__ double xs[];  // nS doubles | 2 x 7 x 32 partial rows | 2 x 32 x 65 solve blocks | 32 seeds | tile lists (ints)
    const int w = blockIdx.x;
    const WinDesc& d = B.desc[w];
    if (!win_on(d, B.ctrl[w])) return;
    const int n = d.nS, nb = d.nb, t = threadIdx.x;
    double* part = xs + n;
    double* R = part + 2 * TRSV_P_DW * 32;
    double* seed = R + 2 * 32 * 65;
    int* lpb = reinterpret_cast<int*>(seed + 32);   // [nb + 1] column starts, then the tile rows
    int* lpan = lpb + nb + 1;
    const double* S = B.Lf + d.S0;
    double* vec = B.vec + d.vec0;
    const double* yv = B.yv + d.vec0;
    {
        const int* pb = B.tl_pan_begin + d.tl_step0;
        const int* pan = B.tl_pan + d.tl_pan0;
        const int np = pb[nb];
        for (int q = t; q <= nb; q += 512) lpb[q] = pb[q];
        for (int q = t; q < np; q += 512) lpan[q] = pan[q];
    }
    for (int q = t; q < n; q += 512) xs[q] = yv[q];
    for (int q = t; q < 2 * TRSV_P_DW * 32 + 2 * 32 * 65 + 32; q += 512) part[q] = 0.0;
    __syncthreads();
    const int wave = t >> 6, lane = t & 63;
    if (wave == 0) {
        // ---------------- the solving wave ----------------
        const int c = lane & 31, hiL = lane >> 5;
        lds_barrier();                               // (the loaders' prologue)
        for (int K = nb - 1; K >= 0; K--) {
            const double* Rk = R + (K & 1) * (32 * 65);
            const double* pk = part + (K & 1) * (TRSV_P_DW * 32);
            double reg[32];
#pragma unroll
            for (int j = 0; j < 32; j++) reg[j] = Rk[j * 65 + lane];
            double acc = 0.0;
            if (!hiL) {
                acc = xs[K * 32 + c] + seed[c];      // D^-1 z (divided by the loaders) - the product with tile (K+1, K)
#pragma unroll
                for (int q = 0; q < TRSV_P_DW; q++) acc -= pk[q * 32 + c];
            }
#pragma unroll
            for (int j = 31; j >= 0; j--) {          // unit-diagonal L_KK^T x_K = acc (reg is zero on and above the diagonal)
                const double xj = rl64(acc, j);
                acc = __builtin_fma(-reg[j], xj, acc);
            }
            if (hiL) seed[c] = acc; else xs[K * 32 + c] = acc;
            lds_barrier();
        }
    } else {
        // ---------------- the seven waves that work ahead ----------------
        const int dw = wave - 1, t2 = t - 64;        // 0..447
        const int cp = lane & 15, rg = lane >> 4;   // column pair, group of eight rows of a tile
        const unsigned rowb = (unsigned)n * 8u;      // row pitch in bytes
        const unsigned lane_off = (unsigned)(rg * 8) * rowb + (unsigned)cp * 16u;
        double2 nlv[TRSV_P_PF][8];
        int nI[TRSV_P_PF];
        double rst[5];
        auto tile_load = [&](int I, size_t dk, double2 (&lv)[8]) {
            const char* tb = reinterpret_cast<const char*>(S + (size_t)I * 32 * n + dk);   // wave-uniform
#pragma unroll
            for (int rr = 0; rr < 8; rr++) lv[rr] = *reinterpret_cast<const double2*>(tb + (lane_off + (unsigned)rr * rowb));
        };
        auto tile_dot = [&](int I, const double2 (&lv)[8], double& s0, double& s1) {
            const double* x = xs + I * 32 + rg * 8;
#pragma unroll
            for (int rr = 0; rr < 8; rr++) { s0 += lv[rr].x * x[rr]; s1 += lv[rr].y * x[rr]; }
        };
        // the tiles (I, col) with I >= col + 2 (tile (col + 1, col), if the column has it, belongs to the solving wave)
        auto dot_range = [&](int col, int& i0, int& m) {
            i0 = lpb[col]; m = lpb[col + 1] - i0;
            if (m > 0 && lpan[i0] == col + 1) { i0++; m--; }
        };
        auto prefetch_dots = [&](int col) {
#pragma unroll
            for (int s = 0; s < TRSV_P_PF; s++) nI[s] = -1;
            if (col < 0) return;
            int i0, m;
            dot_range(col, i0, m);
#pragma unroll
            for (int s = 0; s < TRSV_P_PF; s++) {
                const int i = dw + TRSV_P_DW * s;
                nI[s] = (i < m) ? lpan[i0 + i] : -1;      // (wave-uniform)
                if (nI[s] >= 0) tile_load(nI[s], (size_t)col * 32, nlv[s]);
            }
        };
        // solve block of column K: element e = 1024 tile + 32 j + c; tile 0 = (K, K), tile 1 = (K, K - 1) (zeros if it is not in the
        // factor).  What a lane fetches and where it goes do not depend on K: byte offsets from a wave-uniform base, computed once.
        unsigned roff[5];
        int ridx[5];
        bool rkeep[5];
#pragma unroll
        for (int u = 0; u < 5; u++) {
            const int e = t2 + 448 * u;
            const int tile = (e >> 10) & 1, j = (e >> 5) & 31, cc = e & 31;
            roff[u] = (unsigned)j * rowb + (unsigned)(cc + 32 - 32 * tile) * 8u;   // from 32 columns left of the diagonal tile
            ridx[u] = (e < 2048) ? j * 65 + 32 * tile + cc : -1;
            rkeep[u] = tile == 1 || cc < j;
        }
        const unsigned doff = (unsigned)(lane & 31) * (rowb + 8u) + 256u;           // the diagonal (wave 7 divides z by it)
        double rdg = 1.0;
        auto prefetch_R = [&](int K) {
            if (K < 0) return;
            const bool has_nxt = K >= 1 && lpb[K] > lpb[K - 1] && lpan[lpb[K - 1]] == K;
            const char* base = reinterpret_cast<const char*>(S + (size_t)K * 32 * n + (size_t)K * 32) - 256;   // wave-uniform
#pragma unroll
            for (int u = 0; u < 5; u++) {
                const bool want = ridx[u] >= 0 && (has_nxt || ridx[u] % 65 < 32);   // (ridx % 65 = 32 tile + c)
                rst[u] = want ? *reinterpret_cast<const double*>(base + roff[u]) : 0.0;
            }
            if (dw == TRSV_P_DW - 1) rdg = *reinterpret_cast<const double*>(base + doff);
        };
        auto stage_R = [&](int K) {
            if (K < 0) return;
            double* Rk = R + (K & 1) * (32 * 65);
#pragma unroll
            for (int u = 0; u < 5; u++)
                if (ridx[u] >= 0) Rk[ridx[u]] = rkeep[u] ? rst[u] : 0.0;
            if (dw == TRSV_P_DW - 1 && lane < 32) xs[K * 32 + lane] = xs[K * 32 + lane] / rdg;   // D^-1 z
        };
        // prologue: the block of the last column; nothing to multiply yet
        prefetch_R(nb - 1);
        stage_R(nb - 1);
        prefetch_dots(nb - 2);
        prefetch_R(nb - 2);
        lds_barrier();
        for (int K = nb - 1; K >= 0; K--) {
            const int col = K - 1;                   // the column whose products are formed in this phase
            if (col >= 0) {
                int i0, m;
                dot_range(col, i0, m);
                double s0 = 0.0, s1 = 0.0;
#pragma unroll
                for (int q = 0; q < TRSV_P_PF; q++)  // tile i of the column goes to wave 1 + i % 7
                    if (nI[q] >= 0) tile_dot(nI[q], nlv[q], s0, s1);
                for (int i = dw + TRSV_P_DW * TRSV_P_PF; i < m; i += TRSV_P_DW) {
                    const int I = lpan[i0 + i];
                    double2 lv[8];
                    tile_load(I, (size_t)col * 32, lv);
                    tile_dot(I, lv, s0, s1);
                }
                s0 += __shfl_xor(s0, 16, 64); s1 += __shfl_xor(s1, 16, 64);
                s0 += __shfl_xor(s0, 32, 64); s1 += __shfl_xor(s1, 32, 64);
                if (rg == 0) *reinterpret_cast<double2*>(part + (col & 1) * (TRSV_P_DW * 32) + dw * 32 + 2 * cp) = make_double2(s0, s1);
                stage_R(col);
                prefetch_dots(col - 1);
                prefetch_R(col - 1);
            }
            lds_barrier();
        }
    }
    __syncthreads();
    for (int q = t; q < n; q += 512) vec[q] = xs[q];
}
