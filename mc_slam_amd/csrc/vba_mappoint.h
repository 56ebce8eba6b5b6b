// vba_mappoint.h -- batched map-point refresh on the GPU.
// Replaces, for a batch of point lists, the bodies of MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cpp:366-411) and
// MapPoint::UpdateNormalAndDepth (:470-498).  The exits in front of them (not asked, no observation, no good keyframe), the gather of
// the good keyframes' descriptors and the item table are the host's (vba_host_mappoint.h); the state codes are those of
// include/vislam_ba.h.
//
// Items.  Work per point grows with N^2 and N is ragged, so the host sorts the points of the whole call by their observation count:
// a point of more than VBA_MP_WAVE_OBS observations is a workgroup item (one 256-lane workgroup, all 32 KB of LDS), every other point
// is a wave item, and four wave items, neighbours in the sorted table and so of similar size, share a workgroup, each wave with its
// 8 KB slice.  The kind follows the observation count, bad keyframes counted, and not N: it bounds both parts at once and depends on
// nothing but the point.
//
// Descriptor part.  The group (64 or 256 lanes) stages the N descriptors into its slice; lane l owns the rows l, l + lanes, ... (at
// most VBA_MP_ROWS), holds them in registers and reads descriptor j from LDS, the same address in every lane: a broadcast.  No row is
// sorted and no N x N matrix is stored: the lower median of row i, vDists[(int)(0.5 * (N - 1))], is the smallest d in 0 .. 256 with
// #{j : dist(i, j) <= d} > (N - 1) / 2, and nine bisection passes over the value range find it with popcounts alone; one pass serves
// all rows of a lane, so a descriptor is read once per pass.  The winner is the minimum of (median << 16) | row: the earliest row
// among equal medians, as the strict < of :397 leaves it.
//
// Normal part.  Lanes stride over the observations; unit vectors and sums are FP64 without contraction.  A lane sums its own terms in
// order, the wave combines them in a butterfly (every lane ends with the same bits), a workgroup item adds its four wave sums in
// wave order.  The shape depends on the item's kind and on nothing else, so a point's answer is bit-identical wherever it stands in
// the batch.  No floating-point atomics, no wait on another workgroup, and every loop is bounded by the item's counts, which the
// host checked against VBA_MP_MAX_OBS (and which the kernel clamps to its slice once more).
#pragma once
#include "vba_device.h"
#include "vba_layout.h"
#include "vba_search_area.h"

#define MP_NT VBA_MP_NT

DEVI int mp_wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = min(v, __shfl_xor(v, m));
    return v;
}
DEVI double mp_wave_sum(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m);
    return v;
}

__global__ void __launch_bounds__(MP_NT) k_mappoint_update(MpBatch B) {
#pragma clang fp contract(off)
    __shared__ uint4 mp_desc[2 * VBA_MP_MAX_OBS];   // 32 KB: 1024 descriptors, or four slices of 256
    __shared__ int mp_key[4];
    __shared__ int mp_zero[4];
    __shared__ double mp_sum[4][3];
    const int tid = threadIdx.x, wave = tid >> 6;
    const bool big = (int)blockIdx.x < B.n_big;     // uniform in the workgroup
    const int nl = big ? MP_NT : 64;                // lanes of the group that owns the item
    const int l = big ? tid : (tid & 63);
    const int it = __builtin_amdgcn_readfirstlane(big ? (int)blockIdx.x : B.n_big + 4 * ((int)blockIdx.x - B.n_big) + wave);
    const bool live = it < B.n_items;               // the last workgroup of wave items may have idle waves
    const MpItem& I = B.item[live ? it : 0];
    const int cap = big ? VBA_MP_MAX_OBS : VBA_MP_WAVE_OBS;
    const int n = live ? min(I.n_desc, cap) : 0;
    const int n_obs = live ? min(I.n_obs, VBA_MP_MAX_OBS) : 0;
    uint4* slice = mp_desc + (big ? 0 : wave * (2 * VBA_MP_WAVE_OBS));

    // the descriptors of the good keyframes into the slice, 16 bytes per lane and step
    {
        const uint4* src = reinterpret_cast<const uint4*>(B.desc + 8 * (size_t)I.desc0);
        for (int q = l; q < 2 * n; q += nl) slice[q] = src[q];
    }
    __syncthreads();

    if (n > 0) {
        const int k = (n - 1) >> 1;                 // (int)(0.5 * (N - 1)) (:394)
        const int nr = (n + nl - 1) / nl;           // rows of the busiest lane, at most VBA_MP_ROWS
        unsigned int a[VBA_MP_ROWS][8];
        int lo[VBA_MP_ROWS], hi[VBA_MP_ROWS];
#pragma unroll
        for (int r = 0; r < VBA_MP_ROWS; r++) {
            const int i = min(l + nl * r, n - 1);   // a lane without a row r counts for the last row; its key is dropped below
            const uint4 x = slice[2 * i], y = slice[2 * i + 1];
            a[r][0] = x.x; a[r][1] = x.y; a[r][2] = x.z; a[r][3] = x.w;
            a[r][4] = y.x; a[r][5] = y.y; a[r][6] = y.z; a[r][7] = y.w;
            lo[r] = 0; hi[r] = 256;
        }
        for (int pass = 0; pass < 9; pass++) {      // 257 values: nine halvings
            int cnt[VBA_MP_ROWS] = {0, 0, 0, 0};
            for (int j = 0; j < n; j++) {
                const uint4 x = slice[2 * j], y = slice[2 * j + 1];
                const unsigned int d[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
#pragma unroll
                for (int r = 0; r < VBA_MP_ROWS; r++)
                    if (r < nr) cnt[r] += (sa_hamming(a[r], d) <= ((lo[r] + hi[r]) >> 1)) ? 1 : 0;
            }
#pragma unroll
            for (int r = 0; r < VBA_MP_ROWS; r++) {
                const int mid = (lo[r] + hi[r]) >> 1;
                if (cnt[r] > k) hi[r] = mid; else lo[r] = mid + 1;
            }
        }
        int key = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < VBA_MP_ROWS; r++) {
            const int i = l + nl * r;
            if (r < nr && i < n) key = min(key, (lo[r] << 16) | i);
        }
        key = mp_wave_min(key);
        if (big) {
            if ((tid & 63) == 0) mp_key[wave] = key;
            __syncthreads();
            key = min(min(mp_key[0], mp_key[1]), min(mp_key[2], mp_key[3]));
        }
        if (l == 0) B.best[it] = key;
    } else if (live && l == 0) {
        B.best[it] = -1;
    }

    if (n_obs > 0) {
        const double px = I.pos[0], py = I.pos[1], pz = I.pos[2];
        const int* ob = B.obs + (size_t)I.obs0;
        double sx = 0.0, sy = 0.0, sz = 0.0;
        int zero = 0;
        for (int o = l; o < n_obs; o += nl) {       // :472-481, bad keyframes included
            const double* c = B.center + 3 * (size_t)ob[o];
            const double dx = px - c[0], dy = py - c[1], dz = pz - c[2];
            const double nn = sqrt((dx * dx + dy * dy) + dz * dz);
            if (nn == 0.0) {
                zero = 1;                           // the reference divides by zero here
            } else {
                sx = sx + dx / nn; sy = sy + dy / nn; sz = sz + dz / nn;
            }
        }
        sx = mp_wave_sum(sx); sy = mp_wave_sum(sy); sz = mp_wave_sum(sz);
        zero = __any(zero) ? 1 : 0;
        if (big) {
            if ((tid & 63) == 0) { mp_sum[wave][0] = sx; mp_sum[wave][1] = sy; mp_sum[wave][2] = sz; mp_zero[wave] = zero; }
            __syncthreads();
            sx = ((mp_sum[0][0] + mp_sum[1][0]) + mp_sum[2][0]) + mp_sum[3][0];
            sy = ((mp_sum[0][1] + mp_sum[1][1]) + mp_sum[2][1]) + mp_sum[3][1];
            sz = ((mp_sum[0][2] + mp_sum[1][2]) + mp_sum[2][2]) + mp_sum[3][2];
            zero = mp_zero[0] | mp_zero[1] | mp_zero[2] | mp_zero[3];
        }
        if (l == 0) {
            double* out = B.nrm + 5 * (size_t)it;
            if (zero) {
                out[0] = out[1] = out[2] = out[3] = out[4] = 0.0;
                B.nstate[it] = 3;
            } else {
                const double cnt = (double)n_obs;   // :498
                const double* c = B.center + 3 * (size_t)I.ref;
                const double dx = px - c[0], dy = py - c[1], dz = pz - c[2];
                const double dist = sqrt((dx * dx + dy * dy) + dz * dz);   // :484-485
                const double dmax = dist * I.ref_scale;                    // :494
                out[0] = sx / cnt; out[1] = sy / cnt; out[2] = sz / cnt;
                out[3] = dmax;
                out[4] = dmax / I.ref_top_scale;                           // :496
                B.nstate[it] = 0;
            }
        }
    } else if (live && l == 0) {
        B.nstate[it] = 1;
    }
}
