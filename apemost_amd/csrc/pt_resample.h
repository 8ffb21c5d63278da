// pt_resample.h -- on-device resampling: M equally weighted posterior draws at any beta_t >= 0 from EVERY kept step of
// EVERY chain, beside the reweight fold (pt_reweight.h).  The weights are that fold's: mbar_row_kernel, mbar_max_kernel
// and reweight_weights_kernel as they are leave the fixed-point integers q_n of one target in q[t_count][n_chains].
// Per ladder, over the kept steps [t0, t0 + t_count), sample n = 0 .. N-1 in MBAR's stored order (mbar_at), M draws and
// the caller's uint64 u:
//   C_n = q_0 + ... + q_n                         (uint64; Q = C_{N-1} = q_total < 2^63, pt_reweight.h)
//   a = Q div M,  b = Q mod M,  o = mulhi64(u, a) (the high 64 bits of the 128-bit product u a)
//   p_m = m a + (m b) div M + o,  m = 0 .. M-1
//   draw m is the smallest n with C_n > p_m.
// This is systematic resampling with an integer offset: the positions are Q / M apart (m a + floor(m b / M) is
// floor(m Q / M)) and the offset o takes the place of the uniform in [0, Q / M).  64-bit integers suffice:
//   * the largest e of a ladder is exactly 1, so Q >= 2^shift >= 2^34 (shift = 63 - bit_length(N), N <= 2^28), and
//     M <= 2^24 gives a >= 2^10 >= 1; u < 2^64 gives 0 <= o <= a - 1;
//   * m < M <= 2^24 and b < M give m b < 2^48; m a <= (M - 1) a <= Q < 2^63;
//   * floor(m b / M) is non-decreasing in m and a >= 0, so p_m is non-decreasing;
//   * p_{M-1} <= (M - 1) a + floor((M - 1) b / M) + a - 1 <= M a + b - 1 = Q - 1 (the floor is below b where b > 0 and 0
//     where b = 0): every p_m is below Q, so the smallest n with C_n > p_m exists.
// A sample with q_n = 0 has C_n = C_{n-1} and is never the smallest; sample n owns the positions [C_{n-1}, C_n), an
// interval of length q_n on a lattice of spacing Q / M, so it is drawn floor(M q_n / Q) or ceil(M q_n / Q) times.  The
// draws come out in stored order (time-major, the chain fastest): equally weighted, not exchangeable in order.
//
// No floating point and no atomics: integer addition is associative, so C, and with it every index, is the same
// whatever the grid, the tile and the workgroup sizes.
//
// Kernels (the tiles are MBAR's: kMbarTile = 4096 samples counted from the range's first):
//   resample_tile_sum_kernel   grid (tiles, n_ladders), 256 threads: tsum[ladder][tile] = the sum of the tile's q.
//   resample_tile_scan_kernel  grid (n_ladders), 256 threads: the exclusive scan of a ladder's tile sums in place and
//                              Q into total[ladder].  A pass of the workgroup covers kResampleScanThreads = 256 tiles
//                              (one per thread) and hands its sum to the next pass; 2^28 / 4096 = 65 536 tiles are 256
//                              passes.
//   resample_scan_kernel       grid (tiles, n_ladders), 256 threads: C of the tile into C[ladder][N].  A wave takes 1024
//                              consecutive samples as 16 rows of 64 (a lane's loads and stores are contiguous with its
//                              neighbours'), scans each row with six 64-bit cross-lane moves (__shfl_up: in registers,
//                              no LDS traffic; the 64-bit form saves the carry logic of two 32-bit scans and costs the
//                              same two moves a step) and carries lane 63 into the next row; the four wave totals meet
//                              in 32 B of LDS, once per tile.  C is written rather than fused into the search: M
//                              threads would otherwise each rescan a tile, and a search over a stored C is 12 loads.
//   resample_search_kernel     grid (ceil(M / 256), n_ladders), 256 threads, one thread per draw: p_m, a binary search
//                              over the tile prefixes (the last tile whose exclusive prefix is <= p_m), a binary search
//                              in that tile's C, index[ladder][m] and the n_cols stored values into
//                              x[ladder][m][col].
// C [n_ladders][N] (as many words as q's [t_count][n_chains]) and tsum [n_ladders][tiles_max] are allocated by the first
// resample of a fold at the fold's capacity and freed with the fold's memory (reweight_end, mbar_begin, mbar_end,
// destroy): a fold that never resamples pays nothing.
// Plain vector stores, no scratch memory.  Registers and LDS (hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage) are stated beside each kernel: tile sums 16, tile scan 26, scan 60, search 12;
// 32 B of LDS in the first three; no kernel has scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_mbar.h"
#include "pt_reweight.h"

namespace apemost {

constexpr int kResampleThreads = 256;
constexpr int kResampleScanThreads = 256;        // tiles a pass of resample_tile_scan_kernel covers
constexpr unsigned int kResampleMaxDraws = 1u << 24;
constexpr int kResampleRows = kMbarTile / kResampleThreads; // rows of 64 samples a wave scans: 16

struct ResampleArgs {
    MbarArgs m;                        // the range and the store (mbar_at)
    const unsigned long long *q;       // [t_count][n_chains]
    const double *x;                   // [n_cols][col_stride]
    size_t col_stride;
    int n_cols;
    unsigned long long *tsum;          // [n_ladders][tiles]: the tile sums, then their exclusive scan
    unsigned long long *total;         // [n_ladders]: Q
    unsigned long long *C;             // [n_ladders][N]
    unsigned int M;
    unsigned long long u;
    unsigned int *index;               // [n_ladders][M]
    double *out;                       // [n_ladders][M][n_cols]
};

// the inclusive scan of v over the wave's 64 lanes
__device__ __forceinline__ unsigned long long resample_wave_scan(unsigned long long v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned long long up = __shfl_up(v, off);
        if (lane >= off)
            v += up;
    }
    return v;
}

// grid (tiles, n_ladders).  16 VGPRs, 8 waves per SIMD; 32 B of LDS.
__global__ void __launch_bounds__(kResampleThreads) resample_tile_sum_kernel(ResampleArgs a) {
    __shared__ unsigned long long wsum[kResampleThreads / 64];
    const int b = blockIdx.y;
    const unsigned int tile = blockIdx.x, base = tile * (unsigned int)kMbarTile;
    const int cnt = a.m.N - base < (unsigned int)kMbarTile ? (int)(a.m.N - base) : kMbarTile;
    const size_t rel = (size_t)a.m.t0 * a.m.n_chains;
    unsigned long long s = 0;
    for (int i = threadIdx.x; i < cnt; i += kResampleThreads)
        s += a.q[mbar_at(a.m, b, base + i) - rel];
    for (int off = 32; off >= 1; off >>= 1)
        s += __shfl_xor(s, off);
    if ((threadIdx.x & 63) == 0)
        wsum[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0)
        a.tsum[(size_t)b * a.m.tiles + tile] = (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
}

// grid (n_ladders).  26 VGPRs; 32 B of LDS.
__global__ void __launch_bounds__(kResampleScanThreads) resample_tile_scan_kernel(ResampleArgs a) {
    __shared__ unsigned long long wsum[kResampleScanThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long *t = a.tsum + (size_t)blockIdx.x * a.m.tiles;
    unsigned long long carry = 0;
    for (unsigned int k0 = 0; k0 < a.m.tiles; k0 += kResampleScanThreads) {
        const unsigned int k = k0 + threadIdx.x;
        const unsigned long long v = k < a.m.tiles ? t[k] : 0;
        const unsigned long long inc = resample_wave_scan(v, lane);
        if (lane == 63)
            wsum[wave] = inc;
        __syncthreads();
        unsigned long long before = carry, all = carry;
#pragma unroll
        for (int w = 0; w < kResampleScanThreads / 64; w++) {
            if (w < wave)
                before += wsum[w];
            all += wsum[w];
        }
        if (k < a.m.tiles)
            t[k] = before + (inc - v);
        carry = all;
        __syncthreads(); // (wsum is written again by the next pass)
    }
    if (threadIdx.x == 0)
        a.total[blockIdx.x] = carry;
}

// grid (tiles, n_ladders); tsum holds the exclusive scan.  60 VGPRs (the wave's 16 rows stay in registers between the
// scan and the store), 8 waves per SIMD; 32 B of LDS.
__global__ void __launch_bounds__(kResampleThreads) resample_scan_kernel(ResampleArgs a) {
    __shared__ unsigned long long wsum[kResampleThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y;
    const unsigned int tile = blockIdx.x;
    const unsigned int base = tile * (unsigned int)kMbarTile + (unsigned int)(wave * kResampleRows * 64);
    const size_t rel = (size_t)a.m.t0 * a.m.n_chains;
    unsigned long long v[kResampleRows];
#pragma unroll
    for (int j = 0; j < kResampleRows; j++) {
        const unsigned int n = base + (unsigned int)(j * 64 + lane);
        v[j] = n < a.m.N ? a.q[mbar_at(a.m, b, n) - rel] : 0;
    }
    unsigned long long carry = 0;
#pragma unroll
    for (int j = 0; j < kResampleRows; j++) {
        v[j] = resample_wave_scan(v[j], lane) + carry;
        carry = __shfl(v[j], 63);
    }
    if (lane == 0)
        wsum[wave] = carry;
    __syncthreads();
    unsigned long long before = a.tsum[(size_t)b * a.m.tiles + tile];
#pragma unroll
    for (int w = 0; w < kResampleThreads / 64; w++)
        if (w < wave)
            before += wsum[w];
    unsigned long long *C = a.C + (size_t)b * a.m.N;
#pragma unroll
    for (int j = 0; j < kResampleRows; j++) {
        const unsigned int n = base + (unsigned int)(j * 64 + lane);
        if (n < a.m.N)
            C[n] = v[j] + before;
    }
}

// grid (ceil(M / 256), n_ladders).  12 VGPRs (Q, a and b are uniform: the divisions are scalar but for (m b) div M),
// 8 waves per SIMD, no LDS.
__global__ void __launch_bounds__(kResampleThreads) resample_search_kernel(ResampleArgs a) {
    const unsigned int m = blockIdx.x * kResampleThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (m >= a.M)
        return;
    const unsigned long long Q = a.total[b], M = a.M;
    const unsigned long long qa = Q / M, qb = Q - qa * M;
    const unsigned long long p = (unsigned long long)m * qa + ((unsigned long long)m * qb) / M + __umul64hi(a.u, qa);
    // the last tile whose exclusive prefix is <= p (prefix[0] = 0 <= p): the draw's tile, since p < Q
    const unsigned long long *pre = a.tsum + (size_t)b * a.m.tiles;
    unsigned int lo = 0, hi = a.m.tiles; // pre[lo] <= p, and pre[hi] > p where hi < tiles
    while (hi - lo > 1) {
        const unsigned int mid = lo + (hi - lo) / 2;
        if (pre[mid] <= p)
            lo = mid;
        else
            hi = mid;
    }
    // the smallest n of the tile with C_n > p
    const unsigned long long *C = a.C + (size_t)b * a.m.N;
    unsigned int first = lo * (unsigned int)kMbarTile;
    unsigned int last = a.m.N - first < (unsigned int)kMbarTile ? a.m.N : first + (unsigned int)kMbarTile; // one past
    while (first < last) {
        const unsigned int mid = first + (last - first) / 2;
        if (C[mid] > p)
            last = mid;
        else
            first = mid + 1;
    }
    if (first >= a.m.N)
        first = a.m.N - 1; // (unreachable: p < Q = C_{N-1}; keeps the gather inside the store whatever total holds)
    if (a.index)
        a.index[(size_t)b * a.M + m] = first;
    if (a.out) {
        const size_t at = mbar_at(a.m, b, first);
        double *dst = a.out + ((size_t)b * a.M + m) * a.n_cols;
        for (int k = 0; k < a.n_cols; k++)
            dst[k] = a.x[(size_t)k * a.col_stride + at];
    }
}

} // namespace apemost
