// pt_reweight.h -- on-device reweighted posteriors: the moments and the marginal histograms of chosen columns of the
// sample row at any beta_t >= 0, sampled or not, from EVERY kept step of EVERY chain with the MBAR weights of
// pt_mbar.h.  The fold is attached to an open MBAR fold and keeps, beside its ell[capacity][n_chains], the columns
// x[n_cols][capacity][n_chains]: every column has the layout of ell, so mbar_at addresses it and a wave's loads are
// contiguous.  Per ladder, over the kept steps [t0, t0 + t_count), sample n in MBAR's stored order, N = t_count * K:
//   lnD_n, x_tn = beta_t * l_n - lnD_n, the exact maximum m_t and e_n = exp(x_tn - m_t)
// are those of pt_mbar.h (mbar_row_kernel and mbar_max_kernel as they are).  Contraction is off and every line is one
// rounding.
//
// Moments, about the range's first sample of the ladder: origin_a = x_a of sample 0, d_a = x_a,n - origin_a;
//   the terms  e_n;  (e_n * e_n);  (e_n * d_a);  ((e_n * d_a) * d_b), a <= b   of S0, SS, S1[a], cross[a][b].
// Every sum follows the order of pt_mbar.h: tiles of 4096 samples counted from the range's first; in a tile lane i of
// 64 starts at +0.0 and adds the terms of samples i, i + 64, ... in that order; the 64 partials go through the
// adjacent-pairs tree (joint_tree_sum, the association of wave_allreduce_sum); the tile partials are added in tile
// order from +0.0.  m, S0 and SS are therefore mbar_evaluate's on the bits.
//
// Weighted histograms, exact and order-free.  The bins are the run summary's: summary_edge and summary_bin over
// [lo[a], hi[a]], nbins bins; values outside, NaN included, are not counted.  A sample's weight is the fixed-point
// integer
//   q_n = (uint64) rint(ldexp(e_n, s)),   s = 63 - bit_length(N):
// the scaling is exact (a power of two, upwards), rint is the one rounding, and e <= 1 gives sum q <= N 2^s < 2^63.
// hist[a][bin] = sum of q_n over the samples in the bin, q_total = sum of q_n over all samples: integer sums, the same
// on any grid and in any order.  |q_n - 2^s e_n| <= 1/2, so a bin differs from 2^s sum e by at most N_bin / 2, that is
// from sum e by N_bin 2^-(s+1); S0 is at least Kish's effective sample size S0^2 / SS (SS <= S0 because e <= 1), so
// relative to the normalisation the error of a bin is at most N 2^-(s+1) / ESS: below 2^-33 at N = 2^28 and ESS = 1,
// below 2^-46 at N = 16 000.
//
// Kernels:
//   reweight_gather_kernel   mbar_gather_kernel for the columns: grid z is the column; every stored value that is not
//                            finite adds 1 to n_bad[ladder][column] (an integer atomic).
//   reweight_weights_kernel  grid (ceil(N / 256), n_ladders): e_n and q_n of one target into e, q [t_count][n_chains].
//   reweight_moments_kernel  grid (tiles, ceil(items / 4), n_ladders), 256 threads, one item per wave.  With 16
//                            columns there are 154 sums per sample; an item is what a wave carries in registers
//                            through its tile: item 0 is S0 and SS; the others are (a, g): S1[a] where g = 0 and the
//                            cross sums of a with the columns a + 4 g .. a + 4 g + 3.  A lane's walk is samples lane,
//                            lane + 64, ...: consecutive lanes read consecutive doubles of e and of a column.  The
//                            tile partials go to part[word][ladder][tile], word = 0: S0, 1: SS, 2 + a: S1[a],
//                            2 + n_cols + tri(a, b): cross[a][b], tri the upper triangle row-major.
//   reweight_hist_kernel     grid (G, n_cols, n_ladders), 256 threads: a workgroup takes the tiles x, x + G, ... of
//                            one column into a histogram of its own in LDS (uint64 [nbins], ds_add_u64; the edges
//                            beside it, 64 KiB in all) and adds every non-zero bin to the result with one global
//                            integer atomic.  The workgroups of column 0 add q_total.
//   reweight_finish_kernel   one thread per (ladder, word) adds its tile partials in tile order and writes the result
//                            where the caller's arrays want it.
// No float atomics, plain vector stores, no scratch.  Registers (hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage) are stated beside each kernel: gather 12, weights 30, moments 36, histogram 24,
// finish 26; no kernel has scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_mbar.h"
#include "pt_summary.h"

namespace apemost {

constexpr int kReweightMaxCols = 16;
constexpr int kReweightMaxBins = 4096;
constexpr int kReweightSide = 4;       // cross sums of an item
constexpr int kReweightThreads = 256;
constexpr int kReweightHistGrid = 256; // workgroups of the histogram kernel per (column, ladder), at most

struct ReweightGatherArgs {
    const double *rows;                // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, K, n_cols;
    int cols[kReweightMaxCols];
    unsigned long long skip, thin;     // kept steps of this piece: skip, skip + thin, ... (n of them)
    unsigned int n;
    double *x;                         // column 0 of the store from the first row this piece fills
    size_t col_stride;                 // capacity * n_chains
    unsigned long long *n_bad;         // [n_ladders][n_cols]
};

// grid (ceil(n_chains / 256), ceil(n / 8), n_cols).  12 VGPRs, 8 waves per SIMD.
__global__ void __launch_bounds__(kMbarGatherThreads) reweight_gather_kernel(ReweightGatherArgs a) {
    const int c = blockIdx.x * kMbarGatherThreads + threadIdx.x;
    if (c >= a.n_chains)
        return;
    const int k = blockIdx.z;
    const size_t w = (size_t)a.n_par + 2, row = (size_t)a.n_chains * w;
    const double *src = a.rows + a.skip * row + (size_t)c * w + a.cols[k];
    const size_t stride = (size_t)a.thin * row;
    double *dst = a.x + (size_t)k * a.col_stride;
    const unsigned int i0 = blockIdx.y * 8u;
    unsigned long long bad = 0;
#pragma unroll
    for (unsigned int r = 0; r < 8u; r++) {
        const unsigned int i = i0 + r;
        if (i >= a.n)
            break;
        const double v = src[i * stride];
        dst[(size_t)i * a.n_chains + c] = v;
        bad += !(__builtin_fabs(v) < __builtin_inf()); // (NaN compares false)
    }
    if (bad)
        atomicAdd(&a.n_bad[(size_t)(c / a.K) * a.n_cols + k], bad);
}

struct ReweightArgs {
    MbarArgs m;                        // the range and the store; one target: beta_t[0], mkey[ladder]; part
                                       // [words][part_stride], word w: [n_ladders][tiles]
    const double *x;                   // [n_cols][col_stride]
    size_t col_stride;
    int n_cols, nbins, shift;
    const double *lo, *hi;             // [n_cols]
    double *e;                         // [t_count][n_chains]
    unsigned long long *q;             // [t_count][n_chains]
    unsigned long long *hist;          // this target's [n_cols][nbins] of ladder 0; ladder b: + b * hist_stride
    unsigned long long *q_total;       // this target's word of ladder 0; ladder b: + b * n_t
    size_t hist_stride;
    int n_t, t;                        // the targets of the call and this one: where finish writes
    double *out_m, *out_S0, *out_SS;   // [n_ladders][n_t]
    double *out_S1, *out_cross;        // [n_ladders][n_t][n_cols], [n_ladders][n_t][n_cols (n_cols + 1) / 2]
};

// grid (ceil(N / 256), n_ladders).  30 VGPRs, 8 waves per SIMD.
__global__ void __launch_bounds__(kReweightThreads) reweight_weights_kernel(ReweightArgs a) {
#pragma clang fp contract(off)
    const unsigned int n = blockIdx.x * kReweightThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= a.m.N)
        return;
    const size_t at = mbar_at(a.m, b, n);
    const double prod = a.m.beta_t[0] * a.m.ell[at];
    const double x = prod - a.m.lnD[at];
    const double e = exp(x - mbar_unkey(a.m.mkey[b]));
    const size_t o = at - (size_t)a.m.t0 * a.m.n_chains;
    a.e[o] = e;
    a.q[o] = (unsigned long long)rint(ldexp(e, a.shift));
}

// the items of n_cols columns: 1 + sum over a of ceil((n_cols - a) / 4)
__host__ __device__ inline int reweight_items(int n_cols) {
    int n = 1;
    for (int a = 0; a < n_cols; a++)
        n += (n_cols - a + kReweightSide - 1) / kReweightSide;
    return n;
}

// grid (tiles, ceil(items / 4), n_ladders).  36 VGPRs (S1, four cross sums, four origins), 8 waves per SIMD, no LDS.
__global__ void __launch_bounds__(kReweightThreads) reweight_moments_kernel(ReweightArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.z;
    const unsigned int tile = blockIdx.x, base = tile * (unsigned int)kMbarTile;
    const int cnt = a.m.N - base < (unsigned int)kMbarTile ? (int)(a.m.N - base) : kMbarTile;
    int item = (int)blockIdx.y * (kReweightThreads / 64) + wave;
    const size_t rel = (size_t)a.m.t0 * a.m.n_chains;
    double *part = a.m.part + (size_t)b * a.m.tiles + tile;
    if (item == 0) {
        double s0 = 0.0, ss = 0.0;
#pragma unroll 4
        for (int i = lane; i < cnt; i += 64) {
            const double e = a.e[mbar_at(a.m, b, base + i) - rel];
            const double ee = e * e;
            s0 += e;
            ss += ee;
        }
        s0 = wave_allreduce_sum(s0);
        ss = wave_allreduce_sum(ss);
        if (lane == 0) {
            part[0] = s0;
            part[a.m.part_stride] = ss;
        }
        return;
    }
    // item -> (ca, g)
    item -= 1;
    int ca = 0;
    for (; ca < a.n_cols; ca++) {
        const int groups = (a.n_cols - ca + kReweightSide - 1) / kReweightSide;
        if (item < groups)
            break;
        item -= groups;
    }
    if (ca >= a.n_cols)
        return; // (a wave beyond the last item)
    const int g = item, b0 = ca + g * kReweightSide;
    const int nb = a.n_cols - b0 < kReweightSide ? a.n_cols - b0 : kReweightSide;
    const size_t first = mbar_at(a.m, b, 0);
    const double *xa = a.x + (size_t)ca * a.col_stride, *xb = a.x + (size_t)b0 * a.col_stride;
    const double oa = xa[first];
    double ob[kReweightSide], c[kReweightSide];
#pragma unroll
    for (int j = 0; j < kReweightSide; j++) {
        ob[j] = j < nb ? xb[(size_t)j * a.col_stride + first] : 0.0;
        c[j] = 0.0;
    }
    double s1 = 0.0;
#pragma unroll 2
    for (int i = lane; i < cnt; i += 64) {
        const size_t at = mbar_at(a.m, b, base + i);
        const double e = a.e[at - rel];
        const double da = xa[at] - oa;
        const double ed = e * da;
        s1 += ed;
#pragma unroll
        for (int j = 0; j < kReweightSide; j++)
            if (j < nb) {
                const double db = xb[(size_t)j * a.col_stride + at] - ob[j];
                const double edd = ed * db;
                c[j] += edd;
            }
    }
    if (g == 0) {
        s1 = wave_allreduce_sum(s1);
        if (lane == 0)
            part[(size_t)(2 + ca) * a.m.part_stride] = s1;
    }
    const int tri = ca * a.n_cols - ca * (ca - 1) / 2 + (b0 - ca);
#pragma unroll
    for (int j = 0; j < kReweightSide; j++)
        if (j < nb) {
            const double s = wave_allreduce_sum(c[j]);
            if (lane == 0)
                part[(size_t)(2 + a.n_cols + tri + j) * a.m.part_stride] = s;
        }
}

// grid (G, n_cols -- with nbins = 0: 1 --, n_ladders); hist and q_total zeroed before.  24 VGPRs; 65 552 B of LDS, so
// two workgroups per CU.
__global__ void __launch_bounds__(kReweightThreads) reweight_hist_kernel(ReweightArgs a) {
    __shared__ double edges[kReweightMaxBins + 1];
    __shared__ unsigned long long h[kReweightMaxBins];
    const int b = blockIdx.z, col = blockIdx.y;
    if (a.nbins > 0) {
        const double lo = a.lo[col], hi = a.hi[col];
        for (int i = threadIdx.x; i <= a.nbins; i += kReweightThreads) {
            edges[i] = summary_edge(lo, hi, i, a.nbins);
            if (i < a.nbins)
                h[i] = 0;
        }
    }
    __syncthreads();
    const size_t rel = (size_t)a.m.t0 * a.m.n_chains;
    const double *x = a.x + (size_t)col * a.col_stride;
    unsigned long long tot = 0;
    for (unsigned int tile = blockIdx.x; tile < a.m.tiles; tile += gridDim.x) {
        const unsigned int base = tile * (unsigned int)kMbarTile;
        const int cnt = a.m.N - base < (unsigned int)kMbarTile ? (int)(a.m.N - base) : kMbarTile;
        for (int i = threadIdx.x; i < cnt; i += kReweightThreads) {
            const size_t at = mbar_at(a.m, b, base + i);
            const unsigned long long q = a.q[at - rel];
            tot += q;
            if (a.nbins > 0 && q) {
                const int bin = summary_bin(x[at], edges, a.nbins);
                if (bin >= 0)
                    atomicAdd(&h[bin], q);
            }
        }
    }
    __syncthreads();
    if (a.nbins > 0) {
        unsigned long long *dst = a.hist + (size_t)b * a.hist_stride + (size_t)col * a.nbins;
        for (int i = threadIdx.x; i < a.nbins; i += kReweightThreads)
            if (h[i])
                atomicAdd(&dst[i], h[i]);
    }
    if (col == 0) {
        for (int off = 32; off >= 1; off >>= 1)
            tot += __shfl_xor(tot, off);
        if ((threadIdx.x & 63) == 0 && tot)
            atomicAdd(&a.q_total[(size_t)b * a.n_t], tot);
    }
}

// grid ceil(n_ladders * words / 64), words = 2 + n_cols + n_cols (n_cols + 1) / 2.  26 VGPRs.
__global__ void __launch_bounds__(64) reweight_finish_kernel(ReweightArgs a, int n_ladders) {
#pragma clang fp contract(off)
    const int ntri = a.n_cols * (a.n_cols + 1) / 2, words = 2 + a.n_cols + ntri;
    const size_t idx = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (idx >= (size_t)n_ladders * words)
        return;
    const int b = (int)(idx / words), w = (int)(idx - (size_t)b * words);
    const double *p = a.m.part + (size_t)w * a.m.part_stride + (size_t)b * a.m.tiles;
    double s = 0.0;
#pragma unroll 8
    for (unsigned int k = 0; k < a.m.tiles; k++)
        s += p[k];
    const size_t bt = (size_t)b * a.n_t + a.t;
    if (w == 0) {
        a.out_S0[bt] = s;
        a.out_m[bt] = mbar_unkey(a.m.mkey[b]);
    } else if (w == 1)
        a.out_SS[bt] = s;
    else if (w < 2 + a.n_cols)
        a.out_S1[bt * a.n_cols + (w - 2)] = s;
    else
        a.out_cross[bt * ntri + (w - 2 - a.n_cols)] = s;
}

} // namespace apemost
