// pt_mbar.h -- on-device MBAR (multistate Bennett acceptance ratio, Shirts & Chodera 2008): the free energies
// ln Z(beta_k) of a tempered ladder from the loglike of EVERY kept step of EVERY chain, and the weights that carry any
// of those samples to any beta.  A ladder has K chains, beta_0 > ... > beta_{K-1} > 0; its sample n = (kept step t,
// chain c), in stored order (step-major, the chain fastest), has l_n = v / beta_c with v column n_par+1 of the row
// (one IEEE division).  With g_k the running estimate of ln Z(beta_k) and T kept steps in the range used:
//   lnD_n = ln sum_j exp(beta_j l_n + c_j),   c_j = ln T - g_j                 (row pass)
//   G_t   = ln sum_n exp(beta_t l_n - lnD_n)                                   (column pass, any target beta_t)
//   g <- G(g) at the sampled betas                                             (one self-consistent iteration)
// G(g + a) = G(g) + a, so nothing here normalises: the caller subtracts g_0.
//
// The order of every operation.  Contraction is off and every line is one rounding.
//   row pass, per sample:   x_j = beta_j * l + c_j (the product rounded, then the sum);
//                           m = x_0, then for j = 1 .. K-1 ascending: if (x_j > m) m = x_j;
//                           S = +0.0, then for j = 0 .. K-1 ascending: S = S + exp(x_j - m);
//                           lnD = m + log(S).
//   column pass, per target t:  x_n = beta_t * l_n - lnD_n (the product rounded, then the difference);
//                           m_t = max_n x_n (exact, whatever the order);  e_n = exp(x_n - m_t);  d_n = l_n - l_first with
//                           l_first the l of the range's first sample of the ladder;
//                           the terms  e_n;  (e_n * d_n);  ((e_n * d_n) * d_n);  (e_n * e_n)  of S0, S1, S2, SS.
//   the sums:               the range's samples are cut into tiles of 4096 in stored order, counted from the range's
//                           first sample.  In a tile, lane partial p[i], i = 0 .. 63, starts at +0.0 and adds the terms
//                           of samples i, i + 64, ..., i + 63 * 64 of the tile in that order; samples the ragged last
//                           tile lacks add nothing.  The 64 partials go through the adjacent-pairs tree of
//                           pt_pointwise_joint.h (joint_tree_sum, the association of wave_allreduce_sum).  The tile
//                           partials of a target are added sequentially in tile order, from +0.0.
//   an iteration:           g_t = m_t + log(S0_t), c_t = lnT - g_t.
// exp and log are the device library's fp64 functions.  Nothing depends on the grid, on the other ladders of a batch
// or on where the range starts in the store: a range equals a store that holds only its rows.
//
// Kernels:
//   mbar_gather_kernel   evidence_gather_kernel with a division: l of the kept steps of every chain appended to
//                        ell[capacity][n_chains]; every stored value that is not finite adds 1 to its ladder's n_bad
//                        (an integer atomic: the count is the same in any order).
//   mbar_row_kernel      grid (ceil(N / 256), n_ladders), one thread per sample.  beta_j and c_j are the same for the
//                        whole grid row: their addresses are uniform and nothing stores before them, so they are scalar
//                        loads (s_load) that cost the vector unit nothing; x_j is formed twice instead of being kept.
//   mbar_max_kernel, mbar_col_kernel
//                        grid (tiles, ceil(n_t / 16), n_ladders), 256 threads.  The workgroup loads its tile's l and
//                        lnD into LDS once (2 x 4096 doubles = 64 KiB, so two workgroups = eight waves per CU) and serves
//                        a group of up to 16 targets from it, wave w the targets w, w + 4, ... of the group: the target is
//                        wave-uniform and a lane's 64 samples are a stride-64 walk through LDS (consecutive lanes,
//                        consecutive doubles: no bank conflict).  The work is the exp: 4096 of them per target and
//                        tile against 64 KiB read from LDS, so the ALU bounds it at any occupancy that covers the
//                        latency of exp's dependent chain; the walk is unrolled by four, the exps of four samples side
//                        by side and only the additions in order.  The maxima meet in mkey[ladder][target] through an
//                        integer atomicMax on an order-preserving image of the double (mbar_key): exact and
//                        order-free.  mbar_col_kernel<false> forms S0 alone, what an iteration needs;
//                        mbar_col_kernel<true> all four sums.  Tile partials go to part[word][ladder][target][tile].
//   mbar_finish_kernel   one thread per (ladder, target) adds its tile partials in tile order; for an iteration it
//                        writes g and c, for an evaluation m, S0, S1, S2, SS and G = m + log(S0).
//   mbar_weights_kernel  beta_t * l_n - lnD_n - G_t (two rounded differences) per sample of the range.
// No float atomics, plain vector stores, no scratch.  Registers (hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage) are stated beside each kernel below; gather 22, finish 26, weights 9.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_device.h"

namespace apemost {

constexpr int kMbarTile = 4096;        // samples per tile: 64 lanes x 64 samples
constexpr int kMbarThreads = 256;      // max, col, row, weights: four waves
constexpr int kMbarGroup = 16;         // targets a workgroup serves from one tile
constexpr int kMbarGatherThreads = 256;
constexpr int kMbarWords = 4;          // S0, S1, S2, SS

struct MbarGatherArgs {
    const double *rows;                // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, K;            // K: chains per ladder
    unsigned long long skip, thin;     // kept steps of this piece: skip, skip + thin, ... (n of them)
    unsigned int n;
    const double *betas;               // [n_chains]
    double *ell;                       // the store from the first row this piece fills
    unsigned long long *n_bad;         // [n_ladders]
};

// grid (ceil(n_chains / 256), ceil(n / 8)): consecutive threads take consecutive chains of one kept step
__global__ void __launch_bounds__(kMbarGatherThreads) mbar_gather_kernel(MbarGatherArgs a) {
    const int c = blockIdx.x * kMbarGatherThreads + threadIdx.x;
    if (c >= a.n_chains)
        return;
    const size_t w = (size_t)a.n_par + 2, row = (size_t)a.n_chains * w;
    const double *src = a.rows + a.skip * row + (size_t)c * w + a.n_par + 1;
    const size_t stride = (size_t)a.thin * row;
    const double beta = a.betas[c];
    const unsigned int i0 = blockIdx.y * 8u;
    unsigned long long bad = 0;
#pragma unroll
    for (unsigned int r = 0; r < 8u; r++) {
        const unsigned int i = i0 + r;
        if (i >= a.n)
            break;
        const double l = src[i * stride] / beta;
        a.ell[(size_t)i * a.n_chains + c] = l;
        bad += !(__builtin_fabs(l) < __builtin_inf()); // (NaN compares false)
    }
    if (bad)
        atomicAdd(&a.n_bad[c / a.K], bad);
}

struct MbarArgs {
    const double *ell;                 // [capacity][n_chains]
    double *lnD;                       // [capacity][n_chains]
    int n_chains, K;
    unsigned long long t0;             // the range's first kept step
    unsigned int N;                    // samples of a ladder in the range: t_count * K, at most 2^28
    unsigned int tiles;                // ceil(N / 4096)
    const double *betas, *c;           // [n_chains]
    const double *beta_t;              // target t of ladder b: beta_t[b * t_stride + t]
    int t_stride, n_t;
    unsigned long long *mkey;          // [n_ladders][n_t]: mbar_key of the maxima
    double *part;                      // [kMbarWords][part_stride], word w: [n_ladders][n_t][tiles]
    size_t part_stride;
};

// where sample n of ladder b's range is stored
__device__ __forceinline__ size_t mbar_at(const MbarArgs &a, int b, unsigned int n) {
    const unsigned int t = n / (unsigned int)a.K, c = n - t * (unsigned int)a.K;
    return (size_t)(a.t0 + t) * a.n_chains + (size_t)b * a.K + c;
}

// an image of a double whose unsigned order is the double's order (no NaN comes here)
__device__ __forceinline__ unsigned long long mbar_key(double x) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(x);
    return (u >> 63) ? ~u : u | 0x8000000000000000ull;
}
__device__ __forceinline__ double mbar_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? k & 0x7fffffffffffffffull : ~k));
}

// grid (ceil(N / 256), n_ladders).  39 VGPRs, 8 waves per SIMD.
__global__ void __launch_bounds__(kMbarThreads) mbar_row_kernel(MbarArgs a) {
#pragma clang fp contract(off)
    const unsigned int n = blockIdx.x * kMbarThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= a.N)
        return;
    const size_t at = mbar_at(a, b, n);
    const double l = a.ell[at];
    const double *beta = a.betas + (size_t)b * a.K, *c = a.c + (size_t)b * a.K;
    double m;
    {
        const double prod = beta[0] * l;
        m = prod + c[0];
    }
    for (int j = 1; j < a.K; j++) {
        const double prod = beta[j] * l;
        const double x = prod + c[j];
        m = x > m ? x : m;
    }
    double S = 0.0;
#pragma unroll 4
    for (int j = 0; j < a.K; j++) {
        const double prod = beta[j] * l;
        const double x = prod + c[j];
        S += exp(x - m);
    }
    a.lnD[at] = m + log(S);
}

// the workgroup's tile into LDS; returns the samples it holds (1 .. 4096)
__device__ __forceinline__ int mbar_load_tile(const MbarArgs &a, int b, unsigned int tile, double *sl, double *sd) {
    const unsigned int base = tile * (unsigned int)kMbarTile;
    const int cnt = a.N - base < (unsigned int)kMbarTile ? (int)(a.N - base) : kMbarTile;
    for (int i = threadIdx.x; i < cnt; i += kMbarThreads) {
        const size_t at = mbar_at(a, b, base + i);
        sl[i] = a.ell[at];
        sd[i] = a.lnD[at];
    }
    __syncthreads();
    return cnt;
}

// grid (tiles, ceil(n_t / 16), n_ladders); mkey zeroed before (0 is below every key).  20 VGPRs, 64 KiB LDS.
__global__ void __launch_bounds__(kMbarThreads) mbar_max_kernel(MbarArgs a) {
#pragma clang fp contract(off)
    __shared__ double sl[kMbarTile], sd[kMbarTile];
    const int b = blockIdx.z;
    const int cnt = mbar_load_tile(a, b, blockIdx.x, sl, sd);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t_end = (int)(blockIdx.y + 1) * kMbarGroup < a.n_t ? (int)(blockIdx.y + 1) * kMbarGroup : a.n_t;
    for (int t = (int)blockIdx.y * kMbarGroup + wave; t < t_end; t += kMbarThreads / 64) {
        const double bt = a.beta_t[(size_t)b * a.t_stride + t];
        double m = -__builtin_inf();
        for (int i = lane; i < cnt; i += 64) {
            const double prod = bt * sl[i];
            const double x = prod - sd[i];
            m = x > m ? x : m;
        }
        for (int off = 32; off >= 1; off >>= 1) {
            const double o = __shfl_xor(m, off);
            m = o > m ? o : m;
        }
        if (lane == 0)
            atomicMax(&a.mkey[(size_t)b * a.n_t + t], mbar_key(m));
    }
}

// grid (tiles, ceil(n_t / 16), n_ladders).  FULL = false: 59 VGPRs; true: 73 VGPRs; 64 KiB LDS, so 2 waves per
// SIMD whatever the registers.
template <bool FULL>
__global__ void __launch_bounds__(kMbarThreads) mbar_col_kernel(MbarArgs a) {
#pragma clang fp contract(off)
    __shared__ double sl[kMbarTile], sd[kMbarTile];
    const int b = blockIdx.z;
    const unsigned int tile = blockIdx.x;
    const int cnt = mbar_load_tile(a, b, tile, sl, sd);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int t_end = (int)(blockIdx.y + 1) * kMbarGroup < a.n_t ? (int)(blockIdx.y + 1) * kMbarGroup : a.n_t;
    const double l_first = FULL ? a.ell[mbar_at(a, b, 0)] : 0.0;
    for (int t = (int)blockIdx.y * kMbarGroup + wave; t < t_end; t += kMbarThreads / 64) {
        const size_t bt_at = (size_t)b * a.n_t + t;
        const double bt = a.beta_t[(size_t)b * a.t_stride + t];
        const double mt = mbar_unkey(a.mkey[bt_at]);
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, ss = 0.0;
#pragma unroll 4
        for (int i = lane; i < cnt; i += 64) {
            const double l = sl[i];
            const double prod = bt * l;
            const double x = prod - sd[i];
            const double e = exp(x - mt);
            s0 += e;
            if (FULL) {
                const double d = l - l_first;
                const double ed = e * d;
                const double edd = ed * d;
                const double ee = e * e;
                s1 += ed;
                s2 += edd;
                ss += ee;
            }
        }
        s0 = wave_allreduce_sum(s0);
        if (FULL) {
            s1 = wave_allreduce_sum(s1);
            s2 = wave_allreduce_sum(s2);
            ss = wave_allreduce_sum(ss);
        }
        if (lane == 0) {
            double *p = a.part + bt_at * a.tiles + tile;
            p[0] = s0;
            if (FULL) {
                p[a.part_stride] = s1;
                p[2 * a.part_stride] = s2;
                p[3 * a.part_stride] = ss;
            }
        }
    }
}

// grid ceil(n_ladders * n_t / 64).  full = 0, an iteration (n_t = t_stride = K, or one shared target): g[idx] = m +
// log(S0) and, where c is given, c[idx] = lnT - g[idx].  full = 1: out [6][n_ladders * n_t] = m, S0, S1, S2, SS and
// G = m + log(S0), which at a sampled beta is the next iteration's g on the bits.
__global__ void __launch_bounds__(64) mbar_finish_kernel(MbarArgs a, int n_ladders, int full, double lnT, double *g,
                                                         double *c, double *out) {
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * 64 + threadIdx.x, count = (size_t)n_ladders * a.n_t;
    if (idx >= count)
        return;
    const double m = mbar_unkey(a.mkey[idx]);
    auto total = [&](int w) {
        const double *p = a.part + (size_t)w * a.part_stride + idx * a.tiles;
        double s = 0.0;
#pragma unroll 8
        for (unsigned int k = 0; k < a.tiles; k++)
            s += p[k];
        return s;
    };
    const double S0 = total(0);
    if (!full) {
        const double gt = m + log(S0);
        g[idx] = gt;
        if (c)
            c[idx] = lnT - gt;
    } else {
        out[idx] = m;
        out[count + idx] = S0;
        out[2 * count + idx] = total(1);
        out[3 * count + idx] = total(2);
        out[4 * count + idx] = total(3);
        out[5 * count + idx] = m + log(S0);
    }
}

// grid (ceil(N / 256), n_ladders): w[t_count][n_chains] of the range, G [n_ladders], one target beta_t[0]
__global__ void __launch_bounds__(kMbarThreads) mbar_weights_kernel(MbarArgs a, const double *G, double *w) {
#pragma clang fp contract(off)
    const unsigned int n = blockIdx.x * kMbarThreads + threadIdx.x;
    const int b = blockIdx.y;
    if (n >= a.N)
        return;
    const size_t at = mbar_at(a, b, n);
    const double prod = a.beta_t[0] * a.ell[at];
    const double x = prod - a.lnD[at];
    w[at - (size_t)a.t0 * a.n_chains] = x - G[b];
}

} // namespace apemost
