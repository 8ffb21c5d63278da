// pt_periodogram.h -- on-device residual periodogram: for every kept sample of kept chains the power of the residuals
// y_i - m(x_i; theta_t) on a grid of frequencies, folded from the sample rows [n_steps][n_chains][n_par+2] while they are
// still on the device.  It answers what the SERIAL statistic of pt_check.h only hints at: at which frequency a periodic
// signal is left in the residuals, how strong it is, and with what posterior probability.  For the sine models only: the
// pulse models' data already are a power spectrum and a user model has no residual law here.
//
// The rule.  Contraction is off and every line is one rounding unless it says otherwise.
//   datum, residual   (x_i, y_i) are columns 0 and 1 of the kept chain's own ladder's data as they are at begin, i < L, L
//                     that ladder's length.  r_i = y_i - curve<MODEL>(par, n_par, x_i, k), pt_predict.h's curve unchanged:
//                     the bits of pt_check.h's r.
//   trig              for frequency nu_j of the caller's grid (any doubles, in any order):
//                       u = nu_j * x_i;   s_ij = sin_cw(kTwoPi * u, u, k);
//                       uc = u + 0.25;    c_ij = sin_cw(kTwoPi * uc, uc, k);
//                     both NaN when !(kTwoPi * (fabs(nu_j) * fabs(x_i) + 0.25) < 2^45): predict_sine_in_range with
//                     ph = 0.25.  periodogram_trig is the one device function every kernel takes them from, so a cached
//                     value and a recomputed one have the same bits.
//   sums              C_j and S_j start at +0.0; for i = 0 .. L-1 ascending C_j = fma(r_i, c_ij, C_j) and
//                     S_j = fma(r_i, s_ij, S_j), true fused multiply-adds (v_fma_f64; fma() on the host), strictly
//                     sequential in i: no tree.  (periodogram_sums)
//   power             with the weights w = (wcc, wcs, wss) of the kept chain and frequency, given at begin:
//                       P_j = ((wcc * C) * C + (wcs * C) * S) + (wss * S) * S
//                     five products and two additions, each rounded, in that association (periodogram_power).  The
//                     normalisation is host policy (apemost_amd/periodogram.py, weights); the device sees a quadratic form.
//   no filter         non-finite values go where IEEE arithmetic takes them and touch their own kept chain's words only.
//
// Per series s = (kept chain k, frequency j), s = k * n_freq + j, in kept-sample order, each word one thread's chain of
// operations carried in device memory between calls: equal to a sequential host loop whatever the call and piece
// boundaries are.
//   origin[s]            P of the first sample ever accumulated (0 before there is one);
//   sum[s], sq[s]        check_moment_step of P (pt_check.h): d = P - origin; sum += d; sq += d * d;
//   pmin[s], pmax[s]     from +inf and -inf by strict < and >: a NaN is skipped; both 0 before there is a sample;
//   sum_c[s], sum_s[s]   sum_c += C; sum_s += S: the coherent amplitude.  The periodogram of the mean residual follows on
//                        the host by linearity;
//   exceed[s] (u64)      #{t : P > level[k]}, one level per kept chain given at begin; +inf counts nothing and a NaN P is
//                        not counted.
// Per kept sample the highest peak: m = -inf, arg = n_freq; for j ascending: if (P_j > m) { m = P_j; arg = j; }.  The
// first occurrence wins and a NaN never does (periodogram_peak).  Per kept chain over the samples in order: peak_origin,
// peak_sum, peak_sq (the moments of m), peak_min, peak_max as above, and peak_counts[k][n_freq + 1] (u64):
// peak_counts[arg]++, the last slot for a sample without a P above -inf.
//
// Five launches per piece of at most kPeriodogramPiece kept steps, on the folds' stream (the host takes fewer steps
// per piece where n_keep * max(n_data, n_freq) is large, so that the scratch stays bounded):
//   periodogram_resid_kernel<MODEL>  check_fold_kernel's shape without erfc: one wave per 64 data of a kept chain and 32
//                                    kept samples, the sample's row in scalar registers; writes r [n_keep][piece][n_data].
//   periodogram_sum_kernel           the hot kernel: a dense [samples x data] . [data x 2 freq] product in fp64 with a
//                                    fixed summation order.  A workgroup of kPeriodogramWaves = 4 waves takes one tile of
//                                    64 frequencies, a lane owns a frequency.  The tile's trig is computed
//                                    kPeriodogramChunk = 32 data at a time into LDS (16 KiB of c, 16 KiB of s; each of
//                                    the 256 threads evaluates 8 pairs), and every wave then walks the chunk in ascending
//                                    i for its own kPeriodogramSide = 8 kept samples: c and s from LDS (consecutive lanes,
//                                    consecutive words: no bank conflict), the 8 r_{t,i} wave-uniform from the r scratch
//                                    through scalar loads, 16 independent FMA chains per lane in registers.  The pair costs
//                                    about 40 fp64 operations and is used for 4 x 8 x 2 = 64 FMAs.  It writes C, S and
//                                    P into the scratch [n_keep][piece][n_freq] each.
//   periodogram_fold_kernel          a lane owns a series (k, j), reads the scratch coalesced over j and walks the piece's
//                                    samples in order.
//   periodogram_peak_kernel          one wave per (k, t): see periodogram_wave_peak for the order and its proof.
//   periodogram_peak_fold_kernel     check_stat_fold_kernel's shape: one wave per kept chain, 64 samples at a time, the
//                                    additions and comparisons made in sample order from the lanes' values; the counts
//                                    are 64-bit integer additions.
// periodogram_values_kernel<MODEL> with periodogram_trig_kernel, periodogram_values_sum_kernel and
// periodogram_values_peak_kernel is the stated meaning, as check_values_kernel is for its fold: r, the table c, s, then C,
// S, P from the table (a cached value), peak and arg, by the same device functions.
// No float atomics, plain vector stores, no scratch memory, contraction off.
//
// What was tried for the hot kernel.  Only the form above has been built and measured (tools/periodogram_rate.py,
// profiles/periodogram_rates.txt); the table built once at begin was set aside before measuring, because at the shapes
// the fold is meant for (1024 data x 4096 frequencies x 2 doubles = 64 MiB per kept chain) it turns a compute-bound
// product into one that streams 16 bytes per (i, j) and sample group from HBM or L2.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_check.h"
#include "pt_device.h"
#include "pt_predict.h"

namespace apemost {

constexpr int kPeriodogramWave = 64;
constexpr int kPeriodogramPiece = 512;  // kept steps of one launch at most
constexpr int kPeriodogramSide = 8;     // kept samples a wave of the hot kernel holds side by side
constexpr int kPeriodogramWaves = 4;    // waves of the hot kernel's workgroup: 32 samples share a trig chunk
constexpr int kPeriodogramChunk = 32;   // data per trig chunk in LDS
constexpr int kPeriodogramGroup = 32;   // kept samples per wave of the residual kernel
constexpr int kPeriodogramMaxFreq = 1 << 20;
constexpr bool periodogram_has_residual(int model) { return model == APEMOST_MODEL_SIMPLESIN || model == APEMOST_MODEL_SINE3; }

// REGISTERS (hipcc -O3 --offload-arch=gfx950 -Rpass-analysis=kernel-resource-usage on apemost_hip.hip; no kernel has
// scratch or spills; LDS is the hot kernel's 32 KiB alone)
//   kernel                          VGPRs (simplesin / sine3)   SGPRs
//   periodogram_resid_kernel        46 / 60                     32
//   periodogram_sum_kernel          86                          106 (the residuals of 8 samples x 4 data, 64 of them)
//   periodogram_fold_kernel         82 (16 samples' loads)      35
//   periodogram_peak_kernel         12                          20
//   periodogram_peak_fold_kernel    20                          48
//   periodogram_values_kernel       39 / 52                     20
//   periodogram_trig_kernel         39                          20
//   periodogram_values_sum_kernel   14                          26
//   periodogram_values_peak_kernel  12                          21

// ---- the rule, for the host compiler and the device alike ----
// C and S of one frequency from r[0 .. L), c[0 .. L) and s[0 .. L)
__host__ __device__ inline void periodogram_sums(const double *r, const double *c, const double *s, int L, double &C, double &S) {
    C = 0.0;
    S = 0.0;
    for (int i = 0; i < L; i++) {
        C = __builtin_fma(r[i], c[i], C);
        S = __builtin_fma(r[i], s[i], S);
    }
}

__host__ __device__ inline double periodogram_power(double wcc, double wcs, double wss, double C, double S) {
#pragma clang fp contract(off)
    const double a = wcc * C;
    const double aa = a * C;
    const double b = wcs * C;
    const double bb = b * S;
    const double d = wss * S;
    const double dd = d * S;
    const double ab = aa + bb;
    return ab + dd;
}

// the highest peak of P[0 .. n_freq): the first occurrence wins, a NaN never does
__host__ __device__ inline void periodogram_peak(const double *P, int n_freq, double &m, int &arg) {
    m = -INFINITY;
    arg = n_freq;
    for (int j = 0; j < n_freq; j++)
        if (P[j] > m) {
            m = P[j];
            arg = j;
        }
}

// one sample into the extremes of a series
__host__ __device__ inline void periodogram_extremes_step(double v, double &mn, double &mx) {
    mn = v < mn ? v : mn;
    mx = v > mx ? v : mx;
}

// ---- a datum under a frequency, a datum under a parameter row ----
__device__ __forceinline__ void periodogram_trig(double nu, double x, const SinConsts &k, double &c, double &s) {
#pragma clang fp contract(off)
    const double u = nu * x;
    const double sv = sin_cw(kTwoPi * u, u, k);
    const double uc = u + 0.25;
    const double cv = sin_cw(kTwoPi * uc, uc, k);
    const bool in_range = predict_sine_in_range(nu, 0.25, x);
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    c = in_range ? cv : nan;
    s = in_range ? sv : nan;
}

template <int MODEL>
__device__ __forceinline__ double periodogram_resid(const double *par, int np, double x, double y, const SinConsts &k) {
#pragma clang fp contract(off)
    const double v = curve<MODEL>(par, np, x, k);
    return y - v;
}

struct PeriodogramArgs {
    const double *rows;               // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, n_keep;
    const int *chains;                // [n_keep]
    unsigned long long skip, thin;    // kept steps of this piece: skip, skip + thin, ... (n of them)
    unsigned int n;                   // kept steps of this piece, 1 .. piece
    unsigned int piece;               // kept steps the scratch arrays have room for, <= kPeriodogramPiece
    unsigned long long n0;            // kept samples before this piece
    int n_data, n_blocks;             // n_blocks = ceil(n_data / 64)
    const double *x, *y;              // [n_keep][n_data]: every kept chain's data
    const int *len;                   // [n_keep]: the data kept chain k really has, <= n_data; nullptr: n_data
    int n_freq, n_tiles;              // n_tiles = ceil(n_freq / 64)
    const double *freqs;              // [n_freq]
    const double *weights;            // [n_keep][n_freq][3]
    const double *level;              // [n_keep]
    double *r;                        // [n_keep][piece][n_data]: the residuals of the piece's kept samples
    double *C, *S, *P;                // [n_keep][piece][n_freq] each
    double *origin, *sum, *sq, *pmin, *pmax, *sum_c, *sum_s; // [n_keep][n_freq]
    unsigned long long *exceed;       // [n_keep][n_freq]
    double *pk_m;                     // [n_keep][piece]: the highest peak of the piece's kept samples
    int *pk_arg;                      // [n_keep][piece]: and where it is
    double *peak_origin, *peak_sum, *peak_sq, *peak_min, *peak_max; // [n_keep]
    unsigned long long *peak_counts;  // [n_keep][n_freq + 1]
};

// grid (n_blocks * n_keep, ceil(n / kPeriodogramGroup)), one wave each
template <int MODEL>
__global__ void __launch_bounds__(kPeriodogramWave) periodogram_resid_kernel(PeriodogramArgs a) {
    const int lane = threadIdx.x;
    const int k = blockIdx.x / a.n_blocks, blk = blockIdx.x - k * a.n_blocks;
    const int np = a.n_par, n = (int)a.n;
    const size_t w = (size_t)np + 2, stride = (size_t)a.thin * a.n_chains * w;
    const double *src = a.rows + a.skip * a.n_chains * w + (size_t)a.chains[k] * w;
    const int i = blk * kPeriodogramWave + lane;
    if (i >= (a.len ? a.len[k] : a.n_data))
        return;
    SinConsts sc;
    sc.init();
    const size_t at = (size_t)k * a.n_data + i;
    const double x = a.x[at], y = a.y[at];
    const int t0 = (int)blockIdx.y * kPeriodogramGroup;
    const int t1 = t0 + kPeriodogramGroup < n ? t0 + kPeriodogramGroup : n;
    double *out = a.r + (size_t)k * a.piece * a.n_data + i;
    for (int t = t0; t < t1; t++) // (the row's address is the same in every lane: scalar loads)
        out[(size_t)t * a.n_data] = periodogram_resid<MODEL>(src + (size_t)t * stride, np, x, y, sc);
}

typedef const double __attribute__((address_space(4))) *PeriodogramUniform;

// grid (n_tiles, ceil(n / (kPeriodogramWaves * kPeriodogramSide)), n_keep), kPeriodogramWaves waves each
__global__ void __launch_bounds__(kPeriodogramWaves *kPeriodogramWave) periodogram_sum_kernel(PeriodogramArgs a) {
    constexpr int T = kPeriodogramSide, W = kPeriodogramWaves, CH = kPeriodogramChunk;
    __shared__ double lc[CH][kPeriodogramWave], ls[CH][kPeriodogramWave];
    const int lane = threadIdx.x & (kPeriodogramWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kPeriodogramWave));
    const int k = blockIdx.z;
    const int j = (int)blockIdx.x * kPeriodogramWave + lane;
    const bool live = j < a.n_freq;
    const int n = (int)a.n, nd = a.n_data;
    const int L = a.len ? a.len[k] : nd;
    const double nu = a.freqs[live ? j : 0]; // (a lane past the grid works on frequency 0 and stores nothing)
    const double *x = a.x + (size_t)k * nd;
    const int t0 = ((int)blockIdx.y * W + wave) * T;
    // The residuals are the same for every lane.  Read through the constant address space, which this kernel never
    // writes (the residual kernel's launch has ended), they come through scalar loads into scalar registers; as plain
    // global loads behind the barrier they were vector loads of one address, 16 per 64 FMAs.  This is right only because
    // the scratch is written by an EARLIER LAUNCH on the same stream: the acquire at the start of this dispatch
    // invalidates the scalar cache, so no line of the piece before is read.  A kernel that wrote and read r in one
    // launch, or the two kernels on different streams, would read stale lines through this path.
    // (a sample past the piece reads the piece's last and stores nothing)
    PeriodogramUniform r[T];
#pragma unroll
    for (int q = 0; q < T; q++)
        r[q] = (PeriodogramUniform)(unsigned long long)(a.r + ((size_t)k * a.piece + (size_t)(t0 + q < n ? t0 + q : n - 1)) * nd);
    SinConsts sc;
    sc.init();
    double C[T], S[T];
#pragma unroll
    for (int q = 0; q < T; q++)
        C[q] = S[q] = 0.0;
    for (int i0 = 0; i0 < L; i0 += CH) {
        const int cnt = L - i0 < CH ? L - i0 : CH;
        __syncthreads(); // the chunk before has been read
        for (int ii = wave; ii < cnt; ii += W) {
            double c, s;
            periodogram_trig(nu, x[i0 + ii], sc, c, s);
            lc[ii][lane] = c;
            ls[ii][lane] = s;
        }
        __syncthreads();
#pragma unroll 4
        for (int ii = 0; ii < cnt; ii++) {
            const double c = lc[ii][lane], s = ls[ii][lane];
#pragma unroll
            for (int q = 0; q < T; q++) {
                const double rv = r[q][i0 + ii];
                C[q] = __builtin_fma(rv, c, C[q]);
                S[q] = __builtin_fma(rv, s, S[q]);
            }
        }
    }
    if (!live)
        return;
    const double *wt = a.weights + ((size_t)k * a.n_freq + j) * 3;
    const double wcc = wt[0], wcs = wt[1], wss = wt[2];
#pragma unroll
    for (int q = 0; q < T; q++)
        if (t0 + q < n) {
            const size_t at = ((size_t)k * a.piece + (size_t)(t0 + q)) * a.n_freq + j;
            a.C[at] = C[q];
            a.S[at] = S[q];
            a.P[at] = periodogram_power(wcc, wcs, wss, C[q], S[q]);
        }
}

// grid (n_tiles, n_keep), one wave each: a lane owns the series (k, j)
__global__ void __launch_bounds__(kPeriodogramWave) periodogram_fold_kernel(PeriodogramArgs a) {
#pragma clang fp contract(off)
    const int k = blockIdx.y, j = (int)blockIdx.x * kPeriodogramWave + (int)threadIdx.x;
    if (j >= a.n_freq)
        return;
    const size_t s = (size_t)k * a.n_freq + j, base = (size_t)k * a.piece * a.n_freq + j;
    const double *P = a.P + base, *C = a.C + base, *S = a.S + base;
    const bool first = a.n0 == 0;
    const double level = a.level[k];
    double origin, mn, mx, sum = a.sum[s], sq = a.sq[s], sum_c = a.sum_c[s], sum_s = a.sum_s[s];
    unsigned long long exceed = a.exceed[s];
    if (first) {
        origin = P[0];
        mn = INFINITY;
        mx = -INFINITY;
    } else {
        origin = a.origin[s];
        mn = a.pmin[s];
        mx = a.pmax[s];
    }
    const int n = (int)a.n;
    auto step = [&](double p, double c, double s_) {
        check_moment_step(p, origin, sum, sq);
        periodogram_extremes_step(p, mn, mx);
        sum_c += c;
        sum_s += s_;
        exceed += p > level ? 1ull : 0ull;
    };
    // kFoldAhead samples' loads are issued together and folded in order: a series' chain of additions is short, and
    // taken one sample at a time the loop waits for the memory's latency once per sample (the whole fold of chain 0
    // over 1024 data: 1.13 against 1.37 million kept samples/s at 1024 frequencies, 0.91 against 1.09 at 4096)
    constexpr int kFoldAhead = 16;
    int t = 0;
    for (; t + kFoldAhead <= n; t += kFoldAhead) {
        double p[kFoldAhead], c[kFoldAhead], s_[kFoldAhead];
#pragma unroll
        for (int q = 0; q < kFoldAhead; q++) {
            const size_t at = (size_t)(t + q) * a.n_freq;
            p[q] = P[at];
            c[q] = C[at];
            s_[q] = S[at];
        }
#pragma unroll
        for (int q = 0; q < kFoldAhead; q++)
            step(p[q], c[q], s_[q]);
    }
    for (; t < n; t++) {
        const size_t at = (size_t)t * a.n_freq;
        step(P[at], C[at], S[at]);
    }
    if (first)
        a.origin[s] = origin;
    a.sum[s] = sum;
    a.sq[s] = sq;
    a.pmin[s] = mn;
    a.pmax[s] = mx;
    a.sum_c[s] = sum_c;
    a.sum_s[s] = sum_s;
    a.exceed[s] = exceed;
}

// The highest peak of P[0 .. n_freq) by the whole wave, the same in every lane.  Lane l walks j = l, l + 64, ... in
// ascending order with the rule's own step, so it ends with (m_l, arg_l) = periodogram_peak of its own subsequence: the
// largest P above -inf among its j and the smallest of its j that holds it, or (-inf, n_freq).  The lanes are then joined
// by `b beats a when m_b > m_a, or m_b == m_a and arg_b < arg_a`: the lexicographic maximum over (m, -arg), a total
// order on the pairs (no m is NaN: a NaN never passed the strict >), so the join is associative and commutative and the
// butterfly below gives every lane the maximum over all 64 pairs.  That maximum is the rule's answer: if no P is above
// -inf every pair is (-inf, n_freq), the rule's.  Otherwise let M be the largest P and j* the smallest j with P_j = M,
// the rule's answer by its strict >.  The lane that owns j* has m = M and arg = j* (j* is also the first such j of its
// own subsequence), every other lane has m < M, or m = M with an arg of its own above j*: the pair (M, j*) wins.
__device__ __forceinline__ void periodogram_wave_peak(const double *P, int n_freq, double &m, int &arg) {
    const int lane = threadIdx.x & (kPeriodogramWave - 1);
    m = -INFINITY;
    arg = n_freq;
    for (int j = lane; j < n_freq; j += kPeriodogramWave) {
        const double p = P[j];
        if (p > m) {
            m = p;
            arg = j;
        }
    }
#pragma unroll
    for (int step = 1; step < kPeriodogramWave; step <<= 1) {
        const double om = __shfl_xor(m, step, kPeriodogramWave);
        const int oa = __shfl_xor(arg, step, kPeriodogramWave);
        const bool beats = om > m || (om == m && oa < arg);
        m = beats ? om : m;
        arg = beats ? oa : arg;
    }
}

// grid (n, n_keep), one wave each
__global__ void __launch_bounds__(kPeriodogramWave) periodogram_peak_kernel(PeriodogramArgs a) {
    const int t = blockIdx.x, k = blockIdx.y;
    double m;
    int arg;
    periodogram_wave_peak(a.P + ((size_t)k * a.piece + t) * a.n_freq, a.n_freq, m, arg);
    if (threadIdx.x == 0) {
        a.pk_m[(size_t)k * a.piece + t] = m;
        a.pk_arg[(size_t)k * a.piece + t] = arg;
    }
}

// grid n_keep, one wave each: folds pk_m[k][0 .. n) and pk_arg[k][0 .. n) in sample order; n0 == 0: the first sample ever
__global__ void __launch_bounds__(kPeriodogramWave) periodogram_peak_fold_kernel(PeriodogramArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, k = blockIdx.x;
    const double *M = a.pk_m + (size_t)k * a.piece;
    const int *A = a.pk_arg + (size_t)k * a.piece;
    unsigned long long *counts = a.peak_counts + (size_t)k * ((size_t)a.n_freq + 1);
    const unsigned int n = a.n;
    const bool first = a.n0 == 0;
    double origin, mn, mx, sum = a.peak_sum[k], sq = a.peak_sq[k];
    if (first) {
        origin = M[0];
        mn = INFINITY;
        mx = -INFINITY;
    } else {
        origin = a.peak_origin[k];
        mn = a.peak_min[k];
        mx = a.peak_max[k];
    }
    for (unsigned int t0 = 0; t0 < n; t0 += kPeriodogramWave) {
        const int cnt = n - t0 < (unsigned int)kPeriodogramWave ? (int)(n - t0) : kPeriodogramWave;
        const double v = lane < cnt ? M[t0 + lane] : 0.0;
        const double d = v - origin;
        const double dd = d * d;
        if (lane < cnt) {
            const int arg = A[t0 + lane];
            if (arg >= 0 && arg <= a.n_freq)
                atomicAdd(counts + arg, 1ull); // (an integer: exact in any order)
        }
        for (int r = 0; r < cnt; r++) {
            sum += read_lane(d, r);
            sq += read_lane(dd, r);
            periodogram_extremes_step(read_lane(v, r), mn, mx);
        }
    }
    if (lane == 0) {
        if (first)
            a.peak_origin[k] = origin;
        a.peak_sum[k] = sum;
        a.peak_sq[k] = sq;
        a.peak_min[k] = mn;
        a.peak_max[k] = mx;
    }
}

// ---- the stated meaning ----
// grid (ceil(n_x / 64), n), one wave each: r[row][i] of the parameter row over the n_x data x, y
template <int MODEL>
__global__ void __launch_bounds__(kPeriodogramWave) periodogram_values_kernel(const double *params, int n_par, int n_x,
                                                                            const double *x, const double *y, double *r) {
    const int i = (int)blockIdx.x * kPeriodogramWave + (int)threadIdx.x, row = blockIdx.y;
    if (i >= n_x)
        return;
    SinConsts sc;
    sc.init();
    r[(size_t)row * n_x + i] = periodogram_resid<MODEL>(params + (size_t)row * n_par, n_par, x[i], y[i], sc);
}

// grid (ceil(n_x / 64), n_freq), one wave each: the table c[j][i], s[j][i]
__global__ void __launch_bounds__(kPeriodogramWave) periodogram_trig_kernel(int n_freq, const double *freqs, int n_x,
                                                                          const double *x, double *c, double *s) {
    const int i = (int)blockIdx.x * kPeriodogramWave + (int)threadIdx.x, j = blockIdx.y;
    if (i >= n_x || j >= n_freq)
        return;
    SinConsts sc;
    sc.init();
    double cv, sv;
    periodogram_trig(freqs[j], x[i], sc, cv, sv);
    c[(size_t)j * n_x + i] = cv;
    s[(size_t)j * n_x + i] = sv;
}

// grid (ceil(n_freq / 64), n), one wave each: C, S, P [row][j] from r [n][n_x] and the table, w [n_freq][3]
__global__ void __launch_bounds__(kPeriodogramWave) periodogram_values_sum_kernel(int n_x, int n_freq, const double *r,
                                                                                const double *c, const double *s,
                                                                                const double *w, double *C, double *S,
                                                                                double *P) {
    const int j = (int)blockIdx.x * kPeriodogramWave + (int)threadIdx.x, row = blockIdx.y;
    if (j >= n_freq)
        return;
    double Cv, Sv;
    periodogram_sums(r + (size_t)row * n_x, c + (size_t)j * n_x, s + (size_t)j * n_x, n_x, Cv, Sv);
    const size_t at = (size_t)row * n_freq + j;
    C[at] = Cv;
    S[at] = Sv;
    P[at] = periodogram_power(w[3 * (size_t)j], w[3 * (size_t)j + 1], w[3 * (size_t)j + 2], Cv, Sv);
}

// grid n, one wave each
__global__ void __launch_bounds__(kPeriodogramWave) periodogram_values_peak_kernel(int n_freq, const double *P, double *peak,
                                                                                 int *arg) {
    const int row = blockIdx.x;
    double m;
    int at;
    periodogram_wave_peak(P + (size_t)row * n_freq, n_freq, m, at);
    if (threadIdx.x == 0) {
        peak[row] = m;
        arg[row] = at;
    }
}
} // namespace apemost
