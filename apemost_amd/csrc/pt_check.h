// pt_check.h -- on-device predictive checks: per datum the predictive CDF at the observed value under every kept sample
// of kept chains (the PIT and its leave-one-out form), and per kept sample three discrepancy statistics over the kept
// chain's data, folded from the sample rows [n_steps][n_chains][n_par+2] while they are still on the device.  No sample
// dump holds these quantities: a row carries only the sum over the data.  It answers what the pointwise fold does not:
// is the model adequate for these data, or is there still a signal in the residuals?
//
// The quantities.  The datum is (x_i, y_i), columns 0 and 1 of the sampler's data as they are at begin (of the kept
// chain's own ladder in a batch).  v = curve<MODEL>(par, n_par, x_i, sc) is pt_predict.h's model curve, unchanged, and
// l = pointwise_term<MODEL>(v, y_i, c) is pt_pointwise.h's term, unchanged: it has the pointwise fold's bits.
// Contraction is off and every line is one rounding:
//   simplesin, sine3    r = y_i - v;  e = r * inv_sigma, the standardised residual, with inv_sigma = 1.0 / sigma computed
//                       once on the host;  t = e * (-M_SQRT1_2);  u = 0.5 * erfc(t), the device library's fp64 erfc;
//   pulse, pulse_vrot   e = y_i / v, a true fp64 division: the ratio, Exp(1) under the model;  t = -e;
//                       u = -expm1(t), the device library's fp64 expm1;
//   both                a = u - 0.5.
// u is the predictive CDF at y_i.  There is no filter: a non-finite or non-positive v gives whatever IEEE arithmetic
// gives and touches the words of its own kept chain only.  APEMOST_MODEL_USER has no CDF and is refused at begin.
//
// Per-datum state.  A series is s = (kept chain k, datum i), s = k * n_data + i.  It has seven words, each one thread's
// chain of operations in kept-sample order, carried in device memory between calls: equal to a sequential host loop
// whatever the call and piece boundaries are.
//   origin[s]            e of the first sample ever accumulated (0 before there is one);
//   sum[s], sq[s]        with d = e - origin: sum += d; sq += d * d (the product rounded, then added); the first sample
//                        takes part like every other (its d is e - e);
//   sum_u[s]             sum_u += u.  pit_i = sum_u / n on the host;
//   m[s], S[s], SU[s]    the leave-one-out weighted CDF with x = -l: the first sample sets m = x, S = 1, SU = u; later
//                          if (x > m) { t = exp(m - x); S = S * t + 1; SU = SU * t + u; m = x; }
//                          else       { w = exp(x - m); S += w; uw = u * w; SU += uw; }
//                        (every product rounded before its addition: check_lse_u_step).  m and S are the pointwise
//                        fold's m_dn and S_dn on the same rows, operation for operation.  loo_pit_i = SU / S on the host.
//
// Per kept sample, three statistics over the kept chain's L data.  Every sum follows the rule of pt_pointwise_joint.h:
// 64 lane partials by i % 64 in ascending i, then the adjacent-pairs tree (joint_lane_partials, joint_tree_sum).
//   FIT      sine models sum of e * e (null chi^2 with L degrees of freedom); pulse models sum of e (null Gamma(L, 1));
//   EXTREME  sine models max_i |e_i|, pulse models max_i e_i: m from -inf with t > m ? t : m, so that a NaN term is
//            skipped; T = m + 0.0.  The maximum of values that are not NaN does not depend on the order they are taken
//            in but for the sign of a zero, which the last addition removes: the kernels take it lane by lane and then
//            across the lanes;
//   SERIAL   the terms g_0 = +0.0 and g_i = a_i * a_{i-1} for i >= 1 in data order, summed by the rule.  Under the model
//            the u_i are independent and uniform: mean 0, variance (L - 1) / 144.  This is the statistic that sees an
//            unmodelled periodic signal.
// check_fit_term, check_extreme_term, check_serial_terms, check_sum and check_extreme below state them for the host
// compiler (tests/check_rule.cpp); tests/check_ref.py restates them in numpy.
//
// Per kept chain and statistic, over the samples in sample order: origin, sum, sq as above (of T); min and max, with
// t < m ? t : m from +inf and t > m ? t : m from -inf (a NaN is skipped; both 0 before there is a sample); and, with
// n_edges > 0 ascending edges per statistic given at begin, exact counts [n_edges + 2]: slot b = #{j : edges[j] <= T}
// by binary search (check_slot), the last slot counts NaN.
//
// Three launches per piece of at most kPointwisePiece kept steps, on the folds' stream:
//   check_fold_kernel<MODEL>   pointwise_fold_kernel's shape: one wave per 64 data of a kept chain, x, y and the seven
//                              words in registers over the piece.  Pulse models: the kept parameter rows staged through
//                              an LDS tile of kPointwiseTile doubles, check_side(MODEL) = 4 samples side by side where no
//                              maximum moves and one by one where one does; both ways are the recurrence above,
//                              operation for operation.  Sine models: erfc holds most of the register budget by itself,
//                              so the samples are taken one by one, and a sample's row, whose address is the same in
//                              every lane, is read from the rows themselves into scalar registers; no tile.
//   check_stat_kernel<MODEL>   pointwise_joint_sum_kernel's shape: grid (n_keep, ceil(n / rows)), one wave each,
//                              rows = check_rows(MODEL, n_par) kept samples side by side.  The wave walks its kept chain's data
//                              64 at a time in ascending order, so that a lane's partial is the rule's.  For SERIAL lane
//                              j takes a_{i-1} from lane j - 1 by a shuffle; lane 0 takes the chunk before's lane-63
//                              value, carried through a lane read; the first datum has no predecessor.  It writes T
//                              into the scratch [n_keep][3][kPointwisePiece].
//   check_stat_fold_kernel     grid (n_keep, 3), one wave per kept chain and statistic, 64 samples at a time, one per
//                              lane: d, d * d and the slot are a lane's own; the additions into sum and sq and the
//                              comparisons of min and max are then made in sample order from the lanes' values
//                              (v_readlane), the same in every lane.  The counts are 64-bit integer additions.
// check_values_kernel<MODEL> is the stated meaning, as pointwise_loglike_kernel is for its fold: for n parameter rows and
// n_x data of the caller it gives e, u and the three T, by the same device functions.
// No float atomics, plain vector loads and stores, no scratch memory, contraction off.  Registers (hipcc -O3, gfx950,
// -Rpass-analysis=kernel-resource-usage; the budget is the pointwise fold's, 128 VGPRs): see REGISTERS below.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_pointwise.h"
#include "pt_pointwise_joint.h"

namespace apemost {

constexpr int kCheckStats = 3; // FIT, EXTREME, SERIAL (APEMOST_CHECK_FIT .. in include/apemost_hip.h)
constexpr int kCheckFit = 0, kCheckExtreme = 1, kCheckSerial = 2;
constexpr bool check_is_sine(int model) { return model == APEMOST_MODEL_SIMPLESIN || model == APEMOST_MODEL_SINE3; }
// samples evaluated side by side, in the fold and in the statistics: the sine models' erfc holds most of the register
// budget by itself
constexpr int check_side(int model) { return check_is_sine(model) ? 1 : 4; }
constexpr int kCheckMaxEdges = 4095;

// REGISTERS (VGPRs; no kernel has scratch; LDS is the 4 KiB tile of the fold and of the statistics' kernel, which the
// sine models leave unused).  Four side by side put the sine models at 149 to 175, two at 133 to 152, and the
// compiler's occupancy hint for four waves per SIMD spills: hence one by one there.
//   kernel                   simplesin  sine3  pulse  pulse_vrot
//   check_fold_kernel        126        126    118    124
//   check_stat_kernel        120        128    119    123
//   check_values_kernel      120        124     52     90
//   check_stat_fold_kernel   20 for every model

// ---- the rule, for the host compiler and the device alike ----
// a sample's share of FIT and of EXTREME from its e
__host__ __device__ inline double check_fit_term(double e, bool sine) {
#pragma clang fp contract(off)
    if (sine) {
        const double ee = e * e;
        return ee;
    }
    return e;
}
__host__ __device__ inline double check_extreme_term(double e, bool sine) { return sine ? fabs(e) : e; }

// g[0 .. L): the terms of SERIAL from a[0 .. L)
__host__ __device__ inline void check_serial_terms(const double *a, int L, double *g) {
#pragma clang fp contract(off)
    for (int i = 0; i < L; i++) {
        if (i == 0) {
            g[i] = 0.0;
        } else {
            const double t = a[i] * a[i - 1];
            g[i] = t;
        }
    }
}

// the two-stage sum of pt_pointwise_joint.h over L terms
__host__ __device__ inline double check_sum(const double *terms, int L) {
    double p[kPointwiseWave];
    joint_lane_partials(terms, L, p);
    return joint_tree_sum(p);
}

// EXTREME of L terms
__host__ __device__ inline double check_extreme(const double *terms, int L) {
#pragma clang fp contract(off)
    double m = -INFINITY;
    for (int i = 0; i < L; i++)
        m = terms[i] > m ? terms[i] : m;
    return m + 0.0;
}

// slot of T among n_edges ascending edges: #{j : edges[j] <= T}, n_edges + 1 for a NaN
__host__ __device__ inline int check_slot(double T, const double *edges, int n_edges) {
    if (T != T)
        return n_edges + 1;
    int lo = 0, hi = n_edges;
    while (lo < hi) {
        const int mid = (lo + hi) / 2;
        if (edges[mid] <= T)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo;
}

// one sample into the moments of a series or of a statistic
__host__ __device__ inline void check_moment_step(double v, double origin, double &sum, double &sq) {
#pragma clang fp contract(off)
    const double d = v - origin;
    sum += d;
    const double dd = d * d;
    sq += dd;
}

// one update of the leave-one-out weighted CDF, as the header states it
__host__ __device__ inline void check_lse_u_step(double x, double u, double &m, double &S, double &SU) {
#pragma clang fp contract(off)
    if (x > m) {
        const double t = exp(m - x);
        const double st = S * t;
        S = st + 1.0;
        const double sut = SU * t;
        SU = sut + u;
        m = x;
    } else {
        const double w = exp(x - m);
        S += w;
        const double uw = u * w;
        SU += uw;
    }
}

// ---- a datum under a parameter row ----
template <int MODEL>
__device__ __forceinline__ void check_eu(double v, double y, double inv_sigma, double &e, double &u) {
#pragma clang fp contract(off)
    if (check_is_sine(MODEL)) {
        const double r = y - v;
        e = r * inv_sigma;
        const double t = e * (-M_SQRT1_2);
        u = 0.5 * erfc(t);
    } else {
        e = y / v;
        const double t = -e;
        u = -expm1(t);
    }
}

struct CheckArgs {
    const double *rows;               // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, n_keep;
    const int *chains;                // [n_keep]
    unsigned long long skip, thin;    // kept steps of this piece: skip, skip + thin, ... (n of them)
    unsigned int n;                   // kept steps of this piece, 1 .. kPointwisePiece
    unsigned long long n0;            // kept samples before this piece
    int n_data, n_blocks;             // n_blocks = ceil(n_data / 64)
    const double *x, *y;              // [n_keep][n_data]: every kept chain's data
    double c, inv_sigma;              // 1 / (-2 sigma^2) and 1 / sigma (the sine models)
    double *origin, *sum, *sq, *sum_u, *m, *S, *SU; // [n_keep][n_data]
    const int *len;                   // [n_keep]: the data kept chain k really has, <= n_data; nullptr: n_data
    double *T;                        // [n_keep][3][kPointwisePiece]: the statistics of the piece's kept samples
    double *stat_origin, *stat_sum, *stat_sq, *stat_min, *stat_max; // [n_keep][3]
    const double *edges;              // [3][n_edges], or nullptr
    int n_edges;
    unsigned long long *counts;       // [n_keep][3][n_edges + 2], or nullptr
};

// grid n_blocks * n_keep, one wave each
template <int MODEL>
__global__ void __launch_bounds__(kPointwiseWave) check_fold_kernel(CheckArgs a) {
#pragma clang fp contract(off)
    constexpr int kCheckSide = check_side(MODEL);
    __shared__ double tile[kPointwiseTile];
    const int lane = threadIdx.x;
    const int k = blockIdx.x / a.n_blocks, blk = blockIdx.x - k * a.n_blocks;
    const int np = a.n_par, n = (int)a.n;
    const size_t w = (size_t)np + 2, stride = (size_t)a.thin * a.n_chains * w;
    const double *src = a.rows + a.skip * a.n_chains * w + (size_t)a.chains[k] * w;
    const int i = blk * kPointwiseWave + lane;
    const bool active = i < (a.len ? a.len[k] : a.n_data);
    const size_t s = (size_t)k * a.n_data + (active ? i : 0);
    SinConsts sc;
    sc.init();
    const double x = active ? a.x[s] : 0.0, y = active ? a.y[s] : 0.0;
    const double c = a.c, inv_sigma = a.inv_sigma;
    // l, e and u of this lane's datum under a parameter row (which may lie in LDS)
    auto at = [&](const double *par, double &l, double &e, double &u) {
        const double v = curve<MODEL>(par, np, x, sc);
        l = pointwise_term<MODEL>(v, y, c);
        check_eu<MODEL>(v, y, inv_sigma, e, u);
    };
    const bool first = a.n0 == 0;
    double origin = 0, sum = 0, sq = 0, sum_u = 0, m = 0, S = 0, SU = 0;
    if (active) {
        sum = a.sum[s];
        sq = a.sq[s];
        sum_u = a.sum_u[s];
        if (first) { // the first sample ever: the origin and the maximum; its d = e - e enters the sums below
            double l, u;
            at(src, l, origin, u);
            m = -l;
            S = 1.0;
            SU = u;
            check_moment_step(origin, origin, sum, sq);
            sum_u += u;
        } else {
            origin = a.origin[s];
            m = a.m[s];
            S = a.S[s];
            SU = a.SU[s];
        }
    }
    const int per_tile = kPointwiseTile / np; // >= 1 (n_par <= kPointwiseTile is checked at begin)
    for (int t0 = 0; t0 < n; t0 += per_tile) {
        const int cnt = n - t0 < per_tile ? n - t0 : per_tile;
        if (kCheckSide > 1) {
            __syncthreads(); // the tile before has been read
            for (int q = lane; q < cnt * np; q += kPointwiseWave) {
                const int r = q / np, p = q - r * np;
                tile[q] = src[(size_t)(t0 + r) * stride + p];
            }
            __syncthreads();
        }
        if (active) {
            int r = first && t0 == 0 ? 1 : 0;
            for (; kCheckSide > 1 && r + kCheckSide <= cnt; r += kCheckSide) {
                double e[kCheckSide], u[kCheckSide], xd[kCheckSide];
                bool moves = false;
#pragma unroll
                for (int j = 0; j < kCheckSide; j++) {
                    double l;
                    at(tile + (r + j) * np, l, e[j], u[j]);
                    xd[j] = -l;
                    moves = moves || xd[j] > m;
                }
#pragma unroll
                for (int j = 0; j < kCheckSide; j++) {
                    check_moment_step(e[j], origin, sum, sq);
                    sum_u += u[j];
                }
                if (moves) {
#pragma unroll
                    for (int j = 0; j < kCheckSide; j++)
                        check_lse_u_step(xd[j], u[j], m, S, SU);
                } else {
                    double wt[kCheckSide], uw[kCheckSide];
#pragma unroll
                    for (int j = 0; j < kCheckSide; j++) {
                        wt[j] = exp(xd[j] - m);
                        uw[j] = u[j] * wt[j];
                    }
#pragma unroll
                    for (int j = 0; j < kCheckSide; j++) {
                        S += wt[j];
                        SU += uw[j];
                    }
                }
            }
            for (; r < cnt; r++) {
                double l, e, u;
                // (one sample at a time: the row's address is the same in every lane, and read from the rows themselves it
                // stays in scalar registers, which the sine models' erfc leaves free)
                at(kCheckSide > 1 ? tile + r * np : src + (size_t)(t0 + r) * stride, l, e, u);
                check_moment_step(e, origin, sum, sq);
                sum_u += u;
                check_lse_u_step(-l, u, m, S, SU);
            }
        }
    }
    if (active) {
        if (first)
            a.origin[s] = origin;
        a.sum[s] = sum;
        a.sq[s] = sq;
        a.sum_u[s] = sum_u;
        a.m[s] = m;
        a.S[s] = S;
        a.SU[s] = SU;
    }
}

// kept samples per wave of the statistics' kernel: what fits the LDS tile, at most check_side(model), at least 1
__host__ __device__ inline int check_rows(int model, int n_par) {
    const int fit = kPointwiseTile / n_par, side = check_side(model);
    return fit < 1 ? 1 : fit > side ? side : fit;
}

// the maximum over the 64 lanes, the same in every lane (no lane holds a NaN)
__device__ __forceinline__ double check_wave_max(double v) {
    double o;
    o = dpp_move<0xB1>(v); // quad_perm [1,0,3,2]
    v = o > v ? o : v;
    o = dpp_move<0x4E>(v); // quad_perm [2,3,0,1]
    v = o > v ? o : v;
    o = dpp_move<0x141>(v); // row_half_mirror
    v = o > v ? o : v;
    o = dpp_move<0x140>(v); // row_mirror
    v = o > v ? o : v;
    const double r0 = read_lane(v, 0), r1 = read_lane(v, 16), r2 = read_lane(v, 32), r3 = read_lane(v, 48);
    const double a = r1 > r0 ? r1 : r0, b = r3 > r2 ? r3 : r2;
    return b > a ? b : a;
}

// The three statistics of N parameter rows (par + j * par_stride, which may lie in LDS) over the L data x, y, by the
// whole wave: T[j][0 .. 3) in every lane.  e_out, u_out (N == 1 only; or nullptr): e and u of every datum.
template <int MODEL, int N>
__device__ __forceinline__ void check_wave_stats(const double *par, int par_stride, int np, const double *x, const double *y,
                                                 int L, double inv_sigma, const SinConsts &sc, double (*T)[kCheckStats],
                                                 double *e_out, double *u_out) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x;
    double fit[N], ext[N], ser[N], carry[N];
#pragma unroll
    for (int j = 0; j < N; j++) {
        fit[j] = 0.0;
        ser[j] = 0.0;
        ext[j] = -INFINITY;
        carry[j] = 0.0;
    }
    for (int i0 = 0; i0 < L; i0 += kPointwiseWave) { // (the same in every lane: the shuffle below needs them all)
        const int i = i0 + lane;
        const bool active = i < L;
        const double xi = active ? x[i] : 0.0, yi = active ? y[i] : 0.0;
        double e[N], u[N];
#pragma unroll
        for (int j = 0; j < N; j++)
            check_eu<MODEL>(curve<MODEL>(par + j * par_stride, np, xi, sc), yi, inv_sigma, e[j], u[j]);
#pragma unroll
        for (int j = 0; j < N; j++) {
            const double a = u[j] - 0.5;
            double before = __shfl_up(a, 1, kPointwiseWave);
            if (lane == 0)
                before = carry[j];
            carry[j] = read_lane(a, kPointwiseWave - 1);
            const double prod = a * before;
            const double g = i == 0 ? 0.0 : prod;
            if (active) {
                fit[j] += check_fit_term(e[j], check_is_sine(MODEL));
                ser[j] += g;
                const double t = check_extreme_term(e[j], check_is_sine(MODEL));
                ext[j] = t > ext[j] ? t : ext[j];
            }
        }
        if (N == 1 && e_out && active) {
            e_out[i] = e[0];
            u_out[i] = u[0];
        }
    }
#pragma unroll
    for (int j = 0; j < N; j++) {
        T[j][kCheckFit] = wave_allreduce_sum(fit[j]);
        T[j][kCheckExtreme] = check_wave_max(ext[j]) + 0.0;
        T[j][kCheckSerial] = wave_allreduce_sum(ser[j]);
    }
}

// grid (a.n_keep, ceil(a.n / check_rows(MODEL, a.n_par))), one wave each
template <int MODEL>
__global__ void __launch_bounds__(kPointwiseWave) check_stat_kernel(CheckArgs a) {
    constexpr int kCheckSide = check_side(MODEL);
    __shared__ double tile[kPointwiseTile];
    const int lane = threadIdx.x, k = blockIdx.x;
    const int np = a.n_par, rows = check_rows(MODEL, np);
    const int t0 = (int)blockIdx.y * rows;
    const int cnt = (int)a.n - t0 < rows ? (int)a.n - t0 : rows; // >= 1 by the grid
    const size_t w = (size_t)np + 2, stride = (size_t)a.thin * a.n_chains * w;
    const double *src = a.rows + a.skip * a.n_chains * w + (size_t)a.chains[k] * w + (size_t)t0 * stride;
    if (kCheckSide > 1) {
        for (int q = lane; q < cnt * np; q += kPointwiseWave) {
            const int r = q / np, p = q - r * np;
            tile[q] = src[(size_t)r * stride + p];
        }
        __syncthreads();
    }
    const int L = a.len ? a.len[k] : a.n_data;
    const double *x = a.x + (size_t)k * a.n_data, *y = a.y + (size_t)k * a.n_data;
    SinConsts sc;
    sc.init();
    double *out = a.T + (size_t)k * kCheckStats * kPointwisePiece + t0;
    if (kCheckSide > 1 && cnt == kCheckSide) {
        double T[kCheckSide][kCheckStats];
        check_wave_stats<MODEL, kCheckSide>(tile, np, np, x, y, L, a.inv_sigma, sc, T, nullptr, nullptr);
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < kCheckSide; j++)
#pragma unroll
                for (int q = 0; q < kCheckStats; q++)
                    out[(size_t)q * kPointwisePiece + j] = T[j][q];
        }
    } else {
        for (int r = 0; r < cnt; r++) { // (cnt is the same in every lane)
            double T[1][kCheckStats];
            check_wave_stats<MODEL, 1>(kCheckSide > 1 ? tile + r * np : src + (size_t)r * stride, np, np, x, y, L, a.inv_sigma, sc,
                                       T, nullptr, nullptr);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < kCheckStats; q++)
                    out[(size_t)q * kPointwisePiece + r] = T[0][q];
            }
        }
    }
}

// grid (n_keep, 3), one wave each: folds T[k][q][0 .. n) in sample order; n0 == 0: T[k][q][0] is the first sample ever
__global__ void __launch_bounds__(kPointwiseWave) check_stat_fold_kernel(CheckArgs a) {
#pragma clang fp contract(off)
    const int lane = threadIdx.x, k = blockIdx.x, q = blockIdx.y;
    const size_t at = (size_t)k * kCheckStats + q;
    const double *T = a.T + at * kPointwisePiece;
    const double *edges = a.edges ? a.edges + (size_t)q * a.n_edges : nullptr;
    unsigned long long *counts = a.counts ? a.counts + at * (size_t)(a.n_edges + 2) : nullptr;
    const unsigned int n = a.n;
    const bool first = a.n0 == 0;
    double origin, mn, mx, sum = a.stat_sum[at], sq = a.stat_sq[at];
    if (first) {
        origin = T[0];
        mn = INFINITY;
        mx = -INFINITY;
    } else {
        origin = a.stat_origin[at];
        mn = a.stat_min[at];
        mx = a.stat_max[at];
    }
    for (unsigned int t0 = 0; t0 < n; t0 += kPointwiseWave) {
        const int cnt = n - t0 < (unsigned int)kPointwiseWave ? (int)(n - t0) : kPointwiseWave;
        const double v = lane < cnt ? T[t0 + lane] : 0.0;
        const double d = v - origin;
        const double dd = d * d;
        if (counts && lane < cnt)
            atomicAdd(counts + check_slot(v, edges, a.n_edges), 1ull); // (an integer: exact in any order)
        for (int r = 0; r < cnt; r++) {
            sum += read_lane(d, r);
            sq += read_lane(dd, r);
            const double t = read_lane(v, r);
            mn = t < mn ? t : mn;
            mx = t > mx ? t : mx;
        }
    }
    if (lane == 0) {
        if (first)
            a.stat_origin[at] = origin;
        a.stat_sum[at] = sum;
        a.stat_sq[at] = sq;
        a.stat_min[at] = mn;
        a.stat_max[at] = mx;
    }
}

// grid n, one wave each: e[r][i], u[r][i] and T[r][0 .. 3) of the parameter row r over the n_x data x, y
template <int MODEL>
__global__ void __launch_bounds__(kPointwiseWave) check_values_kernel(const double *params, int n_par, int n_x, const double *x,
                                                                      const double *y, double inv_sigma, double *e, double *u,
                                                                      double *T) {
    const int r = blockIdx.x;
    SinConsts sc;
    sc.init();
    double t[1][kCheckStats];
    check_wave_stats<MODEL, 1>(params + (size_t)r * n_par, n_par, n_par, x, y, n_x, inv_sigma, sc, t, e + (size_t)r * n_x,
                               u + (size_t)r * n_x);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int q = 0; q < kCheckStats; q++)
            T[(size_t)r * kCheckStats + q] = t[0][q];
    }
}
} // namespace apemost
