// pt_pointwise.h -- on-device pointwise log-likelihood: the term l_i(theta) of every datum (x_i, y_i) under every kept
// sample of kept chains, folded from the sample rows [n_steps][n_chains][n_par+2] while they are still on the device
// into what WAIC, importance-sampling leave-one-out and DIC need.  No sample dump holds this quantity: a row carries
// only the sum over the data.
//
// The term.  The datum is (x_i, y_i), columns 0 and 1 of the sampler's data as they are at begin (of the kept chain's
// own ladder in a batch).  v = curve<MODEL>(par, n_par, x_i, k) is pt_predict.h's model curve, unchanged.  Contraction
// is off and every line is one rounding:
//   simplesin, sine3    r = v - y_i;  q = r * r;  l = q * c,  with c = 1.0 / ((-2.0 * sigma) * sigma) computed once on
//                       the host in fp64 from the sampler's sigma and kept in the state: the untempered term of
//                       apps/simplesin.c:31-36.  The constant -ln(sigma sqrt(2 pi)) is left out, as the reference
//                       leaves it out: every criterion is shifted by the same amount per datum;
//   pulse, pulse_vrot   L = log(v), the device library's fp64 log (not the table logarithm of the round kernels);
//                       w = y_i / v, a true fp64 division;  l = -(L + w): apps/pulse.c:50.  The parameter-1 offset that
//                       the reference adds to the sum is not a datum's term and is left out.
// A non-finite or non-positive v gives whatever IEEE arithmetic gives: there is no filter, and it touches the series
// of its own chain only.  APEMOST_MODEL_USER: the term is the optional hook apemost_user_pointwise(ctx, i) of the device
// model (include/apemost_device_model.h) over all n_cols columns of the data; a model without it has no term (term()
// is a lane's share of a sum, and finish() may do anything to that sum).  pt_user_fold.h holds that form of the
// kernels below: a lane keeps its row index i and a ctx over the rows instead of x_i and y_i, nothing else differs.
//
// The fold.  A series is s = (kept chain k, datum i), s = k * n_data + i.  Every item is one thread's chain of
// operations in kept-sample order, its state carried in device memory between calls: equal to a sequential host loop
// whatever the accumulate calls' boundaries are.
//   n                      kept samples so far;
//   origin[s]              l of the first sample ever accumulated (0 before there is one);
//   sum[s], sq[s]          with d = l - origin: sum += d; sq += d * d (the product rounded, then added); the first
//                          sample takes part like every other (its d is l - l);
//   m_up[s], S_up[s]       the running log-sum-exp of x = l: the first sample sets m = x, S = 1, later ones are
//                          evidence_lse_step (pt_evidence.h), unchanged.  lppd_i = m_up + ln(S_up / n);
//   m_dn[s], S_dn[s], S2_dn[s]   the running log-sum-exp of x = -l and, from the same exponentials, the running sum
//                          of their squares: the first sample sets m = x, S = 1, S2 = 1; later ones
//                            if (x > m) { t = exp(m - x); S = S * t + 1; tt = t * t; S2 = S2 * tt + 1; m = x; }
//                            else       { e = exp(x - m); S += e; ee = e * e; S2 += ee; }
//                          (every product rounded before its addition): two exp per sample and datum, not three.
//                          elpd_loo_i = -(m_dn + ln(S_dn / n)); the importance weights' effective sample size is
//                          S_dn^2 / S2_dn.
// Per kept chain, for DIC's posterior mean: par_origin[k][p] the first sample's parameter p, par_sum[k][p] the
// sequential sum of (parameter - par_origin), the first sample included.
//
// One launch per piece of at most kPointwisePiece kept steps: pointwise_fold_kernel, one wave per workgroup,
// (n_blocks + 1) workgroups per kept chain, predict_fold_kernel's shape.  Workgroup b < n_blocks owns 64 consecutive
// data, one per lane; x_i, y_i and the eight state words stay in registers over the piece.  The kept parameter rows are
// wave-uniform: they are staged through LDS in tiles of kPointwiseTile doubles and read as broadcasts.  A lane
// evaluates kPointwiseSide samples side by side, so that their curves, logarithms and exponentials are in flight
// together: where none of them moves a maximum only the additions stay in order; where one does, the samples are taken
// one by one, as evidence_fold_kernel does.  Both ways are the recurrence above, operation for operation.  Workgroup
// n_blocks of a kept chain folds the parameter sums, one lane per parameter.  No float atomics, contraction off, plain
// vector stores.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_evidence.h"
#include "pt_predict.h"

namespace apemost {

constexpr int kPointwiseWave = 64;
constexpr int kPointwisePiece = 8192; // kept steps of one launch
constexpr int kPointwiseTile = 512;   // doubles of one LDS tile of parameter rows: floor(512 / n_par) rows
constexpr int kPointwiseSide = 4;     // samples evaluated side by side

template <int MODEL>
__device__ __forceinline__ double pointwise_term(double v, double y, double c) {
#pragma clang fp contract(off)
    if (MODEL == APEMOST_MODEL_SIMPLESIN || MODEL == APEMOST_MODEL_SINE3) {
        const double r = v - y;
        const double q = r * r;
        return q * c;
    } else {
        const double L = log(v);
        const double w = y / v;
        const double t = L + w;
        return -t;
    }
}

// one update of the downward log-sum-exp and of the sum of squared exponentials, as the header states it
__device__ __forceinline__ void pointwise_lse2_step(double x, double &m, double &S, double &S2) {
#pragma clang fp contract(off)
    if (x > m) {
        const double t = exp(m - x);
        const double st = S * t;
        S = st + 1.0;
        const double tt = t * t;
        const double s2t = S2 * tt;
        S2 = s2t + 1.0;
        m = x;
    } else {
        const double e = exp(x - m);
        S += e;
        const double ee = e * e;
        S2 += ee;
    }
}

struct PointwiseArgs {
    const double *rows;               // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, n_keep;
    const int *chains;                // [n_keep]
    unsigned long long skip, thin;    // kept steps of this piece: skip, skip + thin, ... (n of them)
    unsigned int n;                   // kept steps of this piece, 1 .. kPointwisePiece
    unsigned long long n0;            // kept samples before this piece
    int n_data, n_blocks;             // n_blocks = ceil(n_data / 64)
    const double *x, *y;              // [n_keep][n_data]: every kept chain's data (a user model: x its rows,
                                      // [n_keep][n_cols][n_data], column-major per kept chain; y unused)
    double c;                         // 1 / (-2 sigma^2) (the sine models)
    int n_cols;                       // (a user model's ctx: columns of the rows, the sampler's sigma and hmin)
    double sigma, hmin;
    double *origin, *sum, *sq, *m_up, *S_up, *m_dn, *S_dn, *S2_dn; // [n_keep][n_data]
    double *par_origin, *par_sum;     // [n_keep][n_par]
    const int *len;                   // [n_keep]: the data kept chain k really has, <= n_data (a batch whose ladders
                                      // differ in length); series past them are never touched.  nullptr: n_data
};

// Where a lane's term comes from: its datum in registers and the built-in curve and term.  (pt_user_fold.h: the row
// index and a ctx.)  at() is called by active lanes only; par may point into LDS.
template <int MODEL>
struct PointwiseTermAt {
    SinConsts sc;
    double x, y, c;
    int np;
    __device__ __forceinline__ void init(const PointwiseArgs &a, int, int, size_t s, bool active) {
        sc.init();
        x = active ? a.x[s] : 0.0;
        y = active ? a.y[s] : 0.0;
        c = a.c;
        np = a.n_par;
    }
    __device__ __forceinline__ double at(const double *par) const {
        return pointwise_term<MODEL>(curve<MODEL>(par, np, x, sc), y, c);
    }
};

// a workgroup of pointwise_fold_kernel: grid (n_blocks + 1) * n_keep, one wave each
template <class EVAL>
__device__ __forceinline__ void pointwise_fold_body(const PointwiseArgs &a) {
#pragma clang fp contract(off)
    __shared__ double tile[kPointwiseTile];
    const int lane = threadIdx.x;
    const int k = blockIdx.x / (a.n_blocks + 1), blk = blockIdx.x - k * (a.n_blocks + 1);
    const int np = a.n_par, n = (int)a.n;
    const size_t w = (size_t)np + 2, stride = (size_t)a.thin * a.n_chains * w;
    const double *src = a.rows + a.skip * a.n_chains * w + (size_t)a.chains[k] * w;
    if (blk == a.n_blocks) {
        // the parameter sums: lane j folds the parameters j, j + 64, ... over the piece's steps in order
        for (int p = lane; p < np; p += kPointwiseWave) {
            const size_t at = (size_t)k * np + p;
            const double o = a.n0 == 0 ? src[p] : a.par_origin[at];
            double s = a.par_sum[at];
#pragma unroll 8
            for (int t = 0; t < n; t++)
                s += src[(size_t)t * stride + p] - o;
            if (a.n0 == 0)
                a.par_origin[at] = o;
            a.par_sum[at] = s;
        }
        return;
    }
    const int i = blk * kPointwiseWave + lane;
    const bool active = i < (a.len ? a.len[k] : a.n_data);
    const size_t s = (size_t)k * a.n_data + (active ? i : 0);
    EVAL ev;
    ev.init(a, k, i, s, active);
    const bool first = a.n0 == 0;
    double origin = 0, sum = 0, sq = 0, m_up = 0, S_up = 0, m_dn = 0, S_dn = 0, S2_dn = 0;
    if (active) {
        sum = a.sum[s];
        sq = a.sq[s];
        if (first) { // the first sample ever: the origin and both maxima; its d = l - l enters the sums below
            origin = ev.at(src);
            m_up = origin;
            m_dn = -origin;
            S_up = S_dn = S2_dn = 1.0;
            const double d = origin - origin;
            sum += d;
            const double dd = d * d;
            sq += dd;
        } else {
            origin = a.origin[s];
            m_up = a.m_up[s];
            S_up = a.S_up[s];
            m_dn = a.m_dn[s];
            S_dn = a.S_dn[s];
            S2_dn = a.S2_dn[s];
        }
    }
    auto add = [&](double l) {
        const double d = l - origin;
        sum += d;
        const double dd = d * d;
        sq += dd;
    };
    const int per_tile = kPointwiseTile / np; // >= 1 (n_par <= kPointwiseTile is checked at begin)
    for (int t0 = 0; t0 < n; t0 += per_tile) {
        const int cnt = n - t0 < per_tile ? n - t0 : per_tile;
        __syncthreads(); // the tile before has been read
        for (int e = lane; e < cnt * np; e += kPointwiseWave) {
            const int r = e / np, p = e - r * np;
            tile[e] = src[(size_t)(t0 + r) * stride + p];
        }
        __syncthreads();
        if (active) {
            int r = first && t0 == 0 ? 1 : 0;
            for (; r + kPointwiseSide <= cnt; r += kPointwiseSide) {
                double l[kPointwiseSide], xd[kPointwiseSide];
                bool up = false, dn = false;
#pragma unroll
                for (int j = 0; j < kPointwiseSide; j++) {
                    l[j] = ev.at(tile + (r + j) * np);
                    xd[j] = -l[j];
                    up = up || l[j] > m_up;
                    dn = dn || xd[j] > m_dn;
                }
#pragma unroll
                for (int j = 0; j < kPointwiseSide; j++)
                    add(l[j]);
                if (up) {
#pragma unroll
                    for (int j = 0; j < kPointwiseSide; j++)
                        evidence_lse_step(l[j], m_up, S_up);
                } else {
                    double e[kPointwiseSide];
#pragma unroll
                    for (int j = 0; j < kPointwiseSide; j++)
                        e[j] = exp(l[j] - m_up);
#pragma unroll
                    for (int j = 0; j < kPointwiseSide; j++)
                        S_up += e[j];
                }
                if (dn) {
#pragma unroll
                    for (int j = 0; j < kPointwiseSide; j++)
                        pointwise_lse2_step(xd[j], m_dn, S_dn, S2_dn);
                } else {
                    double e[kPointwiseSide], ee[kPointwiseSide];
#pragma unroll
                    for (int j = 0; j < kPointwiseSide; j++) {
                        e[j] = exp(xd[j] - m_dn);
                        ee[j] = e[j] * e[j];
                    }
#pragma unroll
                    for (int j = 0; j < kPointwiseSide; j++) {
                        S_dn += e[j];
                        S2_dn += ee[j];
                    }
                }
            }
            for (; r < cnt; r++) {
                const double l = ev.at(tile + r * np);
                add(l);
                evidence_lse_step(l, m_up, S_up);
                pointwise_lse2_step(-l, m_dn, S_dn, S2_dn);
            }
        }
    }
    if (active) {
        if (first)
            a.origin[s] = origin;
        a.sum[s] = sum;
        a.sq[s] = sq;
        a.m_up[s] = m_up;
        a.S_up[s] = S_up;
        a.m_dn[s] = m_dn;
        a.S_dn[s] = S_dn;
        a.S2_dn[s] = S2_dn;
    }
}

template <int MODEL>
__global__ void __launch_bounds__(kPointwiseWave) pointwise_fold_kernel(PointwiseArgs a) {
    pointwise_fold_body<PointwiseTermAt<MODEL>>(a);
}

// out[r][i] = l_i(params[r]); grid ceil(n_data / 64) * n
template <int MODEL>
__global__ void __launch_bounds__(kPointwiseWave) pointwise_loglike_kernel(const double *params, int n_par, int n_data,
                                                                           const double *x, const double *y, double c,
                                                                           double *out) {
#pragma clang fp contract(off)
    const int n_blocks = (n_data + kPointwiseWave - 1) / kPointwiseWave;
    const int r = blockIdx.x / n_blocks, i = (blockIdx.x - r * n_blocks) * kPointwiseWave + (int)threadIdx.x;
    if (i >= n_data)
        return;
    SinConsts sc;
    sc.init();
    out[(size_t)r * n_data + i] = pointwise_term<MODEL>(curve<MODEL>(params + (size_t)r * n_par, n_par, x[i], sc), y[i], c);
}

} // namespace apemost
