// pt_predict.h -- on-device posterior predictive: the model curve of every built-in likelihood, evaluated at the
// abscissae x_0 .. x_{n_x-1} for every kept sample of kept chains, folded from the sample rows
// [n_steps][n_chains][n_par+2] while they are still on the device.
//
// The curve.  curve<MODEL>(par, n_par, x, k) is the quantity inside the data loop of the model's likelihood, with
// contraction off and in exactly this operation order (every line one rounding unless it says otherwise):
//   simplesin   par = a, f, ph, o:    u = f*x + ph (two roundings);  m = a * sin_cw(kTwoPi*u, u) + o (the product and
//               the sum rounded separately): Model<SIMPLESIN>::term's unfused form.  NaN when
//               !(kTwoPi * (fabs(f)*fabs(x) + fabs(ph)) < 2^45): sin_cw's range, tested per point here;
//   sine3       par = (a, f, ph) x 3, o:  m = 0; for c in 0..2: u = f[c]*x + ph[c]; m += a[c]*sin_cw(kTwoPi*u, u);
//               then m += o.  NaN when any of the three sines fails the test above;
//   pulse       par = lifetime, (unused), (freq_j, h_j) ...:  y = 0; for each mode j: d = freq_j - x;
//               t = (kTwoPi*d)*lifetime; y += h_j / (1 + t*t), a true fp64 division (apps/pulse.c:41-48 -- pow(t, 2)
//               is the correctly rounded square, so t*t is it);
//   pulse_vrot  par = lifetime, (unused), vrot, f3, h3, f5, h5:  the four terms of apps/pulse_vrot.c:45-59 in that
//               order, at the distances f3 - x, (f5 - x) + (-vrot), f5 - x, (f5 - x) + vrot.
// APEMOST_MODEL_USER: the curve is the optional hook apemost_user_curve(ctx, i) of the device model
// (include/apemost_device_model.h); a model without it has no curve.  pt_user_fold.h holds that form of the kernels
// below: a lane keeps its row index i and a ctx over the rows being evaluated instead of x_i, nothing else differs.
//
// The fold.  A series s = (kept chain k, abscissa i) has the samples v_t = curve(parameters of kept sample t of chain k,
// x_i).  Per series, each equal to a sequential host loop over the kept samples whatever the calls' boundaries are:
//   origin[s]       v_0 of the first sample ever accumulated;
//   sum[s], sq[s]   with d = v - origin: sum += d; sq += d*d (the product rounded, then added);
//   vmin, vmax      from +inf and -inf by strict < and >: a NaN never enters;
//   hist[s][b]      counts over the run summary's edges of [lo, hi] (summary_edge, summary_bin), shared by all series;
//                   values outside and NaN are not counted.
// Per kept chain the best sample: the largest column n_par (prob) from -inf by strict >, so the first occurrence wins
// and a NaN never does; its parameter row and its 1-based kept index (0 before there is one).
//
// One launch per piece of at most kPredictPiece kept steps (the staging size): predict_fold_kernel, one wave per
// workgroup, (n_blocks + 1) workgroups per kept chain.  Workgroup b < n_blocks owns `points` consecutive abscissae,
// one per lane (64 without histograms; fewer where points * nbins counters of 32 bits would not fit the LDS budget).
// The kept parameter rows are wave-uniform: they are staged through LDS in tiles of kPredictTile doubles and read as
// broadcasts.  A lane evaluates kPredictSide samples' curves side by side -- the only dependency between samples is
// the pair of additions -- and adds them in order; origin, sum, sq, vmin and vmax stay in registers over the piece.
// Histogram rows are u32 counters in LDS, one row per lane (ds_add_u32, nothing contended; the rows are padded to an odd
// number of words so that the lanes start in different banks), flushed to the u64 counts in global memory with plain
// loads and stores at the end of the piece; the edges are computed once per workgroup, and where they are strictly
// increasing a value's bin is a guess from the spacing walked to the bin that holds it, which is the bisection's bin
// without its chain of dependent LDS reads (predict_bin).
// Workgroup n_blocks of a kept chain scans prob: every lane its own strided share, then lane 0 joins the 64 candidates
// in index order.  No float atomics, contraction off, plain vector stores.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_device.h"
#include "pt_summary.h"

namespace apemost {

constexpr int kPredictWave = 64;
constexpr int kPredictPiece = 8192;   // kept steps of one launch
constexpr int kPredictTile = 512;     // doubles of one LDS tile of parameter rows: floor(512 / n_par) rows
constexpr int kPredictSide = 4;       // samples evaluated side by side
constexpr int kPredictMaxBins = 4096;
constexpr int kPredictLdsBudget = 56 * 1024; // edges and histogram rows (dynamic LDS); the tile is static

// a lane's row of counters: nbins words padded to an odd number, so that the rows of the 64 lanes start in different
// LDS banks (at 200 bins an unpadded stride of 800 bytes would put every eighth lane on the same bank)
inline __host__ __device__ int predict_row_words(int nbins) { return nbins | 1; }
// points per workgroup: 64, or what the histogram rows leave room for (at least 1: 4097 edges + 4097 counters fit)
inline int predict_points(int nbins) {
    if (nbins <= 0)
        return kPredictWave;
    const int room = (kPredictLdsBudget - (nbins + 1) * (int)sizeof(double)) /
                     (predict_row_words(nbins) * (int)sizeof(unsigned int));
    return room < 1 ? 1 : room > kPredictWave ? kPredictWave : room;
}
inline size_t predict_lds_bytes(int nbins, int points) {
    return nbins <= 0 ? 0
                      : (size_t)(nbins + 1) * sizeof(double) +
                            (size_t)points * predict_row_words(nbins) * sizeof(unsigned int);
}

// summary_bin's answer without its chain of ceil(log2 nbins) dependent LDS reads.  Where the edges are strictly
// increasing (`sorted`, settled once per workgroup) exactly one bin b has e[b] <= v < e[b+1] for a v inside
// [e[0], e[nbins]), and the bisection, whose invariant is e[left] <= v < e[right], ends in it: so a guess from the
// spacing, walked to the bin that holds v, is the same bin.  GSL's uniform edges are not always sorted (pt_summary.h);
// there the bisection itself runs.
// (the guess: any bin index will do, the walk settles it; scale = nbins / (hi - lo); 0 for a NaN)
__device__ __forceinline__ int predict_guess(double v, int nbins, double lo, double scale) {
#pragma clang fp contract(off)
    const double t = (v - lo) * scale;
    return t >= 0 && t < (double)nbins ? (int)t : t >= (double)nbins ? nbins - 1 : 0;
}
// (the walk from the guess g, whose edges el = e[g] and eh = e[g+1] the caller has read already -- for several values
// side by side, so that their LDS reads are in flight together)
__device__ __forceinline__ int predict_walk(double v, const double *e, int nbins, double e0, double etop, int g,
                                            double el, double eh) {
    if (!(v >= e0 && v < etop))
        return -1;
    if (v >= el && v < eh)
        return g;
    while (g > 0 && v < e[g])
        g--;
    while (g < nbins - 1 && v >= e[g + 1])
        g++;
    return g;
}
__device__ __forceinline__ int predict_bin(double v, const double *e, int nbins, double e0, double etop, double lo,
                                           double scale, bool sorted) {
    if (!sorted)
        return summary_bin(v, e, nbins);
    const int g = predict_guess(v, nbins, lo, scale);
    return predict_walk(v, e, nbins, e0, etop, g, e[g], e[g + 1]);
}

__device__ __forceinline__ bool predict_sine_in_range(double f, double ph, double x) {
#pragma clang fp contract(off)
    return kTwoPi * (fabs(f) * fabs(x) + fabs(ph)) < 35184372088832.0; // 2^45; false for NaN
}

template <int MODEL>
__device__ __forceinline__ double curve(const double *par, int n_par, double x, const SinConsts &k);

template <>
__device__ __forceinline__ double curve<APEMOST_MODEL_SIMPLESIN>(const double *par, int, double x, const SinConsts &k) {
#pragma clang fp contract(off)
    const double a = par[0], f = par[1], ph = par[2], o = par[3];
    const double fx = f * x;
    const double u = fx + ph;
    const double as = a * sin_cw(kTwoPi * u, u, k);
    const double m = as + o;
    return predict_sine_in_range(f, ph, x) ? m : __longlong_as_double(0x7ff8000000000000ll);
}

template <>
__device__ __forceinline__ double curve<APEMOST_MODEL_SINE3>(const double *par, int, double x, const SinConsts &k) {
#pragma clang fp contract(off)
    double m = 0;
    bool in_range = true;
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double a = par[3 * c], f = par[3 * c + 1], ph = par[3 * c + 2];
        const double fx = f * x;
        const double u = fx + ph;
        const double as = a * sin_cw(kTwoPi * u, u, k);
        m += as;
        in_range = in_range && predict_sine_in_range(f, ph, x);
    }
    m += par[9];
    return in_range ? m : __longlong_as_double(0x7ff8000000000000ll);
}

__device__ __forceinline__ double predict_lorentz(double h, double d, double lifetime) {
#pragma clang fp contract(off)
    const double t = (kTwoPi * d) * lifetime;
    const double tt = t * t;
    return h / (1 + tt);
}

template <>
__device__ __forceinline__ double curve<APEMOST_MODEL_PULSE>(const double *par, int n_par, double x, const SinConsts &) {
#pragma clang fp contract(off)
    const double lifetime = par[0];
    double y = 0;
    for (int j = 2; j + 1 < n_par; j += 2)
        y += predict_lorentz(par[j + 1], par[j] - x, lifetime);
    return y;
}

template <>
__device__ __forceinline__ double curve<APEMOST_MODEL_PULSE_VROT>(const double *par, int, double x, const SinConsts &) {
#pragma clang fp contract(off)
    const double lifetime = par[0], vrot = par[2];
    double y = 0;
    y += predict_lorentz(par[4], par[3] - x, lifetime);
    const double d = par[5] - x;
    y += predict_lorentz(par[6], d + -vrot, lifetime);
    y += predict_lorentz(par[6], d, lifetime);
    y += predict_lorentz(par[6], d + vrot, lifetime);
    return y;
}

struct PredictArgs {
    const double *rows;               // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, n_keep;
    const int *chains;                // [n_keep]
    unsigned long long skip, thin;    // kept steps of this piece: skip, skip + thin, ... (n of them)
    unsigned int n;                   // kept steps of this piece, 1 .. kPredictPiece
    unsigned long long n0;            // kept samples before this piece
    int n_x;
    const double *x;                  // [n_keep][n_x]: every kept chain's abscissae (a user model: its rows,
                                      // [n_keep][n_cols][n_x], column-major per kept chain)
    int n_cols;                       // (a user model's ctx: columns of the rows, the sampler's sigma and hmin)
    double sigma, hmin;
    int nbins, points, n_blocks;      // points per workgroup, n_blocks = ceil(n_x / points)
    double lo, hi;
    double *origin, *sum, *sq, *vmin, *vmax; // [n_keep][n_x]
    unsigned long long *hist;         // [n_keep][n_x][nbins]
    double *best_prob, *best_params;  // [n_keep], [n_keep][n_par]
    unsigned long long *best_n;       // [n_keep]
    const int *len;                   // [n_keep]: the abscissae kept chain k really has, <= n_x (the data of a batch
                                      // whose ladders differ in length); series past them are never touched.
                                      // nullptr: n_x for every kept chain
};

// Where a lane's value comes from: its abscissa in a register and the built-in curve.  (pt_user_fold.h: the row index
// and a ctx.)  at() is called by active lanes only; par may point into LDS.
template <int MODEL>
struct PredictCurveAt {
    SinConsts sc;
    double x;
    int np;
    __device__ __forceinline__ void init(const PredictArgs &a, int, int, size_t s, bool active) {
        sc.init();
        x = active ? a.x[s] : 0.0;
        np = a.n_par;
    }
    __device__ __forceinline__ double at(const double *par) const { return curve<MODEL>(par, np, x, sc); }
};

// a workgroup of predict_fold_kernel: grid (n_blocks + 1) * n_keep, one wave each; dynamic LDS
// predict_lds_bytes(nbins, points)
template <class EVAL, bool HIST>
__device__ __forceinline__ void predict_fold_body(const PredictArgs &a) {
#pragma clang fp contract(off)
    __shared__ double tile[kPredictTile];
    extern __shared__ double predict_lds[];
    const int lane = threadIdx.x;
    const int k = blockIdx.x / (a.n_blocks + 1), blk = blockIdx.x - k * (a.n_blocks + 1);
    const int np = a.n_par, n = (int)a.n;
    const size_t w = (size_t)np + 2, stride = (size_t)a.thin * a.n_chains * w;
    const double *src = a.rows + a.skip * a.n_chains * w + (size_t)a.chains[k] * w;
    if (blk == a.n_blocks) {
        // the best sample: lane j scans the piece's steps j, j + 64, ...; lane 0 joins the candidates
        double bp = a.best_prob[k];
        int bi = -1;
        for (int t = lane; t < n; t += kPredictWave) {
            const double p = src[(size_t)t * stride + np];
            if (p > bp) {
                bp = p;
                bi = t;
            }
        }
        int *cand_i = (int *)(tile + kPredictWave);
        tile[lane] = bp;
        cand_i[lane] = bi;
        __syncthreads();
        if (lane == 0) {
            double best = a.best_prob[k];
            int at = -1;
            for (int j = 0; j < kPredictWave; j++) {
                const int i = cand_i[j];
                if (i < 0)
                    continue;
                const double p = tile[j];
                if (p > best || (p == best && at >= 0 && i < at)) {
                    best = p;
                    at = i;
                }
            }
            if (at >= 0) {
                a.best_prob[k] = best;
                a.best_n[k] = a.n0 + (unsigned long long)at + 1ull;
                for (int p = 0; p < np; p++)
                    a.best_params[(size_t)k * np + p] = src[(size_t)at * stride + p];
            }
        }
        return;
    }
    const int i0 = blk * a.points, i = i0 + lane;
    const int n_mine = a.len ? a.len[k] : a.n_x; // (uniform over the workgroup)
    const bool active = lane < a.points && i < n_mine;
    const size_t s = (size_t)k * a.n_x + (active ? i : 0);
    EVAL ev;
    ev.init(a, k, i, s, active);
    double *edges = predict_lds;
    unsigned int *bins = (unsigned int *)(predict_lds + a.nbins + 1);
    const int here = n_mine - i0 < a.points ? n_mine - i0 : a.points; // abscissae of this workgroup (<= 0: none)
    const int rw = predict_row_words(a.nbins);
    bool sorted = true;
    double e0 = 0, etop = 0, scale = 0;
    if (HIST) {
        for (int b = lane; b <= a.nbins; b += kPredictWave)
            edges[b] = summary_edge(a.lo, a.hi, b, a.nbins);
        for (int b = lane; b < here * rw; b += kPredictWave)
            bins[b] = 0;
        __syncthreads();
        bool mine = true;
        for (int b = lane; b < a.nbins; b += kPredictWave)
            mine = mine && edges[b] < edges[b + 1];
        sorted = __syncthreads_and(mine) != 0;
        e0 = edges[0];
        etop = edges[a.nbins];
        scale = (double)a.nbins / (a.hi - a.lo);
    }
    double origin = 0, sum = 0, sq = 0, vmin = 0, vmax = 0;
    if (active) {
        origin = a.n0 == 0 ? ev.at(src) : a.origin[s];
        sum = a.sum[s];
        sq = a.sq[s];
        vmin = a.vmin[s];
        vmax = a.vmax[s];
    }
    unsigned int *row = bins + (size_t)lane * rw;
    auto add = [&](double v) {
        const double d = v - origin;
        sum += d;
        const double dd = d * d;
        sq += dd;
        if (v < vmin)
            vmin = v;
        if (v > vmax)
            vmax = v;
    };
    auto count = [&](int b) {
        if (b >= 0)
            atomicAdd(&row[b], 1u);
    };
    const int per_tile = kPredictTile / np; // >= 1 (n_par <= kPredictTile is checked at begin)
    for (int t0 = 0; t0 < n; t0 += per_tile) {
        const int cnt = n - t0 < per_tile ? n - t0 : per_tile;
        __syncthreads(); // the tile before has been read (and, the first time, edges and bins are written)
        for (int e = lane; e < cnt * np; e += kPredictWave) {
            const int r = e / np, p = e - r * np;
            tile[e] = src[(size_t)(t0 + r) * stride + p];
        }
        __syncthreads();
        if (active) {
            int r = 0;
            for (; r + kPredictSide <= cnt; r += kPredictSide) {
                double v[kPredictSide];
#pragma unroll
                for (int j = 0; j < kPredictSide; j++)
                    v[j] = ev.at(tile + (r + j) * np);
                if (HIST) {
                    int b[kPredictSide];
                    if (sorted) {
                        int g[kPredictSide];
                        double el[kPredictSide], eh[kPredictSide];
#pragma unroll
                        for (int j = 0; j < kPredictSide; j++) {
                            g[j] = predict_guess(v[j], a.nbins, a.lo, scale);
                            el[j] = edges[g[j]];
                            eh[j] = edges[g[j] + 1];
                        }
#pragma unroll
                        for (int j = 0; j < kPredictSide; j++)
                            b[j] = predict_walk(v[j], edges, a.nbins, e0, etop, g[j], el[j], eh[j]);
                    } else {
#pragma unroll
                        for (int j = 0; j < kPredictSide; j++)
                            b[j] = summary_bin(v[j], edges, a.nbins);
                    }
#pragma unroll
                    for (int j = 0; j < kPredictSide; j++)
                        count(b[j]);
                }
#pragma unroll
                for (int j = 0; j < kPredictSide; j++)
                    add(v[j]);
            }
            for (; r < cnt; r++) {
                const double v = ev.at(tile + r * np);
                if (HIST)
                    count(predict_bin(v, edges, a.nbins, e0, etop, a.lo, scale, sorted));
                add(v);
            }
        }
    }
    if (active) {
        if (a.n0 == 0)
            a.origin[s] = origin;
        a.sum[s] = sum;
        a.sq[s] = sq;
        a.vmin[s] = vmin;
        a.vmax[s] = vmax;
    }
    if (HIST) {
        __syncthreads();
        // this workgroup's series are consecutive: its slice of hist is one run of here * nbins counts
        unsigned long long *hist = a.hist + ((size_t)k * a.n_x + i0) * a.nbins;
        for (int b = lane; b < here * a.nbins; b += kPredictWave) {
            const int p = b / a.nbins;
            hist[b] += bins[p * rw + (b - p * a.nbins)];
        }
    }
}

template <int MODEL, bool HIST>
__global__ void __launch_bounds__(kPredictWave) predict_fold_kernel(PredictArgs a) {
    predict_fold_body<PredictCurveAt<MODEL>, HIST>(a);
}

// out[r][i] = curve(params[r], x[i]); grid ceil(n_x / 64) * n
template <int MODEL>
__global__ void __launch_bounds__(kPredictWave) predict_curve_kernel(const double *params, int n_par, int n_x,
                                                                     const double *x, double *out) {
#pragma clang fp contract(off)
    const int n_blocks = (n_x + kPredictWave - 1) / kPredictWave;
    const int r = blockIdx.x / n_blocks, i = (blockIdx.x - r * n_blocks) * kPredictWave + (int)threadIdx.x;
    if (i >= n_x)
        return;
    SinConsts sc;
    sc.init();
    out[(size_t)r * n_x + i] = curve<MODEL>(params + (size_t)r * n_par, n_par, x[i], sc);
}

} // namespace apemost
