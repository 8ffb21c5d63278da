// pt_autocorr.h -- on-device autocorrelation: the lag sums of sample columns of kept chains, folded from the sample rows
// [n_steps][n_chains][n_par+2] while they are still on the device.  A series s = (kept chain k, column c) has the
// samples x_0, x_1, ... in kept order and d_t = x_t - origin.  Per series, each equal to a sequential host loop over the
// kept samples, whatever the calls' boundaries are (L = max_lag, H = L - 1):
//   origin[s]     x_0 of the first sample ever accumulated;
//   sum[s]        sum += d_t;
//   lag[s][l]     for l = 0 .. L-1: lag += d_t * d_{t-l} over t >= l in ascending t (the product rounded, then added);
//   head[s][j]    for j < H: d_j (0 where j >= n);
//   tail[s][j]    for j < H: d of sample n - H + j (0 where that index is negative): the carry across calls.
// Three launches per piece of kept steps:
//   autocorr_gather_kernel  reads the rows once: buf[s][0 .. H) = tail[s] (the history), buf[s][H + i] = d of kept step i
//                           of the piece; time is the fastest index.  Sets origin on the first piece and head while
//                           n < H;
//   autocorr_fold_kernel    grid (n_groups + 1, n_series), one wave per workgroup.  Workgroup g < n_groups owns the 256
//                           lags l0 = 256 g ..: lane j takes lags l0 + j, l0 + 64 + j, l0 + 128 + j, l0 + 192 + j, four
//                           independent chains of additions, so that the wave issues a multiply or an add every pass
//                           and never waits for the add before.  It walks time in tiles through LDS: d_t is a
//                           broadcast read, d_{t-l} of one of the four lags a ds_read_b64 of 64 consecutive doubles
//                           across the lanes, which is free of bank conflicts.  A lag l of a piece that starts at
//                           sample n0 begins at piece index max(0, l - n0): only the tiles of the ramp-up (n < L)
//                           test it per step.  Workgroup n_groups is one lane that adds the sum.  lag and sum are
//                           carried in global memory between calls;
//   autocorr_carry_kernel   tail[s][j] = buf[s][n + j]: the last H entries of history and piece together.
// The order within a series is never split across workgroups.  No atomics, contraction off, plain vector stores.
#pragma once

#include <hip/hip_runtime.h>

namespace apemost {

constexpr int kAutocorrMaxLag = 4096;
constexpr int kAutocorrWave = 64;          // fold: one wave per workgroup
constexpr int kAutocorrPerLane = 4;        // lags of one lane
constexpr int kAutocorrGroup = kAutocorrWave * kAutocorrPerLane; // lags of one workgroup
constexpr int kAutocorrTile = 2048;        // time steps of one LDS tile
constexpr int kAutocorrThreads = 256;      // gather and carry

struct AutocorrArgs {
    const double *rows;                    // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, n_keep, n_cols;
    const int *chains;                     // [n_keep]
    const int *cols;                       // [n_cols]
    unsigned long long skip, thin;         // kept steps of this piece: skip, skip + thin, ... (n of them)
    unsigned int n;                        // kept steps of this piece, 1 .. chunk
    unsigned long long n0;                 // kept samples before this piece
    int max_lag;                           // L
    int n_groups;                          // ceil(L / kAutocorrGroup)
    unsigned long long stride;             // H + chunk: one series of buf
    double *buf;                           // [n_series][H + chunk]
    double *origin, *sum;                  // [n_series]
    double *lag;                           // [n_series][L]
    double *head, *tail;                   // [n_series][H]
};

// grid (ceil((H + n) / 256), n_series): thread g < H copies history slot g, thread H + i stages kept step i
__global__ void __launch_bounds__(kAutocorrThreads) autocorr_gather_kernel(AutocorrArgs a) {
    const unsigned int g = blockIdx.x * (unsigned int)kAutocorrThreads + threadIdx.x;
    const unsigned int H = (unsigned int)a.max_lag - 1u;
    const int s = blockIdx.y, k = s / a.n_cols, c = s - k * a.n_cols;
    double *buf = a.buf + (size_t)s * a.stride;
    if (g < H) {
        buf[g] = a.tail[(size_t)s * H + g];
        return;
    }
    const unsigned int i = g - H;
    if (i >= a.n)
        return;
    const size_t w = (size_t)a.n_par + 2, row = (size_t)a.n_chains * w;
    const double *src = a.rows + a.skip * row + (size_t)a.chains[k] * w + a.cols[c];
    const double o = a.n0 == 0 ? src[0] : a.origin[s];
    const double d = src[(size_t)i * a.thin * row] - o;
    buf[H + i] = d;
    if (a.n0 + i < H)
        a.head[(size_t)s * H + a.n0 + i] = d;
    if (a.n0 == 0 && i == 0)
        a.origin[s] = o;
}

// grid (n_groups + 1, n_series)
__global__ void __launch_bounds__(kAutocorrWave) autocorr_fold_kernel(AutocorrArgs a) {
#pragma clang fp contract(off)
    __shared__ double xt[kAutocorrTile];
    __shared__ double win[kAutocorrTile + kAutocorrGroup];
    const int lane = threadIdx.x, s = blockIdx.y;
    const int L = a.max_lag, H = L - 1, n = (int)a.n;
    const double *buf = a.buf + (size_t)s * a.stride;
    if ((int)blockIdx.x == a.n_groups) { // the sum: one chain of additions
        if (lane == 0) {
            double t = a.sum[s];
#pragma unroll 8
            for (int i = 0; i < n; i++)
                t += buf[H + i];
            a.sum[s] = t;
        }
        return;
    }
    const int l0 = blockIdx.x * kAutocorrGroup;
    double acc[kAutocorrPerLane];
    int start[kAutocorrPerLane], off[kAutocorrPerLane];
#pragma unroll
    for (int k = 0; k < kAutocorrPerLane; k++) {
        const int l = l0 + k * kAutocorrWave + lane;
        acc[k] = l < L ? a.lag[(size_t)s * L + l] : 0.0;
        start[k] = (unsigned long long)l > a.n0 ? l - (int)a.n0 : 0; // first piece index with t >= l
        off[k] = kAutocorrGroup - 1 - k * kAutocorrWave - lane;      // 0 .. 255: slot of d_{t-l} in the window at r = 0
    }
    // tiles below this piece index hold a step that some lag of the workgroup must still skip
    const long long ramp = (long long)l0 + kAutocorrGroup - 1 - (long long)(a.n0 < (1ull << 40) ? a.n0 : 1ull << 40);
    for (int i0 = 0; i0 < n; i0 += kAutocorrTile) {
        const int cnt = n - i0 < kAutocorrTile ? n - i0 : kAutocorrTile;
        // window slot w holds buf[wbase + w]; the slots before the buffer belong to lags >= L alone
        const int wbase = H + i0 - l0 - (kAutocorrGroup - 1);
        __syncthreads();
        for (int w = lane; w < cnt + kAutocorrGroup - 1; w += kAutocorrWave) {
            const int p = wbase + w; // <= H + i0 + cnt - 1 - l0 < H + n
            win[w] = p >= 0 ? buf[p] : 0.0;
        }
        for (int r = lane; r < cnt; r += kAutocorrWave)
            xt[r] = buf[H + i0 + r];
        __syncthreads();
        if ((long long)i0 >= ramp) {
#pragma unroll 8
            for (int r = 0; r < cnt; r++) {
                const double x = xt[r];
#pragma unroll
                for (int k = 0; k < kAutocorrPerLane; k++) {
                    const double prod = x * win[r + off[k]];
                    acc[k] += prod;
                }
            }
        } else {
            for (int r = 0; r < cnt; r++) {
                const double x = xt[r];
#pragma unroll
                for (int k = 0; k < kAutocorrPerLane; k++) {
                    const double prod = x * win[r + off[k]];
                    if (i0 + r >= start[k])
                        acc[k] += prod;
                }
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kAutocorrPerLane; k++) {
        const int l = l0 + k * kAutocorrWave + lane;
        if (l < L)
            a.lag[(size_t)s * L + l] = acc[k];
    }
}

// grid (ceil(H / 256), n_series); H >= 1
__global__ void __launch_bounds__(kAutocorrThreads) autocorr_carry_kernel(AutocorrArgs a) {
    const unsigned int j = blockIdx.x * (unsigned int)kAutocorrThreads + threadIdx.x;
    const unsigned int H = (unsigned int)a.max_lag - 1u;
    if (j >= H)
        return;
    const int s = blockIdx.y;
    a.tail[(size_t)s * H + j] = a.buf[(size_t)s * a.stride + a.n + j];
}

} // namespace apemost
