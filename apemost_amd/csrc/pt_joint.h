// pt_joint.h -- on-device joint marginals: how the parameters of a kept chain depend on each other, folded from the
// sample rows [n_steps][n_chains][n_par+2] while they are still on the device.  Two running quantities per kept chain k,
// each equal to a sequential host loop over the kept samples, whatever the calls' boundaries are:
//   counts[k][q][a][b]  samples whose parameter i falls in bin a and whose parameter j falls in bin b, for every
//                       requested pair q = (i, j), i < j.  The bins are the run summary's (pt_summary.h): the edges of
//                       summary_edge, the bisection of summary_bin, both called here and not restated, so the two
//                       projections of counts[k][q] are the 1-D histograms of the summary by construction.  A sample
//                       counts only where both values have a bin;
//   origin, sum, cross  moments about a fixed origin: origin[k][p] is parameter p of the first sample ever accumulated,
//                       and with d_p = v_p - origin_p, sum[k][p] += d_p and cross[k][i][j] += d_i * d_j (i <= j; the
//                       product rounded, then added) in sample order.
// Three launches per chunk of kept steps:
//   joint_gather_kernel   reads the rows once: the kept steps of every kept chain's n_par columns go, contiguous, into
//                         vals[k][p][chunk], and the bin of each value (bisected once per value, over the column's
//                         edges in LDS) into bins[k][p][chunk] as 16 bits; 0xffff: no bin;
//   joint_pair_kernel     one workgroup per (band, q, k).  A grid of nbins x nbins u32 counters does not fit a
//                         workgroup's LDS beyond 128 x 128, so it is cut into bands of whole a-rows of at most 16384
//                         counters (64 KiB).  The workgroup reads the two contiguous 16-bit bin columns of its pair,
//                         counts in LDS (ds_add_u32) the samples whose a lies in its band, and adds its counters into
//                         its own slice of the global u64 counts with plain loads and stores: no two workgroups write
//                         the same word, there are no global atomics;
//   joint_moments_kernel  one thread per entry of sum and cross walks the staged columns in sample order and carries
//                         its sum across calls in global memory, as the summary's batch sums are done.
// No float atomics, contraction off.
#pragma once

#include <hip/hip_runtime.h>

#include "pt_summary.h"

namespace apemost {

constexpr int kJointThreads = 256;
constexpr int kJointMaxBins = 512;
constexpr int kJointBandCounters = 16384;          // u32 counters of one band in LDS (64 KiB)
constexpr int kJointGatherPer = 2048;              // values of one column per gather workgroup
constexpr unsigned short kJointNoBin = 0xffff;
constexpr int kJointMomentThreads = 64;

// whole a-rows of one band
__host__ __device__ inline int joint_band_rows(int nbins) {
    const int r = kJointBandCounters / nbins;
    return r < nbins ? r : nbins;
}

struct JointArgs {
    const double *rows;                    // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, n_keep;
    const int *chains;                     // [n_keep]
    unsigned long long skip, thin;         // kept steps of this chunk: skip, skip + thin, ... (n of them)
    unsigned int n;                        // kept steps of this chunk, 1 .. chunk
    unsigned long long chunk;              // capacity of one staged column
    int nbins, n_pairs;
    const int *pairs;                      // [n_pairs][2]
    const double *lo, *hi;                 // [n_par]
    double *vals;                          // [n_keep][n_par][chunk]
    unsigned short *bins;                  // [n_keep][n_par][chunk]
    int first;                             // this chunk holds the first sample ever accumulated: it sets the origin
    unsigned long long *counts;            // [n_keep][n_pairs][nbins][nbins]
    double *origin, *sum, *cross;          // [n_keep][n_par], [n_keep][n_par], [n_keep][n_par (n_par + 1) / 2]
};

// grid (ceil(n / kJointGatherPer), n_keep * n_par): consecutive threads write consecutive slots of one column
__global__ void __launch_bounds__(kJointThreads) joint_gather_kernel(JointArgs a) {
#pragma clang fp contract(off)
    __shared__ double edges[kJointMaxBins + 1];
    const int t = threadIdx.x;
    const int kp = blockIdx.y, k = kp / a.n_par, p = kp - k * a.n_par;
    const double lo = a.lo[p], hi = a.hi[p];
    for (int b = t; b <= a.nbins; b += kJointThreads)
        edges[b] = summary_edge(lo, hi, b, a.nbins);
    __syncthreads();
    const size_t row = (size_t)a.n_chains * (a.n_par + 2);
    const double *src = a.rows + a.skip * row + (size_t)a.chains[k] * (a.n_par + 2) + p;
    const size_t stride = (size_t)a.thin * row;
    double *vals = a.vals + (size_t)kp * a.chunk;
    unsigned short *bins = a.bins + (size_t)kp * a.chunk;
    const unsigned int i0 = blockIdx.x * (unsigned int)kJointGatherPer;
    for (unsigned int r = t; r < (unsigned int)kJointGatherPer; r += kJointThreads) {
        const unsigned int i = i0 + r;
        if (i >= a.n)
            break;
        const double v = src[i * stride];
        const int b = summary_bin(v, edges, a.nbins);
        vals[i] = v;
        bins[i] = b < 0 ? kJointNoBin : (unsigned short)b;
        if (a.first && i == 0)
            a.origin[kp] = v;
    }
}

// grid (n_bands, n_pairs, n_keep)
__global__ void __launch_bounds__(kJointThreads) joint_pair_kernel(JointArgs a) {
    __shared__ unsigned int cell[kJointBandCounters];
    const int t = threadIdx.x;
    const int q = blockIdx.y, k = blockIdx.z;
    const int nbins = a.nbins, band_rows = joint_band_rows(nbins);
    const int a0 = blockIdx.x * band_rows;                       // the band holds rows a0 .. a0 + rows - 1
    const int rows = nbins - a0 < band_rows ? nbins - a0 : band_rows;
    const int cells = rows * nbins;                              // <= kJointBandCounters
    for (int c = t; c < cells; c += kJointThreads)
        cell[c] = 0;
    __syncthreads();
    const unsigned short *bi = a.bins + ((size_t)k * a.n_par + a.pairs[2 * q]) * a.chunk;
    const unsigned short *bj = a.bins + ((size_t)k * a.n_par + a.pairs[2 * q + 1]) * a.chunk;
    for (unsigned int i = t; i < a.n; i += kJointThreads) {
        const unsigned int ba = bi[i], bb = bj[i];
        const unsigned int r = ba - (unsigned int)a0;            // (no bin: 0xffff - a0 >= 0xffff - 511 > rows)
        if (r < (unsigned int)rows && bb != kJointNoBin)
            atomicAdd(&cell[r * nbins + bb], 1u);
    }
    __syncthreads();
    unsigned long long *out = a.counts + (((size_t)k * a.n_pairs + q) * nbins + a0) * nbins;
    for (int c = t; c < cells; c += kJointThreads) {
        const unsigned int add = cell[c];
        if (add)
            out[c] += add; // this workgroup's slice alone
    }
}

// grid (ceil(n_keep * (n_par + n_par (n_par + 1) / 2) / kJointMomentThreads)): entry e of kept chain k is sum[e] for
// e < n_par, then the upper triangle of cross, row-major
__global__ void __launch_bounds__(kJointMomentThreads) joint_moments_kernel(JointArgs a) {
#pragma clang fp contract(off)
    const int np = a.n_par, tri = np * (np + 1) / 2, per = np + tri;
    const int g = blockIdx.x * kJointMomentThreads + threadIdx.x;
    if (g >= a.n_keep * per)
        return;
    const int k = g / per, e = g - k * per;
    const double *vals = a.vals + (size_t)k * np * a.chunk;
    const double *origin = a.origin + (size_t)k * np;
    if (e < np) {
        const double *v = vals + (size_t)e * a.chunk;
        const double o = origin[e];
        double s = a.sum[(size_t)k * np + e];
#pragma unroll 8
        for (unsigned int i = 0; i < a.n; i++)
            s += v[i] - o;
        a.sum[(size_t)k * np + e] = s;
        return;
    }
    int i = 0, at = e - np; // row i of the triangle holds np - i entries
    while (at >= np - i) {
        at -= np - i;
        i++;
    }
    const int j = i + at;
    const double *vi = vals + (size_t)i * a.chunk, *vj = vals + (size_t)j * a.chunk;
    const double oi = origin[i], oj = origin[j];
    double s = a.cross[(size_t)k * tri + (e - np)];
#pragma unroll 8
    for (unsigned int m = 0; m < a.n; m++) {
        const double prod = (vi[m] - oi) * (vj[m] - oj);
        s += prod;
    }
    a.cross[(size_t)k * tri + (e - np)] = s;
}

} // namespace apemost
