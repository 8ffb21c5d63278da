// pt_summary.h -- on-device run summary: what the `analyse` phase computes from the dump files
// (apemost_amd/host/src/analyse.c), folded from the sample rows [n_steps][n_chains][n_par+2] while they
// are still on the device.  Three running quantities, each equal bit for bit to the host loop it replaces,
// whatever the calls' boundaries are:
//   prob_sum[c]      sum of column n_par+1 (prob - prior) of chain c, `sum += v` in sample order
//                    (analyse_data_probability);
//   hist[h][p][b]    counts of chain h's parameter p in the bins of marginal_distribution(), which are those of
//                    the reference's create_hist(): GSL's gsl_histogram_set_ranges_uniform edges
//                    ((n-b)/n)*lo + (b/n)*hi, the top one widened by (hi-lo)/10000, bin b = [e[b], e[b+1]);
//   batch[h][p][k]   the batch sums of batch_means_error(): batch 0 holds bs-1 samples, every later one bs;
//                    slot n_batches holds the running sum of the batch that is still open.
// One launch per batch of rows.  Workgroups [0, n_hist*n_par) own one (h, p) each: its bins live in LDS
// (ds_add_u32) and go to its own slice of `hist` with plain loads and stores; lane 0 walks the values in
// sample order for the batch sums.  The workgroups behind them give one thread per chain for prob_sum.
// No float atomics anywhere: every sum is one thread's sequential chain, so arrival order cannot change
// a bit, and contraction is off (the edge formula's two products feed an add unfused, as on the host).
// The edges were lo + (hi-lo)*b/n before; that differs from GSL's formula by up to one ulp at about a quarter of
// the edges, so counts in a summary.bin written before this change were binned on edges up to one ulp away.
// Each histogram workgroup now computes its nbins+1 edges once per launch into LDS (32 KB more) and bisects
// them per value: ceil(log2 nbins) LDS reads and compares in place of a division, a multiply and two
// recomputed edges.
#pragma once

#include <hip/hip_runtime.h>

namespace apemost {

constexpr int kSummaryThreads = 256;
constexpr int kSummaryChunk = 1024; // values of one (h, p) staged in LDS per pass
constexpr int kSummaryMaxBins = 4096;

struct SummaryArgs {
    const double *rows;          // [n_steps][n_chains][n_par+2]
    int n_chains, n_par;
    unsigned long long skip, thin, n_kept; // kept steps of this call: skip, skip + thin, ... (n_kept of them)
    int n_hist, nbins;
    const double *lo, *hi;       // [n_par]: the histogram range of every parameter
    unsigned long long bs;       // batch size
    unsigned long long left;     // samples still to come before the open batch closes (1 .. bs)
    unsigned long long n_closed; // batches closed before this call = slot of the open batch
    double *prob_sum;            // [n_chains]
    unsigned long long *hist;    // [n_hist][n_par][nbins]
    double *batch;               // [n_hist][n_par][max_batches + 1]
    unsigned long long batch_stride; // max_batches + 1
};

// gsl_histogram_set_ranges_uniform's edge b of n over [lo, hi], the top one widened as create_hist() does
__device__ inline double summary_edge(double lo, double hi, int b, int nbins) {
#pragma clang fp contract(off)
    const double f1 = (double)(nbins - b) / (double)nbins, f2 = (double)b / (double)nbins;
    double e = f1 * lo + f2 * hi;
    if (b == nbins)
        e += (hi - lo) / 10000;
    return e;
}

// the bin of v over the edges e[0 .. nbins], or -1 when v lies outside [e[0], e[nbins]) (NaN included):
// gsl_histogram_increment's bisection, step for step as the host's (gslcompat.c).  GSL's uniform edges are not
// always sorted -- over [1e15, 1e15+3] with 200 bins six of them step back by an ulp -- and there a guess from
// the spacing followed by a walk settles in another bin than the host does; the same bisection cannot.
__device__ inline int summary_bin(double v, const double *e, int nbins) {
    if (!(v >= e[0] && v < e[nbins]))
        return -1;
    int left = 0, right = nbins;
    while (right - left > 1) { // e[left] <= v < e[right]
        const int mid = (left + right) >> 1;
        if (v >= e[mid])
            left = mid;
        else
            right = mid;
    }
    return left;
}

__global__ void __launch_bounds__(kSummaryThreads) summary_kernel(SummaryArgs a) {
#pragma clang fp contract(off)
    __shared__ unsigned int bins[kSummaryMaxBins];
    __shared__ double vals[kSummaryChunk];
    __shared__ double edges[kSummaryMaxBins + 1];
    const int t = threadIdx.x;
    const size_t row = (size_t)a.n_chains * (a.n_par + 2);
    const int hp = blockIdx.x;
    if (hp >= a.n_hist * a.n_par) {
        // one thread per chain: prob_sum[c] += v in sample order
        const int c = (hp - a.n_hist * a.n_par) * kSummaryThreads + t;
        if (c >= a.n_chains)
            return;
        const double *src = a.rows + a.skip * row + (size_t)c * (a.n_par + 2) + a.n_par + 1;
        const size_t stride = (size_t)a.thin * row;
        double s = a.prob_sum[c];
#pragma unroll 8
        for (unsigned long long k = 0; k < a.n_kept; k++)
            s += src[k * stride];
        a.prob_sum[c] = s;
        return;
    }
    const int h = hp / a.n_par, p = hp - h * a.n_par;
    const double lo = a.lo[p], hi = a.hi[p];
    for (int b = t; b < a.nbins; b += kSummaryThreads)
        bins[b] = 0;
    for (int b = t; b <= a.nbins; b += kSummaryThreads)
        edges[b] = summary_edge(lo, hi, b, a.nbins);
    const double *src = a.rows + a.skip * row + (size_t)h * (a.n_par + 2) + p;
    const size_t stride = (size_t)a.thin * row;
    double *batch = a.batch + (size_t)hp * a.batch_stride;
    unsigned long long nb = a.n_closed, left = a.left;
    double part = 0;
    if (t == 0)
        part = batch[nb];
    __syncthreads();
    for (unsigned long long k0 = 0; k0 < a.n_kept; k0 += kSummaryChunk) {
        const unsigned long long rest = a.n_kept - k0;
        const int len = rest < (unsigned long long)kSummaryChunk ? (int)rest : kSummaryChunk;
        for (int i = t; i < len; i += kSummaryThreads) {
            const double v = src[(k0 + i) * stride];
            vals[i] = v;
            const int b = summary_bin(v, edges, a.nbins);
            if (b >= 0)
                atomicAdd(&bins[b], 1u);
        }
        __syncthreads();
        if (t == 0) {
            // batch_means_error(): batchsum += v; a batch closes after its last sample
            for (int i = 0; i < len; i++) {
                part += vals[i];
                if (--left == 0) {
                    batch[nb++] = part;
                    part = 0;
                    left = a.bs;
                }
            }
        }
        __syncthreads(); // vals is rewritten by the next pass
    }
    if (t == 0)
        batch[nb] = part; // the open batch
    unsigned long long *hist = a.hist + (size_t)hp * a.nbins;
    for (int b = t; b < a.nbins; b += kSummaryThreads)
        hist[b] += bins[b]; // this workgroup's slice alone
}

} // namespace apemost
