// pt_peaks.h -- on-device peaks: what the reference's peaks.exe (tools/peaks.c) computes from the text dump of one
// chain's parameter, from columns kept on the device.  The tool keeps the values inside [min, max] (both ends,
// :101), sorts them (:147), starts a new "peak" wherever two sorted neighbours are more than (max - min) / 100
// apart (:151, :161-188) and reads three order statistics out of each peak (:56-80).  Every result is a selection,
// so it equals the tool's bit for bit.
//   peaks_append_kernel   gathers the kept chains' parameter columns out of the sample rows
//                         [n_steps][n_chains][n_par+2] into cols[k][p][capacity], coalesced;
//   peaks_keys_kernel     one u64 key per stored value into a scratch array padded to a power of two: the key orders
//                         like the double; what the filter drops (outside [lo, hi], NaN) and the padding get ~0;
//   peaks_sort_*          a bitonic network over all (k, p) columns at once (grid.y): tiles of 4096 keys per
//                         256-thread workgroup in LDS (32 KB) run every sub-step whose stride is below the tile,
//                         strides at or above it are global compare-exchange passes;
//   peaks_nvalues_kernel  the lower bound of ~0 in the sorted keys = the values the filter admitted;
//   peaks_cut_*           flag v[i] - v[i-1] > gap on the decoded values (contraction off), count the flags per
//                         segment with plain stores, scan the counts, write the first 99 cut positions;
//   peaks_select_kernel   the three order statistics of each of the first 99 peaks, where they exist.
// No floating-point atomics, plain vector loads and stores.  The stored columns are only read.
// The key transform, the gap and its test and the three index counts are host/device inline functions, so that the
// host compiler can build them for a test (tests/peaks_check.cpp).
#pragma once

#include <hip/hip_runtime.h>

namespace apemost {

constexpr int kPeaksThreads = 256;
constexpr int kPeaksTile = 4096;    // keys of one LDS tile
constexpr int kPeaksSegment = 1024; // sorted values per cut-count segment
constexpr int kPeaksMax = 99;       // peaks reported per column (the tool asserts npeaks < 100)
constexpr unsigned long long kPeaksExcluded = ~0ull; // the image of a NaN pattern: no admitted value has it

// the u64 that orders like the double: negative values have all bits flipped, the others the sign bit set
__host__ __device__ inline unsigned long long peaks_key_of_bits(unsigned long long bits) {
    return bits ^ ((bits >> 63) ? ~0ull : 1ull << 63);
}
__host__ __device__ inline unsigned long long peaks_bits_of_key(unsigned long long key) {
    return key ^ ((key >> 63) ? 1ull << 63 : ~0ull);
}
__host__ __device__ inline unsigned long long peaks_key(double v) {
    union {
        double d;
        unsigned long long u;
    } x;
    x.d = v;
    return peaks_key_of_bits(x.u);
}
__host__ __device__ inline double peaks_value(unsigned long long key) {
    union {
        double d;
        unsigned long long u;
    } x;
    x.u = peaks_bits_of_key(key);
    return x.d;
}
// tools/peaks.c:101: both ends belong to the range, NaN does not
__host__ __device__ inline bool peaks_admits(double v, double lo, double hi) { return v >= lo && v <= hi; }
// tools/peaks.c:151
__host__ __device__ inline double peaks_gap(double lo, double hi) { return (hi - lo) / 100; }
// tools/peaks.c:167: a new peak starts at `cur` (strictly more than the gap; the subtraction as written)
__host__ __device__ inline bool peaks_splits(double prev, double cur, double gap) {
#pragma clang fp contract(off)
    const double d = cur - prev;
    return d > gap;
}
// tools/peaks.c:67-75: how many of a peak's n values lie at or below its left quartile, median, right quartile;
// the statistic is v[left + count - 1] and does not exist when count is 0
__host__ __device__ inline unsigned long long peaks_index_count(unsigned long long n, int which) {
    return n * (unsigned long long)(which + 1) / 4;
}

struct PeaksAppendArgs {
    const double *rows; // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, n_keep;
    const int *chains;  // [n_keep]
    unsigned long long skip, thin, n_kept; // kept steps of this call: skip, skip + thin, ... (n_kept of them)
    double *cols;       // [n_keep][n_par][capacity]
    unsigned long long capacity, n; // samples stored before this call
};

// grid (ceil(n_kept / 256), n_keep * n_par): consecutive threads write consecutive slots of one column
__global__ void __launch_bounds__(kPeaksThreads) peaks_append_kernel(PeaksAppendArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kPeaksThreads + threadIdx.x;
    if (i >= a.n_kept)
        return;
    const int kp = blockIdx.y, k = kp / a.n_par, p = kp - k * a.n_par;
    const size_t row = (size_t)a.n_chains * (a.n_par + 2);
    a.cols[(size_t)kp * a.capacity + a.n + i] = a.rows[(a.skip + i * a.thin) * row + (size_t)a.chains[k] * (a.n_par + 2) + p];
}

struct PeaksArgs {
    const double *cols;             // [n_cols][capacity]
    unsigned long long capacity, n; // stored per column
    unsigned long long padded;      // power of two, >= max(n, kPeaksTile)
    int n_par;
    const double *lo, *hi;          // [n_par]
    unsigned long long *keys;       // [n_cols][padded]
    unsigned long long n_segments;  // ceil(n / kPeaksSegment)
    unsigned int *seg_count;        // [n_cols][n_segments] flags of each segment
    unsigned long long *seg_off;    // [n_cols][n_segments] exclusive scan of seg_count
    // results, one slice per column
    unsigned long long *n_values;   // [n_cols]
    unsigned int *n_peaks;          // [n_cols]
    unsigned long long *cuts;       // [n_cols][kPeaksMax]: sorted index at which peak c + 1 starts
    unsigned long long *left, *right; // [n_cols][kPeaksMax]
    double *q;                      // [n_cols][kPeaksMax][3]
    unsigned char *q_set;           // [n_cols][kPeaksMax]
};

// grid (padded / 256, n_cols)
__global__ void __launch_bounds__(kPeaksThreads) peaks_keys_kernel(PeaksArgs a) {
    const unsigned long long i = (unsigned long long)blockIdx.x * kPeaksThreads + threadIdx.x;
    if (i >= a.padded)
        return;
    const int col = blockIdx.y, p = col % a.n_par;
    unsigned long long key = kPeaksExcluded;
    if (i < a.n) {
        const double v = a.cols[(size_t)col * a.capacity + i];
        if (peaks_admits(v, a.lo[p], a.hi[p]))
            key = peaks_key(v);
    }
    a.keys[(size_t)col * a.padded + i] = key;
}

// Bitonic network over `padded` keys: for k = 2, 4, ..., padded and j = k/2, ..., 1 element i meets i ^ j, ascending
// where (i & k) == 0.  Pair q of a sub-step with stride j: the lower index has q's bits with a 0 inserted at bit j.
__device__ inline unsigned long long peaks_pair_low(unsigned long long q, unsigned long long j) {
    return ((q & ~(j - 1)) << 1) | (q & (j - 1));
}

// The sub-steps with stride below the tile of the stages k_first, 2 k_first, ..., k_last, on one tile in LDS.
// grid (padded / kPeaksTile, n_cols).  (k_first = 2, k_last = tile: the tile sorted from scratch; k_first = k_last
// = k > tile: the tail of stage k behind its global passes.)
__global__ void __launch_bounds__(kPeaksThreads)
peaks_sort_tile_kernel(unsigned long long *keys, unsigned long long padded, unsigned long long k_first,
                       unsigned long long k_last) {
    __shared__ unsigned long long sh[kPeaksTile];
    const int t = threadIdx.x;
    const unsigned long long base = (unsigned long long)blockIdx.x * kPeaksTile;
    unsigned long long *g = keys + (size_t)blockIdx.y * padded + base;
    for (int i = t; i < kPeaksTile; i += kPeaksThreads)
        sh[i] = g[i];
    __syncthreads();
    for (unsigned long long k = k_first; k <= k_last; k <<= 1) {
        for (unsigned int j = k / 2 < (unsigned long long)kPeaksTile / 2 ? (unsigned int)(k / 2) : kPeaksTile / 2; j >= 1;
             j >>= 1) {
            for (unsigned int q = t; q < kPeaksTile / 2; q += kPeaksThreads) {
                const unsigned int i = (unsigned int)peaks_pair_low(q, j);
                const unsigned long long x = sh[i], y = sh[i | j];
                const bool ascending = ((base + i) & k) == 0;
                if ((x > y) == ascending) {
                    sh[i] = y;
                    sh[i | j] = x;
                }
            }
            __syncthreads();
        }
    }
    for (int i = t; i < kPeaksTile; i += kPeaksThreads)
        g[i] = sh[i];
}

// one sub-step with stride j >= tile of stage k.  grid (padded / 2 / 256, n_cols)
__global__ void __launch_bounds__(kPeaksThreads)
peaks_sort_global_kernel(unsigned long long *keys, unsigned long long padded, unsigned long long k, unsigned long long j) {
    const unsigned long long q = (unsigned long long)blockIdx.x * kPeaksThreads + threadIdx.x;
    if (q >= padded / 2)
        return;
    unsigned long long *g = keys + (size_t)blockIdx.y * padded;
    const unsigned long long i = peaks_pair_low(q, j);
    const unsigned long long x = g[i], y = g[i | j];
    const bool ascending = (i & k) == 0;
    if ((x > y) == ascending) {
        g[i] = y;
        g[i | j] = x;
    }
}

// grid (ceil(n_cols / 256)): one thread per column bisects for the first excluded key
__global__ void __launch_bounds__(kPeaksThreads) peaks_nvalues_kernel(PeaksArgs a, int n_cols) {
    const int col = blockIdx.x * kPeaksThreads + threadIdx.x;
    if (col >= n_cols)
        return;
    const unsigned long long *g = a.keys + (size_t)col * a.padded;
    unsigned long long lo = 0, hi = a.n; // the first excluded key lies in [lo, hi]
    while (lo < hi) {
        const unsigned long long mid = lo + (hi - lo) / 2;
        if (g[mid] == kPeaksExcluded)
            hi = mid;
        else
            lo = mid + 1;
    }
    a.n_values[col] = lo;
}

// a peak starts at sorted index i > 0 (both keys admitted: the excluded ones sort behind every value)
__device__ inline bool peaks_cut_at(const unsigned long long *g, unsigned long long i, double gap) {
    const unsigned long long key = g[i];
    return key != kPeaksExcluded && peaks_splits(peaks_value(g[i - 1]), peaks_value(key), gap);
}

// grid (n_segments, n_cols): the flags of one segment of kPeaksSegment sorted values, counted in LDS (integer
// atomics) and stored by one thread
__global__ void __launch_bounds__(kPeaksThreads) peaks_cut_count_kernel(PeaksArgs a) {
    __shared__ unsigned int count;
    const int col = blockIdx.y;
    const unsigned long long *g = a.keys + (size_t)col * a.padded;
    const int p = col % a.n_par;
    const double gap = peaks_gap(a.lo[p], a.hi[p]);
    if (threadIdx.x == 0)
        count = 0;
    __syncthreads();
    const unsigned long long first = (unsigned long long)blockIdx.x * kPeaksSegment;
    unsigned int mine = 0;
    for (int r = threadIdx.x; r < kPeaksSegment; r += kPeaksThreads) {
        const unsigned long long i = first + r;
        if (i > 0 && i < a.n && peaks_cut_at(g, i, gap))
            mine++;
    }
    if (mine)
        atomicAdd(&count, mine);
    __syncthreads();
    if (threadIdx.x == 0)
        a.seg_count[(size_t)col * a.n_segments + blockIdx.x] = count;
}

// grid (n_cols): exclusive scan of the column's segment counts; the total gives the number of peaks
__global__ void __launch_bounds__(kPeaksThreads) peaks_cut_scan_kernel(PeaksArgs a) {
    __shared__ unsigned long long sh[kPeaksThreads];
    const int t = threadIdx.x, col = blockIdx.x;
    const unsigned int *cnt = a.seg_count + (size_t)col * a.n_segments;
    unsigned long long *off = a.seg_off + (size_t)col * a.n_segments;
    unsigned long long carry = 0;
    for (unsigned long long b0 = 0; b0 < a.n_segments; b0 += kPeaksThreads) {
        const unsigned long long b = b0 + t;
        const unsigned long long v = b < a.n_segments ? cnt[b] : 0;
        sh[t] = v;
        __syncthreads();
        for (int d = 1; d < kPeaksThreads; d <<= 1) {
            const unsigned long long add = t >= d ? sh[t - d] : 0;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        if (b < a.n_segments)
            off[b] = carry + sh[t] - v;
        carry += sh[kPeaksThreads - 1];
        __syncthreads(); // sh is rewritten by the next chunk
    }
    if (t == 0) {
        const unsigned long long peaks = a.n_values[col] > 0 ? carry + 1 : 0;
        a.n_peaks[col] = peaks > 0xffffffffull ? 0xffffffffu : (unsigned int)peaks;
    }
}

// grid (ceil(n_segments / 256), n_cols): one thread per segment; the few that hold one of the first kPeaksMax cuts
// walk their segment in order and write the positions
__global__ void __launch_bounds__(kPeaksThreads) peaks_cut_write_kernel(PeaksArgs a) {
    const unsigned long long seg = (unsigned long long)blockIdx.x * kPeaksThreads + threadIdx.x;
    if (seg >= a.n_segments)
        return;
    const int col = blockIdx.y;
    const size_t at = (size_t)col * a.n_segments + seg;
    unsigned long long pos = a.seg_off[at];
    if (a.seg_count[at] == 0 || pos >= (unsigned long long)kPeaksMax)
        return;
    const unsigned long long *g = a.keys + (size_t)col * a.padded;
    const int p = col % a.n_par;
    const double gap = peaks_gap(a.lo[p], a.hi[p]);
    const unsigned long long first = seg * kPeaksSegment;
    for (unsigned long long i = first; i < first + kPeaksSegment && i < a.n && pos < (unsigned long long)kPeaksMax; i++)
        if (i > 0 && peaks_cut_at(g, i, gap))
            a.cuts[(size_t)col * kPeaksMax + pos++] = i;
}

// grid (n_cols), 128 threads: thread c takes peak c of the first kPeaksMax
__global__ void __launch_bounds__(128) peaks_select_kernel(PeaksArgs a) {
    const int col = blockIdx.x, c = threadIdx.x;
    const unsigned int n_peaks = a.n_peaks[col];
    if (c >= kPeaksMax || (unsigned int)c >= n_peaks)
        return;
    const unsigned long long *g = a.keys + (size_t)col * a.padded;
    const unsigned long long *cuts = a.cuts + (size_t)col * kPeaksMax;
    const unsigned long long left = c == 0 ? 0 : cuts[c - 1];
    const unsigned long long right = (unsigned int)c + 1 == n_peaks ? a.n_values[col] - 1 : cuts[c] - 1;
    const unsigned long long n = right - left + 1;
    const size_t at = (size_t)col * kPeaksMax + c;
    a.left[at] = left;
    a.right[at] = right;
    unsigned char set = 0;
    for (int j = 0; j < 3; j++) {
        const unsigned long long count = peaks_index_count(n, j);
        double v = 0;
        if (count >= 1) {
            v = peaks_value(g[left + count - 1]);
            set |= (unsigned char)(1 << j);
        }
        a.q[at * 3 + j] = v;
    }
    a.q_set[at] = set;
}

} // namespace apemost
