// pt_pointwise_tail.h -- the tail of a pointwise fold (pt_pointwise.h): per series s = (kept chain k, datum i) the
// `capacity` largest values of x = -l over the kept samples, exactly, kept on the device beside the fold.  This is what
// Pareto-smoothed importance-sampling leave-one-out (apemost_amd/psis.py) needs besides the fold's own m_dn and S_dn: the
// M + 1 largest leave-one-out log weights of every datum.  Like the term itself they are in no sample dump.
//
// The rule.  l is the fold's term, PointwiseTermAt<MODEL>::at (a user model: UserTermAt::at) of the same parameter row,
// so its bits are the fold's; x = -l is exact.  Values are ordered by tail_key, the peaks fold's peaks_key restated here
// (this header reaches the analysis module of a user model, which the peaks header does not): a total order on the bit
// patterns with -0 below +0; a NaN is never stored, +-inf are ordinary values.  After any number of accumulate calls
//   count[s]              = min(capacity, non-NaN samples so far),
//   values[s][0 .. count) = the count[s] largest x in that order, descending.
// A selection under a total order does not depend on where calls, pieces or compactions fall: every cut of the same
// kept samples gives the same bits.
//
// The state.  P = max(1024, capacity rounded up to a power of two); a series has a buffer of B = 2 P slots, laid out
// slot-major inside a block of 64 data, buf[k][blk][slot][lane], so that a wave whose lanes all append at the same slot
// (the warm-up, when everything is admitted) writes 512 consecutive bytes.  slots[s] says how many are filled, thr[s]
// is the threshold key: the key of the series' capacity-th largest value as of the last compaction, or 0 -- below the
// key of every value that is not NaN -- while there have not been that many.
//   pointwise_tail_append_kernel   the fold's grid without its parameter workgroup: one wave per workgroup, a lane per
//                                  datum, the kept parameter rows staged through the same LDS tile and read as
//                                  broadcasts.  A lane keeps thr and its slot count in registers and stores x where
//                                  x == x and key(x) > thr.  One launch takes at most B - capacity kept steps (the tail
//                                  piece), so a buffer that held at most `capacity` values cannot overflow; the store
//                                  is bounded by B all the same.  Once a series is full, admissions are rare: in
//                                  expectation capacity * piece / n of them per piece.
//   pointwise_tail_compact_kernel  one 256-thread workgroup per series, behind every append.  It leaves at once,
//                                  wave-uniformly, where the series holds at most `capacity` values and no sort is
//                                  forced.  Otherwise it loads the keys into LDS, pads with key 0 up to the next power
//                                  of two N (at most B = 8192 keys = 64 KiB of dynamic LDS, sized by the launch to B),
//                                  runs a descending bitonic network in LDS and writes back the largest
//                                  min(capacity, slots) values, the new slot count and the new threshold.
//                                  pointwise_tail_get forces the sort, so that a series that never filled comes out
//                                  sorted too; a forced sort changes no selection, only the order inside the buffer.
//   pointwise_tail_gather_kernel / _scatter_kernel   between the buffer and the dense [series][capacity] array of the
//                                  C interface.
// One thread owns a series in the append and one workgroup in the compaction: no atomics, plain vector loads and stores.
// The network's index arithmetic is host/device inline, so that the host compiler can build it for a test
// (tests/tail_check.cpp).
#pragma once

#include <hip/hip_runtime.h>

#include "pt_pointwise.h"

namespace apemost {

constexpr int kTailThreads = 256;
constexpr int kTailMinP = 1024;
constexpr int kTailMaxCapacity = 4096;
constexpr int kTailMaxB = 2 * kTailMaxCapacity; // 8192 keys = 64 KiB of LDS

// the u64 that orders like the double (negative values have all bits flipped, the others the sign bit set), and back
__host__ __device__ inline unsigned long long tail_key(double v) {
    union {
        double d;
        unsigned long long u;
    } x;
    x.d = v;
    return x.u ^ ((x.u >> 63) ? ~0ull : 1ull << 63);
}
__host__ __device__ inline double tail_value(unsigned long long key) {
    union {
        double d;
        unsigned long long u;
    } x;
    x.u = key ^ ((key >> 63) ? 1ull << 63 : ~0ull);
    return x.d;
}

// P of a capacity: the power of two at or above it, at least kTailMinP
__host__ __device__ inline int tail_p(int capacity) {
    int p = kTailMinP;
    while (p < capacity)
        p <<= 1;
    return p;
}
// slots of a series' buffer, and the kept steps one append launch may take
__host__ __device__ inline int tail_buffer(int capacity) { return 2 * tail_p(capacity); }
__host__ __device__ inline int tail_piece(int capacity) { return tail_buffer(capacity) - capacity; }
// where slot `slot` of lane `lane` of block `blk` (64 data) of kept chain k lies
__host__ __device__ inline size_t tail_slot_at(int k, int n_blocks, int blk, int B, int slot, int lane) {
    return (((size_t)k * n_blocks + blk) * B + slot) * 64 + lane;
}

// The bitonic network over N keys, N a power of two: for stage = 2, 4, ..., N and stride = stage/2, ..., 1 the element i
// meets i ^ stride.  Pair q of a sub-step: its lower index is q with a 0 inserted at the stride's bit.  The pair is put
// in descending order where (i & stage) == 0 and in ascending order elsewhere, which leaves the whole descending.
__host__ __device__ inline unsigned int tail_sort_size(unsigned int n) {
    unsigned int p = 2;
    while (p < n)
        p <<= 1;
    return p;
}
__host__ __device__ inline unsigned int tail_pair_low(unsigned int q, unsigned int stride) {
    return ((q & ~(stride - 1)) << 1) | (q & (stride - 1));
}
__host__ __device__ inline bool tail_pair_descending(unsigned int i, unsigned int stage) { return (i & stage) == 0; }
// one compare-exchange of the network on keys[]
__host__ __device__ inline void tail_compare_exchange(unsigned long long *keys, unsigned int q, unsigned int stride,
                                                      unsigned int stage) {
    const unsigned int i = tail_pair_low(q, stride);
    const unsigned long long a = keys[i], b = keys[i | stride];
    if ((a < b) == tail_pair_descending(i, stage)) {
        keys[i] = b;
        keys[i | stride] = a;
    }
}
// count and threshold of a series whose `slots` stored keys have been sorted descending into keys[]
__host__ __device__ inline unsigned int tail_kept(unsigned int slots, unsigned int capacity) {
    return slots < capacity ? slots : capacity;
}
__host__ __device__ inline unsigned long long tail_threshold(const unsigned long long *keys, unsigned int slots,
                                                             unsigned int capacity) {
    return slots >= capacity ? keys[capacity - 1] : 0ull;
}

struct PointwiseTailArgs {
    double *buf;             // [n_keep][n_blocks][B][64]
    unsigned int *slots;     // [n_keep][n_data] filled slots of the series' buffer
    unsigned long long *thr; // [n_keep][n_data] threshold key
    int capacity, B;
    int n_data, n_blocks;
    int force;               // the compaction sorts every series
    double *dense;           // gather / scatter: [n_keep][n_data][capacity]
    unsigned long long *count; // gather / scatter: [n_keep][n_data]
};

// a workgroup of pointwise_tail_append_kernel: grid n_blocks * n_keep, one wave each; a.n <= tail_piece(capacity)
template <class EVAL>
__device__ __forceinline__ void pointwise_tail_append_body(const PointwiseArgs &a, const PointwiseTailArgs &t) {
#pragma clang fp contract(off)
    __shared__ double tile[kPointwiseTile];
    const int lane = threadIdx.x;
    const int k = blockIdx.x / a.n_blocks, blk = blockIdx.x - k * a.n_blocks;
    const int np = a.n_par, n = (int)a.n;
    const size_t w = (size_t)np + 2, stride = (size_t)a.thin * a.n_chains * w;
    const double *src = a.rows + a.skip * a.n_chains * w + (size_t)a.chains[k] * w;
    const int i = blk * kPointwiseWave + lane;
    const bool active = i < a.n_data;
    const size_t s = (size_t)k * a.n_data + (active ? i : 0);
    EVAL ev;
    ev.init(a, k, i, s, active);
    unsigned int slots = active ? t.slots[s] : 0u;
    const unsigned long long thr = active ? t.thr[s] : 0ull;
    double *const mine = t.buf + tail_slot_at(k, a.n_blocks, blk, t.B, 0, lane);
    auto admit = [&](double x) {
        if (x == x && tail_key(x) > thr && slots < (unsigned int)t.B) {
            mine[(size_t)slots * 64] = x;
            slots++;
        }
    };
    const int per_tile = kPointwiseTile / np;
    for (int t0 = 0; t0 < n; t0 += per_tile) {
        const int cnt = n - t0 < per_tile ? n - t0 : per_tile;
        __syncthreads(); // the tile before has been read
        for (int e = lane; e < cnt * np; e += kPointwiseWave) {
            const int r = e / np, p = e - r * np;
            tile[e] = src[(size_t)(t0 + r) * stride + p];
        }
        __syncthreads();
        if (active) {
            // kPointwiseSide terms side by side, as the fold evaluates them, so that their curves are in flight
            // together; they are admitted in sample order
            int r = 0;
            for (; r + kPointwiseSide <= cnt; r += kPointwiseSide) {
                double x[kPointwiseSide];
#pragma unroll
                for (int j = 0; j < kPointwiseSide; j++)
                    x[j] = -ev.at(tile + (r + j) * np);
#pragma unroll
                for (int j = 0; j < kPointwiseSide; j++)
                    admit(x[j]);
            }
            for (; r < cnt; r++)
                admit(-ev.at(tile + r * np));
        }
    }
    if (active)
        t.slots[s] = slots;
}

template <int MODEL>
__global__ void __launch_bounds__(kPointwiseWave) pointwise_tail_append_kernel(PointwiseArgs a, PointwiseTailArgs t) {
    pointwise_tail_append_body<PointwiseTermAt<MODEL>>(a, t);
}

// grid n_keep * n_data, kTailThreads threads, t.B * 8 bytes of dynamic LDS
__global__ void __launch_bounds__(kTailThreads) pointwise_tail_compact_kernel(PointwiseTailArgs t) {
    extern __shared__ unsigned long long tail_keys[];
    const unsigned int s = blockIdx.x, tid = threadIdx.x;
    const unsigned int k = s / (unsigned int)t.n_data, i = s - k * (unsigned int)t.n_data;
    unsigned int slots = t.slots[s];
    if (slots > (unsigned int)t.B) // (never: the append is bounded)
        slots = (unsigned int)t.B;
    const unsigned int capacity = (unsigned int)t.capacity;
    if (!t.force && slots <= capacity)
        return; // the whole workgroup: slots is uniform
    double *const mine = t.buf + tail_slot_at((int)k, t.n_blocks, (int)(i / 64), t.B, 0, (int)(i % 64));
    const unsigned int N = tail_sort_size(slots); // <= B
    for (unsigned int j = tid; j < N; j += kTailThreads)
        tail_keys[j] = j < slots ? tail_key(mine[(size_t)j * 64]) : 0ull;
    __syncthreads();
    for (unsigned int stage = 2; stage <= N; stage <<= 1)
        for (unsigned int stride = stage >> 1; stride >= 1; stride >>= 1) {
            for (unsigned int q = tid; q < N / 2; q += kTailThreads)
                tail_compare_exchange(tail_keys, q, stride, stage);
            __syncthreads();
        }
    const unsigned int kept = tail_kept(slots, capacity);
    for (unsigned int j = tid; j < kept; j += kTailThreads)
        mine[(size_t)j * 64] = tail_value(tail_keys[j]);
    if (tid == 0) {
        t.slots[s] = kept;
        t.thr[s] = tail_threshold(tail_keys, slots, capacity);
    }
}

// grid (n_keep * n_data, ceil(capacity / 256)): dense[s][j] = slot j of series s (j < count), count[s] = slots[s]
__global__ void __launch_bounds__(kTailThreads) pointwise_tail_gather_kernel(PointwiseTailArgs t) {
    const unsigned int s = blockIdx.x, j = blockIdx.y * kTailThreads + threadIdx.x;
    const unsigned int k = s / (unsigned int)t.n_data, i = s - k * (unsigned int)t.n_data;
    const unsigned int kept = tail_kept(t.slots[s], (unsigned int)t.capacity);
    if (j == 0)
        t.count[s] = kept;
    if (j >= (unsigned int)t.capacity)
        return;
    t.dense[(size_t)s * t.capacity + j] =
        j < kept ? t.buf[tail_slot_at((int)k, t.n_blocks, (int)(i / 64), t.B, (int)j, (int)(i % 64))] : 0.0;
}

// the reverse; the forced compaction behind it sorts the series and sets its threshold
__global__ void __launch_bounds__(kTailThreads) pointwise_tail_scatter_kernel(PointwiseTailArgs t) {
    const unsigned int s = blockIdx.x, j = blockIdx.y * kTailThreads + threadIdx.x;
    const unsigned int k = s / (unsigned int)t.n_data, i = s - k * (unsigned int)t.n_data;
    const unsigned int kept = tail_kept((unsigned int)t.count[s], (unsigned int)t.capacity);
    if (j == 0) {
        t.slots[s] = kept;
        t.thr[s] = 0ull;
    }
    if (j < kept)
        t.buf[tail_slot_at((int)k, t.n_blocks, (int)(i / 64), t.B, (int)j, (int)(i % 64))] = t.dense[(size_t)s * t.capacity + j];
}

} // namespace apemost
