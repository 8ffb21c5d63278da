// pt_text.h -- the reference's text sample dumps, formatted on the device.
//
// The C host's text sink writes two conversions (apemost_amd/host/src/parallel_tempering.c):
//   <name>-chain-<i>.prob.dump   "%.15e\n"      one line per parameter per step (16 significant digits)
//   prob-chain<i>.dump           "%6e\t%6e\n"   one line per chain per step: prob, prob - prior (7 digits)
// text_format_e() prints one double exactly as glibc's printf does for "%*.*e": the decimal digits of the
// exact binary value rounded half to even, "-" for the sign bit (of zero and NaN too), "inf"/"nan",
// exponents of at least two digits.  Integer arithmetic only, no floating-point operation anywhere: the
// value v = m 2^e is scaled to q = floor(v / 10^s) with one or two guard digits and a sticky bit (the
// remainder is not zero), and the guard digits and the sticky bit decide the rounding.  Computing q:
//   fast paths  m 10^t / 2^k with m 10^t below 2^128 (t <= 22), or (m 2^f) / 5^s in 64 bits (s <= 27):
//               every value between about 1e-6 and 1e19 takes one of them;
//   exact path  the same quotient with a big integer of 32-bit limbs (the very small and very large values;
//               its cost grows with the binary exponent).
// All three are exact; the fast ones only avoid the limb loops.  The powers of five live in __constant__.
//
// The kernels turn sample rows [n_steps][n_chains][n_par+2] (kept steps skip, skip + thin, ...) into byte
// streams, in this order:
//   streams 0 .. n_param_chains*n_par - 1    parameter p of chain c is stream c*n_par + p   ("%.15e\n")
//   stream n_param_chains*n_par + c          prob-chain<c>, for every chain c of the sampler ("%6e\t%6e\n")
// Line l = stream * n_kept + k (kept step k), so the streams lie one after the other in one output and
// stream i is out[offsets[i], offsets[i+1]).  Three launches, all deterministic:
//   text_format_kernel   one line per thread into a fixed 32-byte slot, its length, a sum per workgroup;
//   text_scan_kernel     one workgroup: exclusive scan of the workgroup sums, and the total;
//   text_compact_kernel  the workgroup's scan of the lengths, every line copied to its place, and
//                        offsets[i] written by the thread that holds stream i's first line.
// No atomics, no floating-point work, plain stores.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace apemost {

constexpr int kTextSlot = 32;       // bytes per formatted line before compaction
constexpr int kTextParamLine = 24;  // the longest "%.15e\n": "-1.234567890123456e-308\n"
constexpr int kTextProbLine = 30;   // the longest "%6e\t%6e\n": "-1.234567e-308\t-1.234567e-308\n"
constexpr int kTextThreads = 256;
constexpr int kTextScanThreads = 1024;

#define APEMOST_TEXT_POW5                                                                                        \
    {1ull, 5ull, 25ull, 125ull, 625ull, 3125ull, 15625ull, 78125ull, 390625ull, 1953125ull, 9765625ull,          \
     48828125ull, 244140625ull, 1220703125ull, 6103515625ull, 30517578125ull, 152587890625ull, 762939453125ull,  \
     3814697265625ull, 19073486328125ull, 95367431640625ull, 476837158203125ull, 2384185791015625ull,             \
     11920928955078125ull, 59604644775390625ull, 298023223876953125ull, 1490116119384765625ull,                  \
     7450580596923828125ull}
__constant__ const uint64_t kTextPow5Device[28] = APEMOST_TEXT_POW5;
static constexpr uint64_t kTextPow5Host[28] = APEMOST_TEXT_POW5;
#undef APEMOST_TEXT_POW5

// 5^k, k in [0, 27]
__host__ __device__ inline uint64_t text_pow5(int k) {
#if defined(__HIP_DEVICE_COMPILE__)
    return kTextPow5Device[k];
#else
    return kTextPow5Host[k];
#endif
}

// 10^k, k in [0, 19]
__host__ __device__ inline uint64_t text_pow10(int k) { return text_pow5(k) << k; }

// floor(log10(2^b)) for b in [-1100, 1100]
__host__ __device__ inline int text_floor_log10_pow2(int b) { return (b * 78913) >> 18; }

// ---- the exact path: unsigned big integers of 32-bit limbs, least significant first ----
constexpr int kTextLimbs = 40; // m 10^t for t <= 342 has at most 1190 bits, m 2^f for f < 1000 at most 1053

struct TextBig {
    uint32_t w[kTextLimbs];
    int n; // limbs in use
};

__host__ __device__ inline uint32_t text_big_limb(const TextBig &a, int i) { return i >= 0 && i < a.n ? a.w[i] : 0; }

__host__ __device__ inline void text_big_set(TextBig &a, uint64_t m) {
    a.w[0] = (uint32_t)m;
    a.w[1] = (uint32_t)(m >> 32);
    a.n = a.w[1] ? 2 : 1;
}

// a *= f
__host__ __device__ inline void text_big_mul(TextBig &a, uint32_t f) {
    uint64_t carry = 0;
    for (int i = 0; i < a.n; i++) {
        const uint64_t p = (uint64_t)a.w[i] * f + carry;
        a.w[i] = (uint32_t)p;
        carry = p >> 32;
    }
    if (carry)
        a.w[a.n++] = (uint32_t)carry;
}

// a = floor(a / d); returns the remainder
__host__ __device__ inline uint32_t text_big_div(TextBig &a, uint32_t d) {
    uint64_t rem = 0;
    for (int i = a.n - 1; i >= 0; i--) {
        const uint64_t cur = (rem << 32) | a.w[i];
        a.w[i] = (uint32_t)(cur / d);
        rem = cur % d;
    }
    while (a.n > 1 && a.w[a.n - 1] == 0)
        a.n--;
    return (uint32_t)rem;
}

// a <<= k
__host__ __device__ inline void text_big_shl(TextBig &a, int k) {
    const int words = k >> 5, bits = k & 31;
    const int n = a.n + words + 1;
    for (int i = n - 1; i >= 0; i--) { // reads limbs at or below i only: not yet overwritten
        const uint32_t hi = text_big_limb(a, i - words), lo = text_big_limb(a, i - words - 1);
        a.w[i] = bits ? (hi << bits) | (lo >> (32 - bits)) : hi;
    }
    a.n = n;
    while (a.n > 1 && a.w[a.n - 1] == 0)
        a.n--;
}

// floor(a / 2^k), which the caller knows to fit in 64 bits; sticky |= any bit below k is set
__host__ __device__ inline uint64_t text_big_shr64(const TextBig &a, int k, bool &sticky) {
    const int words = k >> 5, bits = k & 31;
    for (int i = 0; i < words && i < a.n; i++)
        sticky |= a.w[i] != 0;
    if (bits)
        sticky |= (text_big_limb(a, words) & ((1u << bits) - 1)) != 0;
    const uint64_t lo = (uint64_t)text_big_limb(a, words) | (uint64_t)text_big_limb(a, words + 1) << 32;
    if (bits == 0)
        return lo;
    return (lo >> bits) | (uint64_t)text_big_limb(a, words + 2) << (64 - bits);
}

// floor(m 2^e / 10^s), sticky |= the remainder is not zero.  The caller picks s so that the quotient
// lies in [10, 10^19).
__host__ __device__ inline uint64_t text_scaled(uint64_t m, int e, int s, bool &sticky) {
    if (s <= 0) {
        const int t = -s;
        if (e >= 0) // v >= 2^52, so t <= 2: an integer product
            return (m * text_pow10(t)) << e;
        const int k = -e;
        if (t <= 22) {
            unsigned __int128 p = (unsigned __int128)m * text_pow10(t < 19 ? t : 19);
            if (t > 19)
                p *= text_pow10(t - 19);
            // p < 2^127 and the quotient is at least 10, so k < 124
            sticky |= (p & (((unsigned __int128)1 << k) - 1)) != 0;
            return (uint64_t)(p >> k);
        }
        TextBig a;
        text_big_set(a, m);
        int r = t;
        for (; r >= 9; r -= 9)
            text_big_mul(a, 1000000000u);
        if (r > 0)
            text_big_mul(a, (uint32_t)text_pow10(r));
        return text_big_shr64(a, k, sticky);
    }
    // v / 10^s = (m 2^f) / 5^s with f = e - s
    const int f = e - s;
    if (f <= 11 && s <= 27) {
        uint64_t x;
        if (f >= 0) {
            x = m << f;
        } else if (f > -64) {
            sticky |= (m & ((1ull << -f) - 1)) != 0;
            x = m >> -f;
        } else {
            sticky |= m != 0;
            x = 0;
        }
        const uint64_t d = text_pow5(s);
        sticky |= x % d != 0;
        return x / d;
    }
    // here f > 11: s > 27 means v >= 10^34, where f = e - s exceeds 30
    TextBig a;
    text_big_set(a, m);
    text_big_shl(a, f);
    int r = s;
    for (; r >= 13; r -= 13)
        sticky |= text_big_div(a, 1220703125u) != 0; // 5^13
    if (r > 0)
        sticky |= text_big_div(a, (uint32_t)text_pow5(r)) != 0;
    return (uint64_t)text_big_limb(a, 0) | (uint64_t)text_big_limb(a, 1) << 32;
}

// the n significant digits of m 2^e (m > 0) rounded half to even: returns them as an integer in
// [10^(n-1), 10^n) and the decimal exponent of the first one in exp10.  n in [1, 17].
__host__ __device__ inline uint64_t text_digits(uint64_t m, int e, int n, int &exp10) {
    const int b = 63 - __builtin_clzll(m) + e; // floor(log2 v)
    const int e0 = text_floor_log10_pow2(b);   // floor(log10 v) is e0 or e0 + 1
    bool sticky = false;
    // n + 1 digits when floor(log10 v) == e0, else n + 2: one or two guard digits
    const uint64_t q = text_scaled(m, e, e0 - n, sticky);
    const bool wide = q >= text_pow10(n + 1);
    const uint64_t div = wide ? 100 : 10, half = div / 2;
    uint64_t d = q / div;
    const uint64_t r = q - d * div;
    exp10 = e0 + (wide ? 1 : 0);
    if (r > half || (r == half && (sticky || (d & 1))))
        d++;
    if (d == text_pow10(n)) { // the carry ran through every digit
        d = text_pow10(n - 1);
        exp10++;
    }
    return d;
}

// writes x as printf("%*.*e", width, prec, x) does, prec in [0, 16]; returns the length (no terminator).
// o must hold max(width, prec + 10) bytes.
__host__ __device__ inline int text_format_e(char *o, double x, int prec, int width) {
    const uint64_t bits = __builtin_bit_cast(uint64_t, x);
    const bool neg = bits >> 63;
    const int bexp = (int)((bits >> 52) & 0x7ff);
    const uint64_t frac = bits & ((1ull << 52) - 1);
    int len = 0;
    if (bexp == 0x7ff) {
        for (const int body = neg ? 4 : 3; len < width - body; len++)
            o[len] = ' ';
        if (neg)
            o[len++] = '-';
        o[len++] = frac ? 'n' : 'i';
        o[len++] = frac ? 'a' : 'n';
        o[len++] = frac ? 'n' : 'f';
        return len;
    }
    if (neg)
        o[len++] = '-';
    uint64_t d = 0;
    int ex = 0;
    if (bexp != 0 || frac != 0) {
        const uint64_t m = bexp ? frac | (1ull << 52) : frac;
        const int e = bexp ? bexp - 1075 : -1074;
        d = text_digits(m, e, prec + 1, ex);
    }
    // digit j (0 = the leading one) goes to o[len + (j ? j + 1 : 0)], behind the point; the low 8 digits
    // come from lo, the others from hi
    const int nd = prec + 1;
    uint32_t hi = (uint32_t)(d / 100000000u), lo = (uint32_t)(d % 100000000u);
    for (int j = nd - 1; j >= 0; j--) {
        uint32_t &part = nd - 1 - j < 8 ? lo : hi;
        o[len + (j ? j + 1 : 0)] = (char)('0' + part % 10);
        part /= 10;
    }
    if (prec > 0)
        o[len + 1] = '.';
    len += prec > 0 ? nd + 1 : nd;
    o[len++] = 'e';
    o[len++] = ex < 0 ? '-' : '+';
    const int ae = ex < 0 ? -ex : ex;
    if (ae >= 100)
        o[len++] = (char)('0' + ae / 100);
    o[len++] = (char)('0' + ae / 10 % 10);
    o[len++] = (char)('0' + ae % 10);
    return len;
}

// one line of a parameter file: "%.15e\n"
__host__ __device__ inline int text_param_line(char *o, double v) {
    int n = text_format_e(o, v, 15, 0);
    o[n++] = '\n';
    return n;
}

// one line of a prob-chain file: "%6e\t%6e\n"
__host__ __device__ inline int text_prob_line(char *o, double prob, double rel) {
    int n = text_format_e(o, prob, 6, 6);
    o[n++] = '\t';
    n += text_format_e(o + n, rel, 6, 6);
    o[n++] = '\n';
    return n;
}

// ---- kernels ----
struct TextArgs {
    const double *rows;                   // [n_steps][n_chains][n_par+2]
    int n_chains, n_par, n_param_chains;
    unsigned long long skip, thin, n_kept; // kept steps skip, skip + thin, ... (n_kept >= 1 of them)
    unsigned long long n_lines;           // n_kept * n_streams
    unsigned long long n_tiles;           // workgroups of kTextThreads lines
    char *slots;                          // [n_lines][kTextSlot]
    unsigned char *lens;                  // [n_lines]
    unsigned long long *tile_sum;         // [n_tiles]: bytes of workgroup b's lines
    unsigned long long *tile_off;         // [n_tiles]: exclusive scan of tile_sum
    char *out;                            // the streams, one after the other
    unsigned long long *offsets;          // [n_streams + 1]
};

// exclusive scan of one value per thread over a workgroup of kTextThreads; the total goes to *total
__device__ inline unsigned int text_block_scan(unsigned int v, unsigned int *sh, unsigned int *total) {
    const int t = threadIdx.x;
    sh[t] = v;
    __syncthreads();
    for (int d = 1; d < kTextThreads; d <<= 1) {
        const unsigned int add = t >= d ? sh[t - d] : 0;
        __syncthreads();
        sh[t] += add;
        __syncthreads();
    }
    *total = sh[kTextThreads - 1];
    return sh[t] - v;
}

__global__ void __launch_bounds__(kTextThreads) text_format_kernel(TextArgs a) {
    __shared__ unsigned int sh[kTextThreads];
    const unsigned long long l = (unsigned long long)blockIdx.x * kTextThreads + threadIdx.x;
    unsigned int len = 0;
    if (l < a.n_lines) {
        const unsigned long long stream = l / a.n_kept, k = l - stream * a.n_kept;
        const size_t row = (size_t)a.n_chains * (a.n_par + 2);
        const double *r = a.rows + (a.skip + k * a.thin) * row;
        char *o = a.slots + l * kTextSlot;
        const unsigned long long n_head = (unsigned long long)a.n_param_chains * a.n_par;
        if (stream < n_head) {
            const unsigned long long c = stream / a.n_par, p = stream - c * a.n_par;
            len = (unsigned int)text_param_line(o, r[c * (a.n_par + 2) + p]);
        } else {
            const double *q = r + (stream - n_head) * (a.n_par + 2) + a.n_par;
            len = (unsigned int)text_prob_line(o, q[0], q[1]);
        }
        a.lens[l] = (unsigned char)len;
    }
    unsigned int total;
    text_block_scan(len, sh, &total);
    if (threadIdx.x == 0)
        a.tile_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kTextScanThreads) text_scan_kernel(TextArgs a, unsigned long long n_streams) {
    __shared__ unsigned long long sh[kTextScanThreads];
    const int t = threadIdx.x;
    unsigned long long carry = 0;
    for (unsigned long long b0 = 0; b0 < a.n_tiles; b0 += kTextScanThreads) {
        const unsigned long long b = b0 + t;
        const unsigned long long v = b < a.n_tiles ? a.tile_sum[b] : 0;
        sh[t] = v;
        __syncthreads();
        for (int d = 1; d < kTextScanThreads; d <<= 1) {
            const unsigned long long add = t >= d ? sh[t - d] : 0;
            __syncthreads();
            sh[t] += add;
            __syncthreads();
        }
        if (b < a.n_tiles)
            a.tile_off[b] = carry + sh[t] - v;
        carry += sh[kTextScanThreads - 1];
        __syncthreads(); // sh is rewritten by the next chunk
    }
    if (t == 0)
        a.offsets[n_streams] = carry;
}

__global__ void __launch_bounds__(kTextThreads) text_compact_kernel(TextArgs a) {
    __shared__ unsigned int sh[kTextThreads];
    const unsigned long long l = (unsigned long long)blockIdx.x * kTextThreads + threadIdx.x;
    const unsigned int len = l < a.n_lines ? a.lens[l] : 0;
    unsigned int total;
    const unsigned int pre = text_block_scan(len, sh, &total);
    if (l >= a.n_lines)
        return;
    const unsigned long long pos = a.tile_off[blockIdx.x] + pre;
    const char *src = a.slots + l * kTextSlot;
    char *dst = a.out + pos;
    for (unsigned int i = 0; i < len; i++)
        dst[i] = src[i];
    const unsigned long long stream = l / a.n_kept;
    if (l == stream * a.n_kept)
        a.offsets[stream] = pos;
}

} // namespace apemost
