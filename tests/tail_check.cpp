// Host build of the inline helpers of apemost_amd/csrc/pt_pointwise_tail.h (tests/test_pointwise_tail_cpu.py), under the
// address and undefined-behaviour sanitizers: the sizes of a capacity, the slot layout, and the bitonic network's index
// arithmetic, run exactly as pointwise_tail_compact_kernel runs it (pad with key 0 to tail_sort_size(n), every stage
// and stride, tail_compare_exchange on every pair) over every size 2 .. 8192 against std::sort of the same keys.  The
// keys include both zeros, both infinities, duplicates and runs of one value.
// Prints "<set> <checked> <mismatches>" per set; the test reads them.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <limits>
#include <vector>

#include "pt_peaks.h"
#include "pt_pointwise_tail.h"

using namespace apemost;

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next64() { // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static double draw() {
    const double inf = std::numeric_limits<double>::infinity();
    const double special[] = {0.0, -0.0, inf, -inf, 1.0, -1.0, 1.0, 5e-324, -5e-324, 1.5};
    const uint64_t r = next64();
    if (r % 4 == 0)
        return special[(r >> 8) % 10];
    if (r % 4 == 1)
        return (double)((int64_t)((r >> 8) % 9) - 4); // small integers: many duplicates
    return std::ldexp((double)(int64_t)(r >> 11), (int)((r >> 3) % 40) - 60) * ((r & 4) ? 1 : -1);
}

int main() {
    // sizes
    long checked = 0, bad = 0;
    for (int c = 2; c <= kTailMaxCapacity; c++, checked++) {
        const int p = tail_p(c), B = tail_buffer(c);
        bad += !(p >= kTailMinP && p >= c && (p & (p - 1)) == 0 && (p == kTailMinP || p / 2 < c) && B == 2 * p &&
                 B <= kTailMaxB && tail_piece(c) == B - c && tail_piece(c) >= c);
    }
    bad += !(tail_p(1024) == 1024 && tail_p(1025) == 2048 && tail_piece(8) == 2040 && tail_buffer(4096) == 8192);
    printf("sizes %ld %ld\n", checked, bad);
    // the layout: every (block, slot, lane) of a chain has a place of its own inside the chain's share
    checked = bad = 0;
    {
        const int n_blocks = 3, B = 2048;
        std::vector<unsigned char> seen((size_t)2 * n_blocks * B * 64, 0);
        for (int k = 0; k < 2; k++)
            for (int blk = 0; blk < n_blocks; blk++)
                for (int slot = 0; slot < B; slot++)
                    for (int lane = 0; lane < 64; lane++, checked++) {
                        const size_t at = tail_slot_at(k, n_blocks, blk, B, slot, lane);
                        if (at >= seen.size() || seen[at]++)
                            bad++;
                    }
        bad += !(tail_slot_at(0, n_blocks, 1, B, 5, 1) - tail_slot_at(0, n_blocks, 1, B, 5, 0) == 1 &&
                 tail_slot_at(0, n_blocks, 1, B, 6, 0) - tail_slot_at(0, n_blocks, 1, B, 5, 0) == 64);
    }
    printf("layout %ld %ld\n", checked, bad);
    // the network
    checked = bad = 0;
    long sizes = 0;
    for (unsigned int n = 2; n <= (unsigned int)kTailMaxB; n++, sizes++) {
        std::vector<unsigned long long> keys(n), want;
        for (auto &k : keys) {
            const double v = draw();
            k = tail_key(v);
            bad += k != peaks_key(v) || peaks_key(tail_value(k)) != k; // the peaks fold's key, and its inverse
        }
        if (n % 97 == 0)
            std::fill(keys.begin(), keys.end(), tail_key(-0.0)); // one value throughout
        want = keys;
        std::sort(want.begin(), want.end(), std::greater<unsigned long long>());
        const unsigned int N = tail_sort_size(n);
        if (N < n || (N & (N - 1)) || (N > 2 && N / 2 >= n)) {
            bad++;
            continue;
        }
        std::vector<unsigned long long> lds(N, 0ull);
        std::copy(keys.begin(), keys.end(), lds.begin());
        for (unsigned int stage = 2; stage <= N; stage <<= 1)
            for (unsigned int stride = stage >> 1; stride >= 1; stride >>= 1)
                for (unsigned int q = 0; q < N / 2; q++)
                    tail_compare_exchange(lds.data(), q, stride, stage);
        for (unsigned int j = 0; j < n; j++, checked++)
            bad += lds[j] != want[j];
        for (unsigned int j = n; j < N; j++)
            bad += lds[j] != 0ull; // the padding sorts behind every value
        // count and threshold as the kernel takes them, at a capacity below, at and above n
        for (unsigned int cap : {n / 2 + 1, n, n + 3}) {
            const unsigned int kept = tail_kept(n, cap);
            bad += kept != std::min(n, cap);
            bad += tail_threshold(lds.data(), n, cap) != (n >= cap ? want[cap - 1] : 0ull);
        }
    }
    printf("network %ld %ld\n", checked, bad);
    printf("network_sizes %ld 0\n", sizes);
    // the order of the keys the tests rest on
    checked = bad = 0;
    {
        const double inf = std::numeric_limits<double>::infinity();
        const double asc[] = {-inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, inf};
        for (int i = 0; i + 1 < 8; i++, checked++)
            bad += !(tail_key(asc[i]) < tail_key(asc[i + 1]) && tail_key(asc[i]) > 0ull);
    }
    printf("order %ld %ld\n", checked, bad);
    return 0;
}
