// Host build of the inline helpers of apemost_amd/csrc/pt_peaks.h (tests/test_peaks_cpu.py): the key that orders
// like the double, its inverse, the gap test and the index counts.  Prints "<set> <checked> <mismatches>" per set
// and "count <n> <n/4> <n*2/4> <n*3/4>" for n = 1 .. 10000; the test reads both.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "pt_peaks.h"

using namespace apemost;

static double from_bits(uint64_t u) {
    double d;
    memcpy(&d, &u, sizeof d);
    return d;
}
static uint64_t to_bits(double d) {
    uint64_t u;
    memcpy(&u, &d, sizeof u);
    return u;
}

static uint64_t rng_state = 0x9e3779b97f4a7c15ull;
static uint64_t next64() { // splitmix64
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the keys of a and b compare as a and b do; -0.0 sorts before +0.0, which compare equal as numbers
static int order_mismatch(double a, double b) {
    const unsigned long long ka = peaks_key(a), kb = peaks_key(b);
    if (a < b)
        return !(ka < kb);
    if (a > b)
        return !(ka > kb);
    if (to_bits(a) == to_bits(b))
        return ka != kb;
    return !((std::signbit(a) ? ka < kb : ka > kb)); // the two zeros
}

int main() {
    const int N = 1000000;
    std::vector<uint64_t> bits;
    bits.reserve(N + 64);
    for (int i = 0; i < N; i++)
        bits.push_back(next64());
    const double inf = std::numeric_limits<double>::infinity(), mx = std::numeric_limits<double>::max(),
                 mn = std::numeric_limits<double>::min(), den = std::numeric_limits<double>::denorm_min();
    const double special[] = {inf, -inf, mx, -mx, mn, -mn, den, -den, 2 * den, -2 * den, mn - den, -(mn - den), 0.0, -0.0,
                              1.0, -1.0, std::nextafter(1.0, 2.0), std::nextafter(-1.0, -2.0), 12.000000000000002, 11.0};
    for (double d : special)
        bits.push_back(to_bits(d));

    // the inverse round-trips on every pattern, NaN patterns included
    long bad = 0;
    for (uint64_t u : bits)
        bad += peaks_bits_of_key(peaks_key_of_bits(u)) != u || to_bits(peaks_value(peaks_key(from_bits(u)))) != u;
    printf("round_trip %zu %ld\n", bits.size(), bad);

    // only NaN patterns may have the key of the excluded values
    std::vector<double> vals;
    bad = 0;
    for (uint64_t u : bits) {
        const double d = from_bits(u);
        if (d != d)
            continue;
        vals.push_back(d);
        bad += peaks_key(d) == kPeaksExcluded;
    }
    bad += peaks_key_of_bits(0x7fffffffffffffffull) != kPeaksExcluded;
    printf("excluded_key %zu %ld\n", vals.size(), bad);

    // sorted by key they are sorted as numbers, and neighbours compare as their keys do
    std::vector<double> by_key(vals);
    std::sort(by_key.begin(), by_key.end(), [](double a, double b) { return peaks_key(a) < peaks_key(b); });
    bad = 0;
    for (size_t i = 1; i < by_key.size(); i++)
        bad += !(by_key[i - 1] <= by_key[i]) || order_mismatch(by_key[i - 1], by_key[i]);
    printf("sorted_by_key %zu %ld\n", by_key.size(), bad);

    // random pairs, and every pair of the special values
    bad = 0;
    for (size_t i = 0; i + 1 < vals.size(); i += 2)
        bad += order_mismatch(vals[i], vals[i + 1]);
    size_t pairs = vals.size() / 2;
    for (double a : special)
        for (double b : special) {
            bad += order_mismatch(a, b);
            pairs++;
        }
    printf("pair_order %zu %ld\n", pairs, bad);

    // the filter and the gap test (tools/peaks.c:101, :151, :167)
    bad = 0;
    bad += peaks_gap(0.0, 100.0) != 1.0;
    bad += peaks_splits(10.0, 11.0, 1.0) != false;
    bad += peaks_splits(11.0, 12.000000000000002, 1.0) != true;
    bad += peaks_splits(1.0, 1.0, 0.5) != false;
    bad += !peaks_admits(0.0, 0.0, 1.0) || !peaks_admits(1.0, 0.0, 1.0) || peaks_admits(std::nextafter(1.0, 2.0), 0.0, 1.0) ||
           peaks_admits(-den, 0.0, 1.0) || peaks_admits(std::nan(""), 0.0, 1.0) || peaks_admits(inf, 0.0, 1.0);
    printf("filter_and_gap 10 %ld\n", bad);

    for (unsigned long long n = 1; n <= 10000; n++)
        printf("count %llu %llu %llu %llu\n", n, peaks_index_count(n, 0), peaks_index_count(n, 1), peaks_index_count(n, 2));
    return 0;
}
