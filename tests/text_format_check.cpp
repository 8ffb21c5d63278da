// Host driver of tests/test_text_format.py: apemost_amd/csrc/pt_text.h's formatter against glibc's snprintf, in
// the two conversions of the text sink ("%.15e\n" and "%6e\t%6e\n"), over the value sets the test names.
// Prints one line per set: "<set> <values> <mismatches>", then the first mismatches.
#include "pt_text.h"

#include <cfloat>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace apemost;

static uint64_t splitmix(uint64_t &s) {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

static double from_bits(uint64_t b) {
    double d;
    std::memcpy(&d, &b, 8);
    return d;
}

static uint64_t to_bits(double d) {
    uint64_t b;
    std::memcpy(&b, &d, 8);
    return b;
}

static std::mutex report_lock;
static int reported = 0;

// both lines of value v (the prob line pairs it with w); returns the number of mismatching lines
static int check(double v, double w) {
    char mine[64], ref[64];
    int bad = 0;
    int n = text_param_line(mine, v);
    int m = std::snprintf(ref, sizeof ref, "%.15e\n", v);
    if (n != m || std::memcmp(mine, ref, n) != 0) {
        bad++;
        std::lock_guard<std::mutex> g(report_lock);
        if (reported++ < 20)
            std::printf("MISMATCH %%.15e bits %016llx: mine '%.*s' libc '%.*s'\n", (unsigned long long)to_bits(v), n - 1,
                        mine, m - 1, ref);
    }
    n = text_prob_line(mine, v, w);
    m = std::snprintf(ref, sizeof ref, "%6e\t%6e\n", v, w);
    if (n != m || std::memcmp(mine, ref, n) != 0) {
        bad++;
        std::lock_guard<std::mutex> g(report_lock);
        if (reported++ < 20)
            std::printf("MISMATCH %%6e bits %016llx %016llx: mine '%.*s' libc '%.*s'\n", (unsigned long long)to_bits(v),
                        (unsigned long long)to_bits(w), n - 1, mine, m - 1, ref);
    }
    return bad;
}

// checks every value of vs (each paired with its neighbour in the list) on a few threads
static void run_set(const char *name, const std::vector<double> &vs) {
    const int n_threads = 8;
    std::vector<long> bad(n_threads, 0);
    std::vector<std::thread> pool;
    for (int t = 0; t < n_threads; t++)
        pool.emplace_back([&, t] {
            for (size_t i = t; i < vs.size(); i += n_threads)
                bad[t] += check(vs[i], vs[(i + 1) % vs.size()]);
        });
    for (auto &th : pool)
        th.join();
    long total = 0;
    for (long b : bad)
        total += b;
    std::printf("%s %zu %ld\n", name, vs.size(), total);
}

// the neighbours of x: k steps of nextafter each way (and x)
static void around(std::vector<double> &out, double x, int k) {
    double lo = x, hi = x;
    out.push_back(x);
    for (int i = 0; i < k; i++) {
        lo = std::nextafter(lo, -INFINITY);
        hi = std::nextafter(hi, INFINITY);
        out.push_back(lo);
        out.push_back(hi);
    }
}

int main(int argc, char **argv) {
    const long n_random = argc > 1 ? std::atol(argv[1]) : 10000000;
    const long n_typical = argc > 2 ? std::atol(argv[2]) : 1000000;
    uint64_t seed = 20261016;

    std::vector<double> vs;
    for (long i = 0; i < n_random; i++)
        vs.push_back(from_bits(splitmix(seed)));
    run_set("random_bits", vs);

    // what sample rows hold: parameters of order 1e-6 .. 1e6, log-likelihoods of order -1e7 .. 0
    vs.clear();
    for (long i = 0; i < n_typical; i++) {
        const double u = (double)(splitmix(seed) >> 11) / 9007199254740992.0;
        const int e = (int)(splitmix(seed) % 13) - 6;
        const double sign = splitmix(seed) & 1 ? -1.0 : 1.0;
        vs.push_back(sign * u * std::pow(10.0, e));
        vs.push_back(-u * std::pow(10.0, (int)(splitmix(seed) % 8)));
    }
    run_set("typical", vs);

    vs.clear();
    for (int k = -1074; k <= 1023; k++) {
        around(vs, std::ldexp(1.0, k), 1);
        around(vs, -std::ldexp(1.0, k), 1);
    }
    run_set("powers_of_two", vs);

    vs.clear();
    for (int k = -323; k <= 308; k++) {
        char s[32];
        std::snprintf(s, sizeof s, "1e%d", k);
        around(vs, std::strtod(s, nullptr), 2);
    }
    run_set("powers_of_ten", vs);

    // decimal half-way points of 7 and 16 significant digits: the nearest doubles and their neighbours
    vs.clear();
    for (int digits : {7, 16})
        for (int i = 0; i < 100000; i++) {
            std::string s = std::to_string(1 + splitmix(seed) % 9) + ".";
            for (int d = 1; d < digits; d++)
                s += (char)('0' + splitmix(seed) % 10);
            s += "5e" + std::to_string((int)(splitmix(seed) % 600) - 300);
            around(vs, std::strtod(s.c_str(), nullptr), 2);
        }
    run_set("near_halfway", vs);

    // exact ties: k 2^-j with k odd has the decimal digits of k 5^j, the last one a 5 -- a tie at 7 (16) digits
    // when k 5^j has 8 (17) digits; and integers of 8 (17) digits ending in 5, scaled by powers of ten
    vs.clear();
    for (int digits : {8, 17}) {
        const double lo10 = std::pow(10.0, digits - 1);
        for (int j = 1; j <= 22; j++) {
            const double p5 = std::pow(5.0, j);
            const uint64_t kmin = (uint64_t)std::ceil(lo10 / p5), kmax = (uint64_t)std::floor((10 * lo10 - 1) / p5);
            if (kmax < kmin || kmin >= (1ull << 53))
                continue;
            for (int i = 0; i < 400; i++) {
                uint64_t k = kmin + splitmix(seed) % (kmax - kmin + 1);
                k |= 1;
                if (k > kmax || k >= (1ull << 53))
                    continue;
                vs.push_back(std::ldexp((double)k, -j));
                vs.push_back(-std::ldexp((double)k, -j));
            }
        }
        for (int i = 0; i < 4000; i++) {
            uint64_t k = (uint64_t)lo10 + splitmix(seed) % (uint64_t)(9 * lo10);
            k = k / 10 * 10 + 5;
            for (uint64_t scale = 1; k * scale < (1ull << 53); scale *= 10)
                vs.push_back((double)(k * scale));
        }
    }
    vs.push_back(std::ldexp(1.0, -11)); // 4.8828125e-04 -> 4.882812e-04
    vs.push_back(9.9999999e99);         // the carry moves the exponent: 1.000000e+100
    vs.push_back(9.9999995e99);
    vs.push_back(9.99999999999999999e-100);
    run_set("exact_ties", vs);

    vs.clear();
    for (double x : {0.0, -0.0, (double)INFINITY, -(double)INFINITY, from_bits(0x7ff8000000000000ull),
                     from_bits(0xfff8000000000000ull), from_bits(0x7ff0000000000001ull), from_bits(0xfff0000000000001ull),
                     from_bits(0x7fffffffffffffffull), from_bits(1), from_bits(0x000fffffffffffffull),
                     from_bits(0x8000000000000001ull), DBL_MIN, -DBL_MIN, DBL_MAX, -DBL_MAX, 1.0, -1.0, 0.1, 0.5,
                     1e-5, 123456789.0, 9.5, 0.95, 1e22, 1e23})
        vs.push_back(x);
    run_set("special", vs);
    return 0;
}
