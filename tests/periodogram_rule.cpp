// Host build of the rule's helpers of apemost_amd/csrc/pt_periodogram.h (tests/test_periodogram_cpu.py), under the
// address and undefined-behaviour sanitizers: periodogram_sums, periodogram_power, periodogram_peak and
// periodogram_extremes_step, written for the host compiler.  Reads blocks from the file named on the command line, one
// per line: L and n_freq in decimal, then as hexadecimal bit patterns of doubles separated by blanks r [L], c [n_freq][L],
// s [n_freq][L] and w [n_freq][3].  Prints per block one line: the bit patterns of C [n_freq], S [n_freq], P [n_freq] and
// of the highest peak, then arg in decimal.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "pt_periodogram.h"

using namespace apemost;

static uint64_t bits(double v) {
    uint64_t out;
    std::memcpy(&out, &v, sizeof out);
    return out;
}

int main(int argc, char **argv) {
    if (argc != 2)
        return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f)
        return 3;
    std::string text;
    char buf[4096];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, f)) > 0)
        text.append(buf, got);
    fclose(f);
    std::istringstream lines(text);
    std::string line;
    while (std::getline(lines, line)) {
        std::istringstream words(line);
        int L = 0, n_freq = 0;
        if (!(words >> L >> n_freq))
            continue;
        if (L < 1 || n_freq < 1)
            return 4;
        std::vector<double> v;
        std::string word;
        while (words >> word) {
            const uint64_t b = std::stoull(word, nullptr, 16);
            double d;
            std::memcpy(&d, &b, sizeof d);
            v.push_back(d);
        }
        const size_t nl = (size_t)L, nf = (size_t)n_freq;
        if (v.size() != nl + 2 * nf * nl + 3 * nf)
            return 5;
        const double *r = v.data(), *c = r + nl, *s = c + nf * nl, *w = s + nf * nl;
        std::vector<double> C(nf), S(nf), P(nf);
        for (size_t j = 0; j < nf; j++) {
            periodogram_sums(r, c + j * nl, s + j * nl, L, C[j], S[j]);
            P[j] = periodogram_power(w[3 * j], w[3 * j + 1], w[3 * j + 2], C[j], S[j]);
        }
        double m;
        int arg;
        periodogram_peak(P.data(), n_freq, m, arg);
        for (const std::vector<double> *a : {&C, &S, &P})
            for (size_t j = 0; j < nf; j++)
                printf("%016" PRIx64 " ", bits((*a)[j]));
        printf("%016" PRIx64 " %d\n", bits(m), arg);
    }
    // the extremes: strict comparisons, a NaN is skipped
    double mn = INFINITY, mx = -INFINITY;
    for (double p : {2.0, (double)NAN, -1.0, 2.0, 0.5})
        periodogram_extremes_step(p, mn, mx);
    if (mn != -1.0 || mx != 2.0)
        return 6;
    mn = INFINITY, mx = -INFINITY;
    periodogram_extremes_step(NAN, mn, mx);
    if (mn != INFINITY || mx != -INFINITY)
        return 7;
    // the constants the Python side repeats
    if (kPeriodogramPiece != APEMOST_PERIODOGRAM_PIECE || kPeriodogramMaxFreq != APEMOST_PERIODOGRAM_MAX_FREQ ||
        !periodogram_has_residual(APEMOST_MODEL_SIMPLESIN) || !periodogram_has_residual(APEMOST_MODEL_SINE3) ||
        periodogram_has_residual(APEMOST_MODEL_PULSE) || periodogram_has_residual(APEMOST_MODEL_PULSE_VROT) ||
        periodogram_has_residual(APEMOST_MODEL_USER))
        return 8;
    return 0;
}
