// Host build of the rule's helpers of apemost_amd/csrc/pt_check.h (tests/test_check_cpu.py), under the address and
// undefined-behaviour sanitizers: check_fit_term, check_extreme_term, check_serial_terms, check_sum, check_extreme,
// check_slot and check_moment_step, written for the host compiler.  Reads blocks from the file named on the command
// line, one per line: the word "s" (a sine model) or "p" (a pulse model), then L values of e and L values of u as
// hexadecimal bit patterns of doubles separated by blanks.  Prints the bit patterns of FIT, EXTREME and SERIAL of every
// block, one block per line.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "pt_check.h"

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
        std::string word;
        if (!(words >> word))
            continue;
        const bool sine = word == "s";
        std::vector<double> v;
        while (words >> word) {
            const uint64_t b = std::stoull(word, nullptr, 16);
            double d;
            std::memcpy(&d, &b, sizeof d);
            v.push_back(d);
        }
        if (v.empty() || v.size() % 2)
            return 4;
        const int L = (int)(v.size() / 2);
        const double *e = v.data(), *u = v.data() + L;
        std::vector<double> fit(L), ext(L), a(L), g(L);
        for (int i = 0; i < L; i++) {
            fit[i] = check_fit_term(e[i], sine);
            ext[i] = check_extreme_term(e[i], sine);
            a[i] = u[i] - 0.5;
        }
        check_serial_terms(a.data(), L, g.data());
        printf("%016" PRIx64 " %016" PRIx64 " %016" PRIx64 "\n", bits(check_sum(fit.data(), L)), bits(check_extreme(ext.data(), L)),
               bits(check_sum(g.data(), L)));
    }
    // the slot of a statistic: the number of edges at or below it, the last slot for a NaN
    const double edges[3] = {-1.0, 0.0, 2.5};
    if (check_slot(-2.0, edges, 3) != 0 || check_slot(-1.0, edges, 3) != 1 || check_slot(-0.0, edges, 3) != 2 ||
        check_slot(2.4, edges, 3) != 2 || check_slot(2.5, edges, 3) != 3 || check_slot(INFINITY, edges, 3) != 3 ||
        check_slot(-INFINITY, edges, 3) != 0 || check_slot(NAN, edges, 3) != 4 || check_slot(1.0, edges, 0) != 0 ||
        check_slot(NAN, edges, 0) != 1)
        return 5;
    double sum = 0.0, sq = 0.0;
    check_moment_step(3.5, 1.5, sum, sq);
    check_moment_step(0.5, 1.5, sum, sq);
    if (sum != 1.0 || sq != 5.0)
        return 6;
    // samples side by side and rows per wave: the sine models one by one
    if (check_side(APEMOST_MODEL_SIMPLESIN) != 1 || check_side(APEMOST_MODEL_PULSE) != 4 ||
        check_rows(APEMOST_MODEL_SINE3, 10) != 1 || check_rows(APEMOST_MODEL_PULSE, 6) != 4 ||
        check_rows(APEMOST_MODEL_PULSE, 129) != 3 || check_rows(APEMOST_MODEL_PULSE, kPointwiseTile) != 1)
        return 7;
    return 0;
}
