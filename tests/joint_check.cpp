// Host build of the summation helpers of apemost_amd/csrc/pt_pointwise_joint.h (tests/test_kfold_cpu.py), under the
// address and undefined-behaviour sanitizers: joint_lane_partials and joint_tree_sum, the rule of J written for the
// host compiler.  Reads blocks of terms from the file named on the command line, one block per line as hexadecimal bit
// patterns of doubles separated by blanks, and prints the bit pattern of J of every block, one per line.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "pt_pointwise_joint.h"

using namespace apemost;

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
        std::vector<double> terms;
        std::string word;
        while (words >> word) {
            const uint64_t bits = std::stoull(word, nullptr, 16);
            double v;
            std::memcpy(&v, &bits, sizeof v);
            terms.push_back(v);
        }
        if (terms.empty())
            continue;
        double p[kPointwiseWave];
        joint_lane_partials(terms.data(), (int)terms.size(), p);
        const double J = joint_tree_sum(p);
        uint64_t out;
        std::memcpy(&out, &J, sizeof out);
        printf("%016" PRIx64 "\n", out);
    }
    // rows of a wave of the sum kernel: what fits the tile, between 1 and kJointSide
    if (joint_rows(1) != kJointSide || joint_rows(128) != 4 || joint_rows(129) != 3 || joint_rows(256) != 2 ||
        joint_rows(257) != 1 || joint_rows(kPointwiseTile) != 1)
        return 4;
    return 0;
}
