/* The C host's pointwise.bin reader and writer, pointwise.txt and criteria.txt (apemost_amd/host/src/run_pointwise.c)
 * with a main of their own: pointwise_check <pointwise.bin> <pointwise.txt> <criteria.txt> <copy.bin>.  Built by
 * tests/test_pointwise_cpu.py under the address and undefined-behaviour sanitizers; no device. */
#include "run_pointwise.h"

int main(int argc, char **argv) {
    run_pointwise r;
    if (argc != 5 || run_pointwise_read(argv[1], &r) != 0)
        return 2;
    run_pointwise_write_text(argv[2], &r);
    run_pointwise_write_criteria(argv[3], &r);
    run_pointwise_write(argv[4], &r);
    run_pointwise_free(&r);
    return 0;
}
