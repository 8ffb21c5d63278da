/* The C host's pointwise_tail.bin reader and writer (apemost_amd/host/src/run_pointwise.c) with a main of their own:
 * `pointwise_tail_check in.bin out.bin` reads the one and writes the other; `pointwise_tail_check capacity N` prints
 * run_pointwise_tail_capacity_for(N).  Built and run by tests/test_pointwise_tail_cpu.py under the address and
 * undefined-behaviour sanitizers; no device.  Exit status 2 + what run_pointwise_tail_read returned where that is not 0. */
#include "run_pointwise.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

int main(int argc, char **argv) {
    run_pointwise_tail t;
    int rc;
    if (argc != 3)
        return 2;
    if (strcmp(argv[1], "capacity") == 0) {
        printf("%lu\n", (unsigned long)run_pointwise_tail_capacity_for((uint64_t)strtoul(argv[2], NULL, 10)));
        return 0;
    }
    rc = run_pointwise_tail_read(argv[1], &t);
    if (rc != 0)
        return 3 + rc;
    run_pointwise_tail_write(argv[2], &t);
    run_pointwise_tail_free(&t);
    return 0;
}
