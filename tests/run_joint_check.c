/* The C host's joint.bin reader and writer, the .joint files and correlation.matrix (apemost_amd/host/src/run_joint.c)
 * with a main of their own: run_joint_check <joint.bin> <copy.bin> <name>... reads the state, writes it again and
 * writes the text files into the working directory.  Built by tests/test_run_folds_cpu.py without the device library,
 * plain and under the address and undefined-behaviour sanitizers; no device. */
#include "run_joint.h"

#include <stdio.h>

int main(int argc, char **argv) {
    run_joint r;
    uint32_t n_keep = 0, q;
    int32_t chain = -1;
    if (argc < 3) {
        fprintf(stderr, "usage: %s joint.bin copy.bin name...\n", argv[0]);
        return 2;
    }
    if (run_joint_read(argv[1], &r, &n_keep, &chain) != 0 || n_keep != 1 || chain != 0 || r.lo == NULL) {
        fprintf(stderr, "%s: not the state of kept chain 0 alone\n", argv[1]);
        return 1;
    }
    if ((unsigned int)(argc - 3) < r.n_par) {
        fprintf(stderr, "%u parameter names are needed\n", (unsigned int)r.n_par);
        return 2;
    }
    run_joint_write(argv[2], &r);
    for (q = 0; q < r.n_pairs; q++)
        run_joint_write_pair(&r, q, (const char **)(argv + 3));
    run_joint_write_correlation(&r);
    run_joint_free(&r);
    return 0;
}
