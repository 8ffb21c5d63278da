/* The C host's mbar.bin reader and writer, its solver loop and mbar.txt (apemost_amd/host/src/run_mbar.c) with a main
 * of their own: run_mbar_check <mbar.bin> <copy.bin> <solved.bin> <mbar.txt> reads a stored column, writes it again,
 * solves it with the passes in C (run_mbar_host_passes), writes the solved state and the text.  Built by
 * tests/test_run_mbar_cpu.py without the device library, plain and under the address and undefined-behaviour
 * sanitizers. */
#include "run_mbar.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
    run_mbar r;
    run_mbar_passes p;
    double change;
    long used;
    if (argc != 5) {
        fprintf(stderr, "usage: run_mbar_check mbar.bin copy.bin solved.bin mbar.txt\n");
        return 2;
    }
    if (run_mbar_read(argv[1], &r) != 0 || r.n < 1) {
        fprintf(stderr, "%s: no such file, or no samples\n", argv[1]);
        return 1;
    }
    run_mbar_write(argv[2], &r);
    if (r.n_bad != 0) {
        fprintf(stderr, "%s: %lu values that are not finite\n", argv[1], (unsigned long)r.n_bad);
        return 1;
    }
    p = run_mbar_host_passes(&r);
    run_mbar_start(&r, 0, r.n, r.g);
    used = run_mbar_solve(&r, &p, run_mbar_tol_from_env(), run_mbar_iter_from_env(), 0, r.n, r.g, &change);
    if (used < 0) {
        fprintf(stderr, "no convergence: a change of %g is left\n", change);
        return 1;
    }
    r.solved = 1;
    r.t0 = 0;
    r.t_count = r.n;
    run_mbar_write(argv[3], &r);
    run_mbar_write_text(argv[4], &r, &p, run_mbar_tol_from_env(), run_mbar_iter_from_env());
    printf("%ld iterations, change %g\n", used, change);
    run_mbar_free(&r);
    return 0;
}
