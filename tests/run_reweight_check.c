/* The C host's reweight.bin reader and writer, reweight.txt and the environment of the token `reweight`
 * (apemost_amd/host/src/run_reweight.c) with a main of their own: run_reweight_check <reweight.bin> <copy.bin>
 * <reweight.txt> [name ...] reads the sums, writes them again and writes the text, with the names given or col<index>;
 * it prints the bins and the targets the environment asks for.  Built by tests/test_run_reweight_cpu.py without the
 * device library, plain and under the address and undefined-behaviour sanitizers. */
#include "run_reweight.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
    run_reweight r;
    double betas[RUN_REWEIGHT_MAX_TARGETS];
    unsigned int n_t, t;
    if (argc < 4) {
        fprintf(stderr, "usage: run_reweight_check reweight.bin copy.bin reweight.txt [name ...]\n");
        return 2;
    }
    printf("%u bins;", run_reweight_bins_from_env());
    n_t = run_reweight_betas_from_env(betas);
    for (t = 0; t < n_t; t++)
        printf(" %.17g", betas[t]);
    printf("\n");
    if (run_reweight_read(argv[1], &r) != 0) {
        fprintf(stderr, "%s: no such file\n", argv[1]);
        return 1;
    }
    if (argc > 4 && (unsigned int)(argc - 4) != r.n_cols) {
        fprintf(stderr, "%d names for %lu columns\n", argc - 4, (unsigned long)r.n_cols);
        return 1;
    }
    run_reweight_write(argv[2], &r);
    run_reweight_write_text(argv[3], &r, argc > 4 ? (const char *const *)(argv + 4) : NULL);
    run_reweight_free(&r);
    return 0;
}
