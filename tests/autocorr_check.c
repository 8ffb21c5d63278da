/* Stand-alone check of the C host's autocorrelation writer (apemost_amd/host/src/run_autocorr.c), without a device:
 *   autocorr_check <autocorr.bin> <autocorr.txt> <again.bin> <name>...
 * reads the state, writes the text file from it and the state again.  tests/test_autocorr_cpu.py builds it with the
 * address and undefined-behaviour sanitizers and compares the files with what apemost_amd/autocorr.py writes. */
#include "run_autocorr.h"

#include <stdio.h>

int main(int argc, char **argv) {
    run_autocorr r;
    if (argc < 4) {
        fprintf(stderr, "usage: %s autocorr.bin autocorr.txt again.bin name...\n", argv[0]);
        return 2;
    }
    if (run_autocorr_read(argv[1], &r) != 0) {
        fprintf(stderr, "%s: not the state of one kept chain\n", argv[1]);
        return 1;
    }
    if ((unsigned int)(argc - 4) < r.n_par) {
        fprintf(stderr, "%u parameter names are needed\n", (unsigned int)r.n_par);
        return 2;
    }
    run_autocorr_write_text(argv[2], &r, (const char **)(argv + 4));
    run_autocorr_write(argv[3], &r);
    run_autocorr_free(&r);
    return 0;
}
