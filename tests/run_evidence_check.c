/* The C host's evidence.bin reader and writer and evidence.txt (apemost_amd/host/src/run_evidence.c) with a main of
 * their own: run_evidence_check <evidence.bin> <copy.bin> <evidence.txt> reads the state, writes it again and writes
 * the text.  Built by tests/test_run_folds_cpu.py without the device library, plain and under the address and
 * undefined-behaviour sanitizers; no device. */
#include "run_evidence.h"

#include <stdio.h>

int main(int argc, char **argv) {
    run_evidence r;
    uint32_t n_ladders = 0;
    if (argc != 4) {
        fprintf(stderr, "usage: %s evidence.bin copy.bin evidence.txt\n", argv[0]);
        return 2;
    }
    if (run_evidence_read(argv[1], &r, &n_ladders) != 0 || n_ladders != 1) {
        fprintf(stderr, "%s: not the state of one ladder\n", argv[1]);
        return 1;
    }
    run_evidence_write(argv[2], &r);
    run_evidence_write_text(argv[3], &r);
    run_evidence_free(&r);
    return 0;
}
