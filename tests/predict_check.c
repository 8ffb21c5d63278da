/* The C host's predict.bin reader and writer and predict.txt (apemost_amd/host/src/run_predict.c) with a main of their
 * own: predict_check <predict.bin> <curves: y[n_x] then best[n_x], raw doubles> <predict.txt> <copy.bin>.  Built by
 * tests/test_predict_cpu.py under the address and undefined-behaviour sanitizers; no device. */
#include "run_predict.h"

#include <stdio.h>
#include <stdlib.h>

int main(int argc, char **argv) {
    run_predict r;
    double *curves;
    FILE *f;
    if (argc != 5 || run_predict_read(argv[1], &r) != 0)
        return 2;
    curves = (double *)calloc(2 * (size_t)r.n_x, sizeof(double));
    f = fopen(argv[2], "rb");
    if (curves == NULL || f == NULL || fread(curves, sizeof(double), 2 * (size_t)r.n_x, f) != 2 * (size_t)r.n_x)
        return 3;
    fclose(f);
    run_predict_write_text(argv[3], &r, curves, curves + r.n_x);
    run_predict_write(argv[4], &r);
    free(curves);
    run_predict_free(&r);
    return 0;
}
