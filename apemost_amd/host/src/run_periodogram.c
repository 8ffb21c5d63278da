/* periodogram.bin reader and writer, periodogram.txt, the frequency grid and the Lomb-Scargle weights of the
 * APEMOST_DUMP token `periodogram` (run_periodogram.h).  No device and no chain is needed here. */
#include "run_periodogram.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count, size) run_alloc_or_die(count, size, "periodogram")
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "periodogram file")

#define RUN_PERIODOGRAM_MAGIC "APEMOSTG"
#define RUN_PERIODOGRAM_VERSION 1
#define RUN_PERIODOGRAM_SINGULAR 1e-10 /* SINGULAR of apemost_amd/periodogram.py */

static int finite_value(double v) {
    return v - v == 0.0; /* (C90 has no isfinite) */
}

void run_periodogram_grid_from_env(double *lo, double *hi, uint32_t *n) {
    const char *e = getenv("APEMOST_PERIODOGRAM_FREQS");
    char *end;
    long count = 0;
    int ok = e != NULL && *e != 0;
    if (ok) {
        *lo = strtod(e, &end);
        ok = end != e && *end == ':';
    }
    if (ok) {
        e = end + 1;
        *hi = strtod(e, &end);
        ok = end != e && *end == ':';
    }
    if (ok) {
        e = end + 1;
        count = strtol(e, &end, 10);
        ok = end != e && *end == 0 && count >= 1 && count <= RUN_PERIODOGRAM_MAX_FREQ && finite_value(*lo) &&
             finite_value(*hi) && *lo <= *hi;
    }
    if (!ok) {
        fprintf(stderr, "APEMOST_DUMP=periodogram needs APEMOST_PERIODOGRAM_FREQS=lo:hi:n, n frequencies in 1 .. %d from lo "
                        "to hi, lo <= hi both finite; got '%s'\n", RUN_PERIODOGRAM_MAX_FREQ,
                getenv("APEMOST_PERIODOGRAM_FREQS") != NULL ? getenv("APEMOST_PERIODOGRAM_FREQS") : "");
        exit(1);
    }
    *n = (uint32_t)count;
}

void run_periodogram_alloc(run_periodogram *r) {
    const size_t nf = r->n_freq;
    int q;
    r->freqs = (double *)alloc_or_die(nf, sizeof(double));
    r->weights = (double *)alloc_or_die(3 * nf, sizeof(double));
    for (q = 0; q < RUN_PERIODOGRAM_WORDS; q++)
        r->state[q] = (double *)alloc_or_die(nf, sizeof(double));
    r->exceed = (uint64_t *)alloc_or_die(nf, sizeof(uint64_t));
    r->peak_counts = (uint64_t *)alloc_or_die(nf + 1, sizeof(uint64_t));
}

void run_periodogram_free(run_periodogram *r) {
    int q;
    free(r->freqs);
    free(r->weights);
    for (q = 0; q < RUN_PERIODOGRAM_WORDS; q++)
        free(r->state[q]);
    free(r->exceed);
    free(r->peak_counts);
    memset(r, 0, sizeof *r);
}

void run_periodogram_grid(double lo, double hi, uint32_t n, double *freqs) {
    const double step = n > 1 ? (hi - lo) / (double)(n - 1) : 0.0;
    uint32_t j;
    for (j = 0; j < n; j++)
        freqs[j] = lo + (double)j * step;
}

void run_periodogram_weights(const double *x, uint32_t n_data, const double *freqs, uint32_t n_freq, double sigma,
                             double *weights) {
    const double two_pi = 2.0 * 3.14159265358979323846264338328, scale = 2.0 * sigma * sigma;
    uint32_t i, j;
    for (j = 0; j < n_freq; j++) {
        double cc = 0.0, cs = 0.0, ss = 0.0, det, half;
        for (i = 0; i < n_data; i++) {
            const double arg = two_pi * (freqs[j] * x[i]), c = cos(arg), s = sin(arg);
            cc += c * c;
            cs += c * s;
            ss += s * s;
        }
        det = cc * ss - cs * cs;
        half = 0.5 * (cc + ss);
        if (det > RUN_PERIODOGRAM_SINGULAR * (half * half)) {
            weights[3 * j] = ss / det / scale;
            weights[3 * j + 1] = 2.0 * (-cs / det) / scale;
            weights[3 * j + 2] = cc / det / scale;
        } else
            weights[3 * j] = weights[3 * j + 1] = weights[3 * j + 2] = 0.0;
    }
}

int run_periodogram_read(const char *path, run_periodogram *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[8];
    uint64_t u64[2];
    int32_t length;
    int q;
    if (f == NULL)
        return -1;
    memset(r, 0, sizeof *r);
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 8, f, path);
    read_or_die(u64, sizeof(uint64_t), 2, f, path);
    if (memcmp(magic, RUN_PERIODOGRAM_MAGIC, 8) != 0 || u32[0] != RUN_PERIODOGRAM_VERSION) {
        fprintf(stderr, "%s: not a periodogram file of version %d\n", path, RUN_PERIODOGRAM_VERSION);
        exit(1);
    }
    if (u32[1] != 1) {
        fclose(f);
        return 1;
    }
    r->n_freq = u32[2];
    r->model = u32[4];
    r->n = u64[0];
    r->thin = u64[1];
    read_or_die(&r->sigma, sizeof(double), 1, f, path);
    read_or_die(&r->chain, sizeof(int32_t), 1, f, path);
    read_or_die(&length, sizeof(int32_t), 1, f, path);
    r->n_data = (uint32_t)length;
    run_periodogram_alloc(r);
    read_or_die(r->freqs, sizeof(double), r->n_freq, f, path);
    read_or_die(r->weights, sizeof(double), 3 * (size_t)r->n_freq, f, path);
    read_or_die(&r->level, sizeof(double), 1, f, path);
    for (q = 0; q < RUN_PERIODOGRAM_WORDS; q++)
        read_or_die(r->state[q], sizeof(double), r->n_freq, f, path);
    read_or_die(r->exceed, sizeof(uint64_t), r->n_freq, f, path);
    read_or_die(r->peak, sizeof(double), RUN_PERIODOGRAM_PEAK_WORDS, f, path);
    read_or_die(r->peak_counts, sizeof(uint64_t), (size_t)r->n_freq + 1, f, path);
    fclose(f);
    return 0;
}

void run_periodogram_write(const char *path, const run_periodogram *r) {
    FILE *f = run_open_or_die(path, "wb");
    const size_t nf = r->n_freq;
    const int32_t length = (int32_t)r->n_data;
    uint32_t u32[8];
    uint64_t u64[2];
    int q;
    u32[0] = RUN_PERIODOGRAM_VERSION;
    u32[1] = 1;
    u32[2] = r->n_freq;
    u32[3] = 1;
    u32[4] = r->model;
    u32[5] = u32[6] = u32[7] = 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    fwrite(RUN_PERIODOGRAM_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 8, f);
    fwrite(u64, sizeof(uint64_t), 2, f);
    fwrite(&r->sigma, sizeof(double), 1, f);
    fwrite(&r->chain, sizeof(int32_t), 1, f);
    fwrite(&length, sizeof(int32_t), 1, f);
    fwrite(r->freqs, sizeof(double), nf, f);
    fwrite(r->weights, sizeof(double), 3 * nf, f);
    fwrite(&r->level, sizeof(double), 1, f);
    for (q = 0; q < RUN_PERIODOGRAM_WORDS; q++)
        fwrite(r->state[q], sizeof(double), nf, f);
    fwrite(r->exceed, sizeof(uint64_t), nf, f);
    fwrite(r->peak, sizeof(double), RUN_PERIODOGRAM_PEAK_WORDS, f);
    fwrite(r->peak_counts, sizeof(uint64_t), nf + 1, f);
    run_close_or_die(f, path);
}

/* ((wcc C) C + (wcs C) S) + (wss S) S, every operation rounded: periodogram_power of pt_periodogram.h */
static double power(const double *w, double C, double S) {
    const double a = w[0] * C, b = w[1] * C, d = w[2] * S;
    const double aa = a * C, bb = b * S, dd = d * S;
    const double ab = aa + bb;
    return ab + dd;
}

void run_periodogram_write_text(const char *path, const run_periodogram *r) {
    FILE *f = run_open_or_die(path, "w");
    const double n = (double)r->n;
    uint32_t j;
    for (j = 0; j < r->n_freq; j++) {
        const double sum = r->state[1][j], mean = r->state[0][j] + sum / n;
        double t = sum * sum, var;
        t = t / n;
        t = r->state[2][j] - t;
        var = t / (n - 1.0);
        if (var < 0)
            var = 0.0;
        run_print_values(f, 7, r->freqs[j], mean, sqrt(var), r->state[3][j], r->state[4][j],
                         power(r->weights + 3 * (size_t)j, r->state[5][j] / n, r->state[6][j] / n),
                         (double)r->peak_counts[j] / n);
        fprintf(f, "\n");
    }
    run_close_or_die(f, path);
}
