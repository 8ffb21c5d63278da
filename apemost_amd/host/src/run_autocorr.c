/* autocorr.bin reader and writer, the estimators and autocorr.txt of the APEMOST_DUMP token `autocorr`
 * (run_autocorr.h).  No device and no chain is needed here. */
#include "run_autocorr.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count, size) run_alloc_or_die(count, size, "autocorrelation")
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "autocorr file")

#define RUN_AUTOCORR_MAGIC "APEMOSTA"
#define RUN_AUTOCORR_VERSION 1

void run_autocorr_alloc(run_autocorr *r) {
    const size_t nc = r->n_cols, L = r->max_lag;
    r->cols = (int32_t *)alloc_or_die(nc, sizeof(int32_t));
    r->origin = (double *)alloc_or_die(nc, sizeof(double));
    r->sum = (double *)alloc_or_die(nc, sizeof(double));
    r->lag = (double *)alloc_or_die(nc * L, sizeof(double));
    r->head = (double *)alloc_or_die(nc * (L - 1), sizeof(double));
    r->tail = (double *)alloc_or_die(nc * (L - 1), sizeof(double));
}

void run_autocorr_free(run_autocorr *r) {
    free(r->cols);
    free(r->origin);
    free(r->sum);
    free(r->lag);
    free(r->head);
    free(r->tail);
    memset(r, 0, sizeof *r);
}

int run_autocorr_read(const char *path, run_autocorr *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[6];
    uint64_t u64[2];
    size_t nc, L;
    memset(r, 0, sizeof *r);
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 6, f, path);
    if (memcmp(magic, RUN_AUTOCORR_MAGIC, 8) != 0 || u32[0] != RUN_AUTOCORR_VERSION) {
        fprintf(stderr, "%s: not an autocorr file of version %d\n", path, RUN_AUTOCORR_VERSION);
        exit(1);
    }
    read_or_die(u64, sizeof(uint64_t), 2, f, path);
    if (u32[1] != 1 || u32[5] != 1 || u32[2] < 1 || u32[2] > 65535 || u32[3] < 1 || u32[3] > 4096) {
        fclose(f);
        return 1;
    }
    r->n_cols = u32[2];
    r->max_lag = u32[3];
    r->n_par = u32[4];
    r->n = u64[0];
    r->thin = u64[1];
    nc = r->n_cols;
    L = r->max_lag;
    run_autocorr_alloc(r);
    read_or_die(&r->chain, sizeof(int32_t), 1, f, path);
    read_or_die(r->cols, sizeof(int32_t), nc, f, path);
    read_or_die(r->origin, sizeof(double), nc, f, path);
    read_or_die(r->sum, sizeof(double), nc, f, path);
    read_or_die(r->lag, sizeof(double), nc * L, f, path);
    read_or_die(r->head, sizeof(double), nc * (L - 1), f, path);
    read_or_die(r->tail, sizeof(double), nc * (L - 1), f, path);
    fclose(f);
    return 0;
}

void run_autocorr_write(const char *path, const run_autocorr *r) {
    FILE *f = run_open_or_die(path, "wb");
    const size_t nc = r->n_cols, L = r->max_lag;
    uint32_t u32[6];
    uint64_t u64[2];
    u32[0] = RUN_AUTOCORR_VERSION;
    u32[1] = 1;
    u32[2] = r->n_cols;
    u32[3] = r->max_lag;
    u32[4] = r->n_par;
    u32[5] = 1;
    u64[0] = r->n;
    u64[1] = r->thin;
    fwrite(RUN_AUTOCORR_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 6, f);
    fwrite(u64, sizeof(uint64_t), 2, f);
    fwrite(&r->chain, sizeof(int32_t), 1, f);
    fwrite(r->cols, sizeof(int32_t), nc, f);
    fwrite(r->origin, sizeof(double), nc, f);
    fwrite(r->sum, sizeof(double), nc, f);
    fwrite(r->lag, sizeof(double), nc * L, f);
    fwrite(r->head, sizeof(double), nc * (L - 1), f);
    fwrite(r->tail, sizeof(double), nc * (L - 1), f);
    run_close_or_die(f, path);
}

/* lags that have at least one pair */
static unsigned long lags_of(const run_autocorr *r) {
    return r->n < r->max_lag ? (unsigned long)r->n : (unsigned long)r->max_lag;
}

/* Autocorr._acov of apemost_amd/autocorr.py, operation for operation:
 * acov_l = (lag_l - m (sum - first l of d) - m (sum - last l of d) + (n - l) m m) / n */
void run_autocorr_acov(const run_autocorr *r, unsigned int c, double *acov) {
    const unsigned long L = r->max_lag, H = L - 1, lags = lags_of(r);
    const double n = (double)r->n, total = r->sum[c];
    const double *lag = r->lag + (size_t)c * L, *head = r->head + (size_t)c * H, *tail = r->tail + (size_t)c * H;
    double m, first = 0.0, last = 0.0;
    unsigned long l;
    for (l = 0; l < L; l++)
        acov[l] = 0.0;
    if (r->n == 0)
        return;
    m = total / n;
    for (l = 0; l < lags; l++) {
        double a, t;
        if (l > 0) {
            first += head[l - 1];
            last += tail[H - l];
        }
        t = total - first;
        t = m * t;
        a = lag[l] - t;
        t = total - last;
        t = m * t;
        a = a - t;
        t = n - (double)l;
        t = t * m;
        t = t * m;
        a = a + t;
        acov[l] = a / n;
    }
}

double run_autocorr_tau_sokal(const run_autocorr *r, const double *acov, long *window) {
    const unsigned long lags = lags_of(r);
    const double a0 = acov[0];
    double s = 0.0, t;
    unsigned long M;
    for (M = 1; M < lags; M++) {
        s += acov[M] / a0;
        t = 2.0 * s;
        t = 1.0 + t;
        if ((double)M >= 5.0 * t) {
            *window = (long)M;
            return t;
        }
    }
    *window = -1;
    t = 2.0 * s;
    return 1.0 + t;
}

double run_autocorr_tau_geyer(const run_autocorr *r, const double *acov, long *window) {
    const unsigned long lags = lags_of(r);
    const double a0 = acov[0];
    double g = 0.0, t;
    unsigned long j = 0;
    *window = -1;
    while (2 * j + 1 < lags) {
        const double r0 = acov[2 * j] / a0, r1 = acov[2 * j + 1] / a0;
        const double G = r0 + r1;
        if (!(G > 0)) {
            *window = 2 * (long)j - 1;
            break;
        }
        g += G;
        j++;
    }
    t = 2.0 * g;
    return t - 1.0;
}

/* "%.15e", a NaN of either sign as nan */
void run_autocorr_write_text(const char *path, const run_autocorr *r, const char **names) {
    FILE *f = run_open_or_die(path, "w");
    double *acov = (double *)alloc_or_die(r->max_lag, sizeof(double));
    const double n = (double)r->n;
    unsigned int c;
    for (c = 0; c < r->n_cols; c++) {
        const uint32_t col = (uint32_t)r->cols[c];
        long window, closed;
        double mean, ts, tg, t;
        run_autocorr_acov(r, c, acov);
        t = r->sum[c] / n;
        mean = r->origin[c] + t;
        ts = run_autocorr_tau_sokal(r, acov, &window);
        tg = run_autocorr_tau_geyer(r, acov, &closed);
        if (col < r->n_par)
            fprintf(f, "%s\t", names[col]);
        else
            fprintf(f, "%s\t", col == r->n_par ? "prob" : "prob-prior");
        run_print_values(f, 3, mean, acov[0], ts);
        fprintf(f, "\t%ld\t", window);
        t = acov[0] * ts;
        t = t / n;
        run_print_values(f, 3, n / ts, sqrt(t), tg);
        fprintf(f, "\n");
    }
    free(acov);
    run_close_or_die(f, path);
}
