/* predict.bin reader and writer, the quantiles and predict.txt of the APEMOST_DUMP token `predict` (run_predict.h).
 * No device and no chain is needed here. */
#include "run_predict.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count, size) run_alloc_or_die(count, size, "predict")
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "predict file")

#define RUN_PREDICT_MAGIC "APEMOSTP"
#define RUN_PREDICT_VERSION 1

void run_predict_alloc(run_predict *r) {
    const size_t nx = r->n_x;
    size_t i;
    r->x = (double *)alloc_or_die(nx, sizeof(double));
    r->origin = (double *)alloc_or_die(nx, sizeof(double));
    r->sum = (double *)alloc_or_die(nx, sizeof(double));
    r->sq = (double *)alloc_or_die(nx, sizeof(double));
    r->vmin = (double *)alloc_or_die(nx, sizeof(double));
    r->vmax = (double *)alloc_or_die(nx, sizeof(double));
    r->hist = (uint64_t *)alloc_or_die(nx * r->nbins, sizeof(uint64_t));
    r->best_params = (double *)alloc_or_die(r->n_par, sizeof(double));
    for (i = 0; i < nx; i++) {
        r->vmin[i] = HUGE_VAL;
        r->vmax[i] = -HUGE_VAL;
    }
    r->best_prob = -HUGE_VAL;
    r->best_n = 0;
}

void run_predict_free(run_predict *r) {
    free(r->x);
    free(r->origin);
    free(r->sum);
    free(r->sq);
    free(r->vmin);
    free(r->vmax);
    free(r->hist);
    free(r->best_params);
    memset(r, 0, sizeof *r);
}

int run_predict_read(const char *path, run_predict *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[8];
    uint64_t u64[2];
    double range[2];
    size_t nx;
    memset(r, 0, sizeof *r);
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 8, f, path);
    if (memcmp(magic, RUN_PREDICT_MAGIC, 8) != 0 || u32[0] != RUN_PREDICT_VERSION) {
        fprintf(stderr, "%s: not a predict file of version %d\n", path, RUN_PREDICT_VERSION);
        exit(1);
    }
    read_or_die(u64, sizeof(uint64_t), 2, f, path);
    read_or_die(range, sizeof(double), 2, f, path);
    if (u32[1] != 1 || u32[5] != 1 || u32[2] < 1 || u32[2] > (1u << 20) || u32[3] > 4096 || u32[4] > 512) {
        fclose(f);
        return 1;
    }
    r->n_x = u32[2];
    r->nbins = u32[3];
    r->n_par = u32[4];
    r->model = u32[6];
    r->n = u64[0];
    r->thin = u64[1];
    r->lo = range[0];
    r->hi = range[1];
    nx = r->n_x;
    run_predict_alloc(r);
    read_or_die(&r->chain, sizeof(int32_t), 1, f, path);
    read_or_die(r->x, sizeof(double), nx, f, path);
    read_or_die(r->origin, sizeof(double), nx, f, path);
    read_or_die(r->sum, sizeof(double), nx, f, path);
    read_or_die(r->sq, sizeof(double), nx, f, path);
    read_or_die(r->vmin, sizeof(double), nx, f, path);
    read_or_die(r->vmax, sizeof(double), nx, f, path);
    read_or_die(r->hist, sizeof(uint64_t), nx * r->nbins, f, path);
    read_or_die(&r->best_prob, sizeof(double), 1, f, path);
    read_or_die(r->best_params, sizeof(double), r->n_par, f, path);
    read_or_die(&r->best_n, sizeof(uint64_t), 1, f, path);
    fclose(f);
    return 0;
}

void run_predict_write(const char *path, const run_predict *r) {
    FILE *f = run_open_or_die(path, "wb");
    const size_t nx = r->n_x;
    uint32_t u32[8];
    uint64_t u64[2];
    double range[2];
    u32[0] = RUN_PREDICT_VERSION;
    u32[1] = 1;
    u32[2] = r->n_x;
    u32[3] = r->nbins;
    u32[4] = r->n_par;
    u32[5] = 1;
    u32[6] = r->model;
    u32[7] = 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    range[0] = r->lo;
    range[1] = r->hi;
    fwrite(RUN_PREDICT_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 8, f);
    fwrite(u64, sizeof(uint64_t), 2, f);
    fwrite(range, sizeof(double), 2, f);
    fwrite(&r->chain, sizeof(int32_t), 1, f);
    fwrite(r->x, sizeof(double), nx, f);
    fwrite(r->origin, sizeof(double), nx, f);
    fwrite(r->sum, sizeof(double), nx, f);
    fwrite(r->sq, sizeof(double), nx, f);
    fwrite(r->vmin, sizeof(double), nx, f);
    fwrite(r->vmax, sizeof(double), nx, f);
    fwrite(r->hist, sizeof(uint64_t), nx * r->nbins, f);
    fwrite(&r->best_prob, sizeof(double), 1, f);
    fwrite(r->best_params, sizeof(double), r->n_par, f);
    fwrite(&r->best_n, sizeof(uint64_t), 1, f);
    run_close_or_die(f, path);
}

/* the run summary's edges: GSL's uniform ranges, the top one widened */
void run_predict_edges(const run_predict *r, double *edges) {
    uint32_t b;
    for (b = 0; b <= r->nbins; b++)
        edges[b] = run_summary_edge(r->lo, r->hi, b, r->nbins);
}

/* Predict.quantile of apemost_amd/predict.py, operation for operation */
double run_predict_quantile(const run_predict *r, const double *edges, uint32_t i, double q) {
    const uint64_t *h = r->hist + (size_t)i * r->nbins;
    double total = 0.0, want, cum = 0.0, below, t, w;
    uint32_t b;
    for (b = 0; b < r->nbins; b++)
        total += (double)h[b];
    if (total == 0.0)
        return sqrt(-1.0);
    want = q * total;
    for (b = 0; b < r->nbins; b++) { /* the first bin whose cumulative count reaches want */
        cum += (double)h[b];
        if (cum >= want)
            break;
    }
    while (h[b] == 0) { /* (want == 0 with empty leading bins) */
        b++;
        cum += (double)h[b];
    }
    below = cum - (double)h[b];
    t = want - below;
    t = t / (double)h[b];
    w = edges[b + 1] - edges[b];
    t = t * w;
    return edges[b] + t;
}

/* "%.15e", a NaN of either sign as nan */
void run_predict_write_text(const char *path, const run_predict *r, const double *y, const double *best) {
    FILE *f = run_open_or_die(path, "w");
    double *edges = (double *)alloc_or_die((size_t)r->nbins + 1, sizeof(double));
    const double n = (double)r->n;
    const int ratio = r->model == 1 || r->model == 2; /* APEMOST_MODEL_PULSE, APEMOST_MODEL_PULSE_VROT */
    uint32_t i;
    run_predict_edges(r, edges);
    for (i = 0; i < r->n_x; i++) {
        double mean, var, t;
        t = r->sum[i] / n;
        mean = r->origin[i] + t;
        t = r->sum[i] * r->sum[i];
        t = t / n;
        t = r->sq[i] - t;
        var = t / n;
        if (var < 0)
            var = 0.0;
        run_print_values(f, 8, r->x[i], y[i], mean, sqrt(var), ratio ? y[i] / mean : y[i] - mean, r->vmin[i], r->vmax[i],
                         best[i]);
        if (r->nbins > 0) {
            fprintf(f, "\t");
            run_print_values(f, 3, run_predict_quantile(r, edges, i, 0.5), run_predict_quantile(r, edges, i, (1 - 0.68) / 2),
                             run_predict_quantile(r, edges, i, (1 + 0.68) / 2));
        }
        fprintf(f, "\n");
    }
    free(edges);
    run_close_or_die(f, path);
}
