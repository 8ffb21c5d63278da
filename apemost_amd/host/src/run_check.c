/* check.bin reader and writer, check.txt and check_stats.txt of the APEMOST_DUMP token `check` (run_check.h).  No
 * device and no chain is needed here. */
#include "run_check.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count, size) run_alloc_or_die(count, size, "check")
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "check file")

#define RUN_CHECK_MAGIC "APEMOSTK"
#define RUN_CHECK_VERSION 1

static const char *const stat_names[RUN_CHECK_N_STATS] = {"fit", "extreme", "serial"};

void run_check_alloc(run_check *r) {
    const size_t nd = r->n_data;
    int q;
    r->x = (double *)alloc_or_die(nd, sizeof(double));
    r->y = (double *)alloc_or_die(nd, sizeof(double));
    for (q = 0; q < RUN_CHECK_WORDS; q++)
        r->state[q] = (double *)alloc_or_die(nd, sizeof(double));
    r->edges = (double *)alloc_or_die((size_t)RUN_CHECK_N_STATS * r->n_edges, sizeof(double));
    for (q = 0; q < RUN_CHECK_STAT_WORDS; q++)
        r->stat[q] = (double *)alloc_or_die(RUN_CHECK_N_STATS, sizeof(double));
    r->counts = (uint64_t *)alloc_or_die((size_t)RUN_CHECK_N_STATS * (r->n_edges + 2), sizeof(uint64_t));
}

void run_check_free(run_check *r) {
    int q;
    free(r->x);
    free(r->y);
    for (q = 0; q < RUN_CHECK_WORDS; q++)
        free(r->state[q]);
    free(r->edges);
    for (q = 0; q < RUN_CHECK_STAT_WORDS; q++)
        free(r->stat[q]);
    free(r->counts);
    memset(r, 0, sizeof *r);
}

int run_check_read(const char *path, run_check *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[8];
    uint64_t u64[2];
    int q;
    if (f == NULL)
        return -1;
    memset(r, 0, sizeof *r);
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 8, f, path);
    read_or_die(u64, sizeof(uint64_t), 2, f, path);
    if (memcmp(magic, RUN_CHECK_MAGIC, 8) != 0 || u32[0] != RUN_CHECK_VERSION) {
        fprintf(stderr, "%s: not a check file of version %d\n", path, RUN_CHECK_VERSION);
        exit(1);
    }
    if (u32[1] != 1) {
        fclose(f);
        return 1;
    }
    r->n_data = u32[2];
    r->n_edges = u32[3];
    r->model = u32[5];
    r->n = u64[0];
    r->thin = u64[1];
    read_or_die(&r->sigma, sizeof(double), 1, f, path);
    read_or_die(&r->chain, sizeof(int32_t), 1, f, path);
    run_check_alloc(r);
    read_or_die(r->x, sizeof(double), r->n_data, f, path);
    read_or_die(r->y, sizeof(double), r->n_data, f, path);
    for (q = 0; q < RUN_CHECK_WORDS; q++)
        read_or_die(r->state[q], sizeof(double), r->n_data, f, path);
    read_or_die(r->edges, sizeof(double), (size_t)RUN_CHECK_N_STATS * r->n_edges, f, path);
    for (q = 0; q < RUN_CHECK_STAT_WORDS; q++)
        read_or_die(r->stat[q], sizeof(double), RUN_CHECK_N_STATS, f, path);
    read_or_die(r->counts, sizeof(uint64_t), (size_t)RUN_CHECK_N_STATS * (r->n_edges + 2), f, path);
    fclose(f);
    return 0;
}

void run_check_write(const char *path, const run_check *r) {
    FILE *f = run_open_or_die(path, "wb");
    const size_t nd = r->n_data;
    uint32_t u32[8];
    uint64_t u64[2];
    int q;
    u32[0] = RUN_CHECK_VERSION;
    u32[1] = 1;
    u32[2] = r->n_data;
    u32[3] = r->n_edges;
    u32[4] = 1;
    u32[5] = r->model;
    u32[6] = 0;
    u32[7] = 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    fwrite(RUN_CHECK_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 8, f);
    fwrite(u64, sizeof(uint64_t), 2, f);
    fwrite(&r->sigma, sizeof(double), 1, f);
    fwrite(&r->chain, sizeof(int32_t), 1, f);
    fwrite(r->x, sizeof(double), nd, f);
    fwrite(r->y, sizeof(double), nd, f);
    for (q = 0; q < RUN_CHECK_WORDS; q++)
        fwrite(r->state[q], sizeof(double), nd, f);
    fwrite(r->edges, sizeof(double), (size_t)RUN_CHECK_N_STATS * r->n_edges, f);
    for (q = 0; q < RUN_CHECK_STAT_WORDS; q++)
        fwrite(r->stat[q], sizeof(double), RUN_CHECK_N_STATS, f);
    fwrite(r->counts, sizeof(uint64_t), (size_t)RUN_CHECK_N_STATS * (r->n_edges + 2), f);
    run_close_or_die(f, path);
}

/* origin + sum / n and sqrt((sq - sum * sum / n) / (n - 1)), the variance never below 0 */
static void moments(double origin, double sum, double sq, double n, double *mean, double *sd) {
    double t = sum / n, var;
    *mean = origin + t;
    t = sum * sum;
    t = t / n;
    t = sq - t;
    var = t / (n - 1.0);
    if (var < 0)
        var = 0.0;
    *sd = sqrt(var);
}

void run_check_write_text(const char *path, const run_check *r) {
    FILE *f = run_open_or_die(path, "w");
    const double n = (double)r->n;
    uint32_t i;
    for (i = 0; i < r->n_data; i++) {
        double mean, sd;
        moments(r->state[0][i], r->state[1][i], r->state[2][i], n, &mean, &sd);
        run_print_values(f, 6, r->x[i], r->y[i], mean, sd, r->state[3][i] / n, r->state[6][i] / r->state[5][i]);
        fprintf(f, "\n");
    }
    run_close_or_die(f, path);
}

double run_check_p_value(const run_check *r, int q, int tail) {
    const uint32_t nbins = r->n_edges + 1;
    const uint64_t *c = r->counts + (size_t)q * (r->n_edges + 2);
    double n = 0.0, upper = 0.0, lower;
    uint32_t b;
    for (b = 0; b < nbins; b++) {
        n += (double)c[b];
        upper += (double)c[b] * (1.0 - ((double)b + 0.5) / (double)nbins);
    }
    if (nbins < 2 || n == 0.0)
        return sqrt(-1.0);
    upper = upper / n;
    lower = 1.0 - upper;
    if (tail == 0)
        return upper;
    if (tail == 1)
        return lower;
    upper = 2.0 * (upper < lower ? upper : lower);
    return upper > 1.0 ? 1.0 : upper;
}

void run_check_write_stats(const char *path, const run_check *r) {
    FILE *f = run_open_or_die(path, "w");
    int q;
    for (q = 0; q < RUN_CHECK_N_STATS; q++) {
        double mean, sd;
        moments(r->stat[0][q], r->stat[1][q], r->stat[2][q], (double)r->n, &mean, &sd);
        fprintf(f, "%s\t", stat_names[q]);
        run_print_values(f, 7, mean, sd, r->stat[3][q], r->stat[4][q], run_check_p_value(r, q, 0), run_check_p_value(r, q, 1),
                         run_check_p_value(r, q, 2));
        fprintf(f, "\n");
    }
    run_close_or_die(f, path);
}
