/* pointwise.bin reader and writer, pointwise.txt and criteria.txt of the APEMOST_DUMP token `pointwise`
 * (run_pointwise.h).  No device and no chain is needed here. */
#include "run_pointwise.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count, size) run_alloc_or_die(count, size, "pointwise")
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "pointwise file")

#define RUN_POINTWISE_MAGIC "APEMOSTW"
#define RUN_POINTWISE_VERSION 1
#define RUN_POINTWISE_TAIL_MAGIC "APEMOSTT"
#define RUN_POINTWISE_TAIL_VERSION 1

void run_pointwise_alloc(run_pointwise *r) {
    const size_t nd = r->n_data;
    size_t i;
    int q;
    r->x = (double *)alloc_or_die(nd, sizeof(double));
    r->y = (double *)alloc_or_die(nd, sizeof(double));
    for (q = 0; q < RUN_POINTWISE_WORDS; q++)
        r->state[q] = (double *)alloc_or_die(nd, sizeof(double));
    r->par_origin = (double *)alloc_or_die(r->n_par, sizeof(double));
    r->par_sum = (double *)alloc_or_die(r->n_par, sizeof(double));
    r->at_mean = (double *)alloc_or_die(nd, sizeof(double));
    for (i = 0; i < nd; i++)
        r->at_mean[i] = sqrt(-1.0); /* NaN until somebody fills it */
}

void run_pointwise_free(run_pointwise *r) {
    int q;
    free(r->x);
    free(r->y);
    for (q = 0; q < RUN_POINTWISE_WORDS; q++)
        free(r->state[q]);
    free(r->par_origin);
    free(r->par_sum);
    free(r->at_mean);
    run_pointwise_tail_free(&r->tail);
    memset(r, 0, sizeof *r);
}

uint32_t run_pointwise_tail_capacity_for(uint64_t n) {
    const double a = 0.2 * (double)n, b = 3.0 * sqrt((double)n);
    const double m = ceil(a < b ? a : b) + 1.0;
    return m > 4096.0 ? 4096u : m < 2.0 ? 2u : (uint32_t)m;
}

void run_pointwise_tail_alloc(run_pointwise_tail *t) {
    t->count = (uint64_t *)alloc_or_die(t->n_data, sizeof(uint64_t));
    t->values = (double *)alloc_or_die((size_t)t->n_data * t->capacity, sizeof(double));
}

void run_pointwise_tail_free(run_pointwise_tail *t) {
    free(t->count);
    free(t->values);
    memset(t, 0, sizeof *t);
}

int run_pointwise_read(const char *path, run_pointwise *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[8];
    uint64_t u64[2];
    double sigma;
    size_t nd;
    int q;
    memset(r, 0, sizeof *r);
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 8, f, path);
    if (memcmp(magic, RUN_POINTWISE_MAGIC, 8) != 0 || u32[0] != RUN_POINTWISE_VERSION) {
        fprintf(stderr, "%s: not a pointwise file of version %d\n", path, RUN_POINTWISE_VERSION);
        exit(1);
    }
    read_or_die(u64, sizeof(uint64_t), 2, f, path);
    read_or_die(&sigma, sizeof(double), 1, f, path);
    if (u32[1] != 1 || u32[4] != 1 || u32[2] < 1 || u32[2] > (1u << 20) || u32[3] > 512) {
        fclose(f);
        return 1;
    }
    r->n_data = u32[2];
    r->n_par = u32[3];
    r->model = u32[5];
    r->n = u64[0];
    r->thin = u64[1];
    r->sigma = sigma;
    nd = r->n_data;
    run_pointwise_alloc(r);
    read_or_die(&r->chain, sizeof(int32_t), 1, f, path);
    read_or_die(r->x, sizeof(double), nd, f, path);
    read_or_die(r->y, sizeof(double), nd, f, path);
    for (q = 0; q < RUN_POINTWISE_WORDS; q++)
        read_or_die(r->state[q], sizeof(double), nd, f, path);
    read_or_die(r->par_origin, sizeof(double), r->n_par, f, path);
    read_or_die(r->par_sum, sizeof(double), r->n_par, f, path);
    read_or_die(r->at_mean, sizeof(double), nd, f, path);
    fclose(f);
    return 0;
}

int run_pointwise_tail_read(const char *path, run_pointwise_tail *t) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[8], i;
    uint64_t u64[2];
    memset(t, 0, sizeof *t);
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 8, f, path);
    if (memcmp(magic, RUN_POINTWISE_TAIL_MAGIC, 8) != 0 || u32[0] != RUN_POINTWISE_TAIL_VERSION) {
        fprintf(stderr, "%s: not a pointwise tail file of version %d\n", path, RUN_POINTWISE_TAIL_VERSION);
        exit(1);
    }
    read_or_die(u64, sizeof(uint64_t), 2, f, path);
    if (u32[1] != 1 || u32[4] != 1 || u32[2] < 1 || u32[2] > (1u << 20) || u32[3] < 2 || u32[3] > 4096) {
        fclose(f);
        return 1;
    }
    t->n_data = u32[2];
    t->capacity = u32[3];
    t->n = u64[0];
    t->thin = u64[1];
    run_pointwise_tail_alloc(t);
    read_or_die(&t->chain, sizeof(int32_t), 1, f, path);
    read_or_die(t->count, sizeof(uint64_t), t->n_data, f, path);
    read_or_die(t->values, sizeof(double), (size_t)t->n_data * t->capacity, f, path);
    fclose(f);
    for (i = 0; i < t->n_data; i++)
        if (t->count[i] > t->capacity) {
            run_pointwise_tail_free(t);
            return 1;
        }
    return 0;
}

void run_pointwise_write(const char *path, const run_pointwise *r) {
    FILE *f = run_open_or_die(path, "wb");
    const size_t nd = r->n_data;
    uint32_t u32[8];
    uint64_t u64[2];
    int q;
    u32[0] = RUN_POINTWISE_VERSION;
    u32[1] = 1;
    u32[2] = r->n_data;
    u32[3] = r->n_par;
    u32[4] = 1;
    u32[5] = r->model;
    u32[6] = 0;
    u32[7] = 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    fwrite(RUN_POINTWISE_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 8, f);
    fwrite(u64, sizeof(uint64_t), 2, f);
    fwrite(&r->sigma, sizeof(double), 1, f);
    fwrite(&r->chain, sizeof(int32_t), 1, f);
    fwrite(r->x, sizeof(double), nd, f);
    fwrite(r->y, sizeof(double), nd, f);
    for (q = 0; q < RUN_POINTWISE_WORDS; q++)
        fwrite(r->state[q], sizeof(double), nd, f);
    fwrite(r->par_origin, sizeof(double), r->n_par, f);
    fwrite(r->par_sum, sizeof(double), r->n_par, f);
    fwrite(r->at_mean, sizeof(double), nd, f);
    run_close_or_die(f, path);
}

void run_pointwise_tail_write(const char *path, const run_pointwise_tail *t) {
    FILE *f = run_open_or_die(path, "wb");
    const double zero = 0.0;
    uint32_t u32[8], i, j;
    uint64_t u64[2];
    u32[0] = RUN_POINTWISE_TAIL_VERSION;
    u32[1] = 1;
    u32[2] = t->n_data;
    u32[3] = t->capacity;
    u32[4] = 1;
    u32[5] = u32[6] = u32[7] = 0;
    u64[0] = t->n;
    u64[1] = t->thin;
    fwrite(RUN_POINTWISE_TAIL_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 8, f);
    fwrite(u64, sizeof(uint64_t), 2, f);
    fwrite(&t->chain, sizeof(int32_t), 1, f);
    fwrite(t->count, sizeof(uint64_t), t->n_data, f);
    for (i = 0; i < t->n_data; i++)
        for (j = 0; j < t->capacity; j++)
            fwrite(j < t->count[i] ? &t->values[(size_t)i * t->capacity + j] : &zero, sizeof(double), 1, f);
    run_close_or_die(f, path);
}

/* what Pointwise gives per datum (apemost_amd/pointwise.py), operation for operation */
typedef struct {
    double mean, var, lppd, p_waic1, elpd_waic, elpd_loo, ess;
} pointwise_datum;

static pointwise_datum datum(const run_pointwise *r, uint32_t i) {
    const double n = (double)r->n;
    const double origin = r->state[0][i], sum = r->state[1][i], sq = r->state[2][i], m_up = r->state[3][i],
                 S_up = r->state[4][i], m_dn = r->state[5][i], S_dn = r->state[6][i], S2_dn = r->state[7][i];
    pointwise_datum d;
    double t;
    t = sum / n;
    d.mean = origin + t;
    t = sum * sum;
    t = t / n;
    t = sq - t;
    d.var = t / (n - 1.0);
    if (d.var < 0)
        d.var = 0.0;
    t = S_up / n;
    d.lppd = m_up + log(t);
    t = d.lppd - d.mean;
    d.p_waic1 = 2.0 * t;
    d.elpd_waic = d.lppd - d.var;
    t = S_dn / n;
    t = m_dn + log(t);
    d.elpd_loo = -t;
    t = S_dn * S_dn;
    d.ess = t / S2_dn;
    return d;
}

/* "%.15e", a NaN of either sign as nan */
void run_pointwise_write_text(const char *path, const run_pointwise *r) {
    FILE *f = run_open_or_die(path, "w");
    uint32_t i;
    for (i = 0; i < r->n_data; i++) {
        const pointwise_datum d = datum(r, i);
        run_print_values(f, 8, r->x[i], r->y[i], d.mean, sqrt(d.var), d.lppd, d.var, d.elpd_loo, d.ess);
        fprintf(f, "\n");
    }
    run_close_or_die(f, path);
}

static void print_named(FILE *f, const char *name, double v) {
    fprintf(f, "%s\t", name);
    run_print_value(f, v);
    fprintf(f, "\n");
}

void run_pointwise_write_criteria(const char *path, const run_pointwise *r) {
    FILE *f = run_open_or_die(path, "w");
    const double nd = (double)r->n_data;
    double lppd = 0.0, p1 = 0.0, p2 = 0.0, waic = 0.0, loo = 0.0, at = 0.0, mean = 0.0, spread = 0.0, centre, p_dic, t, u;
    uint32_t i;
    for (i = 0; i < r->n_data; i++) {
        const pointwise_datum d = datum(r, i);
        lppd = lppd + d.lppd;
        p1 = p1 + d.p_waic1;
        p2 = p2 + d.var;
        waic = waic + d.elpd_waic;
        loo = loo + d.elpd_loo;
        at = at + r->at_mean[i];
        mean = mean + d.mean;
    }
    /* sqrt(n_data * variance of the pointwise elpd_waic), the variance divided by n_data - 1 */
    centre = waic / nd;
    for (i = 0; i < r->n_data; i++) {
        t = datum(r, i).elpd_waic - centre;
        t = t * t;
        spread = spread + t;
    }
    spread = spread / (nd - 1.0);
    spread = nd * spread;
    t = at - mean;
    p_dic = 2.0 * t;
    print_named(f, "n", (double)r->n);
    print_named(f, "lppd", lppd);
    print_named(f, "p_waic1", p1);
    print_named(f, "p_waic2", p2);
    print_named(f, "elpd_waic", waic);
    print_named(f, "waic", -2.0 * waic);
    print_named(f, "waic_se", sqrt(spread));
    print_named(f, "elpd_loo", loo);
    print_named(f, "looic", -2.0 * loo);
    print_named(f, "p_loo", lppd - loo);
    t = -2.0 * at;
    u = 2.0 * p_dic;
    print_named(f, "dic", t + u);
    print_named(f, "p_dic", p_dic);
    run_close_or_die(f, path);
}
