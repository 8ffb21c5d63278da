/* joint.bin reader and writer and the text files of the APEMOST_DUMP token `joint` (run_joint.h) */
#include "run_joint.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count, size) run_alloc_or_die(count, size, "joint marginals")
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "joint file")

#define RUN_JOINT_MAGIC "APEMOSTJ"
#define RUN_JOINT_VERSION 1

static size_t tri_index(const run_joint *r, unsigned int i, unsigned int j) {
    return (size_t)i * r->n_par - (size_t)i * (i > 0 ? i - 1 : 0) / 2 + (j - i);
}

void run_joint_alloc(run_joint *r) {
    r->pairs = (int32_t *)alloc_or_die((size_t)r->n_pairs * 2, sizeof(int32_t));
    r->lo = (double *)alloc_or_die(r->n_par, sizeof(double));
    r->hi = (double *)alloc_or_die(r->n_par, sizeof(double));
    r->origin = (double *)alloc_or_die(r->n_par, sizeof(double));
    r->sum = (double *)alloc_or_die(r->n_par, sizeof(double));
    r->cross = (double *)alloc_or_die(run_tri_count(r->n_par), sizeof(double));
    r->counts = (uint64_t *)alloc_or_die((size_t)r->n_pairs * r->nbins * r->nbins, sizeof(uint64_t));
}

void run_joint_free(run_joint *r) {
    free(r->pairs);
    free(r->lo);
    free(r->hi);
    free(r->origin);
    free(r->sum);
    free(r->cross);
    free(r->counts);
    memset(r, 0, sizeof *r);
}

int run_joint_read(const char *path, run_joint *r, uint32_t *n_keep, int32_t *chain) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[6];
    uint64_t u64[2];
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 6, f, path);
    if (memcmp(magic, RUN_JOINT_MAGIC, 8) != 0 || u32[0] != RUN_JOINT_VERSION) {
        fprintf(stderr, "%s: not a joint file of version %d\n", path, RUN_JOINT_VERSION);
        exit(1);
    }
    *n_keep = u32[1];
    r->n_par = u32[2];
    r->nbins = u32[3];
    r->n_pairs = u32[4];
    read_or_die(u64, sizeof(uint64_t), 2, f, path);
    r->n = u64[0];
    r->thin = u64[1];
    *chain = -1;
    if (*n_keep != 1 || r->nbins < 1 || r->nbins > 512 || r->n_par < 1 || r->n_par > 65535 ||
        r->n_pairs > r->n_par * (r->n_par - 1) / 2) { /* (not this program's: the caller refuses it by its shape) */
        fclose(f);
        r->pairs = NULL;
        r->lo = r->hi = r->origin = r->sum = r->cross = NULL;
        r->counts = NULL;
        return 0;
    }
    run_joint_alloc(r);
    read_or_die(chain, sizeof(int32_t), 1, f, path);
    read_or_die(r->pairs, sizeof(int32_t), (size_t)r->n_pairs * 2, f, path);
    read_or_die(r->lo, sizeof(double), r->n_par, f, path);
    read_or_die(r->hi, sizeof(double), r->n_par, f, path);
    read_or_die(r->origin, sizeof(double), r->n_par, f, path);
    read_or_die(r->sum, sizeof(double), r->n_par, f, path);
    read_or_die(r->cross, sizeof(double), run_tri_count(r->n_par), f, path);
    read_or_die(r->counts, sizeof(uint64_t), (size_t)r->n_pairs * r->nbins * r->nbins, f, path);
    fclose(f);
    return 0;
}

void run_joint_write(const char *path, const run_joint *r) {
    FILE *f = run_open_or_die(path, "wb");
    uint32_t u32[6];
    uint64_t u64[2];
    const int32_t chain = 0;
    u32[0] = RUN_JOINT_VERSION;
    u32[1] = 1;
    u32[2] = r->n_par;
    u32[3] = r->nbins;
    u32[4] = r->n_pairs;
    u32[5] = 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    fwrite(RUN_JOINT_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 6, f);
    fwrite(u64, sizeof(uint64_t), 2, f);
    fwrite(&chain, sizeof(int32_t), 1, f);
    fwrite(r->pairs, sizeof(int32_t), (size_t)r->n_pairs * 2, f);
    fwrite(r->lo, sizeof(double), r->n_par, f);
    fwrite(r->hi, sizeof(double), r->n_par, f);
    fwrite(r->origin, sizeof(double), r->n_par, f);
    fwrite(r->sum, sizeof(double), r->n_par, f);
    fwrite(r->cross, sizeof(double), run_tri_count(r->n_par), f);
    fwrite(r->counts, sizeof(uint64_t), (size_t)r->n_pairs * r->nbins * r->nbins, f);
    run_close_or_die(f, path);
}

void run_joint_write_pair(const run_joint *r, unsigned int q, const char **names) {
    const unsigned int i = (unsigned int)r->pairs[2 * q], j = (unsigned int)r->pairs[2 * q + 1], n = r->nbins;
    const uint64_t *c = r->counts + (size_t)q * n * n;
    char name[500], (*ey)[32];
    char x0[32], x1[32];
    unsigned int a, b;
    FILE *f;
    sprintf(name, "%.200s-%.200s.joint", names[i], names[j]);
    f = run_open_or_die(name, "w");
    ey = (char(*)[32])alloc_or_die((size_t)n + 1, 32);
    for (b = 0; b <= n; b++)
        sprintf(ey[b], "%.15e", run_summary_edge(r->lo[j], r->hi[j], b, n));
    for (a = 0; a < n; a++) {
        sprintf(x0, "%.15e", run_summary_edge(r->lo[i], r->hi[i], a, n));
        sprintf(x1, "%.15e", run_summary_edge(r->lo[i], r->hi[i], a + 1, n));
        for (b = 0; b < n; b++)
            fprintf(f, "%s %s %s %s %lu\n", x0, x1, ey[b], ey[b + 1], (unsigned long)c[(size_t)a * n + b]);
        fprintf(f, "\n");
    }
    free(ey);
    run_close_or_die(f, name);
}

/* cov_ij = (cross_ij - sum_i sum_j / n) / (n - 1); corr_ij = cov_ij / (sqrt(cov_ii) sqrt(cov_jj)), the diagonal 1 where
 * the variance is finite and positive and NaN elsewhere: apemost_amd/joint.py, operation for operation */
void run_joint_write_correlation(const run_joint *r) {
    const unsigned int np = r->n_par;
    const double n = (double)r->n, n1 = n - 1.0;
    double *cov = (double *)alloc_or_die((size_t)np * np, sizeof(double));
    double *sd = (double *)alloc_or_die(np, sizeof(double));
    unsigned int i, j;
    FILE *f = run_open_or_die("correlation.matrix", "w");
    for (i = 0; i < np; i++)
        for (j = 0; j < np; j++) {
            const double cr = r->cross[i <= j ? tri_index(r, i, j) : tri_index(r, j, i)];
            const double prod = r->sum[i] * r->sum[j];
            const double part = prod / n;
            const double diff = cr - part;
            cov[(size_t)i * np + j] = diff / n1;
        }
    for (i = 0; i < np; i++)
        sd[i] = sqrt(cov[(size_t)i * np + i]);
    for (i = 0; i < np; i++) {
        for (j = 0; j < np; j++) {
            const double v = cov[(size_t)i * np + i], scale = sd[i] * sd[j];
            double x = cov[(size_t)i * np + j] / scale;
            if (i == j)
                x = (v > 0 && v - v == 0) ? 1.0 : sqrt(-1.0);
            if (j > 0)
                fprintf(f, "\t");
            run_print_value(f, x);
        }
        fprintf(f, "\n");
    }
    free(cov);
    free(sd);
    run_close_or_die(f, "correlation.matrix");
}
