/* reweight.bin reader and writer, reweight.txt, resample.bin, the resampled text dumps and the environment of the
 * APEMOST_DUMP token `reweight` (run_reweight.h).  No device symbol. */
#include "run_reweight.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "run_io.h"

#define alloc_or_die(count) ((double *)run_alloc_or_die(count, sizeof(double), "reweight"))
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "reweight file")

#define RUN_REWEIGHT_MAGIC "APEMOSTW"
#define RUN_REWEIGHT_VERSION 1
#define RUN_RESAMPLE_MAGIC "APEMOSTS"
#define RUN_RESAMPLE_VERSION 1

void run_reweight_alloc(run_reweight *r) {
    const size_t k = r->n_cols, nt = r->n_t, ntri = run_tri_count(k);
    r->lo = alloc_or_die(k);
    r->hi = alloc_or_die(k);
    r->betas_t = alloc_or_die(nt);
    r->m = alloc_or_die(nt);
    r->S0 = alloc_or_die(nt);
    r->SS = alloc_or_die(nt);
    r->origin = alloc_or_die(k);
    r->S1 = alloc_or_die(nt * k);
    r->cross = alloc_or_die(nt * ntri);
    r->hist = (uint64_t *)run_alloc_or_die(nt * k * r->nbins, sizeof(uint64_t), "reweight");
    r->q_total = (uint64_t *)run_alloc_or_die(nt, sizeof(uint64_t), "reweight");
}

void run_reweight_free(run_reweight *r) {
    free(r->lo);
    free(r->hi);
    free(r->betas_t);
    free(r->m);
    free(r->S0);
    free(r->SS);
    free(r->origin);
    free(r->S1);
    free(r->cross);
    free(r->hist);
    free(r->q_total);
    memset(r, 0, sizeof *r);
}

int run_reweight_read(const char *path, run_reweight *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[8];
    uint64_t u64[4];
    size_t k, nt, ntri;
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 8, f, path);
    read_or_die(u64, sizeof(uint64_t), 4, f, path);
    if (memcmp(magic, RUN_REWEIGHT_MAGIC, 8) != 0 || u32[0] != RUN_REWEIGHT_VERSION || u32[2] != 1) {
        fprintf(stderr, "%s: not a reweight file of version %d with one ladder\n", path, RUN_REWEIGHT_VERSION);
        exit(1);
    }
    memset(r, 0, sizeof *r);
    r->n_chains = u32[1];
    r->n_cols = u32[3];
    r->n_t = u32[4];
    r->nbins = u32[5];
    memcpy(&r->shift, &u32[6], sizeof(int32_t));
    r->n = u64[0];
    r->thin = u64[1];
    r->t0 = u64[2];
    r->t_count = u64[3];
    if (r->n_cols < 1 || r->n_cols > RUN_REWEIGHT_MAX_COLS || r->n_t < 1 || r->n_t > RUN_REWEIGHT_MAX_TARGETS ||
        r->nbins > RUN_REWEIGHT_MAX_BINS) {
        fprintf(stderr, "%s: %lu columns, %lu targets and %lu bins are out of range\n", path, (unsigned long)r->n_cols,
                (unsigned long)r->n_t, (unsigned long)r->nbins);
        exit(1);
    }
    read_or_die(r->cols, sizeof(int32_t), RUN_REWEIGHT_MAX_COLS, f, path);
    run_reweight_alloc(r);
    k = r->n_cols;
    nt = r->n_t;
    ntri = run_tri_count(k);
    read_or_die(r->lo, sizeof(double), k, f, path);
    read_or_die(r->hi, sizeof(double), k, f, path);
    read_or_die(r->betas_t, sizeof(double), nt, f, path);
    read_or_die(r->m, sizeof(double), nt, f, path);
    read_or_die(r->S0, sizeof(double), nt, f, path);
    read_or_die(r->SS, sizeof(double), nt, f, path);
    read_or_die(r->origin, sizeof(double), k, f, path);
    read_or_die(r->S1, sizeof(double), nt * k, f, path);
    read_or_die(r->cross, sizeof(double), nt * ntri, f, path);
    read_or_die(r->hist, sizeof(uint64_t), nt * k * r->nbins, f, path);
    read_or_die(r->q_total, sizeof(uint64_t), nt, f, path);
    fclose(f);
    return 0;
}

void run_reweight_write(const char *path, const run_reweight *r) {
    FILE *f = run_open_or_die(path, "wb");
    const size_t k = r->n_cols, nt = r->n_t, ntri = run_tri_count(k);
    uint32_t u32[8];
    uint64_t u64[4];
    u32[0] = RUN_REWEIGHT_VERSION;
    u32[1] = r->n_chains;
    u32[2] = 1;
    u32[3] = r->n_cols;
    u32[4] = r->n_t;
    u32[5] = r->nbins;
    memcpy(&u32[6], &r->shift, sizeof(int32_t));
    u32[7] = 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    u64[2] = r->t0;
    u64[3] = r->t_count;
    fwrite(RUN_REWEIGHT_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 8, f);
    fwrite(u64, sizeof(uint64_t), 4, f);
    fwrite(r->cols, sizeof(int32_t), RUN_REWEIGHT_MAX_COLS, f);
    fwrite(r->lo, sizeof(double), k, f);
    fwrite(r->hi, sizeof(double), k, f);
    fwrite(r->betas_t, sizeof(double), nt, f);
    fwrite(r->m, sizeof(double), nt, f);
    fwrite(r->S0, sizeof(double), nt, f);
    fwrite(r->SS, sizeof(double), nt, f);
    fwrite(r->origin, sizeof(double), k, f);
    fwrite(r->S1, sizeof(double), nt * k, f);
    fwrite(r->cross, sizeof(double), nt * ntri, f);
    fwrite(r->hist, sizeof(uint64_t), nt * k * r->nbins, f);
    fwrite(r->q_total, sizeof(uint64_t), nt, f);
    run_close_or_die(f, path);
}

void run_reweight_write_text(const char *path, const run_reweight *r, const char *const *names) {
    FILE *f = run_open_or_die(path, "w");
    const size_t k = r->n_cols, ntri = run_tri_count(k);
    unsigned int t, a;
    for (t = 0; t < r->n_t; t++)
        for (a = 0; a < k; a++) {
            const double S0 = r->S0[t], ratio = r->S1[t * k + a] / S0;
            const double second = r->cross[t * ntri + a * k - a * (a - 1) / 2] / S0, square = ratio * ratio;
            run_print_value(f, r->betas_t[t]);
            if (names != NULL)
                fprintf(f, "\t%s\t", names[a]);
            else
                fprintf(f, "\tcol%ld\t", (long)r->cols[a]);
            run_print_values(f, 3, r->origin[a] + ratio, sqrt(second - square), S0 * S0 / r->SS[t]);
            fprintf(f, "\n");
        }
    run_close_or_die(f, path);
}

unsigned int run_reweight_bins_from_env(void) {
    const char *spec = getenv("APEMOST_REWEIGHT_BINS");
    char *end;
    long n;
    if (spec == NULL || *spec == 0)
        return 200;
    n = strtol(spec, &end, 10);
    if (*end != 0 || n < 1 || n > RUN_REWEIGHT_MAX_BINS) {
        fprintf(stderr, "APEMOST_REWEIGHT_BINS: expected an integer in 1 .. %d, got '%s'\n", RUN_REWEIGHT_MAX_BINS, spec);
        exit(1);
    }
    return (unsigned int)n;
}

unsigned int run_reweight_betas_from_env(double *betas) {
    const char *spec = getenv("APEMOST_REWEIGHT_BETAS"), *p;
    unsigned int n = 0;
    if (spec == NULL || *spec == 0) {
        betas[0] = 1.0;
        return 1;
    }
    for (p = spec;;) {
        char *end;
        const double v = strtod(p, &end);
        if (end == p || (*end != 0 && *end != ',') || !(v >= 0) || v - v != 0 || n == RUN_REWEIGHT_MAX_TARGETS) {
            fprintf(stderr, "APEMOST_REWEIGHT_BETAS: expected a comma list of at most %d finite numbers >= 0, got '%s'\n",
                    RUN_REWEIGHT_MAX_TARGETS, spec);
            exit(1);
        }
        betas[n++] = v;
        if (*end == 0)
            break;
        p = end + 1;
    }
    return n;
}

/* a decimal uint64 up to `max`, the whole string; 0: malformed */
static int parse_u64(const char *spec, uint64_t max, uint64_t *out) {
    uint64_t v = 0;
    const char *p = spec;
    if (*p == 0)
        return 0;
    for (; *p != 0; p++) {
        uint64_t d;
        if (*p < '0' || *p > '9')
            return 0;
        d = (uint64_t)(*p - '0');
        if (v > (max - d) / 10)
            return 0;
        v = v * 10 + d;
    }
    *out = v;
    return 1;
}

uint32_t run_resample_draws_from_env(void) {
    const char *spec = getenv("APEMOST_RESAMPLE_DRAWS");
    uint64_t n;
    if (spec == NULL || *spec == 0)
        return 0;
    if (!parse_u64(spec, RUN_RESAMPLE_MAX_DRAWS, &n)) {
        fprintf(stderr, "APEMOST_RESAMPLE_DRAWS: expected an integer in 0 .. %lu, got '%s'\n", RUN_RESAMPLE_MAX_DRAWS, spec);
        exit(1);
    }
    return (uint32_t)n;
}

uint64_t run_resample_seed_from_env(void) {
    const char *spec = getenv("APEMOST_RESAMPLE_SEED");
    uint64_t u;
    if (spec == NULL || *spec == 0)
        return 0;
    if (!parse_u64(spec, ~(uint64_t)0, &u)) {
        fprintf(stderr, "APEMOST_RESAMPLE_SEED: expected an integer in 0 .. 2^64 - 1, got '%s'\n", spec);
        exit(1);
    }
    return u;
}

void run_resample_write(const char *path, const run_reweight *r, uint32_t n_draws, uint64_t u, const uint64_t *q_total,
                        const uint32_t *index, const double *x) {
    FILE *f = run_open_or_die(path, "wb");
    const size_t k = r->n_cols;
    uint32_t u32[8];
    uint64_t u64[5];
    unsigned int t;
    u32[0] = RUN_RESAMPLE_VERSION;
    u32[1] = r->n_chains;
    u32[2] = 1;
    u32[3] = r->n_cols;
    u32[4] = r->n_t;
    u32[5] = n_draws;
    memcpy(&u32[6], &r->shift, sizeof(int32_t));
    u32[7] = 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    u64[2] = r->t0;
    u64[3] = r->t_count;
    u64[4] = u;
    fwrite(RUN_RESAMPLE_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 8, f);
    fwrite(u64, sizeof(uint64_t), 5, f);
    fwrite(r->cols, sizeof(int32_t), RUN_REWEIGHT_MAX_COLS, f);
    for (t = 0; t < r->n_t; t++) {
        fwrite(&r->betas_t[t], sizeof(double), 1, f);
        fwrite(&q_total[t], sizeof(uint64_t), 1, f);
        fwrite(index + (size_t)t * n_draws, sizeof(uint32_t), n_draws, f);
        fwrite(x + (size_t)t * n_draws * k, sizeof(double), (size_t)n_draws * k, f);
    }
    run_close_or_die(f, path);
}

void run_resample_write_dumps(const run_reweight *r, unsigned int t, uint32_t n_draws, const double *x,
                              const char *const *names) {
    const size_t k = r->n_cols;
    unsigned int a;
    uint32_t m;
    for (a = 0; a < k; a++) {
        char path[512];
        FILE *f;
        if (names != NULL)
            sprintf(path, "%.400s-reweighted-%u.dump", names[a], t);
        else
            sprintf(path, "col%ld-reweighted-%u.dump", (long)r->cols[a], t);
        f = run_open_or_die(path, "w");
        for (m = 0; m < n_draws; m++)
            fprintf(f, "%.15e\n", x[(size_t)m * k + a]);
        run_close_or_die(f, path);
    }
}
