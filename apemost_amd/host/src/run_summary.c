/* summary.bin reader and writer (run_summary.h) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "run_summary.h"
#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count, size) run_alloc_or_die(count, size, "run summary")
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "run summary")

#define RUN_SUMMARY_MAGIC "APEMOSTS"
#define RUN_SUMMARY_VERSION 1

void run_summary_alloc(run_summary *r) {
    const size_t n_hp = (size_t)r->n_hist * r->n_par;
    r->lo = (double *)alloc_or_die(r->n_par, sizeof(double));
    r->hi = (double *)alloc_or_die(r->n_par, sizeof(double));
    r->prob_sum = (double *)alloc_or_die(r->n_beta, sizeof(double));
    r->hist = (uint64_t *)alloc_or_die(n_hp * r->nbins, sizeof(uint64_t));
    r->batch_sums = (double *)alloc_or_die(n_hp * (r->max_batches + 1), sizeof(double));
}

void run_summary_free(run_summary *r) {
    free(r->lo);
    free(r->hi);
    free(r->prob_sum);
    free(r->hist);
    free(r->batch_sums);
    r->lo = r->hi = r->prob_sum = r->batch_sums = NULL;
    r->hist = NULL;
}

int run_summary_read(const char *path, run_summary *r) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[4], zero;
    uint64_t u64[5];
    size_t n_hp;
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 4, f, path);
    if (memcmp(magic, RUN_SUMMARY_MAGIC, 8) != 0 || u32[0] != RUN_SUMMARY_VERSION) {
        fprintf(stderr, "%s: not a run summary of version %d\n", path, RUN_SUMMARY_VERSION);
        exit(1);
    }
    r->n_beta = u32[1];
    r->n_par = u32[2];
    r->nbins = u32[3];
    read_or_die(u64, sizeof(uint64_t), 2, f, path);
    r->thin = u64[0];
    r->bs = u64[1];
    read_or_die(&r->n_hist, sizeof(uint32_t), 1, f, path);
    read_or_die(&zero, sizeof(uint32_t), 1, f, path);
    read_or_die(u64, sizeof(uint64_t), 3, f, path);
    r->n = u64[0];
    r->n_batches = u64[1];
    r->max_batches = u64[2];
    if (r->bs < 1 || r->n_batches > r->max_batches || r->n_batches != run_batches_closed(r->n, r->bs)) {
        fprintf(stderr, "%s: inconsistent run summary\n", path);
        exit(1);
    }
    run_summary_alloc(r);
    n_hp = (size_t)r->n_hist * r->n_par;
    read_or_die(r->lo, sizeof(double), r->n_par, f, path);
    read_or_die(r->hi, sizeof(double), r->n_par, f, path);
    read_or_die(r->prob_sum, sizeof(double), r->n_beta, f, path);
    read_or_die(r->hist, sizeof(uint64_t), n_hp * r->nbins, f, path);
    read_or_die(r->batch_sums, sizeof(double), n_hp * (r->max_batches + 1), f, path);
    fclose(f);
    return 0;
}

void run_summary_write(const char *path, const run_summary *r) {
    FILE *f = fopen(path, "wb");
    uint32_t u32[4], tail[2];
    uint64_t u64[5];
    const size_t n_hp = (size_t)r->n_hist * r->n_par;
    if (f == NULL) {
        fprintf(stderr, "opening file %s failed\n", path);
        exit(1);
    }
    u32[0] = RUN_SUMMARY_VERSION;
    u32[1] = r->n_beta;
    u32[2] = r->n_par;
    u32[3] = r->nbins;
    fwrite(RUN_SUMMARY_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 4, f);
    u64[0] = r->thin;
    u64[1] = r->bs;
    fwrite(u64, sizeof(uint64_t), 2, f);
    tail[0] = r->n_hist;
    tail[1] = 0;
    fwrite(tail, sizeof(uint32_t), 2, f);
    u64[0] = r->n;
    u64[1] = r->n_batches;
    u64[2] = r->max_batches;
    fwrite(u64, sizeof(uint64_t), 3, f);
    fwrite(r->lo, sizeof(double), r->n_par, f);
    fwrite(r->hi, sizeof(double), r->n_par, f);
    fwrite(r->prob_sum, sizeof(double), r->n_beta, f);
    fwrite(r->hist, sizeof(uint64_t), n_hp * r->nbins, f);
    fwrite(r->batch_sums, sizeof(double), n_hp * (r->max_batches + 1), f);
    run_close_or_die(f, path);
}
