/* evidence.bin reader and writer and evidence.txt of the APEMOST_DUMP token `evidence` (run_evidence.h) */
#include "run_evidence.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count) ((double *)run_alloc_or_die(count, sizeof(double), "evidence"))
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "evidence file")

#define RUN_EVIDENCE_MAGIC "APEMOSTE"
#define RUN_EVIDENCE_VERSION 1

void run_evidence_alloc(run_evidence *r) {
    const size_t nc = r->n_chains;
    r->betas = alloc_or_die(nc);
    r->coef_up = alloc_or_die(nc);
    r->coef_down = alloc_or_die(nc);
    r->origin = alloc_or_die(nc);
    r->sum = alloc_or_die(nc);
    r->sq = alloc_or_die(nc);
    r->m = alloc_or_die(2 * nc);
    r->S = alloc_or_die(2 * nc);
    r->batch = alloc_or_die(nc * (size_t)(r->max_batches + 1));
}

void run_evidence_free(run_evidence *r) {
    free(r->betas);
    free(r->coef_up);
    free(r->coef_down);
    free(r->origin);
    free(r->sum);
    free(r->sq);
    free(r->m);
    free(r->S);
    free(r->batch);
    memset(r, 0, sizeof *r);
}

int run_evidence_read(const char *path, run_evidence *r, uint32_t *n_ladders) {
    FILE *f = fopen(path, "rb");
    char magic[8];
    uint32_t u32[4];
    uint64_t u64[4];
    size_t nc;
    if (f == NULL)
        return -1;
    read_or_die(magic, 1, 8, f, path);
    read_or_die(u32, sizeof(uint32_t), 4, f, path);
    read_or_die(u64, sizeof(uint64_t), 4, f, path);
    if (memcmp(magic, RUN_EVIDENCE_MAGIC, 8) != 0 || u32[0] != RUN_EVIDENCE_VERSION) {
        fprintf(stderr, "%s: not an evidence file of version %d\n", path, RUN_EVIDENCE_VERSION);
        exit(1);
    }
    r->n_chains = u32[1];
    *n_ladders = u32[2];
    r->n = u64[0];
    r->thin = u64[1];
    r->bs = u64[2];
    r->max_batches = u64[3];
    if (r->bs < 1 || r->max_batches > ((uint64_t)1 << 40) || run_batches_closed(r->n, r->bs) > r->max_batches) {
        fprintf(stderr, "%s: batch size %lu and %lu batches do not fit %lu samples\n", path, (unsigned long)r->bs,
                (unsigned long)r->max_batches, (unsigned long)r->n);
        exit(1);
    }
    nc = r->n_chains;
    run_evidence_alloc(r);
    read_or_die(r->betas, sizeof(double), nc, f, path);
    read_or_die(r->coef_up, sizeof(double), nc, f, path);
    read_or_die(r->coef_down, sizeof(double), nc, f, path);
    read_or_die(r->origin, sizeof(double), nc, f, path);
    read_or_die(r->sum, sizeof(double), nc, f, path);
    read_or_die(r->sq, sizeof(double), nc, f, path);
    read_or_die(r->m, sizeof(double), 2 * nc, f, path);
    read_or_die(r->S, sizeof(double), 2 * nc, f, path);
    read_or_die(r->batch, sizeof(double), nc * (size_t)(r->max_batches + 1), f, path);
    fclose(f);
    return 0;
}

void run_evidence_write(const char *path, const run_evidence *r) {
    FILE *f = run_open_or_die(path, "wb");
    const size_t nc = r->n_chains;
    uint32_t u32[4];
    uint64_t u64[4];
    u32[0] = RUN_EVIDENCE_VERSION;
    u32[1] = r->n_chains;
    u32[2] = 1;
    u32[3] = 0;
    u64[0] = r->n;
    u64[1] = r->thin;
    u64[2] = r->bs;
    u64[3] = r->max_batches;
    fwrite(RUN_EVIDENCE_MAGIC, 1, 8, f);
    fwrite(u32, sizeof(uint32_t), 4, f);
    fwrite(u64, sizeof(uint64_t), 4, f);
    fwrite(r->betas, sizeof(double), nc, f);
    fwrite(r->coef_up, sizeof(double), nc, f);
    fwrite(r->coef_down, sizeof(double), nc, f);
    fwrite(r->origin, sizeof(double), nc, f);
    fwrite(r->sum, sizeof(double), nc, f);
    fwrite(r->sq, sizeof(double), nc, f);
    fwrite(r->m, sizeof(double), 2 * nc, f);
    fwrite(r->S, sizeof(double), 2 * nc, f);
    fwrite(r->batch, sizeof(double), nc * (size_t)(r->max_batches + 1), f);
    run_close_or_die(f, path);
}

/* "%.15e", a NaN of either sign as nan */
static void print_total(FILE *f, const char *name, double v) {
    fprintf(f, "%s\t", name);
    run_print_value(f, v);
    fprintf(f, "\n");
}

/* the weight of chain c's mean loglike in a thermodynamic rule over beta_min .. beta_0 (trapezoid != 0: both ends of
 * every interval by halves), plus beta_last for the last chain: the base `rectangle` */
static double rule_weight(const run_evidence *r, unsigned int c, int trapezoid) {
    const unsigned int nc = r->n_chains;
    const double *b = r->betas;
    double w = 0;
    if (!trapezoid) {
        if (c + 1 < nc)
            w = b[c] - b[c + 1];
    } else {
        if (c + 1 < nc)
            w += (b[c] - b[c + 1]) / 2;
        if (c > 0)
            w += (b[c - 1] - b[c]) / 2;
    }
    if (c + 1 == nc)
        w += b[c];
    return w;
}

/* apemost_amd/evidence.py, Evidence.text(), operation for operation */
void run_evidence_write_text(const char *path, const run_evidence *r) {
    const unsigned int nc = r->n_chains;
    const double n = (double)r->n, n1 = n - 1.0;
    const uint64_t nb = run_batches_closed(r->n, r->bs);
    double *mean = alloc_or_die(nc), *var = alloc_or_die(nc), *mcse = alloc_or_die(nc);
    double *up = alloc_or_die(nc), *down = alloc_or_die(nc);
    double base_rect, base_down, rect, trap, corr, ss_up, ss_down, e_rect = 0, e_trap = 0;
    unsigned int c;
    uint64_t k;
    FILE *f = run_open_or_die(path, "w");
    for (c = 0; c < nc; c++) {
        const double beta = r->betas[c], mean_v = r->origin[c] + r->sum[c] / n;
        const double *batch = r->batch + (size_t)c * (size_t)(r->max_batches + 1);
        double errorsum = 0;
        mean[c] = mean_v / beta;
        var[c] = (r->sq[c] - r->sum[c] * r->sum[c] / n) / n1 / (beta * beta);
        for (k = 0; k < nb; k++) { /* a batch's mean over the samples it holds: batch 0 holds bs - 1 (1 for bs = 1) */
            const double count = k == 0 ? (r->bs > 1 ? (double)(r->bs - 1) : 1.0) : (double)r->bs;
            const double d = batch[k] / count - mean_v;
            errorsum += d * d;
        }
        mcse[c] = nb < 2 ? sqrt(-1.0) : sqrt(errorsum / (double)nb) / sqrt((double)nb) / beta;
        up[c] = r->m[c] + log(r->S[c] / n);
        down[c] = r->m[nc + c] + log(r->S[nc + c] / n);
        run_print_values(f, 6, beta, mean[c], var[c], mcse[c], up[c], down[c]);
        fprintf(f, "\n");
    }
    base_rect = mean[nc - 1] * r->betas[nc - 1];
    base_down = -down[nc - 1];
    rect = trap = corr = base_rect;
    ss_up = ss_down = base_down;
    for (c = nc - 1; c-- > 0;) { /* from the hottest interval up */
        const double db = r->betas[c] - r->betas[c + 1];
        rect += mean[c] * db;
        trap += (mean[c] + mean[c + 1]) / 2 * db;
        corr += (mean[c] + mean[c + 1]) / 2 * db;
        corr -= db * db / 12 * (var[c] - var[c + 1]);
        ss_up += up[c + 1];
        ss_down += -down[c];
    }
    for (c = 0; c < nc; c++) {
        const double wr = rule_weight(r, c, 0) * mcse[c], wt = rule_weight(r, c, 1) * mcse[c];
        e_rect += wr * wr;
        e_trap += wt * wt;
    }
    print_total(f, "thermodynamic_rectangle", rect);
    print_total(f, "thermodynamic_trapezoid", trap);
    print_total(f, "thermodynamic_corrected", corr);
    print_total(f, "thermodynamic_corrected_base_down", corr - base_rect + base_down);
    print_total(f, "stepping_stone_up", ss_up);
    print_total(f, "stepping_stone_down", ss_down);
    print_total(f, "base_rectangle", base_rect);
    print_total(f, "base_down", base_down);
    print_total(f, "error_rectangle", sqrt(e_rect));
    print_total(f, "error_trapezoid", sqrt(e_trap));
    print_total(f, "error_corrected", sqrt(e_trap));
    free(mean);
    free(var);
    free(mcse);
    free(up);
    free(down);
    run_close_or_die(f, path);
}
