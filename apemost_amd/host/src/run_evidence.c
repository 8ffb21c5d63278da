/* evidence.bin reader and writer and evidence.txt of the APEMOST_DUMP token `evidence` (run_evidence.h) */
#include "run_evidence.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parallel_tempering_beta.h"
#include "run_summary.h"
#include "run_io.h"

/* run_io.h with this file's word in the messages */
#define alloc_or_die(count) ((double *)run_alloc_or_die(count, sizeof(double), "evidence"))
#define read_or_die(p, size, count, f, path) run_read_or_die(p, size, count, f, path, "evidence file")

#define RUN_EVIDENCE_MAGIC "APEMOSTE"
#define RUN_EVIDENCE_VERSION 1

static void evidence_alloc(run_evidence *r) {
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

static void evidence_free(run_evidence *r) {
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

/* 0: read; -1: no such file.  *n_ladders receives the ladders the file holds */
static int evidence_read(const char *path, run_evidence *r, uint32_t *n_ladders) {
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
    if (r->bs < 1 || r->max_batches > ((uint64_t)1 << 40) || run_summary_batches(r->n, r->bs) > r->max_batches) {
        fprintf(stderr, "%s: batch size %lu and %lu batches do not fit %lu samples\n", path, (unsigned long)r->bs,
                (unsigned long)r->max_batches, (unsigned long)r->n);
        exit(1);
    }
    nc = r->n_chains;
    evidence_alloc(r);
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

static void evidence_write(const char *path, const run_evidence *r) {
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

/* the view of shard j over the whole ladder's arrays; m and S of a shard are [2][its chains], staged in `ms` */
static void evidence_view(run_evidence *r, apemost_hip_evidence_view *v, unsigned int first, double *ms,
                          unsigned int n_local) {
    v->n = &r->n;
    v->origin = r->origin + first;
    v->sum = r->sum + first;
    v->sq = r->sq + first;
    v->batch = r->batch + (size_t)first * (size_t)(r->max_batches + 1);
    v->m = ms;
    v->S = ms + 2 * (size_t)n_local;
}

void run_evidence_open(run_evidence *r, apemost_ladder *l, mcmc **chains, const unsigned int *lo, unsigned int n_shards,
                       uint64_t planned, uint64_t thin, int append) {
    const unsigned int nc = lo[n_shards];
    run_evidence old;
    uint32_t old_ladders = 0;
    int resumed = 0;
    unsigned int c, j, s;
    uint64_t b;
    double *ms;
    memset(&old, 0, sizeof old);
    memset(r, 0, sizeof *r);
    if (append && evidence_read(RUN_EVIDENCE_FILE, &old, &old_ladders) == 0) {
        if (old.n_chains != nc || old_ladders != 1 || old.thin != thin) {
            fprintf(stderr, "%s: written by a run of another shape (chains or thin:N); cannot append\n", RUN_EVIDENCE_FILE);
            exit(1);
        }
        resumed = 1;
    } else if (append)
        fprintf(stderr, "--append: no %s, the evidence fold starts with this run\n", RUN_EVIDENCE_FILE);
    r->n_chains = nc;
    r->thin = thin;
    r->n = resumed ? old.n : 0;
    r->bs = resumed ? old.bs : (uint64_t)sqrt((double)planned);
    if (r->bs < 1)
        r->bs = 1;
    r->max_batches = run_summary_batches(r->n + planned, r->bs);
    evidence_alloc(r);
    for (c = 0; c < nc; c++) {
        r->betas[c] = get_beta(chains[c]);
        if (!(r->betas[c] > 0) || r->betas[c] - r->betas[c] != 0 || (c > 0 && !(r->betas[c] < r->betas[c - 1]))) {
            fprintf(stderr, "APEMOST_DUMP=evidence: beta of chain %u is %g; the betas must be positive and strictly "
                            "decreasing (with beta = 0 the column prob - prior is identically 0)\n", c, r->betas[c]);
            exit(1);
        }
        if (resumed && old.betas[c] != r->betas[c]) {
            fprintf(stderr, "%s: chain %u had beta %g, now %g; cannot append\n", RUN_EVIDENCE_FILE, c, old.betas[c],
                    r->betas[c]);
            exit(1);
        }
    }
    for (c = 0; c < nc; c++) {
        r->coef_up[c] = c > 0 ? (r->betas[c - 1] - r->betas[c]) / r->betas[c] : 0.0;
        r->coef_down[c] = c + 1 < nc ? -(r->betas[c] - r->betas[c + 1]) / r->betas[c] : -1.0;
    }
    if (resumed) {
        memcpy(r->origin, old.origin, nc * sizeof(double));
        memcpy(r->sum, old.sum, nc * sizeof(double));
        memcpy(r->sq, old.sq, nc * sizeof(double));
        memcpy(r->m, old.m, 2 * (size_t)nc * sizeof(double));
        memcpy(r->S, old.S, 2 * (size_t)nc * sizeof(double));
        for (c = 0; c < nc; c++) /* closed batches and the open one, at the new capacity's stride */
            for (b = 0; b <= run_summary_batches(old.n, old.bs); b++)
                r->batch[(size_t)c * (size_t)(r->max_batches + 1) + b] = old.batch[(size_t)c * (size_t)(old.max_batches + 1) + b];
        evidence_free(&old);
    }
    ms = alloc_or_die(4 * (size_t)nc);
    for (j = 0; j < n_shards; j++) {
        apemost_hip_sampler *sampler = apemost_ladder_shard(l, j);
        const unsigned int n_local = lo[j + 1] - lo[j];
        apemost_hip_evidence_config cfg;
        apemost_hip_evidence_view v;
        cfg.batch_size = r->bs;
        cfg.max_batches = r->max_batches;
        cfg.coef_up = r->coef_up + lo[j];
        cfg.coef_down = r->coef_down + lo[j];
        apemost_hip_or_die(apemost_hip_evidence_begin(sampler, &cfg), "evidence_begin");
        if (resumed) {
            for (s = 0; s < 2; s++) {
                memcpy(ms + s * n_local, r->m + (size_t)s * nc + lo[j], n_local * sizeof(double));
                memcpy(ms + (2 + s) * (size_t)n_local, r->S + (size_t)s * nc + lo[j], n_local * sizeof(double));
            }
            evidence_view(r, &v, lo[j], ms, n_local);
            apemost_hip_or_die(apemost_hip_evidence_set(sampler, &v), "evidence_set");
        }
    }
    free(ms);
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
static void evidence_write_text(const char *path, const run_evidence *r) {
    const unsigned int nc = r->n_chains;
    const double n = (double)r->n, n1 = n - 1.0;
    const uint64_t nb = run_summary_batches(r->n, r->bs);
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
        run_print_value(f, beta);
        fprintf(f, "\t");
        run_print_value(f, mean[c]);
        fprintf(f, "\t");
        run_print_value(f, var[c]);
        fprintf(f, "\t");
        run_print_value(f, mcse[c]);
        fprintf(f, "\t");
        run_print_value(f, up[c]);
        fprintf(f, "\t");
        run_print_value(f, down[c]);
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

void run_evidence_close(run_evidence *r, apemost_ladder *l, const unsigned int *lo, unsigned int n_shards) {
    const unsigned int nc = r->n_chains;
    double *ms = alloc_or_die(4 * (size_t)nc);
    unsigned int j, s;
    for (j = 0; j < n_shards; j++) {
        apemost_hip_sampler *sampler = apemost_ladder_shard(l, j);
        const unsigned int n_local = lo[j + 1] - lo[j];
        apemost_hip_evidence_view v;
        evidence_view(r, &v, lo[j], ms, n_local);
        apemost_hip_or_die(apemost_hip_evidence_get(sampler, &v), "evidence_get");
        apemost_hip_or_die(apemost_hip_evidence_end(sampler), "evidence_end");
        for (s = 0; s < 2; s++) {
            memcpy(r->m + (size_t)s * nc + lo[j], ms + s * n_local, n_local * sizeof(double));
            memcpy(r->S + (size_t)s * nc + lo[j], ms + (2 + s) * (size_t)n_local, n_local * sizeof(double));
        }
    }
    free(ms);
    evidence_write(RUN_EVIDENCE_FILE, r);
    evidence_write_text(RUN_EVIDENCE_TEXT, r);
    evidence_free(r);
}
