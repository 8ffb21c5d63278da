/* the device side of the APEMOST_DUMP token `periodogram` (run_periodogram.h): begin, resume, collect */
#include "run_periodogram.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "run_fold.h"
#include "run_io.h"

static run_periodogram periodogram;

static void periodogram_view(run_periodogram *r, apemost_hip_periodogram_view *v) {
    memset(v, 0, sizeof *v);
    v->n = &r->n;
    v->origin = r->state[0];
    v->sum = r->state[1];
    v->sq = r->state[2];
    v->pmin = r->state[3];
    v->pmax = r->state[4];
    v->sum_c = r->state[5];
    v->sum_s = r->state[6];
    v->exceed = r->exceed;
    v->peak_origin = &r->peak[0];
    v->peak_sum = &r->peak[1];
    v->peak_sq = &r->peak[2];
    v->peak_min = &r->peak[3];
    v->peak_max = &r->peak[4];
    v->peak_counts = r->peak_counts;
}

void run_periodogram_check_env(void) {
    double lo, hi;
    uint32_t n;
    run_periodogram_grid_from_env(&lo, &hi, &n);
}

/* begins the fold of chain 0 on shard 0 over the grid of APEMOST_PERIODOGRAM_FREQS; with c->append periodogram.bin is
 * loaded, and one of another shape, grid or data ends the program */
void run_periodogram_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_periodogram *r = &periodogram;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    const int32_t chain = 0;
    apemost_hip_periodogram_view v;
    run_periodogram old;
    double lo, hi, *x;
    int found = -1, q;
    uint32_t i;
    (void)planned;
    memset(r, 0, sizeof *r);
    memset(&old, 0, sizeof old);
    if (ctx->model != APEMOST_MODEL_SIMPLESIN && ctx->model != APEMOST_MODEL_SINE3) {
        fprintf(stderr, "APEMOST_DUMP=periodogram: the residual periodogram is for simplesin and sine3: the pulse models' "
                        "data already are a power spectrum and a device model has no residual law here\n");
        exit(1);
    }
    run_periodogram_grid_from_env(&lo, &hi, &r->n_freq);
    r->n_data = (uint32_t)chain0->data->size1;
    r->model = (uint32_t)ctx->model;
    r->sigma = ctx->sigma;
    r->thin = ctx->thin;
    r->chain = chain;
    r->level = -log(0.01 / (double)r->n_freq);
    run_periodogram_alloc(r);
    run_periodogram_grid(lo, hi, r->n_freq, r->freqs);
    x = (double *)run_alloc_or_die(r->n_data, sizeof(double), "periodogram");
    for (i = 0; i < r->n_data; i++)
        x[i] = gsl_matrix_get(chain0->data, i, 0);
    run_periodogram_weights(x, r->n_data, r->freqs, r->n_freq, r->sigma, r->weights);
    free(x);
    if (ctx->append)
        found = run_periodogram_read(RUN_PERIODOGRAM_FILE, &old);
    if (found >= 0) {
        if (found != 0 || old.chain != 0 || old.n_freq != r->n_freq || old.n_data != r->n_data || old.model != r->model ||
            old.thin != r->thin || old.sigma != r->sigma || old.level != r->level ||
            memcmp(old.freqs, r->freqs, r->n_freq * sizeof(double)) != 0 ||
            memcmp(old.weights, r->weights, 3 * (size_t)r->n_freq * sizeof(double)) != 0) {
            fprintf(stderr, "%s: written by a run of another shape (model, data, sigma, thin:N or "
                            "APEMOST_PERIODOGRAM_FREQS); cannot append\n", RUN_PERIODOGRAM_FILE);
            exit(1);
        }
    } else if (ctx->append)
        fprintf(stderr, "--append: no %s, the periodogram starts with this run\n", RUN_PERIODOGRAM_FILE);
    apemost_hip_or_die(apemost_hip_periodogram_begin(s, 1, &chain, (int32_t)r->n_freq, r->freqs, r->weights, &r->level),
                       "periodogram_begin");
    if (found == 0) {
        r->n = old.n;
        for (q = 0; q < RUN_PERIODOGRAM_WORDS; q++)
            memcpy(r->state[q], old.state[q], r->n_freq * sizeof(double));
        memcpy(r->exceed, old.exceed, r->n_freq * sizeof(uint64_t));
        memcpy(r->peak, old.peak, sizeof r->peak);
        memcpy(r->peak_counts, old.peak_counts, ((size_t)r->n_freq + 1) * sizeof(uint64_t));
        periodogram_view(r, &v);
        apemost_hip_or_die(apemost_hip_periodogram_set(s, &v), "periodogram_set");
        run_periodogram_free(&old);
    }
}

/* collects the accumulator, writes the two files, and frees everything */
void run_periodogram_close(const run_fold_ctx *ctx) {
    run_periodogram *r = &periodogram;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    apemost_hip_periodogram_view v;
    periodogram_view(r, &v);
    apemost_hip_or_die(apemost_hip_periodogram_get(s, &v), "periodogram_get");
    apemost_hip_or_die(apemost_hip_periodogram_end(s), "periodogram_end");
    run_periodogram_write(RUN_PERIODOGRAM_FILE, r);
    run_periodogram_write_text(RUN_PERIODOGRAM_TEXT, r);
    run_periodogram_free(r);
}
