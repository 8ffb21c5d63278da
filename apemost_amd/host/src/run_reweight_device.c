/* the device side of the APEMOST_DUMP token `reweight` (run_reweight.h): begin beside the mbar fold, the evaluation
 * behind its solve, the files at the end */
#include "run_reweight.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mcmc_gettersetter.h"
#include "run_fold.h"
#include "run_io.h"
#include "run_mbar.h"

static run_reweight reweight;
static int is_open, evaluated;
/* APEMOST_RESAMPLE_DRAWS > 0: the draws of every target, kept from the solve to the close, which writes them */
static uint32_t n_draws;
static uint64_t draw_seed;
static uint64_t *draw_q_total; /* [n_t] */
static uint32_t *draw_index;   /* [n_t][n_draws] */
static double *draw_x;         /* [n_t][n_draws][n_cols] */

static void draws_free(void) {
    free(draw_q_total);
    free(draw_index);
    free(draw_x);
    draw_q_total = NULL;
    draw_index = NULL;
    draw_x = NULL;
}

/* the parameters of every chain beside the mbar fold, which the table has opened before (shard 0, the whole ladder).
 * reweight.bin holds the sums and not the columns, so there is nothing a later run could go on from. */
void run_reweight_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_reweight *r = &reweight;
    const unsigned int n_par = get_n_par(ctx->chains[0]);
    apemost_hip_sampler *sampler = apemost_ladder_shard(ctx->l, 0);
    apemost_hip_reweight_config cfg;
    double betas[RUN_REWEIGHT_MAX_TARGETS];
    unsigned int p;
    (void)planned; /* (the capacity is the mbar fold's) */
    memset(r, 0, sizeof *r);
    is_open = evaluated = 0;
    n_draws = run_resample_draws_from_env();
    draw_seed = run_resample_seed_from_env();
    if (ctx->append) {
        fprintf(stderr, "APEMOST_DUMP=reweight cannot go on from an earlier run (--append): %s holds the sums, not the "
                        "columns\n", RUN_REWEIGHT_FILE);
        exit(1);
    }
    if (n_par > RUN_REWEIGHT_MAX_COLS) {
        fprintf(stderr, "APEMOST_DUMP=reweight: %u parameters are more than %d columns\n", n_par, RUN_REWEIGHT_MAX_COLS);
        exit(1);
    }
    r->n_chains = ctx->lo[ctx->n_shards];
    r->n_cols = n_par;
    r->n_t = run_reweight_betas_from_env(betas);
    r->nbins = run_reweight_bins_from_env();
    r->thin = ctx->thin;
    run_reweight_alloc(r);
    memcpy(r->betas_t, betas, r->n_t * sizeof(double));
    for (p = 0; p < n_par; p++) {
        r->cols[p] = (int32_t)p;
        r->lo[p] = get_params_min_for(ctx->chains[0], p);
        r->hi[p] = get_params_max_for(ctx->chains[0], p);
    }
    cfg.n_cols = (int32_t)n_par;
    cfg.cols = r->cols;
    cfg.nbins = (int32_t)r->nbins;
    cfg.lo = r->lo;
    cfg.hi = r->hi;
    apemost_hip_or_die(apemost_hip_reweight_begin(sampler, &cfg), "reweight_begin");
    is_open = 1;
}

/* called by the mbar fold's close between its solve and its end, while both stores are on the device: m is the solved
 * state (m->solved == 0: no free energies, and so no reweight files, which is said) */
void run_reweight_solved(const run_fold_ctx *ctx, const run_mbar *m) {
    run_reweight *r = &reweight;
    apemost_hip_sampler *sampler = apemost_ladder_shard(ctx->l, 0);
    apemost_hip_reweight_view v;
    apemost_hip_reweight_sums out;
    uint64_t bad[RUN_REWEIGHT_MAX_COLS];
    unsigned int p, t;
    if (!is_open)
        return;
    if (!m->solved) {
        fprintf(stderr, "APEMOST_DUMP=reweight: the mbar fold has no free energies; no %s\n", RUN_REWEIGHT_FILE);
        return;
    }
    v.n = &r->n;
    v.n_bad = bad;
    v.x = NULL;
    apemost_hip_or_die(apemost_hip_reweight_get(sampler, &v), "reweight_get");
    for (p = 0; p < r->n_cols; p++)
        if (bad[p] != 0) {
            fprintf(stderr, "APEMOST_DUMP=reweight: %lu stored values of parameter %u are not finite; no %s\n",
                    (unsigned long)bad[p], p, RUN_REWEIGHT_FILE);
            return;
        }
    r->t0 = m->t0;
    r->t_count = m->t_count;
    out.m = r->m;
    out.S0 = r->S0;
    out.SS = r->SS;
    out.origin = r->origin;
    out.S1 = r->S1;
    out.cross = r->cross;
    out.shift = &r->shift;
    out.hist = r->hist;
    out.q_total = r->q_total;
    apemost_hip_or_die(apemost_hip_reweight_evaluate(sampler, m->t0, m->t_count, m->g, r->betas_t, (int32_t)r->n_t, &out),
                       "reweight_evaluate");
    if (n_draws > 0) {
        draw_q_total = (uint64_t *)run_alloc_or_die(r->n_t, sizeof(uint64_t), "resample");
        draw_index = (uint32_t *)run_alloc_or_die((size_t)r->n_t * n_draws, sizeof(uint32_t), "resample");
        draw_x = (double *)run_alloc_or_die((size_t)r->n_t * n_draws * r->n_cols, sizeof(double), "resample");
        for (t = 0; t < r->n_t; t++) {
            apemost_hip_reweight_draws d;
            d.index = draw_index + (size_t)t * n_draws;
            d.x = draw_x + (size_t)t * n_draws * r->n_cols;
            d.q_total = draw_q_total + t;
            d.shift = NULL;
            apemost_hip_or_die(apemost_hip_reweight_resample(sampler, m->t0, m->t_count, m->g, r->betas_t[t], n_draws,
                                                             draw_seed, &d), "reweight_resample");
        }
    }
    evaluated = 1;
}

/* writes reweight.bin and reweight.txt, with APEMOST_RESAMPLE_DRAWS also resample.bin and the resampled dumps, and
 * frees everything (the mbar fold's end has dropped the device's store) */
void run_reweight_close(const run_fold_ctx *ctx) {
    run_reweight *r = &reweight;
    if (evaluated) {
        const char *const *names = (const char *const *)get_params_descr(ctx->chains[0]);
        run_reweight_write(RUN_REWEIGHT_FILE, r);
        run_reweight_write_text(RUN_REWEIGHT_TEXT, r, names);
        if (n_draws > 0) {
            unsigned int t;
            run_resample_write(RUN_RESAMPLE_FILE, r, n_draws, draw_seed, draw_q_total, draw_index, draw_x);
            for (t = 0; t < r->n_t; t++)
                run_resample_write_dumps(r, t, n_draws, draw_x + (size_t)t * n_draws * r->n_cols, names);
        }
    }
    draws_free();
    run_reweight_free(r);
    is_open = evaluated = 0;
}
