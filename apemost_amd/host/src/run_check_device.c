/* the device side of the APEMOST_DUMP token `check` (run_check.h): begin, resume, collect */
#include "run_check.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "run_fold.h"
#include "run_io.h"

static run_check check;

static void check_view(run_check *r, apemost_hip_check_view *v) {
    memset(v, 0, sizeof *v);
    v->n = &r->n;
    v->origin = r->state[0];
    v->sum = r->state[1];
    v->sq = r->state[2];
    v->sum_u = r->state[3];
    v->m = r->state[4];
    v->S = r->state[5];
    v->SU = r->state[6];
    v->stat_origin = r->stat[0];
    v->stat_sum = r->stat[1];
    v->stat_sq = r->stat[2];
    v->stat_min = r->stat[3];
    v->stat_max = r->stat[4];
    v->counts = r->counts;
}

int run_check_bins_from_env(void) {
    const char *e = getenv("APEMOST_CHECK_BINS");
    char *end;
    long v;
    if (e == NULL || *e == 0)
        return 256;
    v = strtol(e, &end, 10);
    if (*end != 0 || v < 1 || v > APEMOST_CHECK_MAX_EDGES + 1) {
        fprintf(stderr, "APEMOST_CHECK_BINS: expected a number of slots in 1 .. %d (1: no histogram), got '%s'\n",
                APEMOST_CHECK_MAX_EDGES + 1, e);
        exit(1);
    }
    return (int)v;
}

/* begins the fold of chain 0 over the null quantiles of its data's length; with c->append check.bin is loaded, and one
 * of another shape or other edges ends the program */
void run_check_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_check *r = &check;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    const int32_t chain = 0;
    apemost_hip_check_view v;
    run_check old;
    int found = -1, q;
    uint32_t i;
    (void)planned;
    memset(r, 0, sizeof *r);
    memset(&old, 0, sizeof old);
    if (ctx->model == APEMOST_MODEL_USER) {
        fprintf(stderr, "APEMOST_DUMP=check: the device model of APEMOST_DEVICE_MODEL_SRC has no predictive CDF: the "
                        "checks need a built-in model\n");
        exit(1);
    }
    r->n_data = (uint32_t)chain0->data->size1;
    r->n_edges = (uint32_t)run_check_bins_from_env() - 1;
    r->model = (uint32_t)ctx->model;
    r->sigma = ctx->sigma;
    r->thin = ctx->thin;
    r->chain = chain;
    run_check_alloc(r);
    for (i = 0; i < r->n_data; i++) {
        r->x[i] = gsl_matrix_get(chain0->data, i, 0);
        r->y[i] = gsl_matrix_get(chain0->data, i, 1);
    }
    for (q = 0; q < RUN_CHECK_N_STATS && r->n_edges > 0; q++)
        apemost_hip_or_die(apemost_hip_check_null_edges(ctx->model, q, (int32_t)r->n_data, (int32_t)r->n_edges,
                                                        r->edges + (size_t)q * r->n_edges), "check_null_edges");
    if (ctx->append)
        found = run_check_read(RUN_CHECK_FILE, &old);
    if (found >= 0) {
        if (found != 0 || old.chain != 0 || old.n_data != r->n_data || old.n_edges != r->n_edges || old.model != r->model ||
            old.thin != r->thin || old.sigma != r->sigma || memcmp(old.x, r->x, r->n_data * sizeof(double)) != 0 ||
            memcmp(old.y, r->y, r->n_data * sizeof(double)) != 0 ||
            memcmp(old.edges, r->edges, (size_t)RUN_CHECK_N_STATS * r->n_edges * sizeof(double)) != 0) {
            fprintf(stderr, "%s: written by a run of another shape (model, data, sigma, thin:N or APEMOST_CHECK_BINS); "
                            "cannot append\n", RUN_CHECK_FILE);
            exit(1);
        }
    } else if (ctx->append)
        fprintf(stderr, "--append: no %s, the predictive checks start with this run\n", RUN_CHECK_FILE);
    apemost_hip_or_die(apemost_hip_check_begin(s, 1, &chain, (int32_t)r->n_edges, r->n_edges > 0 ? r->edges : NULL),
                       "check_begin");
    if (found == 0) {
        r->n = old.n;
        for (q = 0; q < RUN_CHECK_WORDS; q++)
            memcpy(r->state[q], old.state[q], r->n_data * sizeof(double));
        for (q = 0; q < RUN_CHECK_STAT_WORDS; q++)
            memcpy(r->stat[q], old.stat[q], RUN_CHECK_N_STATS * sizeof(double));
        memcpy(r->counts, old.counts, (size_t)RUN_CHECK_N_STATS * (r->n_edges + 2) * sizeof(uint64_t));
        check_view(r, &v);
        apemost_hip_or_die(apemost_hip_check_set(s, &v), "check_set");
        run_check_free(&old);
    }
}

/* collects the accumulator, writes the three files, and frees everything */
void run_check_close(const run_fold_ctx *ctx) {
    run_check *r = &check;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    apemost_hip_check_view v;
    check_view(r, &v);
    apemost_hip_or_die(apemost_hip_check_get(s, &v), "check_get");
    apemost_hip_or_die(apemost_hip_check_end(s), "check_end");
    run_check_write(RUN_CHECK_FILE, r);
    run_check_write_text(RUN_CHECK_TEXT, r);
    run_check_write_stats(RUN_CHECK_STATS, r);
    run_check_free(r);
}
