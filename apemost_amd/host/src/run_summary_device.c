/* the device side of the APEMOST_DUMP token `summary` (run_summary.h): begin, resume, collect, one summary per shard */
#include "run_summary.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mcmc_gettersetter.h"
#include "run_fold.h"
#include "run_io.h"

static run_summary summary;

/* the view of shard j: every shard its slice of prob_sum, shard 0 chain 0's histograms as well */
static void summary_view(run_summary *r, apemost_hip_summary_view *v, const unsigned int *lo, unsigned int j,
                         uint64_t *n_batches) {
    v->n = &r->n;
    v->prob_sum = r->prob_sum + lo[j];
    v->hist = j == 0 ? r->hist : NULL;
    v->batch_sums = j == 0 ? r->batch_sums : NULL;
    v->n_batches = j == 0 ? n_batches : NULL;
}

/* One device summary per shard (chain 0's histograms on shard 0).  The batch size of the error estimate is
 * floor(sqrt(samples planned)); --append loads summary.bin and keeps its own. */
void run_summary_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_summary *r = &summary;
    const unsigned int *lo = ctx->lo;
    const unsigned int n_beta = lo[ctx->n_shards], n_par = get_n_par(ctx->chains[0]), nbins = ctx->nbins;
    uint64_t b;
    run_summary old;
    int resumed = 0;
    unsigned int j, p;
    memset(&old, 0, sizeof old);
    memset(r, 0, sizeof *r);
    if (ctx->append && run_summary_read(RUN_SUMMARY_FILE, &old) == 0) {
        if (old.n_beta != n_beta || old.n_par != n_par || old.nbins != nbins || old.thin != ctx->thin || old.n_hist != 1) {
            fprintf(stderr, "%s: written by a run of another shape (chains, parameters, NBINS or thin:N); "
                            "cannot append\n", RUN_SUMMARY_FILE);
            exit(1);
        }
        resumed = 1;
    } else if (ctx->append)
        fprintf(stderr, "--append: no %s, the summary starts with this run\n", RUN_SUMMARY_FILE);
    r->n_beta = n_beta;
    r->n_par = n_par;
    r->nbins = nbins;
    r->n_hist = 1;
    r->thin = ctx->thin;
    r->n = resumed ? old.n : 0;
    r->bs = run_batch_size(resumed, old.bs, planned);
    r->max_batches = run_batches_closed(r->n + planned, r->bs);
    run_summary_alloc(r);
    for (p = 0; p < n_par; p++) {
        r->lo[p] = get_params_min_for(ctx->chains[0], p);
        r->hi[p] = get_params_max_for(ctx->chains[0], p);
    }
    if (resumed) {
        run_check_ranges_or_die(RUN_SUMMARY_FILE, "parameter", n_par, old.lo, old.hi, r->lo, r->hi);
        memcpy(r->prob_sum, old.prob_sum, n_beta * sizeof(double));
        memcpy(r->hist, old.hist, (size_t)n_par * nbins * sizeof(uint64_t));
        for (p = 0; p < n_par; p++) /* closed batches and the open one, at the new capacity's stride */
            for (b = 0; b <= old.n_batches; b++)
                r->batch_sums[p * (r->max_batches + 1) + b] = old.batch_sums[p * (old.max_batches + 1) + b];
        run_summary_free(&old);
    }
    r->n_batches = run_batches_closed(r->n, r->bs);
    for (j = 0; j < ctx->n_shards; j++) {
        apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, j);
        apemost_hip_summary_config c;
        apemost_hip_summary_view v;
        c.n_hist_chains = j == 0 ? 1 : 0;
        c.nbins = nbins;
        c.batch_size = r->bs;
        c.max_batches = r->max_batches;
        c.lo = r->lo;
        c.hi = r->hi;
        apemost_hip_or_die(apemost_hip_summary_begin(s, &c), "summary_begin");
        if (resumed) {
            summary_view(r, &v, lo, j, NULL);
            apemost_hip_or_die(apemost_hip_summary_set(s, &v), "summary_set");
        }
    }
}

/* collects the shards' summaries into summary.bin */
void run_summary_close(const run_fold_ctx *ctx) {
    run_summary *r = &summary;
    unsigned int j;
    for (j = 0; j < ctx->n_shards; j++) {
        apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, j);
        apemost_hip_summary_view v;
        summary_view(r, &v, ctx->lo, j, &r->n_batches);
        apemost_hip_or_die(apemost_hip_summary_get(s, &v), "summary_get");
        apemost_hip_or_die(apemost_hip_summary_end(s), "summary_end");
    }
    run_summary_write(RUN_SUMMARY_FILE, r);
    run_summary_free(r);
}
