/* the device side of the APEMOST_DUMP token `predict` (run_predict.h): begin, resume, collect */
#include "run_predict.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mcmc_gettersetter.h"
#include "run_fold.h"
#include "run_io.h"

static run_predict predict;

static void predict_view(run_predict *r, apemost_hip_predict_view *v) {
    v->n = &r->n;
    v->origin = r->origin;
    v->sum = r->sum;
    v->sq = r->sq;
    v->vmin = r->vmin;
    v->vmax = r->vmax;
    v->hist = r->nbins > 0 ? r->hist : NULL;
    v->best_prob = &r->best_prob;
    v->best_params = r->best_params;
    v->best_n = &r->best_n;
}

/* histograms only when APEMOST_PREDICT_BINS=N and APEMOST_PREDICT_RANGE=lo:hi are both set */
static void bins_from_env(run_predict *r) {
    const char *bins = getenv("APEMOST_PREDICT_BINS"), *range = getenv("APEMOST_PREDICT_RANGE");
    char *end;
    long v;
    r->nbins = 0;
    r->lo = r->hi = 0.0;
    if (bins == NULL || *bins == 0 || range == NULL || *range == 0)
        return;
    v = strtol(bins, &end, 10);
    if (*end != 0 || v < 1 || v > 4096) {
        fprintf(stderr, "APEMOST_PREDICT_BINS: expected a number of bins in 1 .. 4096; got '%s'\n", bins);
        exit(1);
    }
    r->nbins = (uint32_t)v;
    r->lo = strtod(range, &end);
    if (end == range || *end != ':') {
        fprintf(stderr, "APEMOST_PREDICT_RANGE: expected lo:hi; got '%s'\n", range);
        exit(1);
    }
    range = end + 1;
    r->hi = strtod(range, &end);
    if (end == range || *end != 0 || !(r->lo < r->hi)) {
        fprintf(stderr, "APEMOST_PREDICT_RANGE: expected lo:hi with lo < hi; got '%s'\n", getenv("APEMOST_PREDICT_RANGE"));
        exit(1);
    }
}

/* begins the fold of chain 0 over column 0 of its data; histograms when APEMOST_PREDICT_BINS and APEMOST_PREDICT_RANGE
 * are both set.  With c->append predict.bin is loaded and the fold goes on from it; a file of another shape, range or
 * thin ends the program.  (The bounded run is needed for the refusal alone: `planned` sizes nothing.) */
void run_predict_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_predict *r = &predict;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    const int model = ctx->model, append = ctx->append;
    const uint64_t thin = ctx->thin;
    const int32_t chain = 0;
    apemost_hip_predict_config c;
    apemost_hip_predict_view v;
    run_predict old;
    int found = -1;
    uint32_t i;
    (void)planned;
    memset(r, 0, sizeof *r);
    memset(&old, 0, sizeof old);
    r->n_par = get_n_par(chain0);
    r->n_x = (uint32_t)chain0->data->size1;
    r->model = (uint32_t)model;
    r->thin = thin;
    r->chain = chain;
    if (model == APEMOST_MODEL_USER) { /* the curve is the device model's optional hook */
        int32_t has_curve = 0;
        apemost_hip_or_die(apemost_hip_user_hooks(s, &has_curve, NULL, NULL), "user_hooks");
        if (!has_curve) {
            fprintf(stderr, "APEMOST_DUMP=predict: the device model of APEMOST_DEVICE_MODEL_SRC has no curve: define "
                            "APEMOST_USER_CURVE and apemost_user_curve() in it (include/apemost_device_model.h)\n");
            exit(1);
        }
    }
    bins_from_env(r);
    run_predict_alloc(r);
    for (i = 0; i < r->n_x; i++)
        r->x[i] = gsl_matrix_get(chain0->data, i, 0);
    if (append)
        found = run_predict_read(RUN_PREDICT_FILE, &old);
    if (found >= 0) {
        if (found != 0 || old.chain != 0 || old.n_par != r->n_par || old.n_x != r->n_x || old.nbins != r->nbins ||
            old.model != r->model || old.thin != thin || old.lo != r->lo || old.hi != r->hi ||
            memcmp(old.x, r->x, r->n_x * sizeof(double)) != 0) {
            fprintf(stderr, "%s: written by a run of another shape (model, parameters, data, APEMOST_PREDICT_BINS, "
                            "APEMOST_PREDICT_RANGE or thin:N); cannot append\n", RUN_PREDICT_FILE);
            exit(1);
        }
    } else if (append)
        fprintf(stderr, "--append: no %s, the posterior predictive starts with this run\n", RUN_PREDICT_FILE);
    c.n_keep = 1;
    c.chains = &chain;
    c.n_x = 0;
    c.x = NULL; /* column 0 of the data, as copied above (a user model: the data's rows) */
    c.nbins = (int32_t)r->nbins;
    c.lo = r->lo;
    c.hi = r->hi;
    apemost_hip_or_die(apemost_hip_predict_begin(s, &c), "predict_begin");
    if (found == 0) {
        const size_t nx = r->n_x;
        r->n = old.n;
        memcpy(r->origin, old.origin, nx * sizeof(double));
        memcpy(r->sum, old.sum, nx * sizeof(double));
        memcpy(r->sq, old.sq, nx * sizeof(double));
        memcpy(r->vmin, old.vmin, nx * sizeof(double));
        memcpy(r->vmax, old.vmax, nx * sizeof(double));
        memcpy(r->hist, old.hist, nx * r->nbins * sizeof(uint64_t));
        r->best_prob = old.best_prob;
        memcpy(r->best_params, old.best_params, r->n_par * sizeof(double));
        r->best_n = old.best_n;
        predict_view(r, &v);
        apemost_hip_or_die(apemost_hip_predict_set(s, &v), "predict_set");
        run_predict_free(&old);
    }
}

/* collects the accumulator, evaluates the best-fit curve on the device, writes predict.bin and predict.txt, and frees
 * everything */
void run_predict_close(const run_fold_ctx *ctx) {
    run_predict *r = &predict;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    apemost_hip_predict_view v;
    double *y = (double *)run_alloc_or_die(r->n_x, sizeof(double), "predict");
    double *best = (double *)run_alloc_or_die(r->n_x, sizeof(double), "predict");
    uint32_t i;
    predict_view(r, &v);
    apemost_hip_or_die(apemost_hip_predict_get(s, &v), "predict_get");
    apemost_hip_or_die(apemost_hip_predict_end(s), "predict_end");
    for (i = 0; i < r->n_x; i++)
        y[i] = gsl_matrix_get(chain0->data, i, 1);
    /* the best fit: the same device curve for the best sample's parameters (zeros before there is one); a user
     * model's curve takes whole rows: the data's own (x = NULL) */
    apemost_hip_or_die(apemost_hip_predict_curve(s, 1, r->best_params, (int32_t)r->n_x,
                                                 r->model == APEMOST_MODEL_USER ? NULL : r->x, best), "predict_curve");
    run_predict_write(RUN_PREDICT_FILE, r);
    run_predict_write_text(RUN_PREDICT_TEXT, r, y, best);
    free(y);
    free(best);
    run_predict_free(r);
}
