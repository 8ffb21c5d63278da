/* the device side of the APEMOST_DUMP token `pointwise` (run_pointwise.h): begin, resume, collect */
#include "run_pointwise.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mcmc_gettersetter.h"
#include "run_fold.h"
#include "run_io.h"

static run_pointwise pointwise;

static void pointwise_view(run_pointwise *r, apemost_hip_pointwise_view *v) {
    v->n = &r->n;
    v->origin = r->state[0];
    v->sum = r->state[1];
    v->sq = r->state[2];
    v->m_up = r->state[3];
    v->S_up = r->state[4];
    v->m_dn = r->state[5];
    v->S_dn = r->state[6];
    v->S2_dn = r->state[7];
    v->par_origin = r->par_origin;
    v->par_sum = r->par_sum;
}

int run_pointwise_tail_from_env(void) {
    const char *text = getenv("APEMOST_POINTWISE_TAIL");
    char *end;
    long v;
    if (text == NULL || *text == 0)
        return 0;
    if (strcmp(text, "auto") == 0)
        return -1;
    v = strtol(text, &end, 10);
    if (*end != 0 || v < 2 || v > 4096) {
        fprintf(stderr, "APEMOST_POINTWISE_TAIL: expected auto or a capacity in 2 .. 4096; got '%s'\n", text);
        exit(1);
    }
    return (int)v;
}

/* begins the tail on the fold just begun (and, resuming, just set); `resumed`: pointwise.bin was loaded */
static void tail_open(run_pointwise *r, apemost_hip_sampler *s, int asked, int resumed, uint64_t planned) {
    apemost_hip_pointwise_tail_view v;
    run_pointwise_tail old;
    int found = -1;
    memset(&old, 0, sizeof old);
    if (resumed) {
        found = run_pointwise_tail_read(RUN_POINTWISE_TAIL_FILE, &old);
        if (found < 0) {
            fprintf(stderr, "--append: %s holds %lu samples but there is no %s: their tail is lost; cannot append with "
                            "APEMOST_POINTWISE_TAIL\n", RUN_POINTWISE_FILE, (unsigned long)r->n, RUN_POINTWISE_TAIL_FILE);
            exit(1);
        }
        if (found != 0 || old.chain != 0 || old.n_data != r->n_data || old.n != r->n || old.thin != r->thin ||
            (asked > 0 && old.capacity != (uint32_t)asked)) {
            fprintf(stderr, "%s: written by a run of another shape (data, capacity, thin:N, or not the samples of %s); "
                            "cannot append\n", RUN_POINTWISE_TAIL_FILE, RUN_POINTWISE_FILE);
            exit(1);
        }
    }
    r->tail.n_data = r->n_data;
    r->tail.capacity = found == 0 ? old.capacity : asked > 0 ? (uint32_t)asked : run_pointwise_tail_capacity_for(planned);
    r->tail.chain = 0;
    r->tail.thin = r->thin;
    run_pointwise_tail_alloc(&r->tail);
    apemost_hip_or_die(apemost_hip_pointwise_tail_begin(s, (int32_t)r->tail.capacity), "pointwise_tail_begin");
    if (found == 0) {
        v.count = old.count;
        v.values = old.values;
        apemost_hip_or_die(apemost_hip_pointwise_tail_set(s, &v), "pointwise_tail_set");
        run_pointwise_tail_free(&old);
    }
}

/* begins the fold of chain 0 over its data.  With c->append pointwise.bin is loaded and the fold goes on from it; a file
 * of another shape, data, sigma or thin ends the program.  APEMOST_POINTWISE_TAIL begins the tail as well (`planned`
 * kept samples size it under auto); with c->append pointwise_tail.bin is loaded, and one of another shape, capacity or
 * sample count than pointwise.bin's ends the program. */
void run_pointwise_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_pointwise *r = &pointwise;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    const int model = ctx->model, append = ctx->append;
    const double sigma = ctx->sigma;
    const uint64_t thin = ctx->thin;
    const int32_t chain = 0;
    const int tail = run_pointwise_tail_from_env();
    apemost_hip_pointwise_config c;
    apemost_hip_pointwise_view v;
    run_pointwise old;
    int found = -1, q;
    uint32_t i;
    memset(r, 0, sizeof *r);
    memset(&old, 0, sizeof old);
    r->n_par = get_n_par(chain0);
    r->n_data = (uint32_t)chain0->data->size1;
    r->model = (uint32_t)model;
    r->sigma = sigma;
    r->thin = thin;
    r->chain = chain;
    if (model == APEMOST_MODEL_USER) { /* the term is the device model's optional hook */
        int32_t has_pointwise = 0;
        apemost_hip_or_die(apemost_hip_user_hooks(s, NULL, &has_pointwise, NULL), "user_hooks");
        if (!has_pointwise) {
            fprintf(stderr, "APEMOST_DUMP=pointwise: the device model of APEMOST_DEVICE_MODEL_SRC has no datum's term: "
                            "define APEMOST_USER_POINTWISE and apemost_user_pointwise() in it "
                            "(include/apemost_device_model.h)\n");
            exit(1);
        }
    }
    run_pointwise_alloc(r);
    for (i = 0; i < r->n_data; i++) { /* (the file's x and y; a user model's term sees every column) */
        r->x[i] = gsl_matrix_get(chain0->data, i, 0);
        r->y[i] = gsl_matrix_get(chain0->data, i, 1);
    }
    if (append)
        found = run_pointwise_read(RUN_POINTWISE_FILE, &old);
    if (found >= 0) {
        if (found != 0 || old.chain != 0 || old.n_par != r->n_par || old.n_data != r->n_data || old.model != r->model ||
            old.thin != thin || old.sigma != sigma || memcmp(old.x, r->x, r->n_data * sizeof(double)) != 0 ||
            memcmp(old.y, r->y, r->n_data * sizeof(double)) != 0) {
            fprintf(stderr, "%s: written by a run of another shape (model, parameters, data, sigma or thin:N); cannot "
                            "append\n", RUN_POINTWISE_FILE);
            exit(1);
        }
    } else if (append)
        fprintf(stderr, "--append: no %s, the pointwise log-likelihood starts with this run\n", RUN_POINTWISE_FILE);
    c.n_keep = 1;
    c.chains = &chain;
    apemost_hip_or_die(apemost_hip_pointwise_begin(s, &c), "pointwise_begin");
    if (found == 0) {
        r->n = old.n;
        for (q = 0; q < RUN_POINTWISE_WORDS; q++)
            memcpy(r->state[q], old.state[q], r->n_data * sizeof(double));
        memcpy(r->par_origin, old.par_origin, r->n_par * sizeof(double));
        memcpy(r->par_sum, old.par_sum, r->n_par * sizeof(double));
        pointwise_view(r, &v);
        apemost_hip_or_die(apemost_hip_pointwise_set(s, &v), "pointwise_set");
        run_pointwise_free(&old);
    }
    if (tail != 0)
        tail_open(r, s, tail, found == 0, planned);
}

/* collects the accumulator, evaluates the term at the mean parameters on the device, writes the three files, and
 * frees everything */
void run_pointwise_close(const run_fold_ctx *ctx) {
    run_pointwise *r = &pointwise;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    apemost_hip_pointwise_view v;
    double *mean = (double *)run_alloc_or_die(r->n_par, sizeof(double), "pointwise");
    uint32_t p;
    pointwise_view(r, &v);
    apemost_hip_or_die(apemost_hip_pointwise_get(s, &v), "pointwise_get");
    if (r->tail.capacity > 0) {
        apemost_hip_pointwise_tail_view tv;
        tv.count = r->tail.count;
        tv.values = r->tail.values;
        apemost_hip_or_die(apemost_hip_pointwise_tail_get(s, &tv), "pointwise_tail_get");
        r->tail.n = r->n;
        run_pointwise_tail_write(RUN_POINTWISE_TAIL_FILE, &r->tail);
    }
    apemost_hip_or_die(apemost_hip_pointwise_end(s), "pointwise_end");
    /* the term at the posterior mean parameters, by the same device code (left NaN before there is a sample) */
    if (r->n > 0) {
        for (p = 0; p < r->n_par; p++) {
            const double t = r->par_sum[p] / (double)r->n;
            mean[p] = r->par_origin[p] + t;
        }
        apemost_hip_or_die(apemost_hip_pointwise_loglike(s, 1, mean, r->at_mean), "pointwise_loglike");
    }
    run_pointwise_write(RUN_POINTWISE_FILE, r);
    run_pointwise_write_text(RUN_POINTWISE_TEXT, r);
    run_pointwise_write_criteria(RUN_POINTWISE_CRITERIA, r);
    free(mean);
    run_pointwise_free(r);
}
