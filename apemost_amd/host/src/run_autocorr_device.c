/* the device side of the APEMOST_DUMP token `autocorr` (run_autocorr.h): begin, resume, collect */
#include "run_autocorr.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mcmc_gettersetter.h"
#include "run_fold.h"

static run_autocorr autocorr;

static void autocorr_view(run_autocorr *r, apemost_hip_autocorr_view *v) {
    v->n = &r->n;
    v->origin = r->origin;
    v->sum = r->sum;
    v->lag = r->lag;
    v->head = r->head;
    v->tail = r->tail;
}

static unsigned int lags_from_env(void) {
    const char *text = getenv("APEMOST_AUTOCORR_LAGS");
    char *end;
    long v;
    if (text == NULL || *text == 0)
        return RUN_AUTOCORR_DEFAULT_LAGS;
    v = strtol(text, &end, 10);
    if (*end != 0 || v < 1 || v > 4096) {
        fprintf(stderr, "APEMOST_AUTOCORR_LAGS: expected a number of lags in 1 .. 4096; got '%s'\n", text);
        exit(1);
    }
    return (unsigned int)v;
}

/* begins the fold of chain 0: all parameters and prob - prior, max_lag from APEMOST_AUTOCORR_LAGS.  With c->append
 * autocorr.bin is loaded and the fold goes on from it; a file of another shape, max_lag or thin ends the program. */
void run_autocorr_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_autocorr *r = &autocorr;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const unsigned int n_par = get_n_par(ctx->chains[0]);
    const uint64_t thin = ctx->thin;
    const int append = ctx->append;
    const int32_t chain = 0;
    apemost_hip_autocorr_config c;
    apemost_hip_autocorr_view v;
    run_autocorr old;
    int found = -1;
    unsigned int p;
    (void)planned;
    memset(r, 0, sizeof *r);
    memset(&old, 0, sizeof old);
    r->n_par = n_par;
    r->n_cols = n_par + 1;
    r->max_lag = lags_from_env();
    r->thin = thin;
    r->chain = chain;
    run_autocorr_alloc(r);
    for (p = 0; p < n_par; p++)
        r->cols[p] = (int32_t)p;
    r->cols[n_par] = (int32_t)n_par + 1;
    if (append)
        found = run_autocorr_read(RUN_AUTOCORR_FILE, &old);
    if (found >= 0) {
        if (found != 0 || old.chain != 0 || old.n_par != n_par || old.n_cols != r->n_cols || old.max_lag != r->max_lag ||
            old.thin != thin || memcmp(old.cols, r->cols, r->n_cols * sizeof(int32_t)) != 0) {
            fprintf(stderr, "%s: written by a run of another shape (chains, parameters, APEMOST_AUTOCORR_LAGS or "
                            "thin:N); cannot append\n", RUN_AUTOCORR_FILE);
            exit(1);
        }
    } else if (append)
        fprintf(stderr, "--append: no %s, the autocorrelation starts with this run\n", RUN_AUTOCORR_FILE);
    c.n_keep = 1;
    c.chains = &chain;
    c.max_lag = (int32_t)r->max_lag;
    c.n_cols = 0;
    c.cols = NULL; /* the parameters and prob - prior, as written above */
    apemost_hip_or_die(apemost_hip_autocorr_begin(s, &c), "autocorr_begin");
    if (found == 0) {
        const size_t nc = r->n_cols, L = r->max_lag;
        r->n = old.n;
        memcpy(r->origin, old.origin, nc * sizeof(double));
        memcpy(r->sum, old.sum, nc * sizeof(double));
        memcpy(r->lag, old.lag, nc * L * sizeof(double));
        memcpy(r->head, old.head, nc * (L - 1) * sizeof(double));
        memcpy(r->tail, old.tail, nc * (L - 1) * sizeof(double));
        autocorr_view(r, &v);
        apemost_hip_or_die(apemost_hip_autocorr_set(s, &v), "autocorr_set");
        run_autocorr_free(&old);
    }
}

/* collects the accumulator, writes autocorr.bin and autocorr.txt, and frees everything */
void run_autocorr_close(const run_fold_ctx *ctx) {
    run_autocorr *r = &autocorr;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    apemost_hip_autocorr_view v;
    autocorr_view(r, &v);
    apemost_hip_or_die(apemost_hip_autocorr_get(s, &v), "autocorr_get");
    apemost_hip_or_die(apemost_hip_autocorr_end(s), "autocorr_end");
    run_autocorr_write(RUN_AUTOCORR_FILE, r);
    run_autocorr_write_text(RUN_AUTOCORR_TEXT, r, get_params_descr(ctx->chains[0]));
    run_autocorr_free(r);
}
