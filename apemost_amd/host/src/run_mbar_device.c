/* the device side of the APEMOST_DUMP token `mbar` (run_mbar.h): begin, resume, and at the end the solve on the device */
#include "run_mbar.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parallel_tempering_beta.h"
#include "run_fold.h"
#include "run_io.h"

static run_mbar mbar;

static int device_iterate(void *ctx, uint64_t t0, uint64_t t_count, uint32_t n_iter, double *g, double *g_prev) {
    apemost_hip_or_die(apemost_hip_mbar_iterate((apemost_hip_sampler *)ctx, t0, t_count, n_iter, g, g_prev), "mbar_iterate");
    return 0;
}

static int device_evaluate(void *ctx, uint64_t t0, uint64_t t_count, const double *g, const double *betas_t, int n_t,
                           double *const words[6], double *ell_first) {
    apemost_hip_mbar_sums out;
    out.m = words[0];
    out.S0 = words[1];
    out.S1 = words[2];
    out.S2 = words[3];
    out.SS = words[4];
    out.G = words[5];
    out.ell_first = ell_first;
    apemost_hip_or_die(apemost_hip_mbar_evaluate((apemost_hip_sampler *)ctx, t0, t_count, g, betas_t, n_t, &out),
                       "mbar_evaluate");
    return 0;
}

/* the whole ladder on one device (run_folds_check has refused more than one shard); `planned` kept samples are still to
 * come.  With c->append mbar.bin is loaded and the store goes on from it; a file of another shape, thin or ladder ends
 * the program with the messages an evidence.bin of another shape gets. */
void run_mbar_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_mbar *r = &mbar;
    const unsigned int nc = ctx->lo[ctx->n_shards];
    apemost_hip_sampler *sampler = apemost_ladder_shard(ctx->l, 0);
    apemost_hip_mbar_config cfg;
    run_mbar old;
    int resumed = 0;
    unsigned int c;
    memset(&old, 0, sizeof old);
    memset(r, 0, sizeof *r);
    if (ctx->n_shards != 1) {
        fprintf(stderr, "APEMOST_DUMP=mbar needs the whole ladder on one device: the solve reads every chain\n");
        exit(1);
    }
    if (ctx->append && run_mbar_read(RUN_MBAR_FILE, &old) == 0) {
        if (old.n_chains != nc || old.thin != ctx->thin) {
            fprintf(stderr, "%s: written by a run of another shape (chains or thin:N); cannot append\n", RUN_MBAR_FILE);
            exit(1);
        }
        resumed = 1;
    } else if (ctx->append)
        fprintf(stderr, "--append: no %s, the mbar fold starts with this run\n", RUN_MBAR_FILE);
    r->n_chains = nc;
    r->thin = ctx->thin;
    r->betas = (double *)run_alloc_or_die(nc, sizeof(double), "mbar");
    for (c = 0; c < nc; c++) {
        r->betas[c] = get_beta(ctx->chains[c]);
        if (!(r->betas[c] > 0) || r->betas[c] - r->betas[c] != 0 || (c > 0 && !(r->betas[c] < r->betas[c - 1]))) {
            fprintf(stderr, "APEMOST_DUMP=mbar: beta of chain %u is %g; the betas must be positive and strictly "
                            "decreasing (with beta = 0 the column prob - prior is identically 0)\n", c, r->betas[c]);
            exit(1);
        }
        if (resumed && old.betas[c] != r->betas[c]) {
            fprintf(stderr, "%s: chain %u had beta %g, now %g; cannot append\n", RUN_MBAR_FILE, c, old.betas[c], r->betas[c]);
            exit(1);
        }
    }
    cfg.capacity = (resumed ? old.n : 0) + planned;
    cfg.betas = r->betas;
    apemost_hip_or_die(apemost_hip_mbar_begin(sampler, &cfg), "mbar_begin");
    if (resumed) {
        apemost_hip_mbar_view v;
        v.n = &old.n;
        v.n_bad = &old.n_bad;
        v.ell = old.ell;
        apemost_hip_or_die(apemost_hip_mbar_set(sampler, &v), "mbar_set");
        run_mbar_free(&old);
    }
}

/* collects the store, solves it on the device, writes mbar.bin and mbar.txt and frees everything.  A store with values
 * that are not finite, or a solve that does not converge, leaves mbar.bin unsolved and no mbar.txt, and says so. */
void run_mbar_close(const run_fold_ctx *ctx) {
    run_mbar *r = &mbar;
    apemost_hip_sampler *sampler = apemost_ladder_shard(ctx->l, 0);
    const double tol = run_mbar_tol_from_env();
    const unsigned long max_iter = run_mbar_iter_from_env();
    apemost_hip_mbar_view v;
    run_mbar_passes p;
    double *betas = r->betas, change;
    v.n = &r->n;
    v.n_bad = NULL;
    v.ell = NULL;
    apemost_hip_or_die(apemost_hip_mbar_get(sampler, &v), "mbar_get");
    r->betas = NULL;
    run_mbar_alloc(r);
    memcpy(r->betas, betas, r->n_chains * sizeof(double));
    free(betas);
    v.n_bad = &r->n_bad;
    v.ell = r->ell;
    apemost_hip_or_die(apemost_hip_mbar_get(sampler, &v), "mbar_get");
    p.ctx = sampler;
    p.iterate = device_iterate;
    p.evaluate = device_evaluate;
    if (r->n_bad != 0)
        fprintf(stderr, "APEMOST_DUMP=mbar: %lu stored values are not finite; %s holds the store, unsolved\n",
                (unsigned long)r->n_bad, RUN_MBAR_FILE);
    else if (r->n > 0) {
        run_mbar_start(r, 0, r->n, r->g);
        if (run_mbar_solve(r, &p, tol, max_iter, 0, r->n, r->g, &change) < 0) {
            fprintf(stderr, "APEMOST_DUMP=mbar: %lu iterations left a change of %g, above %g (APEMOST_MBAR_TOL, "
                            "APEMOST_MBAR_ITER); %s holds the store, unsolved\n", max_iter, change, tol, RUN_MBAR_FILE);
            memset(r->g, 0, r->n_chains * sizeof(double));
        } else {
            r->solved = 1;
            r->t0 = 0;
            r->t_count = r->n;
            run_mbar_write_text(RUN_MBAR_TEXT, r, &p, tol, max_iter);
        }
    }
    run_reweight_solved(ctx, r); /* (the token `reweight`: evaluated here, before the end drops its store) */
    apemost_hip_or_die(apemost_hip_mbar_end(sampler), "mbar_end");
    run_mbar_write(RUN_MBAR_FILE, r);
    run_mbar_free(r);
}
