/* the device side of the APEMOST_DUMP token `joint` (run_joint.h): begin, resume, collect */
#include "run_joint.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mcmc_gettersetter.h"
#include "run_fold.h"
#include "run_io.h"

static run_joint joint;

static void joint_view(run_joint *r, apemost_hip_joint_view *v) {
    v->n = &r->n;
    v->counts = r->counts;
    v->origin = r->origin;
    v->sum = r->sum;
    v->cross = r->cross;
}

/* begins the joint marginals of chain 0: all pairs, c->nbins bins, the prior box of the chain.  With c->append joint.bin
 * is loaded and the accumulation goes on from it; a file of another shape, nbins, thin or range ends the program with
 * the messages a summary.bin of another shape gets. */
void run_joint_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_joint *r = &joint;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    const unsigned int n_par = get_n_par(chain0), nbins = ctx->nbins;
    const int32_t chain = 0;
    apemost_hip_joint_config c;
    apemost_hip_joint_view v;
    run_joint old;
    uint32_t old_keep = 0;
    int32_t old_chain = -1;
    int resumed = 0;
    unsigned int i, j, p, q = 0;
    (void)planned;
    memset(&old, 0, sizeof old);
    memset(r, 0, sizeof *r);
    r->n_par = n_par;
    r->nbins = nbins;
    r->n_pairs = n_par * (n_par - 1) / 2;
    r->thin = ctx->thin;
    if (ctx->append && run_joint_read(RUN_JOINT_FILE, &old, &old_keep, &old_chain) == 0) {
        if (old_keep != 1 || old_chain != 0 || old.n_par != n_par || old.nbins != nbins || old.thin != r->thin ||
            old.n_pairs != r->n_pairs) {
            fprintf(stderr, "%s: written by a run of another shape (chains, parameters, NBINS or thin:N); "
                            "cannot append\n", RUN_JOINT_FILE);
            exit(1);
        }
        resumed = 1;
    } else if (ctx->append)
        fprintf(stderr, "--append: no %s, the joint marginals start with this run\n", RUN_JOINT_FILE);
    run_joint_alloc(r);
    for (i = 0; i < n_par; i++)
        for (j = i + 1; j < n_par; j++, q++) {
            r->pairs[2 * q] = (int32_t)i;
            r->pairs[2 * q + 1] = (int32_t)j;
        }
    for (p = 0; p < n_par; p++) {
        r->lo[p] = get_params_min_for(chain0, p);
        r->hi[p] = get_params_max_for(chain0, p);
    }
    if (resumed)
        run_check_ranges_or_die(RUN_JOINT_FILE, "parameter", n_par, old.lo, old.hi, r->lo, r->hi);
    if (resumed && memcmp(old.pairs, r->pairs, (size_t)r->n_pairs * 2 * sizeof(int32_t)) != 0) {
        fprintf(stderr, "%s: written by a run of another shape (chains, parameters, NBINS or thin:N); "
                        "cannot append\n", RUN_JOINT_FILE);
        exit(1);
    }
    c.n_keep = 1;
    c.chains = &chain;
    c.nbins = (int32_t)nbins;
    c.n_pairs = 0;
    c.pairs = NULL; /* all pairs, in the order written above */
    c.lo = r->lo;
    c.hi = r->hi;
    apemost_hip_or_die(apemost_hip_joint_begin(s, &c), "joint_begin");
    if (resumed) {
        r->n = old.n;
        memcpy(r->origin, old.origin, n_par * sizeof(double));
        memcpy(r->sum, old.sum, n_par * sizeof(double));
        memcpy(r->cross, old.cross, run_tri_count(n_par) * sizeof(double));
        memcpy(r->counts, old.counts, (size_t)r->n_pairs * nbins * nbins * sizeof(uint64_t));
        joint_view(r, &v);
        apemost_hip_or_die(apemost_hip_joint_set(s, &v), "joint_set");
    }
    if (old.lo != NULL)
        run_joint_free(&old);
}

/* collects the accumulator, writes joint.bin, the .joint files and correlation.matrix, and frees everything */
void run_joint_close(const run_fold_ctx *ctx) {
    run_joint *r = &joint;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const char **names = get_params_descr(ctx->chains[0]);
    apemost_hip_joint_view v;
    unsigned int q;
    joint_view(r, &v);
    apemost_hip_or_die(apemost_hip_joint_get(s, &v), "joint_get");
    apemost_hip_or_die(apemost_hip_joint_end(s), "joint_end");
    run_joint_write(RUN_JOINT_FILE, r);
    for (q = 0; q < r->n_pairs; q++)
        run_joint_write_pair(r, q, names);
    run_joint_write_correlation(r);
    run_joint_free(r);
}
