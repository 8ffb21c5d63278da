/* the device side of the APEMOST_DUMP token `evidence` (run_evidence.h): begin, resume, collect, one fold per shard */
#include "run_evidence.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "parallel_tempering_beta.h"
#include "run_fold.h"
#include "run_io.h"

#define alloc_or_die(count) ((double *)run_alloc_or_die(count, sizeof(double), "evidence"))

static run_evidence evidence;

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

/* begins one fold per shard of the ladder (shard j holds chains [lo[j], lo[j+1])), the coefficients sliced from the
 * whole ladder's betas, which must be positive and strictly decreasing.  `planned` kept samples are still to come; the
 * batch size is floor(sqrt(planned)).  With c->append evidence.bin is loaded and the fold goes on from it with its own
 * batch size; a file of another shape, thin or ladder ends the program with the messages a summary.bin of another
 * shape gets. */
void run_evidence_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_evidence *r = &evidence;
    const unsigned int *lo = ctx->lo;
    const unsigned int nc = lo[ctx->n_shards];
    run_evidence old;
    uint32_t old_ladders = 0;
    int resumed = 0;
    unsigned int c, j, s;
    uint64_t b;
    double *ms;
    memset(&old, 0, sizeof old);
    memset(r, 0, sizeof *r);
    if (ctx->append && run_evidence_read(RUN_EVIDENCE_FILE, &old, &old_ladders) == 0) {
        if (old.n_chains != nc || old_ladders != 1 || old.thin != ctx->thin) {
            fprintf(stderr, "%s: written by a run of another shape (chains or thin:N); cannot append\n", RUN_EVIDENCE_FILE);
            exit(1);
        }
        resumed = 1;
    } else if (ctx->append)
        fprintf(stderr, "--append: no %s, the evidence fold starts with this run\n", RUN_EVIDENCE_FILE);
    r->n_chains = nc;
    r->thin = ctx->thin;
    r->n = resumed ? old.n : 0;
    r->bs = run_batch_size(resumed, old.bs, planned);
    r->max_batches = run_batches_closed(r->n + planned, r->bs);
    run_evidence_alloc(r);
    for (c = 0; c < nc; c++) {
        r->betas[c] = get_beta(ctx->chains[c]);
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
            for (b = 0; b <= run_batches_closed(old.n, old.bs); b++)
                r->batch[(size_t)c * (size_t)(r->max_batches + 1) + b] = old.batch[(size_t)c * (size_t)(old.max_batches + 1) + b];
        run_evidence_free(&old);
    }
    ms = alloc_or_die(4 * (size_t)nc);
    for (j = 0; j < ctx->n_shards; j++) {
        apemost_hip_sampler *sampler = apemost_ladder_shard(ctx->l, j);
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

/* collects the shards' accumulators, writes evidence.bin and evidence.txt, and frees everything */
void run_evidence_close(const run_fold_ctx *ctx) {
    run_evidence *r = &evidence;
    const unsigned int *lo = ctx->lo;
    const unsigned int nc = r->n_chains;
    double *ms = alloc_or_die(4 * (size_t)nc);
    unsigned int j, s;
    for (j = 0; j < ctx->n_shards; j++) {
        apemost_hip_sampler *sampler = apemost_ladder_shard(ctx->l, j);
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
    run_evidence_write(RUN_EVIDENCE_FILE, r);
    run_evidence_write_text(RUN_EVIDENCE_TEXT, r);
    run_evidence_free(r);
}
