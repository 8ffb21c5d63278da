/* the device side of the APEMOST_DUMP token `derived` (run_derived.h): the derived file, begin, resume, collect */
#include "run_derived.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "mcmc_gettersetter.h"
#include "run_fold.h"
#include "run_io.h"

static run_derived derived;

static void derived_view(run_derived *r, apemost_hip_derived_view *v) {
    memset(v, 0, sizeof *v);
    v->n = &r->n;
    v->hist = r->hist;
    v->batch = r->batch;
    v->counts = r->counts;
    v->origin = r->origin;
    v->sum = r->sum;
    v->cross = r->cross;
    v->nonfinite = r->nonfinite;
    v->vmin = r->vmin;
    v->vmax = r->vmax;
}

static char *whole_file(const char *path) {
    FILE *f = fopen(path, "rb");
    char *text;
    long size;
    if (f == NULL) {
        fprintf(stderr, "APEMOST_DUMP=derived: cannot open the derived file '%s' (one line per column: name lo hi and "
                        "RPN tokens; APEMOST_DERIVED_FILE names another file)\n", path);
        exit(1);
    }
    fseek(f, 0, SEEK_END);
    size = ftell(f);
    fseek(f, 0, SEEK_SET);
    text = (char *)run_alloc_or_die((size_t)(size > 0 ? size : 0) + 1, 1, "derived quantities");
    run_read_or_die(text, 1, (size_t)(size > 0 ? size : 0), f, path, "derived file");
    fclose(f);
    return text;
}

/* reads and checks the derived file (a bad line ends the program with its number), then begins the fold of chain 0 for
 * `planned` more kept samples: c->nbins bins, batches of floor(sqrt(planned)).  With c->append derived.bin is loaded and
 * the accumulation goes on from it with its own batch size; a file of other columns, ranges, nbins or thin ends the
 * program with the messages a summary.bin of another shape gets. */
void run_derived_open(const run_fold_ctx *ctx, uint64_t planned) {
    run_derived *r = &derived;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    const unsigned int n_par = get_n_par(chain0), nbins = ctx->nbins;
    const uint64_t thin = ctx->thin;
    const int append = ctx->append;
    const char *path = getenv("APEMOST_DERIVED_FILE");
    const int32_t chain = 0;
    apemost_hip_derived_config c;
    apemost_hip_derived_view v;
    run_derived old;
    char message[RUN_DERIVED_MESSAGE];
    char *text;
    int resumed = 0, rc;
    unsigned int i, j, q = 0;
    uint64_t b;
    if (path == NULL || *path == 0)
        path = RUN_DERIVED_SPEC;
    text = whole_file(path);
    rc = run_derived_parse(text, n_par, get_params_descr(chain0), r, message);
    free(text);
    if (rc != 0) {
        fprintf(stderr, "%s: %s\n", path, message);
        exit(1);
    }
    memset(&old, 0, sizeof old);
    r->nbins = nbins;
    r->thin = thin;
    r->n_pairs = r->n_col <= RUN_DERIVED_PAIR_COLUMNS ? r->n_col * (r->n_col - 1) / 2 : 0;
    if (append && run_derived_read(RUN_DERIVED_FILE, &old) == 0) {
        int same = old.n_col == r->n_col && old.n_par == n_par && old.nbins == nbins && old.thin == thin &&
                   old.n_pairs == r->n_pairs;
        for (i = 0; same && i < r->n_col; i++)
            same = strcmp(old.names[i], r->names[i]) == 0 && strcmp(old.rpn[i], r->rpn[i]) == 0;
        for (i = 0; same && i < n_par; i++)
            same = strcmp(old.row_names[i], r->row_names[i]) == 0;
        if (!same) {
            fprintf(stderr, "%s: written by a run of another shape (columns, parameters, NBINS or thin:N); "
                            "cannot append\n", RUN_DERIVED_FILE);
            exit(1);
        }
        run_check_ranges_or_die(RUN_DERIVED_FILE, "column", r->n_col, old.lo, old.hi, r->lo, r->hi);
        resumed = 1;
    } else if (append)
        fprintf(stderr, "--append: no %s, the derived quantities start with this run\n", RUN_DERIVED_FILE);
    r->n = resumed ? old.n : 0;
    r->bs = run_batch_size(resumed, old.bs, planned);
    r->max_batches = run_batches_closed(r->n + planned, r->bs);
    r->pairs = (int32_t *)run_alloc_or_die((size_t)r->n_pairs * 2, sizeof(int32_t), "derived quantities");
    for (i = 0; i < r->n_col && r->n_pairs > 0; i++)
        for (j = i + 1; j < r->n_col; j++, q++) {
            r->pairs[2 * q] = (int32_t)i;
            r->pairs[2 * q + 1] = (int32_t)j;
        }
    run_derived_alloc(r);
    c.n_keep = 1;
    c.chains = &chain;
    c.n_col = (int32_t)r->n_col;
    c.code = r->code;
    c.start = r->start;
    c.n_const = (int32_t)r->n_const;
    c.consts = r->consts;
    c.nbins = (int32_t)nbins;
    c.n_pairs = (int32_t)r->n_pairs;
    c.pairs = r->pairs; /* (never NULL: an empty list is no pair, not all of them) */
    c.lo = r->lo;
    c.hi = r->hi;
    c.batch_size = r->bs;
    c.max_batches = r->max_batches;
    c.stage_steps = 0;
    apemost_hip_or_die(apemost_hip_derived_begin(s, &c), "derived_begin");
    if (resumed) {
        const size_t nc = r->n_col;
        memcpy(r->hist, old.hist, nc * nbins * sizeof(uint64_t));
        memcpy(r->nonfinite, old.nonfinite, nc * sizeof(uint64_t));
        memcpy(r->vmin, old.vmin, nc * sizeof(double));
        memcpy(r->vmax, old.vmax, nc * sizeof(double));
        memcpy(r->origin, old.origin, nc * sizeof(double));
        memcpy(r->sum, old.sum, nc * sizeof(double));
        memcpy(r->cross, old.cross, nc * (nc + 1) / 2 * sizeof(double));
        memcpy(r->counts, old.counts, (size_t)r->n_pairs * nbins * nbins * sizeof(uint64_t));
        for (i = 0; i < r->n_col; i++) /* closed batches and the open one, at the new capacity's stride */
            for (b = 0; b <= run_batches_closed(old.n, old.bs); b++)
                r->batch[(size_t)i * (size_t)(r->max_batches + 1) + b] = old.batch[(size_t)i * (size_t)(old.max_batches + 1) + b];
        derived_view(r, &v);
        apemost_hip_or_die(apemost_hip_derived_set(s, &v), "derived_set");
        run_derived_free(&old);
    }
}

/* collects the accumulator, writes derived.bin, derived.txt and the .histogram files, and frees everything */
void run_derived_close(const run_fold_ctx *ctx) {
    run_derived *r = &derived;
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    apemost_hip_derived_view v;
    derived_view(r, &v);
    apemost_hip_or_die(apemost_hip_derived_get(s, &v), "derived_get");
    apemost_hip_or_die(apemost_hip_derived_end(s), "derived_end");
    run_derived_write(RUN_DERIVED_FILE, r);
    run_derived_write_text(r);
    run_derived_free(r);
}
