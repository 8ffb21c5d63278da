/* <paramname>.peaks: the APEMOST_DUMP token `peaks` (include/apemost_hip.h, apemost_hip_peaks_*).  The run phase
 * keeps chain 0's parameter columns on the device and leaves, per parameter, the output of the reference's
 * `peaks.exe min max <paramname>-chain-0.prob.dump` over the parameter's prior box [min, max] -- the analysis its
 * manual prefers to reading the marginal histograms -- without the sample dump having been written. */
#include <stdio.h>
#include <stdlib.h>

#include "mcmc_gettersetter.h"
#include "memory.h"
#include "run_fold.h"
#include "run_io.h"

#define PEAKS_MAX 99

/* begins peaks for chain 0 over its prior box, for `planned` kept samples.  With c->append one line on stderr says
 * that the files will cover this run's samples only. */
void run_peaks_open(const run_fold_ctx *ctx, uint64_t planned) {
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    const unsigned int n_par = get_n_par(chain0);
    const int32_t chain = 0;
    double *lo = (double *)mem_calloc(n_par, sizeof(double)), *hi = (double *)mem_calloc(n_par, sizeof(double));
    apemost_hip_peaks_config c;
    unsigned int p;
    for (p = 0; p < n_par; p++) {
        lo[p] = get_params_min_for(chain0, p);
        hi[p] = get_params_max_for(chain0, p);
    }
    if (ctx->append)
        fprintf(stderr, "--append: the .peaks files cover the samples of this run only\n");
    c.n_keep = 1;
    c.chains = &chain;
    c.capacity = planned > 0 ? planned : 1;
    c.lo = lo;
    c.hi = hi;
    apemost_hip_or_die(apemost_hip_peaks_begin(s, &c), "peaks_begin");
    mem_free(lo);
    mem_free(hi);
}

/* sorts on the device, writes <paramname>.peaks for every parameter and frees the columns.  A parameter with 100
 * peaks or more ends the program, as the reference's assert does. */
void run_peaks_close(const run_fold_ctx *ctx) {
    apemost_hip_sampler *s = apemost_ladder_shard(ctx->l, 0);
    const mcmc *chain0 = ctx->chains[0];
    const unsigned int n_par = get_n_par(chain0);
    const char **names = get_params_descr(chain0);
    apemost_hip_peaks_view v;
    uint64_t n = 0;
    double table[PEAKS_MAX * 4];
    char name[300];
    unsigned int p;
    uint32_t rows, r;
    v.n = &n;
    v.n_values = (uint64_t *)mem_calloc(n_par, sizeof(uint64_t));
    v.n_peaks = (uint32_t *)mem_calloc(n_par, sizeof(uint32_t));
    v.left = (uint64_t *)mem_calloc((size_t)n_par * PEAKS_MAX, sizeof(uint64_t));
    v.right = (uint64_t *)mem_calloc((size_t)n_par * PEAKS_MAX, sizeof(uint64_t));
    v.q = (double *)mem_calloc((size_t)n_par * PEAKS_MAX * 3, sizeof(double));
    v.q_set = (uint8_t *)mem_calloc((size_t)n_par * PEAKS_MAX, sizeof(uint8_t));
    apemost_hip_or_die(apemost_hip_peaks_get(s, &v), "peaks_get");
    for (p = 0; p < n_par; p++) {
        FILE *f;
        apemost_hip_or_die(apemost_hip_peaks_table(&v, (int32_t)n_par, 0, (int32_t)p, table, &rows), "peaks_table");
        sprintf(name, "%.200s.peaks", names[p]);
        f = run_open_or_die(name, "w");
        fprintf(f, "median\t-\t+\tpercent\n");
        for (r = 0; r < rows; r++)
            fprintf(f, "%f\t%f\t%f\t%f\n", table[r * 4], table[r * 4 + 1], table[r * 4 + 2], table[r * 4 + 3]);
        run_close_or_die(f, name);
    }
    apemost_hip_or_die(apemost_hip_peaks_end(s), "peaks_end");
    mem_free(v.n_values);
    mem_free(v.n_peaks);
    mem_free(v.left);
    mem_free(v.right);
    mem_free(v.q);
    mem_free(v.q_set);
}
