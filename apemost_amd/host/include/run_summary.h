/* summary.bin: the run summary of APEMOST_DUMP=summary (include/apemost_hip.h, apemost_hip_summary_*):
 * what the analyse phase needs -- per chain the sum of prob - prior, and chain 0's marginal histogram
 * counts and batch sums -- in place of the sample dumps.  Layout (native little-endian), version 1:
 *   char[8] "APEMOSTS"; uint32 version, n_beta, n_par, nbins; uint64 thin, batch_size;
 *   uint32 n_hist_chains, 0; uint64 n, n_batches, max_batches; double lo[n_par], hi[n_par];
 *   double prob_sum[n_beta]; uint64 hist[n_hist_chains][n_par][nbins];
 *   double batch_sums[n_hist_chains][n_par][max_batches + 1]   (slot n_batches: the open batch)
 * apemost_amd/summary.py reads and writes the same file. */
#ifndef RUN_SUMMARY_H
#define RUN_SUMMARY_H
#include <stdint.h>

#define RUN_SUMMARY_FILE "summary.bin"

typedef struct {
    uint32_t n_beta, n_par, nbins, n_hist;
    uint64_t thin, bs, n, n_batches, max_batches;
    double *lo, *hi;       /* [n_par] */
    double *prob_sum;      /* [n_beta] */
    uint64_t *hist;        /* [n_hist][n_par][nbins] */
    double *batch_sums;    /* [n_hist][n_par][max_batches + 1] */
} run_summary;

/* allocates the arrays of a summary whose sizes are set */
void run_summary_alloc(run_summary *r);
void run_summary_free(run_summary *r);
/* 0 and *r filled, or -1 when the file does not exist; a malformed file ends the program */
int run_summary_read(const char *path, run_summary *r);
void run_summary_write(const char *path, const run_summary *r);

#endif
