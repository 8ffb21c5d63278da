/* autocorr.bin and autocorr.txt: the APEMOST_DUMP token `autocorr` (include/apemost_hip.h, apemost_hip_autocorr_*).
 * The run phase folds chain 0's parameters and its column prob - prior on the device into the lag sums of the lags
 * 0 .. max_lag - 1 (APEMOST_AUTOCORR_LAGS, default 1024), which give the autocorrelation function, the integrated
 * autocorrelation time and the effective sample size without the sample dump having been written.
 *
 * autocorr.bin (little-endian), version 1; apemost_amd/autocorr.py reads and writes the same bytes:
 *   char[8]  "APEMOSTA"
 *   uint32   version, n_keep, n_cols, max_lag, n_par, n_ladders
 *   uint64   n, thin
 *   int32    chains[n_keep], cols[n_cols]
 *   double   origin[n_keep][n_cols], sum[n_keep][n_cols]
 *   double   lag[n_keep][n_cols][max_lag]
 *   double   head[n_keep][n_cols][max_lag - 1], tail[n_keep][n_cols][max_lag - 1]
 * autocorr.txt: one line per column, `name mean variance tau_sokal window ess mcse tau_geyer`, tab separated, "%.15e":
 * the text of Autocorr.text() of apemost_amd/autocorr.py, whose formulas run_autocorr.c repeats operation for
 * operation.
 *
 * run_autocorr.c needs neither the device nor the chains: run_autocorr_read, _write, _write_text and the estimators
 * stand alone.  run_autocorr_device.c holds run_autocorr_open and _close. */
#ifndef RUN_AUTOCORR_H
#define RUN_AUTOCORR_H
#include <stdint.h>

#define RUN_AUTOCORR_FILE "autocorr.bin"
#define RUN_AUTOCORR_TEXT "autocorr.txt"
#define RUN_AUTOCORR_DEFAULT_LAGS 1024

/* one kept chain (n_keep == 1, n_ladders == 1) */
typedef struct {
    uint32_t n_cols, max_lag, n_par;
    int32_t chain;
    uint64_t n, thin;
    int32_t *cols;            /* [n_cols] */
    double *origin, *sum;     /* [n_cols] */
    double *lag;              /* [n_cols][max_lag] */
    double *head, *tail;      /* [n_cols][max_lag - 1] */
} run_autocorr;

/* allocates the arrays of a state whose n_cols and max_lag are set; everything zero */
void run_autocorr_alloc(run_autocorr *r);
void run_autocorr_free(run_autocorr *r);
/* 0: read; -1: no such file; 1: a file of several kept chains (nothing is allocated).  Another magic, version or a
 * truncated file ends the program. */
int run_autocorr_read(const char *path, run_autocorr *r);
void run_autocorr_write(const char *path, const run_autocorr *r);

/* acov[l], l < max_lag, of column c: the autocovariance about the mean, divided by n; 0 from lag n on */
void run_autocorr_acov(const run_autocorr *r, unsigned int c, double *acov);
/* Sokal's automatic window: the smallest M >= 5 tau(M); *window = -1 where none closes, tau is then the sum over all
 * lags */
double run_autocorr_tau_sokal(const run_autocorr *r, const double *acov, long *window);
/* Geyer's initial positive sequence */
double run_autocorr_tau_geyer(const run_autocorr *r, const double *acov, long *window);
/* names: of the n_par parameters */
void run_autocorr_write_text(const char *path, const run_autocorr *r, const char **names);

#endif
