/* The APEMOST_DUMP token `check`: posterior predictive checks of chain 0 folded on the device while the run steps
 * (include/apemost_hip.h, apemost_hip_check_*; the quantities are specified in apemost_amd/csrc/pt_check.h).  Per datum
 * the predictive CDF at the observed value under every kept sample, per kept sample the three discrepancy statistics
 * FIT, EXTREME and SERIAL, histogrammed over APEMOST_CHECK_BINS slots (1 .. 4096, default 256; 1: no histogram) whose
 * edges are the null quantiles j / bins (apemost_hip_check_null_edges).  At the end of the run:
 *   check.bin        the state, in the format of apemost_amd/check.py (Check.read), which --append loads;
 *   check.txt        one line per datum: x, y, the mean and standard deviation of the residual e, pit, loo_pit;
 *   check_stats.txt  one line per statistic: its name, mean, standard deviation, minimum, maximum over the kept samples
 *                    and the posterior predictive p-values of the upper tail, the lower tail and both
 * ("%.15e", tab separated, a NaN as nan).  A bounded run is not needed; a device model (APEMOST_MODEL_USER) has no
 * predictive CDF and ends the program.
 * run_check.c needs neither the device nor the chains: run_check_read, _write, _write_text and _write_stats stand
 * alone.  run_check_device.c holds run_check_open and _close. */
#ifndef RUN_CHECK_H
#define RUN_CHECK_H
#include <stdint.h>

#define RUN_CHECK_FILE "check.bin"
#define RUN_CHECK_TEXT "check.txt"
#define RUN_CHECK_STATS "check_stats.txt"
#define RUN_CHECK_WORDS 7      /* origin, sum, sq, sum_u, m, S, SU */
#define RUN_CHECK_STAT_WORDS 5 /* origin, sum, sq, min, max */
#define RUN_CHECK_N_STATS 3

typedef struct {
    uint32_t n_data, n_edges, model;
    uint64_t n, thin;
    double sigma;
    int32_t chain;
    double *x, *y;                      /* [n_data] */
    double *state[RUN_CHECK_WORDS];     /* [n_data] each */
    double *edges;                      /* [3][n_edges] */
    double *stat[RUN_CHECK_STAT_WORDS]; /* [3] each */
    uint64_t *counts;                   /* [3][n_edges + 2] */
} run_check;

/* allocates every array for the n_data and n_edges already set (zeroed); frees them */
void run_check_alloc(run_check *r);
void run_check_free(run_check *r);
/* -1: no such file; 0: read (arrays allocated); 1: a check file of more than one kept chain.  Anything else that is
 * not a check file of this version ends the program. */
int run_check_read(const char *path, run_check *r);
void run_check_write(const char *path, const run_check *r);
void run_check_write_text(const char *path, const run_check *r);
void run_check_write_stats(const char *path, const run_check *r);
/* the posterior predictive p-value of statistic q from its histogram: tail 0 upper, 1 lower, 2 both; NaN without a
 * histogram or without a sample that is not NaN (Check.p_value of apemost_amd/check.py) */
double run_check_p_value(const run_check *r, int q, int tail);

#endif
