/* pointwise.bin, pointwise.txt and criteria.txt: the APEMOST_DUMP token `pointwise` (include/apemost_hip.h,
 * apemost_hip_pointwise_*).  The run phase folds the log-likelihood term of every datum under chain 0's kept samples on
 * the device: per datum the sums that give the term's mean and variance, the running log-sum-exp of the term (the log
 * pointwise predictive density) and of its negative (importance-sampling leave-one-out) with the effective sample size
 * of the latter's weights; per chain the parameter sums whose mean DIC evaluates the model at.
 *
 * pointwise.bin (little-endian), version 1; apemost_amd/pointwise.py reads and writes the same bytes:
 *   char[8]  "APEMOSTW"
 *   uint32   version, n_keep, n_data, n_par, n_ladders, model, 0, 0
 *   uint64   n, thin
 *   double   sigma
 *   int32    chains[n_keep]
 *   double   x, y: [n_keep][n_data] each
 *   double   origin, sum, sq, m_up, S_up, m_dn, S_dn, S2_dn: [n_keep][n_data] each
 *   double   par_origin, par_sum: [n_keep][n_par] each
 *   double   at_mean[n_keep][n_data]
 * pointwise.txt: one line per datum, `x y mean sd lppd p_waic2 elpd_loo ess`, tab separated, "%.15e": the text of
 * Pointwise.text() of apemost_amd/pointwise.py.  criteria.txt: `name<TAB>value` lines for n, lppd, p_waic1, p_waic2,
 * elpd_waic, waic, waic_se, elpd_loo, looic, p_loo, dic, p_dic: the text of Pointwise.criteria_text().  run_pointwise.c
 * repeats that module's formulas operation for operation.  For the sine models the constant -ln(sigma sqrt(2 pi)) is
 * left out of every term, as the reference's likelihood leaves it out.
 *
 * run_pointwise.c needs neither the device nor the chains: run_pointwise_read, _write, _write_text and _write_criteria
 * stand alone.  run_pointwise_device.c holds run_pointwise_open and _close. */
#ifndef RUN_POINTWISE_H
#define RUN_POINTWISE_H
#include <stdint.h>

#define RUN_POINTWISE_FILE "pointwise.bin"
#define RUN_POINTWISE_TEXT "pointwise.txt"
#define RUN_POINTWISE_CRITERIA "criteria.txt"
#define RUN_POINTWISE_WORDS 8

/* one kept chain (n_keep == 1, n_ladders == 1) */
typedef struct {
    uint32_t n_data, n_par, model;
    int32_t chain;
    uint64_t n, thin;
    double sigma;
    double *x, *y;            /* [n_data] */
    double *state[RUN_POINTWISE_WORDS]; /* origin, sum, sq, m_up, S_up, m_dn, S_dn, S2_dn: [n_data] each */
    double *par_origin, *par_sum; /* [n_par] */
    double *at_mean;          /* [n_data] */
} run_pointwise;

/* allocates the arrays of a state whose n_data and n_par are set; the state of a fold before its first sample */
void run_pointwise_alloc(run_pointwise *r);
void run_pointwise_free(run_pointwise *r);
/* 0: read; -1: no such file; 1: a file of several kept chains (nothing is allocated).  Another magic, version or a
 * truncated file ends the program. */
int run_pointwise_read(const char *path, run_pointwise *r);
void run_pointwise_write(const char *path, const run_pointwise *r);
void run_pointwise_write_text(const char *path, const run_pointwise *r);
void run_pointwise_write_criteria(const char *path, const run_pointwise *r);

#ifndef RUN_POINTWISE_STANDALONE
#include "apemost_hip.h"
#include "mcmc.h"
/* begins the fold of local chain 0 of shard `s` over its data.  With `append` pointwise.bin is loaded and the fold
 * goes on from it; a file of another shape, data, sigma or thin ends the program. */
void run_pointwise_open(run_pointwise *r, apemost_hip_sampler *s, const mcmc *chain0, int model, double sigma,
                        uint64_t thin, int append);
/* collects the accumulator, evaluates the term at the mean parameters on the device, writes the three files, and
 * frees everything */
void run_pointwise_close(run_pointwise *r, apemost_hip_sampler *s);
#endif

#endif
