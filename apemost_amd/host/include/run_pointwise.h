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
 * With APEMOST_POINTWISE_TAIL=auto|N the fold also keeps its tail (include/apemost_hip.h, apemost_hip_pointwise_tail_*):
 * per datum the largest leave-one-out log weights of chain 0's kept samples, which Pareto-smoothed leave-one-out and the
 * Pareto k of every datum need.  N is the capacity (2 .. 4096); auto is min(4096, ceil(min(0.2 n, 3 sqrt(n))) + 1) of the
 * n kept samples the bounded run plans, and with --append the capacity of the file being resumed.  The fit is not
 * restated in C: `python -m apemost_amd.psis DIR` reads pointwise.bin and pointwise_tail.bin and prints the table.
 * pointwise_tail.bin (little-endian), version 1; apemost_amd/psis.py reads and writes the same bytes:
 *   char[8]  "APEMOSTT"
 *   uint32   version, n_keep, n_data, capacity, n_ladders, 0, 0, 0
 *   uint64   n, thin
 *   int32    chains[n_keep]
 *   uint64   count[n_keep][n_data]
 *   double   values[n_keep][n_data][capacity]      descending; the slots at and behind count are 0
 * Without the variable no such file is written and every other file is what it is today.
 *
 * run_pointwise.c needs neither the device nor the chains: run_pointwise_read, _write, _write_text and _write_criteria
 * stand alone.  run_pointwise_device.c holds run_pointwise_open and _close. */
#ifndef RUN_POINTWISE_H
#define RUN_POINTWISE_H
#include <stdint.h>

#define RUN_POINTWISE_FILE "pointwise.bin"
#define RUN_POINTWISE_TEXT "pointwise.txt"
#define RUN_POINTWISE_CRITERIA "criteria.txt"
#define RUN_POINTWISE_TAIL_FILE "pointwise_tail.bin"
#define RUN_POINTWISE_WORDS 8

/* the tail of one kept chain's fold; capacity 0: none */
typedef struct {
    uint32_t n_data, capacity;
    int32_t chain;
    uint64_t n, thin;
    uint64_t *count; /* [n_data] */
    double *values;  /* [n_data][capacity] */
} run_pointwise_tail;

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
    run_pointwise_tail tail;  /* (not part of pointwise.bin) */
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
/* min(4096, ceil(min(0.2 n, 3 sqrt(n))) + 1), at least 2: psis.capacity_for */
uint32_t run_pointwise_tail_capacity_for(uint64_t n);
/* allocates count and values of a tail whose n_data and capacity are set, zeroed */
void run_pointwise_tail_alloc(run_pointwise_tail *t);
void run_pointwise_tail_free(run_pointwise_tail *t);
/* 0: read; -1: no such file; 1: a file of several kept chains or of a count above its capacity (nothing is allocated).
 * Another magic, version or a truncated file ends the program. */
int run_pointwise_tail_read(const char *path, run_pointwise_tail *t);
/* the slots at and behind count are written as 0 */
void run_pointwise_tail_write(const char *path, const run_pointwise_tail *t);

#endif
