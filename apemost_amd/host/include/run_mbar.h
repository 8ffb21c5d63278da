/* mbar.bin and mbar.txt: the APEMOST_DUMP token `mbar` (include/apemost_hip.h, apemost_hip_mbar_*).  The run phase
 * stores loglike = (prob - prior) / beta of EVERY kept step of EVERY chain on the device, and at its end solves the
 * MBAR equations (Shirts & Chodera 2008) there: the free energies ln Z(beta_k) from all chains' samples at once, and
 * from the same weights ln Z, E[loglike], Var[loglike] and the effective sample size at every rung and the evidence
 * ln Z(1) - ln Z(0), without the sample dump having been written.
 *
 * mbar.bin (little-endian), version 1; apemost_amd/mbar.py reads and writes the same bytes:
 *   char[8]  "APEMOSTM"
 *   uint32   version, n_chains, n_ladders (1), solved (0 or 1)
 *   uint64   n, thin, t0, t_count                            (the range of the solve; 0, 0 where not solved)
 *   double   betas[n_chains]
 *   uint64   n_bad[n_ladders]
 *   double   g[n_chains]                                     (g_k - g_0; 0 where not solved)
 *   double   ell[n][n_chains]
 * mbar.txt: one line per rung, `beta ln_z mean_loglike var_loglike ess`, "%.15e", tab separated (a NaN as nan), ln_z
 * being ln Z(beta) - ln Z(beta_0) with both from the same weights; then `ln_evidence value error`, the error being
 * the standard error of the mean of RUN_MBAR_BLOCKS contiguous time blocks, each solved on its own from the whole
 * run's free energies.  The solver loop and the formulas are those of apemost_amd/mbar.py (Mbar.solve, Mbar.text),
 * operation for operation; the passes themselves (the row pass, the column sums in their fixed order) are behind
 * run_mbar_passes: the device's (src/run_mbar_device.c), or run_mbar_host_passes, the same order in C for a stored
 * column without a device.  APEMOST_MBAR_TOL (default 1e-10) and APEMOST_MBAR_ITER (default 10000) set the tolerance
 * and the iteration cap. */
#ifndef RUN_MBAR_H
#define RUN_MBAR_H
#include <stdint.h>

#define RUN_MBAR_FILE "mbar.bin"
#define RUN_MBAR_TEXT "mbar.txt"
#define RUN_MBAR_BLOCKS 10
#define RUN_MBAR_CHECK_EVERY 10

typedef struct {
    uint32_t n_chains, solved;
    uint64_t n, thin, t0, t_count, n_bad;
    double *betas, *g; /* [n_chains] */
    double *ell;       /* [n][n_chains] */
} run_mbar;

/* the passes over the kept steps [t0, t0 + t_count) of a store; both return 0, or end the program */
typedef struct {
    void *ctx;
    /* n_iter updates g <- G(g); g_prev: g before the last of them */
    int (*iterate)(void *ctx, uint64_t t0, uint64_t t_count, uint32_t n_iter, double *g, double *g_prev);
    /* the six words of apemost_hip_mbar_sums for n_t targets, words[w][t] with w = m, S0, S1, S2, SS, G; *ell_first */
    int (*evaluate)(void *ctx, uint64_t t0, uint64_t t_count, const double *g, const double *betas_t, int n_t,
                    double *const words[6], double *ell_first);
} run_mbar_passes;

/* allocates the arrays of a state whose n_chains and n are set; everything zero */
void run_mbar_alloc(run_mbar *r);
void run_mbar_free(run_mbar *r);
/* 0: read; -1: no such file.  Another magic or version, more than one ladder or a truncated file ends the program. */
int run_mbar_read(const char *path, run_mbar *r);
void run_mbar_write(const char *path, const run_mbar *r);
/* the tolerance and the iteration cap from the environment; a malformed value ends the program */
double run_mbar_tol_from_env(void);
unsigned long run_mbar_iter_from_env(void);
/* Mbar.start: the trapezoid rule over the per-chain means of ell from the hottest chain up, less g_0 */
void run_mbar_start(const run_mbar *r, uint64_t t0, uint64_t t_count, double *g);
/* Mbar.solve over [t0, t0 + t_count) from g [n_chains] (relative to g_0 on return): the iterations used, or -1 when
 * max_iter updates left a change above tol; *change receives the last change */
long run_mbar_solve(const run_mbar *r, const run_mbar_passes *p, double tol, unsigned long max_iter, uint64_t t0,
                    uint64_t t_count, double *g, double *change);
/* Mbar.text of a solved state */
void run_mbar_write_text(const char *path, const run_mbar *r, const run_mbar_passes *p, double tol, unsigned long max_iter);
/* the passes in C over r->ell, in the order csrc/pt_mbar.h states, libm's exp and log */
run_mbar_passes run_mbar_host_passes(const run_mbar *r);

#endif
