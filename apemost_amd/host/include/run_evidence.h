/* evidence.bin and evidence.txt: the APEMOST_DUMP token `evidence` (include/apemost_hip.h, apemost_hip_evidence_*).
 * The run phase folds column prob - prior = beta * loglike of EVERY chain on the device into its moments about the
 * first sample, its batch sums and the two log-sum-exps of the stepping-stone estimator, and at its end writes what
 * the estimators of ln p(D|M,I) beyond analyse's rectangle rule need, without the sample dump having been written.
 *
 * evidence.bin (little-endian), version 1; apemost_amd/evidence.py reads and writes the same bytes:
 *   char[8]  "APEMOSTE"
 *   uint32   version, n_chains, n_ladders (1), 0
 *   uint64   n, thin, batch_size, max_batches
 *   double   betas[n_chains], coef_up[n_chains], coef_down[n_chains]
 *   double   origin[n_chains], sum[n_chains], sq[n_chains]
 *   double   m[2][n_chains], S[2][n_chains]                  (up, down)
 *   double   batch[n_chains][max_batches + 1]                (slot n_batches: the open batch)
 * evidence.txt: one line per chain, `beta mean_loglike var_loglike mcse ln_r_up ln_r_down`, "%.15e", tab separated
 * (a NaN as nan), where ln_r_up = ln Z(beta_{c-1}) / Z(beta_c) and ln_r_down = ln Z(beta_{c+1}) / Z(beta_c) from
 * chain c's samples; then one line `name value` per total: thermodynamic_rectangle (what analyse prints),
 * thermodynamic_trapezoid, thermodynamic_corrected, thermodynamic_corrected_base_down, stepping_stone_up,
 * stepping_stone_down, base_rectangle, base_down, error_rectangle, error_trapezoid, error_corrected.  The formulas are
 * those of apemost_amd/evidence.py, operation for operation. */
#ifndef RUN_EVIDENCE_H
#define RUN_EVIDENCE_H
#include <stdint.h>

#define RUN_EVIDENCE_FILE "evidence.bin"
#define RUN_EVIDENCE_TEXT "evidence.txt"

typedef struct {
    uint32_t n_chains;
    uint64_t n, thin, bs, max_batches;
    double *betas, *coef_up, *coef_down; /* [n_chains] */
    double *origin, *sum, *sq;           /* [n_chains] */
    double *m, *S;                       /* [2][n_chains] */
    double *batch;                       /* [n_chains][max_batches + 1] */
} run_evidence;

/* allocates the arrays of a state whose n_chains and max_batches are set; everything zero */
void run_evidence_alloc(run_evidence *r);
void run_evidence_free(run_evidence *r);
/* 0: read; -1: no such file.  *n_ladders receives the ladders the file holds.  Another magic or version, a batch
 * size that does not fit or a truncated file ends the program. */
int run_evidence_read(const char *path, run_evidence *r, uint32_t *n_ladders);
void run_evidence_write(const char *path, const run_evidence *r);
void run_evidence_write_text(const char *path, const run_evidence *r);

#endif
