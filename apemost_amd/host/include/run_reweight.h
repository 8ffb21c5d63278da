/* reweight.bin and reweight.txt: the APEMOST_DUMP token `reweight` (include/apemost_hip.h, apemost_hip_reweight_*).
 * Beside the token `mbar`, which it needs in the same list, the run phase keeps the parameters of EVERY kept step of
 * EVERY chain on the device, and at its end, after MBAR's solve, forms there the posterior's moments and marginal
 * histograms at the targets APEMOST_REWEIGHT_BETAS (a comma list of finite numbers >= 0, at most 64, default `1`) from
 * all chains' samples with the MBAR weights, without the sample dump having been written.  The histograms have
 * APEMOST_REWEIGHT_BINS bins (1 .. 4096, default 200) over the params file's min and max, as the summary's.
 *
 * reweight.bin (little-endian), version 1; apemost_amd/reweight.py reads and writes the same bytes:
 *   char[8]  "APEMOSTW"
 *   uint32   version, n_chains, n_ladders (1), n_cols, n_t, nbins
 *   int32    shift
 *   uint32   0
 *   uint64   n, thin, t0, t_count                            (n: kept steps stored; the range of the evaluation)
 *   int32    cols[16]                                        (the first n_cols; the rest 0)
 *   double   lo[n_cols], hi[n_cols]
 *   double   betas_t[n_t]
 *   double   m[n_t], S0[n_t], SS[n_t]
 *   double   origin[n_cols]
 *   double   S1[n_t][n_cols]
 *   double   cross[n_t][n_cols (n_cols + 1) / 2]             (the upper triangle, row-major)
 *   uint64   hist[n_t][n_cols][nbins]
 *   uint64   q_total[n_t]
 * reweight.txt: per target and parameter one line `beta name mean sd ess`, the numbers "%.15e" (a NaN as nan), tab
 * separated: mean = origin + S1 / S0, sd = sqrt(cross / S0 - (S1 / S0)^2), ess = S0^2 / SS, the formulas of
 * apemost_amd/reweight.py (Reweighted.text) operation for operation.
 *
 * Resampling.  APEMOST_RESAMPLE_DRAWS=M (0 .. 2^24, default 0: nothing) makes the token also draw, for every target, M
 * equally weighted samples from all chains' samples on the device (apemost_hip_reweight_resample: systematic
 * resampling over the fixed-point weights with the offset word APEMOST_RESAMPLE_SEED, a uint64, default 0) and write
 * them as resample.bin and, for target t and every parameter, <paramname>-reweighted-<t>.dump: one "%.15e" line per
 * draw, the format of <paramname>-chain-0.prob.dump, which the reference's histogram and peak tools read.  The draws are in stored
 * order (time-major): equally weighted, not exchangeable in order.
 * resample.bin (little-endian), version 1; apemost_amd/reweight.py (Resampled.write_all) writes the same bytes:
 *   char[8]  "APEMOSTS"
 *   uint32   version, n_chains, n_ladders (1), n_cols, n_t, n_draws
 *   int32    shift
 *   uint32   0
 *   uint64   n, thin, t0, t_count, u
 *   int32    cols[16]
 *   n_t times:  double beta_t;  uint64 q_total;  uint32 index[n_draws];  double x[n_draws][n_cols]
 * This file's half (src/run_reweight.c) names no device symbol; the device's is src/run_reweight_device.c. */
#ifndef RUN_REWEIGHT_H
#define RUN_REWEIGHT_H
#include <stdint.h>

#define RUN_REWEIGHT_FILE "reweight.bin"
#define RUN_REWEIGHT_TEXT "reweight.txt"
#define RUN_REWEIGHT_MAX_COLS 16
#define RUN_REWEIGHT_MAX_TARGETS 64
#define RUN_REWEIGHT_MAX_BINS 4096
#define RUN_RESAMPLE_FILE "resample.bin"
#define RUN_RESAMPLE_MAX_DRAWS 16777216ul

typedef struct {
    uint32_t n_chains, n_cols, n_t, nbins;
    int32_t shift;
    uint64_t n, thin, t0, t_count;
    int32_t cols[RUN_REWEIGHT_MAX_COLS];
    double *lo, *hi;      /* [n_cols] */
    double *betas_t;      /* [n_t] */
    double *m, *S0, *SS;  /* [n_t] */
    double *origin;       /* [n_cols] */
    double *S1;           /* [n_t][n_cols] */
    double *cross;        /* [n_t][n_cols (n_cols + 1) / 2] */
    uint64_t *hist;       /* [n_t][n_cols][nbins] */
    uint64_t *q_total;    /* [n_t] */
} run_reweight;

/* allocates the arrays of a state whose n_cols, n_t and nbins are set; everything zero */
void run_reweight_alloc(run_reweight *r);
void run_reweight_free(run_reweight *r);
/* 0: read; -1: no such file.  Another magic or version, more than one ladder, a header out of range or a truncated file
 * ends the program. */
int run_reweight_read(const char *path, run_reweight *r);
void run_reweight_write(const char *path, const run_reweight *r);
/* Reweighted.text; names [n_cols], or NULL: col<index> */
void run_reweight_write_text(const char *path, const run_reweight *r, const char *const *names);
/* APEMOST_REWEIGHT_BINS; a malformed value ends the program */
unsigned int run_reweight_bins_from_env(void);
/* APEMOST_REWEIGHT_BETAS into betas [RUN_REWEIGHT_MAX_TARGETS]: the count; a malformed value ends the program */
unsigned int run_reweight_betas_from_env(double *betas);
/* APEMOST_RESAMPLE_DRAWS (0: no resampling) and APEMOST_RESAMPLE_SEED; a malformed value ends the program */
uint32_t run_resample_draws_from_env(void);
uint64_t run_resample_seed_from_env(void);
/* resample.bin of the state's targets: q_total [n_t], index [n_t][n_draws], x [n_t][n_draws][n_cols] */
void run_resample_write(const char *path, const run_reweight *r, uint32_t n_draws, uint64_t u, const uint64_t *q_total,
                        const uint32_t *index, const double *x);
/* <name>-reweighted-<t>.dump of target t's draws x [n_draws][n_cols]; names [n_cols], or NULL: col<index> */
void run_resample_write_dumps(const run_reweight *r, unsigned int t, uint32_t n_draws, const double *x,
                              const char *const *names);

#endif
