/* The folds of the run phase: what the APEMOST_DUMP tokens summary, peaks, joint, derived, evidence, autocorr, predict,
 * pointwise, check, periodogram, mbar and reweight leave of the kept sample rows without a sample file (src/parallel_tempering.c documents the tokens,
 * each fold's own header its files).  One descriptor per fold in the table run_folds[] of src/run_fold.c: the one
 * place a new token is added (a fold that refuses something at parse time adds that to run_folds_check() beside the
 * table: those refusals keep an order of their own, which is not the table's).  The run phase parses APEMOST_DUMP against the table into a mask (bit k: run_folds[k])
 * and drives the requested folds in the table's order, which is the order of their refusals and stderr lines. */
#ifndef RUN_FOLD_H
#define RUN_FOLD_H
#include <stdint.h>

#include "apemost_bridge.h"
#include "apemost_hip.h"
#include "mcmc.h"
#include "run_mbar.h"

/* what a fold sees of the run: filled once, before the folds open */
typedef struct {
    apemost_ladder *l;
    mcmc **chains;
    const unsigned int *lo;   /* shard j holds chains [lo[j], lo[j+1]); chain 0 lives on shard 0 */
    unsigned int n_shards, n_swap;
    unsigned long iter;       /* the iteration the run starts at */
    unsigned long max_iterations;
    unsigned long thin;
    int append;
    int model;                /* apemost_ladder_model() */
    double sigma;             /* apemost_ladder_sigma() */
    unsigned int nbins;       /* NBINS of the analyse phase */
} run_fold_ctx;

typedef struct {
    const char *token;
    /* why the fold needs a bounded run (the refusal's text), or NULL where it does not: `planned` is then 0 */
    const char *bounded_why;
    int every_shard;          /* one fold per shard (every chain), or shard 0 only (chain 0) */
    /* begins the fold for `planned` more kept samples; with c->append its file is loaded and the fold goes on from it */
    void (*open)(const run_fold_ctx *c, uint64_t planned);
    /* collects the accumulators, writes the fold's files and frees everything */
    void (*close)(const run_fold_ctx *c);
    int (*accumulate)(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip, uint64_t thin);
} run_fold;

#define RUN_FOLDS 12
extern const run_fold run_folds[RUN_FOLDS];

/* APEMOST_DUMP, a comma separated list: the item after the one at `spec`, or NULL; 1 when the list holds `token` (an
 * item is a token when its end or a comma follows); the table index of the fold whose token the item at `spec` is, or -1 */
const char *run_dump_next(const char *spec);
int run_dump_requested(const char *token);
int run_fold_find(const char *spec);

/* what the requested folds refuse at parse time, before any file is opened: a malformed APEMOST_POINTWISE_TAIL or
 * APEMOST_CHECK_BINS, a missing or malformed APEMOST_PERIODOGRAM_FREQS, a summary under -DHISTOGRAMS_MINMAX, mbar
 * on more than one shard or with a malformed APEMOST_MBAR_TOL or APEMOST_MBAR_ITER, and reweight without mbar in the
 * same list or with a malformed APEMOST_REWEIGHT_BINS or APEMOST_REWEIGHT_BETAS */
void run_folds_check(unsigned int mask);
/* the kept samples a bounded run will produce from iteration `iter` on; an unbounded run ends the program */
uint64_t planned_samples(const char *token, const char *why, unsigned int n_swap, unsigned long iter,
                         unsigned long max_iterations, unsigned long thin);
void run_folds_open(unsigned int mask, const run_fold_ctx *c);
/* folds the batch d_samples[j] of every shard j, on the stream of the sample reads: its first kept step is `skip` */
void run_folds_accumulate(unsigned int mask, const run_fold_ctx *c, double *const *d_samples, uint64_t n_steps,
                          uint64_t skip);
void run_folds_close(unsigned int mask, const run_fold_ctx *c);

/* the folds' device sides (src/run_<fold>_device.c, src/run_peaks.c) */
void run_summary_open(const run_fold_ctx *c, uint64_t planned), run_summary_close(const run_fold_ctx *c);
void run_peaks_open(const run_fold_ctx *c, uint64_t planned), run_peaks_close(const run_fold_ctx *c);
void run_joint_open(const run_fold_ctx *c, uint64_t planned), run_joint_close(const run_fold_ctx *c);
void run_derived_open(const run_fold_ctx *c, uint64_t planned), run_derived_close(const run_fold_ctx *c);
void run_evidence_open(const run_fold_ctx *c, uint64_t planned), run_evidence_close(const run_fold_ctx *c);
void run_autocorr_open(const run_fold_ctx *c, uint64_t planned), run_autocorr_close(const run_fold_ctx *c);
void run_predict_open(const run_fold_ctx *c, uint64_t planned), run_predict_close(const run_fold_ctx *c);
void run_pointwise_open(const run_fold_ctx *c, uint64_t planned), run_pointwise_close(const run_fold_ctx *c);
/* APEMOST_POINTWISE_TAIL: 0 unset, -1 auto, else the capacity; a malformed value ends the program */
int run_pointwise_tail_from_env(void);
void run_check_open(const run_fold_ctx *c, uint64_t planned), run_check_close(const run_fold_ctx *c);
/* APEMOST_CHECK_BINS: the slots of the statistics' histograms, 256 unset; a malformed value ends the program */
int run_check_bins_from_env(void);
void run_periodogram_open(const run_fold_ctx *c, uint64_t planned), run_periodogram_close(const run_fold_ctx *c);
/* APEMOST_PERIODOGRAM_FREQS=lo:hi:n, which the token requires: an unset or malformed value ends the program */
void run_periodogram_check_env(void);
void run_mbar_open(const run_fold_ctx *c, uint64_t planned), run_mbar_close(const run_fold_ctx *c);
void run_reweight_open(const run_fold_ctx *c, uint64_t planned), run_reweight_close(const run_fold_ctx *c);
/* the mbar fold's close calls it between its solve and its end, while both stores are on the device (src/run_reweight_device.c) */
void run_reweight_solved(const run_fold_ctx *c, const run_mbar *m);

#endif
