/* the table of the run phase's folds and the loops over it (run_fold.h) */
#include "run_fold.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "run_mbar.h"
#include "run_reweight.h"

#define BATCH_SIZE_WHY "the batch size of the error estimate is fixed before the first sample"
#define KEPT_ON_DEVICE_WHY "the columns kept on the device are sized before the first sample"

/* In the order the folds open and close.  Only summary and evidence fold every chain, so one fold per shard; the
 * others fold chain 0, which lives on shard 0.  joint and autocorr size nothing by the samples to come and run
 * unbounded too, and so does check; predict needs the bound only for its refusal, and so does periodogram.  mbar keeps
 * every chain's column on one device: its one fold is shard 0's, and more shards than that are refused below.  reweight
 * keeps the parameters beside it and is evaluated from mbar's close, behind its solve: it needs mbar in the same list. */
const run_fold run_folds[RUN_FOLDS] = {
    {"summary", BATCH_SIZE_WHY, 1, run_summary_open, run_summary_close, apemost_hip_summary_accumulate},
    {"peaks", KEPT_ON_DEVICE_WHY, 0, run_peaks_open, run_peaks_close, apemost_hip_peaks_accumulate},
    {"joint", NULL, 0, run_joint_open, run_joint_close, apemost_hip_joint_accumulate},
    {"derived", BATCH_SIZE_WHY, 0, run_derived_open, run_derived_close, apemost_hip_derived_accumulate},
    {"evidence", BATCH_SIZE_WHY, 1, run_evidence_open, run_evidence_close, apemost_hip_evidence_accumulate},
    {"autocorr", NULL, 0, run_autocorr_open, run_autocorr_close, apemost_hip_autocorr_accumulate},
    {"predict", "predict.bin and predict.txt are written when the run ends", 0, run_predict_open, run_predict_close,
     apemost_hip_predict_accumulate},
    {"pointwise", "pointwise.bin, pointwise.txt and criteria.txt are written when the run ends", 0, run_pointwise_open,
     run_pointwise_close, apemost_hip_pointwise_accumulate},
    {"check", NULL, 0, run_check_open, run_check_close, apemost_hip_check_accumulate},
    {"periodogram", "periodogram.bin and periodogram.txt are written when the run ends", 0, run_periodogram_open,
     run_periodogram_close, apemost_hip_periodogram_accumulate},
    {"mbar", KEPT_ON_DEVICE_WHY, 0, run_mbar_open, run_mbar_close, apemost_hip_mbar_accumulate},
    {"reweight", KEPT_ON_DEVICE_WHY, 0, run_reweight_open, run_reweight_close, apemost_hip_reweight_accumulate}};

static int item_is(const char *spec, const char *token) {
    const size_t len = strlen(token);
    return strncmp(spec, token, len) == 0 && (spec[len] == 0 || spec[len] == ',');
}

const char *run_dump_next(const char *spec) {
    spec = strchr(spec, ',');
    return spec != NULL ? spec + 1 : NULL;
}

int run_dump_requested(const char *token) {
    const char *spec = getenv("APEMOST_DUMP");
    for (; spec != NULL && *spec != 0; spec = run_dump_next(spec))
        if (item_is(spec, token))
            return 1;
    return 0;
}

int run_fold_find(const char *spec) {
    int k;
    for (k = 0; k < RUN_FOLDS; k++)
        if (item_is(spec, run_folds[k].token))
            return k;
    return -1;
}

static int in_mask(unsigned int mask, const char *token) {
    const int k = run_fold_find(token);
    return k >= 0 && (mask & (1u << k)) != 0;
}

void run_folds_check(unsigned int mask) {
    if (in_mask(mask, "pointwise"))
        (void)run_pointwise_tail_from_env();
    if (in_mask(mask, "check"))
        (void)run_check_bins_from_env();
    if (in_mask(mask, "periodogram"))
        run_periodogram_check_env();
#ifdef HISTOGRAMS_MINMAX
    if (in_mask(mask, "summary")) {
        fprintf(stderr, "APEMOST_DUMP=summary cannot be combined with -DHISTOGRAMS_MINMAX: the histogram range "
                        "would have to be known before the first sample\n");
        exit(1);
    }
#endif
    if (in_mask(mask, "mbar")) { /* (APEMOST_DEVICES=0,1,...: one shard per device named) */
        const char *devices = getenv("APEMOST_DEVICES");
        if (devices != NULL && strchr(devices, ',') != NULL) {
            fprintf(stderr, "APEMOST_DUMP=mbar needs the whole ladder on one device, APEMOST_DEVICES=%s names several: "
                            "the solve reads every chain\n", devices);
            exit(1);
        }
        (void)run_mbar_tol_from_env();
        (void)run_mbar_iter_from_env();
    }
    if (in_mask(mask, "reweight")) {
        double betas[RUN_REWEIGHT_MAX_TARGETS];
        if (!in_mask(mask, "mbar")) {
            fprintf(stderr, "APEMOST_DUMP=reweight needs mbar in the same list: the weights are the mbar fold's\n");
            exit(1);
        }
        (void)run_reweight_bins_from_env();
        (void)run_reweight_betas_from_env(betas);
        (void)run_resample_draws_from_env();
        (void)run_resample_seed_from_env();
    }
}

uint64_t planned_samples(const char *token, const char *why, unsigned int n_swap, unsigned long iter,
                         unsigned long max_iterations, unsigned long thin) {
    unsigned long end = iter;
    if (max_iterations == 0) {
        fprintf(stderr, "APEMOST_DUMP=%s needs a bounded run (MAX_ITERATIONS > 0): %s\n", token, why);
        exit(1);
    }
    if (end < max_iterations) /* whole rounds: the last one may run past max_iterations */
        end += (max_iterations - iter + n_swap - 1) / n_swap * n_swap;
    return end / thin - iter / thin; /* iterations thin, 2 thin, ... are kept */
}

void run_folds_open(unsigned int mask, const run_fold_ctx *c) {
    int k;
    for (k = 0; k < RUN_FOLDS; k++)
        if (mask & (1u << k)) {
            const run_fold *f = &run_folds[k];
            f->open(c, f->bounded_why == NULL ? 0 : planned_samples(f->token, f->bounded_why, c->n_swap, c->iter,
                                                                    c->max_iterations, c->thin));
        }
}

void run_folds_accumulate(unsigned int mask, const run_fold_ctx *c, double *const *d_samples, uint64_t n_steps,
                          uint64_t skip) {
    char what[32];
    unsigned int j;
    int k;
    for (k = 0; k < RUN_FOLDS; k++)
        if (mask & (1u << k)) {
            const run_fold *f = &run_folds[k];
            for (j = 0; j < (f->every_shard ? c->n_shards : 1); j++) {
                const int rc = f->accumulate(apemost_ladder_shard(c->l, j), d_samples[j], n_steps, skip, c->thin);
                if (rc != APEMOST_HIP_OK) {
                    sprintf(what, "%.16s_accumulate", f->token);
                    apemost_hip_or_die(rc, what);
                }
            }
        }
}

void run_folds_close(unsigned int mask, const run_fold_ctx *c) {
    int k;
    for (k = 0; k < RUN_FOLDS; k++)
        if (mask & (1u << k))
            run_folds[k].close(c);
}
