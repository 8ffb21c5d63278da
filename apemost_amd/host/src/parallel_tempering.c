/* The phases an application main calls: calibrate_first, calibrate_rest, run
 * (behaviour and file formats of reference src/parallel_tempering.c:36-419).  Every
 * Metropolis step, calibration sweep and swap attempt runs on the MI355X engine; this file
 * only moves state between the files, the host chain objects and the device, and writes
 * the reference's text outputs. */
#include <math.h>
#include <string.h>
#include "mcmc.h"
#include "parallel_tempering.h"
#include "parallel_tempering_beta.h"
#include "parallel_tempering_interaction.h"
#include "parallel_tempering_config.h"
#include "parallel_tempering_run.h"
#include "apemost_bridge.h"
#include "run_fold.h"
#include "run_io.h"
#include "debug.h"
#include "define_defaults.h"
#include "gsl_helper.h"
#include "utils.h"

static void fill_calib(apemost_hip_calib_config *c) {
    apemost_hip_calib_defaults(c);
    c->burn_in_iterations = BURN_IN_ITERATIONS;
    c->iter_limit = ITER_LIMIT;
    c->iter_readjust = ITER_READJUST;
    c->no_rescaling_limit = NO_RESCALING_LIMIT;
    c->rat_limit = TARGET_ACCEPTANCE_RATE;
    c->target_global = TARGET_ACCEPTANCE_RATE;
    c->max_ar_deviation = MAX_AR_DEVIATION;
    c->mul = MUL;
    c->adjust_step = DEFAULT_ADJUST_STEP;
}

/* markov_chain_calibrate() for chains [first, first+count) of a resident ladder; exits like the
 * reference when a chain cannot be calibrated */
static void calibrate_on_device(apemost_ladder *l, unsigned int first, unsigned int count, int burn_in_only) {
    apemost_hip_calib_config c;
    int32_t *status = (int32_t *)calloc(count, sizeof(int32_t));
    int rc;
    unsigned int i;
    fill_calib(&c);
    rc = apemost_ladder_calibrate(l, first, count, &c, burn_in_only, status);
    if (rc == APEMOST_HIP_ERR_CALIBRATION) {
        for (i = 0; i < count; i++)
            if (status[i] == 1)
                fprintf(stderr, "calibration failed: a step width of chain %u became too large.\n", first + i);
            else if (status[i] == 2)
                fprintf(stderr, "calibration failed: limit of %d iterations reached (chain %u).\n", ITER_LIMIT,
                        first + i);
        exit(1);
    }
    free(status);
}

static void free_chains(mcmc **chains, unsigned int n_beta) {
    unsigned int i;
    for (i = 0; i < n_beta; i++) {
        mem_free(chains[i]->additional_data);
        if (i != 0)
            set_data(chains[i], NULL); /* aliased: chain 0 frees the matrix */
        chains[i] = mcmc_free(chains[i]);
    }
    mem_free(chains);
}

/* needs: params, data.  provides: line 1 of calibration_results, params_suggested */
void calibrate_first() {
    mcmc **chains = setup_chains();
    apemost_ladder *l;
    printf("Starting markov chain calibration\n");
    fflush(stdout);
    l = apemost_ladder_open(chains, 1);
    apemost_ladder_calc_model(l, 0, 1);
    calibrate_on_device(l, 0, 1, 0);
    apemost_ladder_download(l);
    apemost_ladder_close(l);
    write_calibrations_file(chains, 1);
    write_params_file(chains[0]);
    free_chains(chains, apemost_n_beta());
}

/* start chain i of the ladder from chain 0's best point with predicted step widths
 * steps0 * beta^-1/2 (* factors) */
static void seed_chain(mcmc **chains, unsigned int i, double beta, const gsl_vector *factors) {
    set_beta(chains[i], beta);
    gsl_vector_memcpy(get_steps(chains[i]), get_steps(chains[0]));
    gsl_vector_scale(get_steps(chains[i]), pow(beta, -0.5));
    if (factors != NULL)
        gsl_vector_mul(get_steps(chains[i]), factors);
    set_params(chains[i], dup_vector(get_params_best(chains[0])));
}

/* needs: params, data, line 1 of calibration_results.  provides: calibration_results for the
 * whole ladder, calibration_summary */
void calibrate_rest() {
    const unsigned int n_beta = apemost_n_beta();
    double beta_0 = BETA_0;
    mcmc **chains = setup_chains();
    const unsigned int n_par = get_n_par(chains[0]);
    gsl_vector *factors = gsl_vector_alloc(n_par);
    apemost_ladder *l;
    unsigned int i;

    read_calibration_file(chains, 1);
    printf("Calibrating chains\n");
    fflush(stdout);
    gsl_vector_set_all(factors, 1);

    if (n_beta > 1) {
        /* the second chain alone first: its calibrated widths against the beta^-1/2 prediction
         * give the per-parameter stepwidth factors */
        const double b1 = get_chain_beta(1, n_beta, beta_0 < 0 ? calc_beta_0(chains[0], factors) : beta_0);
        seed_chain(chains, 1, b1, NULL);
        printf("Calibrating second chain to infer stepwidth factor\n");
        printf("\tChain %2d - beta = %f\tsteps: ", 1, get_beta(chains[1]));
        dump_vectorln(get_steps(chains[1]));
        fflush(stdout);
        l = apemost_ladder_open(chains, n_beta);
        apemost_ladder_calc_model(l, 1, 1);
        calibrate_on_device(l, 1, 1, 0);
        apemost_ladder_download(l);
        apemost_ladder_close(l);
        gsl_vector_scale(factors, pow(get_beta(chains[1]), -0.5));
        gsl_vector_mul(factors, get_steps(chains[0]));
        gsl_vector_div(factors, get_steps(chains[1]));
    }
    printf("stepwidth factors: ");
    dump_vectorln(factors);
    if (beta_0 < 0) {
        beta_0 = calc_beta_0(chains[0], factors);
        printf("automatic beta_0: %f\n", beta_0);
    }
    fflush(stdout);

    if (n_beta > 1) {
        for (i = 1; i < n_beta; i++) {
            seed_chain(chains, i, get_chain_beta(i, n_beta, beta_0), factors);
            if (n_beta <= 64) {
                printf("\tChain %2d - beta = %f\tsteps: ", i, get_beta(chains[i]));
                dump_vectorln(get_steps(chains[i]));
            }
        }
        fflush(stdout);
        /* all remaining chains calibrate concurrently, one workgroup each */
        l = apemost_ladder_open(chains, n_beta);
        apemost_ladder_calc_model(l, 1, n_beta - 1);
#ifndef SKIP_CALIBRATE_ALLCHAINS
        calibrate_on_device(l, 1, n_beta - 1, 0);
#else
        calibrate_on_device(l, 1, n_beta - 1, 1);
#endif
        apemost_ladder_download(l);
        apemost_ladder_close(l);
    }
    gsl_vector_free(factors);
    printf("all chains calibrated.\n");
    if (n_beta <= 64)
        for (i = 0; i < n_beta; i++) {
            printf("\tChain %2d - beta = %f \tsteps: ", i, get_beta(chains[i]));
            dump_vectorln(get_steps(chains[i]));
        }
    write_calibration_summary(chains, n_beta);
    write_calibrations_file(chains, n_beta);
    free_chains(chains, n_beta);
}

static void report(const mcmc **chains, const int n_beta) {
    int i;
    print_current_positions(chains, n_beta);
    printf("\nwriting out visited parameters ");
    for (i = 0; i < n_beta; i++) {
        printf(".");
        mcmc_dump_flush(chains[i]);
        fflush(stdout);
#ifndef DUMP_ALL_CHAINS
        break;
#endif
    }
    printf("done.\n");
}

static unsigned long gcd_ul(unsigned long a, unsigned long b) {
    while (b) {
        unsigned long t = a % b;
        a = b;
        b = t;
    }
    return a;
}

/* ---- sample sink ------------------------------------------------------------------------
 * Where the sample rows of the run phase go.  Selected at run time by APEMOST_DUMP, a comma
 * separated list of
 *   text     (default) the reference's files: <name>-chain-<i>.prob.dump ("%.15e", chain 0 or
 *            all chains with -DDUMP_ALL_CHAINS; src/mcmc_dump.c:79-88) and prob-chain<i>.dump
 *            ("%6e\t%6e" for every chain; src/parallel_tempering.c:399-401)
 *   binary   one file samples.bin holding what the text files hold, as doubles: a 64-byte header,
 *            then per kept iteration the parameter vectors of the chains that have parameter dump
 *            files (chain 0; all chains with -DDUMP_ALL_CHAINS) followed by (prob, prob - prior)
 *            of every chain (tools/samples_bin.py reads it and expands it into the text files)
 *   binary:all   the same with the parameter vector of every chain
 *   thin:N   keep every N-th iteration only (either format)
 *   summary  fold the kept rows on the device into summary.bin (run_summary.h): what `analyse` prints,
 *            without the sample files.  On its own (summary, summary,thin:N) no sample file is written;
 *            with text or binary[:all] those are written as well
 *   peaks    keep chain 0's parameter columns on the device and write one <paramname>.peaks per parameter at the
 *            end: the output of the reference's `peaks.exe min max <name>-chain-0.prob.dump` over the prior box
 *            (run_peaks.c).  Combines with every other token and writes no sample file by itself, like summary
 *   joint    fold chain 0's rows on the device into one NBINS x NBINS histogram per pair of parameters over the prior
 *            box, on the bins of the marginal histograms, and into the moments of the parameter covariance; at the end
 *            write joint.bin, one <a>-<b>.joint per pair and correlation.matrix (run_joint.h).  Combines with every
 *            other token and writes no sample file by itself, like peaks
 *   derived  fold functions of chain 0's rows on the device -- the columns of the file `derived` (or of the file
 *            APEMOST_DERIVED_FILE names), one per line as `name lo hi` and a program in reverse Polish notation over the
 *            names of the params file, prob and like -- into histograms, batch sums, pair histograms and moments; at the
 *            end write derived.bin, derived.txt and one <name>.histogram per column (run_derived.h): what the
 *            reference's matrix_man and histogram_tool give from the text dumps.  Needs a bounded run.  Combines with
 *            every other token and writes no sample file by itself, like joint
 *   evidence fold column prob - prior of EVERY chain on the device into its moments, batch sums and the log-sum-exps of
 *            the stepping-stone estimator; at the end write evidence.bin and evidence.txt: thermodynamic integration by
 *            the rectangle, trapezoid and variance-corrected trapezoid rules, the stepping stone in both directions and
 *            error bars (run_evidence.h).  Needs a bounded run and positive, strictly decreasing betas.  Combines with
 *            every other token and writes no sample file by itself, like joint
 *   autocorr fold chain 0's parameters and its column prob - prior on the device into the lag sums of the lags
 *            0 .. APEMOST_AUTOCORR_LAGS - 1 (default 1024, at most 4096; lags count kept samples); at the end write
 *            autocorr.bin and autocorr.txt: mean, variance, integrated autocorrelation time (Sokal's window and
 *            Geyer's initial positive sequence), effective sample size and standard error per column
 *            (run_autocorr.h).  Combines with every other token and writes no sample file by itself, like evidence
 *   predict  fold the model curve of chain 0's kept samples over the data's own abscissae on the device: at the end
 *            write predict.bin and predict.txt, one line per data point with x, the data, the curve's mean and
 *            standard deviation, the residual, the curve's minimum and maximum and the best-fit curve; with
 *            APEMOST_PREDICT_BINS=N and APEMOST_PREDICT_RANGE=lo:hi both set also the median and the 68 % band
 *            (run_predict.h).  Needs a bounded run and a built-in model, or a device model with the curve hook
 *            (include/apemost_device_model.h).  Combines with every other token and writes no sample file by itself,
 *            like autocorr
 *   pointwise  fold the log-likelihood term of every datum under chain 0's kept samples on the device: at the end
 *            write pointwise.bin, pointwise.txt (one line per datum with x, y, the term's mean and standard deviation,
 *            lppd, p_waic2, elpd_loo and the effective sample size of the leave-one-out weights) and criteria.txt
 *            (lppd, WAIC, leave-one-out and DIC; run_pointwise.h).  Needs a bounded run and a built-in model, or a
 *            device model with the pointwise hook (include/apemost_device_model.h).  Combines with every other token
 *            and writes no sample file by itself, like predict.  With APEMOST_POINTWISE_TAIL=auto|N (a capacity in
 *            2 .. 4096; auto sizes it for the samples the run plans) the fold keeps its tail, the largest
 *            leave-one-out log weights of every datum, and writes pointwise_tail.bin as well: `python -m
 *            apemost_amd.psis DIR` turns the two files into Pareto-smoothed leave-one-out and the Pareto k table
 *   check    fold posterior predictive checks of chain 0 on the device: per datum the predictive CDF at the observed
 *            value (PIT, leave-one-out PIT, the residual's moments), per kept sample the discrepancy statistics FIT,
 *            EXTREME and SERIAL, histogrammed over the APEMOST_CHECK_BINS (1 .. 4096, default 256) null quantiles: at
 *            the end write check.bin, check.txt and check_stats.txt (run_check.h).  Needs a built-in model, no
 *            bounded run.  Combines with every other token and writes no sample file by itself, like pointwise
 *   periodogram  fold the residual periodogram of chain 0 on the device: per kept sample the Lomb-Scargle power of
 *            y - model on the grid APEMOST_PERIODOGRAM_FREQS=lo:hi:n (required; n in 1 .. 2^20), per frequency its
 *            moments, extremes, the power of the mean residual and the count above -ln(0.01 / n), and the histogram
 *            of the highest peak's frequency: at the end write periodogram.bin and periodogram.txt
 *            (run_periodogram.h).  Needs a bounded run and simplesin or sine3.  Combines with every other token and
 *            writes no sample file by itself, like check
 *   mbar     keep loglike = (prob - prior) / beta of EVERY kept step of EVERY chain on the device and at the end solve
 *            the MBAR equations there (Shirts & Chodera 2008): write mbar.bin (the store and the free energies
 *            ln Z(beta_k) - ln Z(beta_0)) and mbar.txt (per rung beta, ln Z, E[loglike], Var[loglike] and the effective
 *            sample size of the whole ladder's samples there; then ln p(D|M,I) = ln Z(1) - ln Z(0) with its block
 *            error; run_mbar.h).  APEMOST_MBAR_TOL (default 1e-10) and APEMOST_MBAR_ITER (default 10000) set the
 *            solver's tolerance and iteration cap.  Needs a bounded run, positive, strictly decreasing betas and the
 *            whole ladder on one device.  Combines with every other token and writes no sample file by itself, like
 *            periodogram
 *   reweight keep the parameters of EVERY kept step of EVERY chain on the device beside the token mbar, which it needs
 *            in the same list, and at the end, behind MBAR's solve, form there the posterior's moments and marginal
 *            histograms from all chains' samples with the MBAR weights: write reweight.bin (the sums and the
 *            fixed-point histograms) and reweight.txt (per target and parameter beta, name, mean, sd and the effective
 *            sample size; run_reweight.h).  APEMOST_REWEIGHT_BETAS (a comma list of targets >= 0, sampled or not,
 *            default 1) and APEMOST_REWEIGHT_BINS (default 200) set the targets and the bins; the ranges are the
 *            params file's.  APEMOST_RESAMPLE_DRAWS=M (0 .. 2^24, default 0: nothing) also draws, on the device, M
 *            equally weighted samples per target from all chains' samples (systematic resampling over the fixed-point
 *            weights; APEMOST_RESAMPLE_SEED, a uint64, default 0, is its offset word) and writes resample.bin and, for
 *            target t, <paramname>-reweighted-<t>.dump, one "%.15e" line per draw, the format of
 *            <paramname>-chain-0.prob.dump.  Needs what mbar needs and no --append.  Combines with every other token and
 *            writes no sample file by itself, like mbar
 * The reference prints one line per chain per step with fprintf, which at device speed was the whole run
 * time.  Here the device formats the text lines (apemost_hip_samples_text_read_async, the
 * bytes glibc's printf gives) and the host only writes them: one fwrite per file and batch. */
#define SINK_MAGIC "APEMOSTB"
#ifndef NBINS
#define NBINS 200 /* the analyse phase's histogram bins (analyse.c) */
#endif
#ifndef PROB_FILES_OPEN_MAX
#define PROB_FILES_OPEN_MAX 256 /* beyond this many chains prob-chain files are opened per batch */
#endif

typedef struct {
    int binary;               /* 0 text, 1 binary, 2 binary with every chain's parameters */
    unsigned int folds;       /* the requested folds, bit k: run_folds[k] (run_fold.h) */
    int files;                /* sample files are written (not so for fold tokens alone) */
    unsigned int n_param_chains; /* chains 0..n-1 have parameter files (text) / carry their parameter vectors (binary) */
    double *pack;             /* binary: one batch, packed */
    size_t pack_capacity;
    unsigned long thin;
    unsigned int n_beta, n_par;
    const char *mode;  /* "w" or "a" */
    FILE *bin;         /* binary sink */
    FILE **prob_files; /* text sink, ladders up to PROB_FILES_OPEN_MAX chains: kept open */
    int batches;       /* batches written so far (pooled text files switch to append after the first) */
} sample_sink;

static void sink_parse(sample_sink *k) {
    const char *spec = getenv("APEMOST_DUMP");
    int format_given = 0, fold;
    k->binary = 0;
    k->thin = 1;
    k->folds = 0;
    for (; spec != NULL && *spec != 0; spec = run_dump_next(spec)) {
        if (strncmp(spec, "binary:all", 10) == 0)
            k->binary = 2, format_given = 1;
        else if (strncmp(spec, "binary", 6) == 0)
            k->binary = 1, format_given = 1;
        else if (strncmp(spec, "text", 4) == 0)
            k->binary = 0, format_given = 1;
        else if (strncmp(spec, "thin:", 5) == 0 && atol(spec + 5) > 0)
            k->thin = (unsigned long)atol(spec + 5);
        else if ((fold = run_fold_find(spec)) >= 0)
            k->folds |= 1u << fold;
        else {
            fprintf(stderr, "APEMOST_DUMP: expected a comma separated list of text, binary, binary:all, thin:N, summary, peaks, joint, evidence, autocorr, predict, pointwise, derived, check, periodogram, mbar, reweight; got '%s'\n", spec);
            exit(1);
        }
    }
    k->files = k->folds == 0 || format_given;
    run_folds_check(k->folds); /* what a fold refuses ends the program here, before any file is opened */
}

static void sink_open(sample_sink *k, mcmc **chains, unsigned int n_beta, unsigned int n_par, unsigned int n_swap,
                      const char *mode) {
    unsigned int i;
    char name[100];
    sink_parse(k);
    k->n_beta = n_beta;
    k->n_par = n_par;
    k->mode = mode;
    k->bin = NULL;
    k->prob_files = NULL;
    k->batches = 0;
    k->pack = NULL;
    k->pack_capacity = 0;
    k->n_param_chains = 0;
    if (!k->files)
        return;
    /* the chains with parameter files (chain 0; all with -DDUMP_ALL_CHAINS) come first in the ladder */
    while (k->n_param_chains < n_beta && chains[k->n_param_chains]->files != NULL)
        k->n_param_chains++;
    if (k->binary) {
        unsigned char header[64];
        uint32_t u32[4], u32b;
        uint64_t u64v = k->thin;
        FILE *probe = mode[0] == 'w' ? NULL : fopen("samples.bin", "rb");
        const int fresh = probe == NULL;
        if (k->binary == 2)
            k->n_param_chains = n_beta;
        u32b = k->n_param_chains;
        if (probe != NULL)
            fclose(probe);
        k->bin = run_open_or_die("samples.bin", fresh ? "wb" : "ab");
        if (fresh) {
            memset(header, 0, sizeof header);
            memcpy(header, SINK_MAGIC, 8);
            u32[0] = 2; /* format version */
            u32[1] = n_beta;
            u32[2] = n_par;
            u32[3] = n_swap;
            memcpy(header + 8, u32, sizeof u32);
            memcpy(header + 24, &u64v, sizeof u64v);
            memcpy(header + 32, &u32b, sizeof u32b);
            fwrite(header, 1, sizeof header, k->bin);
        }
        return;
    }
    if (n_beta <= PROB_FILES_OPEN_MAX) {
        k->prob_files = (FILE **)mem_calloc(n_beta, sizeof(FILE *));
        for (i = 0; i < n_beta; i++) {
            sprintf(name, "prob-chain%d.dump", i);
            k->prob_files[i] = run_open_or_die(name, mode);
        }
    }
}

/* the binary sink, the n_steps rows of a batch of a sharded ladder, `skip` its first kept step.  The rows arrive per
 * shard: h[j] = [n_steps][chains of shard j][n_par+2], shard j holding chains [lo[j], lo[j+1]) */
static void sink_write(sample_sink *k, double *const *h, const unsigned int *lo, unsigned int n_shards,
                       unsigned long skip, unsigned long n_steps) {
    const unsigned int n_par = k->n_par;
    /* one record per kept iteration: params of chains 0..n_param_chains-1, then (prob, prob - prior)
     * of every chain; packed for the whole batch, written with one call */
    const size_t record = (size_t)k->n_param_chains * n_par + 2 * (size_t)k->n_beta;
    const size_t kept = skip < n_steps ? (n_steps - skip + k->thin - 1) / k->thin : 0;
    unsigned long step;
    unsigned int i, j;
    double *out;
    if (kept * record > k->pack_capacity) {
        free(k->pack);
        k->pack_capacity = kept * record;
        k->pack = (double *)malloc(k->pack_capacity * sizeof(double));
        assert(k->pack != NULL);
    }
    out = k->pack;
    for (step = skip; step < n_steps; step += k->thin) {
        double *probs = out + (size_t)k->n_param_chains * n_par;
        for (j = 0; j < n_shards; j++) {
            const size_t row = (size_t)(lo[j + 1] - lo[j]) * (n_par + 2);
            const double *r = h[j] + step * row;
            for (i = lo[j]; i < lo[j + 1]; i++, r += n_par + 2) {
                if (i < k->n_param_chains)
                    memcpy(out + (size_t)i * n_par, r, n_par * sizeof(double));
                probs[2 * i] = r[n_par];
                probs[2 * i + 1] = r[n_par + 1];
            }
        }
        out += record;
    }
    fwrite(k->pack, sizeof(double), kept * record, k->bin);
    k->batches++;
}

/* the binary sink when the device has already packed the batch (apemost_hip_samples_pack_read_async; one
 * shard): the pinned buffer is written as it is */
static void sink_write_packed(sample_sink *k, const double *packed, unsigned long kept) {
    const size_t record = (size_t)k->n_param_chains * k->n_par + 2 * (size_t)k->n_beta;
    fwrite(packed, sizeof(double), kept * record, k->bin);
    k->batches++;
}

/* chains of shard j, [lo[j], lo[j+1]), that have parameter files */
static unsigned int sink_shard_param_chains(const sample_sink *k, const unsigned int *lo, unsigned int j) {
    if (k->n_param_chains <= lo[j])
        return 0;
    return k->n_param_chains < lo[j + 1] ? k->n_param_chains - lo[j] : lo[j + 1] - lo[j];
}

/* the text sink: the batch as the device formatted it, per shard (apemost_hip_samples_text_read_async):
 * stream c*n_par + p is parameter p of the shard's chain c, for its chains with parameter files, and the
 * stream after those is the prob-chain file of each of its chains.  One fwrite per stream; ladders beyond
 * the descriptor limit (the reference asserts n_beta < 100) open, append to and close one prob file at a time */
static void sink_write_text(sample_sink *k, mcmc **chains, char *const *text, uint64_t *const *offsets,
                            const unsigned int *lo, unsigned int n_shards) {
    const unsigned int n_par = k->n_par;
    unsigned int i, j, p;
    char name[100];
    for (j = 0; j < n_shards; j++) {
        const unsigned int n_head = sink_shard_param_chains(k, lo, j);
        const uint64_t *off = offsets[j];
        size_t s = 0;
        for (i = lo[j]; i < lo[j] + n_head; i++)
            for (p = 0; p < n_par; p++, s++)
                if (chains[i]->files != NULL && chains[i]->files[p] != NULL)
                    fwrite(text[j] + off[s], 1, off[s + 1] - off[s], chains[i]->files[p]);
        for (i = lo[j]; i < lo[j + 1]; i++, s++) {
            FILE *pf = k->prob_files ? k->prob_files[i] : NULL;
            if (pf == NULL) {
                sprintf(name, "prob-chain%d.dump", i);
                pf = run_open_or_die(name, k->batches == 0 ? k->mode : "a");
            }
            fwrite(text[j] + off[s], 1, off[s + 1] - off[s], pf);
            if (k->prob_files == NULL)
                fclose(pf);
        }
    }
    k->batches++;
}

static void sink_flush(sample_sink *k) {
    unsigned int i;
    if (k->bin)
        fflush(k->bin);
    if (k->prob_files)
        for (i = 0; i < k->n_beta; i++)
            fflush(k->prob_files[i]);
}

static void sink_close(sample_sink *k) {
    unsigned int i;
    free(k->pack);
    if (k->bin)
        fclose(k->bin);
    if (k->prob_files) {
        for (i = 0; i < k->n_beta; i++)
            fclose(k->prob_files[i]);
        mem_free(k->prob_files);
    }
}

/* The sampler loop.  The device runs batches of rounds (apemost_hip_run: n_swap steps per chain,
 * one swap attempt, ... -- the body of the reference's loop, src/parallel_tempering.c:392-409);
 * while batch k+1 runs, the rows of batch k drain into pinned host memory on a second stream and
 * are written by the sink.  Batches end at the iterations where the reference prints its
 * acceptance line (src/parallel_tempering.c:320-326, 405-407); the accept counters for that line are
 * snapshotted in stream order together with the rows, so the loop never stalls the device. */
static void run_sampler(mcmc **chains, const unsigned int n_beta, const unsigned int n_swap,
                        const unsigned long max_iterations, char *mode) {
    const unsigned int n_par = get_n_par(chains[0]);
    const size_t row = (size_t)n_beta * (n_par + 2);
    unsigned long iter = chains[0]->n_iter;
    /* rounds between two acceptance lines; batches never cross such a point */
    const unsigned long interval_rounds = PRINT_PROB_INTERVAL / gcd_ul(PRINT_PROB_INTERVAL, n_swap);
    unsigned long max_rounds = (unsigned long)(((size_t)64 << 20) / (row * n_swap * sizeof(double)));
    unsigned long rounds_now, rounds_next;
    sample_sink sink;
    FILE *acceptance_file;
    apemost_ladder *l;
    /* double-buffered per shard: device rows, pinned host rows, pinned accept/reject snapshot */
    double *d_samples[2][APEMOST_MAX_SHARDS], *h_samples[2][APEMOST_MAX_SHARDS];
    uint64_t *h_counts[2][APEMOST_MAX_SHARDS];
    double *d_packed[2] = {NULL, NULL};
    /* the text sink, double-buffered per shard: device scratch, pinned text and stream offsets, and their sizes */
    void *d_text[2][APEMOST_MAX_SHARDS];
    char *h_text[2][APEMOST_MAX_SHARDS];
    uint64_t *h_offsets[2][APEMOST_MAX_SHARDS];
    uint64_t text_streams[APEMOST_MAX_SHARDS], text_bytes[APEMOST_MAX_SHARDS], text_scratch[APEMOST_MAX_SHARDS];
    unsigned int lo[APEMOST_MAX_SHARDS + 1], n_shards, i, j;
    int k = 0, device_pack, rows_on_host, text_sink;
    run_fold_ctx folds;

    if (max_rounds < 1)
        max_rounds = 1;
    if (max_rounds > interval_rounds)
        max_rounds = interval_rounds;
    sink_open(&sink, chains, n_beta, n_par, n_swap, mode);
    acceptance_file = fopen("acceptance_rate.dump.gnuplot", "w");
    if (acceptance_file != NULL) {
        fprintf(acceptance_file, "# format: iteration | number of accepts for each chain\nplot ");
        for (i = 0; i < n_beta; i++)
            fprintf(acceptance_file, "\"acceptance_rate.dump\" u 1:%d title \"chain %d, beta = %f\"%s", i + 2, i,
                    get_beta(chains[i]), i + 1 != n_beta ? ", " : "");
        fprintf(acceptance_file, "\n");
        fclose(acceptance_file);
    }
    acceptance_file = run_open_or_die("acceptance_rate.dump", mode);

    l = apemost_ladder_open(chains, n_beta);
    n_shards = apemost_ladder_shards(l);
    for (j = 0; j <= n_shards; j++)
        lo[j] = apemost_ladder_shard_first(l, j);
    /* The text sink: the device formats each batch into the files' lines, so that only the text crosses
     * PCIe and the host writes it.  The binary sink with one shard: the device packs each batch into its
     * records, written as they arrive; with several shards the rows come to the host and are packed there. */
    text_sink = sink.files && !sink.binary;
    device_pack = sink.files && sink.binary && n_shards == 1;
    rows_on_host = sink.files && sink.binary && n_shards > 1;
    for (j = 0; j < n_shards && text_sink; j++) /* (the largest batch: max_rounds rounds, thinned from its start) */
        apemost_hip_or_die(apemost_hip_samples_text_bound(apemost_ladder_shard(l, j), max_rounds * n_swap, 0, sink.thin,
                                                          (int32_t)sink_shard_param_chains(&sink, lo, j), &text_streams[j],
                                                          &text_bytes[j], &text_scratch[j]),
                           "samples_text_bound");
    for (i = 0; i < 2; i++)
        for (j = 0; j < n_shards; j++) {
            apemost_hip_sampler *s = apemost_ladder_shard(l, j);
            const size_t n_local = lo[j + 1] - lo[j];
            void *p = NULL;
            apemost_hip_or_die(apemost_hip_samples_alloc(s, max_rounds * n_swap, &d_samples[i][j]), "samples_alloc");
            p = NULL; /* (the text sink and the folds alone bring no rows to the host) */
            if (device_pack || rows_on_host)
                apemost_hip_or_die(apemost_hip_host_alloc(max_rounds * n_swap * n_local * (n_par + 2) * sizeof(double), &p),
                                   "host_alloc");
            h_samples[i][j] = (double *)p;
            /* (+ n_par doubles: chain 0's latest point behind the counters of a packed read) */
            apemost_hip_or_die(apemost_hip_host_alloc((2 * n_local + n_par) * sizeof(uint64_t), &p), "host_alloc");
            h_counts[i][j] = (uint64_t *)p;
            d_text[i][j] = NULL;
            h_text[i][j] = NULL;
            h_offsets[i][j] = NULL;
            if (text_sink) {
                apemost_hip_or_die(apemost_hip_device_alloc(s, text_scratch[j], &d_text[i][j]), "device_alloc");
                apemost_hip_or_die(apemost_hip_host_alloc(text_bytes[j] > 0 ? text_bytes[j] : 1, &p), "host_alloc");
                h_text[i][j] = (char *)p;
                apemost_hip_or_die(apemost_hip_host_alloc((text_streams[j] + 1) * sizeof(uint64_t), &p), "host_alloc");
                h_offsets[i][j] = (uint64_t *)p;
            }
        }
    folds.l = l;
    folds.chains = chains;
    folds.lo = lo;
    folds.n_shards = n_shards;
    folds.n_swap = n_swap;
    folds.iter = iter;
    folds.max_iterations = max_iterations;
    folds.thin = sink.thin;
    folds.append = mode[0] == 'a';
    folds.model = apemost_ladder_model(l);
    folds.sigma = apemost_ladder_sigma(l);
    folds.nbins = NBINS;
    run_folds_open(sink.folds, &folds);
    for (i = 0; i < 2 && device_pack; i++)
        apemost_hip_or_die(apemost_hip_samples_alloc(apemost_ladder_shard(l, 0), max_rounds * n_swap, &d_packed[i]),
                           "samples_alloc");
    get_duration();
    run = 1;
    dumpflag = 0;
    printf("starting the analysis\n");
    fflush(stdout);

#define PLAN_BATCH(at, out)                                                                       \
    do {                                                                                          \
        (out) = 0;                                                                                \
        if (run && (max_iterations == 0 || (at) < max_iterations)) {                              \
            (out) = interval_rounds - ((at) / n_swap) % interval_rounds;                          \
            if ((out) > max_rounds)                                                               \
                (out) = max_rounds;                                                               \
            if (max_iterations != 0 && (out) > (max_iterations - (at) + n_swap - 1) / n_swap)     \
                (out) = (max_iterations - (at) + n_swap - 1) / n_swap;                            \
        }                                                                                         \
    } while (0)

    PLAN_BATCH(iter, rounds_now);
    if (rounds_now > 0)
        apemost_ladder_run(l, rounds_now, n_swap, d_samples[k]);
    while (rounds_now > 0) {
        const unsigned long n_steps = rounds_now * n_swap, iter_after = iter + n_steps;
        /* first kept step of this batch: iteration numbers count from 1 */
        const unsigned long skip = (sink.thin - (iter % sink.thin) - 1) % sink.thin;
        uint64_t kept = 0;
        if (device_pack)
            apemost_hip_or_die(apemost_hip_samples_pack_read_async(apemost_ladder_shard(l, 0), d_samples[k][0], n_steps,
                                                                   skip, sink.thin,
                                                                   (int32_t)sink.n_param_chains, 0, d_packed[k],
                                                                   h_samples[k][0], h_counts[k][0], &kept),
                               "samples_pack_read_async");
        for (j = 0; j < n_shards && rows_on_host; j++)
            apemost_hip_or_die(apemost_hip_samples_read_async(apemost_ladder_shard(l, j), d_samples[k][j], n_steps,
                                                              h_samples[k][j], h_counts[k][j]),
                               "samples_read_async");
        /* the text lines are formatted on the device, on the stream of those reads (the wait below covers it) */
        for (j = 0; j < n_shards && text_sink; j++)
            apemost_hip_or_die(apemost_hip_samples_text_read_async(apemost_ladder_shard(l, j), d_samples[k][j], n_steps,
                                                                   skip, sink.thin,
                                                                   (int32_t)sink_shard_param_chains(&sink, lo, j), d_text[k][j],
                                                                   text_scratch[j], h_text[k][j], text_bytes[j],
                                                                   h_offsets[k][j], text_streams[j] + 1),
                               "samples_text_read_async");
        /* the requested folds take the batch on the device, on the stream of those reads (the wait below covers it) */
        run_folds_accumulate(sink.folds, &folds, d_samples[k], n_steps, skip);
        /* no rows on the host (the text sink, or no sample files): only the counters and chain 0's latest point
         * cross (a packed read that keeps no step) */
        for (j = 0; j < n_shards && !device_pack && !rows_on_host; j++)
            apemost_hip_or_die(apemost_hip_samples_pack_read_async(apemost_ladder_shard(l, j), d_samples[k][j], n_steps,
                                                                   n_steps, 1, 0, 1, d_samples[k][j], (double *)h_counts[k][j],
                                                                   h_counts[k][j], NULL),
                               "samples_pack_read_async");
        PLAN_BATCH(iter_after, rounds_next);
        if (rounds_next > 0) /* the device goes on while this batch drains and is written */
            apemost_ladder_run(l, rounds_next, n_swap, d_samples[k ^ 1]);
        for (j = 0; j < n_shards; j++)
            apemost_hip_or_die(apemost_hip_samples_wait(apemost_ladder_shard(l, j)), "samples_wait");
        if (device_pack)
            sink_write_packed(&sink, h_samples[k][0], (unsigned long)kept);
        else if (rows_on_host)
            sink_write(&sink, h_samples[k], lo, n_shards, skip, n_steps);
        else if (text_sink)
            sink_write_text(&sink, chains, h_text[k], h_offsets[k], lo, n_shards);
        iter = iter_after;
        apemost_swap_round += rounds_now;
        if (iter % PRINT_PROB_INTERVAL == 0) {
            /* chain 0's latest row and counters live in shard 0 */
            /* (a packed batch holds the kept iterations only -- an older one, or none: the packed read leaves
             * chain 0's point after the batch's last step behind the counters) */
            const double *last = rows_on_host ? h_samples[k][0] + (n_steps - 1) * (size_t)(lo[1] - lo[0]) * (n_par + 2)
                                              : (const double *)(h_counts[k][0] + 2 * (lo[1] - lo[0]));
            const uint64_t accept0 = h_counts[k][0][0], reject0 = h_counts[k][0][lo[1] - lo[0]];
            if (dumpflag) {
                /* a report on request: the ladder as the device holds it now (a batch ahead of
                 * the rows just written when another one is already running) */
                apemost_ladder_download(l);
                report((const mcmc **)chains, (int)n_beta);
                dumpflag = 0;
                sink_flush(&sink);
            }
            fprintf(acceptance_file, "%lu", iter);
            for (j = 0; j < n_shards; j++)
                for (i = 0; i < lo[j + 1] - lo[j]; i++)
                    fprintf(acceptance_file, "\t%lu", (unsigned long)h_counts[k][j][i]);
            fprintf(acceptance_file, "\n");
            fflush(acceptance_file);
            printf("iteration: %lu, a/r: %.3f(%lu/%lu), v:", iter, (double)accept0 / (double)(accept0 + reject0),
                   (unsigned long)accept0, (unsigned long)reject0);
            printf("Vector%ud[", n_par); /* dump_vector's format, from the row instead of a gsl_vector */
            for (i = 0; i < n_par; i++)
                printf("%f%s", last[i], i + 1 < n_par ? ";" : "]");
            printf(" [%d/%lu ticks]\r", get_duration(), get_ticks_per_second());
            fflush(stdout);
        }
        rounds_now = rounds_next;
        k ^= 1;
    }
#undef PLAN_BATCH
    apemost_ladder_download(l);
#ifdef TRACK_REPLICAS
    apemost_write_replica_flow(l);
#endif
    run_folds_close(sink.folds, &folds);
    for (i = 0; i < 2; i++)
        for (j = 0; j < n_shards; j++) {
            apemost_hip_samples_free(apemost_ladder_shard(l, j), d_samples[i][j]);
            apemost_hip_host_free(h_samples[i][j]);
            apemost_hip_host_free(h_counts[i][j]);
            apemost_hip_device_free(apemost_ladder_shard(l, j), d_text[i][j]);
            apemost_hip_host_free(h_text[i][j]);
            apemost_hip_host_free(h_offsets[i][j]);
        }
    for (i = 0; i < 2; i++)
        if (d_packed[i] != NULL)
            apemost_hip_samples_free(apemost_ladder_shard(l, 0), d_packed[i]);
    apemost_ladder_close(l);
    fclose(acceptance_file);
    sink_close(&sink);
    printf("handled %lu iterations on %d chains\n", iter, n_beta);
}

void prepare_and_run_sampler(const unsigned long max_iterations, int append) {
    const unsigned int n_beta = apemost_n_beta();
    int n_swap = N_SWAP;
    char *mode = (append == 1 ? "a" : "w");
    mcmc **chains = setup_chains();
    sample_sink wanted;
#ifdef DUMP_ALL_CHAINS
    unsigned int i;
#endif
    read_calibration_file(chains, n_beta);
    sink_parse(&wanted);
    if (wanted.files) {
        mcmc_open_dump_files(chains[0], "-chain", 0, mode);
#ifdef DUMP_ALL_CHAINS
        for (i = 1; i < n_beta; i++)
            mcmc_open_dump_files(chains[i], "-chain", i, mode);
#endif
    }
    if (n_swap < 0) {
        n_swap = 2000 / n_beta;
        printf("automatic n_swap: %d\n", n_swap);
    }
    if (n_swap < 1) {
        /* the reference's rule yields 0 beyond 2000 chains and then never advances */
        fprintf(stderr, "n_swap = %d: set -DN_SWAP to a positive value for ladders of more than 2000 chains\n",
                n_swap);
        exit(1);
    }
    register_signal_handlers();
    run_sampler(chains, n_beta, (unsigned int)n_swap, max_iterations, mode);
    report((const mcmc **)chains, (int)n_beta);
    free_chains(chains, n_beta);
}
