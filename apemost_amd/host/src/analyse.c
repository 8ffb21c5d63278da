/* `analyse` phase: post-processing of the run phase's dump files on the host (disk-bound work,
 * outside the GPU path).  Same inputs, outputs and formulas as reference
 * src/analyse.c:33-285 and its histogram helper (src/histogram.c:33-42, create_hist): the thermodynamic
 * integral over beta of the mean log-likelihood, and per-parameter marginal histograms with a
 * batch-means Monte-Carlo error.  The reference's n_beta < 100 limit does not apply.
 * With `summary` in APEMOST_DUMP the same numbers come from summary.bin (run_summary.h), the sums the
 * device folded during the run, instead of the dump files; the printed lines and written files are the same. */
#include <math.h>
#include <string.h>
#include "mcmc.h"
#include "parallel_tempering.h"
#include "parallel_tempering_config.h"
#include "utils.h"
#include "debug.h"
#include "run_fold.h"
#include "run_summary.h"
#include "histogram.h"

#ifndef NBINS
#define NBINS 200
#endif
#ifndef GNUPLOT_STYLE
#define GNUPLOT_STYLE "with histeps"
#endif

/* ln p(D|M) = integral over beta of <ln L>_beta: per chain the mean of column 2 of
 * prob-chain<i>.dump (prob - prior = beta * ln L) divided by beta, rectangle rule from the
 * hottest chain down to beta = 1 */
static void read_summary_or_die(run_summary *r, unsigned int n_beta, unsigned int n_par) {
    if (run_summary_read(RUN_SUMMARY_FILE, r) != 0) {
        fprintf(stderr, "APEMOST_DUMP=summary: %s not found\n", RUN_SUMMARY_FILE);
        exit(1);
    }
    if (r->n_beta != n_beta || r->n_par != n_par || r->nbins != NBINS || r->n_hist < 1) {
        fprintf(stderr, "%s holds %u chains, %u parameters, %u bins; this analysis has %u, %u, %d\n", RUN_SUMMARY_FILE,
                r->n_beta, r->n_par, r->nbins, n_beta, n_par, NBINS);
        exit(1);
    }
}

void analyse_data_probability() {
    const unsigned int n_beta = apemost_n_beta();
    mcmc **chains = setup_chains();
    double *mean = (double *)calloc(n_beta, sizeof(double));
    double logprob = 0, previous_beta = 0;
    unsigned int i, j;
    run_summary summary;
    const int from_summary = run_dump_requested("summary");
    read_calibration_file(chains, n_beta);
    if (from_summary)
        read_summary_or_die(&summary, n_beta, get_n_par(chains[0]));
    for (i = 0; i < n_beta && from_summary; i++) {
        printf("reading probabilities of chain %d\r", i);
        fflush(stdout);
        if (summary.n == 0) {
            fprintf(stderr, "calculating data probability failed: no data points found in %s\n", RUN_SUMMARY_FILE);
            return;
        }
        mean[i] = summary.prob_sum[i] / get_beta(chains[i]) / summary.n;
    }
    if (from_summary)
        run_summary_free(&summary);
    for (i = 0; i < n_beta && !from_summary; i++) {
        char name[100];
        FILE *f;
        double total, part, sum = 0;
        unsigned long n = 0;
        sprintf(name, "prob-chain%d.dump", i);
        printf("reading probabilities of chain %d\r", i);
        fflush(stdout);
        f = fopen(name, "r");
        if (f == NULL) {
            fprintf(stderr, "calculating data probability failed: file %s not found\n", name);
            return;
        }
        while (fscanf(f, "%le\t%le", &total, &part) == 2) {
            sum += part;
            n++;
        }
        fclose(f);
        if (n == 0) {
            fprintf(stderr, "calculating data probability failed: no data points found in %s\n", name);
            return;
        }
        mean[i] = sum / get_beta(chains[i]) / n;
    }
    for (j = n_beta; j-- > 0;) {
        assert(get_beta(chains[j]) > previous_beta);
        logprob += mean[j] * (get_beta(chains[j]) - previous_beta);
        previous_beta = get_beta(chains[j]);
    }
    printf("Model probability ln(p(D|M, I)): [about 10^%.0f] %.5f\n"
           "\nTable to compare support against other models (Jeffrey):\n"
           " other model ln(p(D|M,I)) | supporting evidence for this model\n"
           " --------------------------------- \n"
           "        >  %04.1f \tnegative (supports other model)\n"
           "  %04.1f .. %04.1f \tBarely worth mentioning\n"
           "  %04.1f .. %04.1f \tSubstantial\n"
           "  %04.1f .. %04.1f \tStrong\n"
           "  %04.1f .. %04.1f \tVery strong\n"
           "        <  %04.1f \tDecisive\n",
           logprob / log(10.0), logprob, logprob, logprob, logprob - log(3.0), logprob - log(3.0),
           logprob - log(10.0), logprob - log(10.0), logprob - log(30.0), logprob - log(30.0),
           logprob - log(100.0), logprob - log(100.0));
    printf("\nbe careful.\n");
    free(mean);
}

/* the same from the batch sums of a run summary: batch k's sum is batch_sums[k] */
static double batch_means_error_summary(double mean, const double *batch_sums, uint64_t nbatches, unsigned long batchsize) {
    double errorsum = 0;
    uint64_t k;
    for (k = 0; k < nbatches; k++) {
        const double d = batch_sums[k] / batchsize - mean;
        errorsum += d * d;
    }
    return sqrt(errorsum / (int)nbatches);
}

/* spread of the batch means (batches of `batchsize` consecutive samples) around the mean */
static double batch_means_error(double mean, const char *filename, unsigned long batchsize) {
    FILE *f = openfile(filename);
    double v, batchsum = 0, errorsum = 0;
    unsigned long n = 0;
    int nbatches = 0;
    while (fscanf(f, "%lf", &v) == 1) {
        n++;
        batchsum += v;
        if (n % batchsize == batchsize - 1) {
            const double d = batchsum / batchsize - mean;
            errorsum += d * d;
            batchsum = 0;
            nbatches++;
        }
    }
    fclose(f);
    return sqrt(errorsum / nbatches);
}

/* NBINS-bin density of one parameter's visited values (chain 0) over [min, max] of the prior box
 * (or of the data with -DHISTOGRAMS_MINMAX), on the reference's own histogram: create_hist() -- GSL's
 * uniform edges ((n-b)/n)*min + (b/n)*max, the top one widened by 1e-4 of the range so the maximum falls
 * into the last bin -- gsl_histogram_increment, _scale, _fprintf, _mean and _sigma, call for call as
 * reference src/analyse.c:216-240.  With a run summary the counts come from it instead of the increments;
 * the device binned them on the same edges.  Output: "<name>.histogram", lines "lower upper density". */
static void marginal_distribution(mcmc **chains, unsigned int param, int find_minmax, const run_summary *summary) {
    const char *name = get_params_descr(chains[0])[param];
    double lo = get_params_min_for(chains[0], param), hi = get_params_max_for(chains[0], param);
    double v, total, mean, sigma, err;
    char in_name[300], out_name[300];
    gsl_histogram *h;
    FILE *f;
    int b;
    sprintf(in_name, "%s-chain-%d.prob.dump", name, 0);
    sprintf(out_name, "%s.histogram", name);
    if (summary != NULL) {
        lo = summary->lo[param]; /* the range the device binned with */
        hi = summary->hi[param];
    } else if (get_column_count(in_name) != 1) {
        fprintf(stderr, "number of columns different in file %s\n", in_name);
        exit(1);
    }
    if (find_minmax) {
        int first = 1;
        f = openfile(in_name);
        while (fscanf(f, "%lf", &v) == 1) {
            if (first || v < lo)
                lo = v;
            if (first || v > hi)
                hi = v;
            first = 0;
        }
        fclose(f);
    }
    h = create_hist(NBINS, lo, hi);
    printf("reading values: chain %3d parameter %s   \r", 0, name);
    fflush(stdout);
    if (summary != NULL)
        for (b = 0; b < NBINS; b++)
            h->bin[b] = (double)summary->hist[(size_t)param * NBINS + b];
    else
        append_to_hists(&h, 1, in_name);
    total = gsl_histogram_sum(h);
    gsl_histogram_scale(h, (hi - lo) / NBINS / total);
    f = fopen(out_name, "w");
    assert(f != NULL);
    gsl_histogram_fprintf(f, h, DUMP_FORMAT, DUMP_FORMAT);
    fclose(f);
    mean = gsl_histogram_mean(h);
    sigma = gsl_histogram_sigma(h);
    gsl_histogram_free(h);
    if (summary != NULL) {
        const unsigned long want = (unsigned long)sqrt(total);
        err = batch_means_error_summary(mean, summary->batch_sums + (size_t)param * (summary->max_batches + 1),
                                        summary->n_batches, (unsigned long)summary->bs);
        if (summary->bs != want)
            fprintf(stderr, "%s: batch size %lu recorded in %s, floor(sqrt(%.0f values)) = %lu\n", name,
                    (unsigned long)summary->bs, RUN_SUMMARY_FILE, total, want);
    } else
        err = batch_means_error(mean, in_name, (unsigned long)sqrt(total));
    printf("mcmc error estimate of %s: %f %s\n", name, err, (err > sigma * 0.01 ? "** high!" : " (ok)"));
    printf("Note: Include a error estimate in your publication!\n");
}

void analyse_marginal_distributions() {
    const unsigned int n_beta = apemost_n_beta();
    mcmc **chains = setup_chains();
    const unsigned int n_par = get_n_par(chains[0]);
    int find_minmax = 0;
    unsigned int i;
    FILE *plot;
    run_summary summary;
    const int from_summary = run_dump_requested("summary");
    read_calibration_file(chains, n_beta);
#ifdef HISTOGRAMS_MINMAX
    find_minmax = 1;
    if (from_summary) {
        fprintf(stderr, "APEMOST_DUMP=summary cannot be combined with -DHISTOGRAMS_MINMAX: the histogram range "
                        "would have to be known before the first sample\n");
        exit(1);
    }
#endif
    if (from_summary)
        read_summary_or_die(&summary, n_beta, n_par);
    for (i = 0; i < n_par; i++)
        marginal_distribution(chains, i, find_minmax, from_summary ? &summary : NULL);
    if (from_summary)
        run_summary_free(&summary);
    plot = fopen("marginal_distributions.gnuplot", "w");
    assert(plot != NULL);
    fprintf(plot, "# set terminal png size %d,%d; set output \"marginal_distributions.png\"\n", 600, 300 * n_par);
    fprintf(plot, "set multiplot\n");
    fprintf(plot, "set size 1,%f\n", 1. / n_par);
    for (i = 0; i < n_par; i++) {
        fprintf(plot, "set origin 0,%f\n", (n_par - i - 1) * 1. / n_par);
        fprintf(plot, "plot \"%s.histogram\" u 1:3 title \"%s\" " GNUPLOT_STYLE "\n", get_params_descr(chains[0])[i],
                get_params_descr(chains[0])[i]);
    }
    fprintf(plot, "unset multiplot\n");
    fclose(plot);
}
