/* predict.bin and predict.txt: the APEMOST_DUMP token `predict` (include/apemost_hip.h, apemost_hip_predict_*).
 * The run phase folds the model curve of chain 0's kept samples over the data's own abscissae (column 0) on the device:
 * per abscissa the sums that give the curve's mean and standard deviation, its minimum and maximum and -- only when
 * APEMOST_PREDICT_BINS=N and APEMOST_PREDICT_RANGE=lo:hi are both set -- a histogram of its values, which gives the
 * median and the 68 % credible band; per chain the best sample, whose curve is the best fit.
 *
 * predict.bin (little-endian), version 1; apemost_amd/predict.py reads and writes the same bytes:
 *   char[8]  "APEMOSTP"
 *   uint32   version, n_keep, n_x, nbins, n_par, n_ladders, model, 0
 *   uint64   n, thin
 *   double   lo, hi
 *   int32    chains[n_keep]
 *   double   x[n_keep][n_x]
 *   double   origin, sum, sq, vmin, vmax: [n_keep][n_x] each
 *   uint64   hist[n_keep][n_x][nbins]
 *   double   best_prob[n_keep], best_params[n_keep][n_par]
 *   uint64   best_n[n_keep]
 * predict.txt: one line per abscissa, `x y mean sd residual min max best` and, with histograms, `median lower68
 * upper68`, tab separated, "%.15e": the text of Predict.text() of apemost_amd/predict.py, whose formulas run_predict.c
 * repeats operation for operation.  The residual is y - mean for the sine models and y / mean for the pulse models.
 *
 * run_predict.c needs neither the device nor the chains: run_predict_read, _write and _write_text stand alone.
 * run_predict_device.c holds run_predict_open and _close. */
#ifndef RUN_PREDICT_H
#define RUN_PREDICT_H
#include <stdint.h>

#define RUN_PREDICT_FILE "predict.bin"
#define RUN_PREDICT_TEXT "predict.txt"

/* one kept chain (n_keep == 1, n_ladders == 1) */
typedef struct {
    uint32_t n_x, nbins, n_par, model;
    int32_t chain;
    uint64_t n, thin;
    double lo, hi;
    double *x;                /* [n_x] */
    double *origin, *sum, *sq, *vmin, *vmax; /* [n_x] */
    uint64_t *hist;           /* [n_x][nbins] */
    double best_prob;
    double *best_params;      /* [n_par] */
    uint64_t best_n;
} run_predict;

/* allocates the arrays of a state whose n_x, nbins and n_par are set; the state of a fold before its first sample */
void run_predict_alloc(run_predict *r);
void run_predict_free(run_predict *r);
/* 0: read; -1: no such file; 1: a file of several kept chains (nothing is allocated).  Another magic, version or a
 * truncated file ends the program. */
int run_predict_read(const char *path, run_predict *r);
void run_predict_write(const char *path, const run_predict *r);
/* the q-quantile of abscissa i's counted values, linear inside its bin; NaN where nothing was counted.
 * edges: [nbins + 1] from run_predict_edges */
void run_predict_edges(const run_predict *r, double *edges);
double run_predict_quantile(const run_predict *r, const double *edges, uint32_t i, double q);
/* y: data column 1, best: the best-fit curve, [n_x] each */
void run_predict_write_text(const char *path, const run_predict *r, const double *y, const double *best);

#endif
