/* joint.bin, <a>-<b>.joint and correlation.matrix: the APEMOST_DUMP token `joint` (include/apemost_hip.h,
 * apemost_hip_joint_*).  The run phase folds chain 0's rows on the device into one NBINS x NBINS histogram per pair of
 * parameters, over the prior box and on the bins of the analyse phase's marginal histograms, and into the moments
 * that give the parameter covariance -- what a corner plot needs -- without the sample dump having been written.
 *
 * joint.bin (little-endian), version 1; apemost_amd/joint.py reads and writes the same bytes:
 *   char[8]  "APEMOSTJ"
 *   uint32   version, n_keep, n_par, nbins, n_pairs, 0
 *   uint64   n, thin
 *   int32    chains[n_keep]
 *   int32    pairs[n_pairs][2]
 *   double   lo[n_par], hi[n_par]
 *   double   origin[n_keep][n_par], sum[n_keep][n_par]
 *   double   cross[n_keep][n_par (n_par + 1) / 2]
 *   uint64   counts[n_keep][n_pairs][nbins][nbins]
 * <a>-<b>.joint: `x_lower x_upper y_lower y_upper count` per cell, edges as "%.15e", x-major, a blank line after each
 * x row (gnuplot: splot "<a>-<b>.joint" using 1:3:5 with pm3d).  correlation.matrix: n_par lines of n_par
 * correlation coefficients, "%.15e", tab separated. */
#ifndef RUN_JOINT_H
#define RUN_JOINT_H
#include <stdint.h>

#include "apemost_hip.h"
#include "mcmc.h"

#define RUN_JOINT_FILE "joint.bin"

typedef struct {
    uint32_t n_par, nbins, n_pairs;
    uint64_t n, thin;
    int32_t *pairs;           /* [n_pairs][2] */
    double *lo, *hi;          /* [n_par] */
    double *origin, *sum;     /* [n_par] */
    double *cross;            /* [n_par (n_par + 1) / 2] */
    uint64_t *counts;         /* [n_pairs][nbins][nbins] */
} run_joint;

/* begins the joint marginals of local chain 0 of shard `s`: all pairs, `nbins` bins, the prior box of `chain0`.  With
 * `append` joint.bin is loaded and the accumulation goes on from it; a file of another shape, nbins, thin or range
 * ends the program with the messages a summary.bin of another shape gets. */
void run_joint_open(run_joint *r, apemost_hip_sampler *s, const mcmc *chain0, unsigned int nbins, uint64_t thin,
                    int append);
/* collects the accumulator, writes joint.bin, the .joint files and correlation.matrix, and frees everything */
void run_joint_close(run_joint *r, apemost_hip_sampler *s, const mcmc *chain0);

#endif
