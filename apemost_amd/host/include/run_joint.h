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

/* allocates the arrays of a state whose n_par, nbins and n_pairs are set; everything zero */
void run_joint_alloc(run_joint *r);
void run_joint_free(run_joint *r);
/* 0: read; -1: no such file.  *n_keep and *chain receive the kept chains and the first of them; a file of another
 * n_keep or of sizes out of range is left unallocated for the caller to refuse by its shape.  Another magic, version
 * or a truncated file ends the program. */
int run_joint_read(const char *path, run_joint *r, uint32_t *n_keep, int32_t *chain);
void run_joint_write(const char *path, const run_joint *r);
/* <names[a]>-<names[b]>.joint of pair q, and correlation.matrix, in the working directory */
void run_joint_write_pair(const run_joint *r, unsigned int q, const char **names);
void run_joint_write_correlation(const run_joint *r);

#endif
