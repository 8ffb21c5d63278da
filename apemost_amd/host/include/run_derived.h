/* derived.bin, derived.txt and <name>.histogram: the APEMOST_DUMP token `derived` (include/apemost_hip.h,
 * apemost_hip_derived_*).  The run phase folds functions of chain 0's sample rows on the device -- what the
 * reference's tools/matrix_man.c computes over the text dumps and pipes into histogram_tool -- and writes the files
 * when it ends.  The columns come from the file `derived` in the working directory, or from the file that
 * APEMOST_DERIVED_FILE names.  Each line is
 *     name lo hi token token ...
 * with the column's name (the stem of its .histogram file), its histogram range and its program in reverse Polish
 * notation: a name of the `params` file, `prob` or `like` (prob - prior) pushes that value, a number pushes itself,
 * and dup swap add sub mul div neg abs inv sqrt floor min max log exp sin cos atan2 act on the stack (`f2 f1 sub` is
 * f2 - f1, `y x atan2` is atan2(y, x)).  `#` starts a comment.  A bad line ends the run before the first launch with
 * its number.  All pairs of columns are folded while there are at most RUN_DERIVED_PAIR_COLUMNS columns, none beyond
 * (the moments, and with them the covariance, are always folded).
 *
 * derived.bin (little-endian), version 1; apemost_amd/derived.py documents the layout and reads and writes the same
 * bytes.  derived.txt: one line per column, `name n mean sd mcse min max nonfinite`, tab separated, "%.15e".
 * <name>.histogram: lines "lower upper density" as `analyse` writes them for a parameter. */
#ifndef RUN_DERIVED_H
#define RUN_DERIVED_H
#include <stdint.h>

#include "apemost_hip.h"

#define RUN_DERIVED_FILE "derived.bin"
#define RUN_DERIVED_SPEC "derived"
#define RUN_DERIVED_PAIR_COLUMNS 8
#define RUN_DERIVED_MESSAGE 400

typedef struct {
    uint32_t n_par, n_col, nbins, n_pairs, n_const;
    uint64_t n, thin, bs, max_batches;
    /* the columns (run_derived_parse, or the head of derived.bin) */
    char **names, **rpn;      /* [n_col] */
    char **row_names;         /* [n_par] */
    int32_t *code, *start;    /* [start[n_col]], [n_col + 1] */
    double *consts;           /* [n_const] */
    double *lo, *hi;          /* [n_col] */
    int32_t *pairs;           /* [n_pairs][2] */
    /* the accumulator (run_derived_alloc) */
    uint64_t *hist;           /* [n_col][nbins] */
    double *batch;            /* [n_col][max_batches + 1] */
    uint64_t *nonfinite;      /* [n_col] */
    double *vmin, *vmax, *origin, *sum; /* [n_col] */
    double *cross;            /* [n_col (n_col + 1) / 2] */
    uint64_t *counts;         /* [n_pairs][nbins][nbins] */
} run_derived;

/* The columns of the text of a derived file over the `n_par` parameter names: names, ranges, RPN text and programs of
 * `r` (zeroed first; free with run_derived_free).  Needs no device.  Returns 0, or the number of the first bad line
 * (from 1) with one line about it in message[RUN_DERIVED_MESSAGE], or -1 for a text without a column. */
int run_derived_parse(const char *text, unsigned int n_par, const char *const *param_names, run_derived *r, char *message);
void run_derived_alloc(run_derived *r);
void run_derived_free(run_derived *r);
/* 0: read (columns and accumulator); -1: no such file.  A file that is not a derived file of one kept chain ends the
 * program. */
int run_derived_read(const char *path, run_derived *r);
void run_derived_write(const char *path, const run_derived *r);
/* derived.txt and one <name>.histogram per column, in the working directory */
void run_derived_write_text(const run_derived *r);

#endif
