/* What the run_*.c files (run summary, joint marginals, evidence, autocorrelation, predictive, pointwise) share
 * when they allocate, read and write their files: a failure prints one line and ends the program.  `what` is the
 * word by which the messages of the files differ.  Below those, the arithmetic more than one fold states: the
 * summary's bin edge, the triangle's size, the batches of the error estimate and the --append check of ranges.
 * (static __inline__: the strict build is C90, which has no inline, and a file need not use every helper.) */
#ifndef RUN_IO_H
#define RUN_IO_H

#include <math.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

/* count elements (at least one) of `size` bytes, zeroed */
static __inline__ void *run_alloc_or_die(size_t count, size_t size, const char *what) {
    void *p = calloc(count > 0 ? count : 1, size);
    if (p == NULL) {
        fprintf(stderr, "%s: out of memory\n", what);
        exit(1);
    }
    return p;
}

static __inline__ void run_read_or_die(void *p, size_t size, size_t count, FILE *f, const char *path, const char *what) {
    if (count > 0 && fread(p, size, count, f) != count) {
        fprintf(stderr, "%s: truncated %s\n", path, what);
        exit(1);
    }
}

static __inline__ FILE *run_open_or_die(const char *path, const char *mode) {
    FILE *f = fopen(path, mode);
    if (f == NULL) {
        fprintf(stderr, "opening file %s failed\n", path);
        perror("opening file failed");
        exit(1);
    }
    return f;
}

static __inline__ void run_close_or_die(FILE *f, const char *path) {
    if (fclose(f) != 0) {
        fprintf(stderr, "writing %s failed\n", path);
        exit(1);
    }
}

/* a value of a text output: 15 digits, a NaN without its sign */
static __inline__ void run_print_value(FILE *f, double v) {
    if (v != v)
        fprintf(f, "nan");
    else
        fprintf(f, "%.15e", v);
}

/* n such values, tab separated.  Every argument after n must be a double: the list is untyped, and an int there
 * compiles clean and is undefined behaviour, so cast what is not one */
static __inline__ void run_print_values(FILE *f, int n, ...) {
    va_list ap;
    int i;
    va_start(ap, n);
    for (i = 0; i < n; i++) {
        if (i > 0)
            fprintf(f, "\t");
        run_print_value(f, va_arg(ap, double));
    }
    va_end(ap);
}

/* the summary's edge b of n over [lo, hi] (gsl_histogram_set_ranges_uniform, the top one widened as create_hist()).
 * The definition it must follow is summary_edge of apemost_amd/csrc/pt_summary.h, which bins the samples: the same
 * two products and one sum, unfused (summary.edges of apemost_amd/summary.py is the Python statement of it). */
static __inline__ double run_summary_edge(double lo, double hi, unsigned int b, unsigned int n) {
    const double f1 = (double)(n - b) / (double)n, f2 = (double)b / (double)n;
    double e = f1 * lo;
    const double t = f2 * hi;
    e = e + t;
    if (b == n)
        e += (hi - lo) / 10000;
    return e;
}

/* entries of the row-major upper triangle, diagonal included, of an n x n matrix */
static __inline__ size_t run_tri_count(size_t n) {
    return n * (n + 1) / 2;
}

/* batches batch_means_error() has closed after n samples (sample n, counted from 1, closes one when
 * n % bs == bs - 1) */
static __inline__ uint64_t run_batches_closed(uint64_t n, uint64_t bs) {
    return bs == 1 ? n : (n + 1) / bs;
}

/* batch size of the error estimate: the old file's on append, else floor(sqrt(planned)), at least 1 */
static __inline__ uint64_t run_batch_size(int resumed, uint64_t old_bs, uint64_t planned) {
    const uint64_t bs = resumed ? old_bs : (uint64_t)sqrt((double)planned);
    return bs < 1 ? 1 : bs;
}

/* --append: the ranges of `file` must be this run's; `what` is `parameter` or `column` */
static __inline__ void run_check_ranges_or_die(const char *file, const char *what, unsigned int n, const double *old_lo,
                                               const double *old_hi, const double *lo, const double *hi) {
    unsigned int p;
    for (p = 0; p < n; p++)
        if (old_lo[p] != lo[p] || old_hi[p] != hi[p]) {
            fprintf(stderr, "%s: %s %u had the range [%g, %g], now [%g, %g]; cannot append\n", file, what, p, old_lo[p],
                    old_hi[p], lo[p], hi[p]);
            exit(1);
        }
}

#endif
