/* What the run_*.c files (run summary, joint marginals, evidence, autocorrelation, predictive, pointwise) share
 * when they allocate, read and write their files: a failure prints one line and ends the program.  `what` is the
 * word by which the messages of the files differ.  (static __inline__: the strict build is C90, which has no
 * inline, and a file need not use every helper.) */
#ifndef RUN_IO_H
#define RUN_IO_H

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

#endif
