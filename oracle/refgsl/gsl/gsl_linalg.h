/*
 * gsl_linalg.h -- the part of the GSL surface that only the compiled reference needs
 * (oracle/ref_build.py); the host layer's own headers (apemost_amd/host/gsl) carry the rest.
 *
 * TEST INFRASTRUCTURE ONLY, like everything under oracle/.
 *
 *   gsl_vector_int_{alloc,free,get,set,set_all}   used by the reference's alternative calibrations
 *                                                 (src/markov_chain_calibrate.c:264,473), which the
 *                                                 default dispatch never reaches
 *   gsl_permutation, gsl_linalg_LU_{decomp,solve} used by a regression helper (src/gsl_helper.c:196-268),
 *                                                 also off the default path: they abort with a message,
 *                                                 so that a pinned run can never have gone through them
 *
 * Plain C90 (the reference compiles with -ansi): no inline, static functions only.
 */
#ifndef APEMOST_REFGSL_GSL_LINALG_H
#define APEMOST_REFGSL_GSL_LINALG_H
#include <stdio.h>
#include <stdlib.h>
#include <gsl/gsl_matrix.h>
#include <gsl/gsl_vector.h>

#if defined(__GNUC__)
#define REFGSL_UNUSED __attribute__((unused))
#else
#define REFGSL_UNUSED
#endif

typedef struct {
    size_t size;
    int *data;
} gsl_vector_int;

static REFGSL_UNUSED gsl_vector_int *gsl_vector_int_alloc(const size_t n) {
    gsl_vector_int *v = (gsl_vector_int *)malloc(sizeof(gsl_vector_int));
    if (v == NULL)
        abort();
    v->size = n;
    v->data = (int *)calloc(n ? n : 1, sizeof(int));
    if (v->data == NULL)
        abort();
    return v;
}

static REFGSL_UNUSED void gsl_vector_int_free(gsl_vector_int *v) {
    if (v != NULL) {
        free(v->data);
        free(v);
    }
}

static REFGSL_UNUSED int gsl_vector_int_get(const gsl_vector_int *v, const size_t i) {
    if (i >= v->size) {
        fprintf(stderr, "refgsl: gsl_vector_int_get: index out of range\n");
        abort();
    }
    return v->data[i];
}

static REFGSL_UNUSED void gsl_vector_int_set(gsl_vector_int *v, const size_t i, int x) {
    if (i >= v->size) {
        fprintf(stderr, "refgsl: gsl_vector_int_set: index out of range\n");
        abort();
    }
    v->data[i] = x;
}

static REFGSL_UNUSED void gsl_vector_int_set_all(gsl_vector_int *v, int x) {
    size_t i;
    for (i = 0; i < v->size; i++)
        v->data[i] = x;
}

typedef struct {
    size_t size;
    size_t *data;
} gsl_permutation;

static REFGSL_UNUSED gsl_permutation *gsl_permutation_alloc(const size_t n) {
    gsl_permutation *p = (gsl_permutation *)malloc(sizeof(gsl_permutation));
    if (p == NULL)
        abort();
    p->size = n;
    p->data = (size_t *)calloc(n ? n : 1, sizeof(size_t));
    if (p->data == NULL)
        abort();
    return p;
}

static REFGSL_UNUSED void gsl_permutation_free(gsl_permutation *p) {
    if (p != NULL) {
        free(p->data);
        free(p);
    }
}

static REFGSL_UNUSED int gsl_linalg_LU_decomp(gsl_matrix *a, gsl_permutation *p, int *signum) {
    (void)a;
    (void)p;
    (void)signum;
    fprintf(stderr, "refgsl: gsl_linalg_LU_decomp is not provided (off the pinned paths)\n");
    abort();
    return 1;
}

static REFGSL_UNUSED int gsl_linalg_LU_solve(const gsl_matrix *lu, const gsl_permutation *p, const gsl_vector *b,
                                             gsl_vector *x) {
    (void)lu;
    (void)p;
    (void)b;
    (void)x;
    fprintf(stderr, "refgsl: gsl_linalg_LU_solve is not provided (off the pinned paths)\n");
    abort();
    return 1;
}

#endif
