/*
 * apemost_device_model.h -- what a user-supplied DEVICE likelihood implements.
 *
 * APEMoST's plugin surface is the pair calc_model() / calc_model_for() (src/mcmc.h:164,173): host C,
 * called once per Metropolis update.  The engine's built-in device models cover the BASELINE apps;
 * any other likelihood (apps/simplesin2.c, apps/normal.c, apps/bernoulli_example.c, or a function
 * registered through set_function, apps/library.c:6-22) is given to the engine as device source:
 * a file with the two functions below, named in apemost_hip_config.device_model_source (C host:
 * environment variable APEMOST_DEVICE_MODEL_SRC).  The engine compiles it with hiprtc into its
 * one-wave round, calibration and evaluation kernels when the sampler is created.  The C host layer
 * accepts it only if it reproduces the application's own host calc_model() on probe points
 * (apemost_detect_model: 1e-9).
 *
 * The likelihood is taken as  m->prob = finish( sum_i term(i) ):  term() is what the loop over the
 * data rows of a calc_model() adds per row (the engine sums the terms in a fixed order over the 64
 * lanes of the chain's wavefront), finish() is everything else: get_beta(m), the prior, set_prob /
 * set_prior.  A likelihood without a data loop returns 0 from term().
 *
 * Under APEMOST_HIP_FLAG_USER_ONE_BARRIER (include/apemost_hip.h) the model also runs in the one-barrier kernels.
 * There every lane of every likelihood wave calls finish(), and so does the chain's own wave, so finish() must
 * be a pure function of (ctx, sum, beta) and must not read *prior before it writes it.  The example sources in
 * apemost_amd/host/examples/device_models/ satisfy this.
 *
 * Two OPTIONAL hooks open the on-device posterior predictive (apemost_hip_predict_*: the fitted curve, its bands,
 * the best fit) and the on-device pointwise log-likelihood (apemost_hip_pointwise_*: WAIC, leave-one-out, DIC) to
 * the model.  A file announces a hook by defining its macro itself, anywhere in the file, and then defines the
 * function:
 *     #define APEMOST_USER_CURVE 1        and  apemost_user_curve(ctx, i)
 *     #define APEMOST_USER_POINTWISE 1    and  apemost_user_pointwise(ctx, i)
 * The engine learns which hooks exist from the preprocessor when it compiles the file a second time, on the first
 * predict_* or pointwise_* call (a comment that names a macro announces nothing; a macro without its function does
 * not compile).  A file with neither hook behaves as it always did: those calls return APEMOST_HIP_ERR_UNSUPPORTED.
 * A file with one hook gets that feature only.  Like finish() under the one-barrier rule above, both hooks must be
 * pure functions of (ctx, i): they are called for the same row and parameters more than once, from kernels that
 * hold nothing of a chain's state, with ctx->params pointing into on-chip memory, and never for i >= ctx->n_data.
 * In a hook ctx->data are the rows being evaluated: the sampler's data, or for the predictive calls the caller's
 * own rows [n_x][n_cols] with ctx->n_data = n_x (include/apemost_hip.h).  The engine cannot check a hook against
 * term() and finish(): it takes them on trust.  simplesin2_hooks.hip and bernoulli_hooks.hip in
 * the examples directory have both.
 *
 * The file is compiled as HIP device code for gfx950 (-O3 -ffp-contract=off -std=c++17); it may use
 * the device math library (sin, exp, log, pow, ...).  No host code, no other includes.
 */
#ifndef APEMOST_DEVICE_MODEL_H
#define APEMOST_DEVICE_MODEL_H

typedef struct {
    const double *data;   /* m->data, column-major: column j of row i is data[j * n_data + i] */
    int n_data, n_cols;   /* m->data->size1, m->data->size2 */
    const double *params; /* m->params of the point being evaluated, [n_par] */
    int n_par;
    double sigma, hmin;   /* apemost_hip_config.sigma / .hmin (the applications' -DSIGMA / -DHMIN) */
} apemost_model_ctx;

/* gsl_matrix_get(m->data, i, j) */
#define APEMOST_DATA(ctx, i, j) ((ctx)->data[(unsigned long)(j) * (unsigned long)(ctx)->n_data + (unsigned long)(i)])

/* what data row i adds to the sum */
__device__ double apemost_user_term(const apemost_model_ctx *ctx, int i);
/* m->prob from the sum over all rows; *prior = m->prior (set_prior), beta = get_beta(m) */
__device__ double apemost_user_finish(const apemost_model_ctx *ctx, double sum, double beta, double *prior);

/* optional (#define APEMOST_USER_CURVE 1): the model's value for row i of ctx->data -- what the data loop compares the
 * datum with -- at ctx->params */
__device__ double apemost_user_curve(const apemost_model_ctx *ctx, int i);
/* optional (#define APEMOST_USER_POINTWISE 1): the untempered log-likelihood of row i of ctx->data at ctx->params:
 * log p(row_i | params), beta not applied, prior not included */
__device__ double apemost_user_pointwise(const apemost_model_ctx *ctx, int i);

#endif
