/* bernoulli_example.hip with the two optional hooks of include/apemost_device_model.h, so that the on-device posterior
 * predictive (apemost_hip_predict_*) and pointwise log-likelihood (apemost_hip_pointwise_*: WAIC, LOO, DIC) work for
 * it.  term() and finish() are bernoulli_example.hip's, unchanged (apps/bernoulli_example.c:10-49): data column 0 is
 * the 0/1 outcome, columns 1.. are the regressors, parameter 0 is the intercept.
 *   curve(i)     = p_i = logistic(eta_i), eta_i = param_0 + sum_j x_ij param_j: the predicted probability of row i
 *   pointwise(i) = term(i) = log(p_i) or log(1 - p_i): finish() is prior + beta * sum, so a row's term is its
 *                  log-likelihood. */
#include "apemost_device_model.h"

#define APEMOST_USER_CURVE 1
#define APEMOST_USER_POINTWISE 1

__device__ double apemost_user_curve(const apemost_model_ctx *ctx, int i) {
    double eta = ctx->params[0], p;
    for (int j = 1; j < ctx->n_par; j++)
        eta += APEMOST_DATA(ctx, i, j) * ctx->params[j];
    if (eta > 0)
        p = 1 / (1 + exp(-eta));
    else
        p = exp(eta) / (1 + exp(eta));
    return p;
}

__device__ double apemost_user_term(const apemost_model_ctx *ctx, int i) {
    double eta = ctx->params[0], p;
    for (int j = 1; j < ctx->n_par; j++)
        eta += APEMOST_DATA(ctx, i, j) * ctx->params[j];
    if (eta > 0)
        p = 1 / (1 + exp(-eta));
    else
        p = exp(eta) / (1 + exp(eta));
    return APEMOST_DATA(ctx, i, 0) == 0 ? log(1 - p) : log(p);
}

__device__ double apemost_user_finish(const apemost_model_ctx *ctx, double sum, double beta, double *prior) {
    double pr = 0;
    for (int j = 1; j < ctx->n_cols; j++) {
        const double t = ctx->params[j] / 2;
        pr += -(t * t) / 2;
    }
    *prior = pr;
    return pr + beta * sum;
}

__device__ double apemost_user_pointwise(const apemost_model_ctx *ctx, int i) { return apemost_user_term(ctx, i); }
