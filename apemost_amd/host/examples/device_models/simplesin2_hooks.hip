/* simplesin2.hip with the two optional hooks of include/apemost_device_model.h, so that the on-device posterior
 * predictive (apemost_hip_predict_*) and pointwise log-likelihood (apemost_hip_pointwise_*: WAIC, LOO, DIC) work for
 * it.  term() and finish() are simplesin2.hip's, unchanged (apps/simplesin2.c:12-34):
 *   term(i)      = (param0 * sin(2 pi (param1 * x_i + 0.3312)) - y_i)^2
 *   finish()     = get_beta(m) * square_sum / (-2 * SIGMA * SIGMA)
 *   curve(i)     = param0 * sin(2 pi (param1 * x_i + 0.3312)): what the data loop compares y_i with
 *   pointwise(i) = ((curve(i) - y_i)^2) * (1 / ((-2 SIGMA) SIGMA)): the datum's share of finish() at beta = 1, in the
 *                  operation order of the built-in sine models' term (apemost_amd/csrc/pt_pointwise.h). */
#include "apemost_device_model.h"

#define APEMOST_USER_CURVE 1
#define APEMOST_USER_POINTWISE 1

__device__ double apemost_user_curve(const apemost_model_ctx *ctx, int i) {
    const double x = APEMOST_DATA(ctx, i, 0);
    return ctx->params[0] * sin(2.0 * 3.14159265358979323846 * (ctx->params[1] * x + 0.3312));
}

__device__ double apemost_user_term(const apemost_model_ctx *ctx, int i) {
    const double x = APEMOST_DATA(ctx, i, 0);
    const double y = ctx->params[0] * sin(2.0 * 3.14159265358979323846 * (ctx->params[1] * x + 0.3312)) - APEMOST_DATA(ctx, i, 1);
    return y * y;
}

__device__ double apemost_user_finish(const apemost_model_ctx *ctx, double sum, double beta, double *prior) {
    (void)prior; /* set_prior is never called: m->prior stays what it was */
    return beta * sum / (-2 * ctx->sigma * ctx->sigma);
}

__device__ double apemost_user_pointwise(const apemost_model_ctx *ctx, int i) {
    const double c = 1.0 / ((-2.0 * ctx->sigma) * ctx->sigma);
    const double r = apemost_user_curve(ctx, i) - APEMOST_DATA(ctx, i, 1);
    const double q = r * r;
    return q * c;
}
