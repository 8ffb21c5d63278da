/* A device model for tests/test_gpu_pointwise_tail.py: its pointwise term is one IEEE multiplication,
 *   pointwise(i) = param0 * y_i,
 * so that a test can give a series any term it likes -- zeros of both signs, both infinities, NaN, exact duplicates --
 * and state it bit for bit in numpy.  term() and finish() make it a sampler like any other; the test never steps it. */
#include "apemost_device_model.h"

#define APEMOST_USER_POINTWISE 1

__device__ double apemost_user_term(const apemost_model_ctx *ctx, int i) {
    const double r = ctx->params[0] - APEMOST_DATA(ctx, i, 1);
    return r * r;
}

__device__ double apemost_user_finish(const apemost_model_ctx *ctx, double sum, double beta, double *prior) {
    (void)prior;
    return beta * sum / (-2 * ctx->sigma * ctx->sigma);
}

__device__ double apemost_user_pointwise(const apemost_model_ctx *ctx, int i) { return ctx->params[0] * APEMOST_DATA(ctx, i, 1); }
