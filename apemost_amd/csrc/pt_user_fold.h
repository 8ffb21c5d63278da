// pt_user_fold.h -- the posterior predictive and pointwise folds (pt_predict.h, pt_pointwise.h) of a user-supplied
// device model (include/apemost_device_model.h), through its optional hooks apemost_user_curve(ctx, i) and
// apemost_user_pointwise(ctx, i).
//
// The kernels are the built-in models' workgroup bodies (predict_fold_body, pointwise_fold_body) with another origin
// of a sample's value, and nothing else: one wave per workgroup, (n_blocks + 1) workgroups per kept chain, pieces of
// 8192 kept steps, parameter rows staged through the LDS tile, four samples side by side, the ordered additions, the
// log-sum-exp recurrences, the histograms and the best-sample scan are the same code.  Where a built-in lane holds x_i
// (and y_i) in registers, a lane here holds its row index i and an apemost_model_ctx:
//   ctx.data            the kept chain's rows being evaluated, column-major [n_cols][n_data] (PredictArgs::x,
//                       PointwiseArgs::x: [n_keep][n_cols][n_data]);
//   ctx.n_data, n_cols  their shape (the predictive fold's n_x is its n_data);
//   ctx.sigma, hmin     the sampler's;
//   ctx.params          the sample's parameter row -- in the LDS tile for all but the first sample ever, hence a generic
//                       pointer; the samples evaluated side by side are copies of the ctx that differ only there.
// A hook is called by lanes with i < n_data only (it dereferences data[i]); what it returns, NaN and inf included, is
// folded as a built-in model's value is.
//
// This header closes the translation unit of the analysis module (apemost_hip.hip user_analysis_build):
//   #define APEMOST_USER_MODEL 1 / #include "pt_kernels.h" / the user's file / #include "pt_user_fold.h"
// so that the preprocessor, not a search of the text, says which hooks the file has: the kernels of an absent hook
// are not part of the module, and the host finds that out when it looks the entry points up by name.
#pragma once

#include "pt_pointwise.h"
#include "pt_pointwise_tail.h"
#include "pt_predict.h"

namespace apemost {

// what the precompiled host code and the analysis module must agree on (pt_kernels.h kAbiFingerprint, which the
// module carries too, covers the engine's own layouts)
constexpr unsigned long long kFoldFingerprint =
    (unsigned long long)sizeof(PredictArgs) ^ ((unsigned long long)sizeof(PointwiseArgs) << 12) ^
    ((unsigned long long)kPredictPiece << 24) ^ ((unsigned long long)kPredictTile << 40) ^
    ((unsigned long long)kPredictSide << 52) ^ ((unsigned long long)sizeof(PointwiseTailArgs) << 4) ^
    0x666f6c6400000000ull;

} // namespace apemost

#ifdef APEMOST_USER_MODEL

extern "C" __device__ __attribute__((used)) const unsigned long long apemost_rtc_fold_fingerprint = apemost::kFoldFingerprint;

namespace apemost {

__device__ __forceinline__ apemost_model_ctx user_fold_ctx(const double *rows, int n_rows, int n_cols, int n_par,
                                                           double sigma, double hmin) {
    apemost_model_ctx c;
    c.data = rows;
    c.n_data = n_rows;
    c.n_cols = n_cols;
    c.params = nullptr;
    c.n_par = n_par;
    c.sigma = sigma;
    c.hmin = hmin;
    return c;
}

} // namespace apemost

#ifdef APEMOST_USER_CURVE
namespace apemost {
struct UserCurveAt {
    apemost_model_ctx ctx;
    int i;
    __device__ __forceinline__ void init(const PredictArgs &a, int k, int i_, size_t, bool) {
        ctx = user_fold_ctx(a.x + (size_t)k * a.n_cols * a.n_x, a.n_x, a.n_cols, a.n_par, a.sigma, a.hmin);
        i = i_;
    }
    __device__ __forceinline__ double at(const double *par) const {
        apemost_model_ctx c = ctx;
        c.params = par;
        return apemost_user_curve(&c, i);
    }
};
} // namespace apemost

extern "C" __global__ void __launch_bounds__(apemost::kPredictWave) apemost_user_predict_fold(apemost::PredictArgs a) {
    apemost::predict_fold_body<apemost::UserCurveAt, false>(a);
}
extern "C" __global__ void __launch_bounds__(apemost::kPredictWave) apemost_user_predict_fold_hist(apemost::PredictArgs a) {
    apemost::predict_fold_body<apemost::UserCurveAt, true>(a);
}
// out[r][i] = apemost_user_curve at params[r] and row i of the rows [n_cols][n_x]; grid ceil(n_x / 64) * n
extern "C" __global__ void __launch_bounds__(apemost::kPredictWave)
apemost_user_predict_curve(const double *params, int n_par, int n_x, int n_cols, const double *rows, double sigma,
                           double hmin, double *out) {
#pragma clang fp contract(off)
    const int n_blocks = (n_x + apemost::kPredictWave - 1) / apemost::kPredictWave;
    const int r = blockIdx.x / n_blocks, i = (blockIdx.x - r * n_blocks) * apemost::kPredictWave + (int)threadIdx.x;
    if (i >= n_x)
        return;
    apemost_model_ctx c = apemost::user_fold_ctx(rows, n_x, n_cols, n_par, sigma, hmin);
    c.params = params + (size_t)r * n_par;
    out[(size_t)r * n_x + i] = apemost_user_curve(&c, i);
}
#endif // APEMOST_USER_CURVE

#ifdef APEMOST_USER_POINTWISE
namespace apemost {
struct UserTermAt {
    apemost_model_ctx ctx;
    int i;
    __device__ __forceinline__ void init(const PointwiseArgs &a, int k, int i_, size_t, bool) {
        ctx = user_fold_ctx(a.x + (size_t)k * a.n_cols * a.n_data, a.n_data, a.n_cols, a.n_par, a.sigma, a.hmin);
        i = i_;
    }
    __device__ __forceinline__ double at(const double *par) const {
        apemost_model_ctx c = ctx;
        c.params = par;
        return apemost_user_pointwise(&c, i);
    }
};
} // namespace apemost

extern "C" __global__ void __launch_bounds__(apemost::kPointwiseWave) apemost_user_pointwise_fold(apemost::PointwiseArgs a) {
    apemost::pointwise_fold_body<apemost::UserTermAt>(a);
}
// the tail of the fold (pt_pointwise_tail.h): the same term, the built-in models' append body
extern "C" __global__ void __launch_bounds__(apemost::kPointwiseWave)
apemost_user_pointwise_tail_append(apemost::PointwiseArgs a, apemost::PointwiseTailArgs t) {
    apemost::pointwise_tail_append_body<apemost::UserTermAt>(a, t);
}
// out[r][i] = apemost_user_pointwise at params[r] and row i of the rows [n_cols][n_data]; grid ceil(n_data / 64) * n
extern "C" __global__ void __launch_bounds__(apemost::kPointwiseWave)
apemost_user_pointwise_loglike(const double *params, int n_par, int n_data, int n_cols, const double *rows,
                               double sigma, double hmin, double *out) {
#pragma clang fp contract(off)
    const int n_blocks = (n_data + apemost::kPointwiseWave - 1) / apemost::kPointwiseWave;
    const int r = blockIdx.x / n_blocks, i = (blockIdx.x - r * n_blocks) * apemost::kPointwiseWave + (int)threadIdx.x;
    if (i >= n_data)
        return;
    apemost_model_ctx c = apemost::user_fold_ctx(rows, n_data, n_cols, n_par, sigma, hmin);
    c.params = params + (size_t)r * n_par;
    out[(size_t)r * n_data + i] = apemost_user_pointwise(&c, i);
}
#endif // APEMOST_USER_POINTWISE

#endif // APEMOST_USER_MODEL
