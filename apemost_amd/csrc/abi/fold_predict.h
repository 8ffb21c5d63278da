// abi/fold_predict.h -- on-device posterior predictive (pt_predict.h; state: PredictFold, protocol: abi/fold_common.h)
#pragma once

// a built-in model, or a user-supplied one with the curve hook (its analysis module is built here on first use)
#define PREDICT_HAS_CURVE(s, what)                                                                                \
    do {                                                                                                        \
        if ((s)->cfg.model == APEMOST_MODEL_USER) {                                                             \
            const int rc_hooks = user_analysis(s);                                                              \
            if (rc_hooks != APEMOST_HIP_OK)                                                                     \
                return rc_hooks;                                                                                \
            if (!(s)->ua.has_curve)                                                                             \
                return fail(APEMOST_HIP_ERR_UNSUPPORTED,                                                        \
                            what ": this user-supplied device model has no curve: it does not define the hook " \
                                 "apemost_user_curve (APEMOST_USER_CURVE, include/apemost_device_model.h)");    \
        }                                                                                                       \
    } while (0)

// host rows [n][n_cols], row-major like m->data -> a ctx's data, [n_cols][n]
static std::vector<double> rows_by_columns(const double *rows, int n, int n_cols) {
    std::vector<double> out((size_t)n * n_cols);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n_cols; j++)
            out[(size_t)j * n + i] = rows[(size_t)i * n_cols + j];
    return out;
}

static hipError_t predict_launch_fold(apemost_hip_sampler *s, const PredictArgs &a) {
    const dim3 grid((unsigned)(a.n_blocks + 1) * (unsigned)a.n_keep), block(kPredictWave);
    const size_t lds = predict_lds_bytes(a.nbins, a.points);
    if (s->cfg.model == APEMOST_MODEL_USER) {
        void *params[] = {const_cast<PredictArgs *>(&a)};
        return user_launch(a.nbins > 0 ? s->ua.predict_fold_hist : s->ua.predict_fold, grid.x, block.x,
                           a.nbins > 0 ? lds : 0, s->copy_stream, params);
    }
    with_builtin_model(s->cfg.model, [&](auto m) {
        if (a.nbins > 0)
            hipLaunchKernelGGL((predict_fold_kernel<decltype(m)::value, true>), grid, block, lds, s->copy_stream, a);
        else
            hipLaunchKernelGGL((predict_fold_kernel<decltype(m)::value, false>), grid, block, 0, s->copy_stream, a);
    });
    return hipGetLastError();
}

extern "C" int apemost_hip_predict_begin(apemost_hip_sampler *s, const apemost_hip_predict_config *cfg) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_begin");
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: config is NULL");
    const int np = s->cfg.n_par;
    FOLD_TRY(fold_check_chains(s, "predict", cfg->n_keep, cfg->chains));
    // at the data's abscissae: the longest data among the kept chains' ladders (a batch's ladders may differ in
    // length: the arrays stay rectangular and every kept chain folds its own len[k] <= n_x series)
    std::vector<int> len;
    bool ragged = false;
    const int n_x = cfg->x ? cfg->n_x : kept_lengths(s, cfg->n_keep, cfg->chains, len, &ragged);
    if (n_x < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: n_x %d < 1", n_x);
    // a user model's abscissae are whole rows: [n_x][n_cols] from the caller, or the sampler's data
    const bool user = s->cfg.model == APEMOST_MODEL_USER;
    const int nc = user ? s->cfg.n_cols : 1;
    if (cfg->x)
        for (size_t i = 0; i < (size_t)n_x * nc; i++)
            if (!std::isfinite(cfg->x[i]))
                return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: x[%zu] is not finite", i);
    if (cfg->nbins < 0 || cfg->nbins > kPredictMaxBins)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: nbins %d outside [0,%d]", cfg->nbins, kPredictMaxBins);
    if (cfg->nbins > 0 && !(std::isfinite(cfg->lo) && std::isfinite(cfg->hi) && cfg->lo < cfg->hi))
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: the histogram range [%g, %g] is not finite with lo < hi",
                    cfg->lo, cfg->hi);
    const u64 n_series = (u64)cfg->n_keep * (u64)n_x;
    if (n_series > ((u64)1 << 20) || n_series * (u64)cfg->nbins > ((u64)1 << 26))
        return fail(APEMOST_HIP_ERR_INVALID,
                    "predict_begin: %d chains x %d abscissae x %d bins: more than 2^20 series or 2^26 counts", cfg->n_keep,
                    n_x, cfg->nbins);
    if (np > kPredictTile)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: %d parameters, more than %d", np, kPredictTile);
    FOLD_TRY(fold_reset(s, s->pr));
    PredictFold &f = s->pr;
    f.n_keep = cfg->n_keep;
    f.n_x = n_x;
    f.n_cols = nc;
    f.nbins = cfg->nbins;
    f.points = predict_points(cfg->nbins);
    f.lo = cfg->lo;
    f.hi = cfg->hi;
    f.n = 0;
    const size_t ns = (size_t)n_series, nk = (size_t)cfg->n_keep;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_chains, nk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_x, ns * nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_origin, ns, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_sum, ns, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_sq, ns, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_vmin, ns, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_vmax, ns, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_hist, ns * (size_t)cfg->nbins, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_best_prob, nk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_best_params, nk * np, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_best_n, nk, true));
    if (ragged) {
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_len, nk, false));
        HIP_TRY(hipMemcpyAsync(f.d_len, len.data(), nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    }
    std::vector<double> pinf(ns, INFINITY), ninf(ns, -INFINITY);
    HIP_TRY(hipMemcpyAsync(f.d_vmin, pinf.data(), ns * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_vmax, ninf.data(), ns * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_best_prob, ninf.data(), nk * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_chains, cfg->chains, nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    const std::vector<double> by_cols = cfg->x && user ? rows_by_columns(cfg->x, n_x, nc) : std::vector<double>();
    const double *host_x = by_cols.empty() ? cfg->x : by_cols.data();
    for (int k = 0; k < cfg->n_keep; k++) {
        double *dst = f.d_x + (size_t)k * nc * n_x;
        if (cfg->x) {
            HIP_TRY(hipMemcpyAsync(dst, host_x, (size_t)nc * n_x * sizeof(double), hipMemcpyHostToDevice, s->stream));
        } else { // column 0 of the kept chain's own ladder (the data is stored by columns, ladder after ladder);
                 // a user model: all of its columns
            // (a batch runs the built-in models only: nc = 1, and len[k] <= n_x values of the ladder's own column)
            const double *col0 = ladder_data(s, s->batch ? cfg->chains[k] / s->per_ladder : 0);
            HIP_TRY(hipMemcpyAsync(dst, col0, (size_t)nc * len[k] * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's arrays are read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_predict_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                              uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_accumulate");
    PredictFold &f = s->pr;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("predict", f.open, d_samples, n_steps, skip, thin, &kept));
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    for (u64 k0 = 0; k0 < kept; k0 += kPredictPiece) {
        PredictArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = s->cfg.n_par;
        a.n_keep = f.n_keep;
        a.chains = f.d_chains;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < (u64)kPredictPiece ? kept - k0 : (u64)kPredictPiece);
        a.n0 = f.n;
        a.n_x = f.n_x;
        a.x = f.d_x;
        a.n_cols = f.n_cols;
        a.sigma = s->sh.consts.sigma;
        a.hmin = s->sh.consts.hmin;
        a.nbins = f.nbins;
        a.points = f.points;
        a.n_blocks = (f.n_x + f.points - 1) / f.points;
        a.lo = f.lo;
        a.hi = f.hi;
        a.origin = f.d_origin;
        a.sum = f.d_sum;
        a.sq = f.d_sq;
        a.vmin = f.d_vmin;
        a.vmax = f.d_vmax;
        a.hist = f.d_hist;
        a.best_prob = f.d_best_prob;
        a.best_params = f.d_best_params;
        a.best_n = f.d_best_n;
        a.len = f.d_len;
        HIP_TRY(predict_launch_fold(s, a));
        f.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int predict_xfer(apemost_hip_sampler *s, const apemost_hip_predict_view *v, bool up) {
    PredictFold &f = s->pr;
    FOLD_TRY(fold_xfer_check("predict", f.open, v, up));
    const size_t nk = (size_t)f.n_keep, ns = nk * f.n_x, np = (size_t)s->cfg.n_par;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    FOLD_TRY(copy(f.d_origin, v->origin, ns * sizeof(double)));
    FOLD_TRY(copy(f.d_sum, v->sum, ns * sizeof(double)));
    FOLD_TRY(copy(f.d_sq, v->sq, ns * sizeof(double)));
    FOLD_TRY(copy(f.d_vmin, v->vmin, ns * sizeof(double)));
    FOLD_TRY(copy(f.d_vmax, v->vmax, ns * sizeof(double)));
    FOLD_TRY(copy(f.d_hist, v->hist, ns * f.nbins * sizeof(u64)));
    FOLD_TRY(copy(f.d_best_prob, v->best_prob, nk * sizeof(double)));
    FOLD_TRY(copy(f.d_best_params, v->best_params, nk * np * sizeof(double)));
    FOLD_TRY(copy(f.d_best_n, v->best_n, nk * sizeof(u64)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_predict_get(apemost_hip_sampler *s, const apemost_hip_predict_view *v) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_get");
    return predict_xfer(s, v, false);
}

extern "C" int apemost_hip_predict_set(apemost_hip_sampler *s, const apemost_hip_predict_view *v) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_set");
    return predict_xfer(s, v, true);
}

extern "C" int apemost_hip_predict_lengths(apemost_hip_sampler *s, int32_t *len) {
    CHECK_S(s);
    const PredictFold &f = s->pr;
    if (!f.open || !len)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_lengths: %s", f.open ? "len is NULL" : "no predict_begin");
    for (int k = 0; k < f.n_keep; k++)
        len[k] = f.n_x;
    if (f.d_len) {
        HIP_TRY(hipMemcpyAsync(len, f.d_len, (size_t)f.n_keep * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_predict_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_end");
    return fold_reset(s, s->pr);
}

// the curve of n parameter rows at n_x abscissae, by the fold's own curve function: no fold need be open
extern "C" int apemost_hip_predict_curve(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x,
                                         const double *x, double *out) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_curve");
    if (!x)
        n_x = ladder_len(s, 0); // (a batch: ladder 0's data, which d.data starts with)
    if (n < 1 || !params || !out || n_x < 1 || (u64)n * (u64)n_x > ((u64)1 << 26))
        return fail(APEMOST_HIP_ERR_INVALID, "predict_curve: %d rows x %d abscissae, or a NULL array", n, n_x);
    const int np = s->cfg.n_par;
    const bool user = s->cfg.model == APEMOST_MODEL_USER;
    int nc = user ? s->cfg.n_cols : 1; // a user model's abscissae are whole rows [n_x][n_cols], finite
    std::vector<double> by_cols;
    if (user && x) {
        for (size_t i = 0; i < (size_t)n_x * nc; i++)
            if (!std::isfinite(x[i]))
                return fail(APEMOST_HIP_ERR_INVALID, "predict_curve: x[%zu] is not finite", i);
        by_cols = rows_by_columns(x, n_x, nc);
        x = by_cols.data();
    }
    FoldScratch scratch;
    double *d_par = nullptr, *d_x = nullptr, *d_out = nullptr;
    const int rc = [&]() -> int { // (whatever fails, the stream is waited for before the scratch goes)
        FOLD_TRY(fold_alloc(s, scratch, &d_par, (size_t)n * np, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_x, (size_t)nc * n_x, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_out, (size_t)n * n_x, false));
        HIP_TRY(hipMemcpyAsync(d_par, params, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(x ? hipMemcpyAsync(d_x, x, (size_t)nc * n_x * sizeof(double), hipMemcpyHostToDevice, s->stream)
                  : hipMemcpyAsync(d_x, s->d.data, (size_t)nc * n_x * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        const unsigned grid = (unsigned)((n_x + kPredictWave - 1) / kPredictWave) * (unsigned)n;
        if (user) {
            int np_ = np;
            double sigma = s->sh.consts.sigma, hmin = s->sh.consts.hmin;
            void *params_[] = {&d_par, &np_, &n_x, &nc, &d_x, &sigma, &hmin, &d_out};
            HIP_TRY(user_launch(s->ua.predict_curve, grid, kPredictWave, 0, s->stream, params_));
        } else {
            with_builtin_model(s->cfg.model, [&](auto m) {
                hipLaunchKernelGGL(predict_curve_kernel<decltype(m)::value>, dim3(grid), dim3(kPredictWave), 0, s->stream,
                                   d_par, np, n_x, d_x, d_out);
            });
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * n_x * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        return APEMOST_HIP_OK;
    }();
    const hipError_t sync = hipStreamSynchronize(s->stream);
    FOLD_TRY(rc);
    HIP_TRY(sync);
    return APEMOST_HIP_OK;
}
