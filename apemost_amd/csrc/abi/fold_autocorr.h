// abi/fold_autocorr.h -- on-device autocorrelation (pt_autocorr.h; state: AutocorrFold, protocol: abi/fold_common.h)
#pragma once

extern "C" int apemost_hip_autocorr_begin(apemost_hip_sampler *s, const apemost_hip_autocorr_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr_begin: config is NULL");
    const int np = s->cfg.n_par;
    FOLD_TRY(fold_check_chains(s, "autocorr", cfg->n_keep, cfg->chains));
    if (cfg->max_lag < 1 || cfg->max_lag > kAutocorrMaxLag)
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr_begin: max_lag %d outside [1,%d]", cfg->max_lag, kAutocorrMaxLag);
    std::vector<int> cols;
    if (!cfg->cols) { // the parameters and prob - prior
        for (int p = 0; p < np; p++)
            cols.push_back(p);
        cols.push_back(np + 1);
    } else {
        if (cfg->n_cols < 1 || cfg->n_cols > np + 2)
            return fail(APEMOST_HIP_ERR_INVALID, "autocorr_begin: n_cols %d outside [1,%d]", cfg->n_cols, np + 2);
        for (int c = 0; c < cfg->n_cols; c++) {
            if (cfg->cols[c] < 0 || cfg->cols[c] > np + 1 || (c > 0 && cfg->cols[c] <= cfg->cols[c - 1]))
                return fail(APEMOST_HIP_ERR_INVALID,
                            "autocorr_begin: cols[%d] = %d: column indices in [0,%d], strictly increasing", c, cfg->cols[c],
                            np + 1);
            cols.push_back(cfg->cols[c]);
        }
    }
    const u64 n_series = (u64)cfg->n_keep * cols.size();
    const u64 L = (u64)cfg->max_lag, H = L - 1;
    if (n_series > 65535 || n_series * L > ((u64)1 << 24))
        return fail(APEMOST_HIP_ERR_INVALID,
                    "autocorr_begin: %d chains x %zu columns x %d lags: more than 65535 series or 2^24 lag sums",
                    cfg->n_keep, cols.size(), cfg->max_lag);
    FOLD_TRY(fold_reset(s, s->ac));
    AutocorrFold &f = s->ac;
    // the staged series: about 1 Mi values over all of them, at most 2^16 kept steps per launch
    const u64 chunk = fold_chunk((u64)1 << 20, n_series, 16);
    f.n_keep = cfg->n_keep;
    f.n_cols = (int)cols.size();
    f.max_lag = cfg->max_lag;
    f.chunk = chunk;
    f.n = 0;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_chains, cfg->n_keep, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_cols, cols.size(), false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_buf, n_series * (H + chunk), false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_origin, n_series, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_sum, n_series, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_lag, n_series * L, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_head, n_series * (H > 0 ? H : 1), true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_tail, n_series * (H > 0 ? H : 1), true));
    HIP_TRY(hipMemcpyAsync(f.d_chains, cfg->chains, cfg->n_keep * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_cols, cols.data(), cols.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (`cols` and the caller's arrays are read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_autocorr_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                               uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    AutocorrFold &f = s->ac;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("autocorr", f.open, d_samples, n_steps, skip, thin, &kept));
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const unsigned n_series = (unsigned)(f.n_keep * f.n_cols);
    const unsigned H = (unsigned)f.max_lag - 1u;
    for (u64 k0 = 0; k0 < kept; k0 += f.chunk) {
        AutocorrArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = s->cfg.n_par;
        a.n_keep = f.n_keep;
        a.n_cols = f.n_cols;
        a.chains = f.d_chains;
        a.cols = f.d_cols;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < f.chunk ? kept - k0 : f.chunk);
        a.n0 = f.n;
        a.max_lag = f.max_lag;
        a.n_groups = (f.max_lag + kAutocorrGroup - 1) / kAutocorrGroup;
        a.stride = H + f.chunk;
        a.buf = f.d_buf;
        a.origin = f.d_origin;
        a.sum = f.d_sum;
        a.lag = f.d_lag;
        a.head = f.d_head;
        a.tail = f.d_tail;
        hipLaunchKernelGGL(autocorr_gather_kernel, dim3((H + a.n + kAutocorrThreads - 1) / kAutocorrThreads, n_series),
                           dim3(kAutocorrThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(autocorr_fold_kernel, dim3((unsigned)a.n_groups + 1u, n_series), dim3(kAutocorrWave), 0,
                           s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        if (H > 0) {
            hipLaunchKernelGGL(autocorr_carry_kernel, dim3((H + kAutocorrThreads - 1) / kAutocorrThreads, n_series),
                               dim3(kAutocorrThreads), 0, s->copy_stream, a);
            HIP_TRY(hipGetLastError());
        }
        f.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int autocorr_xfer(apemost_hip_sampler *s, const apemost_hip_autocorr_view *v, bool up) {
    CHECK_S(s);
    AutocorrFold &f = s->ac;
    FOLD_TRY(fold_xfer_check("autocorr", f.open, v, up));
    const size_t n_series = (size_t)f.n_keep * f.n_cols, L = (size_t)f.max_lag, H = L - 1;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    FOLD_TRY(copy(f.d_origin, v->origin, n_series * sizeof(double)));
    FOLD_TRY(copy(f.d_sum, v->sum, n_series * sizeof(double)));
    FOLD_TRY(copy(f.d_lag, v->lag, n_series * L * sizeof(double)));
    FOLD_TRY(copy(f.d_head, v->head, n_series * H * sizeof(double)));
    FOLD_TRY(copy(f.d_tail, v->tail, n_series * H * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_autocorr_get(apemost_hip_sampler *s, const apemost_hip_autocorr_view *v) {
    return autocorr_xfer(s, v, false);
}

extern "C" int apemost_hip_autocorr_set(apemost_hip_sampler *s, const apemost_hip_autocorr_view *v) {
    return autocorr_xfer(s, v, true);
}

extern "C" int apemost_hip_autocorr_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    return fold_reset(s, s->ac);
}
