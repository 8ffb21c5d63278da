// abi/fold_mbar.h -- on-device MBAR (pt_mbar.h; state: MbarFold, protocol: abi/fold_common.h).  Beside the protocol's
// begin, accumulate, get, set and end it has three entry points that compute on the store: iterate, evaluate and
// log_weights.  They run on copy_stream behind every accumulate and return when their results are on the host.
#pragma once

constexpr u64 kMbarMaxValues = (u64)1 << 28; // capacity x n_chains

extern "C" int apemost_hip_mbar_begin(apemost_hip_sampler *s, const apemost_hip_mbar_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_begin: config is NULL");
    if (s->cfg.n_chains_global > s->cfg.n_chains)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "mbar_begin: a shard of %d chains of a ladder of %lld: the solve needs "
                    "every chain of the ladder on one device", s->cfg.n_chains, (long long)s->cfg.n_chains_global);
    if (!cfg->betas)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_begin: betas are needed");
    const size_t nc = (size_t)s->cfg.n_chains;
    const int L = s->batch ? s->n_ladders : 1, K = (int)(nc / L);
    if (L > 65535)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_begin: %d ladders are more than 65535", L);
    for (int b = 0; b < L; b++)
        for (int c = 0; c < K; c++) {
            const double beta = cfg->betas[(size_t)b * K + c];
            if (!std::isfinite(beta) || !(beta > 0) || (c > 0 && !(beta < cfg->betas[(size_t)b * K + c - 1])))
                return fail(APEMOST_HIP_ERR_INVALID, "mbar_begin: ladder %d: beta of chain %d is %g; the betas must be "
                            "finite, positive and strictly decreasing", b, c, beta);
        }
    if (cfg->capacity < 1 || cfg->capacity > kMbarMaxValues / nc)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_begin: capacity %llu outside [1, %llu]: capacity x %zu chains is at "
                    "most 2^28 values", (unsigned long long)cfg->capacity, (unsigned long long)(kMbarMaxValues / nc), nc);
    FOLD_TRY(fold_reset(s, s->mb));
    fold_free(s->rw); // (an attached reweight fold goes with the store whose capacity it shared)
    MbarFold &f = s->mb;
    f.K = K;
    f.L = L;
    f.capacity = cfg->capacity;
    f.tiles_max = (cfg->capacity * K + kMbarTile - 1) / kMbarTile;
    f.n = 0;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_betas, nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_ell, nc * cfg->capacity, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_lnD, nc * cfg->capacity, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_g, 2 * nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_c, nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_beta_t, nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_part, (size_t)kMbarWords * nc * f.tiles_max, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_out, (size_t)(2 + kMbarWords) * nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_bad, (size_t)L, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_mkey, nc, false));
    HIP_TRY(hipMemcpyAsync(f.d_betas, cfg->betas, nc * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's array is read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_mbar_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                           uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    MbarFold &f = s->mb;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("mbar", f.open, d_samples, n_steps, skip, thin, &kept));
    if (kept > f.capacity - f.n)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_accumulate: %llu samples stored, %llu more are beyond capacity = %llu",
                    (unsigned long long)f.n, (unsigned long long)kept, (unsigned long long)f.capacity);
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const int nc = s->cfg.n_chains;
    const u64 chunk = (u64)1 << 18; // (the grid's y: kept steps / 8)
    for (u64 k0 = 0; k0 < kept; k0 += chunk) {
        MbarGatherArgs a;
        a.rows = d_samples;
        a.n_chains = nc;
        a.n_par = s->cfg.n_par;
        a.K = f.K;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < chunk ? kept - k0 : chunk);
        a.betas = f.d_betas;
        a.ell = f.d_ell + (size_t)f.n * nc;
        a.n_bad = f.d_bad;
        hipLaunchKernelGGL(mbar_gather_kernel,
                           dim3((unsigned)((nc + kMbarGatherThreads - 1) / kMbarGatherThreads), (a.n + 7u) / 8u),
                           dim3(kMbarGatherThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        f.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int mbar_xfer(apemost_hip_sampler *s, const apemost_hip_mbar_view *v, bool up) {
    CHECK_S(s);
    MbarFold &f = s->mb;
    FOLD_TRY(fold_xfer_check("mbar", f.open, v, up));
    if (up && v->n && *v->n > f.capacity)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_set: %llu samples are beyond capacity = %llu",
                    (unsigned long long)*v->n, (unsigned long long)f.capacity);
    const u64 n = up && v->n ? *v->n : f.n;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    FOLD_TRY(copy(f.d_bad, v->n_bad, (size_t)f.L * sizeof(u64)));
    FOLD_TRY(copy(f.d_ell, v->ell, (size_t)n * s->cfg.n_chains * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_mbar_get(apemost_hip_sampler *s, const apemost_hip_mbar_view *v) { return mbar_xfer(s, v, false); }

extern "C" int apemost_hip_mbar_set(apemost_hip_sampler *s, const apemost_hip_mbar_view *v) { return mbar_xfer(s, v, true); }

extern "C" int apemost_hip_mbar_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    FOLD_TRY(fold_reset(s, s->mb));
    fold_free(s->rw); // (its capacity was this fold's)
    return APEMOST_HIP_OK;
}

// ---- computing on the store ----
// The head of iterate, evaluate and log_weights: the range, the count of non-finite values (read behind every
// accumulate), and the arguments every kernel of the range shares.  copy_stream is ordered and idle on return.
static int mbar_range(apemost_hip_sampler *s, const char *what, u64 t0, u64 t_count, MbarArgs *a) {
    MbarFold &f = s->mb;
    if (!f.open)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_%s: no mbar_begin", what);
    if (t_count < 1 || t0 > f.n || t_count > f.n - t0)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_%s: kept steps [%llu, %llu + %llu) are empty or go past the %llu stored",
                    what, (unsigned long long)t0, (unsigned long long)t0, (unsigned long long)t_count,
                    (unsigned long long)f.n);
    FOLD_TRY(fold_order_behind_stream(s));
    std::vector<u64> bad(f.L);
    HIP_TRY(hipMemcpyAsync(bad.data(), f.d_bad, (size_t)f.L * sizeof(u64), hipMemcpyDeviceToHost, s->copy_stream));
    FOLD_TRY(fold_xfer_wait(s));
    for (int b = 0; b < f.L; b++)
        if (bad[b])
            return fail(APEMOST_HIP_ERR_INVALID, "mbar_%s: ladder %d stores %llu values that are not finite", what, b,
                        (unsigned long long)bad[b]);
    a->ell = f.d_ell;
    a->lnD = f.d_lnD;
    a->n_chains = s->cfg.n_chains;
    a->K = f.K;
    a->t0 = t0;
    a->N = (unsigned int)(t_count * f.K);
    a->tiles = (a->N + kMbarTile - 1) / kMbarTile;
    a->betas = f.d_betas;
    a->c = f.d_c;
    a->beta_t = f.d_betas;
    a->t_stride = f.K;
    a->n_t = f.K;
    a->mkey = f.d_mkey;
    a->part = f.d_part;
    a->part_stride = (size_t)s->cfg.n_chains * f.tiles_max;
    return APEMOST_HIP_OK;
}

// g [n_chains] of the host into d_g, c = lnT - g into d_c
static int mbar_upload_g(apemost_hip_sampler *s, const double *g, double lnT, double *d_g, std::vector<double> &c) {
    const size_t nc = (size_t)s->cfg.n_chains;
    c.resize(nc);
    for (size_t k = 0; k < nc; k++) {
        if (!std::isfinite(g[k]))
            return fail(APEMOST_HIP_ERR_INVALID, "mbar: g[%zu] = %g is not finite", k, g[k]);
        c[k] = lnT - g[k];
    }
    HIP_TRY(hipMemcpyAsync(d_g, g, nc * sizeof(double), hipMemcpyHostToDevice, s->copy_stream));
    HIP_TRY(hipMemcpyAsync(s->mb.d_c, c.data(), nc * sizeof(double), hipMemcpyHostToDevice, s->copy_stream));
    return APEMOST_HIP_OK;
}

static int mbar_launch_row(apemost_hip_sampler *s, const MbarArgs &a) {
    hipLaunchKernelGGL(mbar_row_kernel, dim3((a.N + kMbarThreads - 1) / kMbarThreads, (unsigned)s->mb.L),
                       dim3(kMbarThreads), 0, s->copy_stream, a);
    HIP_TRY(hipGetLastError());
    return APEMOST_HIP_OK;
}

// the maxima and the tile partials of a's targets, then mbar_finish_kernel
static int mbar_launch_cols(apemost_hip_sampler *s, const MbarArgs &a, bool full, double lnT, double *g, double *c,
                            double *out) {
    const MbarFold &f = s->mb;
    hipStream_t st = s->copy_stream;
    const dim3 grid(a.tiles, (unsigned)((a.n_t + kMbarGroup - 1) / kMbarGroup), (unsigned)f.L);
    HIP_TRY(hipMemsetAsync(a.mkey, 0, (size_t)f.L * a.n_t * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(mbar_max_kernel, grid, dim3(kMbarThreads), 0, st, a);
    if (full)
        hipLaunchKernelGGL(mbar_col_kernel<true>, grid, dim3(kMbarThreads), 0, st, a);
    else
        hipLaunchKernelGGL(mbar_col_kernel<false>, grid, dim3(kMbarThreads), 0, st, a);
    hipLaunchKernelGGL(mbar_finish_kernel, dim3((unsigned)(((size_t)f.L * a.n_t + 63) / 64)), dim3(64), 0, st, a, f.L,
                       full ? 1 : 0, lnT, g, c, out);
    HIP_TRY(hipGetLastError());
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_mbar_iterate(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, uint32_t n_iter,
                                        double *g_inout, double *g_prev_out) {
    CHECK_S(s);
    if (!g_inout || n_iter < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_iterate: g is NULL or n_iter is 0");
    MbarArgs a;
    FOLD_TRY(mbar_range(s, "iterate", t0, t_count, &a));
    MbarFold &f = s->mb;
    const size_t nc = (size_t)s->cfg.n_chains;
    const double lnT = std::log((double)t_count);
    std::vector<double> c;
    FOLD_TRY(mbar_upload_g(s, g_inout, lnT, f.d_g, c));
    int cur = 0;
    for (uint32_t it = 0; it < n_iter; it++, cur ^= 1) {
        FOLD_TRY(mbar_launch_row(s, a));
        FOLD_TRY(mbar_launch_cols(s, a, false, lnT, f.d_g + (size_t)(cur ^ 1) * nc, f.d_c, nullptr));
    }
    // (cur: the last update's result; cur ^ 1: what it started from)
    HIP_TRY(hipMemcpyAsync(g_inout, f.d_g + (size_t)cur * nc, nc * sizeof(double), hipMemcpyDeviceToHost, s->copy_stream));
    if (g_prev_out)
        HIP_TRY(hipMemcpyAsync(g_prev_out, f.d_g + (size_t)(cur ^ 1) * nc, nc * sizeof(double), hipMemcpyDeviceToHost,
                               s->copy_stream));
    return fold_xfer_wait(s);
}

extern "C" int apemost_hip_mbar_evaluate(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g,
                                         const double *betas_t, int32_t n_t, const apemost_hip_mbar_sums *out) {
    CHECK_S(s);
    if (!g || !betas_t || n_t < 1 || !out)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_evaluate: g, the targets or the sums are missing");
    for (int t = 0; t < n_t; t++)
        if (!std::isfinite(betas_t[t]) || !(betas_t[t] >= 0))
            return fail(APEMOST_HIP_ERR_INVALID, "mbar_evaluate: target %d is %g; a target is finite and >= 0", t, betas_t[t]);
    MbarArgs a;
    FOLD_TRY(mbar_range(s, "evaluate", t0, t_count, &a));
    MbarFold &f = s->mb;
    hipStream_t st = s->copy_stream;
    std::vector<double> c;
    FOLD_TRY(mbar_upload_g(s, g, std::log((double)t_count), f.d_g, c));
    FOLD_TRY(mbar_launch_row(s, a));
    a.beta_t = f.d_beta_t;
    a.t_stride = 0; // (every ladder takes the same targets)
    double *const words[2 + kMbarWords] = {out->m, out->S0, out->S1, out->S2, out->SS, out->G};
    for (int first = 0; first < n_t; first += f.K) { // pieces of at most K targets: what the scratch has room for
        const int n_piece = n_t - first < f.K ? n_t - first : f.K;
        a.n_t = n_piece;
        HIP_TRY(hipMemcpyAsync(f.d_beta_t, betas_t + first, n_piece * sizeof(double), hipMemcpyHostToDevice, st));
        FOLD_TRY(mbar_launch_cols(s, a, true, 0.0, nullptr, nullptr, f.d_out));
        for (int w = 0; w < 2 + kMbarWords; w++)
            if (words[w])
                HIP_TRY(hipMemcpy2DAsync(words[w] + first, (size_t)n_t * sizeof(double),
                                         f.d_out + (size_t)w * f.L * n_piece, (size_t)n_piece * sizeof(double),
                                         (size_t)n_piece * sizeof(double), (size_t)f.L, hipMemcpyDeviceToHost, st));
        FOLD_TRY(fold_xfer_wait(s)); // (d_beta_t and d_out are the next piece's too)
    }
    if (out->ell_first)
        HIP_TRY(hipMemcpy2DAsync(out->ell_first, sizeof(double), f.d_ell + (size_t)t0 * s->cfg.n_chains,
                                 (size_t)f.K * sizeof(double), sizeof(double), (size_t)f.L, hipMemcpyDeviceToHost, st));
    return fold_xfer_wait(s);
}

extern "C" int apemost_hip_mbar_log_weights(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g,
                                            double beta_t, double *host_out) {
    CHECK_S(s);
    if (!g || !host_out)
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_log_weights: g or the output is NULL");
    if (!std::isfinite(beta_t) || !(beta_t >= 0))
        return fail(APEMOST_HIP_ERR_INVALID, "mbar_log_weights: the target is %g; a target is finite and >= 0", beta_t);
    MbarArgs a;
    FOLD_TRY(mbar_range(s, "log_weights", t0, t_count, &a));
    MbarFold &f = s->mb;
    hipStream_t st = s->copy_stream;
    const size_t count = (size_t)t_count * s->cfg.n_chains;
    FoldScratch scratch;
    double *d_w;
    FOLD_TRY(fold_alloc(s, scratch, &d_w, count, false));
    std::vector<double> c;
    FOLD_TRY(mbar_upload_g(s, g, std::log((double)t_count), f.d_g, c));
    FOLD_TRY(mbar_launch_row(s, a));
    a.beta_t = f.d_beta_t;
    a.t_stride = 0;
    a.n_t = 1;
    HIP_TRY(hipMemcpyAsync(f.d_beta_t, &beta_t, sizeof(double), hipMemcpyHostToDevice, st));
    FOLD_TRY(mbar_launch_cols(s, a, false, 0.0, f.d_out, nullptr, nullptr)); // G of every ladder into d_out [n_ladders]
    hipLaunchKernelGGL(mbar_weights_kernel, dim3((a.N + kMbarThreads - 1) / kMbarThreads, (unsigned)f.L),
                       dim3(kMbarThreads), 0, st, a, (const double *)f.d_out, d_w);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_out, d_w, count * sizeof(double), hipMemcpyDeviceToHost, st));
    return fold_xfer_wait(s); // (beta_t and d_w live until here)
}
