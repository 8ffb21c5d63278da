// abi/fold_reweight.h -- on-device reweighted posteriors (pt_reweight.h; state: ReweightFold, protocol:
// abi/fold_common.h).  The fold is attached to the open MBAR fold (abi/fold_mbar.h): the capacity, the ladders and the
// ranges are that fold's, the two stores advance by separate accumulates and every entry point that computes refuses
// while their kept counts differ.  evaluate and weights run on copy_stream behind every accumulate and return when
// their results are on the host; so does resample (pt_resample.h), whose scratch the fold's first resample allocates
// at the fold's capacity and the fold's memory frees.
#pragma once

constexpr u64 kReweightMaxValues = (u64)1 << 30; // n_cols x capacity x n_chains
constexpr int kReweightMaxTargets = 64;
constexpr u64 kReweightMaxCounts = (u64)1 << 24; // n_ladders x n_t x n_cols x nbins
constexpr u64 kResampleMaxValues = (u64)1 << 26; // n_ladders x n_draws x n_cols

extern "C" int apemost_hip_reweight_begin(apemost_hip_sampler *s, const apemost_hip_reweight_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_begin: config is NULL");
    if (s->cfg.n_chains_global > s->cfg.n_chains)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "reweight_begin: a shard of %d chains of a ladder of %lld: the weights "
                    "need every chain of the ladder on one device", s->cfg.n_chains, (long long)s->cfg.n_chains_global);
    const MbarFold &mb = s->mb;
    if (!mb.open)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_begin: no mbar_begin: the fold is attached to an open mbar fold");
    if (mb.n != 0)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_begin: the mbar fold already stores %llu kept steps; begin before "
                    "the first mbar_accumulate or mbar_set", (unsigned long long)mb.n);
    if (cfg->n_cols < 1 || cfg->n_cols > kReweightMaxCols || !cfg->cols)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_begin: n_cols %d outside [1,%d], or no cols", cfg->n_cols,
                    kReweightMaxCols);
    for (int k = 0; k < cfg->n_cols; k++)
        if (cfg->cols[k] < 0 || cfg->cols[k] > s->cfg.n_par + 1 || (k > 0 && cfg->cols[k] <= cfg->cols[k - 1]))
            return fail(APEMOST_HIP_ERR_INVALID, "reweight_begin: cols[%d] = %d: columns in [0,%d], strictly increasing", k,
                        cfg->cols[k], s->cfg.n_par + 1);
    if (cfg->nbins < 0 || cfg->nbins > kReweightMaxBins)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_begin: nbins %d outside [0,%d]", cfg->nbins, kReweightMaxBins);
    if (cfg->nbins > 0) {
        if (!cfg->lo || !cfg->hi)
            return fail(APEMOST_HIP_ERR_INVALID, "reweight_begin: nbins %d needs lo and hi", cfg->nbins);
        FOLD_TRY(fold_check_ranges("reweight", cfg->n_cols, cfg->lo, cfg->hi));
    }
    const size_t nc = (size_t)s->cfg.n_chains;
    const u64 plane = mb.capacity * nc;
    if ((u64)cfg->n_cols > kReweightMaxValues / plane)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_begin: %d columns x capacity %llu x %zu chains are more than 2^30 "
                    "values; at most %llu columns fit", cfg->n_cols, (unsigned long long)mb.capacity, nc,
                    (unsigned long long)(kReweightMaxValues / plane));
    FOLD_TRY(fold_reset(s, s->rw));
    ReweightFold &f = s->rw;
    f.n_cols = cfg->n_cols;
    f.nbins = cfg->nbins;
    f.words = 2 + f.n_cols + f.n_cols * (f.n_cols + 1) / 2;
    for (int k = 0; k < f.n_cols; k++)
        f.cols[k] = cfg->cols[k];
    f.n = 0;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_x, (size_t)f.n_cols * plane, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_lo, (size_t)f.n_cols, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_hi, (size_t)f.n_cols, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_e, (size_t)plane, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_q, (size_t)plane, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_beta_t, (size_t)kReweightMaxTargets, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_part, (size_t)f.words * mb.L * mb.tiles_max, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_bad, (size_t)mb.L * f.n_cols, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_mkey, (size_t)kReweightMaxTargets * mb.L, false));
    if (f.nbins > 0) {
        HIP_TRY(hipMemcpyAsync(f.d_lo, cfg->lo, f.n_cols * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(f.d_hi, cfg->hi, f.n_cols * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's arrays are read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_reweight_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                               uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    ReweightFold &f = s->rw;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("reweight", f.open, d_samples, n_steps, skip, thin, &kept));
    const u64 capacity = s->mb.capacity;
    if (kept > capacity - f.n)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_accumulate: %llu samples stored, %llu more are beyond capacity = %llu",
                    (unsigned long long)f.n, (unsigned long long)kept, (unsigned long long)capacity);
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const int nc = s->cfg.n_chains;
    const u64 chunk = (u64)1 << 18; // (the grid's y: kept steps / 8)
    for (u64 k0 = 0; k0 < kept; k0 += chunk) {
        ReweightGatherArgs a;
        a.rows = d_samples;
        a.n_chains = nc;
        a.n_par = s->cfg.n_par;
        a.K = s->mb.K;
        a.n_cols = f.n_cols;
        for (int k = 0; k < kReweightMaxCols; k++)
            a.cols[k] = k < f.n_cols ? f.cols[k] : 0;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < chunk ? kept - k0 : chunk);
        a.x = f.d_x + (size_t)f.n * nc;
        a.col_stride = (size_t)capacity * nc;
        a.n_bad = f.d_bad;
        hipLaunchKernelGGL(reweight_gather_kernel,
                           dim3((unsigned)((nc + kMbarGatherThreads - 1) / kMbarGatherThreads), (a.n + 7u) / 8u,
                                (unsigned)f.n_cols),
                           dim3(kMbarGatherThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        f.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int reweight_xfer(apemost_hip_sampler *s, const apemost_hip_reweight_view *v, bool up) {
    CHECK_S(s);
    ReweightFold &f = s->rw;
    FOLD_TRY(fold_xfer_check("reweight", f.open, v, up));
    const u64 capacity = s->mb.capacity;
    if (up && v->n && *v->n > capacity)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_set: %llu samples are beyond capacity = %llu",
                    (unsigned long long)*v->n, (unsigned long long)capacity);
    const u64 n = up && v->n ? *v->n : f.n;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    FOLD_TRY(copy(f.d_bad, v->n_bad, (size_t)s->mb.L * f.n_cols * sizeof(u64)));
    const size_t nc = (size_t)s->cfg.n_chains;
    for (int k = 0; k < f.n_cols && v->x; k++) // (the view's columns hold n rows each, the store's capacity rows)
        FOLD_TRY(copy(f.d_x + (size_t)k * capacity * nc, v->x + (size_t)k * n * nc, (size_t)n * nc * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_reweight_get(apemost_hip_sampler *s, const apemost_hip_reweight_view *v) {
    return reweight_xfer(s, v, false);
}

extern "C" int apemost_hip_reweight_set(apemost_hip_sampler *s, const apemost_hip_reweight_view *v) {
    return reweight_xfer(s, v, true);
}

extern "C" int apemost_hip_reweight_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    return fold_reset(s, s->rw);
}

// ---- computing on the two stores ----
static int reweight_shift(unsigned int N) {
    int bits = 0;
    for (; N; N >>= 1)
        bits++;
    return 63 - bits;
}

// The head of evaluate and weights: both folds open and in step, the range and the counts of non-finite values of both
// stores, g uploaded and lnD of the range formed.  Fills what every kernel of the range shares.
static int reweight_range(apemost_hip_sampler *s, const char *what, u64 t0, u64 t_count, const double *g, ReweightArgs *a) {
    ReweightFold &f = s->rw;
    if (!f.open)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_%s: no reweight_begin", what);
    if (f.n != s->mb.n)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_%s: stores out of step: mbar holds %llu kept steps, reweight %llu",
                    what, (unsigned long long)s->mb.n, (unsigned long long)f.n);
    FOLD_TRY(mbar_range(s, "reweight", t0, t_count, &a->m));
    const MbarFold &mb = s->mb;
    std::vector<u64> bad((size_t)mb.L * f.n_cols);
    HIP_TRY(hipMemcpyAsync(bad.data(), f.d_bad, bad.size() * sizeof(u64), hipMemcpyDeviceToHost, s->copy_stream));
    FOLD_TRY(fold_xfer_wait(s));
    for (int b = 0; b < mb.L; b++)
        for (int k = 0; k < f.n_cols; k++)
            if (bad[(size_t)b * f.n_cols + k])
                return fail(APEMOST_HIP_ERR_INVALID, "reweight_%s: ladder %d stores %llu values of column %d that are not "
                            "finite", what, b, (unsigned long long)bad[(size_t)b * f.n_cols + k], f.cols[k]);
    std::vector<double> c;
    FOLD_TRY(mbar_upload_g(s, g, std::log((double)t_count), mb.d_g, c));
    FOLD_TRY(mbar_launch_row(s, a->m));
    FOLD_TRY(fold_xfer_wait(s)); // (c lives until here)
    a->m.t_stride = 0;
    a->m.n_t = 1;
    a->m.part = f.d_part;
    a->m.part_stride = (size_t)mb.L * mb.tiles_max;
    a->x = f.d_x;
    a->col_stride = (size_t)mb.capacity * s->cfg.n_chains;
    a->n_cols = f.n_cols;
    a->nbins = f.nbins;
    a->shift = reweight_shift(a->m.N);
    a->lo = f.d_lo;
    a->hi = f.d_hi;
    a->e = f.d_e;
    a->q = f.d_q;
    return APEMOST_HIP_OK;
}

// target t of the call (beta in d_beta_t[t]): its maxima into d_mkey[t], then e and q of every sample of the range
static int reweight_launch_weights(apemost_hip_sampler *s, ReweightArgs &a, int t) {
    const ReweightFold &f = s->rw;
    const int L = s->mb.L;
    hipStream_t st = s->copy_stream;
    a.m.beta_t = f.d_beta_t + t;
    a.m.mkey = f.d_mkey + (size_t)t * L;
    HIP_TRY(hipMemsetAsync(a.m.mkey, 0, (size_t)L * sizeof(unsigned long long), st));
    hipLaunchKernelGGL(mbar_max_kernel, dim3(a.m.tiles, 1, (unsigned)L), dim3(kMbarThreads), 0, st, a.m);
    hipLaunchKernelGGL(reweight_weights_kernel, dim3((a.m.N + kReweightThreads - 1) / kReweightThreads, (unsigned)L),
                       dim3(kReweightThreads), 0, st, a);
    HIP_TRY(hipGetLastError());
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_reweight_evaluate(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g,
                                             const double *betas_t, int32_t n_t, const apemost_hip_reweight_sums *out) {
    CHECK_S(s);
    if (!g || !betas_t || !out)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_evaluate: g, the targets or the sums are missing");
    if (n_t < 1 || n_t > kReweightMaxTargets)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_evaluate: n_t %d outside [1,%d]", n_t, kReweightMaxTargets);
    for (int t = 0; t < n_t; t++)
        if (!std::isfinite(betas_t[t]) || !(betas_t[t] >= 0))
            return fail(APEMOST_HIP_ERR_INVALID, "reweight_evaluate: target %d is %g; a target is finite and >= 0", t,
                        betas_t[t]);
    ReweightFold &f = s->rw;
    if (f.open && (u64)s->mb.L * n_t * f.n_cols * (u64)f.nbins > kReweightMaxCounts)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_evaluate: %d ladders x %d targets x %d columns x %d bins are more "
                    "than 2^24 counts", s->mb.L, n_t, f.n_cols, f.nbins);
    ReweightArgs a{};
    FOLD_TRY(reweight_range(s, "evaluate", t0, t_count, g, &a));
    const int L = s->mb.L, ntri = f.n_cols * (f.n_cols + 1) / 2;
    hipStream_t st = s->copy_stream;
    const size_t lt = (size_t)L * n_t, n_hist = lt * f.n_cols * f.nbins;
    FoldScratch scratch;
    double *d_out;
    unsigned long long *d_hist;
    FOLD_TRY(fold_alloc(s, scratch, &d_out, lt * (3 + f.n_cols + ntri), false));
    FOLD_TRY(fold_alloc(s, scratch, &d_hist, n_hist + lt, false)); // (q_total behind the histograms)
    HIP_TRY(hipMemsetAsync(d_hist, 0, (n_hist + lt) * sizeof(unsigned long long), st));
    HIP_TRY(hipMemcpyAsync(f.d_beta_t, betas_t, n_t * sizeof(double), hipMemcpyHostToDevice, st));
    a.n_t = n_t;
    a.out_m = d_out;
    a.out_S0 = d_out + lt;
    a.out_SS = d_out + 2 * lt;
    a.out_S1 = d_out + 3 * lt;
    a.out_cross = a.out_S1 + lt * f.n_cols;
    a.hist_stride = (size_t)n_t * f.n_cols * f.nbins;
    const int items = reweight_items(f.n_cols), waves = kReweightThreads / 64;
    const unsigned hist_grid = a.m.tiles < (unsigned)kReweightHistGrid ? a.m.tiles : (unsigned)kReweightHistGrid;
    for (int t = 0; t < n_t; t++) {
        a.t = t;
        a.hist = d_hist + (size_t)t * f.n_cols * f.nbins;
        a.q_total = d_hist + n_hist + t;
        FOLD_TRY(reweight_launch_weights(s, a, t));
        hipLaunchKernelGGL(reweight_moments_kernel, dim3(a.m.tiles, (unsigned)((items + waves - 1) / waves), (unsigned)L),
                           dim3(kReweightThreads), 0, st, a);
        hipLaunchKernelGGL(reweight_hist_kernel, dim3(hist_grid, (unsigned)(f.nbins > 0 ? f.n_cols : 1), (unsigned)L),
                           dim3(kReweightThreads), 0, st, a);
        hipLaunchKernelGGL(reweight_finish_kernel, dim3((unsigned)(((size_t)L * f.words + 63) / 64)), dim3(64), 0, st, a, L);
        HIP_TRY(hipGetLastError());
    }
    const FoldCopy down{s, false};
    FOLD_TRY(down(a.out_m, out->m, lt * sizeof(double)));
    FOLD_TRY(down(a.out_S0, out->S0, lt * sizeof(double)));
    FOLD_TRY(down(a.out_SS, out->SS, lt * sizeof(double)));
    FOLD_TRY(down(a.out_S1, out->S1, lt * f.n_cols * sizeof(double)));
    FOLD_TRY(down(a.out_cross, out->cross, lt * ntri * sizeof(double)));
    FOLD_TRY(down(d_hist, out->hist, n_hist * sizeof(unsigned long long)));
    FOLD_TRY(down(d_hist + n_hist, out->q_total, lt * sizeof(unsigned long long)));
    if (out->origin)
        for (int k = 0; k < f.n_cols; k++)
            HIP_TRY(hipMemcpy2DAsync(out->origin + k, (size_t)f.n_cols * sizeof(double),
                                     f.d_x + (size_t)k * a.col_stride + (size_t)t0 * s->cfg.n_chains,
                                     (size_t)s->mb.K * sizeof(double), sizeof(double), (size_t)L, hipMemcpyDeviceToHost, st));
    if (out->shift)
        *out->shift = a.shift;
    return fold_xfer_wait(s); // (the scratch lives until here)
}

extern "C" int apemost_hip_reweight_weights(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g,
                                            double beta_t, double *host_e, uint64_t *host_q) {
    CHECK_S(s);
    if (!g)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_weights: g is NULL");
    if (!std::isfinite(beta_t) || !(beta_t >= 0))
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_weights: the target is %g; a target is finite and >= 0", beta_t);
    ReweightArgs a{};
    FOLD_TRY(reweight_range(s, "weights", t0, t_count, g, &a));
    ReweightFold &f = s->rw;
    HIP_TRY(hipMemcpyAsync(f.d_beta_t, &beta_t, sizeof(double), hipMemcpyHostToDevice, s->copy_stream));
    FOLD_TRY(reweight_launch_weights(s, a, 0));
    const size_t count = (size_t)t_count * s->cfg.n_chains;
    const FoldCopy down{s, false};
    FOLD_TRY(down(f.d_e, host_e, count * sizeof(double)));
    FOLD_TRY(down(f.d_q, host_q, count * sizeof(uint64_t)));
    return fold_xfer_wait(s); // (beta_t lives until here)
}

extern "C" int apemost_hip_reweight_resample(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g,
                                             double beta_t, uint32_t n_draws, uint64_t u,
                                             const apemost_hip_reweight_draws *out) {
    CHECK_S(s);
    if (!g)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_resample: g is NULL");
    if (!out)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_resample: out is NULL");
    if (!std::isfinite(beta_t) || !(beta_t >= 0))
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_resample: the target is %g; a target is finite and >= 0", beta_t);
    if (n_draws < 1 || n_draws > kResampleMaxDraws)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_resample: n_draws %u outside [1,2^24]", n_draws);
    ReweightFold &f = s->rw;
    if (f.open && s->mb.open && (u64)s->mb.L * n_draws * (u64)f.n_cols > kResampleMaxValues)
        return fail(APEMOST_HIP_ERR_INVALID, "reweight_resample: %d ladders x %u draws x %d columns are more than 2^26 "
                    "values", s->mb.L, n_draws, f.n_cols);
    ReweightArgs a{};
    FOLD_TRY(reweight_range(s, "resample", t0, t_count, g, &a));
    const MbarFold &mb = s->mb;
    const int L = mb.L;
    hipStream_t st = s->copy_stream;
    if (!f.d_C) {
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_tsum, (size_t)L * mb.tiles_max + L, false));
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_C, (size_t)mb.capacity * s->cfg.n_chains, false));
    }
    HIP_TRY(hipMemcpyAsync(f.d_beta_t, &beta_t, sizeof(double), hipMemcpyHostToDevice, st));
    FOLD_TRY(reweight_launch_weights(s, a, 0));
    const size_t lm = (size_t)L * n_draws;
    FoldScratch scratch;
    unsigned int *d_index;
    double *d_out;
    FOLD_TRY(fold_alloc(s, scratch, &d_index, lm, false));
    FOLD_TRY(fold_alloc(s, scratch, &d_out, lm * f.n_cols, false));
    ResampleArgs r{};
    r.m = a.m;
    r.q = f.d_q;
    r.x = f.d_x;
    r.col_stride = a.col_stride;
    r.n_cols = f.n_cols;
    r.tsum = f.d_tsum;
    r.total = f.d_tsum + (size_t)L * a.m.tiles;
    r.C = f.d_C;
    r.M = n_draws;
    r.u = u;
    r.index = d_index;
    r.out = d_out;
    const dim3 per_tile(a.m.tiles, (unsigned)L);
    hipLaunchKernelGGL(resample_tile_sum_kernel, per_tile, dim3(kResampleThreads), 0, st, r);
    hipLaunchKernelGGL(resample_tile_scan_kernel, dim3((unsigned)L), dim3(kResampleScanThreads), 0, st, r);
    hipLaunchKernelGGL(resample_scan_kernel, per_tile, dim3(kResampleThreads), 0, st, r);
    hipLaunchKernelGGL(resample_search_kernel, dim3((n_draws + kResampleThreads - 1) / kResampleThreads, (unsigned)L),
                       dim3(kResampleThreads), 0, st, r);
    HIP_TRY(hipGetLastError());
    const FoldCopy down{s, false};
    FOLD_TRY(down(d_index, out->index, lm * sizeof(unsigned int)));
    FOLD_TRY(down(d_out, out->x, lm * f.n_cols * sizeof(double)));
    FOLD_TRY(down(r.total, out->q_total, (size_t)L * sizeof(unsigned long long)));
    if (out->shift)
        *out->shift = a.shift;
    return fold_xfer_wait(s); // (the scratch and beta_t live until here)
}
