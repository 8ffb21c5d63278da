// abi/fold_summary.h -- the run summary (pt_summary.h; state: SummaryFold, protocol: abi/fold_common.h)
#pragma once

extern "C" int apemost_hip_summary_begin(apemost_hip_sampler *s, const apemost_hip_summary_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "summary_begin: config is NULL");
    const int np = s->cfg.n_par;
    if (cfg->nbins < 1 || cfg->nbins > kSummaryMaxBins)
        return fail(APEMOST_HIP_ERR_INVALID, "summary_begin: nbins %d outside [1,%d]", cfg->nbins, kSummaryMaxBins);
    if (cfg->n_hist_chains < 0 || cfg->n_hist_chains > s->cfg.n_chains)
        return fail(APEMOST_HIP_ERR_INVALID, "summary_begin: n_hist_chains %d outside [0,%d]", cfg->n_hist_chains,
                    s->cfg.n_chains);
    if (cfg->batch_size < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "summary_begin: batch_size must be >= 1");
    if (cfg->n_hist_chains > 0 && (!cfg->lo || !cfg->hi))
        return fail(APEMOST_HIP_ERR_INVALID, "summary_begin: histograms need lo and hi");
    if (cfg->lo && cfg->hi)
        FOLD_TRY(fold_check_ranges("summary", np, cfg->lo, cfg->hi));
    const size_t n_hp = (size_t)cfg->n_hist_chains * np;
    if (cfg->max_batches > ((size_t)1 << 40) || (n_hp > 0 && cfg->max_batches + 1 > ((size_t)1 << 40) / n_hp))
        return fail(APEMOST_HIP_ERR_INVALID, "summary_begin: max_batches %llu too large",
                    (unsigned long long)cfg->max_batches);
    FOLD_TRY(fold_reset(s, s->sum));
    SummaryFold &f = s->sum;
    f.n_hist = cfg->n_hist_chains;
    f.nbins = cfg->nbins;
    f.bs = cfg->batch_size;
    f.max_batches = cfg->max_batches;
    f.n = 0;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_prob_sum, s->cfg.n_chains, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_lo, np, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_hi, np, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_batch, n_hp * (cfg->max_batches + 1), true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_hist, n_hp * cfg->nbins, true));
    if (cfg->lo && cfg->hi) {
        HIP_TRY(hipMemcpyAsync(f.d_lo, cfg->lo, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(f.d_hi, cfg->hi, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_summary_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                              uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    SummaryFold &f = s->sum;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("summary", f.open, d_samples, n_steps, skip, thin, &kept));
    FOLD_TRY(fold_check_batches("summary", f.n, kept, f.bs, f.max_batches));
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const int n_hp = f.n_hist * s->cfg.n_par;
    const int grid = n_hp + (s->cfg.n_chains + kSummaryThreads - 1) / kSummaryThreads;
    // (the LDS bins count in 32 bits: at most 2^31 samples per launch)
    for (u64 k0 = 0; k0 < kept; k0 += (u64)1 << 31) {
        SummaryArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = s->cfg.n_par;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n_kept = kept - k0 < ((u64)1 << 31) ? kept - k0 : (u64)1 << 31;
        a.n_hist = f.n_hist;
        a.nbins = f.nbins;
        a.lo = f.d_lo;
        a.hi = f.d_hi;
        a.bs = f.bs;
        a.left = batches_left(f.n, f.bs);
        a.n_closed = batches_closed(f.n, f.bs);
        a.prob_sum = f.d_prob_sum;
        a.hist = f.d_hist;
        a.batch = f.d_batch;
        a.batch_stride = f.max_batches + 1;
        hipLaunchKernelGGL(summary_kernel, dim3(grid), dim3(kSummaryThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        f.n += a.n_kept;
    }
    return APEMOST_HIP_OK;
}

static int summary_xfer(apemost_hip_sampler *s, const apemost_hip_summary_view *v, bool up) {
    CHECK_S(s);
    SummaryFold &f = s->sum;
    FOLD_TRY(fold_xfer_check("summary", f.open, v, up));
    FOLD_TRY(ensure_copy_stream(s));
    const size_t n_hp = (size_t)f.n_hist * s->cfg.n_par;
    if (up && v->n) {
        if (batches_closed(*v->n, f.bs) > f.max_batches)
            return fail(APEMOST_HIP_ERR_INVALID, "summary_set: %llu samples close more than max_batches batches",
                        (unsigned long long)*v->n);
        if (v->n_batches && *v->n_batches != batches_closed(*v->n, f.bs))
            return fail(APEMOST_HIP_ERR_INVALID, "summary_set: n_batches %llu does not follow from n = %llu",
                        (unsigned long long)*v->n_batches, (unsigned long long)*v->n);
    }
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    FOLD_TRY(copy(f.d_prob_sum, v->prob_sum, s->cfg.n_chains * sizeof(double)));
    FOLD_TRY(copy(f.d_hist, v->hist, n_hp * f.nbins * sizeof(u64)));
    FOLD_TRY(copy(f.d_batch, v->batch_sums, n_hp * (f.max_batches + 1) * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    if (!up && v->n_batches)
        *v->n_batches = batches_closed(f.n, f.bs);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_summary_get(apemost_hip_sampler *s, const apemost_hip_summary_view *v) {
    return summary_xfer(s, v, false);
}

extern "C" int apemost_hip_summary_set(apemost_hip_sampler *s, const apemost_hip_summary_view *v) {
    return summary_xfer(s, v, true);
}

extern "C" int apemost_hip_summary_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    return fold_reset(s, s->sum);
}
