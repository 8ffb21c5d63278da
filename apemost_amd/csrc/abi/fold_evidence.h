// abi/fold_evidence.h -- on-device evidence fold (pt_evidence.h; state: EvidenceFold, protocol: abi/fold_common.h)
#pragma once

extern "C" int apemost_hip_evidence_begin(apemost_hip_sampler *s, const apemost_hip_evidence_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_begin: config is NULL");
    if (cfg->batch_size < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_begin: batch_size must be >= 1");
    if (!cfg->coef_up || !cfg->coef_down)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_begin: coef_up and coef_down are needed");
    const size_t nc = (size_t)s->cfg.n_chains;
    for (size_t c = 0; c < nc; c++)
        if (!std::isfinite(cfg->coef_up[c]) || !std::isfinite(cfg->coef_down[c]))
            return fail(APEMOST_HIP_ERR_INVALID, "evidence_begin: chain %zu: coefficients (%g, %g) are not finite", c,
                        cfg->coef_up[c], cfg->coef_down[c]);
    if (cfg->max_batches > ((size_t)1 << 40) || cfg->max_batches + 1 > ((size_t)1 << 40) / nc)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_begin: max_batches %llu too large",
                    (unsigned long long)cfg->max_batches);
    FOLD_TRY(fold_reset(s, s->ev));
    EvidenceFold &f = s->ev;
    // the staged column: about 1 Mi values over all chains, at most 2^18 kept steps per launch
    const u64 chunk = fold_chunk((u64)1 << 20, nc, 18);
    f.bs = cfg->batch_size;
    f.max_batches = cfg->max_batches;
    f.chunk = chunk;
    f.n = 0;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_coef, 2 * nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_vals, nc * chunk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_origin, nc, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_sum, nc, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_sq, nc, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_batch, nc * (cfg->max_batches + 1), true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_m, 2 * nc, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_S, 2 * nc, true));
    HIP_TRY(hipMemcpyAsync(f.d_coef, cfg->coef_up, nc * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_coef + nc, cfg->coef_down, nc * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's arrays are read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_evidence_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                               uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    EvidenceFold &f = s->ev;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("evidence", f.open, d_samples, n_steps, skip, thin, &kept));
    FOLD_TRY(fold_check_batches("evidence", f.n, kept, f.bs, f.max_batches));
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const int nc = s->cfg.n_chains;
    for (u64 k0 = 0; k0 < kept; k0 += f.chunk) {
        EvidenceArgs a;
        a.rows = d_samples;
        a.n_chains = nc;
        a.n_par = s->cfg.n_par;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < f.chunk ? kept - k0 : f.chunk);
        a.first = f.n == 0;
        a.bs = f.bs;
        a.left = batches_left(f.n, f.bs);
        a.n_closed = batches_closed(f.n, f.bs);
        a.batch_stride = f.max_batches + 1;
        a.coef = f.d_coef;
        a.vals = f.d_vals;
        a.origin = f.d_origin;
        a.sum = f.d_sum;
        a.sq = f.d_sq;
        a.batch = f.d_batch;
        a.m = f.d_m;
        a.S = f.d_S;
        hipLaunchKernelGGL(evidence_gather_kernel,
                           dim3((unsigned)((nc + kEvidenceGatherThreads - 1) / kEvidenceGatherThreads), (a.n + 7u) / 8u),
                           dim3(kEvidenceGatherThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(evidence_fold_kernel,
                           dim3((unsigned)((nc + kEvidenceThreads - 1) / kEvidenceThreads), (unsigned)kEvidenceQuantities),
                           dim3(kEvidenceThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        f.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int evidence_xfer(apemost_hip_sampler *s, const apemost_hip_evidence_view *v, bool up) {
    CHECK_S(s);
    EvidenceFold &f = s->ev;
    FOLD_TRY(fold_xfer_check("evidence", f.open, v, up));
    if (up && v->n && batches_closed(*v->n, f.bs) > f.max_batches)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_set: %llu samples close more than max_batches batches",
                    (unsigned long long)*v->n);
    const size_t nc = (size_t)s->cfg.n_chains;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    FOLD_TRY(copy(f.d_origin, v->origin, nc * sizeof(double)));
    FOLD_TRY(copy(f.d_sum, v->sum, nc * sizeof(double)));
    FOLD_TRY(copy(f.d_sq, v->sq, nc * sizeof(double)));
    FOLD_TRY(copy(f.d_batch, v->batch, nc * (f.max_batches + 1) * sizeof(double)));
    FOLD_TRY(copy(f.d_m, v->m, 2 * nc * sizeof(double)));
    FOLD_TRY(copy(f.d_S, v->S, 2 * nc * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_evidence_get(apemost_hip_sampler *s, const apemost_hip_evidence_view *v) {
    return evidence_xfer(s, v, false);
}

extern "C" int apemost_hip_evidence_set(apemost_hip_sampler *s, const apemost_hip_evidence_view *v) {
    return evidence_xfer(s, v, true);
}

extern "C" int apemost_hip_evidence_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    return fold_reset(s, s->ev);
}
