// abi/fold_joint.h -- on-device joint marginals (pt_joint.h; state: JointFold, protocol: abi/fold_common.h)
#pragma once

extern "C" int apemost_hip_joint_begin(apemost_hip_sampler *s, const apemost_hip_joint_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: config is NULL");
    const int np = s->cfg.n_par;
    FOLD_TRY(fold_check_chains(s, "joint", cfg->n_keep, cfg->chains, 65535));
    if (cfg->nbins < 1 || cfg->nbins > kJointMaxBins)
        return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: nbins %d outside [1,%d]", cfg->nbins, kJointMaxBins);
    std::vector<int> pairs;
    if (!cfg->pairs) { // all i < j in lexicographic order
        for (int i = 0; i < np; i++)
            for (int j = i + 1; j < np; j++) {
                pairs.push_back(i);
                pairs.push_back(j);
            }
    } else {
        const long long all = (long long)np * (np - 1) / 2;
        if (cfg->n_pairs < 0 || cfg->n_pairs > all)
            return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: n_pairs %d outside [0,%lld]", cfg->n_pairs, all);
        std::vector<char> seen((size_t)np * np, 0);
        for (int q = 0; q < cfg->n_pairs; q++) {
            const int i = cfg->pairs[2 * q], j = cfg->pairs[2 * q + 1];
            if (i < 0 || j >= np || i >= j || seen[(size_t)i * np + j])
                return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: pairs[%d] = (%d, %d): 0 <= i < j < %d, no duplicates", q, i,
                            j, np);
            seen[(size_t)i * np + j] = 1;
            pairs.push_back(i);
            pairs.push_back(j);
        }
    }
    const int n_pairs = (int)(pairs.size() / 2);
    if (!cfg->lo || !cfg->hi)
        return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: lo and hi are needed");
    FOLD_TRY(fold_check_ranges("joint", np, cfg->lo, cfg->hi));
    const u64 n_counts = (u64)cfg->n_keep * n_pairs * cfg->nbins * cfg->nbins; // (< 2^16 2^16 2^18: no overflow)
    if (n_pairs > 65535 || n_counts * sizeof(u64) > ((u64)1 << 30))
        return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: %d chains x %d pairs x %d^2 bins: counts above 2^30 bytes",
                    cfg->n_keep, n_pairs, cfg->nbins);
    FOLD_TRY(fold_reset(s, s->jt));
    JointFold &f = s->jt;
    const size_t n_cols = (size_t)cfg->n_keep * np, tri = (size_t)np * (np + 1) / 2;
    // the staged columns: about 4 Mi values over all of them, at most 2^18 kept steps per launch (the LDS counters
    // are 32 bits wide)
    const u64 chunk = fold_chunk((u64)1 << 22, n_cols, 18);
    f.n_keep = cfg->n_keep;
    f.nbins = cfg->nbins;
    f.n_pairs = n_pairs;
    f.chunk = chunk;
    f.n = 0;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_chains, cfg->n_keep, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_pairs, (size_t)n_pairs * 2, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_lo, np, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_hi, np, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_vals, n_cols * chunk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_bins, n_cols * chunk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_origin, n_cols, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_sum, n_cols, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_cross, cfg->n_keep * tri, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_counts, n_counts, true));
    HIP_TRY(hipMemcpyAsync(f.d_chains, cfg->chains, cfg->n_keep * sizeof(int), hipMemcpyHostToDevice, s->stream));
    if (n_pairs > 0)
        HIP_TRY(hipMemcpyAsync(f.d_pairs, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_lo, cfg->lo, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_hi, cfg->hi, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (`pairs` and the caller's arrays are read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_joint_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                            uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    JointFold &f = s->jt;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("joint", f.open, d_samples, n_steps, skip, thin, &kept));
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const int np = s->cfg.n_par, n_cols = f.n_keep * np;
    const int band_rows = joint_band_rows(f.nbins), n_bands = (f.nbins + band_rows - 1) / band_rows;
    const int entries = f.n_keep * (np + np * (np + 1) / 2);
    for (u64 k0 = 0; k0 < kept; k0 += f.chunk) {
        JointArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = np;
        a.n_keep = f.n_keep;
        a.chains = f.d_chains;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < f.chunk ? kept - k0 : f.chunk);
        a.chunk = f.chunk;
        a.nbins = f.nbins;
        a.n_pairs = f.n_pairs;
        a.pairs = f.d_pairs;
        a.lo = f.d_lo;
        a.hi = f.d_hi;
        a.vals = f.d_vals;
        a.bins = f.d_bins;
        a.first = f.n == 0;
        a.counts = f.d_counts;
        a.origin = f.d_origin;
        a.sum = f.d_sum;
        a.cross = f.d_cross;
        hipLaunchKernelGGL(joint_gather_kernel, dim3((a.n + kJointGatherPer - 1) / kJointGatherPer, (unsigned)n_cols),
                           dim3(kJointThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        if (f.n_pairs > 0) {
            hipLaunchKernelGGL(joint_pair_kernel, dim3((unsigned)n_bands, (unsigned)f.n_pairs, (unsigned)f.n_keep),
                               dim3(kJointThreads), 0, s->copy_stream, a);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(joint_moments_kernel, dim3((unsigned)((entries + kJointMomentThreads - 1) / kJointMomentThreads)),
                           dim3(kJointMomentThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        f.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int joint_xfer(apemost_hip_sampler *s, const apemost_hip_joint_view *v, bool up) {
    CHECK_S(s);
    JointFold &f = s->jt;
    FOLD_TRY(fold_xfer_check("joint", f.open, v, up));
    const size_t np = s->cfg.n_par, n_cols = (size_t)f.n_keep * np, tri = np * (np + 1) / 2;
    const size_t n_counts = (size_t)f.n_keep * f.n_pairs * f.nbins * f.nbins;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    FOLD_TRY(copy(f.d_counts, v->counts, n_counts * sizeof(u64)));
    FOLD_TRY(copy(f.d_origin, v->origin, n_cols * sizeof(double)));
    FOLD_TRY(copy(f.d_sum, v->sum, n_cols * sizeof(double)));
    FOLD_TRY(copy(f.d_cross, v->cross, f.n_keep * tri * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_joint_get(apemost_hip_sampler *s, const apemost_hip_joint_view *v) {
    return joint_xfer(s, v, false);
}

extern "C" int apemost_hip_joint_set(apemost_hip_sampler *s, const apemost_hip_joint_view *v) {
    return joint_xfer(s, v, true);
}

extern "C" int apemost_hip_joint_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    return fold_reset(s, s->jt);
}
