// abi/fold_peaks.h -- on-device peaks (pt_peaks.h; state: PeaksFold, protocol: abi/fold_common.h).  Its get sorts
// the stored columns instead of copying arrays, and there is no set.
#pragma once

extern "C" int apemost_hip_peaks_begin(apemost_hip_sampler *s, const apemost_hip_peaks_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: config is NULL");
    const int np = s->cfg.n_par;
    FOLD_TRY(fold_check_chains(s, "peaks", cfg->n_keep, cfg->chains, 65535));
    if (cfg->capacity < 1 || cfg->capacity > ((u64)1 << 30))
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: capacity %llu outside [1, 2^30]",
                    (unsigned long long)cfg->capacity);
    if (!cfg->lo || !cfg->hi)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: lo and hi are needed");
    FOLD_TRY(fold_check_ranges("peaks", np, cfg->lo, cfg->hi));
    FOLD_TRY(fold_reset(s, s->pk));
    PeaksFold &f = s->pk;
    f.n_keep = cfg->n_keep;
    f.capacity = cfg->capacity;
    f.n = 0;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_chains, cfg->n_keep, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_lo, np, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_hi, np, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_cols, (size_t)cfg->n_keep * np * cfg->capacity, false));
    HIP_TRY(hipMemcpyAsync(f.d_chains, cfg->chains, cfg->n_keep * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_lo, cfg->lo, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_hi, cfg->hi, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_peaks_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                            uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    PeaksFold &f = s->pk;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("peaks", f.open, d_samples, n_steps, skip, thin, &kept));
    if (kept > f.capacity - f.n)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_accumulate: %llu samples stored, %llu more are beyond capacity = %llu",
                    (unsigned long long)f.n, (unsigned long long)kept, (unsigned long long)f.capacity);
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    PeaksAppendArgs a;
    a.rows = d_samples;
    a.n_chains = s->cfg.n_chains;
    a.n_par = s->cfg.n_par;
    a.n_keep = f.n_keep;
    a.chains = f.d_chains;
    a.skip = skip;
    a.thin = thin;
    a.n_kept = kept;
    a.cols = f.d_cols;
    a.capacity = f.capacity;
    a.n = f.n;
    const dim3 grid((unsigned)((kept + kPeaksThreads - 1) / kPeaksThreads), (unsigned)(f.n_keep * s->cfg.n_par));
    hipLaunchKernelGGL(peaks_append_kernel, grid, dim3(kPeaksThreads), 0, s->copy_stream, a);
    HIP_TRY(hipGetLastError());
    f.n += kept;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_peaks_get(apemost_hip_sampler *s, const apemost_hip_peaks_view *v) {
    CHECK_S(s);
    FOLD_TRY(fold_xfer_check("peaks", s->pk.open, v, false));
    FOLD_TRY(ensure_copy_stream(s));
    const int np = s->cfg.n_par, n_cols = s->pk.n_keep * np;
    const u64 n = s->pk.n;
    u64 padded = kPeaksTile;
    while (padded < n)
        padded <<= 1;
    const u64 n_segments = n > 0 ? (n + kPeaksSegment - 1) / kPeaksSegment : 1;
    // the scratch: keys, segment counts and offsets, and the results, each 256-byte aligned
    size_t at = 0;
    auto region = [&at](size_t bytes) {
        const size_t here = at;
        at = (at + bytes + 255) & ~(size_t)255;
        return here;
    };
    const size_t at_keys = region((size_t)n_cols * padded * sizeof(u64));
    const size_t at_count = region((size_t)n_cols * n_segments * sizeof(unsigned int));
    const size_t at_off = region((size_t)n_cols * n_segments * sizeof(u64));
    const size_t at_values = region((size_t)n_cols * sizeof(u64));
    const size_t at_peaks = region((size_t)n_cols * sizeof(unsigned int));
    const size_t at_cuts = region((size_t)n_cols * kPeaksMax * sizeof(u64));
    const size_t at_left = region((size_t)n_cols * kPeaksMax * sizeof(u64));
    const size_t at_right = region((size_t)n_cols * kPeaksMax * sizeof(u64));
    const size_t at_q = region((size_t)n_cols * kPeaksMax * 3 * sizeof(double));
    const size_t at_set = region((size_t)n_cols * kPeaksMax);
    FoldScratch scratch;
    char *base;
    FOLD_TRY(fold_alloc(s, scratch, &base, at, false));
    PeaksArgs a;
    a.cols = s->pk.d_cols;
    a.capacity = s->pk.capacity;
    a.n = n;
    a.padded = padded;
    a.n_par = np;
    a.lo = s->pk.d_lo;
    a.hi = s->pk.d_hi;
    a.keys = (unsigned long long *)(base + at_keys);
    a.n_segments = n_segments;
    a.seg_count = (unsigned int *)(base + at_count);
    a.seg_off = (unsigned long long *)(base + at_off);
    a.n_values = (unsigned long long *)(base + at_values);
    a.n_peaks = (unsigned int *)(base + at_peaks);
    a.cuts = (unsigned long long *)(base + at_cuts);
    a.left = (unsigned long long *)(base + at_left);
    a.right = (unsigned long long *)(base + at_right);
    a.q = (double *)(base + at_q);
    a.q_set = (unsigned char *)(base + at_set);
    FOLD_TRY(fold_order_behind_stream(s));
    hipStream_t st = s->copy_stream;
    // (peaks beyond those a column has leave their slots 0)
    HIP_TRY(hipMemsetAsync(base + at_cuts, 0, at - at_cuts, st));
    const dim3 threads(kPeaksThreads);
    hipLaunchKernelGGL(peaks_keys_kernel, dim3((unsigned)(padded / kPeaksThreads), n_cols), threads, 0, st, a);
    const dim3 tiles((unsigned)(padded / kPeaksTile), n_cols), pairs((unsigned)(padded / 2 / kPeaksThreads), n_cols);
    hipLaunchKernelGGL(peaks_sort_tile_kernel, tiles, threads, 0, st, a.keys, (unsigned long long)padded, 2ull,
                       (unsigned long long)kPeaksTile);
    for (u64 k = 2 * (u64)kPeaksTile; k <= padded; k <<= 1) {
        for (u64 j = k / 2; j >= (u64)kPeaksTile; j >>= 1)
            hipLaunchKernelGGL(peaks_sort_global_kernel, pairs, threads, 0, st, a.keys, (unsigned long long)padded,
                               (unsigned long long)k, (unsigned long long)j);
        hipLaunchKernelGGL(peaks_sort_tile_kernel, tiles, threads, 0, st, a.keys, (unsigned long long)padded,
                           (unsigned long long)k, (unsigned long long)k);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(peaks_nvalues_kernel, dim3((n_cols + kPeaksThreads - 1) / kPeaksThreads), threads, 0, st, a, n_cols);
    hipLaunchKernelGGL(peaks_cut_count_kernel, dim3((unsigned)n_segments, n_cols), threads, 0, st, a);
    hipLaunchKernelGGL(peaks_cut_scan_kernel, dim3(n_cols), threads, 0, st, a);
    hipLaunchKernelGGL(peaks_cut_write_kernel, dim3((unsigned)((n_segments + kPeaksThreads - 1) / kPeaksThreads), n_cols),
                       threads, 0, st, a);
    hipLaunchKernelGGL(peaks_select_kernel, dim3(n_cols), dim3(128), 0, st, a);
    HIP_TRY(hipGetLastError());
    std::vector<u64> h_values(n_cols), h_left((size_t)n_cols * kPeaksMax), h_right((size_t)n_cols * kPeaksMax);
    std::vector<unsigned int> h_peaks(n_cols);
    std::vector<double> h_q((size_t)n_cols * kPeaksMax * 3);
    std::vector<unsigned char> h_set((size_t)n_cols * kPeaksMax);
    HIP_TRY(hipMemcpyAsync(h_values.data(), a.n_values, h_values.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_peaks.data(), a.n_peaks, h_peaks.size() * sizeof(unsigned int), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_left.data(), a.left, h_left.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_right.data(), a.right, h_right.size() * sizeof(u64), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_q.data(), a.q, h_q.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_set.data(), a.q_set, h_set.size(), hipMemcpyDeviceToHost, st));
    FOLD_TRY(fold_xfer_wait(s));
    if (v->n)
        *v->n = n;
    if (v->n_values)
        memcpy(v->n_values, h_values.data(), h_values.size() * sizeof(u64));
    if (v->n_peaks)
        memcpy(v->n_peaks, h_peaks.data(), h_peaks.size() * sizeof(unsigned int));
    if (v->left)
        memcpy(v->left, h_left.data(), h_left.size() * sizeof(u64));
    if (v->right)
        memcpy(v->right, h_right.data(), h_right.size() * sizeof(u64));
    if (v->q)
        memcpy(v->q, h_q.data(), h_q.size() * sizeof(double));
    if (v->q_set)
        memcpy(v->q_set, h_set.data(), h_set.size());
    for (int col = 0; col < n_cols; col++)
        if (h_peaks[col] > (unsigned int)kPeaksMax)
            return fail(APEMOST_HIP_ERR_INVALID, "peaks_get: kept chain %d, parameter %d: %u peaks, more than %d "
                        "(the reference asserts npeaks < 100)", col / np, col % np, h_peaks[col], kPeaksMax);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_peaks_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    return fold_reset(s, s->pk);
}
