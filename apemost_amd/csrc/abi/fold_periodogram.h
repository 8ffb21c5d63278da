// abi/fold_periodogram.h -- on-device residual periodogram (pt_periodogram.h; state: PeriodogramFold, protocol:
// abi/fold_common.h)
#pragma once

constexpr int kPeriodogramWords = 7;     // origin, sum, sq, pmin, pmax, sum_c, sum_s
constexpr int kPeriodogramPeakWords = 5; // origin, sum, sq, min, max of a kept chain's highest peak
constexpr u64 kPeriodogramScratch = (u64)1 << 25; // doubles of one scratch array at most, while a piece holds a step

#define PERIODOGRAM_HAS_RESIDUAL(s, what)                                                                             \
    do {                                                                                                             \
        if ((s)->cfg.model == APEMOST_MODEL_USER)                                                                    \
            return fail(APEMOST_HIP_ERR_UNSUPPORTED, what ": a user-supplied device model has no residual law here"); \
        if (!periodogram_has_residual((s)->cfg.model))                                                               \
            return fail(APEMOST_HIP_ERR_UNSUPPORTED, what ": the pulse models' data already are a power spectrum; "  \
                        "the residual periodogram is for simplesin and sine3");                                     \
    } while (0)

static int periodogram_check_grid(const char *who, int32_t n_freq, const double *freqs) {
    if (n_freq < 1 || n_freq > kPeriodogramMaxFreq)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: n_freq %d outside [1,%d]", who, n_freq, kPeriodogramMaxFreq);
    if (!freqs)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: freqs is NULL", who);
    for (int j = 0; j < n_freq; j++)
        if (std::isnan(freqs[j]))
            return fail(APEMOST_HIP_ERR_INVALID, "%s: freqs[%d] is NaN", who, j);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_periodogram_begin(apemost_hip_sampler *s, int32_t n_keep, const int32_t *chains, int32_t n_freq,
                                             const double *freqs, const double *weights, const double *level) {
    CHECK_S(s);
    PERIODOGRAM_HAS_RESIDUAL(s, "periodogram_begin");
    FOLD_TRY(fold_check_chains(s, "periodogram", n_keep, chains));
    FOLD_TRY(periodogram_check_grid("periodogram_begin", n_freq, freqs));
    if (n_keep > 65535) // (the kept chain is a grid's y or z)
        return fail(APEMOST_HIP_ERR_INVALID, "periodogram_begin: n_keep %d above 65535", n_keep);
    if (!weights || !level)
        return fail(APEMOST_HIP_ERR_INVALID, "periodogram_begin: %s is NULL", weights ? "level" : "weights");
    const u64 n_series = (u64)n_keep * (u64)n_freq;
    if (n_series > ((u64)1 << 24))
        return fail(APEMOST_HIP_ERR_INVALID, "periodogram_begin: %d chains x %d frequencies: more than 2^24 series", n_keep,
                    n_freq);
    for (u64 q = 0; q < 3 * n_series; q++)
        if (std::isnan(weights[q]))
            return fail(APEMOST_HIP_ERR_INVALID, "periodogram_begin: weights[%llu][%llu][%llu] is NaN",
                        (unsigned long long)(q / 3 / (u64)n_freq), (unsigned long long)(q / 3 % (u64)n_freq),
                        (unsigned long long)(q % 3));
    for (int k = 0; k < n_keep; k++)
        if (std::isnan(level[k]))
            return fail(APEMOST_HIP_ERR_INVALID, "periodogram_begin: level[%d] is NaN", k);
    const int np = s->cfg.n_par;
    std::vector<int> len;
    bool ragged = false;
    const int nd = kept_lengths(s, n_keep, chains, len, &ragged);
    const u64 n_rows = (u64)n_keep * (u64)nd;
    if (n_rows > ((u64)1 << 20))
        return fail(APEMOST_HIP_ERR_INVALID, "periodogram_begin: %d chains x %d data: more than 2^20 series", n_keep, nd);
    if (np > kPointwiseTile)
        return fail(APEMOST_HIP_ERR_INVALID, "periodogram_begin: %d parameters, more than %d", np, kPointwiseTile);
    FOLD_TRY(fold_reset(s, s->pg));
    PeriodogramFold &f = s->pg;
    f.n_keep = n_keep;
    f.n_data = nd;
    f.n_freq = n_freq;
    const u64 widest = n_series > n_rows ? n_series : n_rows, fit = kPeriodogramScratch / widest;
    f.piece = (int)(fit < 1 ? 1 : fit > (u64)kPeriodogramPiece ? (u64)kPeriodogramPiece : fit);
    f.n = 0;
    const size_t ns = (size_t)n_series, nk = (size_t)n_keep, piece = (size_t)f.piece;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_chains, nk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_x, (size_t)n_rows, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_y, (size_t)n_rows, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_freqs, (size_t)n_freq, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_weights, 3 * ns, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_level, nk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_state, kPeriodogramWords * ns, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_exceed, ns, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_peak, kPeriodogramPeakWords * nk, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_peak_counts, nk * ((size_t)n_freq + 1), true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_r, (size_t)n_rows * piece, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_C, ns * piece, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_S, ns * piece, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_P, ns * piece, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_pk_m, nk * piece, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_pk_arg, nk * piece, false));
    HIP_TRY(hipMemcpyAsync(f.d_chains, chains, nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_freqs, freqs, (size_t)n_freq * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_weights, weights, 3 * ns * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_level, level, nk * sizeof(double), hipMemcpyHostToDevice, s->stream));
    if (ragged) {
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_len, nk, false));
        HIP_TRY(hipMemcpyAsync(f.d_len, len.data(), nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    }
    for (int k = 0; k < n_keep; k++) {
        // columns 0 and 1 of the kept chain's own ladder (the data is stored by columns, ladder after ladder), in that
        // ladder's own length
        const size_t mine = (size_t)len[k];
        const double *col0 = ladder_data(s, s->batch ? chains[k] / s->per_ladder : 0);
        HIP_TRY(hipMemcpyAsync(f.d_x + (size_t)k * nd, col0, mine * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(f.d_y + (size_t)k * nd, col0 + mine, mine * sizeof(double), hipMemcpyDeviceToDevice,
                               s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's arrays are read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_periodogram_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                                  uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    PERIODOGRAM_HAS_RESIDUAL(s, "periodogram_accumulate");
    PeriodogramFold &f = s->pg;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("periodogram", f.open, d_samples, n_steps, skip, thin, &kept));
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const size_t ns = (size_t)f.n_keep * f.n_freq, nk = (size_t)f.n_keep;
    const u64 piece = (u64)f.piece;
    for (u64 k0 = 0; k0 < kept; k0 += piece) {
        PeriodogramArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = s->cfg.n_par;
        a.n_keep = f.n_keep;
        a.chains = f.d_chains;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < piece ? kept - k0 : piece);
        a.piece = (unsigned int)f.piece;
        a.n0 = f.n;
        a.n_data = f.n_data;
        a.n_blocks = (f.n_data + kPeriodogramWave - 1) / kPeriodogramWave;
        a.x = f.d_x;
        a.y = f.d_y;
        a.len = f.d_len;
        a.n_freq = f.n_freq;
        a.n_tiles = (f.n_freq + kPeriodogramWave - 1) / kPeriodogramWave;
        a.freqs = f.d_freqs;
        a.weights = f.d_weights;
        a.level = f.d_level;
        a.r = f.d_r;
        a.C = f.d_C;
        a.S = f.d_S;
        a.P = f.d_P;
        a.origin = f.d_state;
        a.sum = f.d_state + ns;
        a.sq = f.d_state + 2 * ns;
        a.pmin = f.d_state + 3 * ns;
        a.pmax = f.d_state + 4 * ns;
        a.sum_c = f.d_state + 5 * ns;
        a.sum_s = f.d_state + 6 * ns;
        a.exceed = f.d_exceed;
        a.pk_m = f.d_pk_m;
        a.pk_arg = f.d_pk_arg;
        a.peak_origin = f.d_peak;
        a.peak_sum = f.d_peak + nk;
        a.peak_sq = f.d_peak + 2 * nk;
        a.peak_min = f.d_peak + 3 * nk;
        a.peak_max = f.d_peak + 4 * nk;
        a.peak_counts = f.d_peak_counts;
        const dim3 wave(kPeriodogramWave);
        const unsigned int group = kPeriodogramGroup, side = kPeriodogramWaves * kPeriodogramSide;
        with_builtin_model(s->cfg.model, [&](auto m) {
            constexpr int M = decltype(m)::value;
            if constexpr (periodogram_has_residual(M))
                hipLaunchKernelGGL(periodogram_resid_kernel<M>, dim3((unsigned)a.n_blocks * (unsigned)a.n_keep,
                                                                    (a.n + group - 1) / group), wave, 0, s->copy_stream, a);
        });
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(periodogram_sum_kernel, dim3((unsigned)a.n_tiles, (a.n + side - 1) / side, (unsigned)a.n_keep),
                           dim3(kPeriodogramWaves * kPeriodogramWave), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(periodogram_fold_kernel, dim3((unsigned)a.n_tiles, (unsigned)a.n_keep), wave, 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(periodogram_peak_kernel, dim3(a.n, (unsigned)a.n_keep), wave, 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(periodogram_peak_fold_kernel, dim3((unsigned)a.n_keep), wave, 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        f.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int periodogram_xfer(apemost_hip_sampler *s, const apemost_hip_periodogram_view *v, bool up) {
    PeriodogramFold &f = s->pg;
    FOLD_TRY(fold_xfer_check("periodogram", f.open, v, up));
    const size_t ns = (size_t)f.n_keep * f.n_freq, nk = (size_t)f.n_keep;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    double *const series[kPeriodogramWords] = {v->origin, v->sum, v->sq, v->pmin, v->pmax, v->sum_c, v->sum_s};
    for (int q = 0; q < kPeriodogramWords; q++)
        FOLD_TRY(copy(f.d_state + (size_t)q * ns, series[q], ns * sizeof(double)));
    FOLD_TRY(copy(f.d_exceed, v->exceed, ns * sizeof(u64)));
    double *const peak[kPeriodogramPeakWords] = {v->peak_origin, v->peak_sum, v->peak_sq, v->peak_min, v->peak_max};
    for (int q = 0; q < kPeriodogramPeakWords; q++)
        FOLD_TRY(copy(f.d_peak + (size_t)q * nk, peak[q], nk * sizeof(double)));
    FOLD_TRY(copy(f.d_peak_counts, v->peak_counts, nk * ((size_t)f.n_freq + 1) * sizeof(u64)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_periodogram_get(apemost_hip_sampler *s, const apemost_hip_periodogram_view *v) {
    CHECK_S(s);
    PERIODOGRAM_HAS_RESIDUAL(s, "periodogram_get");
    return periodogram_xfer(s, v, false);
}

extern "C" int apemost_hip_periodogram_set(apemost_hip_sampler *s, const apemost_hip_periodogram_view *v) {
    CHECK_S(s);
    PERIODOGRAM_HAS_RESIDUAL(s, "periodogram_set");
    return periodogram_xfer(s, v, true);
}

extern "C" int apemost_hip_periodogram_lengths(apemost_hip_sampler *s, int32_t *len) {
    CHECK_S(s);
    PERIODOGRAM_HAS_RESIDUAL(s, "periodogram_lengths");
    const PeriodogramFold &f = s->pg;
    if (!f.open || !len)
        return fail(APEMOST_HIP_ERR_INVALID, "periodogram_lengths: %s", f.open ? "len is NULL" : "no periodogram_begin");
    for (int k = 0; k < f.n_keep; k++)
        len[k] = f.n_data;
    if (f.d_len) {
        HIP_TRY(hipMemcpyAsync(len, f.d_len, (size_t)f.n_keep * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_periodogram_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    PERIODOGRAM_HAS_RESIDUAL(s, "periodogram_end");
    return fold_reset(s, s->pg);
}

extern "C" int apemost_hip_periodogram_values(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x,
                                              const double *x, const double *y, int32_t n_freq, const double *freqs,
                                              const double *w, double *r, double *c, double *s_out, double *C, double *S,
                                              double *P, double *peak, int32_t *arg) {
    CHECK_S(s);
    PERIODOGRAM_HAS_RESIDUAL(s, "periodogram_values");
    FOLD_TRY(periodogram_check_grid("periodogram_values", n_freq, freqs));
    const int np = s->cfg.n_par;
    const u64 most = (u64)1 << 26;
    if (n < 1 || n_x < 1 || !params || !x || !y || !w || !r || !c || !s_out || !C || !S || !P || !peak || !arg ||
        (u64)n * (u64)n_x > most || (u64)n_freq * (u64)n_x > most || (u64)n * (u64)n_freq > most)
        return fail(APEMOST_HIP_ERR_INVALID, "periodogram_values: %d rows x %d data (n_x) x %d frequencies: a product above "
                    "2^26, or a NULL array", n, n_x, n_freq);
    FoldScratch scratch;
    double *d_par = nullptr, *d_x = nullptr, *d_y = nullptr, *d_f = nullptr, *d_w = nullptr, *d_r = nullptr, *d_c = nullptr,
           *d_s = nullptr, *d_C = nullptr, *d_S = nullptr, *d_P = nullptr, *d_peak = nullptr;
    int *d_arg = nullptr;
    const size_t nr = (size_t)n * n_x, nt = (size_t)n_freq * n_x, nf = (size_t)n * n_freq;
    const int rc = [&]() -> int { // (whatever fails, the stream is waited for before the scratch goes)
        FOLD_TRY(fold_alloc(s, scratch, &d_par, (size_t)n * np, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_x, (size_t)n_x, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_y, (size_t)n_x, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_f, (size_t)n_freq, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_w, 3 * (size_t)n_freq, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_r, nr, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_c, nt, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_s, nt, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_C, nf, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_S, nf, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_P, nf, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_peak, (size_t)n, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_arg, (size_t)n, false));
        HIP_TRY(hipMemcpyAsync(d_par, params, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(d_x, x, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(d_y, y, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(d_f, freqs, (size_t)n_freq * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(d_w, w, 3 * (size_t)n_freq * sizeof(double), hipMemcpyHostToDevice, s->stream));
        const dim3 wave(kPeriodogramWave);
        const unsigned int xb = (unsigned)((n_x + kPeriodogramWave - 1) / kPeriodogramWave),
                           fb = (unsigned)((n_freq + kPeriodogramWave - 1) / kPeriodogramWave);
        // (the grid's y holds at most 65535 blocks: rows and frequencies are taken 32768 at a time)
        for (int r0 = 0; r0 < n; r0 += 32768) {
            const int cnt = n - r0 < 32768 ? n - r0 : 32768;
            with_builtin_model(s->cfg.model, [&](auto m) {
                constexpr int M = decltype(m)::value;
                if constexpr (periodogram_has_residual(M))
                    hipLaunchKernelGGL(periodogram_values_kernel<M>, dim3(xb, (unsigned)cnt), wave, 0, s->stream,
                                       (const double *)d_par + (size_t)r0 * np, np, (int)n_x, (const double *)d_x,
                                       (const double *)d_y, d_r + (size_t)r0 * n_x);
            });
            HIP_TRY(hipGetLastError());
        }
        for (int j0 = 0; j0 < n_freq; j0 += 32768) {
            const int cnt = n_freq - j0 < 32768 ? n_freq - j0 : 32768;
            hipLaunchKernelGGL(periodogram_trig_kernel, dim3(xb, (unsigned)cnt), wave, 0, s->stream, cnt,
                               (const double *)d_f + j0, (int)n_x, (const double *)d_x, d_c + (size_t)j0 * n_x,
                               d_s + (size_t)j0 * n_x);
            HIP_TRY(hipGetLastError());
        }
        for (int r0 = 0; r0 < n; r0 += 32768) {
            const int cnt = n - r0 < 32768 ? n - r0 : 32768;
            hipLaunchKernelGGL(periodogram_values_sum_kernel, dim3(fb, (unsigned)cnt), wave, 0, s->stream, (int)n_x, (int)n_freq,
                               (const double *)d_r + (size_t)r0 * n_x, (const double *)d_c, (const double *)d_s,
                               (const double *)d_w, d_C + (size_t)r0 * n_freq, d_S + (size_t)r0 * n_freq,
                               d_P + (size_t)r0 * n_freq);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(periodogram_values_peak_kernel, dim3((unsigned)n), wave, 0, s->stream, (int)n_freq,
                           (const double *)d_P, d_peak, d_arg);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(r, d_r, nr * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(c, d_c, nt * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(s_out, d_s, nt * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(C, d_C, nf * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(S, d_S, nf * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(P, d_P, nf * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(peak, d_peak, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(arg, d_arg, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        return APEMOST_HIP_OK;
    }();
    const hipError_t sync = hipStreamSynchronize(s->stream);
    FOLD_TRY(rc);
    HIP_TRY(sync);
    return APEMOST_HIP_OK;
}
