// abi/fold_check.h -- on-device predictive checks (pt_check.h; state: CheckFold, protocol: abi/fold_common.h) and the
// null quantiles of its statistics, which are host arithmetic
#pragma once

constexpr int kCheckWords = 7;     // origin, sum, sq, sum_u, m, S, SU
constexpr int kCheckStatWords = 5; // origin, sum, sq, min, max of a kept chain's statistic

#define CHECK_HAS_CDF(s, what)                                                                                   \
    do {                                                                                                        \
        if ((s)->cfg.model == APEMOST_MODEL_USER)                                                               \
            return fail(APEMOST_HIP_ERR_UNSUPPORTED, what ": a user-supplied device model: its hooks give a "   \
                        "curve and a datum's term but no predictive CDF; hooks for the checks are a follow-up"); \
    } while (0)

extern "C" int apemost_hip_check_begin(apemost_hip_sampler *s, int32_t n_keep, const int32_t *chains, int32_t n_edges,
                                       const double *edges) {
    CHECK_S(s);
    CHECK_HAS_CDF(s, "check_begin");
    FOLD_TRY(fold_check_chains(s, "check", n_keep, chains));
    if (n_edges < 0 || n_edges > kCheckMaxEdges)
        return fail(APEMOST_HIP_ERR_INVALID, "check_begin: n_edges %d outside [0,%d]", n_edges, kCheckMaxEdges);
    if ((n_edges > 0) != (edges != nullptr))
        return fail(APEMOST_HIP_ERR_INVALID, "check_begin: n_edges = %d with edges %s: edges [3][n_edges], or NULL and 0",
                    n_edges, edges ? "given" : "NULL");
    for (int q = 0; q < kCheckStats; q++)
        for (int j = 0; j < n_edges; j++) {
            const double e = edges[(size_t)q * n_edges + j];
            if (!std::isfinite(e) || (j > 0 && !(e > edges[(size_t)q * n_edges + j - 1])))
                return fail(APEMOST_HIP_ERR_INVALID, "check_begin: edges[%d][%d] = %g: finite and strictly ascending", q, j, e);
        }
    const int np = s->cfg.n_par;
    std::vector<int> len;
    bool ragged = false;
    const int nd = kept_lengths(s, n_keep, chains, len, &ragged);
    const u64 n_series = (u64)n_keep * (u64)nd;
    if (n_series > ((u64)1 << 20))
        return fail(APEMOST_HIP_ERR_INVALID, "check_begin: %d chains x %d data: more than 2^20 series", n_keep, nd);
    if (np > kPointwiseTile)
        return fail(APEMOST_HIP_ERR_INVALID, "check_begin: %d parameters, more than %d", np, kPointwiseTile);
    FOLD_TRY(fold_reset(s, s->ck));
    CheckFold &f = s->ck;
    f.n_keep = n_keep;
    f.n_data = nd;
    f.n_edges = n_edges;
    f.c = pointwise_c(s);
    f.inv_sigma = 1.0 / s->sh.consts.sigma;
    f.n = 0;
    const size_t ns = (size_t)n_series, nk = (size_t)n_keep;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_chains, nk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_x, ns, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_y, ns, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_state, kCheckWords * ns, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_stat, kCheckStatWords * nk * kCheckStats, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_T, nk * kCheckStats * kPointwisePiece, false));
    HIP_TRY(hipMemcpyAsync(f.d_chains, chains, nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    if (ragged) {
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_len, nk, false));
        HIP_TRY(hipMemcpyAsync(f.d_len, len.data(), nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    }
    if (n_edges > 0) {
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_edges, (size_t)kCheckStats * n_edges, false));
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_counts, nk * kCheckStats * (size_t)(n_edges + 2), true));
        HIP_TRY(hipMemcpyAsync(f.d_edges, edges, (size_t)kCheckStats * n_edges * sizeof(double), hipMemcpyHostToDevice,
                               s->stream));
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

extern "C" int apemost_hip_check_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                            uint64_t thin) {
    CHECK_S(s);
    CHECK_HAS_CDF(s, "check_accumulate");
    CheckFold &f = s->ck;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("check", f.open, d_samples, n_steps, skip, thin, &kept));
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const size_t ns = (size_t)f.n_keep * f.n_data, nq = (size_t)f.n_keep * kCheckStats;
    for (u64 k0 = 0; k0 < kept; k0 += kPointwisePiece) {
        CheckArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = s->cfg.n_par;
        a.n_keep = f.n_keep;
        a.chains = f.d_chains;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < (u64)kPointwisePiece ? kept - k0 : (u64)kPointwisePiece);
        a.n0 = f.n;
        a.n_data = f.n_data;
        a.n_blocks = (f.n_data + kPointwiseWave - 1) / kPointwiseWave;
        a.x = f.d_x;
        a.y = f.d_y;
        a.c = f.c;
        a.inv_sigma = f.inv_sigma;
        a.origin = f.d_state;
        a.sum = f.d_state + ns;
        a.sq = f.d_state + 2 * ns;
        a.sum_u = f.d_state + 3 * ns;
        a.m = f.d_state + 4 * ns;
        a.S = f.d_state + 5 * ns;
        a.SU = f.d_state + 6 * ns;
        a.len = f.d_len;
        a.T = f.d_T;
        a.stat_origin = f.d_stat;
        a.stat_sum = f.d_stat + nq;
        a.stat_sq = f.d_stat + 2 * nq;
        a.stat_min = f.d_stat + 3 * nq;
        a.stat_max = f.d_stat + 4 * nq;
        a.edges = f.d_edges;
        a.n_edges = f.n_edges;
        a.counts = f.d_counts;
        const dim3 block(kPointwiseWave);
        const unsigned int rows = (unsigned int)check_rows(s->cfg.model, a.n_par);
        with_builtin_model(s->cfg.model, [&](auto m) {
            hipLaunchKernelGGL(check_fold_kernel<decltype(m)::value>, dim3((unsigned)a.n_blocks * (unsigned)a.n_keep), block, 0,
                               s->copy_stream, a);
            hipLaunchKernelGGL(check_stat_kernel<decltype(m)::value>, dim3((unsigned)a.n_keep, (a.n + rows - 1) / rows), block,
                               0, s->copy_stream, a);
        });
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(check_stat_fold_kernel, dim3((unsigned)a.n_keep, kCheckStats), block, 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        f.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int check_xfer(apemost_hip_sampler *s, const apemost_hip_check_view *v, bool up) {
    CheckFold &f = s->ck;
    FOLD_TRY(fold_xfer_check("check", f.open, v, up));
    const size_t ns = (size_t)f.n_keep * f.n_data, nq = (size_t)f.n_keep * kCheckStats;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    double *const series[kCheckWords] = {v->origin, v->sum, v->sq, v->sum_u, v->m, v->S, v->SU};
    for (int q = 0; q < kCheckWords; q++)
        FOLD_TRY(copy(f.d_state + (size_t)q * ns, series[q], ns * sizeof(double)));
    double *const stat[kCheckStatWords] = {v->stat_origin, v->stat_sum, v->stat_sq, v->stat_min, v->stat_max};
    for (int q = 0; q < kCheckStatWords; q++)
        FOLD_TRY(copy(f.d_stat + (size_t)q * nq, stat[q], nq * sizeof(double)));
    if (f.d_counts)
        FOLD_TRY(copy(f.d_counts, v->counts, nq * (size_t)(f.n_edges + 2) * sizeof(u64)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_check_get(apemost_hip_sampler *s, const apemost_hip_check_view *v) {
    CHECK_S(s);
    CHECK_HAS_CDF(s, "check_get");
    return check_xfer(s, v, false);
}

extern "C" int apemost_hip_check_set(apemost_hip_sampler *s, const apemost_hip_check_view *v) {
    CHECK_S(s);
    CHECK_HAS_CDF(s, "check_set");
    return check_xfer(s, v, true);
}

extern "C" int apemost_hip_check_lengths(apemost_hip_sampler *s, int32_t *len) {
    CHECK_S(s);
    const CheckFold &f = s->ck;
    if (!f.open || !len)
        return fail(APEMOST_HIP_ERR_INVALID, "check_lengths: %s", f.open ? "len is NULL" : "no check_begin");
    for (int k = 0; k < f.n_keep; k++)
        len[k] = f.n_data;
    if (f.d_len) {
        HIP_TRY(hipMemcpyAsync(len, f.d_len, (size_t)f.n_keep * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_check_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    CHECK_HAS_CDF(s, "check_end");
    return fold_reset(s, s->ck);
}

extern "C" int apemost_hip_check_values(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x, const double *x,
                                        const double *y, double *e, double *u, double *T) {
    CHECK_S(s);
    CHECK_HAS_CDF(s, "check_values");
    const int np = s->cfg.n_par;
    if (n < 1 || n_x < 1 || !params || !x || !y || !e || !u || !T || (u64)n * (u64)n_x > ((u64)1 << 26))
        return fail(APEMOST_HIP_ERR_INVALID, "check_values: %d rows x %d data (n_x), or a NULL array among params, x, y, e, "
                    "u and T", n, n_x);
    FoldScratch scratch;
    double *d_par = nullptr, *d_x = nullptr, *d_y = nullptr, *d_e = nullptr, *d_u = nullptr, *d_T = nullptr;
    const size_t nn = (size_t)n * n_x;
    const int rc = [&]() -> int { // (whatever fails, the stream is waited for before the scratch goes)
        FOLD_TRY(fold_alloc(s, scratch, &d_par, (size_t)n * np, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_x, (size_t)n_x, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_y, (size_t)n_x, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_e, nn, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_u, nn, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_T, (size_t)n * kCheckStats, false));
        HIP_TRY(hipMemcpyAsync(d_par, params, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(d_x, x, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(d_y, y, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, s->stream));
        const double inv_sigma = 1.0 / s->sh.consts.sigma;
        with_builtin_model(s->cfg.model, [&](auto m) {
            hipLaunchKernelGGL(check_values_kernel<decltype(m)::value>, dim3((unsigned)n), dim3(kPointwiseWave), 0, s->stream,
                               (const double *)d_par, np, (int)n_x, (const double *)d_x, (const double *)d_y, inv_sigma, d_e,
                               d_u, d_T);
        });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(e, d_e, nn * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(u, d_u, nn * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipMemcpyAsync(T, d_T, (size_t)n * kCheckStats * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        return APEMOST_HIP_OK;
    }();
    const hipError_t sync = hipStreamSynchronize(s->stream);
    FOLD_TRY(rc);
    HIP_TRY(sync);
    return APEMOST_HIP_OK;
}

// ---- the null quantiles (host arithmetic only) ----
namespace {
// ln of x^a e^-x / Gamma(a).  From a = 20 on through Stirling's series, so that the three terms of size a ln a never
// meet: a (ln mu - mu + 1) + ln(a / (2 pi)) / 2 - (1 / (12 a) - 1 / (360 a^3) + 1 / (1260 a^5)), mu = x / a
double gamma_log_prefactor(double a, double x) {
    if (a < 20.0)
        return a * std::log(x) - x - std::lgamma(a);
    const double d = (x - a) / a, a2 = a * a;
    const double corr = 1.0 / (12.0 * a) - 1.0 / (360.0 * a * a2) + 1.0 / (1260.0 * a * a2 * a2);
    return a * (std::log1p(d) - d) + 0.5 * std::log(a / 6.283185307179586476925) - corr;
}

// the regularised lower incomplete gamma function P(a, x), a > 0: the series below a + 1, Lentz's continued fraction
// of Q = 1 - P above
double gamma_p(double a, double x) {
    if (!(x > 0.0))
        return 0.0;
    const double pre = std::exp(gamma_log_prefactor(a, x));
    if (x < a + 1.0) {
        double ap = a, del = 1.0 / a, sum = del;
        for (int it = 0; it < 10000000; it++) {
            ap += 1.0;
            del *= x / ap;
            sum += del;
            if (std::fabs(del) < std::fabs(sum) * 1e-17)
                break;
        }
        return sum * pre;
    }
    const double tiny = 1e-300;
    double b = x + 1.0 - a, c = 1.0 / tiny, d = 1.0 / b, h = d;
    for (int it = 1; it < 10000000; it++) {
        const double an = -(double)it * ((double)it - a);
        b += 2.0;
        d = an * d + b;
        if (std::fabs(d) < tiny)
            d = tiny;
        c = b + an / c;
        if (std::fabs(c) < tiny)
            c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < 1e-16)
            break;
    }
    return 1.0 - pre * h;
}

// the largest x in [lo, hi] with f(x) <= 0 to the last bit; f ascending
template <class F>
double bisect_up(F &&f, double lo, double hi) {
    for (int it = 0; it < 2200; it++) {
        const double mid = 0.5 * (lo + hi);
        if (!(mid > lo && mid < hi))
            break;
        if (f(mid) <= 0.0)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}
} // namespace

extern "C" int apemost_hip_check_null_edges(int32_t model, int32_t stat, int32_t n_data, int32_t n_edges, double *edges) {
    if (model == APEMOST_MODEL_USER)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "check_null_edges: a user-supplied device model has no null law here");
    if (model != APEMOST_MODEL_SIMPLESIN && model != APEMOST_MODEL_SINE3 && model != APEMOST_MODEL_PULSE &&
        model != APEMOST_MODEL_PULSE_VROT)
        return fail(APEMOST_HIP_ERR_INVALID, "check_null_edges: unknown model %d", model);
    if (stat < 0 || stat >= kCheckStats || n_data < 1 || n_edges < 1 || n_edges > kCheckMaxEdges || !edges)
        return fail(APEMOST_HIP_ERR_INVALID, "check_null_edges: stat %d outside [0,%d), n_data %d < 1, n_edges %d outside "
                    "[1,%d], or edges is NULL", stat, kCheckStats, n_data, n_edges, kCheckMaxEdges);
    const bool sine = check_is_sine(model);
    const double L = (double)n_data, parts = (double)(n_edges + 1);
    double floor_ = 0.0; // (the quantiles ascend: each search starts at the one before)
    for (int j = 0; j < n_edges; j++) {
        const double p = (double)(j + 1) / parts;
        double t;
        if (stat == kCheckFit) {
            const double a = sine ? 0.5 * L : L;
            const double x = bisect_up([&](double v) { return gamma_p(a, v) - p; }, floor_, a + 60.0 * std::sqrt(a) + 60.0);
            floor_ = x;
            t = sine ? 2.0 * x : x;
        } else if (stat == kCheckExtreme) {
            const double lp = std::log(p);
            if (sine) {
                t = bisect_up([&](double v) { return L * std::log1p(-std::erfc(v * M_SQRT1_2)) - lp; }, floor_, 60.0);
                floor_ = t;
            } else {
                t = -std::log(-std::expm1(lp / L));
            }
        } else {
            // symmetric about 0 by construction: the upper half from the upper tail, the lower half its mirror
            const int up = j >= n_edges / 2 ? j : n_edges - 1 - j;
            const double q = (double)(n_edges - up) / parts; // the upper tail's mass, <= 1/2
            const double sd = std::sqrt((n_data > 1 ? L - 1.0 : 1.0) / 144.0);
            const double z = 2 * up + 1 == n_edges ? 0.0
                                                   : bisect_up([&](double v) { return q - 0.5 * std::erfc(v * M_SQRT1_2); }, 0.0, 60.0);
            t = (j >= n_edges / 2 ? z : -z) * sd;
        }
        edges[j] = t;
    }
    for (int j = 0; j < n_edges; j++)
        if (!std::isfinite(edges[j]) || (j > 0 && !(edges[j] > edges[j - 1])))
            return fail(APEMOST_HIP_ERR_RUNTIME, "check_null_edges: quantile %d of %d is %g behind %g: the null law of "
                        "%d data does not resolve %d edges in fp64", j + 1, n_edges + 1, edges[j], j > 0 ? edges[j - 1] : 0.0,
                        n_data, n_edges);
    return APEMOST_HIP_OK;
}
