// abi/fold_common.h -- the protocol every on-device fold follows, written once.  A fold is begun
// (apemost_hip_<fold>_begin: checks, then its device memory), accumulates kept steps of sample rows on copy_stream
// behind the stepping stream, is read or loaded through a view (get / set) and ended.  What is particular to a
// fold -- its own checks, how its kernels' arguments are filled and launched, which arrays its view copies -- is in
// abi/fold_<fold>.h; its state is in abi/sampler.h.  A part of apemost_hip.hip.
#pragma once

#define FOLD_TRY(call)                                                                           \
    do {                                                                                         \
        const int rc__ = (call);                                                                 \
        if (rc__ != APEMOST_HIP_OK)                                                              \
            return rc__;                                                                         \
    } while (0)

// ---- memory ----
// `count` elements (at least one) owned by the fold from here on, whatever fails next: a begin that fails halfway
// leaves them to the next begin, end or release.  zeroed: cleared on the sampler's stream.
template <class T>
static int fold_alloc(apemost_hip_sampler *s, FoldMem &mem, T **p, size_t count, bool zeroed) {
    const size_t bytes = (count > 0 ? count : 1) * sizeof(T);
    void *q = nullptr;
    if (mem.n_owned == kFoldMaxOwned)
        return fail(APEMOST_HIP_ERR_RUNTIME, "fold_alloc: more than kFoldMaxOwned = %d device arrays", kFoldMaxOwned);
    HIP_TRY(hipMalloc(&q, bytes));
    mem.owned[mem.n_owned++] = q;
    *p = (T *)q;
    if (zeroed)
        HIP_TRY(hipMemsetAsync(q, 0, bytes, s->stream));
    return APEMOST_HIP_OK;
}

// what every begin does once its checks have passed, and all an end does: the fold begun before may still be
// accumulating on copy_stream
template <class Fold>
static int fold_reset(apemost_hip_sampler *s, Fold &f) {
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    fold_free(f);
    return APEMOST_HIP_OK;
}

// ---- stream order ----
static int ensure_copy_stream(apemost_hip_sampler *s) {
    if (!s->copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s->ev_copy, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc((void **)&s->h_word, sizeof(u64), hipHostMallocDefault));
        *s->h_word = 0;
    }
    return APEMOST_HIP_OK;
}

// what is queued on copy_stream next runs behind everything launched so far on the sampler's stream, and behind
// every accumulate queued so far; launches issued after it overlap with it
static int fold_order_behind_stream(apemost_hip_sampler *s) {
    FOLD_TRY(ensure_copy_stream(s));
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    return APEMOST_HIP_OK;
}

// ---- accumulate ----
static u64 kept_steps(u64 n_steps, u64 skip, u64 thin) { return skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0; }

// The head of apemost_hip_<fold>_accumulate.  The fold's own checks follow it, then the return on *kept == 0, then
// fold_order_behind_stream and the launches: apemost_hip_samples_wait or the fold's get waits for them, and the
// caller does one of the two before d_samples is written again.
static int fold_accumulate_check(const char *fold, bool open, const double *d_samples, u64 n_steps, u64 skip, u64 thin,
                                 u64 *kept) {
    if (!open)
        return fail(APEMOST_HIP_ERR_INVALID, "%s_accumulate: no %s_begin", fold, fold);
    if (thin < 1 || (!d_samples && n_steps > 0))
        return fail(APEMOST_HIP_ERR_INVALID, "%s_accumulate: bad arguments", fold);
    *kept = kept_steps(n_steps, skip, thin);
    return APEMOST_HIP_OK;
}

// ---- get and set through a view ----
// The head of <fold>_xfer; fold_order_behind_stream, the copies and fold_xfer_wait follow.
static int fold_xfer_check(const char *fold, bool open, const void *view, bool up) {
    if (!open)
        return fail(APEMOST_HIP_ERR_INVALID, "%s_%s: no %s_begin", fold, up ? "set" : "get", fold);
    if (!view)
        return fail(APEMOST_HIP_ERR_INVALID, "%s view is NULL", fold);
    return APEMOST_HIP_OK;
}

// one array of a view, up (set) or down (get), on copy_stream; an array the view leaves NULL is skipped
namespace {
struct FoldCopy {
    apemost_hip_sampler *s;
    bool up;
    int operator()(void *dev, void *host, size_t bytes) const {
        if (host && bytes > 0)
            HIP_TRY(up ? hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, s->copy_stream)
                       : hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, s->copy_stream));
        return APEMOST_HIP_OK;
    }
};
} // namespace

static int fold_xfer_wait(apemost_hip_sampler *s) {
    HIP_TRY(hipStreamSynchronize(s->copy_stream));
    return APEMOST_HIP_OK;
}

// the count of kept samples goes the way the arrays went
static void fold_xfer_count(u64 &n, uint64_t *view_n, bool up) {
    if (!view_n)
        return;
    if (up)
        n = *view_n;
    else
        *view_n = n;
}

// ---- checks that several folds share ----
// the kept chains of a begin; max_columns > 0: also a bound on n_keep x n_par
static int fold_check_chains(const apemost_hip_sampler *s, const char *fold, int n_keep, const int32_t *chains,
                             long long max_columns = 0) {
    if (n_keep < 1 || n_keep > s->cfg.n_chains || !chains)
        return fail(APEMOST_HIP_ERR_INVALID, "%s_begin: n_keep %d outside [1,%d], or no chains", fold, n_keep,
                    s->cfg.n_chains);
    if (max_columns > 0 && (long long)n_keep * s->cfg.n_par > max_columns)
        return fail(APEMOST_HIP_ERR_INVALID, "%s_begin: %d chains of %d parameters are more than %lld columns", fold,
                    n_keep, s->cfg.n_par, max_columns);
    for (int k = 0; k < n_keep; k++)
        if (chains[k] < 0 || chains[k] >= s->cfg.n_chains || (k > 0 && chains[k] <= chains[k - 1]))
            return fail(APEMOST_HIP_ERR_INVALID,
                        "%s_begin: chains[%d] = %d: local chain indices in [0,%d), strictly increasing", fold, k, chains[k],
                        s->cfg.n_chains);
    return APEMOST_HIP_OK;
}

// the histogram range [lo[p], hi[p]] of every parameter
static int fold_check_ranges(const char *fold, int n_par, const double *lo, const double *hi) {
    for (int p = 0; p < n_par; p++)
        if (!std::isfinite(lo[p]) || !std::isfinite(hi[p]) || !(lo[p] < hi[p]) ||
            !std::isfinite(hi[p] - lo[p])) // (a width that overflows: the bin guess divides by it)
            return fail(APEMOST_HIP_ERR_INVALID, "%s_begin: parameter %d: range [%g, %g] invalid", fold, p, lo[p], hi[p]);
    return APEMOST_HIP_OK;
}

// kept steps staged per launch: about `budget` values over all `columns`, at least 256 and at most 2^log2_max
static u64 fold_chunk(u64 budget, u64 columns, int log2_max) {
    const u64 chunk = budget / columns, most = (u64)1 << log2_max;
    return chunk < 256 ? 256 : chunk > most ? most : chunk;
}

// batches of batch_means_error() closed after n samples: sample n (counted from 1) closes one when
// n % bs == bs - 1 -- for bs >= 2 the first batch holds bs - 1 samples, every later one bs
static u64 batches_closed(u64 n, u64 bs) { return bs == 1 ? n : (n + 1) / bs; }
// samples still to come before the batch that is open after n samples closes (1 .. bs)
static u64 batches_left(u64 n, u64 bs) {
    const u64 m = (bs - (n + 1) % bs) % bs;
    return m == 0 ? bs : m;
}

// an accumulate of `kept` samples more stays within the batches the fold has room for
static int fold_check_batches(const char *fold, u64 n, u64 kept, u64 bs, u64 max_batches) {
    if (batches_closed(n + kept, bs) > max_batches)
        return fail(APEMOST_HIP_ERR_INVALID, "%s_accumulate: %llu samples would close batch %llu, beyond max_batches = %llu",
                    fold, (unsigned long long)(n + kept), (unsigned long long)batches_closed(n + kept, bs),
                    (unsigned long long)max_batches);
    return APEMOST_HIP_OK;
}

// ---- kernels that are templates over the model ----
// f(std::integral_constant<int, M>) for the built-in model M of a sampler; a user-supplied model never comes here, its
// kernels are functions of a run-time module (user_launch)
template <class F>
static void with_builtin_model(int model, F &&f) {
    switch (model) {
    case APEMOST_MODEL_SIMPLESIN: f(std::integral_constant<int, APEMOST_MODEL_SIMPLESIN>()); break;
    case APEMOST_MODEL_SINE3: f(std::integral_constant<int, APEMOST_MODEL_SINE3>()); break;
    case APEMOST_MODEL_PULSE: f(std::integral_constant<int, APEMOST_MODEL_PULSE>()); break;
    default: f(std::integral_constant<int, APEMOST_MODEL_PULSE_VROT>()); break;
    }
}

static hipError_t user_launch(hipFunction_t f, unsigned grid, unsigned block, size_t lds, hipStream_t stream, void **params) {
    return hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, (unsigned)lds, stream, params, nullptr);
}
