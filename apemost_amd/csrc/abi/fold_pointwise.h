// abi/fold_pointwise.h -- on-device pointwise log-likelihood (pt_pointwise.h) and its tail (pt_pointwise_tail.h), which
// shares the fold's state (PointwiseFold and its PointwiseTailFold; protocol: abi/fold_common.h); the fold begun at the
// caller's data and the joint predictive of every kept chain's block (pt_pointwise_joint.h)
#pragma once

// a built-in model, or a user-supplied one with the pointwise hook
#define POINTWISE_HAS_TERM(s, what)                                                                              \
    do {                                                                                                        \
        if ((s)->cfg.model == APEMOST_MODEL_USER) {                                                             \
            const int rc_hooks = user_analysis(s);                                                              \
            if (rc_hooks != APEMOST_HIP_OK)                                                                     \
                return rc_hooks;                                                                                \
            if (!(s)->ua.has_pointwise)                                                                         \
                return fail(APEMOST_HIP_ERR_UNSUPPORTED,                                                        \
                            what ": this user-supplied device model has no datum's term: it does not define "   \
                                 "the hook apemost_user_pointwise (APEMOST_USER_POINTWISE, "                    \
                                 "include/apemost_device_model.h)");                                            \
        }                                                                                                       \
    } while (0)

constexpr int kPointwiseWords = 8; // origin, sum, sq, m_up, S_up, m_dn, S_dn, S2_dn
constexpr int kPointwiseJointWords = 5; // origin, sum, sq, m, S of a kept chain's block (pt_pointwise_joint.h)

static double pointwise_c(const apemost_hip_sampler *s) {
    const double sigma = s->sh.consts.sigma;
    const double t = -2.0 * sigma;
    const double denom = t * sigma;
    return 1.0 / denom;
}

// What pointwise_begin and pointwise_begin_at share.  at == nullptr: every kept chain is scored on columns 0 and 1 of its
// own ladder's data; else on the caller's, at->n_at[k] data per kept chain.  The checks of the caller's arguments have
// been made.
static int pointwise_open(apemost_hip_sampler *s, const char *what, const apemost_hip_pointwise_config *cfg,
                          const apemost_hip_pointwise_at *at) {
    const int np = s->cfg.n_par;
    // the longest data among the kept chains (a batch's ladders, or the caller's blocks, may differ in length: the
    // arrays stay rectangular and every kept chain folds its own len[k] <= nd series)
    std::vector<int> len;
    bool ragged = false;
    int nd = 0;
    if (at) {
        len.assign(at->n_at, at->n_at + cfg->n_keep);
        for (int k = 0; k < cfg->n_keep; k++) {
            nd = len[k] > nd ? len[k] : nd;
            ragged = ragged || len[k] != len[0];
        }
    } else
        nd = kept_lengths(s, cfg->n_keep, cfg->chains, len, &ragged);
    const u64 n_series = (u64)cfg->n_keep * (u64)nd;
    if (n_series > ((u64)1 << 20))
        return fail(APEMOST_HIP_ERR_INVALID, "%s: %d chains x %d data: more than 2^20 series", what, cfg->n_keep, nd);
    if (np > kPointwiseTile)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: %d parameters, more than %d", what, np, kPointwiseTile);
    FOLD_TRY(fold_reset(s, s->pw));
    PointwiseFold &f = s->pw;
    f.n_keep = cfg->n_keep;
    f.n_data = nd;
    f.c = pointwise_c(s);
    f.n = 0;
    const size_t ns = (size_t)n_series, nk = (size_t)cfg->n_keep;
    const bool user = s->cfg.model == APEMOST_MODEL_USER;
    const size_t nc = user ? (size_t)s->cfg.n_cols : 1; // a user model's data: all of its columns, in d_x
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_chains, nk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_x, ns * nc, false));
    if (!user)
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_y, ns, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_state, kPointwiseWords * ns, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_par, 2 * nk * np, true));
    HIP_TRY(hipMemcpyAsync(f.d_chains, cfg->chains, nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    if (ragged) {
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_len, nk, false));
        HIP_TRY(hipMemcpyAsync(f.d_len, len.data(), nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    }
    if (at && at->joint) {
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_joint, kPointwiseJointWords * nk, true));
        FOLD_TRY(fold_alloc(s, f.mem, &f.d_J, nk * kPointwisePiece, false));
    }
    size_t packed = 0; // where kept chain k's block starts in the caller's arrays
    for (int k = 0; k < cfg->n_keep; k++) {
        const size_t mine = (size_t)len[k];
        if (at) { // (a built-in model: begin_at refuses a user-supplied one)
            HIP_TRY(hipMemcpyAsync(f.d_x + (size_t)k * nd, at->x + packed, mine * sizeof(double), hipMemcpyHostToDevice,
                                   s->stream));
            HIP_TRY(hipMemcpyAsync(f.d_y + (size_t)k * nd, at->y + packed, mine * sizeof(double), hipMemcpyHostToDevice,
                                   s->stream));
            packed += mine;
            continue;
        }
        // columns 0 and 1 of the kept chain's own ladder (the data is stored by columns, ladder after ladder), in
        // that ladder's own length (a user model, which no batch runs: len[k] = nd)
        const double *col0 = ladder_data(s, s->batch ? cfg->chains[k] / s->per_ladder : 0);
        HIP_TRY(hipMemcpyAsync(f.d_x + (size_t)k * nc * nd, col0, nc * mine * sizeof(double), hipMemcpyDeviceToDevice,
                               s->stream));
        if (!user)
            HIP_TRY(hipMemcpyAsync(f.d_y + (size_t)k * nd, col0 + mine, mine * sizeof(double),
                                   hipMemcpyDeviceToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's arrays are read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_begin(apemost_hip_sampler *s, const apemost_hip_pointwise_config *cfg) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_begin");
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin: config is NULL");
    FOLD_TRY(fold_check_chains(s, "pointwise", cfg->n_keep, cfg->chains));
    return pointwise_open(s, "pointwise_begin", cfg, nullptr);
}

// the fold begun at the caller's data: held-out data that the sampler was not fitted to
extern "C" int apemost_hip_pointwise_begin_at(apemost_hip_sampler *s, const apemost_hip_pointwise_config *cfg,
                                              const apemost_hip_pointwise_at *at) {
    CHECK_S(s);
    if (s->cfg.model == APEMOST_MODEL_USER)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "pointwise_begin_at: a user-supplied device model: its datum is a whole "
                    "row of the sampler's data and it runs in no batch; the hook on held-out rows is a follow-up");
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin_at: config is NULL");
    if (!at)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin_at: at is NULL");
    FOLD_TRY(fold_check_chains(s, "pointwise", cfg->n_keep, cfg->chains));
    if (!at->n_at || !at->x || !at->y)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin_at: at->%s is NULL", !at->n_at ? "n_at" : !at->x ? "x" : "y");
    if (at->joint != 0 && at->joint != 1)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin_at: at->joint = %d: 0 or 1", at->joint);
    for (int k = 0; k < cfg->n_keep; k++)
        if (at->n_at[k] < 1)
            return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin_at: at->n_at[%d] = %d: every kept chain is scored on at "
                        "least one datum", k, at->n_at[k]);
    return pointwise_open(s, "pointwise_begin_at", cfg, at);
}

// ---- the tail of the pointwise fold (pt_pointwise_tail.h) ----
static PointwiseTailArgs pointwise_tail_args(const apemost_hip_sampler *s, bool force) {
    PointwiseTailArgs t;
    t.buf = s->pw.tail.d_buf;
    t.slots = s->pw.tail.d_slots;
    t.thr = s->pw.tail.d_thr;
    t.capacity = s->pw.tail.capacity;
    t.B = s->pw.tail.B;
    t.n_data = s->pw.n_data;
    t.n_blocks = (s->pw.n_data + kPointwiseWave - 1) / kPointwiseWave;
    t.force = force ? 1 : 0;
    t.dense = nullptr;
    t.count = nullptr;
    return t;
}

static int pointwise_tail_compact(apemost_hip_sampler *s, bool force) {
    const PointwiseTailArgs t = pointwise_tail_args(s, force);
    const dim3 grid((unsigned)s->pw.n_keep * (unsigned)s->pw.n_data), block(kTailThreads);
    hipLaunchKernelGGL(pointwise_tail_compact_kernel, grid, block, (size_t)t.B * sizeof(unsigned long long), s->copy_stream, t);
    HIP_TRY(hipGetLastError());
    return APEMOST_HIP_OK;
}

// the kept steps of the fold piece `fold` (already launched), in tail pieces: append, then compact, on copy_stream
static int pointwise_tail_pieces(apemost_hip_sampler *s, const PointwiseArgs &fold) {
    const PointwiseTailArgs t = pointwise_tail_args(s, false);
    const unsigned int piece = (unsigned int)tail_piece(t.capacity);
    for (unsigned int k0 = 0; k0 < fold.n; k0 += piece) {
        PointwiseArgs a = fold;
        a.skip = fold.skip + (u64)k0 * fold.thin;
        a.n = fold.n - k0 < piece ? fold.n - k0 : piece;
        a.n0 = fold.n0 + k0;
        const dim3 grid((unsigned)a.n_blocks * (unsigned)a.n_keep), block(kPointwiseWave);
        PointwiseTailArgs tt = t;
        if (s->cfg.model == APEMOST_MODEL_USER) {
            void *params[] = {&a, &tt};
            HIP_TRY(user_launch(s->ua.pointwise_tail_append, grid.x, block.x, 0, s->copy_stream, params));
        } else {
            with_builtin_model(s->cfg.model, [&](auto m) {
                hipLaunchKernelGGL(pointwise_tail_append_kernel<decltype(m)::value>, grid, block, 0, s->copy_stream, a, tt);
            });
        }
        HIP_TRY(hipGetLastError());
        FOLD_TRY(pointwise_tail_compact(s, false));
    }
    return APEMOST_HIP_OK;
}

// ---- the joint predictive of the kept chains' blocks (pt_pointwise_joint.h) ----
static PointwiseJointArgs pointwise_joint_args(const apemost_hip_sampler *s) {
    const PointwiseFold &f = s->pw;
    const size_t nk = (size_t)f.n_keep;
    PointwiseJointArgs q;
    q.J = f.d_J;
    q.origin = f.d_joint;
    q.sum = f.d_joint + nk;
    q.sq = f.d_joint + 2 * nk;
    q.m = f.d_joint + 3 * nk;
    q.S = f.d_joint + 4 * nk;
    return q;
}

// the kept steps of the fold piece `fold` (already launched): J of every kept sample, then the fold of them in sample
// order, on copy_stream (a built-in model: begin_at refuses a user-supplied one)
static int pointwise_joint_piece(apemost_hip_sampler *s, const PointwiseArgs &fold) {
    const PointwiseJointArgs q = pointwise_joint_args(s);
    const unsigned int rows = (unsigned int)joint_rows(fold.n_par);
    const dim3 grid((unsigned)fold.n_keep, (fold.n + rows - 1) / rows), block(kPointwiseWave);
    with_builtin_model(s->cfg.model, [&](auto m) {
        hipLaunchKernelGGL(pointwise_joint_sum_kernel<decltype(m)::value>, grid, block, 0, s->copy_stream, fold, q);
    });
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(pointwise_joint_fold_kernel, dim3((unsigned)fold.n_keep), block, 0, s->copy_stream, q, fold.n,
                       fold.n0 == 0 ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                                uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_accumulate");
    PointwiseFold &f = s->pw;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("pointwise", f.open, d_samples, n_steps, skip, thin, &kept));
    if (f.tail.awaits_set)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_accumulate: the tail was begun on a fold of %llu samples that "
                    "pointwise_set loaded: pointwise_tail_set must load the tail of those samples first",
                    (unsigned long long)f.n);
    if (f.joint_awaits_set)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_accumulate: the fold keeps the joint predictive of its blocks and "
                    "pointwise_set loaded %llu samples: pointwise_joint_set must load the joint state of those samples "
                    "first", (unsigned long long)f.n);
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const size_t ns = (size_t)f.n_keep * f.n_data;
    for (u64 k0 = 0; k0 < kept; k0 += kPointwisePiece) {
        PointwiseArgs a;
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
        a.len = f.d_len;
        a.x = f.d_x;
        a.y = f.d_y;
        a.c = f.c;
        a.n_cols = s->cfg.n_cols;
        a.sigma = s->sh.consts.sigma;
        a.hmin = s->sh.consts.hmin;
        a.origin = f.d_state;
        a.sum = f.d_state + ns;
        a.sq = f.d_state + 2 * ns;
        a.m_up = f.d_state + 3 * ns;
        a.S_up = f.d_state + 4 * ns;
        a.m_dn = f.d_state + 5 * ns;
        a.S_dn = f.d_state + 6 * ns;
        a.S2_dn = f.d_state + 7 * ns;
        a.par_origin = f.d_par;
        a.par_sum = f.d_par + (size_t)f.n_keep * s->cfg.n_par;
        const dim3 grid((unsigned)(a.n_blocks + 1) * (unsigned)a.n_keep), block(kPointwiseWave);
        if (s->cfg.model == APEMOST_MODEL_USER) {
            void *params[] = {&a};
            HIP_TRY(user_launch(s->ua.pointwise_fold, grid.x, block.x, 0, s->copy_stream, params));
        } else {
            with_builtin_model(s->cfg.model, [&](auto m) {
                hipLaunchKernelGGL(pointwise_fold_kernel<decltype(m)::value>, grid, block, 0, s->copy_stream, a);
            });
        }
        HIP_TRY(hipGetLastError());
        if (f.tail.capacity > 0)
            FOLD_TRY(pointwise_tail_pieces(s, a));
        if (f.d_joint)
            FOLD_TRY(pointwise_joint_piece(s, a));
        f.n += a.n;
        f.n_set = false;
    }
    return APEMOST_HIP_OK;
}

static int pointwise_xfer(apemost_hip_sampler *s, const apemost_hip_pointwise_view *v, bool up) {
    PointwiseFold &f = s->pw;
    FOLD_TRY(fold_xfer_check("pointwise", f.open, v, up));
    const size_t nk = (size_t)f.n_keep, ns = nk * f.n_data, np = (size_t)s->cfg.n_par;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    double *const host[kPointwiseWords] = {v->origin, v->sum, v->sq, v->m_up, v->S_up, v->m_dn, v->S_dn, v->S2_dn};
    for (int q = 0; q < kPointwiseWords; q++)
        FOLD_TRY(copy(f.d_state + (size_t)q * ns, host[q], ns * sizeof(double)));
    FOLD_TRY(copy(f.d_par, v->par_origin, nk * np * sizeof(double)));
    FOLD_TRY(copy(f.d_par + nk * np, v->par_sum, nk * np * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    if (up && v->n)
        f.n_set = true;
    if (up && v->n && f.d_joint) // (the tail's awaits_set rule: the joint state of the loaded samples comes next)
        f.joint_awaits_set = f.n > 0;
    return APEMOST_HIP_OK;
}

static int pointwise_joint_xfer(apemost_hip_sampler *s, const apemost_hip_pointwise_joint_view *v, bool up) {
    CHECK_S(s);
    PointwiseFold &f = s->pw;
    const char *what = up ? "set" : "get";
    if (!f.open || !f.d_joint)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_joint_%s: no pointwise_begin_at with joint = 1", what);
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_joint view is NULL");
    if (up && v->n && *v->n != f.n)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_joint_set: the view holds %llu samples, the fold %llu: "
                    "pointwise_set loads the fold's samples first", (unsigned long long)*v->n, (unsigned long long)f.n);
    const size_t nk = (size_t)f.n_keep;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    double *const host[kPointwiseJointWords] = {v->origin, v->sum, v->sq, v->m, v->S};
    for (int q = 0; q < kPointwiseJointWords; q++)
        FOLD_TRY(copy(f.d_joint + (size_t)q * nk, host[q], nk * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    if (!up && v->n)
        *v->n = f.n;
    if (up)
        f.joint_awaits_set = false;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_joint_get(apemost_hip_sampler *s, const apemost_hip_pointwise_joint_view *v) {
    return pointwise_joint_xfer(s, v, false);
}

extern "C" int apemost_hip_pointwise_joint_set(apemost_hip_sampler *s, const apemost_hip_pointwise_joint_view *v) {
    return pointwise_joint_xfer(s, v, true);
}

extern "C" int apemost_hip_pointwise_get(apemost_hip_sampler *s, const apemost_hip_pointwise_view *v) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_get");
    return pointwise_xfer(s, v, false);
}

extern "C" int apemost_hip_pointwise_set(apemost_hip_sampler *s, const apemost_hip_pointwise_view *v) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_set");
    return pointwise_xfer(s, v, true);
}

extern "C" int apemost_hip_pointwise_lengths(apemost_hip_sampler *s, int32_t *len) {
    CHECK_S(s);
    const PointwiseFold &f = s->pw;
    if (!f.open || !len)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_lengths: %s", f.open ? "len is NULL" : "no pointwise_begin");
    for (int k = 0; k < f.n_keep; k++)
        len[k] = f.n_data;
    if (f.d_len) {
        HIP_TRY(hipMemcpyAsync(len, f.d_len, (size_t)f.n_keep * sizeof(int), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_end");
    return fold_reset(s, s->pw);
}

// padded series (64 per block of data) times the slots of a series' buffer
static u64 pointwise_tail_slots(const apemost_hip_sampler *s, int B) {
    const u64 n_blocks = ((u64)s->pw.n_data + kPointwiseWave - 1) / kPointwiseWave;
    return (u64)s->pw.n_keep * n_blocks * kPointwiseWave * (u64)B;
}

extern "C" int apemost_hip_pointwise_tail_begin(apemost_hip_sampler *s, int32_t capacity) {
    if (!s)
        return fail(APEMOST_HIP_ERR_INVALID, "sampler is NULL");
    if (capacity < 2 || capacity > kTailMaxCapacity)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: capacity %d outside [2,%d]", capacity, kTailMaxCapacity);
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_tail_begin");
    PointwiseFold &f = s->pw;
    if (!f.open)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: no pointwise_begin");
    if (f.d_len)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "pointwise_tail_begin: the kept chains' ladders differ in n_data: the tail "
                    "of a ragged batch is a follow-up; keep chains of ladders of one length, or one fold per length");
    if (f.n > 0 && !f.n_set)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: the fold has accumulated %llu samples whose tail is "
                    "lost: begin the tail before the first accumulate, or right behind pointwise_set",
                    (unsigned long long)f.n);
    const u64 limit = (u64)1 << 28;
    const int B = tail_buffer(capacity);
    if (pointwise_tail_slots(s, B) > limit) {
        int fits = 0; // the largest capacity whose buffers fit
        for (int b = kTailMaxB; b >= 2 * kTailMinP && !fits; b >>= 1)
            if (pointwise_tail_slots(s, b) <= limit)
                fits = b / 2;
        if (fits)
            return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: %d chains x %d data (in blocks of 64) x %d slots "
                        "for capacity %d: more than 2^28 slots (2 GiB); the largest capacity that fits is %d",
                        f.n_keep, f.n_data, B, capacity, fits);
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: %d chains x %d data (in blocks of 64) x %d slots for "
                    "capacity %d: more than 2^28 slots (2 GiB); the largest capacity that fits is 0: no capacity fits, "
                    "keep fewer chains", f.n_keep, f.n_data, B, capacity);
    }
    FOLD_TRY(fold_reset(s, f.tail));
    PointwiseTailFold &t = f.tail;
    const size_t ns = (size_t)f.n_keep * f.n_data;
    const int rc = [&]() -> int {
        FOLD_TRY(fold_alloc(s, t.mem, &t.d_buf, (size_t)pointwise_tail_slots(s, B), false));
        FOLD_TRY(fold_alloc(s, t.mem, &t.d_slots, ns, true));
        FOLD_TRY(fold_alloc(s, t.mem, &t.d_thr, ns, true));
        HIP_TRY(hipStreamSynchronize(s->stream));
        return APEMOST_HIP_OK;
    }();
    if (rc != APEMOST_HIP_OK) { // the fold stays as it was, without a tail
        fold_free(t);
        return rc;
    }
    t.capacity = capacity;
    t.B = B;
    t.awaits_set = f.n > 0;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_tail_capacity(apemost_hip_sampler *s, int32_t *capacity) {
    if (!s)
        return fail(APEMOST_HIP_ERR_INVALID, "sampler is NULL");
    if (!capacity)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_capacity: capacity is NULL");
    *capacity = s->pw.open ? s->pw.tail.capacity : 0;
    return APEMOST_HIP_OK;
}

// A tail's view holds dense arrays, which a scatter or gather kernel takes to or from the buffers: its xfer shares
// the stream order with the other folds', not the copies.
static int pointwise_tail_xfer(apemost_hip_sampler *s, const apemost_hip_pointwise_tail_view *v, bool up) {
    CHECK_S(s);
    const char *what = up ? "set" : "get";
    if (!s->pw.open || s->pw.tail.capacity == 0)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_%s: no pointwise_tail_begin", what);
    if (!v || !v->count || !v->values)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_%s: the view or one of its arrays is NULL", what);
    const size_t ns = (size_t)s->pw.n_keep * s->pw.n_data, cap = (size_t)s->pw.tail.capacity;
    if (up)
        for (size_t q = 0; q < ns; q++) {
            if (v->count[q] > cap)
                return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_set: count[%zu] = %llu, more than the capacity %zu", q,
                            (unsigned long long)v->count[q], cap);
            for (size_t j = 0; j < (size_t)v->count[q]; j++)
                if (v->values[q * cap + j] != v->values[q * cap + j])
                    return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_set: values[%zu][%zu] is NaN: a tail holds none", q, j);
        }
    FOLD_TRY(fold_order_behind_stream(s));
    PointwiseTailArgs t = pointwise_tail_args(s, true);
    FoldScratch scratch;
    const int rc = [&]() -> int { // (whatever fails, the stream is waited for before the scratch goes)
        FOLD_TRY(fold_alloc(s, scratch, &t.dense, ns * cap, false));
        FOLD_TRY(fold_alloc(s, scratch, &t.count, ns, false));
        const dim3 grid((unsigned)ns, (unsigned)((cap + kTailThreads - 1) / kTailThreads)), block(kTailThreads);
        if (up) {
            HIP_TRY(hipMemcpyAsync(t.dense, v->values, ns * cap * sizeof(double), hipMemcpyHostToDevice, s->copy_stream));
            HIP_TRY(hipMemcpyAsync(t.count, v->count, ns * sizeof(unsigned long long), hipMemcpyHostToDevice, s->copy_stream));
            hipLaunchKernelGGL(pointwise_tail_scatter_kernel, grid, block, 0, s->copy_stream, t);
            HIP_TRY(hipGetLastError());
            FOLD_TRY(pointwise_tail_compact(s, true)); // sorts what was loaded and sets every threshold from it
        } else {
            FOLD_TRY(pointwise_tail_compact(s, true));
            hipLaunchKernelGGL(pointwise_tail_gather_kernel, grid, block, 0, s->copy_stream, t);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(v->values, t.dense, ns * cap * sizeof(double), hipMemcpyDeviceToHost, s->copy_stream));
            HIP_TRY(hipMemcpyAsync(v->count, t.count, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->copy_stream));
        }
        return APEMOST_HIP_OK;
    }();
    const hipError_t sync = hipStreamSynchronize(s->copy_stream);
    FOLD_TRY(rc);
    HIP_TRY(sync);
    if (up)
        s->pw.tail.awaits_set = false;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_tail_get(apemost_hip_sampler *s, const apemost_hip_pointwise_tail_view *v) {
    return pointwise_tail_xfer(s, v, false);
}

extern "C" int apemost_hip_pointwise_tail_set(apemost_hip_sampler *s, const apemost_hip_pointwise_tail_view *v) {
    return pointwise_tail_xfer(s, v, true);
}

// the term of every datum of ladder `ladder` under n parameter rows, by the fold's own function: no fold need be open
extern "C" int apemost_hip_pointwise_loglike_ladder(apemost_hip_sampler *s, int32_t ladder, int32_t n,
                                                    const double *params, double *out) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_loglike");
    const int np = s->cfg.n_par;
    if (ladder < 0 || ladder >= (s->batch ? s->n_ladders : 1))
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_loglike: ladder %d outside [0,%d)", ladder,
                    s->batch ? s->n_ladders : 1);
    const int nd = ladder_len(s, ladder);
    if (n < 1 || !params || !out || (u64)n * (u64)nd > ((u64)1 << 26))
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_loglike: %d rows x %d data, or a NULL array", n, nd);
    FoldScratch scratch;
    double *d_par = nullptr, *d_out = nullptr;
    const int rc = [&]() -> int { // (whatever fails, the stream is waited for before the scratch goes)
        FOLD_TRY(fold_alloc(s, scratch, &d_par, (size_t)n * np, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_out, (size_t)n * nd, false));
        HIP_TRY(hipMemcpyAsync(d_par, params, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, s->stream));
        const dim3 grid((unsigned)((nd + kPointwiseWave - 1) / kPointwiseWave) * (unsigned)n), block(kPointwiseWave);
        // the ladder's columns 0 and 1 (the data is stored by columns, ladder after ladder)
        const double *x = ladder_data(s, ladder), *y = x + nd;
        const double c = pointwise_c(s);
        if (s->cfg.model == APEMOST_MODEL_USER) { // all n_cols columns of the ladder's rows
            int np_ = np, nd_ = nd, nc = s->cfg.n_cols;
            double sigma = s->sh.consts.sigma, hmin = s->sh.consts.hmin;
            void *params_[] = {&d_par, &np_, &nd_, &nc, &x, &sigma, &hmin, &d_out};
            HIP_TRY(user_launch(s->ua.pointwise_loglike, grid.x, block.x, 0, s->stream, params_));
        } else {
            with_builtin_model(s->cfg.model, [&](auto m) {
                hipLaunchKernelGGL(pointwise_loglike_kernel<decltype(m)::value>, grid, block, 0, s->stream, d_par, np, nd, x,
                                   y, c, d_out);
            });
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * nd * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        return APEMOST_HIP_OK;
    }();
    const hipError_t sync = hipStreamSynchronize(s->stream);
    FOLD_TRY(rc);
    HIP_TRY(sync);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_loglike(apemost_hip_sampler *s, int32_t n, const double *params, double *out) {
    return apemost_hip_pointwise_loglike_ladder(s, 0, n, params, out);
}

// the term of the caller's n_x data under n parameter rows, by the fold's own function: what a fold begun with
// pointwise_begin_at folds; no fold need be open, and nothing of the sampler's data is read
extern "C" int apemost_hip_pointwise_loglike_at(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x,
                                                const double *x, const double *y, double *out) {
    CHECK_S(s);
    if (s->cfg.model == APEMOST_MODEL_USER)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "pointwise_loglike_at: a user-supplied device model: its datum is a "
                    "whole row of the sampler's data; the hook on held-out rows is a follow-up");
    const int np = s->cfg.n_par;
    if (n < 1 || n_x < 1 || !params || !x || !y || !out || (u64)n * (u64)n_x > ((u64)1 << 26))
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_loglike_at: %d rows x %d data (n_x), or a NULL array among "
                    "params, x, y and out", n, n_x);
    FoldScratch scratch;
    double *d_par = nullptr, *d_x = nullptr, *d_y = nullptr, *d_out = nullptr;
    const int rc = [&]() -> int { // (whatever fails, the stream is waited for before the scratch goes)
        FOLD_TRY(fold_alloc(s, scratch, &d_par, (size_t)n * np, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_x, (size_t)n_x, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_y, (size_t)n_x, false));
        FOLD_TRY(fold_alloc(s, scratch, &d_out, (size_t)n * n_x, false));
        HIP_TRY(hipMemcpyAsync(d_par, params, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(d_x, x, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(d_y, y, (size_t)n_x * sizeof(double), hipMemcpyHostToDevice, s->stream));
        const dim3 grid((unsigned)((n_x + kPointwiseWave - 1) / kPointwiseWave) * (unsigned)n), block(kPointwiseWave);
        const double c = pointwise_c(s);
        with_builtin_model(s->cfg.model, [&](auto m) {
            hipLaunchKernelGGL(pointwise_loglike_kernel<decltype(m)::value>, grid, block, 0, s->stream, d_par, np,
                               (int)n_x, (const double *)d_x, (const double *)d_y, c, d_out);
        });
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * n_x * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        return APEMOST_HIP_OK;
    }();
    const hipError_t sync = hipStreamSynchronize(s->stream);
    FOLD_TRY(rc);
    HIP_TRY(sync);
    return APEMOST_HIP_OK;
}
