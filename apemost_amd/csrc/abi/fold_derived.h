// abi/fold_derived.h -- on-device derived quantities (pt_derived.h; state: DerivedFold, protocol: abi/fold_common.h)
#pragma once

// values an opcode takes from the stack and values it leaves (-1: no such opcode)
static void derived_effect(int op, int *pops, int *pushes) {
    switch (op) {
    case APEMOST_DERIVED_COL:
    case APEMOST_DERIVED_CONST: *pops = 0, *pushes = 1; break;
    case APEMOST_DERIVED_DUP: *pops = 1, *pushes = 2; break;
    case APEMOST_DERIVED_SWAP: *pops = 2, *pushes = 2; break;
    case APEMOST_DERIVED_ADD:
    case APEMOST_DERIVED_SUB:
    case APEMOST_DERIVED_MUL:
    case APEMOST_DERIVED_DIV:
    case APEMOST_DERIVED_MIN:
    case APEMOST_DERIVED_MAX:
    case APEMOST_DERIVED_ATAN2: *pops = 2, *pushes = 1; break;
    case APEMOST_DERIVED_NEG:
    case APEMOST_DERIVED_ABS:
    case APEMOST_DERIVED_INV:
    case APEMOST_DERIVED_SQRT:
    case APEMOST_DERIVED_FLOOR:
    case APEMOST_DERIVED_LOG:
    case APEMOST_DERIVED_EXP:
    case APEMOST_DERIVED_SIN:
    case APEMOST_DERIVED_COS: *pops = 1, *pushes = 1; break;
    default: *pops = *pushes = -1; break;
    }
}

// `who`: the entry point the message names
static int derived_check_programs(const char *who, int n_par, int n_col, const int32_t *code, const int32_t *start,
                                  int n_const, int32_t *depth_out) {
    if (n_col < 1 || n_col > kDerivedMaxCols)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: %d columns outside [1,%d]", who, n_col, kDerivedMaxCols);
    if (n_par < 0 || !code || !start)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: n_par %d, or no code or no start", who, n_par);
    if (n_const < 0 || n_const > kDerivedMaxConsts)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: %d constants outside [0,%d]", who, n_const, kDerivedMaxConsts);
    if (start[0] != 0)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: start[0] = %d, not 0", who, start[0]);
    for (int c = 0; c < n_col; c++) {
        const long long len = (long long)start[c + 1] - start[c];
        if (len < 1 || len > kDerivedMaxCode)
            return fail(APEMOST_HIP_ERR_INVALID, "%s: column %d: %lld instructions outside [1,%d]", who, c, len,
                        kDerivedMaxCode);
        int depth = 0, deepest = 0;
        for (int i = 0; i < (int)len; i++) {
            const uint32_t ins = (uint32_t)code[start[c] + i];
            const int op = (int)(ins & 255);
            const uint32_t arg = ins >> 8;
            int pops, pushes;
            derived_effect(op, &pops, &pushes);
            if (pops < 0)
                return fail(APEMOST_HIP_ERR_INVALID, "%s: column %d, instruction %d: unknown opcode %d", who, c, i, op);
            if (op == APEMOST_DERIVED_COL && arg > (uint32_t)n_par + 1)
                return fail(APEMOST_HIP_ERR_INVALID, "%s: column %d, instruction %d: COL %u beyond n_par + 1 = %d", who, c,
                            i, arg, n_par + 1);
            if (op == APEMOST_DERIVED_CONST && arg >= (uint32_t)n_const)
                return fail(APEMOST_HIP_ERR_INVALID, "%s: column %d, instruction %d: CONST %u of %d constants", who, c, i,
                            arg, n_const);
            if (depth < pops)
                return fail(APEMOST_HIP_ERR_INVALID, "%s: column %d, instruction %d: stack underflow (%d of %d values)",
                            who, c, i, depth, pops);
            depth += pushes - pops;
            if (depth > kDerivedMaxDepth)
                return fail(APEMOST_HIP_ERR_INVALID, "%s: column %d, instruction %d: stack depth %d above %d", who, c, i,
                            depth, kDerivedMaxDepth);
            if (depth > deepest)
                deepest = depth;
        }
        if (depth != 1)
            return fail(APEMOST_HIP_ERR_INVALID, "%s: column %d leaves %d values, not 1", who, c, depth);
        if (depth_out)
            depth_out[c] = deepest;
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_derived_check(int32_t n_par, int32_t n_col, const int32_t *code, const int32_t *start,
                                         int32_t n_const, int32_t *depth_out) {
    return derived_check_programs("derived_check", n_par, n_col, code, start, n_const, depth_out);
}

static DerivedProgram derived_program(const apemost_hip_sampler *s) {
    const DerivedFold &f = s->dv;
    DerivedProgram p;
    p.code = f.d_code;
    p.start = f.d_start;
    p.consts = f.d_consts;
    p.n_const = f.n_const;
    p.row_par = s->cfg.n_par;
    return p;
}

extern "C" int apemost_hip_derived_begin(apemost_hip_sampler *s, const apemost_hip_derived_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: config is NULL");
    FOLD_TRY(fold_check_chains(s, "derived", cfg->n_keep, cfg->chains));
    FOLD_TRY(derived_check_programs("derived_begin", s->cfg.n_par, cfg->n_col, cfg->code, cfg->start, cfg->n_const, nullptr));
    const int nc = cfg->n_col;
    if (cfg->n_const > 0 && !cfg->consts)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: %d constants and no consts", cfg->n_const);
    if ((long long)cfg->n_keep * nc > 65535)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: %d chains of %d columns are more than 65535 columns",
                    cfg->n_keep, nc);
    if (cfg->nbins < 1 || cfg->nbins > kJointMaxBins)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: nbins %d outside [1,%d]", cfg->nbins, kJointMaxBins);
    std::vector<int> pairs;
    if (!cfg->pairs) { // all i < j in lexicographic order
        for (int i = 0; i < nc; i++)
            for (int j = i + 1; j < nc; j++) {
                pairs.push_back(i);
                pairs.push_back(j);
            }
    } else {
        const long long all = (long long)nc * (nc - 1) / 2;
        if (cfg->n_pairs < 0 || cfg->n_pairs > all)
            return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: n_pairs %d outside [0,%lld]", cfg->n_pairs, all);
        std::vector<char> seen((size_t)nc * nc, 0);
        for (int q = 0; q < cfg->n_pairs; q++) {
            const int i = cfg->pairs[2 * q], j = cfg->pairs[2 * q + 1];
            if (i < 0 || j >= nc || i >= j || seen[(size_t)i * nc + j])
                return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: pairs[%d] = (%d, %d): 0 <= i < j < %d, no duplicates", q,
                            i, j, nc);
            seen[(size_t)i * nc + j] = 1;
            pairs.push_back(i);
            pairs.push_back(j);
        }
    }
    const int n_pairs = (int)(pairs.size() / 2);
    if (!cfg->lo || !cfg->hi)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: lo and hi are needed");
    FOLD_TRY(fold_check_ranges("derived", nc, cfg->lo, cfg->hi));
    const u64 n_counts = (u64)cfg->n_keep * n_pairs * cfg->nbins * cfg->nbins;
    if (n_counts * sizeof(u64) > ((u64)1 << 30))
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: %d chains x %d pairs x %d^2 bins: counts above 2^30 bytes",
                    cfg->n_keep, n_pairs, cfg->nbins);
    if (cfg->batch_size < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: batch_size must be >= 1");
    const size_t n_cols = (size_t)cfg->n_keep * nc, tri = (size_t)nc * (nc + 1) / 2;
    if (cfg->max_batches > ((u64)1 << 40) || cfg->max_batches + 1 > ((u64)1 << 40) / n_cols)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: max_batches %llu too large",
                    (unsigned long long)cfg->max_batches);
    if (cfg->stage_steps > ((u64)1 << 18))
        return fail(APEMOST_HIP_ERR_INVALID, "derived_begin: stage_steps %llu outside [0,%d]",
                    (unsigned long long)cfg->stage_steps, 1 << 18);
    FOLD_TRY(fold_reset(s, s->dv));
    DerivedFold &f = s->dv;
    // the staged columns: as the joint fold's, unless the caller sets the piece (the LDS counters are 32 bits wide)
    const u64 chunk = cfg->stage_steps ? cfg->stage_steps : fold_chunk((u64)1 << 22, n_cols, 18);
    const int n_code = cfg->start[nc];
    f.n_keep = cfg->n_keep;
    f.n_col = nc;
    f.nbins = cfg->nbins;
    f.n_pairs = n_pairs;
    f.n_const = cfg->n_const;
    f.bs = cfg->batch_size;
    f.max_batches = cfg->max_batches;
    f.chunk = chunk;
    f.n = 0;
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_chains, cfg->n_keep, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_pairs, (size_t)n_pairs * 2, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_code, n_code, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_start, nc + 1, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_consts, cfg->n_const, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_lo, nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_hi, nc, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_vals, n_cols * chunk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_bins, n_cols * chunk, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_origin, n_cols, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_sum, n_cols, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_cross, cfg->n_keep * tri, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_counts, n_counts, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_hist, n_cols * cfg->nbins, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_batch, n_cols * (cfg->max_batches + 1), true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_nonfinite, n_cols, true));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_vmin, n_cols, false));
    FOLD_TRY(fold_alloc(s, f.mem, &f.d_vmax, n_cols, false));
    const std::vector<double> least(n_cols, (double)INFINITY), greatest(n_cols, -(double)INFINITY);
    HIP_TRY(hipMemcpyAsync(f.d_chains, cfg->chains, cfg->n_keep * sizeof(int), hipMemcpyHostToDevice, s->stream));
    if (n_pairs > 0)
        HIP_TRY(hipMemcpyAsync(f.d_pairs, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_code, cfg->code, n_code * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_start, cfg->start, (nc + 1) * sizeof(int), hipMemcpyHostToDevice, s->stream));
    if (cfg->n_const > 0)
        HIP_TRY(hipMemcpyAsync(f.d_consts, cfg->consts, cfg->n_const * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_lo, cfg->lo, nc * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_hi, cfg->hi, nc * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_vmin, least.data(), n_cols * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(f.d_vmax, greatest.data(), n_cols * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the host vectors and the caller's arrays are read until here)
    f.open = true;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_derived_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                              uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    DerivedFold &f = s->dv;
    u64 kept;
    FOLD_TRY(fold_accumulate_check("derived", f.open, d_samples, n_steps, skip, thin, &kept));
    FOLD_TRY(fold_check_batches("derived", f.n, kept, f.bs, f.max_batches));
    if (kept == 0)
        return APEMOST_HIP_OK;
    FOLD_TRY(fold_order_behind_stream(s));
    const int nc = f.n_col, n_cols = f.n_keep * nc;
    const int band_rows = joint_band_rows(f.nbins), n_bands = (f.nbins + band_rows - 1) / band_rows;
    const int entries = f.n_keep * (nc + nc * (nc + 1) / 2);
    for (u64 k0 = 0; k0 < kept; k0 += f.chunk) {
        DerivedArgs d;
        JointArgs &a = d.j;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = nc;
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
        d.prog = derived_program(s);
        d.bs = f.bs;
        d.left = batches_left(f.n, f.bs);
        d.n_closed = batches_closed(f.n, f.bs);
        d.batch_stride = f.max_batches + 1;
        d.hist = f.d_hist;
        d.batch = f.d_batch;
        d.nonfinite = f.d_nonfinite;
        d.vmin = f.d_vmin;
        d.vmax = f.d_vmax;
        hipLaunchKernelGGL(derived_gather_kernel, dim3((a.n + kJointGatherPer - 1) / kJointGatherPer, (unsigned)n_cols),
                           dim3(kDerivedThreads), 0, s->copy_stream, d);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(derived_marginal_kernel, dim3((unsigned)n_cols), dim3(kDerivedThreads), 0, s->copy_stream, d);
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

static int derived_xfer(apemost_hip_sampler *s, const apemost_hip_derived_view *v, bool up) {
    CHECK_S(s);
    DerivedFold &f = s->dv;
    FOLD_TRY(fold_xfer_check("derived", f.open, v, up));
    if (up && v->n) {
        if (batches_closed(*v->n, f.bs) > f.max_batches)
            return fail(APEMOST_HIP_ERR_INVALID, "derived_set: %llu samples close more than max_batches batches",
                        (unsigned long long)*v->n);
        if (v->n_batches && *v->n_batches != batches_closed(*v->n, f.bs))
            return fail(APEMOST_HIP_ERR_INVALID, "derived_set: n_batches %llu does not follow from n = %llu",
                        (unsigned long long)*v->n_batches, (unsigned long long)*v->n);
    }
    const size_t nc = f.n_col, n_cols = (size_t)f.n_keep * nc, tri = nc * (nc + 1) / 2;
    const size_t n_counts = (size_t)f.n_keep * f.n_pairs * f.nbins * f.nbins;
    FOLD_TRY(fold_order_behind_stream(s));
    const FoldCopy copy{s, up};
    FOLD_TRY(copy(f.d_hist, v->hist, n_cols * f.nbins * sizeof(u64)));
    FOLD_TRY(copy(f.d_batch, v->batch, n_cols * (f.max_batches + 1) * sizeof(double)));
    FOLD_TRY(copy(f.d_counts, v->counts, n_counts * sizeof(u64)));
    FOLD_TRY(copy(f.d_origin, v->origin, n_cols * sizeof(double)));
    FOLD_TRY(copy(f.d_sum, v->sum, n_cols * sizeof(double)));
    FOLD_TRY(copy(f.d_cross, v->cross, f.n_keep * tri * sizeof(double)));
    FOLD_TRY(copy(f.d_nonfinite, v->nonfinite, n_cols * sizeof(u64)));
    FOLD_TRY(copy(f.d_vmin, v->vmin, n_cols * sizeof(double)));
    FOLD_TRY(copy(f.d_vmax, v->vmax, n_cols * sizeof(double)));
    FOLD_TRY(fold_xfer_wait(s));
    fold_xfer_count(f.n, v->n, up);
    if (!up && v->n_batches)
        *v->n_batches = batches_closed(f.n, f.bs);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_derived_get(apemost_hip_sampler *s, const apemost_hip_derived_view *v) {
    return derived_xfer(s, v, false);
}

extern "C" int apemost_hip_derived_set(apemost_hip_sampler *s, const apemost_hip_derived_view *v) {
    return derived_xfer(s, v, true);
}

extern "C" int apemost_hip_derived_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    return fold_reset(s, s->dv);
}

// the open fold's programs on the caller's rows, by the gather kernel's own device function
extern "C" int apemost_hip_derived_eval(apemost_hip_sampler *s, uint64_t n, const double *rows, double *out) {
    CHECK_S(s);
    DerivedFold &f = s->dv;
    if (!f.open)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_eval: no derived_begin");
    const u64 w = (u64)s->cfg.n_par + 2, most = (u64)1 << 26;
    if (n < 1 || !rows || !out || n > most / w || n > most / (u64)f.n_col)
        return fail(APEMOST_HIP_ERR_INVALID, "derived_eval: %llu rows, or a NULL array", (unsigned long long)n);
    FoldScratch scratch;
    double *d_rows = nullptr, *d_out = nullptr;
    const int rc = [&]() -> int { // (whatever fails, the stream is waited for before the scratch goes)
        FOLD_TRY(fold_alloc(s, scratch, &d_rows, (size_t)(n * w), false));
        FOLD_TRY(fold_alloc(s, scratch, &d_out, (size_t)n * f.n_col, false));
        HIP_TRY(hipMemcpyAsync(d_rows, rows, (size_t)(n * w) * sizeof(double), hipMemcpyHostToDevice, s->stream));
        hipLaunchKernelGGL(derived_eval_kernel, dim3((unsigned)((n + kDerivedThreads - 1) / kDerivedThreads), (unsigned)f.n_col),
                           dim3(kDerivedThreads), 0, s->stream, derived_program(s), f.n_col, (unsigned int)n, d_rows, d_out);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(out, d_out, (size_t)n * f.n_col * sizeof(double), hipMemcpyDeviceToHost, s->stream));
        return APEMOST_HIP_OK;
    }();
    const hipError_t sync = hipStreamSynchronize(s->stream);
    FOLD_TRY(rc);
    HIP_TRY(sync);
    return APEMOST_HIP_OK;
}
