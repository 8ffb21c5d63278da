// abi/sampler.h -- the sampler behind the C ABI's handle, how its entry points report errors, and what it owns.
// A part of apemost_hip.hip, which includes it once, behind the kernel headers and the standard ones.
#pragma once

static thread_local std::string g_last_error;

static int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                            \
    do {                                                                                         \
        hipError_t err__ = (expr);                                                               \
        if (err__ != hipSuccess)                                                                 \
            return fail(APEMOST_HIP_ERR_RUNTIME, "%s failed: %s (%s:%d)", #expr,                 \
                        hipGetErrorString(err__), __FILE__, __LINE__);                           \
    } while (0)

#define CHECK_S(s)                                                                               \
    do {                                                                                         \
        if (!(s))                                                                                \
            return fail(APEMOST_HIP_ERR_INVALID, "sampler is NULL");                             \
        HIP_TRY(hipSetDevice((s)->cfg.device));                                                  \
    } while (0)

// ---- the state of the on-device folds (abi/fold_common.h, abi/fold_*.h) ----
// Every fold lives between its apemost_hip_<fold>_begin and _end, accumulates on copy_stream, and knows its count of
// kept samples `n` on the host without a sync.  The structs stand here, not in the folds' own files, because the
// sampler holds one of each by value and every entry point of every fold needs the complete sampler.

namespace { // (internal linkage, like the unnamed structs of the sampler: no symbol of the library comes from here)

// the device memory a fold owns: filled by fold_alloc (abi/fold_common.h), released as a whole.  Plain data, so
// that a fold's struct is reset by `= {}` like everything else in the sampler.
constexpr int kFoldMaxOwned = 24;
struct FoldMem {
    void *owned[kFoldMaxOwned];
    int n_owned;
    void free_all() { // (the caller has synchronised the streams that use the memory, or hipFree waits for them)
        for (int i = 0; i < n_owned; i++)
            hipFree(owned[i]);
        n_owned = 0;
    }
};

// the scratch of one call: freed on every way out of it
struct FoldScratch : FoldMem {
    FoldScratch() : FoldMem{} {}
    ~FoldScratch() { free_all(); }
};

// a fold back to "not begun": its memory freed, every field zero
template <class Fold>
static void fold_free(Fold &f) {
    f.mem.free_all();
    f = {};
}

// the run summary (pt_summary.h)
struct SummaryFold {
    bool open;
    int n_hist, nbins;
    u64 bs, max_batches;
    u64 n;
    double *d_lo, *d_hi, *d_prob_sum, *d_batch;
    u64 *d_hist;
    FoldMem mem;
};

// on-device peaks (pt_peaks.h): the kept chains' parameter columns; n = samples stored per column
struct PeaksFold {
    bool open;
    int n_keep;
    u64 capacity;
    u64 n;
    int *d_chains;
    double *d_lo, *d_hi, *d_cols;
    FoldMem mem;
};

// on-device joint marginals (pt_joint.h): pair histograms and moments
struct JointFold {
    bool open;
    int n_keep, nbins, n_pairs;
    u64 chunk; // kept steps staged per launch
    u64 n;
    int *d_chains, *d_pairs;
    double *d_lo, *d_hi, *d_vals, *d_origin, *d_sum, *d_cross;
    unsigned short *d_bins;
    u64 *d_counts;
    FoldMem mem;
};

// on-device derived quantities (pt_derived.h): the summary's histograms and batch sums and the joint fold's pair
// counts and moments of computed columns
struct DerivedFold {
    bool open;
    int n_keep, n_col, nbins, n_pairs, n_const;
    u64 bs, max_batches;
    u64 chunk; // kept steps staged per launch
    u64 n;
    int *d_chains, *d_pairs, *d_code, *d_start;
    double *d_consts, *d_lo, *d_hi, *d_vals, *d_origin, *d_sum, *d_cross, *d_batch, *d_vmin, *d_vmax;
    unsigned short *d_bins;
    u64 *d_counts, *d_hist, *d_nonfinite;
    FoldMem mem;
};

// on-device evidence fold (pt_evidence.h): moments, batch sums and log-sum-exps of column n_par+1 of every chain
struct EvidenceFold {
    bool open;
    u64 bs, max_batches;
    u64 chunk; // kept steps staged per launch
    u64 n;
    double *d_coef, *d_vals, *d_origin, *d_sum, *d_sq, *d_batch, *d_m, *d_S;
    FoldMem mem;
};

// on-device MBAR (pt_mbar.h): loglike of every kept step of every chain, resident; n = kept steps stored
struct MbarFold {
    bool open;
    int K, L; // chains per ladder, ladders
    u64 capacity;
    u64 tiles_max; // tiles of a ladder's whole store: ceil(capacity * K / kMbarTile)
    u64 n;
    double *d_betas, *d_ell, *d_lnD;
    double *d_g;      // [2][n_chains]: g of the iteration under way and of the one before
    double *d_c;      // [n_chains]
    double *d_beta_t; // [n_chains]: the targets of one piece of an evaluate
    double *d_part;   // [kMbarWords][n_chains][tiles_max]
    double *d_out;    // [2 + kMbarWords][n_chains]: m, the sums, G
    unsigned long long *d_bad, *d_mkey; // [n_ladders], [n_chains]
    FoldMem mem;
};

// on-device reweighted posteriors (pt_reweight.h): chosen columns of every kept step of every chain, beside an open
// MbarFold whose capacity, ladders and ranges it shares; n = kept steps stored
struct ReweightFold {
    bool open;
    int n_cols, nbins, words; // words: 2 + n_cols + n_cols (n_cols + 1) / 2 sums per (ladder, target)
    int cols[16];
    u64 n;
    double *d_x;              // [n_cols][capacity][n_chains]
    double *d_lo, *d_hi;      // [n_cols]
    double *d_e;              // [capacity][n_chains]: e of the target under way
    unsigned long long *d_q;  // [capacity][n_chains]: its fixed-point image
    double *d_beta_t;         // [64]
    double *d_part;           // [words][n_ladders][tiles_max]
    unsigned long long *d_bad, *d_mkey; // [n_ladders][n_cols], [64][n_ladders]
    unsigned long long *d_C, *d_tsum;   // pt_resample.h, from the first resample on: [capacity][n_chains] words of C;
                                        // [n_ladders][tiles_max] tile prefixes and, behind them, [n_ladders] totals
    FoldMem mem;
};

// on-device autocorrelation (pt_autocorr.h): lag sums of kept chains' columns
struct AutocorrFold {
    bool open;
    int n_keep, n_cols, max_lag;
    u64 chunk; // kept steps staged per launch
    u64 n;
    int *d_chains, *d_cols;
    double *d_buf, *d_origin, *d_sum, *d_lag, *d_head, *d_tail;
    FoldMem mem;
};

// on-device posterior predictive (pt_predict.h): the model curve of kept chains' samples at n_x abscissae
struct PredictFold {
    bool open;
    int n_keep, n_x, nbins, points;
    int n_cols; // columns of the rows in d_x: 1, or the n_cols of a user model
    double lo, hi;
    u64 n;
    int *d_chains;
    double *d_x, *d_origin, *d_sum, *d_sq, *d_vmin, *d_vmax, *d_best_prob, *d_best_params;
    u64 *d_hist, *d_best_n;
    int *d_len; // [n_keep] abscissae per kept chain where they differ (the data of a ragged batch), else nullptr
    FoldMem mem;
};

// the tail of the pointwise fold (pt_pointwise_tail.h); capacity 0: none
struct PointwiseTailFold {
    int capacity, B;
    bool awaits_set;           // begun on a fold whose state was set: no accumulate before tail_set
    double *d_buf;             // [n_keep][n_blocks][B][64]
    unsigned int *d_slots;     // [n_keep][n_data]
    unsigned long long *d_thr; // [n_keep][n_data]
    FoldMem mem;
};

// on-device pointwise log-likelihood (pt_pointwise.h): the term of every datum under the kept chains' samples
struct PointwiseFold {
    bool open;
    int n_keep;
    int n_data; // the width of every [n_keep][n_data] array: the longest data among the kept chains' ladders
    double c;   // 1 / (-2 sigma^2)
    u64 n;
    int *d_chains;
    int *d_len; // [n_keep] data per kept chain where they differ (a ragged batch), else nullptr
    double *d_x, *d_y; // [n_keep][n_data] (a user model: d_x [n_keep][n_cols][n_data], no d_y)
    double *d_state;   // the eight [n_keep][n_data] words, one after the other (kPointwiseWords)
    double *d_par;     // par_origin, par_sum: [n_keep][n_par] each
    bool n_set;        // n is what pointwise_set put there: nothing has been accumulated since
    // the joint predictive of every kept chain's block (pt_pointwise_joint.h; pointwise_begin_at with joint = 1)
    double *d_joint;   // origin, sum, sq, m, S: [n_keep] each, one after the other (kPointwiseJointWords); else nullptr
    double *d_J;       // [n_keep][kPointwisePiece]: J of a piece's kept samples
    bool joint_awaits_set; // pointwise_set loaded samples: no accumulate before pointwise_joint_set has loaded theirs
    PointwiseTailFold tail;
    FoldMem mem;
};

// (the tail's memory is its own list: pointwise_tail_begin replaces the tail of an open fold)
static void fold_free(PointwiseFold &f) {
    f.tail.mem.free_all();
    f.mem.free_all();
    f = {};
}

// on-device predictive checks (pt_check.h): the predictive CDF of every datum and three discrepancy statistics per
// kept sample
struct CheckFold {
    bool open;
    int n_keep;
    int n_data;  // the width of every [n_keep][n_data] array: the longest data among the kept chains' ladders
    int n_edges; // edges per statistic; 0: no counts
    double c, inv_sigma; // 1 / (-2 sigma^2), 1 / sigma
    u64 n;
    int *d_chains;
    int *d_len;          // [n_keep] data per kept chain where they differ (a ragged batch), else nullptr
    double *d_x, *d_y;   // [n_keep][n_data]
    double *d_state;     // the seven [n_keep][n_data] words, one after the other (kCheckWords)
    double *d_stat;      // origin, sum, sq, min, max: [n_keep][3] each, one after the other (kCheckStatWords)
    double *d_T;         // [n_keep][3][kPointwisePiece]: the statistics of a piece's kept samples
    double *d_edges;     // [3][n_edges], or nullptr
    u64 *d_counts;       // [n_keep][3][n_edges + 2], or nullptr
    FoldMem mem;
};

// on-device residual periodogram (pt_periodogram.h): the power of every kept sample's residuals on a frequency grid
struct PeriodogramFold {
    bool open;
    int n_keep;
    int n_data; // the width of every [n_keep][n_data] array: the longest data among the kept chains' ladders
    int n_freq;
    int piece;  // kept steps of one launch: what the scratch arrays have room for, <= kPeriodogramPiece
    u64 n;
    int *d_chains;
    int *d_len;          // [n_keep] data per kept chain where they differ (a ragged batch), else nullptr
    double *d_x, *d_y;   // [n_keep][n_data]
    double *d_freqs, *d_weights, *d_level; // [n_freq], [n_keep][n_freq][3], [n_keep]
    double *d_state;     // the seven [n_keep][n_freq] words, one after the other (kPeriodogramWords)
    u64 *d_exceed;       // [n_keep][n_freq]
    double *d_peak;      // origin, sum, sq, min, max: [n_keep] each, one after the other (kPeriodogramPeakWords)
    u64 *d_peak_counts;  // [n_keep][n_freq + 1]
    double *d_r;         // [n_keep][piece][n_data]: a piece's residuals
    double *d_C, *d_S, *d_P; // [n_keep][piece][n_freq] each
    double *d_pk_m;      // [n_keep][piece]
    int *d_pk_arg;       // [n_keep][piece]
    FoldMem mem;
};

} // namespace

struct apemost_hip_sampler {
    apemost_hip_config cfg;
    DevArrays d;
    ChainShape sh;
    int waves;
    bool producers; // candidate-producer wavefronts in the round / calibrate kernels
    bool lds_data;
    size_t lds_bytes, lds_fixed_bytes;
    bool resident_ok; // the whole grid of the round kernel fits the device at once ...
    bool resident_lds, resident_plain; // ... with / without the data vector staged in LDS
    int cur;
    u64 round;
    int swap_pending;
    hipStream_t stream;
    hipEvent_t ev0, ev1;
    u64 launches, launches_at_begin;
    std::vector<void *> allocations;
    // a calibration in progress (calibrate_begin .. calibrate_end): launched in segments
    struct {
        bool open;      // between begin and end
        bool in_flight; // a segment has been launched and its records not collected yet
        bool cancelled;
        int first, count, burn_in_only, capacity, progress_slot, progress_cap;
        apemost_hip_calib_config cfg;
        CalibRec *d_rec;
        double *d_orig, *d_progress;
        int *d_list;
        CalibRec *h_rec; // pinned [capacity]
        int *h_list;     // pinned [capacity]: slots still calibrating
        int n_active;
        hipEvent_t ev;
        u64 segments, launches_by_waves[9];
        double seconds_by_waves[9]; // wall time of the segments of each workgroup shape (launch to collection)
        std::chrono::steady_clock::time_point segment_start;
        int segment_waves;
    } cal;
    unsigned big_lds_set; // bit w: the LDS opt-in of the w-wave kernels has been made
    // APEMOST_MODEL_USER: the kernels of the user's likelihood, compiled by hiprtc at create time
    // (indexed by the waves per chain of the two-phase kernels: 1, 2, 4, 8; with
    // APEMOST_HIP_FLAG_USER_ONE_BARRIER also the one-barrier kernels of 4 and 8 likelihood waves, which decide
    // through the user's finish() instead of the built-in models' threshold form)
    struct {
        hipModule_t module;
        hipFunction_t round[9], calibrate[9], calc_model[9], loglike[9];
        hipFunction_t round_ob[9], calibrate_ob[9]; // (calibrate_ob: not for the variant instantiations)
    } user;
    // ... and the kernels of its optional hooks (pt_user_fold.h), a second module compiled on the first predict_* or
    // pointwise_* call (user_analysis): the functions of an absent hook stay null
    struct {
        bool ready; // the hooks are known (and, where there is one, the module is loaded)
        bool has_curve, has_pointwise;
        hipModule_t module;
        hipFunction_t predict_fold, predict_fold_hist, predict_curve, pointwise_fold, pointwise_loglike, pointwise_tail_append;
        double compile_seconds; // hiprtc's time for this sampler's analysis module (0: from the process's cache)
    } ua;
    std::string user_source, user_shown; // the model's text as user_model_build read it, its path as a C string literal
    // edge records for in-process shard exchanges (created on first use), one set per side (0 = lower edge,
    // 1 = upper edge): under the even-odd schedule an interior shard exchanges on both edges before one launch
    double *edge_out[2], *edge_in[2];
    hipEvent_t ev_exported[2], ev_imported[2];
    hipStream_t copy_stream; // drains sample rows and runs the folds while the next launch runs (created on first use)
    hipEvent_t ev_copy;
    u64 *h_word;             // pinned copy of the launch error word, refreshed by every async read
    bool one_barrier;    // stepping launches use pt_round_ob_kernel
    bool ob_helper;      // ... in its form with a helper wavefront (see ob_wants_helper), where the betas allow it:
    bool betas_split_ok; // every beta on the device is > 0 with a finite 1/beta (betas_allow_split; true until betas arrive)
    int cus;             // compute units of the device
    int kmodel;          // template argument of this sampler's kernels: cfg.model, + kVariantModel when a
                         // non-default proposal law or swap schedule is asked for (pt_device.h)
    bool cooperative;    // multi-round launches through hipLaunchCooperativeKernel
    bool handoff_failed; // an in-launch hand-off timed out once: single-round launches from then on
    double user_compile_seconds; // hiprtc's time for this sampler's user model (0: taken from the process's cache)
    double *rwm_keep;            // APEMOST_HIP_FLAG_RWM: what the extra step of a round must not be seen to change
    bool in_rwm;
    // a ladder batch (apemost_hip_create_batch): n_ladders independent ladders of `per_ladder` chains in one grid;
    // cfg.n_chains = cfg.n_chains_global = their product, sh.n_global = per_ladder, cfg.seed = seeds[0]
    bool batch;
    bool track; // APEMOST_HIP_FLAG_TRACK_REPLICAS: the flow words behind the ladder words exist
    int n_ladders, per_ladder;
    std::vector<u64> seeds;        // [n_ladders] (empty for an ordinary sampler)
    std::vector<double> x_abs_max; // [n_ladders] of each ladder's data
    // each ladder's data rows and where its matrix starts in d.data, in doubles (apemost_hip_create_batch_ragged;
    // an equal batch: cfg.n_data and b * n_cols * cfg.n_data); cfg.n_data is the largest length.  data_off has
    // n_ladders + 1 entries, the last being the whole allocation.  Empty for an ordinary sampler.
    std::vector<int> data_len;
    std::vector<u64> data_off;
    bool ragged; // the lengths differ
    // the folds (apemost_hip_<fold>_begin .. _end), each in abi/fold_<fold>.h
    SummaryFold sum;
    PeaksFold pk;
    JointFold jt;
    EvidenceFold ev;
    AutocorrFold ac;
    PredictFold pr;
    PointwiseFold pw;
    DerivedFold dv;
    CheckFold ck;
    PeriodogramFold pg;
    MbarFold mb;
    ReweightFold rw;
};

// the data rows of ladder b and its column-major matrix on the device (an ordinary sampler: b = 0)
static int ladder_len(const apemost_hip_sampler *s, int b) { return s->batch ? s->data_len[b] : s->cfg.n_data; }
static const double *ladder_data(const apemost_hip_sampler *s, int b) { return s->d.data + (s->batch ? s->data_off[b] : 0); }

// the data rows of each kept chain's ladder; returns the largest, *differ: they are not all equal
static int kept_lengths(const apemost_hip_sampler *s, int n_keep, const int *chains, std::vector<int> &len, bool *differ) {
    len.resize(n_keep);
    int longest = 0;
    *differ = false;
    for (int k = 0; k < n_keep; k++) {
        len[k] = ladder_len(s, s->batch ? chains[k] / s->per_ladder : 0);
        longest = len[k] > longest ? len[k] : longest;
        *differ = *differ || len[k] != len[0];
    }
    return longest;
}

// everything a sampler owns on the device; safe on a half-built sampler
static void release(apemost_hip_sampler *s) {
    if (s->stream)
        hipStreamSynchronize(s->stream);
    for (void *p : s->allocations)
        hipFree(p);
    if (s->cal.d_rec)
        hipFree(s->cal.d_rec);
    if (s->cal.d_orig)
        hipFree(s->cal.d_orig);
    if (s->cal.d_progress)
        hipFree(s->cal.d_progress);
    if (s->cal.d_list)
        hipFree(s->cal.d_list);
    if (s->cal.h_rec)
        hipHostFree(s->cal.h_rec);
    if (s->cal.h_list)
        hipHostFree(s->cal.h_list);
    if (s->cal.ev)
        hipEventDestroy(s->cal.ev);
    if (s->user.module)
        hipModuleUnload(s->user.module);
    if (s->ua.module)
        hipModuleUnload(s->ua.module);
    if (s->copy_stream) {
        hipStreamSynchronize(s->copy_stream);
        hipStreamDestroy(s->copy_stream);
    }
    fold_free(s->sum); // (the folds' kernels ran on copy_stream)
    fold_free(s->pk);
    fold_free(s->jt);
    fold_free(s->ev);
    fold_free(s->ac);
    fold_free(s->pr);
    fold_free(s->pw);
    fold_free(s->dv);
    fold_free(s->ck);
    fold_free(s->pg);
    fold_free(s->mb);
    fold_free(s->rw);
    if (s->ev_copy)
        hipEventDestroy(s->ev_copy);
    for (int k = 0; k < 2; k++) {
        if (s->ev_exported[k])
            hipEventDestroy(s->ev_exported[k]);
        if (s->ev_imported[k])
            hipEventDestroy(s->ev_imported[k]);
    }
    if (s->h_word)
        hipHostFree(s->h_word);
    if (s->ev0)
        hipEventDestroy(s->ev0);
    if (s->ev1)
        hipEventDestroy(s->ev1);
    if (s->stream)
        hipStreamDestroy(s->stream);
    delete s;
}
