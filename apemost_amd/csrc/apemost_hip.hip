// apemost_hip.hip -- kernels and C ABI of the gfx950 parallel-tempering engine
// (declared in include/apemost_hip.h).  Written for MI355X only.
#include "pt_autocorr.h"
#include "pt_evidence.h"
#include "pt_joint.h"
#include "pt_kernels.h"
#include "pt_peaks.h"
#include "pt_pointwise.h"
#include "pt_pointwise_tail.h"
#include "pt_predict.h"
#include "pt_user_fold.h"
#include "pt_summary.h"
#include "pt_text.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <hip/hiprtc.h>
#include <dlfcn.h>

#include <chrono>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

using namespace apemost;

// ===========================================================================
// kernels that are not templates over the model (the others: pt_kernels.h)
// ===========================================================================
// ---- test hooks ----
__global__ void rng_raw_kernel(u64 seed, u64 subseq, u64 offset, int n, unsigned int *out) {
    if (threadIdx.x != 0 || blockIdx.x != 0)
        return;
    rocrand_state_philox4x32_10 st;
    rocrand_init(seed, subseq, offset, &st);
    for (int i = 0; i < n; i++)
        out[i] = rocrand(&st);
}

__global__ void rng_attempts_kernel(u64 seed, u64 chain, int slot, u64 tick, u64 q0, int n, double *y,
                                    double *s, int *valid, double *log_u) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {
        double yy, ss;
        valid[i] = gaussian_attempt(seed, chain, slot, tick, q0 + (u64)i, yy, ss) ? 1 : 0;
        y[i] = yy;
        s[i] = ss;
    }
    if (i == 0)
        *log_u = accept_log_uniform(seed, chain, slot, tick);
}

// edge records for sharded ladders: beta, prob, prob_best, params[n], params_best[n]
// adapt() of -DADAPT (src/parallel_tempering.c:282-301), called by the reference once per round
// between the n_swap steps and tempering_interaction (:404): one thread per chain.  The counters
// summed over the parameters (src/mcmc_gettersetter.c:25-41), accepts / REJECTS against the
// target, all step widths of the chain scaled by 0.99 or by the double 1 / 0.99
// (gsl_vector_scale), counters restarted past 100000 counted updates (reset_accept_rejects).
// A kernel of its own rather than a tail of the round kernels: those carry no register for it.
__global__ void pt_adapt_kernel(DevArrays d, double target) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d.n)
        return;
    const int n = d.np;
    u64 *pacc = d.params_accepts() + (size_t)c * n, *prej = d.params_rejects() + (size_t)c * n;
    double *step = d.step() + (size_t)c * n;
    u64 acc = 0, rej = 0;
    for (int p = 0; p < n; p++) {
        acc += pacc[p];
        rej += prej[p];
    }
    if (acc + rej < 20000)
        return;
    const double ratio = (double)acc * 1.0 / (double)rej;
    if (ratio < target - 0.05) {
        for (int p = 0; p < n; p++)
            step[p] *= 0.99;
    } else if (ratio > target + 0.05) {
        for (int p = 0; p < n; p++)
            step[p] *= 1 / 0.99;
    }
    if (acc + rej > 100000) {
        for (int p = 0; p < n; p++)
            pacc[p] = prej[p] = 0;
        d.accept()[c] = d.reject()[c] = 0;
    }
}

// adapt() of -DRWM (src/parallel_tempering.c:268-281 + rmw_adapt_stepwidth, src/markov_chain.c:342-367) around
// ONE more step of the ordinary round kernel: `pre` keeps what that step must not be seen to have changed (the
// log-posterior before it, the best point), `post` puts the best point and n_iter back and moves the step widths.
// keep: [n][2 + n_par] = prob, prob_best, params_best.  One thread per chain; `half` = the half of the
// double-buffered state the chain currently lives in.
__global__ void pt_rwm_pre_kernel(DevArrays d, int half, double *keep) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d.n)
        return;
    const int n = d.np, row = c + 1;
    double *k = keep + (size_t)c * (2 + n);
    k[0] = d.prob(half)[row];
    k[1] = d.prob_best(half)[row];
    for (int p = 0; p < n; p++)
        k[2 + p] = d.params_best(half)[(size_t)row * n + p];
}

__global__ void pt_rwm_post_kernel(DevArrays d, ChainShape sh, int half, const double *keep, double target) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= d.n)
        return;
    const int n = d.np, row = c + 1;
    const double *k = keep + (size_t)c * (2 + n);
    d.prob_best(half)[row] = k[1];
    for (int p = 0; p < n; p++)
        d.params_best(half)[(size_t)row * n + p] = k[2 + p];
    const u64 n_iter = d.n_iter()[c] - 1; // (no mcmc_check behind the extra step)
    d.n_iter()[c] = n_iter;
    double alpha = exp(d.prob(half)[row] - k[0]);
    if (alpha > 1)
        alpha = 1;
    const u64 tick = d.ticks()[c] - 1; // the extra step's
    const u64 g = (u64)(sh.chain_offset + c);
    for (int p = 0; p < n; p++) {
        const size_t i = (size_t)c * n + p;
        const double scale = d.pmax()[i] - d.pmin()[i];
        const double lo = 0.0000001 * scale, hi = 1000000 * scale;
        const uint4 b = philox_block(sh.seed, g * APEMOST_HIP_STREAMS_PER_CHAIN + (u64)n, (tick << kTickShift) | (u64)(1 + p / 4));
        const unsigned int w = (p & 3) == 0 ? b.x : (p & 3) == 1 ? b.y : (p & 3) == 2 ? b.z : b.w;
        double step = d.step()[i];
        step += u32_to_uniform(w) / sqrt((double)n_iter) * (alpha - target) * scale;
        if (step < lo)
            step = lo;
        if (step > hi)
            step = hi;
        d.step()[i] = step;
    }
}

// Sample rows [n_steps][n_chains][n_par+2] -> what a sink writes, for the kept steps skip, skip + thin, ...
// layout 0: the record of the C host's binary sink (apemost_amd/host/src/parallel_tempering.c): the
//   parameter vectors of chains 0..n_param_chains-1, then (prob, prob - prior) of every chain;
// layout 1: the rows themselves, thinned.
// One thread per output double: coalesced writes, gathered reads; a few KB per step against HBM.
__global__ void samples_pack_kernel(const double *rows, int n_chains, int n_par, unsigned long long n_kept,
                                    unsigned long long skip, unsigned long long thin, int n_param_chains, int layout,
                                    double *out) {
    const size_t row = (size_t)n_chains * (n_par + 2);
    const size_t record = layout == 0 ? (size_t)n_param_chains * n_par + 2 * (size_t)n_chains : row;
    const size_t total = (size_t)n_kept * record;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const size_t k = i / record, r = i - k * record;
        const double *src = rows + (skip + k * thin) * row;
        size_t from = r;
        if (layout == 0) {
            const size_t head = (size_t)n_param_chains * n_par;
            if (r < head) {
                const size_t chain = r / n_par;
                from = chain * (n_par + 2) + (r - chain * n_par);
            } else {
                const size_t q = r - head;
                from = (q >> 1) * (n_par + 2) + n_par + (q & 1);
            }
        }
        out[i] = src[from];
    }
}

__global__ void edge_export_kernel(DevArrays d, int n_par, int cur, int row, double *buf) {
    const int t = threadIdx.x;
    if (t == 0) {
        buf[0] = d.beta()[row];
        buf[1] = d.prob(cur)[row];
        buf[2] = d.prob_best(cur)[row];
    }
    if (t < n_par) {
        buf[3 + t] = d.params(cur)[(size_t)row * n_par + t];
        buf[3 + n_par + t] = d.params_best(cur)[(size_t)row * n_par + t];
    }
}

__global__ void edge_import_kernel(DevArrays d, int n_par, int cur, int row, const double *buf) {
    const int t = threadIdx.x;
    if (t == 0) {
        d.beta()[row] = buf[0];
        d.prob(cur)[row] = buf[1];
        d.prob_best(cur)[row] = buf[2];
    }
    if (t < n_par) {
        d.params(cur)[(size_t)row * n_par + t] = buf[3 + t];
        d.params_best(cur)[(size_t)row * n_par + t] = buf[3 + n_par + t];
    }
}

// ===========================================================================
// host side of the C ABI
// ===========================================================================

// ---- run-time model -> the translation unit that holds its kernels (pt_kernels.h) ----
#define APEMOST_EXTERN_MODEL(M) extern template hipError_t apemost::model_dispatch<M>(int, const AnyOp &);
APEMOST_EXTERN_MODEL(0)
APEMOST_EXTERN_MODEL(1)
APEMOST_EXTERN_MODEL(2)
APEMOST_EXTERN_MODEL(3)
APEMOST_EXTERN_MODEL(8)
APEMOST_EXTERN_MODEL(9)
APEMOST_EXTERN_MODEL(10)
APEMOST_EXTERN_MODEL(11)

static hipError_t dispatch_any(int model, int waves, const AnyOp &op) {
    switch (model) {
    case 0:
        return model_dispatch<0>(waves, op);
    case 1:
        return model_dispatch<1>(waves, op);
    case 2:
        return model_dispatch<2>(waves, op);
    case 3:
        return model_dispatch<3>(waves, op);
    case 8:
        return model_dispatch<8>(waves, op);
    case 9:
        return model_dispatch<9>(waves, op);
    case 10:
        return model_dispatch<10>(waves, op);
    case 11:
        return model_dispatch<11>(waves, op);
    }
    return hipErrorInvalidDeviceFunction; // (APEMOST_MODEL_USER never comes here: its kernels are a run-time module)
}
static hipError_t dispatch(int model, int waves, const LaunchOp &f) {
    AnyOp op;
    op.what = AnyOp::LAUNCH;
    op.launch = f;
    return dispatch_any(model, waves, op);
}
static hipError_t dispatch(int model, int waves, const LdsAttrOp &f) {
    AnyOp op;
    op.what = AnyOp::LDS_ATTR;
    op.lds = f;
    return dispatch_any(model, waves, op);
}
static hipError_t dispatch(int model, int waves, const OccupancyOp<true> &f) {
    AnyOp op;
    op.what = AnyOp::OCCUPANCY_LDS;
    op.occ_lds = f;
    return dispatch_any(model, waves, op);
}
static hipError_t dispatch(int model, int waves, const OccupancyOp<false> &f) {
    AnyOp op;
    op.what = AnyOp::OCCUPANCY_PLAIN;
    op.occ_plain = f;
    return dispatch_any(model, waves, op);
}

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
    hipStream_t copy_stream; // drains sample rows while the next launch runs (created on first use)
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
    // the run summary (apemost_hip_summary_begin .. end): accumulated by summary_kernel on copy_stream
    // a ladder batch (apemost_hip_create_batch): n_ladders independent ladders of `per_ladder` chains in one grid;
    // cfg.n_chains = cfg.n_chains_global = their product, sh.n_global = per_ladder, cfg.seed = seeds[0]
    bool batch;
    bool track; // APEMOST_HIP_FLAG_TRACK_REPLICAS: the flow words behind the ladder words exist
    int n_ladders, per_ladder;
    std::vector<u64> seeds;        // [n_ladders] (empty for an ordinary sampler)
    std::vector<double> x_abs_max; // [n_ladders] of each ladder's data
    struct {
        bool open;
        int n_hist, nbins;
        u64 bs, max_batches;
        u64 n; // kept samples so far (the host knows it without a sync)
        double *d_lo, *d_hi, *d_prob_sum, *d_batch;
        u64 *d_hist;
    } sum;
    // on-device peaks (apemost_hip_peaks_begin .. end): the kept chains' parameter columns, appended on copy_stream
    struct {
        bool open;
        int n_keep;
        u64 capacity;
        u64 n; // samples stored per column (the host knows it without a sync)
        int *d_chains;
        double *d_lo, *d_hi, *d_cols;
    } pk;
    // on-device joint marginals (apemost_hip_joint_begin .. end): pair histograms and moments, on copy_stream
    struct {
        bool open;
        int n_keep, nbins, n_pairs;
        u64 chunk; // kept steps staged per launch
        u64 n;     // kept samples so far (the host knows it without a sync)
        int *d_chains, *d_pairs;
        double *d_lo, *d_hi, *d_vals, *d_origin, *d_sum, *d_cross;
        unsigned short *d_bins;
        u64 *d_counts;
    } jt;
    // on-device evidence fold (apemost_hip_evidence_begin .. end): moments, batch sums and log-sum-exps of column
    // n_par+1 of every chain, on copy_stream
    struct {
        bool open;
        u64 bs, max_batches;
        u64 chunk; // kept steps staged per launch
        u64 n;     // kept samples so far (the host knows it without a sync)
        double *d_coef, *d_vals, *d_origin, *d_sum, *d_sq, *d_batch, *d_m, *d_S;
    } ev;
    // on-device autocorrelation (apemost_hip_autocorr_begin .. end): lag sums of kept chains' columns, on copy_stream
    struct {
        bool open;
        int n_keep, n_cols, max_lag;
        u64 chunk; // kept steps staged per launch
        u64 n;     // kept samples so far (the host knows it without a sync)
        int *d_chains, *d_cols;
        double *d_buf, *d_origin, *d_sum, *d_lag, *d_head, *d_tail;
    } ac;
    // on-device posterior predictive (apemost_hip_predict_begin .. end): the model curve of kept chains' samples at
    // n_x abscissae, on copy_stream
    struct {
        bool open;
        int n_keep, n_x, nbins, points;
        int n_cols; // columns of the rows in d_x: 1, or the n_cols of a user model
        double lo, hi;
        u64 n; // kept samples so far (the host knows it without a sync)
        int *d_chains;
        double *d_x, *d_origin, *d_sum, *d_sq, *d_vmin, *d_vmax, *d_best_prob, *d_best_params;
        u64 *d_hist, *d_best_n;
    } pr;
    // on-device pointwise log-likelihood (apemost_hip_pointwise_begin .. end): the term of every datum under the kept
    // chains' samples, on copy_stream
    struct {
        bool open;
        int n_keep;
        double c; // 1 / (-2 sigma^2)
        u64 n;    // kept samples so far (the host knows it without a sync)
        int *d_chains;
        double *d_x, *d_y;    // [n_keep][n_data] (a user model: d_x [n_keep][n_cols][n_data], no d_y)
        double *d_state;      // the eight [n_keep][n_data] words, one after the other (kPointwiseWords)
        double *d_par;        // par_origin, par_sum: [n_keep][n_par] each
        bool n_set;           // n is what pointwise_set put there: nothing has been accumulated since
        // its tail (apemost_hip_pointwise_tail_begin, pt_pointwise_tail.h); capacity 0: none
        struct {
            int capacity, B;
            bool awaits_set; // begun on a fold whose state was set: no accumulate before tail_set
            double *d_buf;               // [n_keep][n_blocks][B][64]
            unsigned int *d_slots;       // [n_keep][n_data]
            unsigned long long *d_thr;   // [n_keep][n_data]
        } tail;
    } pw;
};

extern "C" const char *apemost_hip_last_error(void) { return g_last_error.c_str(); }
extern "C" int apemost_hip_abi_version(void) { return APEMOST_HIP_ABI_VERSION; }

extern "C" int apemost_hip_device_count(int *count) {
    if (!count)
        return fail(APEMOST_HIP_ERR_INVALID, "count is NULL");
    int n = 0;
    hipError_t err = hipGetDeviceCount(&n);
    if (err != hipSuccess || n <= 0) {
        *count = 0;
        return fail(APEMOST_HIP_ERR_NO_DEVICE, "no HIP device: %s", hipGetErrorString(err));
    }
    *count = n;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_device_info(int device, char *name, size_t name_len, int *compute_units,
                                       uint64_t *hbm_bytes) {
    int n = 0;
    int rc = apemost_hip_device_count(&n);
    if (rc != APEMOST_HIP_OK)
        return rc;
    if (device < 0 || device >= n)
        return fail(APEMOST_HIP_ERR_INVALID, "device %d out of range [0,%d)", device, n);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (name && name_len) {
        strncpy(name, prop.gcnArchName, name_len - 1);
        name[name_len - 1] = 0;
    }
    if (compute_units)
        *compute_units = prop.multiProcessorCount;
    if (hbm_bytes)
        *hbm_bytes = prop.totalGlobalMem;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(APEMOST_HIP_ERR_NO_DEVICE, "device %d is %s; this engine is built for gfx950 only",
                    device, prop.gcnArchName);
    return APEMOST_HIP_OK;
}

static int enable_big_lds(apemost_hip_sampler *s, int waves);
static int max_rounds_per_launch(apemost_hip_sampler *s);
static int user_model_build(apemost_hip_sampler *s);
template <bool LDS>
static hipError_t round_occupancy(int model, int waves, bool producers, bool one_barrier, bool helper, size_t lds_bytes, int *blocks);
static size_t ob_lds_bytes(const apemost_hip_sampler *s, bool lds_data);
static bool ob_wants_helper(const apemost_hip_sampler *s, int n_chains);
static bool user_may_ob(const apemost_hip_sampler *s);
static int user_analysis(apemost_hip_sampler *s);

template <class T>
static int dev_alloc(apemost_hip_sampler *s, T **p, size_t count) {
    void *q = nullptr;
    HIP_TRY(hipMalloc(&q, (count ? count : 1) * sizeof(T)));
    s->allocations.push_back(q); // owned from here on, whatever fails next
    HIP_TRY(hipMemsetAsync(q, 0, (count ? count : 1) * sizeof(T), s->stream));
    *p = (T *)q;
    return APEMOST_HIP_OK;
}

// Staging pays when the staged bytes are re-read (several steps per launch) and the LDS
// footprint still lets enough workgroups share a CU; otherwise the data vector is read through
// L2 (it is shared by every chain, so it stays resident there).
static bool choose_lds(const apemost_hip_config &c, size_t lds_bytes) {
    const long long wg_per_cu = (160 * 1024) / (long long)lds_bytes;
    const long long wanted = ((long long)c.n_chains + 255) / 256;
    return wg_per_cu >= (wanted < 4 ? wanted : 4);
}

static int choose_waves(const apemost_hip_config &c) {
    if (c.waves_per_chain > 0)
        return c.waves_per_chain;
    // Measured on one MI355X (simplesin, 1024 points, steps/s by waves 1/2/4/8):
    //    128 chains  -   /  -   / 1.23 / 1.33 e8      512 chains  2.07 / 2.10 / 2.59 / 1.97 e8
    //    256 chains  1.09 / 1.46 / 2.22 / 1.82 e8    1024 chains  3.98 / 3.29 / 2.84 / 2.07 e8
    // (sine3 1024 x 8192: 3.5e7 with 1 wave, 3.1e7 with 2; pulse_vrot 2048 x 65536: 4.2 / 3.9 / 4.0 /
    // 3.5 e6.)  A chain's step is a latency chain: while CUs are idle more waves per chain shorten
    // it; once every SIMD has a wave, a chain per wave without barriers does more.
    // Since the one-barrier kernel (see has_one_barrier): four likelihood waves per chain up to 512
    // chains -- two waves per SIMD with the owner and the producers, no likelihood wave waits for a
    // sibling on its SIMD -- and eight only where a step is long enough to be bound by issue rather
    // than by the chain of dependent operations (>= 8192 points at <= 128 chains).
    // The pulse likelihood with more than three modes -- a loop over the modes that reads its parameters
    // from LDS as it goes, a longer chain per point than the others -- is the exception: eight waves up
    // to 256 chains (256 x 1024: 1.51 vs 1.41e8, 128 x 1024: 9.0 vs 8.2e7 in round 2; pulse_vrot and
    // sine3 stay with four: 8.9 vs 8.4e7 and 1.05 vs 1.03e8 at 128 x 1024; tools/experiments/gpu_exp_w8.sh).  Up
    // to three modes the spectrum is taken over a common denominator since round 3 (16 instead of 46
    // instructions per point) and four waves do more: 64 / 128 / 256 / 512 x 1024 5.14 / 11.2 / 23.6 /
    // 35.5e7 against 5.01 / 10.9 / 21.5 / 4.8e7 with eight (profiles/r03_pulse_waves.txt).
    // Two waves per chain only while such a ladder is still resident (three or four two-wave
    // workgroups per CU: up to 768 chains; 700 x 1024: 2.55 vs 2.46e8); beyond that a launch would
    // hold one round and one wave per chain does more (900 x 1024: 3.11 vs 1.68e8).
    int by_chip = (c.n_chains <= 128 && c.n_data >= 8192) ? 8 : c.n_chains <= 512 ? 4 : c.n_chains <= 768 ? 2 : 1;
    if (c.model == APEMOST_MODEL_PULSE && c.n_chains <= 256 && c.n_par > 8)
        by_chip = 8;
    // never fewer than 2 data points per lane
    int by_data = 1;
    while (by_data < 8 && c.n_data >= by_data * 2 * kWave * 2)
        by_data *= 2;
    return by_chip < by_data ? by_chip : by_data;
}

// the run summary's device arrays (the caller has synchronised the streams that use them)
static void summary_free(apemost_hip_sampler *s) {
    for (void *p : {(void *)s->sum.d_lo, (void *)s->sum.d_hi, (void *)s->sum.d_prob_sum, (void *)s->sum.d_batch,
                    (void *)s->sum.d_hist})
        if (p)
            hipFree(p);
    s->sum = {};
}

static void peaks_free(apemost_hip_sampler *s) {
    for (void *p : {(void *)s->pk.d_chains, (void *)s->pk.d_lo, (void *)s->pk.d_hi, (void *)s->pk.d_cols})
        if (p)
            hipFree(p);
    s->pk = {};
}

static void joint_free(apemost_hip_sampler *s) {
    for (void *p : {(void *)s->jt.d_chains, (void *)s->jt.d_pairs, (void *)s->jt.d_lo, (void *)s->jt.d_hi,
                    (void *)s->jt.d_vals, (void *)s->jt.d_origin, (void *)s->jt.d_sum, (void *)s->jt.d_cross,
                    (void *)s->jt.d_bins, (void *)s->jt.d_counts})
        if (p)
            hipFree(p);
    s->jt = {};
}

static void evidence_free(apemost_hip_sampler *s) {
    for (double *p : {s->ev.d_coef, s->ev.d_vals, s->ev.d_origin, s->ev.d_sum, s->ev.d_sq, s->ev.d_batch, s->ev.d_m,
                      s->ev.d_S})
        if (p)
            hipFree(p);
    s->ev = {};
}

static void autocorr_free(apemost_hip_sampler *s) {
    for (int *p : {s->ac.d_chains, s->ac.d_cols})
        if (p)
            hipFree(p);
    for (double *p : {s->ac.d_buf, s->ac.d_origin, s->ac.d_sum, s->ac.d_lag, s->ac.d_head, s->ac.d_tail})
        if (p)
            hipFree(p);
    s->ac = {};
}

static void predict_free(apemost_hip_sampler *s) {
    for (void *p : {(void *)s->pr.d_chains, (void *)s->pr.d_x, (void *)s->pr.d_origin, (void *)s->pr.d_sum,
                    (void *)s->pr.d_sq, (void *)s->pr.d_vmin, (void *)s->pr.d_vmax, (void *)s->pr.d_best_prob,
                    (void *)s->pr.d_best_params, (void *)s->pr.d_hist, (void *)s->pr.d_best_n})
        if (p)
            hipFree(p);
    s->pr = {};
}

static void pointwise_tail_free(apemost_hip_sampler *s) {
    for (void *p : {(void *)s->pw.tail.d_buf, (void *)s->pw.tail.d_slots, (void *)s->pw.tail.d_thr})
        if (p)
            hipFree(p);
    s->pw.tail = {};
}

static void pointwise_free(apemost_hip_sampler *s) {
    pointwise_tail_free(s);
    for (void *p : {(void *)s->pw.d_chains, (void *)s->pw.d_x, (void *)s->pw.d_y, (void *)s->pw.d_state,
                    (void *)s->pw.d_par})
        if (p)
            hipFree(p);
    s->pw = {};
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
    summary_free(s); // (its kernels ran on copy_stream)
    peaks_free(s);
    joint_free(s);
    evidence_free(s);
    autocorr_free(s);
    predict_free(s);
    pointwise_free(s);
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

// ---- APEMOST_MODEL_USER: the user's likelihood compiled into the two-phase kernels at run time ----
// hiprtc is loaded on demand (a sampler of a built-in model never needs it).  The translation unit is
// "#include pt_kernels.h" -- the same kernel templates this library was built from -- followed by the
// user's file, which defines the two functions Model<APEMOST_MODEL_USER> calls; the four kernels a
// sampler launches, for workgroups of 1, 2, 4 and 8 wavefronts per chain (round 4: the reference's
// ladders are <= 99 chains, where one wave per chain leaves most of the chip idle), are named as template
// instantiations and fetched by their lowered names.
namespace {
struct HipRtc {
    void *lib;
    hiprtcResult (*create)(hiprtcProgram *, const char *, const char *, int, const char **, const char **);
    hiprtcResult (*destroy)(hiprtcProgram *);
    hiprtcResult (*add_name)(hiprtcProgram, const char *);
    hiprtcResult (*compile)(hiprtcProgram, int, const char **);
    hiprtcResult (*log_size)(hiprtcProgram, size_t *);
    hiprtcResult (*log)(hiprtcProgram, char *);
    hiprtcResult (*lowered)(hiprtcProgram, const char *, const char **);
    hiprtcResult (*code_size)(hiprtcProgram, size_t *);
    hiprtcResult (*code)(hiprtcProgram, char *);
};
} // namespace

static int hiprtc_load(HipRtc &r) {
    static HipRtc cached = {};
    static std::mutex once;
    std::lock_guard<std::mutex> hold(once); // (samplers may be created from several host threads)
    if (!cached.lib) {
        const char *names[] = {"libhiprtc.so", "libhiprtc.so.7", "/opt/rocm/lib/libhiprtc.so"};
        for (const char *n : names)
            if ((cached.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL)))
                break;
        if (!cached.lib)
            return fail(APEMOST_HIP_ERR_UNSUPPORTED, "a user-supplied device model needs libhiprtc.so: %s", dlerror());
        bool ok = true;
        auto sym = [&](const char *n) {
            void *p = dlsym(cached.lib, n);
            ok = ok && p;
            return p;
        };
        cached.create = (decltype(cached.create))sym("hiprtcCreateProgram");
        cached.destroy = (decltype(cached.destroy))sym("hiprtcDestroyProgram");
        cached.add_name = (decltype(cached.add_name))sym("hiprtcAddNameExpression");
        cached.compile = (decltype(cached.compile))sym("hiprtcCompileProgram");
        cached.log_size = (decltype(cached.log_size))sym("hiprtcGetProgramLogSize");
        cached.log = (decltype(cached.log))sym("hiprtcGetProgramLog");
        cached.lowered = (decltype(cached.lowered))sym("hiprtcGetLoweredName");
        cached.code_size = (decltype(cached.code_size))sym("hiprtcGetCodeSize");
        cached.code = (decltype(cached.code))sym("hiprtcGetCode");
        if (!ok) {
            cached.lib = nullptr;
            return fail(APEMOST_HIP_ERR_UNSUPPORTED, "libhiprtc.so lacks an expected entry point");
        }
    }
    r = cached;
    return APEMOST_HIP_OK;
}

// where this library's kernel headers are: csrc/ beside the .so, include/ one level up (in-tree
// layout), or APEMOST_HIP_SOURCE_DIR / APEMOST_HIP_INCLUDE_DIR
static void source_dirs(std::string &csrc, std::string &inc) {
    Dl_info info;
    std::string dir = ".";
    if (dladdr((const void *)&apemost_hip_abi_version, &info) && info.dli_fname) {
        dir = info.dli_fname;
        const size_t slash = dir.rfind('/');
        dir = slash == std::string::npos ? "." : dir.substr(0, slash);
    }
    const char *e1 = getenv("APEMOST_HIP_SOURCE_DIR"), *e2 = getenv("APEMOST_HIP_INCLUDE_DIR");
    csrc = e1 ? e1 : dir + "/csrc";
    inc = e2 ? e2 : dir + "/../include";
}

// a compiled user model: the code object and the lowered names of its four kernels.  Kept per process
// and keyed by (source text, kernel variant, device architecture): a host creates several samplers per
// phase (the one that checks the device model against the host plugin, one per shard, the one-chain
// twin of the single-chain API) and compiles once.
namespace {
constexpr int kUserShapes = 4;
constexpr int kUserWaves[kUserShapes] = {1, 2, 4, 8};
constexpr int kUserObShapes = 2; // APEMOST_HIP_FLAG_USER_ONE_BARRIER: likelihood waves of the one-barrier kernels
constexpr int kUserObWaves[kUserObShapes] = {4, 8};
struct UserModelCode {
    std::string key;
    std::vector<char> code;
    std::string lowered[4 * kUserShapes];
    std::string lowered_ob[2 * kUserObShapes]; // round, calibration ("": not compiled)
    double compile_seconds;
};
std::vector<UserModelCode> g_user_models;
std::mutex g_user_models_lock;
} // namespace

static int user_model_load(apemost_hip_sampler *s, const UserModelCode &m) {
    HIP_TRY(hipModuleLoadData(&s->user.module, m.code.data()));
    {
        // the headers hiprtc compiled are the ones this library was built from
        hipDeviceptr_t sym = nullptr;
        size_t bytes = 0;
        unsigned long long theirs = 0;
        if (hipModuleGetGlobal(&sym, &bytes, s->user.module, "apemost_rtc_fingerprint") != hipSuccess || bytes != sizeof theirs)
            return fail(APEMOST_HIP_ERR_RUNTIME, "the compiled device model has no layout fingerprint: kernel headers older than this library?");
        HIP_TRY(hipMemcpyDtoH(&theirs, sym, sizeof theirs));
        if (theirs != kAbiFingerprint)
            return fail(APEMOST_HIP_ERR_RUNTIME,
                        "the kernel headers compiled for the device model (APEMOST_HIP_SOURCE_DIR, or csrc/ beside the library) "
                        "do not match this library: layout fingerprint %llx, library %llx", theirs, kAbiFingerprint);
    }
    for (int k = 0; k < kUserShapes; k++) {
        const int w = kUserWaves[k];
        HIP_TRY(hipModuleGetFunction(&s->user.round[w], s->user.module, m.lowered[4 * k + 0].c_str()));
        HIP_TRY(hipModuleGetFunction(&s->user.calibrate[w], s->user.module, m.lowered[4 * k + 1].c_str()));
        HIP_TRY(hipModuleGetFunction(&s->user.calc_model[w], s->user.module, m.lowered[4 * k + 2].c_str()));
        HIP_TRY(hipModuleGetFunction(&s->user.loglike[w], s->user.module, m.lowered[4 * k + 3].c_str()));
    }
    for (int k = 0; k < kUserObShapes; k++) {
        const int w = kUserObWaves[k];
        if (!m.lowered_ob[2 * k + 0].empty())
            HIP_TRY(hipModuleGetFunction(&s->user.round_ob[w], s->user.module, m.lowered_ob[2 * k + 0].c_str()));
        if (!m.lowered_ob[2 * k + 1].empty())
            HIP_TRY(hipModuleGetFunction(&s->user.calibrate_ob[w], s->user.module, m.lowered_ob[2 * k + 1].c_str()));
    }
    s->user_compile_seconds = m.compile_seconds;
    return APEMOST_HIP_OK;
}

static int user_model_build(apemost_hip_sampler *s) {
    HipRtc rtc;
    int rc = hiprtc_load(rtc);
    if (rc)
        return rc;
    FILE *f = fopen(s->cfg.device_model_source, "rb");
    if (!f)
        return fail(APEMOST_HIP_ERR_INVALID, "device model source %s: cannot be read", s->cfg.device_model_source);
    std::string user;
    char buf[4096];
    for (size_t n; (n = fread(buf, 1, sizeof buf, f)) > 0;)
        user.append(buf, n);
    fclose(f);
    std::string csrc, inc;
    source_dirs(csrc, inc);
    std::string shown; // the path as a C string literal (#line): backslashes and quotes escaped
    for (const char *q = s->cfg.device_model_source; *q; q++) {
        if (*q == '\\' || *q == '"')
            shown += '\\';
        if (*q != '\n' && *q != '\r')
            shown += *q;
    }
    const std::string src = "#define APEMOST_USER_MODEL 1\n#include \"pt_kernels.h\"\n#line 1 \"" + shown + "\"\n" + user + "\n";
    s->user_source = user; // (user_analysis compiles the same text, whatever becomes of the file)
    s->user_shown = shown;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, s->cfg.device)); // (before the program exists: nothing to release on failure)
    hiprtcProgram prog = nullptr;
    if (rtc.create(&prog, src.c_str(), "apemost_user_model.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return fail(APEMOST_HIP_ERR_RUNTIME, "hiprtcCreateProgram failed");
    char names[4 * kUserShapes][128];
    const int km = s->kmodel, base = APEMOST_MODEL_USER;
    for (int k = 0; k < kUserShapes; k++) {
        const int w = kUserWaves[k];
        const char *prod = has_producer(w) ? "true" : "false";
        snprintf(names[4 * k + 0], sizeof names[0], "apemost::pt_round_kernel<%d, %d, false, %s>", km, w, prod);
        snprintf(names[4 * k + 1], sizeof names[0], "apemost::pt_calibrate_kernel<%d, %d, false, %s>", km, w, prod);
        snprintf(names[4 * k + 2], sizeof names[0], "apemost::pt_calc_model_kernel<%d, %d, false>", base, w);
        snprintf(names[4 * k + 3], sizeof names[0], "apemost::pt_loglike_kernel<%d, %d, false>", base, w);
    }
    for (auto &n : names)
        rtc.add_name(prog, n);
    // APEMOST_HIP_FLAG_USER_ONE_BARRIER: the one-barrier round kernels, and the calibration kernels where the
    // calibration takes them (the default proposal law and swap schedule: calib_shape)
    const bool ob = (s->cfg.flags & APEMOST_HIP_FLAG_USER_ONE_BARRIER) != 0;
    char names_ob[2 * kUserObShapes][128] = {};
    for (int k = 0; ob && k < kUserObShapes; k++) {
        const int w = kUserObWaves[k];
        snprintf(names_ob[2 * k + 0], sizeof names_ob[0], "apemost::pt_round_ob_kernel<%d, %d, false, false>", km, w);
        if (km < kVariantModel)
            snprintf(names_ob[2 * k + 1], sizeof names_ob[0], "apemost::pt_calibrate_ob_kernel<%d, %d, false, false>", km, w);
    }
    for (auto &n : names_ob)
        if (n[0])
            rtc.add_name(prog, n);
    const std::string key = std::to_string(s->kmodel) + (ob ? "|ob|" : "|") + prop.gcnArchName + "|" + user;
    {
        std::lock_guard<std::mutex> hold(g_user_models_lock);
        for (const UserModelCode &m : g_user_models)
            if (m.key == key) {
                rtc.destroy(&prog);
                return user_model_load(s, m);
            }
    }
    const std::string arch = std::string("--offload-arch=") + prop.gcnArchName, i1 = "-I" + csrc, i2 = "-I" + inc;
    const char *opts[] = {arch.c_str(), "-O3", "-ffp-contract=off", "-std=c++17", i1.c_str(), i2.c_str(), "-I/opt/rocm/include"};
    const auto t_compile = std::chrono::steady_clock::now();
    const hiprtcResult cr = rtc.compile(prog, (int)(sizeof opts / sizeof opts[0]), opts);
    if (cr != HIPRTC_SUCCESS) {
        size_t n = 0;
        rtc.log_size(prog, &n);
        std::string log(n + 1, 0);
        if (n)
            rtc.log(prog, &log[0]);
        rtc.destroy(&prog);
        return fail(APEMOST_HIP_ERR_INVALID, "device model %s does not compile:\n%s", s->cfg.device_model_source, log.c_str());
    }
    UserModelCode m;
    m.key = key;
    m.compile_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_compile).count();
    size_t code_bytes = 0;
    rtc.code_size(prog, &code_bytes);
    m.code.resize(code_bytes);
    rtc.code(prog, m.code.data());
    for (int i = 0; i < 4 * kUserShapes; i++) {
        const char *low = nullptr;
        if (rtc.lowered(prog, names[i], &low) != HIPRTC_SUCCESS || !low) {
            rtc.destroy(&prog);
            return fail(APEMOST_HIP_ERR_RUNTIME, "hiprtcGetLoweredName(%s) failed", names[i]);
        }
        m.lowered[i] = low;
    }
    for (int i = 0; i < 2 * kUserObShapes; i++) {
        if (!names_ob[i][0])
            continue;
        const char *low = nullptr;
        if (rtc.lowered(prog, names_ob[i], &low) != HIPRTC_SUCCESS || !low) {
            rtc.destroy(&prog);
            return fail(APEMOST_HIP_ERR_RUNTIME, "hiprtcGetLoweredName(%s) failed", names_ob[i]);
        }
        m.lowered_ob[i] = low;
    }
    rtc.destroy(&prog);
    rc = user_model_load(s, m);
    if (rc == APEMOST_HIP_OK) {
        std::lock_guard<std::mutex> hold(g_user_models_lock);
        g_user_models.push_back(std::move(m));
    }
    return rc;
}

// ---- APEMOST_MODEL_USER: the optional hooks' kernels (pt_user_fold.h), a second run-time module ----
// Built on the first predict_* or pointwise_* call of a sampler, not at create: a run that never asks for a fold
// never pays for it.  The translation unit is user_model_build's -- the same prefix, text, options and include
// directories -- closed by '#include "pt_user_fold.h"', which defines the kernels of the hooks the text announces.
// Which hooks exist is what the module holds: the entry points are looked up by name.  Kept per process like the
// round module, keyed by (source text, device architecture, "analysis"); a text without hooks is remembered too, so
// it is compiled once and no more.
namespace {
struct UserAnalysisCode {
    std::string key;
    std::vector<char> code;
};
std::vector<UserAnalysisCode> g_user_analysis;
} // namespace

static int user_analysis_load(apemost_hip_sampler *s, const UserAnalysisCode &m) {
    HIP_TRY(hipModuleLoadData(&s->ua.module, m.code.data()));
    const struct {
        const char *name;
        unsigned long long ours;
    } prints[] = {{"apemost_rtc_fingerprint", kAbiFingerprint}, {"apemost_rtc_fold_fingerprint", kFoldFingerprint}};
    for (const auto &fp : prints) {
        // the headers hiprtc compiled are the ones this library was built from
        hipDeviceptr_t sym = nullptr;
        size_t bytes = 0;
        unsigned long long theirs = 0;
        if (hipModuleGetGlobal(&sym, &bytes, s->ua.module, fp.name) != hipSuccess || bytes != sizeof theirs)
            return fail(APEMOST_HIP_ERR_RUNTIME, "the compiled device model's hooks have no layout fingerprint: kernel headers older than this library?");
        HIP_TRY(hipMemcpyDtoH(&theirs, sym, sizeof theirs));
        if (theirs != fp.ours)
            return fail(APEMOST_HIP_ERR_RUNTIME,
                        "the kernel headers compiled for the device model's hooks (APEMOST_HIP_SOURCE_DIR, or csrc/ beside the "
                        "library) do not match this library: %s %llx, library %llx", fp.name, theirs, fp.ours);
    }
    // a hook is there when all of its kernels are (they share one #ifdef)
    auto get = [&](hipFunction_t *f, const char *name) {
        if (hipModuleGetFunction(f, s->ua.module, name) != hipSuccess)
            *f = nullptr;
        return *f != nullptr;
    };
    const bool c1 = get(&s->ua.predict_fold, "apemost_user_predict_fold"),
               c2 = get(&s->ua.predict_fold_hist, "apemost_user_predict_fold_hist"),
               c3 = get(&s->ua.predict_curve, "apemost_user_predict_curve");
    const bool p1 = get(&s->ua.pointwise_fold, "apemost_user_pointwise_fold"),
               p2 = get(&s->ua.pointwise_loglike, "apemost_user_pointwise_loglike"),
               p3 = get(&s->ua.pointwise_tail_append, "apemost_user_pointwise_tail_append");
    (void)hipGetLastError(); // (a lookup that found nothing is an answer, not an error to report later)
    s->ua.has_curve = c1 && c2 && c3;
    s->ua.has_pointwise = p1 && p2 && p3;
    return APEMOST_HIP_OK;
}

// the hooks of this sampler's model, compiled and loaded on first use
static int user_analysis(apemost_hip_sampler *s) {
    if (s->ua.ready)
        return APEMOST_HIP_OK;
    HipRtc rtc;
    int rc = hiprtc_load(rtc);
    if (rc)
        return rc;
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, s->cfg.device));
    const std::string key = std::string("analysis|") + prop.gcnArchName + "|" + s->user_source;
    {
        std::lock_guard<std::mutex> hold(g_user_models_lock);
        for (const UserAnalysisCode &m : g_user_analysis)
            if (m.key == key) {
                rc = user_analysis_load(s, m);
                s->ua.compile_seconds = 0;
                s->ua.ready = rc == APEMOST_HIP_OK;
                return rc;
            }
    }
    std::string csrc, inc;
    source_dirs(csrc, inc);
    const std::string src = "#define APEMOST_USER_MODEL 1\n#include \"pt_kernels.h\"\n#line 1 \"" + s->user_shown + "\"\n" +
                            s->user_source + "\n#include \"pt_user_fold.h\"\n";
    hiprtcProgram prog = nullptr;
    if (rtc.create(&prog, src.c_str(), "apemost_user_model.hip", 0, nullptr, nullptr) != HIPRTC_SUCCESS)
        return fail(APEMOST_HIP_ERR_RUNTIME, "hiprtcCreateProgram failed");
    const std::string arch = std::string("--offload-arch=") + prop.gcnArchName, i1 = "-I" + csrc, i2 = "-I" + inc;
    const char *opts[] = {arch.c_str(), "-O3", "-ffp-contract=off", "-std=c++17", i1.c_str(), i2.c_str(), "-I/opt/rocm/include"};
    const auto t_compile = std::chrono::steady_clock::now();
    if (rtc.compile(prog, (int)(sizeof opts / sizeof opts[0]), opts) != HIPRTC_SUCCESS) {
        size_t n = 0;
        rtc.log_size(prog, &n);
        std::string log(n + 1, 0);
        if (n)
            rtc.log(prog, &log[0]);
        rtc.destroy(&prog);
        return fail(APEMOST_HIP_ERR_INVALID, "the hooks of device model %s (include/apemost_device_model.h) do not compile:\n%s",
                    s->user_shown.c_str(), log.c_str());
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_compile).count();
    UserAnalysisCode m;
    m.key = key;
    size_t code_bytes = 0;
    rtc.code_size(prog, &code_bytes);
    m.code.resize(code_bytes);
    rtc.code(prog, m.code.data());
    rtc.destroy(&prog);
    rc = user_analysis_load(s, m);
    if (rc == APEMOST_HIP_OK) {
        s->ua.compile_seconds = seconds;
        s->ua.ready = true;
        std::lock_guard<std::mutex> hold(g_user_models_lock);
        g_user_analysis.push_back(std::move(m));
    }
    return rc;
}

// the two words per ladder a batch keeps behind its counters (DevArrays::ladder_words)
static int ladder_words_upload(apemost_hip_sampler *s) {
    std::vector<u64> w(2 * (size_t)s->n_ladders);
    for (int b = 0; b < s->n_ladders; b++) {
        w[2 * b] = s->seeds[b];
        memcpy(&w[2 * b + 1], &s->x_abs_max[b], sizeof(double));
    }
    HIP_TRY(hipMemcpyAsync(s->d.ladder_words(), w.data(), w.size() * sizeof(u64), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return APEMOST_HIP_OK;
}

// Replica flow (APEMOST_HIP_FLAG_TRACK_REPLICAS): the rung words go to the device three times -- the word the
// rung's workgroup works on and its hand-off copy in either half of the state -- so that whichever half the next
// launch reads holds them.  replica == nullptr: labels to identity and headings to the initial state, per ladder;
// zero_counters: the four counter arrays too.
static int flow_upload(apemost_hip_sampler *s, const uint32_t *replica, const uint32_t *heading, bool zero_counters) {
    const size_t n = s->cfg.n_chains, per = s->per_ladder;
    std::vector<u64> w(3 * n);
    for (size_t c = 0; c < n; c++) {
        const size_t a = c % per;
        u64 label = replica ? replica[c] : a, head = heading ? heading[c] : (per == 1 ? 0 : a == 0 ? 1 : a == per - 1 ? 2 : 0);
        w[c] = w[n + c] = w[2 * n + c] = label << 2 | head;
    }
    HIP_TRY(hipMemcpyAsync(s->d.flow_word(), w.data(), w.size() * sizeof(u64), hipMemcpyHostToDevice, s->stream));
    if (zero_counters)
        HIP_TRY(hipMemsetAsync(s->d.flow_up(), 0, 4 * n * sizeof(u64), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return APEMOST_HIP_OK;
}

// the part of apemost_hip_create that can fail after the sampler object exists
static int create_body(apemost_hip_sampler *s) {
    const apemost_hip_config *cfg = &s->cfg;
    int rc;
    // waves 1-3 produce the proposal candidates in the serial window of each step
    s->producers = has_producer(s->waves);
    if (s->waves != 1 && s->waves != 2 && s->waves != 4 && s->waves != 6 && s->waves != 8)
        return fail(APEMOST_HIP_ERR_INVALID, "waves_per_chain must be 1, 2, 4, 6 or 8");
    const size_t fixed_lds = (kFixedLdsDoubles + (size_t)cand_slots(s->waves) * 2 * kWave) * sizeof(double);
    const size_t data_lds = (size_t)2 * cfg->n_data * sizeof(double);
    const size_t fixed_max = fixed_lds > kObFixedDoubles * sizeof(double) ? fixed_lds : kObFixedDoubles * sizeof(double);
    s->lds_data = fixed_max + data_lds <= 160 * 1024 - 1024 && cfg->lds_policy != 2 && cfg->model != APEMOST_MODEL_USER &&
                  (cfg->lds_policy == 1 || choose_lds(*cfg, fixed_lds + data_lds));
    s->lds_bytes = fixed_lds + (s->lds_data ? data_lds : 0);
    s->lds_fixed_bytes = fixed_lds;
    HIP_TRY(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
    HIP_TRY(hipEventCreate(&s->ev0));
    HIP_TRY(hipEventCreate(&s->ev1));

    DevArrays &d = s->d;
    d.n = cfg->n_chains;
    d.np = cfg->n_par;
    double *data = nullptr;
    if ((rc = dev_alloc(s, &d.f, d.f_count())) || (rc = dev_alloc(s, &d.u, d.u_count() + (s->track ? d.flow_count() : s->batch ? 2 * (size_t)s->n_ladders : 0))) ||
        (rc = dev_alloc(s, &data, (size_t)cfg->n_cols * cfg->n_data * s->n_ladders)))
        return rc;
    d.data = data;
    if (s->batch && (rc = ladder_words_upload(s)))
        return rc;
    if (s->track && (rc = flow_upload(s, nullptr, nullptr, true)))
        return rc;

    s->sh.n_par = cfg->n_par;
    s->sh.n_data = cfg->n_data;
    s->sh.n_chains = cfg->n_chains;
    s->sh.chain_offset = cfg->chain_offset;
    s->sh.n_global = s->batch ? s->per_ladder : cfg->n_chains_global;
    s->sh.seed = cfg->seed;
    s->sh.consts.sigma = cfg->sigma;
    s->sh.consts.hmin = cfg->hmin;
    s->sh.circular = cfg->circular_params;
    if (cfg->flags & APEMOST_HIP_FLAG_PROPOSAL_LOGISTIC)
        s->sh.circular |= (u64)kProposalLogistic << kProposalShift;
    if (cfg->flags & APEMOST_HIP_FLAG_PROPOSAL_UNIFORM)
        s->sh.circular |= (u64)kProposalFlat << kProposalShift;
    s->sh.variant = (cfg->flags & APEMOST_HIP_FLAG_RANDOMSWAP) ? kVariantRandomSwap : 0;
    s->sh.variant |= (int)((unsigned)cfg->n_cols << 16);
    if (cfg->flags & APEMOST_HIP_FLAG_TEST_WITHHOLD_PUBLISH)
        s->sh.variant |= kVariantTestWithhold;
    if (cfg->flags & APEMOST_HIP_FLAG_SWAP_EVEN_ODD)
        s->sh.variant |= kVariantEvenOdd;
    if (s->batch)
        s->sh.variant |= kVariantBatch;
    if (s->track)
        s->sh.variant |= kVariantTrack;
    s->kmodel = cfg->model + (((cfg->flags & (APEMOST_HIP_FLAG_PROPOSAL_LOGISTIC | APEMOST_HIP_FLAG_PROPOSAL_UNIFORM |
                                              APEMOST_HIP_FLAG_RANDOMSWAP | APEMOST_HIP_FLAG_SWAP_EVEN_ODD |
                                              APEMOST_HIP_FLAG_TRACK_REPLICAS)) || s->batch)
                                  ? kVariantModel
                                  : 0);
    s->sh.x_abs_max = INFINITY; // until set_data
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (cfg->model == APEMOST_MODEL_USER && (rc = user_model_build(s)))
        return rc;
    if ((rc = enable_big_lds(s, s->waves)))
        return rc;
    {
        // Multi-round launches need every workgroup resident at once.  Blocks per CU from the
        // occupancy query, one held back (the query over-reports by one block for scalar-register-
        // heavy kernels: MI355X_MICROARCH.md "Residency and cooperative launch").
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, cfg->device));
        // the round kernel this sampler's stepping launches use: one barrier per step where that
        // variant exists (8 likelihood waves per chain), the classic two-phase step otherwise
        s->one_barrier = has_one_barrier(s->waves) && !(cfg->flags & APEMOST_HIP_FLAG_TWO_BARRIER_STEP) && user_may_ob(s);
        s->cus = prop.multiProcessorCount;
        s->ob_helper = s->one_barrier && ob_wants_helper(s, cfg->n_chains);
        s->betas_split_ok = true;
        int b_lds = 0, b_plain = 0;
        if (s->user.module && s->one_barrier) {
            HIP_TRY(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&b_plain, s->user.round_ob[s->waves], ob_block(s->waves, false),
                                                                       ob_lds_bytes(s, false)));
        } else if (s->user.module) {
            HIP_TRY(hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&b_plain, s->user.round[s->waves], s->waves * kWave, s->lds_fixed_bytes));
        } else {
        if (s->lds_data)
            HIP_TRY(round_occupancy<true>(s->kmodel, s->waves, s->producers, s->one_barrier, s->ob_helper,
                                          s->one_barrier ? ob_lds_bytes(s, true) : s->lds_bytes, &b_lds));
        HIP_TRY(round_occupancy<false>(s->kmodel, s->waves, s->producers, s->one_barrier, s->ob_helper,
                                       s->one_barrier ? ob_lds_bytes(s, false) : s->lds_fixed_bytes, &b_plain));
        }
        const long long cus = prop.multiProcessorCount;
        s->resident_lds = s->lds_data && (long long)cfg->n_chains <= (long long)(b_lds - 1) * cus;
        s->resident_plain = (long long)cfg->n_chains <= (long long)(b_plain - 1) * cus;
        if (s->ob_helper) {
            // Workgroups with a helper wavefront are chosen for ladders of at most one chain per CU (ob_wants_helper)
            // and a CU admits one of them or two: a kernel that launches at all has a workgroup per CU resident,
            // whatever the occupancy query's last block is worth.
            s->resident_lds = s->lds_data && b_lds >= 1;
            s->resident_plain = b_plain >= 1;
        }
        if ((long long)cfg->n_chains * 2 <= cus) { // at most one workgroup per two CUs
            s->resident_lds = s->lds_data;
            s->resident_plain = true;
        }
        s->resident_ok = s->resident_lds || s->resident_plain;
        s->cooperative = (cfg->flags & APEMOST_HIP_FLAG_COOPERATIVE_LAUNCH) && prop.cooperativeLaunch && !s->user.module;
        // (APEMOST_COOP_ANY=1: the same for the two-phase kernels -- an experiment switch, tools/experiments/r04_session6.sh)
        if (!s->resident_ok && prop.cooperativeLaunch && (s->one_barrier || getenv("APEMOST_COOP_ANY")) && !s->user.module) {
            // (the one-barrier kernels only: their steps take a microsecond and a launch per round
            // costs a multiple of that; 2048 one-wave chains of config 5 would fit too, but a round
            // there is a 340 us launch and the in-launch hand-off was measured 3 % behind)
            // Between the cautious estimate and the occupancy figure itself (e.g. 257-512 chains of
            // eight-wave workgroups, two per CU) the runtime decides: multi-round launches go through
            // hipLaunchCooperativeKernel, which places the whole grid or refuses -- and a refusal
            // turns this sampler to one round per launch (apemost_hip_run retries, see there).
            const bool fits_lds = s->lds_data && (long long)cfg->n_chains <= (long long)b_lds * cus;
            const bool fits_plain = (long long)cfg->n_chains <= (long long)b_plain * cus;
            if (fits_lds || fits_plain) {
                s->resident_lds = fits_lds;
                s->resident_plain = fits_plain;
                s->resident_ok = true;
                s->cooperative = true;
            }
        }
        // -DADAPT: adapt() sits between a round's steps and its swap attempt and runs as a launch
        // of its own (pt_adapt_kernel), so every round is a launch
        if (cfg->flags & (APEMOST_HIP_FLAG_SINGLE_ROUND_LAUNCHES | APEMOST_HIP_FLAG_ADAPT | APEMOST_HIP_FLAG_RWM))
            s->resident_ok = false;
    }
    return APEMOST_HIP_OK;
}

// seeds == nullptr: an ordinary sampler; else a batch of n_ladders ladders of per_ladder chains, *cfg already
// describing the whole grid (apemost_hip_create_batch)
static int create_impl(const apemost_hip_config *cfg, int n_ladders, int per_ladder, const uint64_t *seeds,
                       apemost_hip_sampler **out) {
    if (cfg->abi_version != APEMOST_HIP_ABI_VERSION)
        return fail(APEMOST_HIP_ERR_INVALID, "ABI version %d, library has %d", cfg->abi_version,
                    APEMOST_HIP_ABI_VERSION);
    if (cfg->n_par < 1 || cfg->n_par > APEMOST_HIP_MAX_PAR)
        return fail(APEMOST_HIP_ERR_INVALID, "n_par %d outside [1,%d]", cfg->n_par, APEMOST_HIP_MAX_PAR);
    if (cfg->n_chains < 1 || cfg->n_data < 1 || cfg->n_cols < 2)
        return fail(APEMOST_HIP_ERR_INVALID, "n_chains %d, n_data %d, n_cols %d invalid", cfg->n_chains,
                    cfg->n_data, cfg->n_cols);
    if (cfg->n_cols > 65535)
        return fail(APEMOST_HIP_ERR_INVALID, "n_cols %d: at most 65535 data columns", cfg->n_cols);
    if (cfg->chain_offset < 0 || cfg->chain_offset + cfg->n_chains > cfg->n_chains_global)
        return fail(APEMOST_HIP_ERR_INVALID, "shard [%lld,%lld) outside ladder of %lld chains",
                    (long long)cfg->chain_offset, (long long)(cfg->chain_offset + cfg->n_chains),
                    (long long)cfg->n_chains_global);
    if (cfg->n_par < 64 && (cfg->circular_params >> cfg->n_par) != 0)
        return fail(APEMOST_HIP_ERR_INVALID, "circular_params names a parameter beyond n_par");
    if (cfg->flags & ~(APEMOST_HIP_FLAG_SINGLE_ROUND_LAUNCHES | APEMOST_HIP_FLAG_COOPERATIVE_LAUNCH |
                       APEMOST_HIP_FLAG_TWO_BARRIER_STEP | APEMOST_HIP_FLAG_PROPOSAL_LOGISTIC |
                       APEMOST_HIP_FLAG_PROPOSAL_UNIFORM | APEMOST_HIP_FLAG_RANDOMSWAP | APEMOST_HIP_FLAG_ADAPT |
                       APEMOST_HIP_FLAG_TEST_REFUSE_COOPERATIVE | APEMOST_HIP_FLAG_TEST_WITHHOLD_PUBLISH | APEMOST_HIP_FLAG_RWM |
                       APEMOST_HIP_FLAG_USER_ONE_BARRIER | APEMOST_HIP_FLAG_SWAP_EVEN_ODD | APEMOST_HIP_FLAG_TRACK_REPLICAS))
        return fail(APEMOST_HIP_ERR_INVALID, "unknown bits in flags: 0x%x", (unsigned)cfg->flags);
    // (seeds: a batch, whose create_batch has refused sharding already and whose *cfg describes the whole grid)
    if ((cfg->flags & APEMOST_HIP_FLAG_TRACK_REPLICAS) && !seeds && (cfg->chain_offset != 0 || cfg->n_chains_global != cfg->n_chains))
        return fail(APEMOST_HIP_ERR_UNSUPPORTED,
                    "TRACK_REPLICAS: replica flow is not tracked over a sharded ladder (chain_offset %lld, n_chains_global %lld, "
                    "n_chains %d)", (long long)cfg->chain_offset, (long long)cfg->n_chains_global, cfg->n_chains);
    if ((cfg->flags & APEMOST_HIP_FLAG_SWAP_EVEN_ODD) &&
        (cfg->flags & (APEMOST_HIP_FLAG_RANDOMSWAP | APEMOST_HIP_FLAG_TEST_WITHHOLD_PUBLISH)))
        return fail(APEMOST_HIP_ERR_INVALID, "SWAP_EVEN_ODD excludes RANDOMSWAP and TEST_WITHHOLD_PUBLISH");
    if ((cfg->flags & APEMOST_HIP_FLAG_PROPOSAL_LOGISTIC) && (cfg->flags & APEMOST_HIP_FLAG_PROPOSAL_UNIFORM))
        return fail(APEMOST_HIP_ERR_INVALID, "PROPOSAL_LOGISTIC and PROPOSAL_UNIFORM are alternatives");
    if (!(cfg->adapt_target >= 0 && cfg->adapt_target < 1e300))
        return fail(APEMOST_HIP_ERR_INVALID, "adapt_target %g invalid", cfg->adapt_target);
    if (cfg->n_chains_global > 2000000)
        return fail(APEMOST_HIP_ERR_INVALID, "n_beta*1000 must fit an int (interaction.c:92)");
    switch (cfg->model) {
    case APEMOST_MODEL_SIMPLESIN:
        if (cfg->n_par != 4)
            return fail(APEMOST_HIP_ERR_INVALID, "simplesin needs n_par = 4");
        break;
    case APEMOST_MODEL_SINE3:
        if (cfg->n_par != 10)
            return fail(APEMOST_HIP_ERR_INVALID, "sine3 needs n_par = 10");
        break;
    case APEMOST_MODEL_PULSE:
        if (cfg->n_par < 4 || (cfg->n_par - 2) % 2 != 0)
            return fail(APEMOST_HIP_ERR_INVALID, "pulse needs n_par = 2 + 2*modes");
        break;
    case APEMOST_MODEL_PULSE_VROT:
        if (cfg->n_par != 7)
            return fail(APEMOST_HIP_ERR_INVALID, "pulse_vrot needs n_par = 7");
        break;
    case APEMOST_MODEL_USER:
        if (!cfg->device_model_source || !*cfg->device_model_source)
            return fail(APEMOST_HIP_ERR_INVALID, "APEMOST_MODEL_USER needs device_model_source (include/apemost_device_model.h)");
        if (cfg->lds_policy == 1)
            return fail(APEMOST_HIP_ERR_INVALID, "a user-supplied model reads the data rows by index, through L2: they are not staged in LDS");
        if (cfg->waves_per_chain == 6)
            return fail(APEMOST_HIP_ERR_INVALID, "a user-supplied device model runs with 1, 2, 4 or 8 waves per chain");
        break;
    default:
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "unknown device model %d", cfg->model);
    }
    if (cfg->model != APEMOST_MODEL_USER && cfg->device_model_source)
        return fail(APEMOST_HIP_ERR_INVALID, "device_model_source is for APEMOST_MODEL_USER only");
    if (cfg->model != APEMOST_MODEL_USER && (cfg->flags & APEMOST_HIP_FLAG_USER_ONE_BARRIER))
        return fail(APEMOST_HIP_ERR_INVALID, "APEMOST_HIP_FLAG_USER_ONE_BARRIER is for APEMOST_MODEL_USER only");
    int rc = apemost_hip_device_info(cfg->device, nullptr, 0, nullptr, nullptr);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipSetDevice(cfg->device));

    apemost_hip_sampler *s = new apemost_hip_sampler();
    s->cfg = *cfg;
    s->cur = 0;
    s->round = 0;
    s->swap_pending = 0;
    s->launches = 0;
    s->launches_at_begin = 0;
    s->cal = {};
    memset(&s->user, 0, sizeof s->user);
    s->big_lds_set = 0;
    s->stream = nullptr;
    s->ev0 = s->ev1 = nullptr;
    s->copy_stream = nullptr;
    s->ev_copy = nullptr;
    for (int k = 0; k < 2; k++) {
        s->edge_out[k] = s->edge_in[k] = nullptr;
        s->ev_exported[k] = s->ev_imported[k] = nullptr;
    }
    s->h_word = nullptr;
    s->handoff_failed = false;
    s->waves = choose_waves(*cfg);
    s->user_compile_seconds = 0;
    s->rwm_keep = nullptr;
    s->in_rwm = false;
    s->sum = {};
    s->batch = seeds != nullptr;
    s->track = (cfg->flags & APEMOST_HIP_FLAG_TRACK_REPLICAS) != 0;
    s->n_ladders = n_ladders;
    s->per_ladder = per_ladder;
    if (seeds) {
        s->seeds.assign(seeds, seeds + n_ladders);
        s->x_abs_max.assign(n_ladders, INFINITY); // until set_data
    }
    if (s->waves == 6 && (s->batch || (cfg->flags & (APEMOST_HIP_FLAG_PROPOSAL_LOGISTIC | APEMOST_HIP_FLAG_PROPOSAL_UNIFORM |
                                                     APEMOST_HIP_FLAG_RANDOMSWAP | APEMOST_HIP_FLAG_SWAP_EVEN_ODD |
                                                     APEMOST_HIP_FLAG_TRACK_REPLICAS)))) {
        delete s;
        return fail(APEMOST_HIP_ERR_INVALID, "the proposal / swap variants and ladder batches are built for 1, 2, 4 or 8 waves per chain");
    }
    rc = create_body(s);
    if (rc != APEMOST_HIP_OK) {
        release(s); // the stream, the events and every allocation made so far
        return rc;
    }
    *out = s;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_create(const apemost_hip_config *cfg, apemost_hip_sampler **out) {
    if (!cfg || !out)
        return fail(APEMOST_HIP_ERR_INVALID, "cfg/out is NULL");
    *out = nullptr;
    return create_impl(cfg, 1, cfg->n_chains, nullptr, out);
}

// A ladder batch: what it cannot do is refused here, before any device is touched, so that nothing runs
// silently as a single ladder (the list: include/apemost_hip.h).
extern "C" int apemost_hip_create_batch(const apemost_hip_config *cfg, int32_t n_ladders, const uint64_t *seeds,
                                        apemost_hip_sampler **out) {
    if (!cfg || !out)
        return fail(APEMOST_HIP_ERR_INVALID, "cfg/out is NULL");
    *out = nullptr;
    if (!seeds || n_ladders < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "create_batch: n_ladders %d needs that many seeds", n_ladders);
    if (cfg->abi_version != APEMOST_HIP_ABI_VERSION)
        return fail(APEMOST_HIP_ERR_INVALID, "ABI version %d, library has %d", cfg->abi_version, APEMOST_HIP_ABI_VERSION);
    if (cfg->model == APEMOST_MODEL_USER)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "create_batch: a user-supplied device model does not run in ladder batches");
    const struct {
        int bit;
        const char *name;
    } refused[] = {{APEMOST_HIP_FLAG_RANDOMSWAP, "RANDOMSWAP"},
                   {APEMOST_HIP_FLAG_ADAPT, "ADAPT"},
                   {APEMOST_HIP_FLAG_RWM, "RWM"},
                   {APEMOST_HIP_FLAG_TEST_REFUSE_COOPERATIVE, "TEST_REFUSE_COOPERATIVE"},
                   {APEMOST_HIP_FLAG_TEST_WITHHOLD_PUBLISH, "TEST_WITHHOLD_PUBLISH"},
                   {APEMOST_HIP_FLAG_COOPERATIVE_LAUNCH, "COOPERATIVE_LAUNCH"},
                   {APEMOST_HIP_FLAG_USER_ONE_BARRIER, "USER_ONE_BARRIER"}};
    for (const auto &r : refused)
        if (cfg->flags & r.bit)
            return fail(APEMOST_HIP_ERR_UNSUPPORTED, "create_batch: APEMOST_HIP_FLAG_%s does not run in ladder batches", r.name);
    if (cfg->chain_offset != 0 || cfg->n_chains_global != cfg->n_chains)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED,
                    "create_batch: ladder batches are not sharded (chain_offset %lld, n_chains_global %lld, n_chains %d)",
                    (long long)cfg->chain_offset, (long long)cfg->n_chains_global, cfg->n_chains);
    if (cfg->n_chains < 1 || (long long)cfg->n_chains * n_ladders > 2000000)
        return fail(APEMOST_HIP_ERR_INVALID, "create_batch: %d ladders of %d chains: 1 .. 2000000 chains in all", n_ladders,
                    cfg->n_chains);
    apemost_hip_config grid = *cfg; // the whole grid: what the geometry, the residency check and every view index
    grid.n_chains = cfg->n_chains * n_ladders;
    grid.n_chains_global = grid.n_chains;
    grid.seed = seeds[0];
    return create_impl(&grid, n_ladders, cfg->n_chains, seeds, out);
}

extern "C" int apemost_hip_n_ladders(apemost_hip_sampler *s, int32_t *n_ladders) {
    if (!s || !n_ladders)
        return fail(APEMOST_HIP_ERR_INVALID, "sampler / n_ladders is NULL");
    *n_ladders = s->n_ladders;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_destroy(apemost_hip_sampler *s) {
    if (!s)
        return APEMOST_HIP_OK;
    hipSetDevice(s->cfg.device);
    release(s);
    return APEMOST_HIP_OK;
}

#define CHECK_S(s)                                                                               \
    do {                                                                                         \
        if (!(s))                                                                                \
            return fail(APEMOST_HIP_ERR_INVALID, "sampler is NULL");                             \
        HIP_TRY(hipSetDevice((s)->cfg.device));                                                  \
    } while (0)

// Words the kernels raise instead of spinning for ever: 1 = an in-launch swap hand-off timed out (a
// partner workgroup was not resident), 2 = an in-launch swap picked a pair that straddles the shard,
// 3 = a proposal found no point inside [min,max] in 2^24 attempts.  The results of that launch are
// void.  The word is cleared here so that the sampler can be reloaded (set_state) and used again;
// after a hand-off timeout it only issues single-round launches, which never wait for anybody.
static int check_handoff(apemost_hip_sampler *s) {
    u64 word = 0;
    HIP_TRY(hipMemcpyAsync(&word, s->d.timeout_word(), sizeof word, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (word == 0)
        return APEMOST_HIP_OK;
    HIP_TRY(hipMemsetAsync(s->d.timeout_word(), 0, sizeof(u64), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (word == 1)
        s->handoff_failed = true;
    return fail(APEMOST_HIP_ERR_RUNTIME, "%s (code %llu): the results of that launch are void%s",
                word == 3 ? "a proposal found no point inside its prior box"
                          : "in-launch swap hand-off failed",
                (unsigned long long)word, word == 1 ? "; falling back to one round per launch" : "");
}

extern "C" int apemost_hip_synchronize(apemost_hip_sampler *s) {
    CHECK_S(s);
    HIP_TRY(hipStreamSynchronize(s->stream));
    return check_handoff(s);
}

extern "C" int apemost_hip_stream(apemost_hip_sampler *s, void **stream) {
    CHECK_S(s);
    if (!stream)
        return fail(APEMOST_HIP_ERR_INVALID, "stream is NULL");
    *stream = (void *)s->stream;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_waves_per_chain(apemost_hip_sampler *s, int *waves, int *data_in_lds) {
    CHECK_S(s);
    if (waves)
        *waves = s->waves;
    if (data_in_lds)
        *data_in_lds = s->lds_data ? 1 : 0;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_user_model_compile_seconds(apemost_hip_sampler *s, double *seconds) {
    CHECK_S(s);
    if (!s->user.module || !seconds)
        return fail(APEMOST_HIP_ERR_INVALID, "not a sampler of a user-supplied device model");
    *seconds = s->user_compile_seconds;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_user_hooks(apemost_hip_sampler *s, int32_t *has_curve, int32_t *has_pointwise,
                                      double *compile_seconds) {
    CHECK_S(s);
    if (!s->user.module)
        return fail(APEMOST_HIP_ERR_INVALID, "not a sampler of a user-supplied device model");
    const int rc = user_analysis(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    if (has_curve)
        *has_curve = s->ua.has_curve ? 1 : 0;
    if (has_pointwise)
        *has_pointwise = s->ua.has_pointwise ? 1 : 0;
    if (compile_seconds)
        *compile_seconds = s->ua.compile_seconds;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_launch_policy(apemost_hip_sampler *s, int32_t *one_barrier, int32_t *cooperative,
                                         int32_t *max_rounds) {
    CHECK_S(s);
    if (one_barrier)
        *one_barrier = s->one_barrier ? (s->ob_helper && s->betas_split_ok ? 2 : 1) : 0;
    if (cooperative)
        *cooperative = (s->cooperative && s->resident_ok && !s->handoff_failed) ? 1 : 0;
    if (max_rounds)
        *max_rounds = max_rounds_per_launch(s);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_set_chain_offset(apemost_hip_sampler *s, int64_t chain_offset) {
    CHECK_S(s);
    if (s->batch)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "set_chain_offset: ladder batches are not sharded");
    if (s->track)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "set_chain_offset: replica flow is not tracked over a sharded ladder");
    if (chain_offset < 0 || chain_offset + s->cfg.n_chains > s->cfg.n_chains_global)
        return fail(APEMOST_HIP_ERR_INVALID, "chain offset %lld outside the ladder", (long long)chain_offset);
    s->cfg.chain_offset = chain_offset;
    s->sh.chain_offset = chain_offset;
    return APEMOST_HIP_OK;
}

// ladder < 0: every ladder gets the matrix
static int set_data_impl(apemost_hip_sampler *s, int ladder, const double *data_rowmajor) {
    if (!data_rowmajor)
        return fail(APEMOST_HIP_ERR_INVALID, "data is NULL");
    const int n = s->cfg.n_data, nc = s->cfg.n_cols;
    std::vector<double> col((size_t)n * nc);
    double x_abs_max = 0;
    for (int i = 0; i < n; i++) {
        for (int j = 0; j < nc; j++)
            col[(size_t)j * n + i] = data_rowmajor[(size_t)i * nc + j];
        const double ax = std::fabs(data_rowmajor[(size_t)i * nc]);
        if (!(ax <= x_abs_max)) // also catches NaN
            x_abs_max = std::isfinite(ax) ? ax : INFINITY;
    }
    for (int b = ladder < 0 ? 0 : ladder; b < (ladder < 0 ? s->n_ladders : ladder + 1); b++) {
        HIP_TRY(hipMemcpyAsync((void *)(s->d.data + (size_t)b * col.size()), col.data(), col.size() * sizeof(double),
                               hipMemcpyHostToDevice, s->stream));
        if (s->batch)
            s->x_abs_max[b] = x_abs_max;
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (!s->batch) {
        s->sh.x_abs_max = x_abs_max;
        return APEMOST_HIP_OK;
    }
    // (the batch kernels take each ladder's own figure from its ladder words; the shared one is the largest)
    s->sh.x_abs_max = 0;
    for (double x : s->x_abs_max)
        if (!(x <= s->sh.x_abs_max))
            s->sh.x_abs_max = x;
    return ladder_words_upload(s);
}

extern "C" int apemost_hip_set_data(apemost_hip_sampler *s, const double *data_rowmajor) {
    CHECK_S(s);
    return set_data_impl(s, -1, data_rowmajor);
}

extern "C" int apemost_hip_set_data_ladder(apemost_hip_sampler *s, int32_t ladder, const double *data_rowmajor) {
    CHECK_S(s);
    if (ladder < 0 || ladder >= s->n_ladders)
        return fail(APEMOST_HIP_ERR_INVALID, "set_data_ladder: ladder %d outside [0,%d)", ladder, s->n_ladders);
    return set_data_impl(s, ladder, data_rowmajor);
}

// copy one [n_chains][width] field between host and the interior rows of a device array
template <class T>
static int xfer(apemost_hip_sampler *s, T *dev, T *host, size_t width, bool rows_layout, bool to_device) {
    if (!host)
        return APEMOST_HIP_OK;
    T *p = dev + (rows_layout ? width : 0);
    const size_t bytes = (size_t)s->cfg.n_chains * width * sizeof(T);
    if (to_device)
        HIP_TRY(hipMemcpyAsync(p, host, bytes, hipMemcpyHostToDevice, s->stream));
    else
        HIP_TRY(hipMemcpyAsync(host, p, bytes, hipMemcpyDeviceToHost, s->stream));
    return APEMOST_HIP_OK;
}

static int xfer_state(apemost_hip_sampler *s, const apemost_hip_state_view *v, bool up) {
    CHECK_S(s);
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "state view is NULL");
    const size_t np = s->cfg.n_par;
    const int h = s->cur;
    DevArrays &d = s->d;
    int rc;
    if ((rc = xfer(s, d.params(h), v->params, np, true, up)) ||
        (rc = xfer(s, d.params_best(h), v->params_best, np, true, up)) ||
        (rc = xfer(s, d.prob(h), v->prob, 1, true, up)) ||
        (rc = xfer(s, d.prob_best(h), v->prob_best, 1, true, up)) ||
        (rc = xfer(s, d.prior(h), v->prior, 1, true, up)) || (rc = xfer(s, d.beta(), v->beta, 1, true, up)) ||
        (rc = xfer(s, d.step(), v->step, np, false, up)) || (rc = xfer(s, d.pmin(), v->pmin, np, false, up)) ||
        (rc = xfer(s, d.pmax(), v->pmax, np, false, up)) ||
        (rc = xfer(s, (uint64_t *)d.params_accepts(), v->params_accepts, np, false, up)) ||
        (rc = xfer(s, (uint64_t *)d.params_rejects(), v->params_rejects, np, false, up)) ||
        (rc = xfer(s, (uint64_t *)d.accept(), v->accept, 1, false, up)) ||
        (rc = xfer(s, (uint64_t *)d.reject(), v->reject, 1, false, up)) ||
        (rc = xfer(s, (uint64_t *)d.n_iter(), v->n_iter, 1, false, up)) ||
        (rc = xfer(s, (uint64_t *)d.swapcount(), v->swapcount, 1, false, up)) ||
        (rc = xfer(s, (uint64_t *)d.ticks(), v->ticks, 1, false, up)))
        return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return APEMOST_HIP_OK;
}

// A prior box with min > max can never be hit: the reference's redraw loop (src/markov_chain.c:235-240)
// would spin on the host, the kernel's on the GPU.  Refuse it at the door.
static int check_box(apemost_hip_sampler *s, const apemost_hip_state_view *v) {
    if (!v->pmin && !v->pmax)
        return APEMOST_HIP_OK;
    const size_t count = (size_t)s->cfg.n_chains * s->cfg.n_par;
    std::vector<double> other;
    const double *lo = v->pmin, *hi = v->pmax;
    if (!lo || !hi) { // only one side comes with this view: the other one is what the device holds
        other.resize(count);
        HIP_TRY(hipMemcpyAsync(other.data(), lo ? s->d.pmax() : s->d.pmin(), count * sizeof(double),
                               hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        (lo ? hi : lo) = other.data();
    }
    for (size_t k = 0; k < count; k++)
        if (!(lo[k] <= hi[k]))
            return fail(APEMOST_HIP_ERR_INVALID, "chain %zu parameter %zu: min %g > max %g (or NaN)",
                        k / s->cfg.n_par, k % s->cfg.n_par, lo[k], hi[k]);
    return APEMOST_HIP_OK;
}

// The helper wavefront's threshold S_max = X - Y (pt_onebarrier.h, ObThreshold<PULSE>) holds both halves scaled by
// 1/beta: where that is not finite (beta = 0, or a beta below ~5.6e-309) X and Y are infinities of the same sign
// whenever prior_new and T = prob + ln U are, their difference is NaN and the step is rejected whatever it
// proposed.  The owner's form (prior_new - T) / beta - p1 gives the right infinity.  Such a ladder (BETA_0 = 0: the hottest chain at beta 0)
// is a legitimate configuration of the reference, so it is not refused: its launches take the eight-wave form.
static bool betas_allow_split(const double *beta, int n) {
    for (int i = 0; i < n; i++)
        if (!(beta[i] > 0 && std::isfinite(1.0 / beta[i])))
            return false;
    return true;
}

extern "C" int apemost_hip_set_state(apemost_hip_sampler *s, const apemost_hip_state_view *v) {
    CHECK_S(s);
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "state view is NULL");
    int rc = check_box(s, v);
    if (rc)
        return rc;
    // (a transfer that fails half way may have left the new betas on the device: only a good one clears them)
    const bool split_ok = v->beta ? betas_allow_split(v->beta, s->cfg.n_chains) : s->betas_split_ok;
    s->betas_split_ok = s->betas_split_ok && split_ok;
    if ((rc = xfer_state(s, v, true)))
        return rc;
    s->betas_split_ok = split_ok;
    return APEMOST_HIP_OK;
}
extern "C" int apemost_hip_get_state(apemost_hip_sampler *s, const apemost_hip_state_view *v) {
    int rc = xfer_state(s, v, false);
    return rc ? rc : check_handoff(s);
}

// ---- replica flow (APEMOST_HIP_FLAG_TRACK_REPLICAS) ----
static int flow_check(apemost_hip_sampler *s, const char *what) {
    CHECK_S(s);
    if (!s->track)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "%s: the sampler was created without APEMOST_HIP_FLAG_TRACK_REPLICAS", what);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_replica_flow_get(apemost_hip_sampler *s, const apemost_hip_replica_flow_view *v) {
    int rc = flow_check(s, "replica_flow_get");
    if (rc)
        return rc;
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "replica_flow_get: the view is NULL");
    const size_t n = s->cfg.n_chains;
    std::vector<u64> w(n);
    HIP_TRY(hipMemcpyAsync(w.data(), s->d.flow_word(), n * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    uint64_t *const host[4] = {v->n_up, v->n_down, v->attempts, v->round_trips};
    for (int k = 0; k < 4; k++)
        if (host[k])
            HIP_TRY(hipMemcpyAsync(host[k], s->d.flow_up() + k * n, n * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    for (size_t c = 0; c < n; c++) {
        if (v->replica)
            v->replica[c] = (uint32_t)(w[c] >> 2);
        if (v->heading)
            v->heading[c] = (uint32_t)(w[c] & 3);
    }
    return check_handoff(s); // the flow of a void launch is void like its state
}

extern "C" int apemost_hip_replica_flow_set(apemost_hip_sampler *s, const apemost_hip_replica_flow_view *v) {
    int rc = flow_check(s, "replica_flow_set");
    if (rc)
        return rc;
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "replica_flow_set: the view is NULL");
    const size_t n = s->cfg.n_chains, per = s->per_ladder;
    if (v->replica) {
        std::vector<char> seen(n, 0);
        for (size_t c = 0; c < n; c++) {
            const size_t base = c - c % per;
            if (v->replica[c] >= per || seen[base + v->replica[c]]++)
                return fail(APEMOST_HIP_ERR_INVALID, "replica_flow_set: the labels of ladder %zu are not a permutation of 0 .. %zu",
                            c / per, per - 1);
        }
    }
    for (size_t c = 0; v->heading && c < n; c++)
        if (v->heading[c] > 2)
            return fail(APEMOST_HIP_ERR_INVALID, "replica_flow_set: heading %u of chain %zu is not 0, 1 or 2", v->heading[c], c);
    HIP_TRY(hipStreamSynchronize(s->stream));
    std::vector<uint32_t> replica(n), heading(n);
    if (!v->replica || !v->heading) { // the half of the word that does not come with this view stays
        std::vector<u64> w(n);
        HIP_TRY(hipMemcpy(w.data(), s->d.flow_word(), n * sizeof(u64), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < n; c++) {
            replica[c] = (uint32_t)(w[c] >> 2);
            heading[c] = (uint32_t)(w[c] & 3);
        }
    }
    if (v->replica)
        replica.assign(v->replica, v->replica + n);
    if (v->heading)
        heading.assign(v->heading, v->heading + n);
    if ((rc = flow_upload(s, replica.data(), heading.data(), false)))
        return rc;
    const uint64_t *const host[4] = {v->n_up, v->n_down, v->attempts, v->round_trips};
    for (int k = 0; k < 4; k++)
        if (host[k])
            HIP_TRY(hipMemcpyAsync(s->d.flow_up() + k * n, host[k], n * sizeof(u64), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_replica_flow_reset(apemost_hip_sampler *s) {
    int rc = flow_check(s, "replica_flow_reset");
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    return flow_upload(s, nullptr, nullptr, true);
}

extern "C" int apemost_hip_set_round(apemost_hip_sampler *s, uint64_t round, int swap_pending) {
    CHECK_S(s);
    s->round = round;
    s->swap_pending = swap_pending ? 1 : 0;
    // hand-off words count swap indices upwards; a rewound swap stream restarts them
    HIP_TRY(hipMemsetAsync(s->d.published(), 0, (2 * (size_t)s->cfg.n_chains + 2) * sizeof(u64), s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return APEMOST_HIP_OK;
}
extern "C" int apemost_hip_get_round(apemost_hip_sampler *s, uint64_t *round, int *swap_pending) {
    CHECK_S(s);
    if (round)
        *round = s->round;
    if (swap_pending)
        *swap_pending = s->swap_pending;
    return APEMOST_HIP_OK;
}

// The one-barrier step with a helper wavefront (pt_onebarrier.h, HELPER): the models with a prior, where every
// workgroup of the launch has a CU to itself -- nine (thirteen) wavefronts; two such workgroups on a CU were not
// measured to gain (ladders of 257-512 chains keep the eight-wave form and its two workgroups per CU).
// APEMOST_OB_HELPER=0 switches it off (A/B runs, tests); it never runs on ladders of more than one chain per CU,
// whose nine-wave grids would not be resident.
static bool ob_wants_helper(const apemost_hip_sampler *s, int n_chains) {
    if (!ob_can_help(s->kmodel))
        return false;
    if (const char *env = getenv("APEMOST_OB_HELPER")) // (0 switches it off; 1 is the default where it may run at all)
        return atoi(env) != 0 && n_chains <= s->cus;
    return n_chains <= s->cus;
}

// the one-barrier kernels are for the built-in models, and for a user-supplied one that opts in
// (APEMOST_HIP_FLAG_USER_ONE_BARRIER: user_model_build compiled them)
static bool user_may_ob(const apemost_hip_sampler *s) {
    return !s->user.module || (s->cfg.flags & APEMOST_HIP_FLAG_USER_ONE_BARRIER);
}

static size_t ob_lds_bytes(const apemost_hip_sampler *s, bool lds_data) {
    if (s->cfg.model == APEMOST_MODEL_USER) // (no data staged: the user rows' copies where the built-in models put their data)
        return (size_t)(kObFixedDoubles + kObUserDoubles) * sizeof(double);
    return (size_t)kObFixedDoubles * sizeof(double) + (lds_data ? (size_t)2 * s->cfg.n_data * sizeof(double) : 0);
}
// dynamic LDS of the two-phase kernels for workgroups of `waves` likelihood wavefronts
static size_t classic_lds_bytes(const apemost_hip_sampler *s, int waves, bool lds_data) {
    return (kFixedLdsDoubles + (size_t)cand_slots(waves) * 2 * kWave) * sizeof(double) +
           (lds_data ? (size_t)2 * s->cfg.n_data * sizeof(double) : 0);
}

// one launch with an explicit workgroup shape (the stepping launches use the sampler's own; the
// calibration picks one per segment, by the number of chains that are still calibrating)
static int launch_shape(apemost_hip_sampler *s, KernelKind kind, int grid, const void *args, int waves, bool lds_data,
                        bool coop, bool helper = false) {
    LaunchOp op;
    op.kind = kind;
    op.lds_data = lds_data;
    op.producers = has_producer(waves);
    op.helper = helper;
    op.coop = coop;
    op.grid = grid;
    op.lds = (kind == K_ROUND_OB || kind == K_CALIB_OB) ? ob_lds_bytes(s, lds_data) : classic_lds_bytes(s, waves, lds_data);
    op.st = s->stream;
    op.args = args;
    if (coop && (s->cfg.flags & APEMOST_HIP_FLAG_TEST_REFUSE_COOPERATIVE)) // test hook: see the header
        return fail(APEMOST_HIP_ERR_RUNTIME, "kernel launch failed: cooperative launch refused (test hook)");
    if (s->user.module) {
        // the kernels of a user-supplied model live in a run-time module: the two-phase step, data through L2
        // (APEMOST_HIP_FLAG_USER_ONE_BARRIER: the one-barrier kernels too, without a helper wavefront)
        hipFunction_t f = nullptr;
        const bool ob = kind == K_ROUND_OB || kind == K_CALIB_OB;
        if (waves >= 1 && waves <= 8)
            f = kind == K_ROUND ? s->user.round[waves] : kind == K_CALIB ? s->user.calibrate[waves]
                : kind == K_CALC ? s->user.calc_model[waves] : kind == K_EVAL ? s->user.loglike[waves]
                : kind == K_ROUND_OB ? s->user.round_ob[waves] : s->user.calibrate_ob[waves];
        if (!f || lds_data || coop || helper)
            return fail(APEMOST_HIP_ERR_RUNTIME, "kernel launch failed: no such kernel for a user-supplied model");
        const unsigned block = ob ? (unsigned)ob_block(waves, false) : (unsigned)(waves * kWave);
        void *params[] = {const_cast<void *>(args)};
        const hipError_t e = hipModuleLaunchKernel(f, (unsigned)grid, 1, 1, block, 1, 1, (unsigned)op.lds, s->stream, params, nullptr);
        if (e != hipSuccess)
            return fail(APEMOST_HIP_ERR_RUNTIME, "kernel launch failed: %s", hipGetErrorString(e));
        return APEMOST_HIP_OK;
    }
    const hipError_t err = dispatch(s->kmodel, waves, op);
    if (err != hipSuccess)
        return fail(APEMOST_HIP_ERR_RUNTIME, "kernel launch failed: %s", hipGetErrorString(err));
    return APEMOST_HIP_OK;
}

// stage_data: a launch that walks the data vector only a few times (n_swap < 4, single
// likelihood evaluations) reads it through L2 instead of copying it into LDS first
static int launch(apemost_hip_sampler *s, KernelKind kind, int grid, const void *args, bool stage_data = true,
                  bool coop = false) {
    return launch_shape(s, kind, grid, args, s->waves, s->lds_data && stage_data, coop,
                        kind == K_ROUND_OB && s->ob_helper && s->betas_split_ok);
}

extern "C" int apemost_hip_calc_model(apemost_hip_sampler *s, int32_t first, int32_t count) {
    CHECK_S(s);
    if (count < 0)
        count = s->cfg.n_chains - first;
    if (first < 0 || count < 1 || first + count > s->cfg.n_chains)
        return fail(APEMOST_HIP_ERR_INVALID, "calc_model: chains [%d,%d) outside [0,%d)", first,
                    first + count, s->cfg.n_chains);
    RoundArgs a;
    a.d = s->d;
    a.sh = s->sh;
    a.cur = s->cur;
    a.first = first;
    a.which = -1;
    a.apply_swap = 0;
    a.n_steps = 0;
    a.n_rounds = 0;
    a.round = 0;
    a.samples = nullptr;
    if (!s->batch)
        return launch(s, K_CALC, count, &a, false);
    // a batch: the model-only kernel knows nothing of ladders (it uses no seed), so each ladder the range
    // touches gets a launch of its own with that ladder's data
    for (int b = first / s->per_ladder; b * s->per_ladder < first + count; b++) {
        const int lo = b * s->per_ladder > first ? b * s->per_ladder : first;
        const int hi = (b + 1) * s->per_ladder < first + count ? (b + 1) * s->per_ladder : first + count;
        a.d.data = s->d.data + (size_t)b * s->cfg.n_cols * s->cfg.n_data;
        a.sh.x_abs_max = s->x_abs_max[b];
        a.first = lo;
        const int rc = launch(s, K_CALC, hi - lo, &a, false);
        if (rc)
            return rc;
    }
    return APEMOST_HIP_OK;
}

static int loglike_on_device(apemost_hip_sampler *s, int32_t n, const double *params, const double *beta,
                             double *prob, double *prior, double *d_params, double *d_beta, double *d_prob,
                             double *d_prior) {
    const size_t np = s->cfg.n_par;
    HIP_TRY(hipMemcpyAsync(d_params, params, n * np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(d_beta, beta, n * sizeof(double), hipMemcpyHostToDevice, s->stream));
    EvalArgs a;
    a.sh = s->sh;
    a.data = s->d.data;
    a.params = d_params;
    a.beta = d_beta;
    a.prob = d_prob;
    a.prior = d_prior;
    const int rc = launch(s, K_EVAL, n, &a, false);
    if (rc) {
        hipStreamSynchronize(s->stream);
        return rc;
    }
    HIP_TRY(hipMemcpyAsync(prob, d_prob, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    if (prior)
        HIP_TRY(hipMemcpyAsync(prior, d_prior, n * sizeof(double), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_loglike(apemost_hip_sampler *s, int32_t n, const double *params,
                                   const double *beta, double *prob, double *prior) {
    CHECK_S(s);
    if (n < 1 || !params || !beta || !prob)
        return fail(APEMOST_HIP_ERR_INVALID, "loglike: bad arguments");
    if (s->batch && s->n_ladders > 1)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "loglike: a batch of %d ladders has no single data matrix", s->n_ladders);
    const size_t np = s->cfg.n_par;
    // one scratch block: params [n][np], beta [n], prob [n], prior [n]
    double *scratch = nullptr;
    HIP_TRY(hipMalloc((void **)&scratch, (size_t)n * (np + 3) * sizeof(double)));
    double *d_params = scratch, *d_beta = scratch + (size_t)n * np, *d_prob = d_beta + n, *d_prior = d_prob + n;
    const int rc = loglike_on_device(s, n, params, beta, prob, prior, d_params, d_beta, d_prob, d_prior);
    hipFree(scratch);
    return rc;
}

template <bool LDS>
static hipError_t round_occupancy(int model, int waves, bool producers, bool one_barrier, bool helper, size_t lds_bytes, int *blocks) {
    OccupancyOp<LDS> op;
    op.producers = producers;
    op.one_barrier = one_barrier;
    op.helper = helper;
    op.lds_bytes = lds_bytes;
    op.blocks = blocks;
    return dispatch(model, waves, op);
}

// Kernels that stage more than 64 KiB must opt in once per function: every kernel of the `waves`-wave
// shape that may stage the data vector, each with its own footprint (the one-barrier kernels carve
// 1 KiB more than the two-phase ones).  Made once per shape, before its first launch.
static int enable_big_lds(apemost_hip_sampler *s, int waves) {
    if (((s->big_lds_set >> waves) & 1) || s->user.module)
        return APEMOST_HIP_OK;
    LdsAttrOp op;
    op.bytes = classic_lds_bytes(s, waves, true);
    op.ob_bytes = ob_lds_bytes(s, true);
    const size_t most = has_one_barrier(waves) && op.ob_bytes > op.bytes ? op.ob_bytes : op.bytes;
    if (s->cfg.lds_policy != 2 && most > 64 * 1024 && most <= 160 * 1024 - 1024) {
        const hipError_t e = dispatch(s->kmodel, waves, op);
        if (e != hipSuccess)
            return fail(APEMOST_HIP_ERR_RUNTIME, "hipFuncSetAttribute(LDS %zu B): %s", most, hipGetErrorString(e));
    }
    s->big_lds_set |= 1u << waves;
    return APEMOST_HIP_OK;
}

static int launch_round_impl(apemost_hip_sampler *s, uint32_t n_rounds, uint32_t n_steps, int apply_swap, int which,
                             double *d_samples);

extern "C" int apemost_hip_launch_round(apemost_hip_sampler *s, uint32_t n_steps, int apply_swap,
                                        double *d_samples) {
    return launch_round_impl(s, 1, n_steps, apply_swap, -1, d_samples);
}

extern "C" int apemost_hip_launch_rounds(apemost_hip_sampler *s, uint32_t n_rounds, uint32_t n_steps,
                                         int apply_swap, double *d_samples) {
    if (n_rounds < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "launch_rounds: n_rounds must be >= 1");
    return launch_round_impl(s, n_rounds, n_steps, apply_swap, -1, d_samples);
}

extern "C" int apemost_hip_launch_round_for(apemost_hip_sampler *s, uint32_t n_steps, int32_t param,
                                            double *d_samples) {
    if (s && (param < 0 || param >= s->cfg.n_par))
        return fail(APEMOST_HIP_ERR_INVALID, "launch_round_for: parameter %d outside [0,%d)", param, s->cfg.n_par);
    return launch_round_impl(s, 1, n_steps, 0, param, d_samples);
}

// Multi-round launches hand swap records from workgroup to workgroup inside the launch, which
// is only safe when every workgroup of the grid is resident at once.
static int max_rounds_per_launch(apemost_hip_sampler *s) {
    return (s->resident_ok && !s->handoff_failed) ? 1024 : 1;
}

extern "C" int apemost_hip_max_rounds_per_launch(apemost_hip_sampler *s, int32_t *max_rounds) {
    CHECK_S(s);
    if (!max_rounds)
        return fail(APEMOST_HIP_ERR_INVALID, "max_rounds is NULL");
    *max_rounds = max_rounds_per_launch(s);
    return APEMOST_HIP_OK;
}

static int launch_round_impl(apemost_hip_sampler *s, uint32_t n_rounds, uint32_t n_steps, int apply_swap, int which,
                             double *d_samples) {
    CHECK_S(s);
    int rc;
    if ((int)n_rounds > max_rounds_per_launch(s))
        return fail(APEMOST_HIP_ERR_INVALID, "%u rounds in one launch, this sampler allows %d (grid residency)",
                    n_rounds, max_rounds_per_launch(s));
    if (n_rounds > 1 && n_steps == 0)
        return fail(APEMOST_HIP_ERR_INVALID, "multi-round launches need n_steps > 0");
    RoundArgs a;
    a.d = s->d;
    a.sh = s->sh;
    a.cur = s->cur;
    a.first = 0;
    a.which = which;
    a.apply_swap = apply_swap ? 1 : 0;
    a.n_steps = n_steps;
    a.n_rounds = n_rounds;
    a.round = s->round;
    a.samples = d_samples;
    bool stage = (u64)n_steps * n_rounds >= 4 || s->cfg.lds_policy == 1;
    if (n_rounds > 1) // residency decides when workgroups wait for each other
        stage = s->resident_lds ? stage || !s->resident_plain : false;
    const bool one_barrier = s->one_barrier && which < 0 && n_steps > 0;
    rc = launch(s, one_barrier ? K_ROUND_OB : K_ROUND, s->cfg.n_chains, &a, stage, s->cooperative && n_rounds > 1);
    if (rc && s->cooperative && n_rounds > 1) {
        // The runtime cannot place the grid at once (nothing has run): this sampler issues one
        // round per launch from now on, beginning with the rounds asked for here -- the swap
        // attempt between two of them is then the fused swap-in at the second one's start.
        s->resident_ok = false;
        const size_t row = (size_t)s->cfg.n_chains * (s->cfg.n_par + 2);
        for (uint32_t i = 0; i < n_rounds; i++) {
            rc = launch_round_impl(s, 1, n_steps, i == 0 ? apply_swap : 1, which,
                                   d_samples ? d_samples + (size_t)i * n_steps * row : nullptr);
            if (rc)
                return rc;
        }
        return APEMOST_HIP_OK;
    }
    if (rc)
        return rc;
    if ((s->cfg.flags & APEMOST_HIP_FLAG_RWM) && n_steps > 0 && which < 0 && !s->in_rwm) {
        // a round of run_sampler has stepped (n_rounds is 1 here): adapt()'s RWM block before its ADAPT block
        // and before the swap attempt.  The chain now lives in the other half of the state; the extra step is
        // an ordinary launch of one step (no rows, the pending swap attempt left pending).
        if (!s->rwm_keep && (rc = dev_alloc(s, &s->rwm_keep, (size_t)s->cfg.n_chains * (2 + s->cfg.n_par))))
            return rc;
        const dim3 grid((s->cfg.n_chains + 255) / 256), block(256);
        const double target = s->cfg.adapt_target != 0 ? s->cfg.adapt_target : 0.5;
        const u64 round_before = s->round;
        s->cur ^= 1;
        s->launches++;
        hipLaunchKernelGGL(pt_rwm_pre_kernel, grid, block, 0, s->stream, s->d, s->cur, s->rwm_keep);
        HIP_TRY(hipGetLastError());
        s->in_rwm = true;
        rc = launch_round_impl(s, 1, 1, 0, -1, nullptr);
        s->in_rwm = false;
        if (rc)
            return rc;
        hipLaunchKernelGGL(pt_rwm_post_kernel, grid, block, 0, s->stream, s->d, s->sh, s->cur, (const double *)s->rwm_keep, target);
        HIP_TRY(hipGetLastError());
        s->cur ^= 1; // (the bookkeeping below flips it back: the state is where the extra step left it)
        s->launches--;
        s->round = round_before;
    }
    if ((s->cfg.flags & APEMOST_HIP_FLAG_ADAPT) && n_steps > 0 && which < 0 && !s->in_rwm) {
        // a round of run_sampler has stepped: adapt() before its swap attempt (n_rounds is 1 here)
        const double target = s->cfg.adapt_target != 0 ? s->cfg.adapt_target : 0.5;
        hipLaunchKernelGGL(pt_adapt_kernel, dim3((s->cfg.n_chains + 255) / 256), dim3(256), 0, s->stream, s->d, target);
        HIP_TRY(hipGetLastError());
    }
    s->cur ^= 1;
    s->launches++;
    s->round += (apply_swap ? 1 : 0) + (n_rounds - 1); // swap attempts consumed by this launch
    if (apply_swap)
        s->swap_pending = 0;
    if (n_steps > 0 && which < 0)
        s->swap_pending = 1;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_run(apemost_hip_sampler *s, uint64_t n_rounds, uint32_t n_swap,
                               double *d_samples) {
    CHECK_S(s);
    if (s->cfg.n_chains != s->cfg.n_chains_global)
        return fail(APEMOST_HIP_ERR_INVALID,
                    "apemost_hip_run needs the whole ladder on one device; sharded ladders drive "
                    "apemost_hip_launch_rounds + apemost_hip_edge_*");
    const size_t row = (size_t)s->cfg.n_chains * (s->cfg.n_par + 2);
    for (uint64_t r = 0; r < n_rounds;) {
        const uint64_t per_launch = n_swap > 0 ? (uint64_t)max_rounds_per_launch(s) : 1;
        const uint64_t k = n_rounds - r < per_launch ? n_rounds - r : per_launch;
        int rc = launch_round_impl(s, (uint32_t)k, n_swap, s->swap_pending, -1,
                                   d_samples ? d_samples + r * n_swap * row : nullptr);
        if (rc)
            return rc;
        r += k;
    }
    if (s->swap_pending)
        return apemost_hip_launch_round(s, 0, 1, nullptr);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_samples_alloc(apemost_hip_sampler *s, uint64_t n_steps, double **d_samples) {
    CHECK_S(s);
    if (!d_samples || n_steps == 0)
        return fail(APEMOST_HIP_ERR_INVALID, "samples_alloc: bad arguments");
    const size_t bytes = (size_t)n_steps * s->cfg.n_chains * (s->cfg.n_par + 2) * sizeof(double);
    HIP_TRY(hipMalloc((void **)d_samples, bytes));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_samples_read(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                        double *host) {
    CHECK_S(s);
    if (!d_samples || !host)
        return fail(APEMOST_HIP_ERR_INVALID, "samples_read: bad arguments");
    const size_t bytes = (size_t)n_steps * s->cfg.n_chains * (s->cfg.n_par + 2) * sizeof(double);
    HIP_TRY(hipMemcpyAsync(host, d_samples, bytes, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return check_handoff(s); // rows of a void launch are not handed to the caller as samples
}

extern "C" int apemost_hip_samples_read_async(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                              double *host_samples, uint64_t *counters) {
    CHECK_S(s);
    if (!d_samples || !host_samples)
        return fail(APEMOST_HIP_ERR_INVALID, "samples_read_async: bad arguments");
    if (!s->copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s->ev_copy, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc((void **)&s->h_word, sizeof(u64), hipHostMallocDefault));
        *s->h_word = 0;
    }
    const size_t n = s->cfg.n_chains;
    // small things ride on the sampler's own stream, in launch order: the counters as they stand now
    // and the error word of the launches so far
    if (counters)
        HIP_TRY(hipMemcpyAsync(counters, s->d.accept(), 2 * n * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipMemcpyAsync(s->h_word, s->d.timeout_word(), sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const size_t bytes = (size_t)n_steps * n * (s->cfg.n_par + 2) * sizeof(double);
    HIP_TRY(hipMemcpyAsync(host_samples, d_samples, bytes, hipMemcpyDeviceToHost, s->copy_stream));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_samples_pack_read_async(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                                   uint64_t skip, uint64_t thin, int32_t n_param_chains, int32_t layout,
                                                   double *d_packed, double *host_packed, uint64_t *counters,
                                                   uint64_t *n_kept) {
    CHECK_S(s);
    if (!d_samples || !d_packed || !host_packed || thin < 1 || (layout != 0 && layout != 1) || n_param_chains < 0 ||
        n_param_chains > s->cfg.n_chains)
        return fail(APEMOST_HIP_ERR_INVALID, "samples_pack_read_async: bad arguments");
    if (!s->copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s->ev_copy, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc((void **)&s->h_word, sizeof(u64), hipHostMallocDefault));
        *s->h_word = 0;
    }
    const size_t n = s->cfg.n_chains, np = s->cfg.n_par;
    const uint64_t kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    const size_t record = layout == 0 ? (size_t)n_param_chains * np + 2 * n : n * (np + 2);
    if (n_kept)
        *n_kept = kept;
    if (kept > 0) {
        const size_t total = (size_t)kept * record;
        size_t blocks = (total + 255) / 256;
        if (blocks > 65535)
            blocks = 65535;
        hipLaunchKernelGGL(samples_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s->stream, d_samples, (int)n, (int)np,
                           (unsigned long long)kept, (unsigned long long)skip, (unsigned long long)thin, (int)n_param_chains,
                           (int)layout, d_packed);
        HIP_TRY(hipGetLastError());
    }
    if (counters) {
        HIP_TRY(hipMemcpyAsync(counters, s->d.accept(), 2 * n * sizeof(u64), hipMemcpyDeviceToHost, s->stream));
        // ... and, behind them, chain 0's parameter vector of the batch's LAST step (n_par doubles): what a
        // progress line prints, whatever the packing kept
        if (n_steps > 0)
            HIP_TRY(hipMemcpyAsync(counters + 2 * n, d_samples + (size_t)(n_steps - 1) * n * (np + 2), np * sizeof(double),
                                   hipMemcpyDeviceToHost, s->stream));
    }
    HIP_TRY(hipMemcpyAsync(s->h_word, s->d.timeout_word(), sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    if (kept > 0)
        HIP_TRY(hipMemcpyAsync(host_packed, d_packed, (size_t)kept * record * sizeof(double), hipMemcpyDeviceToHost,
                               s->copy_stream));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_samples_wait(apemost_hip_sampler *s) {
    CHECK_S(s);
    if (!s->copy_stream)
        return APEMOST_HIP_OK;
    HIP_TRY(hipStreamSynchronize(s->copy_stream));
    if (*s->h_word != 0)
        return apemost_hip_synchronize(s); // reports, clears and falls back (check_handoff)
    return APEMOST_HIP_OK;
}

// ---- run summary (pt_summary.h) ----
// batches of batch_means_error() closed after n samples: sample n (counted from 1) closes one when
// n % bs == bs - 1 -- for bs >= 2 the first batch holds bs - 1 samples, every later one bs
static u64 summary_closed(u64 n, u64 bs) { return bs == 1 ? n : (n + 1) / bs; }
// samples still to come before the batch that is open after n samples closes (1 .. bs)
static u64 summary_left(u64 n, u64 bs) {
    const u64 m = (bs - (n + 1) % bs) % bs;
    return m == 0 ? bs : m;
}

static int ensure_copy_stream(apemost_hip_sampler *s) {
    if (!s->copy_stream) {
        HIP_TRY(hipStreamCreateWithFlags(&s->copy_stream, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&s->ev_copy, hipEventDisableTiming));
        HIP_TRY(hipHostMalloc((void **)&s->h_word, sizeof(u64), hipHostMallocDefault));
        *s->h_word = 0;
    }
    return APEMOST_HIP_OK;
}

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
    for (int p = 0; p < np && cfg->lo && cfg->hi; p++)
        if (!std::isfinite(cfg->lo[p]) || !std::isfinite(cfg->hi[p]) || !(cfg->lo[p] < cfg->hi[p]) ||
            !std::isfinite(cfg->hi[p] - cfg->lo[p])) // (a width that overflows: the bin guess divides by it)
            return fail(APEMOST_HIP_ERR_INVALID, "summary_begin: parameter %d: range [%g, %g] invalid", p, cfg->lo[p],
                        cfg->hi[p]);
    const size_t n_hp = (size_t)cfg->n_hist_chains * np;
    if (cfg->max_batches > ((size_t)1 << 40) || (n_hp > 0 && cfg->max_batches + 1 > ((size_t)1 << 40) / n_hp))
        return fail(APEMOST_HIP_ERR_INVALID, "summary_begin: max_batches %llu too large",
                    (unsigned long long)cfg->max_batches);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream)); // a summary before this one may still be accumulating
    summary_free(s);
    s->sum.n_hist = cfg->n_hist_chains;
    s->sum.nbins = cfg->nbins;
    s->sum.bs = cfg->batch_size;
    s->sum.max_batches = cfg->max_batches;
    s->sum.n = 0;
    const size_t nb = n_hp * (cfg->max_batches + 1), nh = n_hp * cfg->nbins;
    HIP_TRY(hipMalloc((void **)&s->sum.d_prob_sum, s->cfg.n_chains * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->sum.d_lo, np * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->sum.d_hi, np * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->sum.d_batch, (nb > 0 ? nb : 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->sum.d_hist, (nh > 0 ? nh : 1) * sizeof(u64)));
    HIP_TRY(hipMemsetAsync(s->sum.d_prob_sum, 0, s->cfg.n_chains * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->sum.d_batch, 0, (nb > 0 ? nb : 1) * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->sum.d_hist, 0, (nh > 0 ? nh : 1) * sizeof(u64), s->stream));
    HIP_TRY(hipMemsetAsync(s->sum.d_lo, 0, np * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->sum.d_hi, 0, np * sizeof(double), s->stream));
    if (cfg->lo && cfg->hi) {
        HIP_TRY(hipMemcpyAsync(s->sum.d_lo, cfg->lo, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
        HIP_TRY(hipMemcpyAsync(s->sum.d_hi, cfg->hi, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->sum.open = true;
    return APEMOST_HIP_OK;
}

// Queued on copy_stream behind everything launched so far on the sampler's stream, like
// apemost_hip_samples_read_async: launches issued after this call overlap with it, and
// apemost_hip_samples_wait / apemost_hip_summary_get wait for it -- the caller does one of them before
// d_samples is written again.
extern "C" int apemost_hip_summary_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                              uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    if (!s->sum.open)
        return fail(APEMOST_HIP_ERR_INVALID, "summary_accumulate: no summary_begin");
    if (thin < 1 || (!d_samples && n_steps > 0))
        return fail(APEMOST_HIP_ERR_INVALID, "summary_accumulate: bad arguments");
    const u64 kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    if (summary_closed(s->sum.n + kept, s->sum.bs) > s->sum.max_batches)
        return fail(APEMOST_HIP_ERR_INVALID,
                    "summary_accumulate: %llu samples would close batch %llu, beyond max_batches = %llu",
                    (unsigned long long)(s->sum.n + kept), (unsigned long long)summary_closed(s->sum.n + kept, s->sum.bs),
                    (unsigned long long)s->sum.max_batches);
    if (kept == 0)
        return APEMOST_HIP_OK;
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const int n_hp = s->sum.n_hist * s->cfg.n_par;
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
        a.n_hist = s->sum.n_hist;
        a.nbins = s->sum.nbins;
        a.lo = s->sum.d_lo;
        a.hi = s->sum.d_hi;
        a.bs = s->sum.bs;
        a.left = summary_left(s->sum.n, s->sum.bs);
        a.n_closed = summary_closed(s->sum.n, s->sum.bs);
        a.prob_sum = s->sum.d_prob_sum;
        a.hist = s->sum.d_hist;
        a.batch = s->sum.d_batch;
        a.batch_stride = s->sum.max_batches + 1;
        hipLaunchKernelGGL(summary_kernel, dim3(grid), dim3(kSummaryThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        s->sum.n += a.n_kept;
    }
    return APEMOST_HIP_OK;
}

static int summary_xfer(apemost_hip_sampler *s, const apemost_hip_summary_view *v, bool up) {
    if (!s->sum.open)
        return fail(APEMOST_HIP_ERR_INVALID, "summary_%s: no summary_begin", up ? "set" : "get");
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "summary view is NULL");
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    const size_t n_hp = (size_t)s->sum.n_hist * s->cfg.n_par;
    const size_t nb = n_hp * (s->sum.max_batches + 1), nh = n_hp * s->sum.nbins;
    if (up && v->n) {
        if (summary_closed(*v->n, s->sum.bs) > s->sum.max_batches)
            return fail(APEMOST_HIP_ERR_INVALID, "summary_set: %llu samples close more than max_batches batches",
                        (unsigned long long)*v->n);
        if (v->n_batches && *v->n_batches != summary_closed(*v->n, s->sum.bs))
            return fail(APEMOST_HIP_ERR_INVALID, "summary_set: n_batches %llu does not follow from n = %llu",
                        (unsigned long long)*v->n_batches, (unsigned long long)*v->n);
    }
    // stream order: behind every accumulate queued so far, on the stream they run on
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
#define SUMMARY_COPY(dev, host, bytes)                                                                          \
    do {                                                                                                       \
        if ((host) && (bytes) > 0)                                                                             \
            HIP_TRY(up ? hipMemcpyAsync((void *)(dev), (const void *)(host), (bytes), kind, s->copy_stream)    \
                       : hipMemcpyAsync((void *)(host), (const void *)(dev), (bytes), kind, s->copy_stream));  \
    } while (0)
    SUMMARY_COPY(s->sum.d_prob_sum, v->prob_sum, s->cfg.n_chains * sizeof(double));
    SUMMARY_COPY(s->sum.d_hist, v->hist, nh * sizeof(u64));
    SUMMARY_COPY(s->sum.d_batch, v->batch_sums, nb * sizeof(double));
#undef SUMMARY_COPY
    HIP_TRY(hipStreamSynchronize(s->copy_stream));
    if (up) {
        if (v->n)
            s->sum.n = *v->n;
    } else {
        if (v->n)
            *v->n = s->sum.n;
        if (v->n_batches)
            *v->n_batches = summary_closed(s->sum.n, s->sum.bs);
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_summary_get(apemost_hip_sampler *s, const apemost_hip_summary_view *v) {
    CHECK_S(s);
    return summary_xfer(s, v, false);
}

extern "C" int apemost_hip_summary_set(apemost_hip_sampler *s, const apemost_hip_summary_view *v) {
    CHECK_S(s);
    return summary_xfer(s, v, true);
}

extern "C" int apemost_hip_summary_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    summary_free(s);
    return APEMOST_HIP_OK;
}

// ---- on-device peaks (pt_peaks.h) ----
extern "C" int apemost_hip_peaks_begin(apemost_hip_sampler *s, const apemost_hip_peaks_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: config is NULL");
    const int np = s->cfg.n_par;
    if (cfg->n_keep < 1 || cfg->n_keep > s->cfg.n_chains || !cfg->chains)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: n_keep %d outside [1,%d], or no chains", cfg->n_keep,
                    s->cfg.n_chains);
    if ((long long)cfg->n_keep * np > 65535)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: %d chains of %d parameters are more than 65535 columns",
                    cfg->n_keep, np);
    for (int k = 0; k < cfg->n_keep; k++)
        if (cfg->chains[k] < 0 || cfg->chains[k] >= s->cfg.n_chains || (k > 0 && cfg->chains[k] <= cfg->chains[k - 1]))
            return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: chains[%d] = %d: local chain indices in [0,%d), strictly increasing",
                        k, cfg->chains[k], s->cfg.n_chains);
    if (cfg->capacity < 1 || cfg->capacity > ((u64)1 << 30))
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: capacity %llu outside [1, 2^30]",
                    (unsigned long long)cfg->capacity);
    if (!cfg->lo || !cfg->hi)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: lo and hi are needed");
    for (int p = 0; p < np; p++)
        if (!std::isfinite(cfg->lo[p]) || !std::isfinite(cfg->hi[p]) || !(cfg->lo[p] < cfg->hi[p]) ||
            !std::isfinite(cfg->hi[p] - cfg->lo[p]))
            return fail(APEMOST_HIP_ERR_INVALID, "peaks_begin: parameter %d: range [%g, %g] invalid", p, cfg->lo[p],
                        cfg->hi[p]);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream)); // columns begun before may still be filling
    peaks_free(s);
    s->pk.n_keep = cfg->n_keep;
    s->pk.capacity = cfg->capacity;
    s->pk.n = 0;
    HIP_TRY(hipMalloc((void **)&s->pk.d_chains, cfg->n_keep * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&s->pk.d_lo, np * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pk.d_hi, np * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pk.d_cols, (size_t)cfg->n_keep * np * cfg->capacity * sizeof(double)));
    HIP_TRY(hipMemcpyAsync(s->pk.d_chains, cfg->chains, cfg->n_keep * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->pk.d_lo, cfg->lo, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->pk.d_hi, cfg->hi, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    s->pk.open = true;
    return APEMOST_HIP_OK;
}

// Queued on copy_stream behind everything launched so far on the sampler's stream, like
// apemost_hip_summary_accumulate; apemost_hip_samples_wait covers it.
extern "C" int apemost_hip_peaks_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                            uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    if (!s->pk.open)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_accumulate: no peaks_begin");
    if (thin < 1 || (!d_samples && n_steps > 0))
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_accumulate: bad arguments");
    const u64 kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    if (kept > s->pk.capacity - s->pk.n)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_accumulate: %llu samples stored, %llu more are beyond capacity = %llu",
                    (unsigned long long)s->pk.n, (unsigned long long)kept, (unsigned long long)s->pk.capacity);
    if (kept == 0)
        return APEMOST_HIP_OK;
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    PeaksAppendArgs a;
    a.rows = d_samples;
    a.n_chains = s->cfg.n_chains;
    a.n_par = s->cfg.n_par;
    a.n_keep = s->pk.n_keep;
    a.chains = s->pk.d_chains;
    a.skip = skip;
    a.thin = thin;
    a.n_kept = kept;
    a.cols = s->pk.d_cols;
    a.capacity = s->pk.capacity;
    a.n = s->pk.n;
    const dim3 grid((unsigned)((kept + kPeaksThreads - 1) / kPeaksThreads), (unsigned)(s->pk.n_keep * s->cfg.n_par));
    hipLaunchKernelGGL(peaks_append_kernel, grid, dim3(kPeaksThreads), 0, s->copy_stream, a);
    HIP_TRY(hipGetLastError());
    s->pk.n += kept;
    return APEMOST_HIP_OK;
}

namespace {
struct PeaksScratch { // freed on every way out of peaks_get (hipFree waits for the kernels that use it)
    void *p = nullptr;
    ~PeaksScratch() {
        if (p)
            hipFree(p);
    }
};
} // namespace

extern "C" int apemost_hip_peaks_get(apemost_hip_sampler *s, const apemost_hip_peaks_view *v) {
    CHECK_S(s);
    if (!s->pk.open)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_get: no peaks_begin");
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks view is NULL");
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
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
    PeaksScratch scratch;
    HIP_TRY(hipMalloc(&scratch.p, at));
    char *base = (char *)scratch.p;
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
    // stream order: behind every accumulate queued so far, on the stream they run on
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
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
    HIP_TRY(hipStreamSynchronize(st));
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
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    peaks_free(s);
    return APEMOST_HIP_OK;
}

// ---- on-device joint marginals (pt_joint.h) ----
extern "C" int apemost_hip_joint_begin(apemost_hip_sampler *s, const apemost_hip_joint_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: config is NULL");
    const int np = s->cfg.n_par;
    if (cfg->n_keep < 1 || cfg->n_keep > s->cfg.n_chains || !cfg->chains)
        return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: n_keep %d outside [1,%d], or no chains", cfg->n_keep,
                    s->cfg.n_chains);
    if ((long long)cfg->n_keep * np > 65535)
        return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: %d chains of %d parameters are more than 65535 columns",
                    cfg->n_keep, np);
    for (int k = 0; k < cfg->n_keep; k++)
        if (cfg->chains[k] < 0 || cfg->chains[k] >= s->cfg.n_chains || (k > 0 && cfg->chains[k] <= cfg->chains[k - 1]))
            return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: chains[%d] = %d: local chain indices in [0,%d), strictly increasing",
                        k, cfg->chains[k], s->cfg.n_chains);
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
    for (int p = 0; p < np; p++)
        if (!std::isfinite(cfg->lo[p]) || !std::isfinite(cfg->hi[p]) || !(cfg->lo[p] < cfg->hi[p]) ||
            !std::isfinite(cfg->hi[p] - cfg->lo[p]))
            return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: parameter %d: range [%g, %g] invalid", p, cfg->lo[p],
                        cfg->hi[p]);
    const u64 n_counts = (u64)cfg->n_keep * n_pairs * cfg->nbins * cfg->nbins; // (< 2^16 2^16 2^18: no overflow)
    if (n_pairs > 65535 || n_counts * sizeof(u64) > ((u64)1 << 30))
        return fail(APEMOST_HIP_ERR_INVALID, "joint_begin: %d chains x %d pairs x %d^2 bins: counts above 2^30 bytes",
                    cfg->n_keep, n_pairs, cfg->nbins);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream)); // a joint begun before may still be accumulating
    joint_free(s);
    const size_t n_cols = (size_t)cfg->n_keep * np, tri = (size_t)np * (np + 1) / 2;
    // the staged columns: about 4 Mi values over all of them, at least 256 and at most 2^18 kept steps per launch
    // (the LDS counters are 32 bits wide)
    u64 chunk = ((u64)1 << 22) / n_cols;
    chunk = chunk < 256 ? 256 : chunk > ((u64)1 << 18) ? (u64)1 << 18 : chunk;
    s->jt.n_keep = cfg->n_keep;
    s->jt.nbins = cfg->nbins;
    s->jt.n_pairs = n_pairs;
    s->jt.chunk = chunk;
    s->jt.n = 0;
    HIP_TRY(hipMalloc((void **)&s->jt.d_chains, cfg->n_keep * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_pairs, (n_pairs > 0 ? n_pairs : 1) * 2 * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_lo, np * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_hi, np * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_vals, n_cols * chunk * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_bins, n_cols * chunk * sizeof(unsigned short)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_origin, n_cols * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_sum, n_cols * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_cross, cfg->n_keep * tri * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->jt.d_counts, (n_counts > 0 ? n_counts : 1) * sizeof(u64)));
    HIP_TRY(hipMemsetAsync(s->jt.d_origin, 0, n_cols * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->jt.d_sum, 0, n_cols * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->jt.d_cross, 0, cfg->n_keep * tri * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->jt.d_counts, 0, (n_counts > 0 ? n_counts : 1) * sizeof(u64), s->stream));
    HIP_TRY(hipMemcpyAsync(s->jt.d_chains, cfg->chains, cfg->n_keep * sizeof(int), hipMemcpyHostToDevice, s->stream));
    if (n_pairs > 0)
        HIP_TRY(hipMemcpyAsync(s->jt.d_pairs, pairs.data(), pairs.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->jt.d_lo, cfg->lo, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->jt.d_hi, cfg->hi, np * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (`pairs` and the caller's arrays are read until here)
    s->jt.open = true;
    return APEMOST_HIP_OK;
}

// Queued on copy_stream behind everything launched so far on the sampler's stream, like
// apemost_hip_summary_accumulate; apemost_hip_samples_wait covers it.
extern "C" int apemost_hip_joint_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                            uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    if (!s->jt.open)
        return fail(APEMOST_HIP_ERR_INVALID, "joint_accumulate: no joint_begin");
    if (thin < 1 || (!d_samples && n_steps > 0))
        return fail(APEMOST_HIP_ERR_INVALID, "joint_accumulate: bad arguments");
    const u64 kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    if (kept == 0)
        return APEMOST_HIP_OK;
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const int np = s->cfg.n_par, n_cols = s->jt.n_keep * np;
    const int band_rows = joint_band_rows(s->jt.nbins), n_bands = (s->jt.nbins + band_rows - 1) / band_rows;
    const int entries = s->jt.n_keep * (np + np * (np + 1) / 2);
    for (u64 k0 = 0; k0 < kept; k0 += s->jt.chunk) {
        JointArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = np;
        a.n_keep = s->jt.n_keep;
        a.chains = s->jt.d_chains;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < s->jt.chunk ? kept - k0 : s->jt.chunk);
        a.chunk = s->jt.chunk;
        a.nbins = s->jt.nbins;
        a.n_pairs = s->jt.n_pairs;
        a.pairs = s->jt.d_pairs;
        a.lo = s->jt.d_lo;
        a.hi = s->jt.d_hi;
        a.vals = s->jt.d_vals;
        a.bins = s->jt.d_bins;
        a.first = s->jt.n == 0;
        a.counts = s->jt.d_counts;
        a.origin = s->jt.d_origin;
        a.sum = s->jt.d_sum;
        a.cross = s->jt.d_cross;
        hipLaunchKernelGGL(joint_gather_kernel, dim3((a.n + kJointGatherPer - 1) / kJointGatherPer, (unsigned)n_cols),
                           dim3(kJointThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        if (s->jt.n_pairs > 0) {
            hipLaunchKernelGGL(joint_pair_kernel, dim3((unsigned)n_bands, (unsigned)s->jt.n_pairs, (unsigned)s->jt.n_keep),
                               dim3(kJointThreads), 0, s->copy_stream, a);
            HIP_TRY(hipGetLastError());
        }
        hipLaunchKernelGGL(joint_moments_kernel, dim3((unsigned)((entries + kJointMomentThreads - 1) / kJointMomentThreads)),
                           dim3(kJointMomentThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        s->jt.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int joint_xfer(apemost_hip_sampler *s, const apemost_hip_joint_view *v, bool up) {
    if (!s->jt.open)
        return fail(APEMOST_HIP_ERR_INVALID, "joint_%s: no joint_begin", up ? "set" : "get");
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "joint view is NULL");
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    const size_t np = s->cfg.n_par, n_cols = (size_t)s->jt.n_keep * np, tri = np * (np + 1) / 2;
    const size_t n_counts = (size_t)s->jt.n_keep * s->jt.n_pairs * s->jt.nbins * s->jt.nbins;
    // stream order: behind every accumulate queued so far, on the stream they run on
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
#define JOINT_COPY(dev, host, bytes)                                                                            \
    do {                                                                                                       \
        if ((host) && (bytes) > 0)                                                                             \
            HIP_TRY(up ? hipMemcpyAsync((void *)(dev), (const void *)(host), (bytes), kind, s->copy_stream)    \
                       : hipMemcpyAsync((void *)(host), (const void *)(dev), (bytes), kind, s->copy_stream));  \
    } while (0)
    JOINT_COPY(s->jt.d_counts, v->counts, n_counts * sizeof(u64));
    JOINT_COPY(s->jt.d_origin, v->origin, n_cols * sizeof(double));
    JOINT_COPY(s->jt.d_sum, v->sum, n_cols * sizeof(double));
    JOINT_COPY(s->jt.d_cross, v->cross, s->jt.n_keep * tri * sizeof(double));
#undef JOINT_COPY
    HIP_TRY(hipStreamSynchronize(s->copy_stream));
    if (v->n) {
        if (up)
            s->jt.n = *v->n;
        else
            *v->n = s->jt.n;
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_joint_get(apemost_hip_sampler *s, const apemost_hip_joint_view *v) {
    CHECK_S(s);
    return joint_xfer(s, v, false);
}

extern "C" int apemost_hip_joint_set(apemost_hip_sampler *s, const apemost_hip_joint_view *v) {
    CHECK_S(s);
    return joint_xfer(s, v, true);
}

extern "C" int apemost_hip_joint_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    joint_free(s);
    return APEMOST_HIP_OK;
}

// ---- on-device evidence fold (pt_evidence.h) ----
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
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream)); // a fold begun before may still be accumulating
    evidence_free(s);
    // the staged column: about 1 Mi values over all chains, at least 256 and at most 2^18 kept steps per launch
    u64 chunk = ((u64)1 << 20) / nc;
    chunk = chunk < 256 ? 256 : chunk > ((u64)1 << 18) ? (u64)1 << 18 : chunk;
    s->ev.bs = cfg->batch_size;
    s->ev.max_batches = cfg->max_batches;
    s->ev.chunk = chunk;
    s->ev.n = 0;
    const size_t nb = nc * (cfg->max_batches + 1);
    HIP_TRY(hipMalloc((void **)&s->ev.d_coef, 2 * nc * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ev.d_vals, nc * chunk * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ev.d_origin, nc * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ev.d_sum, nc * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ev.d_sq, nc * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ev.d_batch, nb * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ev.d_m, 2 * nc * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ev.d_S, 2 * nc * sizeof(double)));
    HIP_TRY(hipMemsetAsync(s->ev.d_origin, 0, nc * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ev.d_sum, 0, nc * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ev.d_sq, 0, nc * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ev.d_batch, 0, nb * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ev.d_m, 0, 2 * nc * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ev.d_S, 0, 2 * nc * sizeof(double), s->stream));
    HIP_TRY(hipMemcpyAsync(s->ev.d_coef, cfg->coef_up, nc * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->ev.d_coef + nc, cfg->coef_down, nc * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's arrays are read until here)
    s->ev.open = true;
    return APEMOST_HIP_OK;
}

// Queued on copy_stream behind everything launched so far on the sampler's stream, like
// apemost_hip_summary_accumulate; apemost_hip_samples_wait covers it.
extern "C" int apemost_hip_evidence_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                               uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    if (!s->ev.open)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_accumulate: no evidence_begin");
    if (thin < 1 || (!d_samples && n_steps > 0))
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_accumulate: bad arguments");
    const u64 kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    if (summary_closed(s->ev.n + kept, s->ev.bs) > s->ev.max_batches)
        return fail(APEMOST_HIP_ERR_INVALID,
                    "evidence_accumulate: %llu samples would close batch %llu, beyond max_batches = %llu",
                    (unsigned long long)(s->ev.n + kept), (unsigned long long)summary_closed(s->ev.n + kept, s->ev.bs),
                    (unsigned long long)s->ev.max_batches);
    if (kept == 0)
        return APEMOST_HIP_OK;
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const int nc = s->cfg.n_chains;
    for (u64 k0 = 0; k0 < kept; k0 += s->ev.chunk) {
        EvidenceArgs a;
        a.rows = d_samples;
        a.n_chains = nc;
        a.n_par = s->cfg.n_par;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < s->ev.chunk ? kept - k0 : s->ev.chunk);
        a.first = s->ev.n == 0;
        a.bs = s->ev.bs;
        a.left = summary_left(s->ev.n, s->ev.bs);
        a.n_closed = summary_closed(s->ev.n, s->ev.bs);
        a.batch_stride = s->ev.max_batches + 1;
        a.coef = s->ev.d_coef;
        a.vals = s->ev.d_vals;
        a.origin = s->ev.d_origin;
        a.sum = s->ev.d_sum;
        a.sq = s->ev.d_sq;
        a.batch = s->ev.d_batch;
        a.m = s->ev.d_m;
        a.S = s->ev.d_S;
        hipLaunchKernelGGL(evidence_gather_kernel,
                           dim3((unsigned)((nc + kEvidenceGatherThreads - 1) / kEvidenceGatherThreads), (a.n + 7u) / 8u),
                           dim3(kEvidenceGatherThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(evidence_fold_kernel,
                           dim3((unsigned)((nc + kEvidenceThreads - 1) / kEvidenceThreads), (unsigned)kEvidenceQuantities),
                           dim3(kEvidenceThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        s->ev.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int evidence_xfer(apemost_hip_sampler *s, const apemost_hip_evidence_view *v, bool up) {
    if (!s->ev.open)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_%s: no evidence_begin", up ? "set" : "get");
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence view is NULL");
    if (up && v->n && summary_closed(*v->n, s->ev.bs) > s->ev.max_batches)
        return fail(APEMOST_HIP_ERR_INVALID, "evidence_set: %llu samples close more than max_batches batches",
                    (unsigned long long)*v->n);
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    const size_t nc = (size_t)s->cfg.n_chains;
    // stream order: behind every accumulate queued so far, on the stream they run on
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
#define EVIDENCE_COPY(dev, host, bytes)                                                                        \
    do {                                                                                                       \
        if ((host) && (bytes) > 0)                                                                             \
            HIP_TRY(up ? hipMemcpyAsync((void *)(dev), (const void *)(host), (bytes), kind, s->copy_stream)    \
                       : hipMemcpyAsync((void *)(host), (const void *)(dev), (bytes), kind, s->copy_stream));  \
    } while (0)
    EVIDENCE_COPY(s->ev.d_origin, v->origin, nc * sizeof(double));
    EVIDENCE_COPY(s->ev.d_sum, v->sum, nc * sizeof(double));
    EVIDENCE_COPY(s->ev.d_sq, v->sq, nc * sizeof(double));
    EVIDENCE_COPY(s->ev.d_batch, v->batch, nc * (s->ev.max_batches + 1) * sizeof(double));
    EVIDENCE_COPY(s->ev.d_m, v->m, 2 * nc * sizeof(double));
    EVIDENCE_COPY(s->ev.d_S, v->S, 2 * nc * sizeof(double));
#undef EVIDENCE_COPY
    HIP_TRY(hipStreamSynchronize(s->copy_stream));
    if (v->n) {
        if (up)
            s->ev.n = *v->n;
        else
            *v->n = s->ev.n;
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_evidence_get(apemost_hip_sampler *s, const apemost_hip_evidence_view *v) {
    CHECK_S(s);
    return evidence_xfer(s, v, false);
}

extern "C" int apemost_hip_evidence_set(apemost_hip_sampler *s, const apemost_hip_evidence_view *v) {
    CHECK_S(s);
    return evidence_xfer(s, v, true);
}

extern "C" int apemost_hip_evidence_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    evidence_free(s);
    return APEMOST_HIP_OK;
}

// ---- on-device autocorrelation (pt_autocorr.h) ----
extern "C" int apemost_hip_autocorr_begin(apemost_hip_sampler *s, const apemost_hip_autocorr_config *cfg) {
    CHECK_S(s);
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr_begin: config is NULL");
    const int np = s->cfg.n_par;
    if (cfg->n_keep < 1 || cfg->n_keep > s->cfg.n_chains || !cfg->chains)
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr_begin: n_keep %d outside [1,%d], or no chains", cfg->n_keep,
                    s->cfg.n_chains);
    for (int k = 0; k < cfg->n_keep; k++)
        if (cfg->chains[k] < 0 || cfg->chains[k] >= s->cfg.n_chains || (k > 0 && cfg->chains[k] <= cfg->chains[k - 1]))
            return fail(APEMOST_HIP_ERR_INVALID,
                        "autocorr_begin: chains[%d] = %d: local chain indices in [0,%d), strictly increasing", k,
                        cfg->chains[k], s->cfg.n_chains);
    if (cfg->max_lag < 1 || cfg->max_lag > kAutocorrMaxLag)
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr_begin: max_lag %d outside [1,%d]", cfg->max_lag, kAutocorrMaxLag);
    std::vector<int> cols;
    if (!cfg->cols) { // the parameters and prob - prior
        for (int p = 0; p < np; p++)
            cols.push_back(p);
        cols.push_back(np + 1);
    } else {
        if (cfg->n_cols < 1 || cfg->n_cols > np + 2)
            return fail(APEMOST_HIP_ERR_INVALID, "autocorr_begin: n_cols %d outside [1,%d]", cfg->n_cols, np + 2);
        for (int c = 0; c < cfg->n_cols; c++) {
            if (cfg->cols[c] < 0 || cfg->cols[c] > np + 1 || (c > 0 && cfg->cols[c] <= cfg->cols[c - 1]))
                return fail(APEMOST_HIP_ERR_INVALID,
                            "autocorr_begin: cols[%d] = %d: column indices in [0,%d], strictly increasing", c, cfg->cols[c],
                            np + 1);
            cols.push_back(cfg->cols[c]);
        }
    }
    const u64 n_series = (u64)cfg->n_keep * cols.size();
    const u64 L = (u64)cfg->max_lag, H = L - 1;
    if (n_series > 65535 || n_series * L > ((u64)1 << 24))
        return fail(APEMOST_HIP_ERR_INVALID,
                    "autocorr_begin: %d chains x %zu columns x %d lags: more than 65535 series or 2^24 lag sums",
                    cfg->n_keep, cols.size(), cfg->max_lag);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream)); // a fold begun before may still be accumulating
    autocorr_free(s);
    // the staged series: about 1 Mi values over all of them, at least 256 and at most 2^16 kept steps per launch
    u64 chunk = ((u64)1 << 20) / n_series;
    chunk = chunk < 256 ? 256 : chunk > ((u64)1 << 16) ? (u64)1 << 16 : chunk;
    s->ac.n_keep = cfg->n_keep;
    s->ac.n_cols = (int)cols.size();
    s->ac.max_lag = cfg->max_lag;
    s->ac.chunk = chunk;
    s->ac.n = 0;
    const size_t nh = (size_t)(n_series * (H > 0 ? H : 1));
    HIP_TRY(hipMalloc((void **)&s->ac.d_chains, cfg->n_keep * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&s->ac.d_cols, cols.size() * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&s->ac.d_buf, n_series * (H + chunk) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ac.d_origin, n_series * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ac.d_sum, n_series * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ac.d_lag, n_series * L * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ac.d_head, nh * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->ac.d_tail, nh * sizeof(double)));
    HIP_TRY(hipMemsetAsync(s->ac.d_origin, 0, n_series * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ac.d_sum, 0, n_series * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ac.d_lag, 0, n_series * L * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ac.d_head, 0, nh * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->ac.d_tail, 0, nh * sizeof(double), s->stream));
    HIP_TRY(hipMemcpyAsync(s->ac.d_chains, cfg->chains, cfg->n_keep * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->ac.d_cols, cols.data(), cols.size() * sizeof(int), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream)); // (`cols` and the caller's arrays are read until here)
    s->ac.open = true;
    return APEMOST_HIP_OK;
}

// Queued on copy_stream behind everything launched so far on the sampler's stream, like
// apemost_hip_summary_accumulate; apemost_hip_samples_wait covers it.
extern "C" int apemost_hip_autocorr_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                               uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    if (!s->ac.open)
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr_accumulate: no autocorr_begin");
    if (thin < 1 || (!d_samples && n_steps > 0))
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr_accumulate: bad arguments");
    const u64 kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    if (kept == 0)
        return APEMOST_HIP_OK;
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const unsigned n_series = (unsigned)(s->ac.n_keep * s->ac.n_cols);
    const unsigned H = (unsigned)s->ac.max_lag - 1u;
    for (u64 k0 = 0; k0 < kept; k0 += s->ac.chunk) {
        AutocorrArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = s->cfg.n_par;
        a.n_keep = s->ac.n_keep;
        a.n_cols = s->ac.n_cols;
        a.chains = s->ac.d_chains;
        a.cols = s->ac.d_cols;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < s->ac.chunk ? kept - k0 : s->ac.chunk);
        a.n0 = s->ac.n;
        a.max_lag = s->ac.max_lag;
        a.n_groups = (s->ac.max_lag + kAutocorrGroup - 1) / kAutocorrGroup;
        a.stride = H + s->ac.chunk;
        a.buf = s->ac.d_buf;
        a.origin = s->ac.d_origin;
        a.sum = s->ac.d_sum;
        a.lag = s->ac.d_lag;
        a.head = s->ac.d_head;
        a.tail = s->ac.d_tail;
        hipLaunchKernelGGL(autocorr_gather_kernel, dim3((H + a.n + kAutocorrThreads - 1) / kAutocorrThreads, n_series),
                           dim3(kAutocorrThreads), 0, s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(autocorr_fold_kernel, dim3((unsigned)a.n_groups + 1u, n_series), dim3(kAutocorrWave), 0,
                           s->copy_stream, a);
        HIP_TRY(hipGetLastError());
        if (H > 0) {
            hipLaunchKernelGGL(autocorr_carry_kernel, dim3((H + kAutocorrThreads - 1) / kAutocorrThreads, n_series),
                               dim3(kAutocorrThreads), 0, s->copy_stream, a);
            HIP_TRY(hipGetLastError());
        }
        s->ac.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int autocorr_xfer(apemost_hip_sampler *s, const apemost_hip_autocorr_view *v, bool up) {
    if (!s->ac.open)
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr_%s: no autocorr_begin", up ? "set" : "get");
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "autocorr view is NULL");
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    const size_t n_series = (size_t)s->ac.n_keep * s->ac.n_cols, L = (size_t)s->ac.max_lag, H = L - 1;
    // stream order: behind every accumulate queued so far, on the stream they run on
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
#define AUTOCORR_COPY(dev, host, bytes)                                                                        \
    do {                                                                                                       \
        if ((host) && (bytes) > 0)                                                                             \
            HIP_TRY(up ? hipMemcpyAsync((void *)(dev), (const void *)(host), (bytes), kind, s->copy_stream)    \
                       : hipMemcpyAsync((void *)(host), (const void *)(dev), (bytes), kind, s->copy_stream));  \
    } while (0)
    AUTOCORR_COPY(s->ac.d_origin, v->origin, n_series * sizeof(double));
    AUTOCORR_COPY(s->ac.d_sum, v->sum, n_series * sizeof(double));
    AUTOCORR_COPY(s->ac.d_lag, v->lag, n_series * L * sizeof(double));
    AUTOCORR_COPY(s->ac.d_head, v->head, n_series * H * sizeof(double));
    AUTOCORR_COPY(s->ac.d_tail, v->tail, n_series * H * sizeof(double));
#undef AUTOCORR_COPY
    HIP_TRY(hipStreamSynchronize(s->copy_stream));
    if (v->n) {
        if (up)
            s->ac.n = *v->n;
        else
            *v->n = s->ac.n;
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_autocorr_get(apemost_hip_sampler *s, const apemost_hip_autocorr_view *v) {
    CHECK_S(s);
    return autocorr_xfer(s, v, false);
}

extern "C" int apemost_hip_autocorr_set(apemost_hip_sampler *s, const apemost_hip_autocorr_view *v) {
    CHECK_S(s);
    return autocorr_xfer(s, v, true);
}

extern "C" int apemost_hip_autocorr_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    autocorr_free(s);
    return APEMOST_HIP_OK;
}

// ---- on-device posterior predictive (pt_predict.h) ----
// a built-in model, or a user-supplied one with the curve hook (its analysis module is built here on first use)
#define PREDICT_HAS_CURVE(s, what)                                                                                \
    do {                                                                                                        \
        if ((s)->cfg.model == APEMOST_MODEL_USER) {                                                             \
            const int rc_hooks = user_analysis(s);                                                              \
            if (rc_hooks != APEMOST_HIP_OK)                                                                     \
                return rc_hooks;                                                                                \
            if (!(s)->ua.has_curve)                                                                             \
                return fail(APEMOST_HIP_ERR_UNSUPPORTED,                                                        \
                            what ": this user-supplied device model has no curve: it does not define the hook " \
                                 "apemost_user_curve (APEMOST_USER_CURVE, include/apemost_device_model.h)");    \
        }                                                                                                       \
    } while (0)

static hipError_t user_launch(hipFunction_t f, unsigned grid, unsigned block, size_t lds, hipStream_t stream, void **params) {
    return hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, (unsigned)lds, stream, params, nullptr);
}

// host rows [n][n_cols], row-major like m->data -> a ctx's data, [n_cols][n]
static std::vector<double> rows_by_columns(const double *rows, int n, int n_cols) {
    std::vector<double> out((size_t)n * n_cols);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n_cols; j++)
            out[(size_t)j * n + i] = rows[(size_t)i * n_cols + j];
    return out;
}

static hipError_t predict_launch_fold(apemost_hip_sampler *s, const PredictArgs &a) {
    const dim3 grid((unsigned)(a.n_blocks + 1) * (unsigned)a.n_keep), block(kPredictWave);
    const size_t lds = predict_lds_bytes(a.nbins, a.points);
    if (s->cfg.model == APEMOST_MODEL_USER) {
        void *params[] = {const_cast<PredictArgs *>(&a)};
        return user_launch(a.nbins > 0 ? s->ua.predict_fold_hist : s->ua.predict_fold, grid.x, block.x,
                           a.nbins > 0 ? lds : 0, s->copy_stream, params);
    }
#define PREDICT_FOLD(M)                                                                                          \
    do {                                                                                                         \
        if (a.nbins > 0)                                                                                         \
            hipLaunchKernelGGL((predict_fold_kernel<M, true>), grid, block, lds, s->copy_stream, a);            \
        else                                                                                                     \
            hipLaunchKernelGGL((predict_fold_kernel<M, false>), grid, block, 0, s->copy_stream, a);             \
    } while (0)
    switch (s->cfg.model) {
    case APEMOST_MODEL_SIMPLESIN: PREDICT_FOLD(APEMOST_MODEL_SIMPLESIN); break;
    case APEMOST_MODEL_SINE3: PREDICT_FOLD(APEMOST_MODEL_SINE3); break;
    case APEMOST_MODEL_PULSE: PREDICT_FOLD(APEMOST_MODEL_PULSE); break;
    default: PREDICT_FOLD(APEMOST_MODEL_PULSE_VROT); break;
    }
#undef PREDICT_FOLD
    return hipGetLastError();
}

extern "C" int apemost_hip_predict_begin(apemost_hip_sampler *s, const apemost_hip_predict_config *cfg) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_begin");
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: config is NULL");
    const int np = s->cfg.n_par;
    if (cfg->n_keep < 1 || cfg->n_keep > s->cfg.n_chains || !cfg->chains)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: n_keep %d outside [1,%d], or no chains", cfg->n_keep,
                    s->cfg.n_chains);
    for (int k = 0; k < cfg->n_keep; k++)
        if (cfg->chains[k] < 0 || cfg->chains[k] >= s->cfg.n_chains || (k > 0 && cfg->chains[k] <= cfg->chains[k - 1]))
            return fail(APEMOST_HIP_ERR_INVALID,
                        "predict_begin: chains[%d] = %d: local chain indices in [0,%d), strictly increasing", k,
                        cfg->chains[k], s->cfg.n_chains);
    const int n_x = cfg->x ? cfg->n_x : s->cfg.n_data;
    if (n_x < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: n_x %d < 1", n_x);
    // a user model's abscissae are whole rows: [n_x][n_cols] from the caller, or the sampler's data
    const bool user = s->cfg.model == APEMOST_MODEL_USER;
    const int nc = user ? s->cfg.n_cols : 1;
    if (cfg->x)
        for (size_t i = 0; i < (size_t)n_x * nc; i++)
            if (!std::isfinite(cfg->x[i]))
                return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: x[%zu] is not finite", i);
    if (cfg->nbins < 0 || cfg->nbins > kPredictMaxBins)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: nbins %d outside [0,%d]", cfg->nbins, kPredictMaxBins);
    if (cfg->nbins > 0 && !(std::isfinite(cfg->lo) && std::isfinite(cfg->hi) && cfg->lo < cfg->hi))
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: the histogram range [%g, %g] is not finite with lo < hi",
                    cfg->lo, cfg->hi);
    const u64 n_series = (u64)cfg->n_keep * (u64)n_x;
    if (n_series > ((u64)1 << 20) || n_series * (u64)cfg->nbins > ((u64)1 << 26))
        return fail(APEMOST_HIP_ERR_INVALID,
                    "predict_begin: %d chains x %d abscissae x %d bins: more than 2^20 series or 2^26 counts", cfg->n_keep,
                    n_x, cfg->nbins);
    if (np > kPredictTile)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_begin: %d parameters, more than %d", np, kPredictTile);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream)); // a fold begun before may still be accumulating
    predict_free(s);
    s->pr.n_keep = cfg->n_keep;
    s->pr.n_x = n_x;
    s->pr.n_cols = nc;
    s->pr.nbins = cfg->nbins;
    s->pr.points = predict_points(cfg->nbins);
    s->pr.lo = cfg->lo;
    s->pr.hi = cfg->hi;
    s->pr.n = 0;
    const size_t ns = (size_t)n_series, nk = (size_t)cfg->n_keep, nh = ns * (size_t)cfg->nbins;
    HIP_TRY(hipMalloc((void **)&s->pr.d_chains, nk * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_x, ns * nc * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_origin, ns * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_sum, ns * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_sq, ns * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_vmin, ns * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_vmax, ns * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_hist, (nh ? nh : 1) * sizeof(u64)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_best_prob, nk * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_best_params, nk * np * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pr.d_best_n, nk * sizeof(u64)));
    HIP_TRY(hipMemsetAsync(s->pr.d_origin, 0, ns * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->pr.d_sum, 0, ns * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->pr.d_sq, 0, ns * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->pr.d_hist, 0, (nh ? nh : 1) * sizeof(u64), s->stream));
    HIP_TRY(hipMemsetAsync(s->pr.d_best_params, 0, nk * np * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->pr.d_best_n, 0, nk * sizeof(u64), s->stream));
    std::vector<double> pinf(ns, INFINITY), ninf(ns, -INFINITY);
    HIP_TRY(hipMemcpyAsync(s->pr.d_vmin, pinf.data(), ns * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->pr.d_vmax, ninf.data(), ns * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->pr.d_best_prob, ninf.data(), nk * sizeof(double), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(s->pr.d_chains, cfg->chains, nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    const std::vector<double> by_cols = cfg->x && user ? rows_by_columns(cfg->x, n_x, nc) : std::vector<double>();
    const double *host_x = by_cols.empty() ? cfg->x : by_cols.data();
    for (int k = 0; k < cfg->n_keep; k++) {
        double *dst = s->pr.d_x + (size_t)k * nc * n_x;
        if (cfg->x) {
            HIP_TRY(hipMemcpyAsync(dst, host_x, (size_t)nc * n_x * sizeof(double), hipMemcpyHostToDevice, s->stream));
        } else { // column 0 of the kept chain's own ladder (the data is stored by columns, ladder after ladder);
                 // a user model: all of its columns
            const int ladder = s->batch ? cfg->chains[k] / s->per_ladder : 0;
            const double *col0 = s->d.data + (size_t)ladder * s->cfg.n_cols * s->cfg.n_data;
            HIP_TRY(hipMemcpyAsync(dst, col0, (size_t)nc * n_x * sizeof(double), hipMemcpyDeviceToDevice, s->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's arrays are read until here)
    s->pr.open = true;
    return APEMOST_HIP_OK;
}

// Queued on copy_stream behind everything launched so far on the sampler's stream, like
// apemost_hip_autocorr_accumulate; apemost_hip_samples_wait covers it.
extern "C" int apemost_hip_predict_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                              uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_accumulate");
    if (!s->pr.open)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_accumulate: no predict_begin");
    if (thin < 1 || (!d_samples && n_steps > 0))
        return fail(APEMOST_HIP_ERR_INVALID, "predict_accumulate: bad arguments");
    const u64 kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    if (kept == 0)
        return APEMOST_HIP_OK;
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    for (u64 k0 = 0; k0 < kept; k0 += kPredictPiece) {
        PredictArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = s->cfg.n_par;
        a.n_keep = s->pr.n_keep;
        a.chains = s->pr.d_chains;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < (u64)kPredictPiece ? kept - k0 : (u64)kPredictPiece);
        a.n0 = s->pr.n;
        a.n_x = s->pr.n_x;
        a.x = s->pr.d_x;
        a.n_cols = s->pr.n_cols;
        a.sigma = s->sh.consts.sigma;
        a.hmin = s->sh.consts.hmin;
        a.nbins = s->pr.nbins;
        a.points = s->pr.points;
        a.n_blocks = (s->pr.n_x + s->pr.points - 1) / s->pr.points;
        a.lo = s->pr.lo;
        a.hi = s->pr.hi;
        a.origin = s->pr.d_origin;
        a.sum = s->pr.d_sum;
        a.sq = s->pr.d_sq;
        a.vmin = s->pr.d_vmin;
        a.vmax = s->pr.d_vmax;
        a.hist = s->pr.d_hist;
        a.best_prob = s->pr.d_best_prob;
        a.best_params = s->pr.d_best_params;
        a.best_n = s->pr.d_best_n;
        HIP_TRY(predict_launch_fold(s, a));
        s->pr.n += a.n;
    }
    return APEMOST_HIP_OK;
}

static int predict_xfer(apemost_hip_sampler *s, const apemost_hip_predict_view *v, bool up) {
    if (!s->pr.open)
        return fail(APEMOST_HIP_ERR_INVALID, "predict_%s: no predict_begin", up ? "set" : "get");
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "predict view is NULL");
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    const size_t nk = (size_t)s->pr.n_keep, ns = nk * s->pr.n_x, np = (size_t)s->cfg.n_par;
    // stream order: behind every accumulate queued so far, on the stream they run on
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
#define PREDICT_COPY(dev, host, bytes)                                                                         \
    do {                                                                                                       \
        if ((host) && (bytes) > 0)                                                                             \
            HIP_TRY(up ? hipMemcpyAsync((void *)(dev), (const void *)(host), (bytes), kind, s->copy_stream)    \
                       : hipMemcpyAsync((void *)(host), (const void *)(dev), (bytes), kind, s->copy_stream));  \
    } while (0)
    PREDICT_COPY(s->pr.d_origin, v->origin, ns * sizeof(double));
    PREDICT_COPY(s->pr.d_sum, v->sum, ns * sizeof(double));
    PREDICT_COPY(s->pr.d_sq, v->sq, ns * sizeof(double));
    PREDICT_COPY(s->pr.d_vmin, v->vmin, ns * sizeof(double));
    PREDICT_COPY(s->pr.d_vmax, v->vmax, ns * sizeof(double));
    PREDICT_COPY(s->pr.d_hist, v->hist, ns * s->pr.nbins * sizeof(u64));
    PREDICT_COPY(s->pr.d_best_prob, v->best_prob, nk * sizeof(double));
    PREDICT_COPY(s->pr.d_best_params, v->best_params, nk * np * sizeof(double));
    PREDICT_COPY(s->pr.d_best_n, v->best_n, nk * sizeof(u64));
#undef PREDICT_COPY
    HIP_TRY(hipStreamSynchronize(s->copy_stream));
    if (v->n) {
        if (up)
            s->pr.n = *v->n;
        else
            *v->n = s->pr.n;
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_predict_get(apemost_hip_sampler *s, const apemost_hip_predict_view *v) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_get");
    return predict_xfer(s, v, false);
}

extern "C" int apemost_hip_predict_set(apemost_hip_sampler *s, const apemost_hip_predict_view *v) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_set");
    return predict_xfer(s, v, true);
}

extern "C" int apemost_hip_predict_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_end");
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    predict_free(s);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_predict_curve(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x,
                                         const double *x, double *out) {
    CHECK_S(s);
    PREDICT_HAS_CURVE(s, "predict_curve");
    if (!x)
        n_x = s->cfg.n_data;
    if (n < 1 || !params || !out || n_x < 1 || (u64)n * (u64)n_x > ((u64)1 << 26))
        return fail(APEMOST_HIP_ERR_INVALID, "predict_curve: %d rows x %d abscissae, or a NULL array", n, n_x);
    const int np = s->cfg.n_par;
    const bool user = s->cfg.model == APEMOST_MODEL_USER;
    int nc = user ? s->cfg.n_cols : 1; // a user model's abscissae are whole rows [n_x][n_cols], finite
    std::vector<double> by_cols;
    if (user && x) {
        for (size_t i = 0; i < (size_t)n_x * nc; i++)
            if (!std::isfinite(x[i]))
                return fail(APEMOST_HIP_ERR_INVALID, "predict_curve: x[%zu] is not finite", i);
        by_cols = rows_by_columns(x, n_x, nc);
        x = by_cols.data();
    }
    double *d_par = nullptr, *d_x = nullptr, *d_out = nullptr;
    hipError_t err = hipMalloc((void **)&d_par, (size_t)n * np * sizeof(double));
    if (err == hipSuccess)
        err = hipMalloc((void **)&d_x, (size_t)nc * n_x * sizeof(double));
    if (err == hipSuccess)
        err = hipMalloc((void **)&d_out, (size_t)n * n_x * sizeof(double));
    if (err == hipSuccess)
        err = hipMemcpyAsync(d_par, params, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, s->stream);
    if (err == hipSuccess)
        err = x ? hipMemcpyAsync(d_x, x, (size_t)nc * n_x * sizeof(double), hipMemcpyHostToDevice, s->stream)
                : hipMemcpyAsync(d_x, s->d.data, (size_t)nc * n_x * sizeof(double), hipMemcpyDeviceToDevice, s->stream);
    if (err == hipSuccess && user) {
        int np_ = np;
        double sigma = s->sh.consts.sigma, hmin = s->sh.consts.hmin;
        void *params_[] = {&d_par, &np_, &n_x, &nc, &d_x, &sigma, &hmin, &d_out};
        err = user_launch(s->ua.predict_curve, (unsigned)((n_x + kPredictWave - 1) / kPredictWave) * (unsigned)n,
                          kPredictWave, 0, s->stream, params_);
    } else if (err == hipSuccess) {
        const dim3 grid((unsigned)((n_x + kPredictWave - 1) / kPredictWave) * (unsigned)n), block(kPredictWave);
        switch (s->cfg.model) {
        case APEMOST_MODEL_SIMPLESIN:
            hipLaunchKernelGGL(predict_curve_kernel<APEMOST_MODEL_SIMPLESIN>, grid, block, 0, s->stream, d_par, np, n_x, d_x, d_out);
            break;
        case APEMOST_MODEL_SINE3:
            hipLaunchKernelGGL(predict_curve_kernel<APEMOST_MODEL_SINE3>, grid, block, 0, s->stream, d_par, np, n_x, d_x, d_out);
            break;
        case APEMOST_MODEL_PULSE:
            hipLaunchKernelGGL(predict_curve_kernel<APEMOST_MODEL_PULSE>, grid, block, 0, s->stream, d_par, np, n_x, d_x, d_out);
            break;
        default:
            hipLaunchKernelGGL(predict_curve_kernel<APEMOST_MODEL_PULSE_VROT>, grid, block, 0, s->stream, d_par, np, n_x, d_x, d_out);
            break;
        }
        err = hipGetLastError();
    }
    if (err == hipSuccess)
        err = hipMemcpyAsync(out, d_out, (size_t)n * n_x * sizeof(double), hipMemcpyDeviceToHost, s->stream);
    const hipError_t sync = hipStreamSynchronize(s->stream);
    for (double *p : {d_par, d_x, d_out})
        if (p)
            hipFree(p);
    HIP_TRY(err);
    HIP_TRY(sync);
    return APEMOST_HIP_OK;
}

// ---- on-device pointwise log-likelihood (pt_pointwise.h) ----
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

static double pointwise_c(const apemost_hip_sampler *s) {
    const double sigma = s->sh.consts.sigma;
    const double t = -2.0 * sigma;
    const double denom = t * sigma;
    return 1.0 / denom;
}

extern "C" int apemost_hip_pointwise_begin(apemost_hip_sampler *s, const apemost_hip_pointwise_config *cfg) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_begin");
    if (!cfg)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin: config is NULL");
    const int np = s->cfg.n_par, nd = s->cfg.n_data;
    if (cfg->n_keep < 1 || cfg->n_keep > s->cfg.n_chains || !cfg->chains)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin: n_keep %d outside [1,%d], or no chains", cfg->n_keep,
                    s->cfg.n_chains);
    for (int k = 0; k < cfg->n_keep; k++)
        if (cfg->chains[k] < 0 || cfg->chains[k] >= s->cfg.n_chains || (k > 0 && cfg->chains[k] <= cfg->chains[k - 1]))
            return fail(APEMOST_HIP_ERR_INVALID,
                        "pointwise_begin: chains[%d] = %d: local chain indices in [0,%d), strictly increasing", k,
                        cfg->chains[k], s->cfg.n_chains);
    const u64 n_series = (u64)cfg->n_keep * (u64)nd;
    if (n_series > ((u64)1 << 20))
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin: %d chains x %d data: more than 2^20 series", cfg->n_keep,
                    nd);
    if (np > kPointwiseTile)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_begin: %d parameters, more than %d", np, kPointwiseTile);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream)); // a fold begun before may still be accumulating
    pointwise_free(s);
    s->pw.n_keep = cfg->n_keep;
    s->pw.c = pointwise_c(s);
    s->pw.n = 0;
    const size_t ns = (size_t)n_series, nk = (size_t)cfg->n_keep;
    const bool user = s->cfg.model == APEMOST_MODEL_USER;
    const size_t nc = user ? (size_t)s->cfg.n_cols : 1; // a user model's data: all of its columns, in d_x
    HIP_TRY(hipMalloc((void **)&s->pw.d_chains, nk * sizeof(int)));
    HIP_TRY(hipMalloc((void **)&s->pw.d_x, ns * nc * sizeof(double)));
    if (!user)
        HIP_TRY(hipMalloc((void **)&s->pw.d_y, ns * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pw.d_state, kPointwiseWords * ns * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&s->pw.d_par, 2 * nk * np * sizeof(double)));
    HIP_TRY(hipMemsetAsync(s->pw.d_state, 0, kPointwiseWords * ns * sizeof(double), s->stream));
    HIP_TRY(hipMemsetAsync(s->pw.d_par, 0, 2 * nk * np * sizeof(double), s->stream));
    HIP_TRY(hipMemcpyAsync(s->pw.d_chains, cfg->chains, nk * sizeof(int), hipMemcpyHostToDevice, s->stream));
    for (int k = 0; k < cfg->n_keep; k++) {
        // columns 0 and 1 of the kept chain's own ladder (the data is stored by columns, ladder after ladder)
        const int ladder = s->batch ? cfg->chains[k] / s->per_ladder : 0;
        const double *col0 = s->d.data + (size_t)ladder * s->cfg.n_cols * nd;
        HIP_TRY(hipMemcpyAsync(s->pw.d_x + (size_t)k * nc * nd, col0, nc * nd * sizeof(double), hipMemcpyDeviceToDevice,
                               s->stream));
        if (!user)
            HIP_TRY(hipMemcpyAsync(s->pw.d_y + (size_t)k * nd, col0 + nd, (size_t)nd * sizeof(double),
                               hipMemcpyDeviceToDevice, s->stream));
    }
    HIP_TRY(hipStreamSynchronize(s->stream)); // (the caller's array is read until here)
    s->pw.open = true;
    return APEMOST_HIP_OK;
}

// ---- the tail of the pointwise fold (pt_pointwise_tail.h) ----
static PointwiseTailArgs pointwise_tail_args(const apemost_hip_sampler *s, bool force) {
    PointwiseTailArgs t;
    t.buf = s->pw.tail.d_buf;
    t.slots = s->pw.tail.d_slots;
    t.thr = s->pw.tail.d_thr;
    t.capacity = s->pw.tail.capacity;
    t.B = s->pw.tail.B;
    t.n_data = s->cfg.n_data;
    t.n_blocks = (s->cfg.n_data + kPointwiseWave - 1) / kPointwiseWave;
    t.force = force ? 1 : 0;
    t.dense = nullptr;
    t.count = nullptr;
    return t;
}

static int pointwise_tail_compact(apemost_hip_sampler *s, bool force) {
    const PointwiseTailArgs t = pointwise_tail_args(s, force);
    const dim3 grid((unsigned)s->pw.n_keep * (unsigned)s->cfg.n_data), block(kTailThreads);
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
        switch (s->cfg.model) {
        case APEMOST_MODEL_USER: {
            void *params[] = {&a, &tt};
            HIP_TRY(user_launch(s->ua.pointwise_tail_append, grid.x, block.x, 0, s->copy_stream, params));
            break;
        }
        case APEMOST_MODEL_SIMPLESIN:
            hipLaunchKernelGGL(pointwise_tail_append_kernel<APEMOST_MODEL_SIMPLESIN>, grid, block, 0, s->copy_stream, a, tt);
            break;
        case APEMOST_MODEL_SINE3:
            hipLaunchKernelGGL(pointwise_tail_append_kernel<APEMOST_MODEL_SINE3>, grid, block, 0, s->copy_stream, a, tt);
            break;
        case APEMOST_MODEL_PULSE:
            hipLaunchKernelGGL(pointwise_tail_append_kernel<APEMOST_MODEL_PULSE>, grid, block, 0, s->copy_stream, a, tt);
            break;
        default:
            hipLaunchKernelGGL(pointwise_tail_append_kernel<APEMOST_MODEL_PULSE_VROT>, grid, block, 0, s->copy_stream, a, tt);
            break;
        }
        HIP_TRY(hipGetLastError());
        const int rc = pointwise_tail_compact(s, false);
        if (rc != APEMOST_HIP_OK)
            return rc;
    }
    return APEMOST_HIP_OK;
}

// Queued on copy_stream behind everything launched so far on the sampler's stream, like
// apemost_hip_predict_accumulate; apemost_hip_samples_wait covers it.
extern "C" int apemost_hip_pointwise_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                                uint64_t skip, uint64_t thin) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_accumulate");
    if (!s->pw.open)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_accumulate: no pointwise_begin");
    if (thin < 1 || (!d_samples && n_steps > 0))
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_accumulate: bad arguments");
    if (s->pw.tail.awaits_set)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_accumulate: the tail was begun on a fold of %llu samples that "
                    "pointwise_set loaded: pointwise_tail_set must load the tail of those samples first",
                    (unsigned long long)s->pw.n);
    const u64 kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    if (kept == 0)
        return APEMOST_HIP_OK;
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const size_t ns = (size_t)s->pw.n_keep * s->cfg.n_data;
    for (u64 k0 = 0; k0 < kept; k0 += kPointwisePiece) {
        PointwiseArgs a;
        a.rows = d_samples;
        a.n_chains = s->cfg.n_chains;
        a.n_par = s->cfg.n_par;
        a.n_keep = s->pw.n_keep;
        a.chains = s->pw.d_chains;
        a.skip = skip + k0 * thin;
        a.thin = thin;
        a.n = (unsigned int)(kept - k0 < (u64)kPointwisePiece ? kept - k0 : (u64)kPointwisePiece);
        a.n0 = s->pw.n;
        a.n_data = s->cfg.n_data;
        a.n_blocks = (s->cfg.n_data + kPointwiseWave - 1) / kPointwiseWave;
        a.x = s->pw.d_x;
        a.y = s->pw.d_y;
        a.c = s->pw.c;
        a.n_cols = s->cfg.n_cols;
        a.sigma = s->sh.consts.sigma;
        a.hmin = s->sh.consts.hmin;
        a.origin = s->pw.d_state;
        a.sum = s->pw.d_state + ns;
        a.sq = s->pw.d_state + 2 * ns;
        a.m_up = s->pw.d_state + 3 * ns;
        a.S_up = s->pw.d_state + 4 * ns;
        a.m_dn = s->pw.d_state + 5 * ns;
        a.S_dn = s->pw.d_state + 6 * ns;
        a.S2_dn = s->pw.d_state + 7 * ns;
        a.par_origin = s->pw.d_par;
        a.par_sum = s->pw.d_par + (size_t)s->pw.n_keep * s->cfg.n_par;
        const dim3 grid((unsigned)(a.n_blocks + 1) * (unsigned)a.n_keep), block(kPointwiseWave);
        switch (s->cfg.model) {
        case APEMOST_MODEL_USER: {
            void *params[] = {&a};
            HIP_TRY(user_launch(s->ua.pointwise_fold, grid.x, block.x, 0, s->copy_stream, params));
            break;
        }
        case APEMOST_MODEL_SIMPLESIN:
            hipLaunchKernelGGL(pointwise_fold_kernel<APEMOST_MODEL_SIMPLESIN>, grid, block, 0, s->copy_stream, a);
            break;
        case APEMOST_MODEL_SINE3:
            hipLaunchKernelGGL(pointwise_fold_kernel<APEMOST_MODEL_SINE3>, grid, block, 0, s->copy_stream, a);
            break;
        case APEMOST_MODEL_PULSE:
            hipLaunchKernelGGL(pointwise_fold_kernel<APEMOST_MODEL_PULSE>, grid, block, 0, s->copy_stream, a);
            break;
        default:
            hipLaunchKernelGGL(pointwise_fold_kernel<APEMOST_MODEL_PULSE_VROT>, grid, block, 0, s->copy_stream, a);
            break;
        }
        HIP_TRY(hipGetLastError());
        if (s->pw.tail.capacity > 0) {
            rc = pointwise_tail_pieces(s, a);
            if (rc != APEMOST_HIP_OK)
                return rc;
        }
        s->pw.n += a.n;
        s->pw.n_set = false;
    }
    return APEMOST_HIP_OK;
}

static int pointwise_xfer(apemost_hip_sampler *s, const apemost_hip_pointwise_view *v, bool up) {
    if (!s->pw.open)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_%s: no pointwise_begin", up ? "set" : "get");
    if (!v)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise view is NULL");
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    const size_t nk = (size_t)s->pw.n_keep, ns = nk * s->cfg.n_data, np = (size_t)s->cfg.n_par;
    // stream order: behind every accumulate queued so far, on the stream they run on
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    const hipMemcpyKind kind = up ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
    double *const host[kPointwiseWords] = {v->origin, v->sum, v->sq, v->m_up, v->S_up, v->m_dn, v->S_dn, v->S2_dn};
#define POINTWISE_COPY(dev, hst, bytes)                                                                        \
    do {                                                                                                       \
        if ((hst) && (bytes) > 0)                                                                              \
            HIP_TRY(up ? hipMemcpyAsync((void *)(dev), (const void *)(hst), (bytes), kind, s->copy_stream)     \
                       : hipMemcpyAsync((void *)(hst), (const void *)(dev), (bytes), kind, s->copy_stream));   \
    } while (0)
    for (int q = 0; q < kPointwiseWords; q++)
        POINTWISE_COPY(s->pw.d_state + (size_t)q * ns, host[q], ns * sizeof(double));
    POINTWISE_COPY(s->pw.d_par, v->par_origin, nk * np * sizeof(double));
    POINTWISE_COPY(s->pw.d_par + nk * np, v->par_sum, nk * np * sizeof(double));
#undef POINTWISE_COPY
    HIP_TRY(hipStreamSynchronize(s->copy_stream));
    if (v->n) {
        if (up) {
            s->pw.n = *v->n;
            s->pw.n_set = true;
        } else
            *v->n = s->pw.n;
    }
    return APEMOST_HIP_OK;
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

extern "C" int apemost_hip_pointwise_end(apemost_hip_sampler *s) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_end");
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    pointwise_free(s);
    return APEMOST_HIP_OK;
}

// padded series (64 per block of data) times the slots of a series' buffer
static u64 pointwise_tail_slots(const apemost_hip_sampler *s, int B) {
    const u64 n_blocks = ((u64)s->cfg.n_data + kPointwiseWave - 1) / kPointwiseWave;
    return (u64)s->pw.n_keep * n_blocks * kPointwiseWave * (u64)B;
}

extern "C" int apemost_hip_pointwise_tail_begin(apemost_hip_sampler *s, int32_t capacity) {
    if (!s)
        return fail(APEMOST_HIP_ERR_INVALID, "sampler is NULL");
    if (capacity < 2 || capacity > kTailMaxCapacity)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: capacity %d outside [2,%d]", capacity, kTailMaxCapacity);
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_tail_begin");
    if (!s->pw.open)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: no pointwise_begin");
    if (s->pw.n > 0 && !s->pw.n_set)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: the fold has accumulated %llu samples whose tail is "
                    "lost: begin the tail before the first accumulate, or right behind pointwise_set",
                    (unsigned long long)s->pw.n);
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
                        s->pw.n_keep, s->cfg.n_data, B, capacity, fits);
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_begin: %d chains x %d data (in blocks of 64) x %d slots for "
                    "capacity %d: more than 2^28 slots (2 GiB); the largest capacity that fits is 0: no capacity fits, "
                    "keep fewer chains", s->pw.n_keep, s->cfg.n_data, B, capacity);
    }
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    pointwise_tail_free(s);
    const size_t ns = (size_t)s->pw.n_keep * s->cfg.n_data;
    double *buf = nullptr;
    unsigned int *slots = nullptr;
    unsigned long long *thr = nullptr;
    hipError_t err = hipMalloc((void **)&buf, (size_t)pointwise_tail_slots(s, B) * sizeof(double));
    if (err == hipSuccess)
        err = hipMalloc((void **)&slots, ns * sizeof(unsigned int));
    if (err == hipSuccess)
        err = hipMalloc((void **)&thr, ns * sizeof(unsigned long long));
    if (err == hipSuccess)
        err = hipMemsetAsync(slots, 0, ns * sizeof(unsigned int), s->stream);
    if (err == hipSuccess)
        err = hipMemsetAsync(thr, 0, ns * sizeof(unsigned long long), s->stream);
    if (err == hipSuccess)
        err = hipStreamSynchronize(s->stream);
    if (err != hipSuccess) { // the fold stays as it was, without a tail
        for (void *p : {(void *)buf, (void *)slots, (void *)thr})
            if (p)
                hipFree(p);
        HIP_TRY(err);
    }
    s->pw.tail.capacity = capacity;
    s->pw.tail.B = B;
    s->pw.tail.d_buf = buf;
    s->pw.tail.d_slots = slots;
    s->pw.tail.d_thr = thr;
    s->pw.tail.awaits_set = s->pw.n > 0;
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

static int pointwise_tail_xfer(apemost_hip_sampler *s, const apemost_hip_pointwise_tail_view *v, bool up) {
    const char *what = up ? "set" : "get";
    if (!s->pw.open || s->pw.tail.capacity == 0)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_%s: no pointwise_tail_begin", what);
    if (!v || !v->count || !v->values)
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_%s: the view or one of its arrays is NULL", what);
    const size_t ns = (size_t)s->pw.n_keep * s->cfg.n_data, cap = (size_t)s->pw.tail.capacity;
    if (up)
        for (size_t q = 0; q < ns; q++) {
            if (v->count[q] > cap)
                return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_set: count[%zu] = %llu, more than the capacity %zu", q,
                            (unsigned long long)v->count[q], cap);
            for (size_t j = 0; j < (size_t)v->count[q]; j++)
                if (v->values[q * cap + j] != v->values[q * cap + j])
                    return fail(APEMOST_HIP_ERR_INVALID, "pointwise_tail_set: values[%zu][%zu] is NaN: a tail holds none", q, j);
        }
    int rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    PointwiseTailArgs t = pointwise_tail_args(s, true);
    hipError_t err = hipMalloc((void **)&t.dense, ns * cap * sizeof(double));
    if (err == hipSuccess)
        err = hipMalloc((void **)&t.count, ns * sizeof(unsigned long long));
    const dim3 grid((unsigned)ns, (unsigned)((cap + kTailThreads - 1) / kTailThreads)), block(kTailThreads);
    if (err == hipSuccess && up) {
        err = hipMemcpyAsync(t.dense, v->values, ns * cap * sizeof(double), hipMemcpyHostToDevice, s->copy_stream);
        if (err == hipSuccess)
            err = hipMemcpyAsync(t.count, v->count, ns * sizeof(unsigned long long), hipMemcpyHostToDevice, s->copy_stream);
        if (err == hipSuccess) {
            hipLaunchKernelGGL(pointwise_tail_scatter_kernel, grid, block, 0, s->copy_stream, t);
            err = hipGetLastError();
        }
        if (err == hipSuccess) // sorts what was loaded and sets every threshold from it
            err = pointwise_tail_compact(s, true) == APEMOST_HIP_OK ? hipSuccess : hipErrorLaunchFailure;
    } else if (err == hipSuccess) {
        err = pointwise_tail_compact(s, true) == APEMOST_HIP_OK ? hipSuccess : hipErrorLaunchFailure;
        if (err == hipSuccess) {
            hipLaunchKernelGGL(pointwise_tail_gather_kernel, grid, block, 0, s->copy_stream, t);
            err = hipGetLastError();
        }
        if (err == hipSuccess)
            err = hipMemcpyAsync(v->values, t.dense, ns * cap * sizeof(double), hipMemcpyDeviceToHost, s->copy_stream);
        if (err == hipSuccess)
            err = hipMemcpyAsync(v->count, t.count, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, s->copy_stream);
    }
    const hipError_t sync = hipStreamSynchronize(s->copy_stream);
    for (void *p : {(void *)t.dense, (void *)t.count})
        if (p)
            hipFree(p);
    HIP_TRY(err);
    HIP_TRY(sync);
    if (up)
        s->pw.tail.awaits_set = false;
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_tail_get(apemost_hip_sampler *s, const apemost_hip_pointwise_tail_view *v) {
    CHECK_S(s);
    return pointwise_tail_xfer(s, v, false);
}

extern "C" int apemost_hip_pointwise_tail_set(apemost_hip_sampler *s, const apemost_hip_pointwise_tail_view *v) {
    CHECK_S(s);
    return pointwise_tail_xfer(s, v, true);
}

extern "C" int apemost_hip_pointwise_loglike_ladder(apemost_hip_sampler *s, int32_t ladder, int32_t n,
                                                    const double *params, double *out) {
    CHECK_S(s);
    POINTWISE_HAS_TERM(s, "pointwise_loglike");
    const int np = s->cfg.n_par, nd = s->cfg.n_data;
    if (ladder < 0 || ladder >= (s->batch ? s->n_ladders : 1))
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_loglike: ladder %d outside [0,%d)", ladder,
                    s->batch ? s->n_ladders : 1);
    if (n < 1 || !params || !out || (u64)n * (u64)nd > ((u64)1 << 26))
        return fail(APEMOST_HIP_ERR_INVALID, "pointwise_loglike: %d rows x %d data, or a NULL array", n, nd);
    double *d_par = nullptr, *d_out = nullptr;
    hipError_t err = hipMalloc((void **)&d_par, (size_t)n * np * sizeof(double));
    if (err == hipSuccess)
        err = hipMalloc((void **)&d_out, (size_t)n * nd * sizeof(double));
    if (err == hipSuccess)
        err = hipMemcpyAsync(d_par, params, (size_t)n * np * sizeof(double), hipMemcpyHostToDevice, s->stream);
    if (err == hipSuccess) {
        const dim3 grid((unsigned)((nd + kPointwiseWave - 1) / kPointwiseWave) * (unsigned)n), block(kPointwiseWave);
        // the ladder's columns 0 and 1 (the data is stored by columns, ladder after ladder)
        const double *x = s->d.data + (size_t)ladder * s->cfg.n_cols * nd, *y = x + nd;
        const double c = pointwise_c(s);
        switch (s->cfg.model) {
        case APEMOST_MODEL_USER: { // all n_cols columns of the ladder's rows
            int np_ = np, nd_ = nd, nc = s->cfg.n_cols;
            double sigma = s->sh.consts.sigma, hmin = s->sh.consts.hmin;
            void *params_[] = {&d_par, &np_, &nd_, &nc, &x, &sigma, &hmin, &d_out};
            err = user_launch(s->ua.pointwise_loglike, grid.x, block.x, 0, s->stream, params_);
            break;
        }
        case APEMOST_MODEL_SIMPLESIN:
            hipLaunchKernelGGL(pointwise_loglike_kernel<APEMOST_MODEL_SIMPLESIN>, grid, block, 0, s->stream, d_par, np, nd, x, y, c, d_out);
            break;
        case APEMOST_MODEL_SINE3:
            hipLaunchKernelGGL(pointwise_loglike_kernel<APEMOST_MODEL_SINE3>, grid, block, 0, s->stream, d_par, np, nd, x, y, c, d_out);
            break;
        case APEMOST_MODEL_PULSE:
            hipLaunchKernelGGL(pointwise_loglike_kernel<APEMOST_MODEL_PULSE>, grid, block, 0, s->stream, d_par, np, nd, x, y, c, d_out);
            break;
        default:
            hipLaunchKernelGGL(pointwise_loglike_kernel<APEMOST_MODEL_PULSE_VROT>, grid, block, 0, s->stream, d_par, np, nd, x, y, c, d_out);
            break;
        }
        if (err == hipSuccess)
            err = hipGetLastError();
    }
    if (err == hipSuccess)
        err = hipMemcpyAsync(out, d_out, (size_t)n * nd * sizeof(double), hipMemcpyDeviceToHost, s->stream);
    const hipError_t sync = hipStreamSynchronize(s->stream);
    for (double *p : {d_par, d_out})
        if (p)
            hipFree(p);
    HIP_TRY(err);
    HIP_TRY(sync);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_pointwise_loglike(apemost_hip_sampler *s, int32_t n, const double *params, double *out) {
    return apemost_hip_pointwise_loglike_ladder(s, 0, n, params, out);
}

// Host arithmetic only (no device): tools/peaks.c:130, 177-200 and the selection sort of src/gsl_helper.c:102-127.
extern "C" int apemost_hip_peaks_table(const apemost_hip_peaks_view *v, int32_t n_par, int32_t k, int32_t p,
                                       double *table, uint32_t *n_rows) {
    if (!v || !v->n_values || !v->n_peaks || !v->left || !v->right || !v->q || !v->q_set || !table || !n_rows)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_table: the view's n_values, n_peaks, left, right, q and q_set, "
                    "table and n_rows are all needed");
    if (n_par < 1 || k < 0 || p < 0 || p >= n_par)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_table: bad column (%d, %d) of %d parameters", k, p, n_par);
    const size_t col = (size_t)k * n_par + p;
    const uint32_t np = v->n_peaks[col];
    if (np > (uint32_t)kPeaksMax)
        return fail(APEMOST_HIP_ERR_INVALID, "peaks_table: kept chain %d, parameter %d: %u peaks, more than %d", k, p, np,
                    kPeaksMax);
    // a statistic whose index count is 0 keeps the value it had after the peak before (0 at the start)
    double stat[3] = {0, 0, 0}; // left quartile, median, right quartile
    double raw[kPeaksMax][4];   // share, median, left quartile, right quartile: the tool's four vectors
    for (uint32_t c = 0; c < np; c++) {
        const size_t at = col * kPeaksMax + c;
        for (int j = 0; j < 3; j++)
            if (v->q_set[at] >> j & 1)
                stat[j] = v->q[at * 3 + j];
        raw[c][0] = 1.0 * (double)(v->right[at] - v->left[at] + 1) / (double)v->n_values[col];
        raw[c][1] = stat[1];
        raw[c][2] = stat[0];
        raw[c][3] = stat[2];
    }
    for (uint32_t j = 0; j < np; j++) { // descending by share, strict >: rows j and best change places
        uint32_t best = j;
        for (uint32_t i = j + 1; i < np; i++)
            if (raw[i][0] > raw[best][0])
                best = i;
        if (j != best)
            for (int f = 0; f < 4; f++)
                std::swap(raw[j][f], raw[best][f]);
    }
    for (uint32_t c = 0; c < np; c++) {
        table[c * 4 + 0] = raw[c][1];
        table[c * 4 + 1] = raw[c][1] - raw[c][2];
        table[c * 4 + 2] = raw[c][3] - raw[c][1];
        table[c * 4 + 3] = raw[c][0];
    }
    *n_rows = np;
    return APEMOST_HIP_OK;
}

// ---- the reference's text dumps, formatted on the device (pt_text.h) ----
// One batch shape: its streams, the host text buffer (every line at its longest) and the device scratch
// (the regions below, each 256-byte aligned).
struct TextLayout {
    u64 kept, n_streams, n_lines, n_tiles, text_bytes;
    u64 at_slots, at_lens, at_sum, at_off, at_offsets, at_out, scratch_bytes;
};

static u64 text_align(u64 x) { return (x + 255) & ~(u64)255; }

static TextLayout text_layout(const apemost_hip_sampler *s, u64 n_steps, u64 skip, u64 thin, int n_param_chains) {
    TextLayout t;
    const u64 head = (u64)n_param_chains * s->cfg.n_par, n = (u64)s->cfg.n_chains;
    t.kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    t.n_streams = head + n;
    t.n_lines = t.kept * t.n_streams;
    t.n_tiles = (t.n_lines + kTextThreads - 1) / kTextThreads;
    t.text_bytes = t.kept * (head * kTextParamLine + n * kTextProbLine);
    u64 at = 0;
    t.at_slots = at;
    at += text_align(t.n_lines * kTextSlot);
    t.at_lens = at;
    at += text_align(t.n_lines);
    t.at_sum = at;
    at += text_align(t.n_tiles * sizeof(u64));
    t.at_off = at;
    at += text_align(t.n_tiles * sizeof(u64));
    t.at_offsets = at;
    at += text_align((t.n_streams + 1) * sizeof(u64));
    t.at_out = at;
    at += text_align(t.text_bytes);
    t.scratch_bytes = at;
    return t;
}

static int text_check(const apemost_hip_sampler *s, u64 n_steps, u64 skip, u64 thin, int32_t n_param_chains,
                      const char *what) {
    if (thin < 1 || n_param_chains < 0 || n_param_chains > s->cfg.n_chains)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: bad arguments", what);
    // at most 2^36 lines per call: every size and offset stays far inside 64 bits, the grid inside 2^31
    const u64 kept = skip < n_steps ? (n_steps - skip + thin - 1) / thin : 0;
    const u64 streams = (u64)n_param_chains * s->cfg.n_par + (u64)s->cfg.n_chains;
    if (kept > ((u64)1 << 36) / streams)
        return fail(APEMOST_HIP_ERR_INVALID, "%s: %llu kept steps of %llu lines: too many for one call", what,
                    (unsigned long long)kept, (unsigned long long)streams);
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_samples_text_bound(apemost_hip_sampler *s, uint64_t n_steps, uint64_t skip, uint64_t thin,
                                              int32_t n_param_chains, uint64_t *n_streams, uint64_t *text_bytes,
                                              uint64_t *scratch_bytes) {
    CHECK_S(s);
    const int rc = text_check(s, n_steps, skip, thin, n_param_chains, "samples_text_bound");
    if (rc != APEMOST_HIP_OK)
        return rc;
    const TextLayout t = text_layout(s, n_steps, skip, thin, n_param_chains);
    if (n_streams)
        *n_streams = t.n_streams;
    if (text_bytes)
        *text_bytes = t.text_bytes;
    if (scratch_bytes)
        *scratch_bytes = t.scratch_bytes;
    return APEMOST_HIP_OK;
}

// Queued on copy_stream behind everything launched so far on the sampler's stream, like
// apemost_hip_summary_accumulate; apemost_hip_samples_wait covers it.
extern "C" int apemost_hip_samples_text_read_async(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                                   uint64_t skip, uint64_t thin, int32_t n_param_chains,
                                                   void *d_scratch, uint64_t scratch_bytes, char *host_text,
                                                   uint64_t text_capacity, uint64_t *host_offsets, uint64_t n_offsets) {
    CHECK_S(s);
    int rc = text_check(s, n_steps, skip, thin, n_param_chains, "samples_text_read_async");
    if (rc != APEMOST_HIP_OK)
        return rc;
    const TextLayout t = text_layout(s, n_steps, skip, thin, n_param_chains);
    if (!host_offsets || n_offsets < t.n_streams + 1)
        return fail(APEMOST_HIP_ERR_INVALID, "samples_text_read_async: offsets hold %llu entries, the batch needs %llu",
                    (unsigned long long)n_offsets, (unsigned long long)(t.n_streams + 1));
    if (t.kept > 0 && (!d_samples || !d_scratch || !host_text))
        return fail(APEMOST_HIP_ERR_INVALID, "samples_text_read_async: bad arguments");
    if (t.kept > 0 && scratch_bytes < t.scratch_bytes)
        return fail(APEMOST_HIP_ERR_INVALID, "samples_text_read_async: device scratch of %llu bytes, the batch needs %llu",
                    (unsigned long long)scratch_bytes, (unsigned long long)t.scratch_bytes);
    if (t.kept > 0 && text_capacity < t.text_bytes)
        return fail(APEMOST_HIP_ERR_INVALID, "samples_text_read_async: host text buffer of %llu bytes, the batch needs %llu",
                    (unsigned long long)text_capacity, (unsigned long long)t.text_bytes);
    rc = ensure_copy_stream(s);
    if (rc != APEMOST_HIP_OK)
        return rc;
    // the error word of the launches so far rides on the sampler's stream, as for the other reads
    HIP_TRY(hipMemcpyAsync(s->h_word, s->d.timeout_word(), sizeof(u64), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(s->ev_copy, s->stream));
    HIP_TRY(hipStreamWaitEvent(s->copy_stream, s->ev_copy, 0));
    if (t.kept == 0) {
        for (u64 i = 0; i <= t.n_streams; i++)
            host_offsets[i] = 0;
        return APEMOST_HIP_OK;
    }
    char *base = (char *)d_scratch;
    TextArgs a;
    a.rows = d_samples;
    a.n_chains = s->cfg.n_chains;
    a.n_par = s->cfg.n_par;
    a.n_param_chains = n_param_chains;
    a.skip = skip;
    a.thin = thin;
    a.n_kept = t.kept;
    a.n_lines = t.n_lines;
    a.n_tiles = t.n_tiles;
    a.slots = base + t.at_slots;
    a.lens = (unsigned char *)(base + t.at_lens);
    a.tile_sum = (unsigned long long *)(base + t.at_sum);
    a.tile_off = (unsigned long long *)(base + t.at_off);
    a.offsets = (unsigned long long *)(base + t.at_offsets);
    a.out = base + t.at_out;
    hipLaunchKernelGGL(text_format_kernel, dim3((unsigned)t.n_tiles), dim3(kTextThreads), 0, s->copy_stream, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(text_scan_kernel, dim3(1), dim3(kTextScanThreads), 0, s->copy_stream, a,
                       (unsigned long long)t.n_streams);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(text_compact_kernel, dim3((unsigned)t.n_tiles), dim3(kTextThreads), 0, s->copy_stream, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(host_offsets, a.offsets, (t.n_streams + 1) * sizeof(u64), hipMemcpyDeviceToHost,
                           s->copy_stream));
    // (the whole bound: the length of the text is known on the device only)
    HIP_TRY(hipMemcpyAsync(host_text, a.out, t.text_bytes, hipMemcpyDeviceToHost, s->copy_stream));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_device_alloc(apemost_hip_sampler *s, uint64_t bytes, void **d) {
    CHECK_S(s);
    if (!d || bytes == 0)
        return fail(APEMOST_HIP_ERR_INVALID, "device_alloc: bad arguments");
    HIP_TRY(hipMalloc(d, bytes));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_device_free(apemost_hip_sampler *s, void *d) {
    CHECK_S(s);
    if (s->copy_stream)
        HIP_TRY(hipStreamSynchronize(s->copy_stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (d)
        HIP_TRY(hipFree(d));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_host_alloc(size_t bytes, void **p) {
    if (!p || bytes == 0)
        return fail(APEMOST_HIP_ERR_INVALID, "host_alloc: bad arguments");
    HIP_TRY(hipHostMalloc(p, bytes, hipHostMallocDefault));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_host_free(void *p) {
    if (p)
        HIP_TRY(hipHostFree(p));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_samples_free(apemost_hip_sampler *s, double *d_samples) {
    CHECK_S(s);
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (d_samples)
        HIP_TRY(hipFree(d_samples));
    return APEMOST_HIP_OK;
}

// host Philox4x32-10, bit-identical to the device's rocRAND stream; only used to
// tell sharded hosts which pair the next swap touches
static void philox_host(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
    uint32_t c[4] = {ctr[0], ctr[1], ctr[2], ctr[3]}, k[2] = {key[0], key[1]};
    for (int i = 0; i < 10; i++) {
        const uint64_t m0 = (uint64_t)ROCRAND_PHILOX_M4x32_0 * c[0];
        const uint64_t m1 = (uint64_t)ROCRAND_PHILOX_M4x32_1 * c[2];
        const uint32_t n0 = (uint32_t)(m1 >> 32) ^ c[1] ^ k[0], n1 = (uint32_t)m1;
        const uint32_t n2 = (uint32_t)(m0 >> 32) ^ c[3] ^ k[1], n3 = (uint32_t)m0;
        c[0] = n0, c[1] = n1, c[2] = n2, c[3] = n3;
        k[0] += ROCRAND_PHILOX_W32_0;
        k[1] += ROCRAND_PHILOX_W32_1;
    }
    memcpy(out, c, sizeof c);
}

extern "C" int64_t apemost_hip_swap_pair(uint64_t seed, uint64_t round, int64_t n_chains_global) {
    if (n_chains_global <= 1)
        return -1;
    const uint64_t sub = APEMOST_HIP_SWAP_SUBSEQUENCE;
    uint32_t ctr[4] = {(uint32_t)round, (uint32_t)(round >> 32), (uint32_t)sub, (uint32_t)(sub >> 32)};
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)}, out[4];
    philox_host(ctr, key, out);
    const double u = out[0] * (1.0 / 4294967296.0);
    const int nb = (int)n_chains_global;
    return (int)(nb * 1000 * u) % (nb - 1);
}

extern "C" int64_t apemost_hip_sampler_swap_pair(const apemost_hip_sampler *s, uint64_t round) {
    if (!s || s->cfg.n_chains_global <= 1)
        return -1;
    if (s->batch) // every ladder has a pair of its own: apemost_hip_swap_pair(seed_b, round, n_chains) answers per ladder
        return fail(APEMOST_HIP_ERR_INVALID, "sampler_swap_pair is ambiguous on a ladder batch");
    if (s->cfg.flags & APEMOST_HIP_FLAG_SWAP_EVEN_ODD) // the lowest lower chain of sweep `round`
        return (int64_t)(round % 2) <= s->cfg.n_chains_global - 2 ? (int64_t)(round % 2) : -1;
    if (!(s->cfg.flags & APEMOST_HIP_FLAG_RANDOMSWAP))
        return apemost_hip_swap_pair(s->cfg.seed, round, s->cfg.n_chains_global);
    const uint64_t sub = APEMOST_HIP_SWAP_SUBSEQUENCE;
    uint32_t ctr[4] = {(uint32_t)round, (uint32_t)(round >> 32), (uint32_t)sub, (uint32_t)(sub >> 32)};
    uint32_t key[2] = {(uint32_t)s->cfg.seed, (uint32_t)(s->cfg.seed >> 32)}, out[4];
    philox_host(ctr, key, out);
    if (!(out[0] * (1.0 / 4294967296.0) < 1.0 / 1)) // swap_probability < 1.0 / n_swap, n_swap = 1
        return -1;
    const int nb = (int)s->cfg.n_chains_global;
    return (int)(nb * 1000 * (out[1] * (1.0 / 4294967296.0))) % (nb - 1);
}

extern "C" int64_t apemost_hip_rounds_within_shard(const apemost_hip_sampler *s, uint64_t first_round,
                                                   int64_t max_rounds) {
    if (!s || max_rounds <= 0)
        return 0;
    const int64_t lo = s->cfg.chain_offset, hi = lo + s->cfg.n_chains, n = s->cfg.n_chains_global;
    if (lo == 0 && hi == n) // the whole ladder: no edge to straddle
        return max_rounds;
    int64_t k = 0;
    if (s->cfg.flags & APEMOST_HIP_FLAG_SWAP_EVEN_ODD) {
        // the edge between chains o-1 and o is straddled by the sweeps of the parity of o-1: at most two rounds
        for (; k < max_rounds; k++) {
            const int64_t par = (int64_t)((first_round + (uint64_t)k) % 2);
            if ((lo > 0 && (lo - 1) % 2 == par) || (hi < n && (hi - 1) % 2 == par))
                break;
        }
        return k;
    }
    for (; k < max_rounds; k++) {
        const int64_t a = apemost_hip_sampler_swap_pair(s, first_round + (uint64_t)k);
        if (a >= 0 && (a == lo - 1 || (a == hi - 1 && a + 1 < n)))
            break;
    }
    return k;
}

extern "C" int32_t apemost_hip_edge_doubles(int32_t n_par) { return 3 + 2 * n_par; }

extern "C" int apemost_hip_edge_export(apemost_hip_sampler *s, int side, double *d_buf) {
    CHECK_S(s);
    if (!d_buf || (side != 0 && side != 1))
        return fail(APEMOST_HIP_ERR_INVALID, "edge_export: bad arguments");
    if (s->batch)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "edge_export: ladder batches are not sharded");
    if (s->track)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "edge_export: replica flow is not tracked over a sharded ladder");
    const int row = side == 0 ? 1 : s->cfg.n_chains;
    hipLaunchKernelGGL(edge_export_kernel, dim3(1), dim3(kWave), 0, s->stream, s->d, s->cfg.n_par, s->cur, row,
                       d_buf);
    HIP_TRY(hipGetLastError());
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_edge_import(apemost_hip_sampler *s, int side, const double *d_buf) {
    CHECK_S(s);
    if (!d_buf || (side != 0 && side != 1))
        return fail(APEMOST_HIP_ERR_INVALID, "edge_import: bad arguments");
    if (s->batch)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "edge_import: ladder batches are not sharded");
    if (s->track)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "edge_import: replica flow is not tracked over a sharded ladder");
    const int row = side == 0 ? 0 : s->cfg.n_chains + 1;
    hipLaunchKernelGGL(edge_import_kernel, dim3(1), dim3(kWave), 0, s->stream, s->d, s->cfg.n_par, s->cur, row,
                       d_buf);
    HIP_TRY(hipGetLastError());
    return APEMOST_HIP_OK;
}

static int edge_buffers(apemost_hip_sampler *s) {
    if (s->edge_out[0])
        return APEMOST_HIP_OK;
    HIP_TRY(hipSetDevice(s->cfg.device));
    const size_t n = (size_t)apemost_hip_edge_doubles(s->cfg.n_par);
    int rc;
    for (int k = 0; k < 2; k++) {
        if ((rc = dev_alloc(s, &s->edge_out[k], n)) || (rc = dev_alloc(s, &s->edge_in[k], n)))
            return rc;
        HIP_TRY(hipEventCreateWithFlags(&s->ev_exported[k], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s->ev_imported[k], hipEventDisableTiming));
    }
    HIP_TRY(hipStreamSynchronize(s->stream));
    // recorded once so that the first exchange has something to wait on
    for (int k = 0; k < 2; k++) {
        HIP_TRY(hipEventRecord(s->ev_exported[k], s->stream));
        HIP_TRY(hipEventRecord(s->ev_imported[k], s->stream));
    }
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_edge_exchange(apemost_hip_sampler *lower, apemost_hip_sampler *upper) {
    if (!lower || !upper || lower == upper)
        return fail(APEMOST_HIP_ERR_INVALID, "edge_exchange: two different samplers are needed");
    if (lower->batch || upper->batch)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "edge_exchange: ladder batches are not sharded");
    if (lower->track || upper->track)
        return fail(APEMOST_HIP_ERR_UNSUPPORTED, "edge_exchange: replica flow is not tracked over a sharded ladder");
    if (lower->cfg.n_par != upper->cfg.n_par || lower->cfg.n_chains_global != upper->cfg.n_chains_global ||
        lower->cfg.seed != upper->cfg.seed ||
        lower->cfg.chain_offset + lower->cfg.n_chains != upper->cfg.chain_offset)
        return fail(APEMOST_HIP_ERR_INVALID, "edge_exchange: the shards are not neighbours of one ladder");
    int rc;
    if ((rc = edge_buffers(lower)) || (rc = edge_buffers(upper)))
        return rc;
    const size_t bytes = (size_t)apemost_hip_edge_doubles(lower->cfg.n_par) * sizeof(double);
    apemost_hip_sampler *side[2] = {lower, upper};
    // 1. each shard packs its edge chain, once its neighbour has finished reading the previous record
    // (the lower shard works with the buffers and events of its upper edge, the upper shard with those of its
    // lower edge: the two edges of an interior shard do not share any)
    for (int k = 0; k < 2; k++) {
        apemost_hip_sampler *me = side[k], *other = side[k ^ 1];
        const int mine = k == 0 ? 1 : 0, theirs = mine ^ 1;
        HIP_TRY(hipSetDevice(me->cfg.device));
        HIP_TRY(hipStreamWaitEvent(me->stream, other->ev_imported[theirs], 0));
        if ((rc = apemost_hip_edge_export(me, mine, me->edge_out[mine])))
            return rc;
        HIP_TRY(hipEventRecord(me->ev_exported[mine], me->stream));
    }
    // 2. each shard pulls the neighbour's record into its halo row
    for (int k = 0; k < 2; k++) {
        apemost_hip_sampler *me = side[k], *other = side[k ^ 1];
        const int mine = k == 0 ? 1 : 0, theirs = mine ^ 1;
        HIP_TRY(hipSetDevice(me->cfg.device));
        HIP_TRY(hipStreamWaitEvent(me->stream, other->ev_exported[theirs], 0));
        HIP_TRY(hipMemcpyPeerAsync(me->edge_in[mine], me->cfg.device, other->edge_out[theirs], other->cfg.device, bytes,
                                   me->stream));
        HIP_TRY(hipEventRecord(me->ev_imported[mine], me->stream));
        if ((rc = apemost_hip_edge_import(me, mine, me->edge_in[mine])))
            return rc;
    }
    return APEMOST_HIP_OK;
}

// the first shard pair (j, j+1), j >= from, the swap attempt `index` straddles, or -1.  The reference's schedules
// pick one pair; an even-odd sweep straddles every edge whose lower chain has the sweep's parity.
static int straddled_edge(apemost_hip_sampler **sh, int n_shards, u64 index, int from = 0) {
    if (sh[0]->cfg.flags & APEMOST_HIP_FLAG_SWAP_EVEN_ODD) {
        for (int j = from; j + 1 < n_shards; j++)
            if ((u64)(sh[j]->cfg.chain_offset + sh[j]->cfg.n_chains - 1) % 2 == index % 2)
                return j;
        return -1;
    }
    const int64_t a = apemost_hip_sampler_swap_pair(sh[0], index);
    for (int j = from; a >= 0 && j + 1 < n_shards; j++)
        if (a == sh[j]->cfg.chain_offset + sh[j]->cfg.n_chains - 1)
            return j;
    return -1;
}

extern "C" int apemost_hip_run_shards(apemost_hip_sampler **sh, int32_t n_shards, uint64_t n_rounds, uint32_t n_swap,
                                      double **d_samples) {
    if (!sh || n_shards < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "run_shards: no shards");
    for (int j = 0; j < n_shards; j++)
        if (sh[j] && sh[j]->batch)
            return fail(APEMOST_HIP_ERR_UNSUPPORTED, "run_shards: shard %d is a ladder batch; batches are not sharded", j);
    for (int j = 0; j < n_shards; j++)
        if (sh[j] && sh[j]->track)
            return fail(APEMOST_HIP_ERR_UNSUPPORTED, "run_shards: shard %d tracks replica flow, which is not sharded", j);
    int64_t next = 0;
    for (int j = 0; j < n_shards; j++) {
        if (!sh[j] || sh[j]->cfg.chain_offset != next || sh[j]->cfg.n_chains_global != sh[0]->cfg.n_chains_global ||
            sh[j]->cfg.seed != sh[0]->cfg.seed || sh[j]->round != sh[0]->round ||
            sh[j]->swap_pending != sh[0]->swap_pending ||
            ((sh[j]->cfg.flags ^ sh[0]->cfg.flags) & (APEMOST_HIP_FLAG_SWAP_EVEN_ODD | APEMOST_HIP_FLAG_RANDOMSWAP)))
            return fail(APEMOST_HIP_ERR_INVALID, "run_shards: shard %d does not continue the ladder (offset, seed, "
                                                 "ladder size, swap schedule and swap position must agree)", j);
        next += sh[j]->cfg.n_chains;
    }
    if (next != sh[0]->cfg.n_chains_global)
        return fail(APEMOST_HIP_ERR_INVALID, "run_shards: the shards cover %lld of %lld chains", (long long)next,
                    (long long)sh[0]->cfg.n_chains_global);
    // Shards that share a device launch their grids side by side on separate streams: the residency
    // every multi-round launch relies on (a workgroup may wait for its swap partner inside the launch)
    // was established for one grid alone on the device, so such shards hold one round per launch.
    bool device_shared = false;
    for (int j = 0; j < n_shards; j++)
        for (int i = 0; i < j; i++)
            device_shared = device_shared || sh[i]->cfg.device == sh[j]->cfg.device;
    int rc;
    for (uint64_t r = 0; r < n_rounds || (r == n_rounds && sh[0]->swap_pending);) {
        const bool finalise = r == n_rounds; // the swap attempt that closes the last round
        const int pending = sh[0]->swap_pending;
        const u64 first_inside = sh[0]->round + (pending ? 1 : 0);
        uint64_t limit = finalise || n_swap == 0 || device_shared ? 1 : n_rounds - r;
        for (int j = 0; j < n_shards; j++)
            if ((uint64_t)max_rounds_per_launch(sh[j]) < limit)
                limit = (uint64_t)max_rounds_per_launch(sh[j]);
        uint64_t k = 1;
        while (k < limit && straddled_edge(sh, n_shards, first_inside + k - 1) < 0)
            k++;
        if (pending) // (an even-odd sweep: each straddled edge; an interior shard can have both of its edges in it)
            for (int j = straddled_edge(sh, n_shards, sh[0]->round); j >= 0; j = straddled_edge(sh, n_shards, sh[0]->round, j + 1))
                if ((rc = apemost_hip_edge_exchange(sh[j], sh[j + 1])))
                    return rc;
        for (int j = 0; j < n_shards; j++) {
            const size_t row = (size_t)sh[j]->cfg.n_chains * (sh[j]->cfg.n_par + 2);
            double *out = (d_samples && d_samples[j] && !finalise) ? d_samples[j] + r * n_swap * row : nullptr;
            if ((rc = launch_round_impl(sh[j], (uint32_t)k, finalise ? 0 : n_swap, pending, -1, out)))
                return rc;
        }
        if (finalise)
            break;
        r += k;
    }
    return APEMOST_HIP_OK;
}

extern "C" void apemost_hip_calib_defaults(apemost_hip_calib_config *c) {
    if (!c)
        return;
    c->burn_in_iterations = 10000;
    c->iter_limit = 100000;
    c->iter_readjust = 200;
    c->no_rescaling_limit = 15;
    c->rat_limit = 0.5;
    c->target_global = 0.5;
    c->max_ar_deviation = 0.01;
    c->mul = 0.85;
    c->adjust_step = 0.5;
    c->progress_chain = -1;
    c->reserved = 0;
}

// ---- markov_chain_calibrate on the device, in segments -------------------------------------
// workgroup shape of a segment: what the sampler itself would choose for a ladder of as many chains
// as are still calibrating (a forced waves_per_chain stays forced)
struct CalibShape {
    int waves;
    bool lds_data, one_barrier, helper;
    u64 budget;
};

static CalibShape calib_shape(const apemost_hip_sampler *s, int n_active) {
    CalibShape g;
    apemost_hip_config c = s->cfg;
    c.n_chains = n_active;
    g.waves = choose_waves(c);
    if (!s->user.module && !built(s->kmodel, g.waves))
        g.waves = s->waves; // (development builds hold only some shapes)
    g.one_barrier = has_one_barrier(g.waves) && s->kmodel < kVariantModel && !(s->cfg.flags & APEMOST_HIP_FLAG_TWO_BARRIER_STEP) &&
                    user_may_ob(s);
    g.helper = g.one_barrier && ob_wants_helper(s, n_active) && s->betas_split_ok;
    const size_t bytes = g.one_barrier ? ob_lds_bytes(s, true) : classic_lds_bytes(s, g.waves, true);
    g.lds_data = !s->user.module && bytes <= 160 * 1024 - 1024 && c.lds_policy != 2 && (c.lds_policy == 1 || choose_lds(c, bytes));
    // A segment of about a quarter of a second: likelihood evaluations a chain gets through in that
    // time, from a coarse model of one evaluation (1.7 ns per data point and wavefront, 0.7 us at
    // least, stretched when the wavefronts outnumber the SIMDs).  Always whole blocks, at least one.
    const double waves_per_wg = g.one_barrier ? g.waves + 4 + (g.helper ? 1 : 0) : g.waves;
    double t_eval = 1.7e-9 * s->cfg.n_data / g.waves;
    if (t_eval < 0.7e-6)
        t_eval = 0.7e-6;
    const double crowd = n_active * waves_per_wg / 1024.0;
    if (crowd > 1)
        t_eval *= crowd;
    g.budget = (u64)(0.25 / t_eval);
    if (g.budget < 1)
        g.budget = 1;
    // (tests cut the calibration into many more segments: APEMOST_CALIB_SEGMENT_EVALS=1 ends every
    // launch after one block)
    if (const char *env = getenv("APEMOST_CALIB_SEGMENT_EVALS")) {
        const long long v = atoll(env);
        if (v > 0)
            g.budget = (u64)v;
    }
    return g;
}

static int calib_launch_segment(apemost_hip_sampler *s) {
    auto &k = s->cal;
    const CalibShape g = calib_shape(s, k.n_active);
    int rc = enable_big_lds(s, g.waves);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(k.d_list, k.h_list, (size_t)k.n_active * sizeof(int), hipMemcpyHostToDevice, s->stream));
    CalibArgs a;
    a.d = s->d;
    a.sh = s->sh;
    a.cur = s->cur;
    a.first = k.first;
    a.burn_in_only = k.burn_in_only;
    a.progress_slot = k.progress_slot;
    a.cfg = k.cfg;
    a.list = k.d_list;
    a.rec = k.d_rec;
    a.orig_step = k.d_orig;
    a.progress = k.d_progress;
    a.progress_cap = k.progress_cap;
    a.budget = g.budget;
    rc = launch_shape(s, g.one_barrier ? K_CALIB_OB : K_CALIB, k.n_active, &a, g.waves, g.lds_data, false, g.helper);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(k.h_rec, k.d_rec, (size_t)k.count * sizeof(CalibRec), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipEventRecord(k.ev, s->stream));
    k.in_flight = true;
    k.segments++;
    k.launches_by_waves[g.waves]++;
    k.segment_start = std::chrono::steady_clock::now();
    k.segment_waves = g.waves;
    return APEMOST_HIP_OK;
}

// the records of the segment that has just ended: who is still calibrating
static void calib_collect(apemost_hip_sampler *s) {
    auto &k = s->cal;
    int n = 0;
    for (int i = 0; i < k.n_active; i++) {
        const int slot = k.h_list[i];
        if (k.h_rec[slot].stage != CAL_DONE)
            k.h_list[n++] = slot;
    }
    k.n_active = n;
    k.in_flight = false;
    k.seconds_by_waves[k.segment_waves] +=
        std::chrono::duration<double>(std::chrono::steady_clock::now() - k.segment_start).count();
}

extern "C" int apemost_hip_calibrate_begin(apemost_hip_sampler *s, int32_t first, int32_t count,
                                           const apemost_hip_calib_config *c, int burn_in_only) {
    CHECK_S(s);
    if (!c || first < 0 || count < 1 || first + count > s->cfg.n_chains)
        return fail(APEMOST_HIP_ERR_INVALID, "calibrate_chains: chains [%d,%d) outside [0,%d)", first,
                    first + count, s->cfg.n_chains);
    if (c->iter_readjust == 0)
        return fail(APEMOST_HIP_ERR_INVALID, "iter_readjust must be > 0");
    if (c->progress_chain >= 0 && (c->progress_chain < first || c->progress_chain >= first + count))
        return fail(APEMOST_HIP_ERR_INVALID, "progress_chain %d outside the chains [%d,%d) of this calibration",
                    c->progress_chain, first, first + count);
    auto &k = s->cal;
    if (k.open)
        return fail(APEMOST_HIP_ERR_INVALID, "calibrate_begin: the previous calibration was not collected (calibrate_end)");
    const int cap = (int)(c->iter_limit / c->iter_readjust) + 2; // readjustments a chain can reach
    if (count > k.capacity || cap > k.progress_cap) {
        if (k.d_rec)
            hipFree(k.d_rec);
        if (k.d_orig)
            hipFree(k.d_orig);
        if (k.d_list)
            hipFree(k.d_list);
        if (k.d_progress)
            hipFree(k.d_progress);
        if (k.h_rec)
            hipHostFree(k.h_rec);
        if (k.h_list)
            hipHostFree(k.h_list);
        k.d_rec = nullptr, k.d_orig = nullptr, k.d_list = nullptr, k.d_progress = nullptr, k.h_rec = nullptr, k.h_list = nullptr;
        k.capacity = k.progress_cap = 0;
        const int want = count > k.capacity ? count : k.capacity, pcap = cap > k.progress_cap ? cap : k.progress_cap;
        HIP_TRY(hipMalloc((void **)&k.d_rec, (size_t)want * sizeof(CalibRec)));
        HIP_TRY(hipMalloc((void **)&k.d_orig, (size_t)want * s->cfg.n_par * sizeof(double)));
        HIP_TRY(hipMalloc((void **)&k.d_list, (size_t)want * sizeof(int)));
        HIP_TRY(hipMalloc((void **)&k.d_progress, (size_t)pcap * (1 + 2 * s->cfg.n_par) * sizeof(double)));
        HIP_TRY(hipHostMalloc((void **)&k.h_rec, (size_t)want * sizeof(CalibRec), hipHostMallocDefault));
        HIP_TRY(hipHostMalloc((void **)&k.h_list, (size_t)want * sizeof(int), hipHostMallocDefault));
        k.capacity = want;
        k.progress_cap = pcap;
    }
    if (!k.ev)
        HIP_TRY(hipEventCreateWithFlags(&k.ev, hipEventDisableTiming));
    k.first = first;
    k.count = count;
    k.burn_in_only = burn_in_only ? 1 : 0;
    k.cfg = *c;
    k.progress_slot = c->progress_chain >= 0 ? c->progress_chain - first : -1;
    k.cancelled = false;
    k.segments = 0;
    memset(k.launches_by_waves, 0, sizeof k.launches_by_waves);
    for (double &t : k.seconds_by_waves)
        t = 0;
    HIP_TRY(hipMemsetAsync(k.d_rec, 0, (size_t)count * sizeof(CalibRec), s->stream)); // stage = CAL_INIT
    HIP_TRY(hipMemsetAsync(k.d_orig, 0, (size_t)count * s->cfg.n_par * sizeof(double), s->stream));
    for (int i = 0; i < count; i++)
        k.h_list[i] = i;
    k.n_active = count;
    const int rc = calib_launch_segment(s);
    if (rc)
        return rc;
    k.open = true;
    return APEMOST_HIP_OK;
}

// One turn of the segment loop without blocking: if the segment in flight has ended, its records are
// collected and the chains that are not done yet are launched again.  *active = chains still
// calibrating (0: calibrate_end will not wait).
extern "C" int apemost_hip_calibrate_poll(apemost_hip_sampler *s, int32_t *active) {
    CHECK_S(s);
    auto &k = s->cal;
    if (!k.open)
        return fail(APEMOST_HIP_ERR_INVALID, "calibrate_poll without calibrate_begin");
    if (k.in_flight) {
        const hipError_t q = hipEventQuery(k.ev);
        if (q == hipErrorNotReady) {
            if (active)
                *active = k.n_active;
            return APEMOST_HIP_OK;
        }
        HIP_TRY(q);
        calib_collect(s);
        if (k.n_active > 0 && !k.cancelled) {
            const int rc = calib_launch_segment(s);
            if (rc)
                return rc;
        }
    }
    if (active)
        *active = k.in_flight ? k.n_active : 0;
    return APEMOST_HIP_OK;
}

// for hosts that calibrate on several devices from one thread: returns when a segment of one of the
// samplers has ended (and its successor has been launched), or when none of them has chains left
extern "C" int apemost_hip_calibrate_wait_any(apemost_hip_sampler **ss, int32_t n, int32_t *active_total) {
    if (!ss || n < 1)
        return fail(APEMOST_HIP_ERR_INVALID, "calibrate_wait_any: no samplers");
    for (;;) {
        int total = 0;
        bool advanced = false;
        for (int i = 0; i < n; i++) {
            if (!ss[i] || !ss[i]->cal.open)
                continue;
            const u64 before = ss[i]->cal.segments;
            const bool was_busy = ss[i]->cal.in_flight;
            int32_t active = 0;
            const int rc = apemost_hip_calibrate_poll(ss[i], &active);
            if (rc)
                return rc;
            total += active;
            advanced = advanced || ss[i]->cal.segments != before || (was_busy && !ss[i]->cal.in_flight);
        }
        if (advanced || total == 0) {
            if (active_total)
                *active_total = total;
            return APEMOST_HIP_OK;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(50));
    }
}

// stop after the segment in flight: calibrate_end then returns the chains as they are (status -1 for
// those that were not done)
extern "C" int apemost_hip_calibrate_cancel(apemost_hip_sampler *s) {
    CHECK_S(s);
    if (!s->cal.open)
        return fail(APEMOST_HIP_ERR_INVALID, "calibrate_cancel without calibrate_begin");
    s->cal.cancelled = true;
    return APEMOST_HIP_OK;
}

// ... and its results: status[count] / iters[count] of the chains of the matching begin
extern "C" int apemost_hip_calibrate_end(apemost_hip_sampler *s, int32_t *status, uint64_t *iters) {
    CHECK_S(s);
    auto &k = s->cal;
    if (!k.open)
        return fail(APEMOST_HIP_ERR_INVALID, "calibrate_end without calibrate_begin");
    int rc = APEMOST_HIP_OK;
    while (k.in_flight && !rc) {
        const hipError_t w = hipEventSynchronize(k.ev);
        if (w != hipSuccess)
            rc = fail(APEMOST_HIP_ERR_RUNTIME, "hipEventSynchronize failed: %s", hipGetErrorString(w));
        else
            rc = apemost_hip_calibrate_poll(s, nullptr);
    }
    k.open = false;
    k.in_flight = false;
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    rc = check_handoff(s);
    if (rc)
        return rc;
    int worst = 0;
    for (int i = 0; i < k.count; i++) {
        const CalibRec &r = k.h_rec[i];
        const int st = r.stage == CAL_DONE ? r.status : -1;
        if (status)
            status[i] = st;
        if (iters)
            iters[i] = r.sweeps;
        if (st && !worst)
            worst = st;
    }
    if (worst)
        return fail(APEMOST_HIP_ERR_CALIBRATION, "calibration %s",
                    worst == 1 ? "failed: a step width became too large"
                               : worst == 2 ? "failed: iteration limit reached" : "cancelled");
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_calibrate_chains(apemost_hip_sampler *s, int32_t first, int32_t count,
                                            const apemost_hip_calib_config *c, int burn_in_only,
                                            int32_t *status, uint64_t *iters) {
    const int rc = apemost_hip_calibrate_begin(s, first, count, c, burn_in_only);
    return rc ? rc : apemost_hip_calibrate_end(s, status, iters);
}

extern "C" int apemost_hip_calibrate_progress(apemost_hip_sampler *s, double *rows, int32_t capacity_rows,
                                              int32_t *n_rows) {
    CHECK_S(s);
    auto &k = s->cal;
    if (k.open || !n_rows || capacity_rows < 0 || (capacity_rows > 0 && !rows))
        return fail(APEMOST_HIP_ERR_INVALID, "calibrate_progress: bad arguments, or a calibration is still open");
    *n_rows = 0;
    if (k.progress_slot < 0 || !k.h_rec || k.progress_slot >= k.count)
        return APEMOST_HIP_OK;
    long long n = (long long)(k.h_rec[k.progress_slot].sweeps / k.cfg.iter_readjust);
    const CalibRec &r = k.h_rec[k.progress_slot];
    if (r.stage == CAL_ALL) // the sweeps of the last readjustment were not followed by their steps
        n -= 1;
    if (r.stage == CAL_DONE && r.status == 1)
        n -= 1;
    if (n > k.progress_cap)
        n = k.progress_cap;
    if (n < 0)
        n = 0;
    *n_rows = (int32_t)n;
    const long long take = n < capacity_rows ? n : capacity_rows;
    if (take > 0)
        HIP_TRY(hipMemcpy(rows, k.d_progress, (size_t)take * (1 + 2 * s->cfg.n_par) * sizeof(double), hipMemcpyDeviceToHost));
    return APEMOST_HIP_OK;
}

// segments and launches per workgroup shape of the latest calibration (bench, tests)
extern "C" int apemost_hip_calibrate_stats(apemost_hip_sampler *s, uint64_t *segments, uint64_t *evaluations,
                                           uint64_t launches_by_waves[9], double seconds_by_waves[9]) {
    CHECK_S(s);
    auto &k = s->cal;
    if (segments)
        *segments = k.segments;
    if (evaluations) {
        u64 sum = 0;
        for (int i = 0; k.h_rec && i < k.count; i++)
            sum += k.h_rec[i].evals;
        *evaluations = sum;
    }
    if (launches_by_waves)
        memcpy(launches_by_waves, k.launches_by_waves, sizeof k.launches_by_waves);
    if (seconds_by_waves)
        memcpy(seconds_by_waves, k.seconds_by_waves, sizeof k.seconds_by_waves);
    return APEMOST_HIP_OK;
}

static int rng_device(int device) {
    int rc = apemost_hip_device_info(device, nullptr, 0, nullptr, nullptr);
    if (rc)
        return rc;
    HIP_TRY(hipSetDevice(device));
    return APEMOST_HIP_OK;
}

// device scratch of the two test hooks, released on every path
struct DeviceScratch {
    std::vector<void *> blocks;
    ~DeviceScratch() {
        for (void *p : blocks)
            hipFree(p);
    }
    template <class T>
    hipError_t get(T **p, size_t count) {
        void *q = nullptr;
        const hipError_t e = hipMalloc(&q, count * sizeof(T));
        if (e == hipSuccess)
            blocks.push_back(q);
        *p = (T *)q;
        return e;
    }
};

extern "C" int apemost_hip_rng_raw(int device, uint64_t seed, uint64_t subsequence, uint64_t offset,
                                   int32_t n, uint32_t *out) {
    int rc = rng_device(device);
    if (rc)
        return rc;
    if (n < 1 || !out)
        return fail(APEMOST_HIP_ERR_INVALID, "rng_raw: bad arguments");
    DeviceScratch mem;
    unsigned int *d;
    HIP_TRY(mem.get(&d, n));
    hipLaunchKernelGGL(rng_raw_kernel, dim3(1), dim3(kWave), 0, 0, seed, subsequence, offset, n, d);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(out, d, n * sizeof(unsigned int), hipMemcpyDeviceToHost));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_rng_attempts(int device, uint64_t seed, uint64_t chain, int32_t slot, uint64_t tick,
                                        uint64_t q0, int32_t n, double *y, double *s, int32_t *valid,
                                        double *accept_log_u) {
    int rc = rng_device(device);
    if (rc)
        return rc;
    if (n < 1 || !y || !s || !valid)
        return fail(APEMOST_HIP_ERR_INVALID, "rng_attempts: bad arguments");
    DeviceScratch mem;
    double *dy, *ds, *dl;
    int *dv;
    HIP_TRY(mem.get(&dy, n));
    HIP_TRY(mem.get(&ds, n));
    HIP_TRY(mem.get(&dl, 1));
    HIP_TRY(mem.get(&dv, n));
    hipLaunchKernelGGL(rng_attempts_kernel, dim3((n + 63) / 64), dim3(kWave), 0, 0, seed, chain, slot, tick, q0, n,
                       dy, ds, dv, dl);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(y, dy, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(s, ds, n * sizeof(double), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(valid, dv, n * sizeof(int), hipMemcpyDeviceToHost));
    if (accept_log_u)
        HIP_TRY(hipMemcpy(accept_log_u, dl, sizeof(double), hipMemcpyDeviceToHost));
    return APEMOST_HIP_OK;
}

#ifdef APEMOST_STAMPS
// diagnostic build only: read and clear the per-segment cycle sums of workgroup 0
extern "C" int apemost_hip_debug_stamps(unsigned long long *out16) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), 16 * sizeof(unsigned long long)));
    unsigned long long zero[16] = {0};
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), zero, sizeof zero));
    return APEMOST_HIP_OK;
}
// steps x 16 waves x points s_memtime values of workgroup 0 (zero = stamp not reached)
extern "C" int apemost_hip_debug_timeline(unsigned long long *out, int *steps, int *points) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(g_timeline), sizeof(unsigned long long) * kTimelineSteps * 16 * kTimelinePoints));
    *steps = kTimelineSteps;
    *points = kTimelinePoints;
    return APEMOST_HIP_OK;
}
#endif

extern "C" int apemost_hip_timer_begin(apemost_hip_sampler *s) {
    CHECK_S(s);
    s->launches_at_begin = s->launches;
    HIP_TRY(hipEventRecord(s->ev0, s->stream));
    return APEMOST_HIP_OK;
}

extern "C" int apemost_hip_timer_end(apemost_hip_sampler *s, float *elapsed_ms, uint64_t *launches) {
    CHECK_S(s);
    HIP_TRY(hipEventRecord(s->ev1, s->stream));
    HIP_TRY(hipEventSynchronize(s->ev1));
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    if (elapsed_ms)
        *elapsed_ms = ms;
    if (launches)
        *launches = s->launches - s->launches_at_begin;
    return APEMOST_HIP_OK;
}

// A build from this file alone (development and diagnostic builds: apemost_amd/build.py build_dev,
// build_stamps) holds every model's kernels itself.
#ifdef APEMOST_SINGLE_TU
namespace apemost {
template hipError_t model_dispatch<0>(int, const AnyOp &);
template hipError_t model_dispatch<1>(int, const AnyOp &);
template hipError_t model_dispatch<2>(int, const AnyOp &);
template hipError_t model_dispatch<3>(int, const AnyOp &);
template hipError_t model_dispatch<8>(int, const AnyOp &);
template hipError_t model_dispatch<9>(int, const AnyOp &);
template hipError_t model_dispatch<10>(int, const AnyOp &);
template hipError_t model_dispatch<11>(int, const AnyOp &);
} // namespace apemost
#endif
