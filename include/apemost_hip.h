/*
 * apemost_hip.h -- C ABI of the MI355X (gfx950) parallel-tempering engine.
 *
 * This is the drop-in boundary for APEMoST's hot path: the body of
 * run_sampler() (src/parallel_tempering.c:347-419), i.e. per chain
 * markov_chain_step() (src/markov_chain.c:369-386) + mcmc_check_best()
 * (src/mcmc_calculate.c:35-41) + sample output, then tempering_interaction()
 * (src/parallel_tempering_interaction.c:125-141); and the calibration phases
 * built from the same step (src/markov_chain.c:34-79,
 * src/markov_chain_calibrate.c:1039-1204, src/parallel_tempering.c:78-207).
 *
 * Plain C: pointers, sizes, integers.  No torch / C++ types.  A reference
 * maintainer binds it directly from C (INTEGRATION.md shows the patch to
 * src/parallel_tempering.c); the Python host mirror binds it with ctypes.
 *
 * All chain state crosses the boundary as structure-of-arrays blocks
 * (apemost_hip_state_view) -- the flattened form of the reference's `mcmc`
 * struct (src/mcmc_struct.h:30-106) plus `parallel_tempering_mcmc`
 * (src/parallel_tempering_beta.h:65-76).
 *
 * Every function returns APEMOST_HIP_OK (0) or a negative error code;
 * apemost_hip_last_error() gives the message.  There is no CPU fallback: with
 * no usable HIP device every compute entry point fails with
 * APEMOST_HIP_ERR_NO_DEVICE.
 */
#ifndef APEMOST_HIP_H
#define APEMOST_HIP_H

#if !defined(__HIPCC_RTC__)
#include <stddef.h>
#include <stdint.h>
#else /* compiled by hiprtc (a user-supplied device model): no C library headers, its own fixed-width types */
using __hip_internal::int32_t;
using __hip_internal::int64_t;
using __hip_internal::uint32_t;
using __hip_internal::uint64_t;
using __hip_internal::uint8_t;
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define APEMOST_HIP_ABI_VERSION 3

enum {
    APEMOST_HIP_OK = 0,
    APEMOST_HIP_ERR_INVALID = -1,   /* bad argument / shape mismatch */
    APEMOST_HIP_ERR_NO_DEVICE = -2, /* no HIP device, or not gfx950 */
    APEMOST_HIP_ERR_RUNTIME = -3,   /* a HIP call failed */
    APEMOST_HIP_ERR_UNSUPPORTED = -4,
    APEMOST_HIP_ERR_CALIBRATION = -5 /* calibration failed (reference: exit(1)) */
};

/* device-side likelihoods = re-implementations of the user plugins calc_model()
 * (src/mcmc.h:164) of the BASELINE apps */
enum {
    APEMOST_MODEL_SIMPLESIN = 0,  /* apps/simplesin.c:12-38   n_par = 4            */
    APEMOST_MODEL_PULSE = 1,      /* apps/pulse.c:12-54       n_par = 2 + 2*modes  */
    APEMOST_MODEL_PULSE_VROT = 2, /* apps/pulse_vrot.c:12-65  n_par = 7            */
    APEMOST_MODEL_SINE3 = 3,      /* 10-parameter 3-sinusoid model  */
    /* any other calc_model(): device source supplied by the user (apemost_device_model.h), named in
     * apemost_hip_config.device_model_source and compiled with hiprtc when the sampler is created;
     * any n_par; runs in the one-wave kernels */
    APEMOST_MODEL_USER = 4
};

/* BETA_ALIGNMENT choices, src/parallel_tempering_beta.c:53-83 */
enum {
    APEMOST_LADDER_CHEBYSHEV_BETA = 0,
    APEMOST_LADDER_EQUIDISTANT_BETA = 1,
    APEMOST_LADDER_EQUIDISTANT_TEMPERATURE = 2,
    APEMOST_LADDER_CHEBYSHEV_TEMPERATURE = 3,
    APEMOST_LADDER_EQUIDISTANT_STEPWIDTH = 4,
    APEMOST_LADDER_CHEBYSHEV_STEPWIDTH = 5,
    APEMOST_LADDER_HOT_CHAINS = 6
};

#define APEMOST_HIP_MAX_PAR 62            /* n_par + 2 lanes of one wavefront */
/* RNG addressing (rocRAND Philox4x32-10): stream (chain, slot) = subsequence chain*256+slot;
 * attempt q of parameter p's proposal at tick t = block (t<<24)|q of slot p, words 0,1;
 * accept uniform of tick t = word 0 of block t<<24 of slot n_par; swap attempt number r =
 * block r of the swap subsequence (word 0 pair choice, word 1 accept; with
 * APEMOST_HIP_FLAG_RANDOMSWAP words 1 and 2, word 0 being the swap_probability draw; with
 * APEMOST_HIP_FLAG_SWAP_EVEN_ODD pair a of sweep r reads word 0 of block r of subsequence
 * APEMOST_HIP_SWAP_SUBSEQUENCE + 1 + a).
 * Non-Gaussian proposals read word 0 of the attempt's block. */
#define APEMOST_HIP_STREAMS_PER_CHAIN 256
#define APEMOST_HIP_TICK_SHIFT 24
#define APEMOST_HIP_SWAP_SUBSEQUENCE 0x8000000000000000ULL

typedef struct apemost_hip_sampler apemost_hip_sampler;

/* apemost_hip_config.flags */
enum {
    /* one round per launch: every swap attempt is the fused swap-in at the start of the next
     * launch; no workgroup ever waits for another one (the fallback the engine also takes by
     * itself when the grid cannot be co-resident, or after a failed in-launch hand-off) */
    APEMOST_HIP_FLAG_SINGLE_ROUND_LAUNCHES = 1,
    /* multi-round launches go through hipLaunchCooperativeKernel: the runtime guarantees (or
     * refuses) co-residency of the whole grid instead of the engine's occupancy estimate.  The
     * engine does so by itself where the grid fits the occupancy figure but not its estimate; a
     * refused launch is re-issued one round at a time, as are all later ones */
    APEMOST_HIP_FLAG_COOPERATIVE_LAUNCH = 2,
    /* stepping launches of workgroups with 8 likelihood waves use the classic two-phase step
     * (two barriers, the chain's wave alone between them) instead of the one-barrier kernel; same
     * chain either way (A/B comparisons, fallback) */
    APEMOST_HIP_FLAG_TWO_BARRIER_STEP = 4,
    /* the reference's compile-time variants (defaults: Gaussian proposal, decide_swap_now, no
     * adaptation).  At most one of the two proposal bits.  The proposal and swap variants run in
     * kernel instantiations of their own (the default kernels carry no test for them), built for
     * 1, 2, 4 and 8 waves per chain. */
    /* -DPROPOSAL_LOGISTIC: get_next_random_jump = gsl_ran_logistic(r, step),
     * src/mcmc_gettersetter.c:291-292 (uniform of word 0 of the attempt's block) */
    APEMOST_HIP_FLAG_PROPOSAL_LOGISTIC = 8,
    /* -DPROPOSAL_UNIFORM: gsl_ran_flat(r, -step, step), src/mcmc_gettersetter.c:293-294 */
    APEMOST_HIP_FLAG_PROPOSAL_UNIFORM = 16,
    /* -DRANDOMSWAP: tempering_interaction() goes through
     * parallel_tempering_decide_swap_random(chains, n_beta, 1)
     * (src/parallel_tempering_interaction.c:47-64, 130-131): one more uniform ahead of the pair
     * choice -- swap attempt r reads words 0 (swap_probability), 1 (pair), 2 (accept) of block r */
    APEMOST_HIP_FLAG_RANDOMSWAP = 32,
    /* -DADAPT: adapt() after the steps of every round of a stepping launch
     * (src/parallel_tempering.c:282-301, 404) nudges the chain's step widths by 0.99 or 1/0.99
     * towards apemost_hip_config.adapt_target */
    APEMOST_HIP_FLAG_ADAPT = 64,
    /* test hook: every cooperative launch is treated as refused by the runtime, so that the path a
     * real refusal takes (the launch re-issued round by round, single-round launches from then on)
     * can be exercised on a machine where the runtime never refuses */
    APEMOST_HIP_FLAG_TEST_REFUSE_COOPERATIVE = 128,
    /* test hook for the other designed failure: inside a multi-round launch the lower chain of the
     * pair of swap attempt 3 does not publish its record, and every bounded wait of the launch gives
     * up after a few thousand polls instead of eight million -- the partner's wait runs out, the
     * launch's error word is raised, apemost_hip_synchronize reports it, and the sampler issues one
     * round per launch from then on */
    APEMOST_HIP_FLAG_TEST_WITHHOLD_PUBLISH = 256,
    /* -DRWM: adapt()'s other block (src/parallel_tempering.c:268-281; it does not compile in the reference:
     * `markov_chain_step(chains[i], 0)` passes two arguments to a function of one).  As restated here: after
     * the steps of every round and before its swap attempt every chain keeps its log-posterior, takes ONE
     * more markov_chain_step -- accept / reject counters and the RNG tick move, but no mcmc_check follows it:
     * no sample row, n_iter and the best point stay what the round's own steps left -- and
     * rmw_adapt_stepwidth (src/markov_chain.c:342-367) moves every step width by
     * U / sqrt(n_iter) * (min(1, exp(prob - prob_old)) - adapt_target) * (max - min), clamped to
     * [1e-7, 1e6] * (max - min); U = word p % 4 of block (tick << 24) | (1 + p / 4) of the accept slot.
     * Every round is a launch of its own (as with APEMOST_HIP_FLAG_ADAPT, which runs after it). */
    APEMOST_HIP_FLAG_RWM = 512,
    /* APEMOST_MODEL_USER only (APEMOST_HIP_ERR_INVALID with a built-in model): the user's likelihood also runs in
     * the one-barrier round and calibration kernels, wherever a built-in model would take them (4 or 8 likelihood
     * waves per chain; APEMOST_HIP_FLAG_TWO_BARRIER_STEP still wins; the calibration of the default proposal law and
     * swap schedule only; launch_round_for stays two-phase).  No helper wavefront, no cooperative launches.  Every
     * likelihood wave and the chain's wave call apemost_user_finish() and apply the reference's check_accept to its
     * result: the same decisions, bit for bit, as the two-phase kernels, if finish() keeps the contract stated in
     * include/apemost_device_model.h.  hiprtc compiles four more kernels at create time. */
    APEMOST_HIP_FLAG_USER_ONE_BARRIER = 1024,
    /* Even-odd swap sweeps (deterministic even-odd, Okabe 2001 / Syed 2019), not in the reference:
     * "swap attempt r" -- swap-stream position r, what apemost_hip_set_round / get_round count -- is SWEEP r: every
     * pair (a, a+1) of the GLOBAL ladder with a % 2 == r % 2, 0 <= a <= n_chains_global - 2, is attempted.  The
     * pairs of a sweep are disjoint, so their order does not matter; a chain without a partner in sweep r sits it
     * out (chain 0 in odd sweeps, the top chain where the parity leaves it alone).
     * Each pair is decided and applied by the reference's own primitives, unchanged: check_swap_probability
     * (r = beta_a p_b / beta_b + beta_b p_a / beta_a - (p_a + p_b), swap iff r > ln U, ln 0 = -inf) and
     * parallel_tempering_do_swap with its quirks (prob is not exchanged; the larger prob_best and its point are
     * copied over; swapcount of the lower chain counts), src/parallel_tempering_interaction.c:25-42, 99-123.
     * Only the schedule is new.
     * RNG: the uniform U of pair a in sweep r is word 0 of Philox block r of subsequence
     * APEMOST_HIP_SWAP_SUBSEQUENCE + 1 + a (a = global index of the lower chain).  Chain streams use subsequences
     * below 2^63 and the reference schedules' swap stream is 2^63 itself: nothing collides.  Both chains of a pair,
     * every shard and every rank derive the same word; results do not depend on launch boundaries, waves per chain
     * or the number of shards.
     * Limits: excludes APEMOST_HIP_FLAG_RANDOMSWAP and APEMOST_HIP_FLAG_TEST_WITHHOLD_PUBLISH
     * (APEMOST_HIP_ERR_INVALID); combines with the proposal-law bits, with ADAPT and RWM (every round is then a
     * launch of its own) and with a user-supplied model (hiprtc compiles the variant kernels).  Runs in the variant
     * kernel instantiations, like RANDOMSWAP: 1, 2, 4 or 8 waves per chain.  The calibration has no swaps: its
     * results are the same with and without the flag.  apemost_hip_sampler_swap_pair gives the lowest lower chain
     * of sweep r (r % 2, or -1 when that is not a pair of the ladder); on a sharded ladder an edge between chains
     * o-1 and o is straddled by the sweeps with r % 2 == (o-1) % 2, so apemost_hip_rounds_within_shard gives at
     * most two rounds, and apemost_hip_run_shards exchanges on every straddled edge before such a launch.  The
     * torch.distributed driver (distributed.ShardedLadder) does not run this schedule. */
    APEMOST_HIP_FLAG_SWAP_EVEN_ODD = 2048,
    /* Replica-flow tracking, not in the reference: follows which replica sits at which rung through every swap
     * attempt, inside the kernels that take the decision, and counts round trips and up / down moves -- what tells
     * whether a ladder works and how its betas should be re-spaced (round-trip rate and up-moving fraction:
     * Katzgraber 2006; equal-rejection spacing: Syed 2019).  Read with apemost_hip_replica_flow_get.
     * "Rung" = a chain's index a inside its ladder (0 = the beta = 1 end, n-1 = the last chain).  A replica is a
     * point travelling over rungs; replicas are labelled 0 .. n-1.
     * State.  Per rung: replica[a], the label of the replica whose params sit at the rung; heading[a] in {0 none,
     * 1 from-bottom: the last end visited was rung 0, 2 from-top: the last end visited was rung n-1}; the counters
     * n_up[a], n_down[a], attempts[a].  Per replica: round_trips[label].  Initially replica[a] = a, heading[0] = 1,
     * heading[n-1] = 2, all others 0 (n = 1: heading 0, and nothing ever changes), counters 0.
     * For every swap attempt of any schedule -- pair (a, a+1), decided and applied by the unchanged primitives --
     * in this order:
     *   1. if the swap was accepted, rungs a and a+1 exchange (replica, heading): the label follows params, as
     *      parallel_tempering_do_swap moves them, not the best point, which its quirk copies;
     *   2. if a = 0 and the replica now at rung 0 has heading 2: round_trips[its label] += 1; then its heading = 1;
     *   3. if a+1 = n-1: the replica now at rung n-1 gets heading 2;
     *   4. for both rungs of the pair: n_up += 1 if the rung's heading is now 1, n_down += 1 if it is 2;
     *   5. attempts[a] += 1 (the lower rung only): swapcount[a] / attempts[a] is the pair's swap rate.
     * Counters move only at attempts a rung takes part in: under the default schedule the pair is drawn
     * independently of the state, so this is an unbiased subsample of the per-round up / down fraction; under
     * even-odd sweeps it is nearly every sweep.  A RANDOMSWAP attempt that draws "no attempt" changes nothing.
     * The (replica, heading) word of a rung is one more field of the swap hand-off record, so the flow, like every
     * other result, does not depend on launch boundaries, waves per chain or kernel family, and the chain itself
     * -- every sample row, every state field -- is bit for bit what it is without the flag.
     * Runs in the variant kernel instantiations (1, 2, 4 or 8 waves per chain; 6 is APEMOST_HIP_ERR_INVALID); the
     * default kernels carry no test for it.  Combines with every model (user-supplied ones included), every swap
     * schedule, both proposal laws, ADAPT, RWM, both launch forms and kernel families, and ladder batches (labels
     * are per ladder, every array is [n_ladders][n_chains]).
     * Not sharded: apemost_hip_create with chain_offset != 0 or n_chains_global != n_chains is refused with
     * APEMOST_HIP_ERR_UNSUPPORTED before any device is touched, and so are, on such a sampler,
     * apemost_hip_run_shards, apemost_hip_edge_export / import / exchange and apemost_hip_set_chain_offset. */
    APEMOST_HIP_FLAG_TRACK_REPLICAS = 4096
};

typedef struct {
    int32_t abi_version;     /* APEMOST_HIP_ABI_VERSION */
    int32_t device;          /* HIP device ordinal */
    int32_t model;           /* APEMOST_MODEL_* */
    int32_t n_par;           /* get_n_par(), src/mcmc_gettersetter.c:174-183 */
    int32_t n_chains;        /* chains resident on this device (a shard of the ladder) */
    int32_t n_data;          /* m->data->size1 */
    int32_t n_cols;          /* m->data->size2 (>= 2) */
    int32_t waves_per_chain; /* likelihood wavefronts per chain: 1, 2, 4, 6 or 8; 0 = choose */
    int32_t lds_policy;      /* data vector staged in LDS: 0 = choose, 1 = always (if it fits), 2 = never */
    int32_t flags;           /* APEMOST_HIP_FLAG_* bits, 0 = defaults */
    int64_t chain_offset;    /* ladder index of local chain 0 */
    int64_t n_chains_global; /* N_BETA, src/define_defaults.h:24-31 */
    uint64_t seed;           /* rocRAND Philox4x32-10 seed (role of GSL_RNG_SEED) */
    double sigma;            /* SIGMA, apps/simplesin.c:8-10 */
    double hmin;             /* HMIN, apps/pulse.c:8-10 */
    uint64_t circular_params; /* bit p set: parameter p wraps around [min,max] instead of being
                               * redrawn (-DCIRCULAR_PARAMS, src/markov_chain.c:241-265) */
    double adapt_target;      /* TARGET_ACCEPTANCE_RATE (src/define_defaults.h:77-79) for
                               * APEMOST_HIP_FLAG_ADAPT; 0 = the reference's default 0.5 */
    const char *device_model_source; /* APEMOST_MODEL_USER: path of the device source of the likelihood
                                      * (include/apemost_device_model.h); NULL otherwise */
} apemost_hip_config;

/* Host-side structure-of-arrays view of n_chains chains; any pointer may be NULL
 * (that field is skipped).  Shapes: [n_chains][n_par] or [n_chains]. */
typedef struct {
    double *params;           /* m->params */
    double *params_best;      /* m->params_best */
    double *step;             /* m->params_step */
    double *pmin;             /* m->params_min */
    double *pmax;             /* m->params_max */
    uint64_t *params_accepts; /* m->params_accepts */
    uint64_t *params_rejects; /* m->params_rejects */
    double *beta;             /* parallel_tempering_mcmc.beta */
    double *prob;             /* m->prob */
    double *prior;            /* m->prior */
    double *prob_best;        /* m->prob_best */
    uint64_t *accept;         /* m->accept */
    uint64_t *reject;         /* m->reject */
    uint64_t *n_iter;         /* m->n_iter */
    uint64_t *swapcount;      /* parallel_tempering_mcmc.swapcount */
    uint64_t *ticks;          /* [n_chains] Metropolis updates performed = RNG address of the next one */
} apemost_hip_state_view;

/* calibration knobs: src/define_defaults.h:24-86, src/markov_chain.h:25-32 */
typedef struct {
    uint32_t burn_in_iterations; /* BURN_IN_ITERATIONS */
    uint32_t iter_limit;         /* ITER_LIMIT */
    uint32_t iter_readjust;      /* ITER_READJUST */
    int32_t no_rescaling_limit;  /* NO_RESCALING_LIMIT */
    double rat_limit;            /* desired_acceptance_rate argument */
    double target_global;        /* TARGET_ACCEPTANCE_RATE */
    double max_ar_deviation;     /* MAX_AR_DEVIATION */
    double mul;                  /* MUL */
    double adjust_step;          /* DEFAULT_ADJUST_STEP */
    int32_t progress_chain;      /* local chain whose readjustments are logged for calibration_progress.data
                                  * (src/markov_chain_calibrate.c:1143-1146; the reference reopens that file
                                  * "w" for every chain, so the last chain calibrated is the one whose lines
                                  * survive), or -1 */
    int32_t reserved;            /* 0 */
} apemost_hip_calib_config;

/* ---- environment ---------------------------------------------------------- */
const char *apemost_hip_last_error(void);
int apemost_hip_abi_version(void);
int apemost_hip_device_count(int *count);
/* name[] receives the gcnArchName; fails unless it is a gfx950 part */
int apemost_hip_device_info(int device, char *name, size_t name_len, int *compute_units,
                            uint64_t *hbm_bytes);

/* ---- lifetime ------------------------------------------------------------- */
int apemost_hip_create(const apemost_hip_config *cfg, apemost_hip_sampler **out);
/* ---- ladder batches: many independent ladders in one sampler and one launch -------------------
 * apemost_hip_create_batch makes ONE sampler that holds n_ladders independent ladders of cfg->n_chains chains each
 * (cfg->n_chains is the number PER LADDER; cfg->seed is ignored, ladder b runs under seeds[b]).  All ladders share
 * the model, n_par, n_data, n_cols, the flags, n_swap and the round counter; each has its own seed, its own data
 * matrix and its own state.  One launch steps all n_ladders * n_chains chains, one workgroup per chain, and swaps
 * happen inside a ladder only.
 * Indexing: local chain c of the sampler is chain a = c % n_chains of ladder b = c / n_chains (ladder-major).  Every
 * RNG address of the header's scheme is taken with chain = a under the key seeds[b]: the chain streams, the swap
 * stream (subsequence APEMOST_HIP_SWAP_SUBSEQUENCE) and, with APEMOST_HIP_FLAG_SWAP_EVEN_ODD, the pair streams
 * (+ 1 + a); the swap schedule's n_chains_global is the per-ladder n_chains.  Streams do not depend on the launch
 * shape, so ladder b is, bit for bit, the chain a stand-alone sampler with seed seeds[b], ladder b's data and the
 * same waves_per_chain produces (the summation order of the likelihood follows the wave count, and a count left to
 * the engine is chosen for the whole grid).
 * Geometry -- waves per chain, LDS staging, the one-barrier kernels and their helper wavefront, the residency check
 * behind multi-round launches, the calibration's segment shapes -- follows the TOTAL number of chains, which is what
 * occupies the chip: 16 ladders of 8 chains are launched like one ladder of 128.
 * The existing calls on a batch:
 *   apemost_hip_set_data gives every ladder the same matrix (replicas); apemost_hip_set_data_ladder one ladder its own;
 *   state views, sample rows ([n_steps][n_ladders * n_chains][n_par+2]), the summary's prob_sum, the packed and text
 *   sample reads, calc_model / calibrate_* (first, count) and launch_round_for index chains 0 .. n_ladders * n_chains
 *   - 1, ladder-major; a range may span ladders;
 *   apemost_hip_sampler_swap_pair is ambiguous and returns APEMOST_HIP_ERR_INVALID (= -1, with a last_error text):
 *   apemost_hip_swap_pair(seeds[b], round, n_chains) answers per ladder;
 *   n_ladders = 1 is legal and equals an ordinary sampler with that seed.
 * Supported: the four built-in models, the default swap schedule and APEMOST_HIP_FLAG_SWAP_EVEN_ODD, both proposal-law
 * flags, SINGLE_ROUND_LAUNCHES, TWO_BARRIER_STEP, circular parameters, waves_per_chain 0, 1, 2, 4 or 8.  Batches run
 * in the variant kernel instantiations (like the proposal laws): the default kernels carry no test for them.
 * Refused by apemost_hip_create_batch with APEMOST_HIP_ERR_UNSUPPORTED, before any device is touched -- nothing runs
 * silently as a single ladder: APEMOST_MODEL_USER; the flags RANDOMSWAP, ADAPT, RWM, TEST_REFUSE_COOPERATIVE,
 * TEST_WITHHOLD_PUBLISH, COOPERATIVE_LAUNCH (the engine still takes cooperative launches by itself where it would
 * for a ladder of as many chains) and USER_ONE_BARRIER; chain_offset != 0 or n_chains_global != n_chains (batches
 * are not sharded).  Refused on a batch with APEMOST_HIP_ERR_UNSUPPORTED: apemost_hip_run_shards,
 * apemost_hip_edge_export / import / exchange, apemost_hip_set_chain_offset, and apemost_hip_loglike when
 * n_ladders > 1 (no single data matrix).  waves_per_chain = 6 is APEMOST_HIP_ERR_INVALID, as for every variant. */
int apemost_hip_create_batch(const apemost_hip_config *cfg, int32_t n_ladders, const uint64_t *seeds,
                             apemost_hip_sampler **out);
/* ---- ragged ladder batches: one data set per ladder, each of its own length --------------------
 * apemost_hip_create_batch_ragged is apemost_hip_create_batch with one number of data rows per ladder: n_data[b] >= 1
 * rows for ladder b (cfg->n_data is ignored on input, as cfg->seed is; the sampler's own n_data is the largest of
 * them).  Everything said of apemost_hip_create_batch holds, its list of refusals included, with these changes:
 *   Identity: ladder b is, bit for bit, the stand-alone sampler with n_data = n_data[b], seed seeds[b], ladder b's
 *   data and the same waves_per_chain.  Every loop of the likelihood takes its trip counts from the ladder's own
 *   length, which is uniform over the chain's workgroup.
 *   Data: apemost_hip_set_data_ladder(s, b, data) reads n_data[b] rows of [n_cols].  apemost_hip_set_data, which gives
 *   every ladder one matrix, returns APEMOST_HIP_ERR_INVALID on a batch whose lengths differ (use set_data_ladder).
 *   On the device the matrices lie one behind the other, column-major, ladder b's at the offset
 *   sum over b' < b of n_cols * n_data[b'] doubles (apemost_hip_ragged_layout).
 *   Geometry: one launch has one LDS size and one wave count.  What follows the data length -- LDS staging and its
 *   size, the by-data bound of waves_per_chain = 0, the residency check, the calibration's segment shapes -- follows
 *   the LONGEST ladder; what follows the chip follows the total number of chains, as in every batch.  A batch's
 *   launch therefore lasts about as long as its longest ladder's.
 *   Folds: those over sample rows alone (summary, joint, evidence, autocorr, peaks, derived) know nothing of data and
 *   work as on every batch.  apemost_hip_predict_* at the data's abscissae (x == NULL) and apemost_hip_pointwise_* keep
 *   their rectangular arrays [n_keep][n_x], n_x being the longest data among the KEPT chains' ladders; kept chain k
 *   folds its own len[k] <= n_x series, which apemost_hip_predict_lengths / apemost_hip_pointwise_lengths report.
 *   Entries with i >= len[k] are never written: after *_get they hold their initial values (origin, sums and
 *   log-sum-exp words 0, vmin +inf, vmax -inf, counts 0), and *_set takes the same rectangular arrays back.  Predict
 *   over a caller's grid (x != NULL) does not depend on the data and is unchanged.  The pointwise tail
 *   (apemost_hip_pointwise_tail_begin) on kept chains whose ladders differ in length is refused with
 *   APEMOST_HIP_ERR_UNSUPPORTED: a follow-up.
 * If all n_data[b] are equal the sampler is in every respect the one apemost_hip_create_batch makes with that n_data.
 * APEMOST_HIP_ERR_INVALID, before any device is touched: n_data == NULL, a length < 1, or a total
 * sum of n_cols * n_data[b] beyond 2^60 doubles (the allocation's arithmetic). */
int apemost_hip_create_batch_ragged(const apemost_hip_config *cfg, int32_t n_ladders, const uint64_t *seeds,
                                    const int32_t *n_data, apemost_hip_sampler **out);
/* The data layout of a ragged batch, on the host alone (no device, no sampler): offsets[b] = sum over b' < b of
 * n_cols * n_data[b'] for b = 0 .. n_ladders (the last one is the whole allocation, also in *total), *n_data_max the
 * longest length.  offsets, n_data_max and total may each be NULL.  The argument errors are those of
 * apemost_hip_create_batch_ragged. */
int apemost_hip_ragged_layout(int32_t n_ladders, int32_t n_cols, const int32_t *n_data, uint64_t *offsets,
                              int32_t *n_data_max, uint64_t *total);
/* the data rows of ladder `ladder`: n_data[ladder] of a ragged batch, cfg.n_data of an equal batch and (ladder 0) of
 * an ordinary sampler */
int apemost_hip_ladder_n_data(apemost_hip_sampler *s, int32_t ladder, int32_t *n_data);
/* 1 for an ordinary sampler */
int apemost_hip_n_ladders(apemost_hip_sampler *s, int32_t *n_ladders);
/* row-major [n_data][n_cols] host matrix for ladder `ladder` alone (ladder 0 of an ordinary sampler: its data); on a
 * ragged batch n_data is that ladder's own */
int apemost_hip_set_data_ladder(apemost_hip_sampler *s, int32_t ladder, const double *data_rowmajor);
int apemost_hip_destroy(apemost_hip_sampler *s);
int apemost_hip_synchronize(apemost_hip_sampler *s);
/* the HIP stream (hipStream_t) every launch of this sampler goes to */
int apemost_hip_stream(apemost_hip_sampler *s, void **stream);
int apemost_hip_waves_per_chain(apemost_hip_sampler *s, int *waves, int *data_in_lds);
/* how this sampler's stepping launches are issued as things stand: the one-barrier kernel (1; 2: in its form
 * with a helper wavefront, the models with a prior on ladders of at most one chain per CU whose betas are all
 * > 0 with a finite 1/beta -- so it depends on the state: a set_state whose betas include 0 or one below
 * ~5.6e-309 turns it to 1, one without them back to 2; before any betas are set it assumes they allow it) or the
 * two-phase one (0), multi-round launches through hipLaunchCooperativeKernel or plain, and how many
 * rounds one launch may hold (1: the grid is not resident, a cooperative launch was refused, or a
 * hand-off timed out) */
int apemost_hip_launch_policy(apemost_hip_sampler *s, int32_t *one_barrier, int32_t *cooperative, int32_t *max_rounds);
/* APEMOST_MODEL_USER: seconds hiprtc took to compile this sampler's device model (the kernels of the
 * user's likelihood for 1, 2, 4 and 8 waves per chain); 0 when the process had compiled the same source
 * before.  Fails for the built-in models. */
int apemost_hip_user_model_compile_seconds(apemost_hip_sampler *s, double *seconds);
/* Which of the optional hooks of include/apemost_device_model.h this sampler's device model defines: *has_curve
 * (apemost_user_curve: apemost_hip_predict_* work) and *has_pointwise (apemost_user_pointwise: apemost_hip_pointwise_*
 * work), each 0 or 1.  The hooks' kernels are a second run-time module, compiled on the first call of this function
 * or of any predict_* / pointwise_* entry point of the sampler -- never at create -- and kept per process by source
 * text like the first; *compile_seconds is hiprtc's time for it, 0 when it came from that cache (a source without
 * hooks is compiled once per process too).  Any pointer may be NULL.  APEMOST_HIP_ERR_INVALID for a sampler of a
 * built-in model, or when a source announces a hook (APEMOST_USER_CURVE, APEMOST_USER_POINTWISE) and does not define
 * its function. */
int apemost_hip_user_hooks(apemost_hip_sampler *s, int32_t *has_curve, int32_t *has_pointwise, double *compile_seconds);
/* move the shard along the ladder (single-chain API of the C host layer: the chain's ladder
 * position selects its RNG streams); offset + n_chains must stay <= n_chains_global */
int apemost_hip_set_chain_offset(apemost_hip_sampler *s, int64_t chain_offset);

/* ---- data and state (mcmc_load_data / setup_chains / read_calibration_file) */
/* row-major [n_data][n_cols] host matrix, as gsl_matrix stores it */
int apemost_hip_set_data(apemost_hip_sampler *s, const double *data_rowmajor);
int apemost_hip_set_state(apemost_hip_sampler *s, const apemost_hip_state_view *v);
int apemost_hip_get_state(apemost_hip_sampler *s, const apemost_hip_state_view *v);
/* position of the swap stream = number of tempering_interaction() calls so far */
int apemost_hip_set_round(apemost_hip_sampler *s, uint64_t round, int swap_pending);
int apemost_hip_get_round(apemost_hip_sampler *s, uint64_t *round, int *swap_pending);

/* ---- the hot path --------------------------------------------------------- */
/* calc_model() for local chains [first, first+count) at their current params: prob,
 * prior updated on device (src/parallel_tempering.c:88,147,185 call sites);
 * count < 0 means every chain from `first` on */
int apemost_hip_calc_model(apemost_hip_sampler *s, int32_t first, int32_t count);

/* calc_model() at arbitrary points (apps/eval_main.c:52-66): n points, params
 * [n][n_par], beta [n]; results to host arrays prob[n], prior[n] */
int apemost_hip_loglike(apemost_hip_sampler *s, int32_t n, const double *params, const double *beta,
                        double *prob, double *prior);

/* One launch of the round kernel: optionally apply the pending swap attempt
 * (tempering_interaction for swap-stream position `round`), then n_steps x
 * {markov_chain_step, mcmc_check_best, n_iter++, sample row}.  d_samples is a
 * DEVICE pointer to [n_steps][n_chains][n_par+2] doubles (params.., prob,
 * prob-prior; the rows the reference prints to <name>-chain-<i>.prob.dump and
 * prob-chain<i>.dump) or NULL.  Asynchronous on the sampler's stream.
 * Sharded ladders call apemost_hip_edge_* around it; whole ladders use
 * apemost_hip_run. */
int apemost_hip_launch_round(apemost_hip_sampler *s, uint32_t n_steps, int apply_swap,
                             double *d_samples);

/* Several rounds in one launch: [pending swap] steps [swap] steps ... (n_rounds x n_steps steps,
 * n_rounds-1 swap attempts exchanged between workgroups inside the launch).  d_samples:
 * DEVICE [n_rounds*n_steps][n_chains][n_par+2] or NULL.  n_rounds may not exceed
 * apemost_hip_max_rounds_per_launch() (1 when the grid cannot be fully resident), and on a sharded
 * ladder none of the in-launch swap attempts may pick a pair that straddles a shard edge. */
int apemost_hip_launch_rounds(apemost_hip_sampler *s, uint32_t n_rounds, uint32_t n_steps, int apply_swap,
                              double *d_samples);
int apemost_hip_max_rounds_per_launch(apemost_hip_sampler *s, int32_t *max_rounds);

/* n_steps x markov_chain_step_for(m, param) (src/markov_chain.c:317-333) for every resident
 * chain: only parameter `param` is proposed, only its counters move */
int apemost_hip_launch_round_for(apemost_hip_sampler *s, uint32_t n_steps, int32_t param, double *d_samples);

/* run_sampler() for a ladder that lives entirely on this device: n_rounds x
 * {n_swap steps, swap attempt}; the last swap is applied before returning
 * control (still asynchronous).  d_samples: DEVICE [n_rounds*n_swap][n_chains][n_par+2] or NULL */
int apemost_hip_run(apemost_hip_sampler *s, uint64_t n_rounds, uint32_t n_swap, double *d_samples);

/* device buffers for sample rows, for hosts without their own device allocator (the C host
 * layer): [n_steps][n_chains][n_par+2] doubles */
int apemost_hip_samples_alloc(apemost_hip_sampler *s, uint64_t n_steps, double **d_samples);
int apemost_hip_samples_read(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, double *host);
int apemost_hip_samples_free(apemost_hip_sampler *s, double *d_samples);

/* The same read without stalling the sampler: the copy is queued behind everything launched so far
 * but runs on a second stream, so launches issued after this call overlap with it (double-buffered
 * sample sinks: the device fills buffer B while buffer A drains to the host).  host_samples should
 * be pinned memory (apemost_hip_host_alloc).  counters, if not NULL, receives [2][n_chains]
 * uint64: m->accept then m->reject of every chain as they stand after the launches issued so far
 * (what the reference prints to acceptance_rate.dump, src/parallel_tempering.c:320-326), without a
 * host synchronisation of the sampler's stream.  apemost_hip_samples_wait blocks until the latest
 * such read has landed (and reports a void launch like apemost_hip_samples_read). */
int apemost_hip_samples_read_async(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                   double *host_samples, uint64_t *counters);
/* The same with the rows packed ON THE DEVICE into what the sink will write, so that only that crosses
 * PCIe and the host writes the pinned buffer as it is: of the n_steps rows the steps skip, skip + thin,
 * ... are kept (*n_kept of them);
 *   layout 0: per kept step the parameter vectors of chains 0 .. n_param_chains-1, then
 *             (prob, prob - prior) of every chain  -- the record of the C host's binary sink;
 *   layout 1: the kept rows themselves, [n_kept][n_chains][n_par+2].
 * d_packed: DEVICE scratch for the packed batch (apemost_hip_samples_alloc sizes fit), host_packed:
 * pinned; the wait as for apemost_hip_samples_read_async; counters, if not NULL, receives [2][n_chains]
 * uint64 as there and BEHIND them n_par doubles: chain 0's parameter vector after the batch's last step
 * (the reference's progress line prints chain 0's current point, src/parallel_tempering.c:309-318; a
 * packed batch may have kept an older step, or none) -- (2 n_chains + n_par) * 8 bytes. */
int apemost_hip_samples_pack_read_async(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                        uint64_t skip, uint64_t thin, int32_t n_param_chains, int32_t layout,
                                        double *d_packed, double *host_packed, uint64_t *counters, uint64_t *n_kept);
int apemost_hip_samples_wait(apemost_hip_sampler *s);
/* The kept steps skip, skip + thin, ... of d_samples as the reference's text dump lines, formatted ON THE DEVICE,
 * byte for byte what glibc's printf gives: "%.15e\n" for the parameter files of chains 0 .. n_param_chains-1 and
 * "%6e\t%6e\n" (prob, prob - prior) for the prob-chain files of every chain.  One byte stream per file, in this
 * order: stream c*n_par + p holds parameter p of chain c (c < n_param_chains), stream n_param_chains*n_par + c
 * the prob-chain lines of chain c.  Stream i is host_text[host_offsets[i], host_offsets[i+1]), and
 * host_offsets[n_streams] is the batch's total.
 * The sizing call gives, for a batch shape, n_streams, the host text buffer it needs (text_bytes: every line at
 * its longest) and the DEVICE scratch it needs (scratch_bytes); any of the three pointers may be NULL.
 * The read is queued like apemost_hip_summary_accumulate, behind the launches issued so far on the stream of
 * apemost_hip_samples_read_async: launches issued afterwards overlap with it, and host_text / host_offsets
 * (pinned: apemost_hip_host_alloc) hold the batch once apemost_hip_samples_wait has returned.  scratch_bytes,
 * text_capacity and n_offsets (at least n_streams + 1) are the sizes of the buffers given: one that is too
 * small gives APEMOST_HIP_ERR_INVALID, and then nothing is queued or copied. */
int apemost_hip_samples_text_bound(apemost_hip_sampler *s, uint64_t n_steps, uint64_t skip, uint64_t thin,
                                   int32_t n_param_chains, uint64_t *n_streams, uint64_t *text_bytes,
                                   uint64_t *scratch_bytes);
int apemost_hip_samples_text_read_async(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps,
                                        uint64_t skip, uint64_t thin, int32_t n_param_chains, void *d_scratch,
                                        uint64_t scratch_bytes, char *host_text, uint64_t text_capacity,
                                        uint64_t *host_offsets, uint64_t n_offsets);
/* device memory on the sampler's device (the scratch of the text read); the free waits for the sampler's
 * streams */
int apemost_hip_device_alloc(apemost_hip_sampler *s, uint64_t bytes, void **d);
int apemost_hip_device_free(apemost_hip_sampler *s, void *d);
/* page-locked host memory for those reads */
int apemost_hip_host_alloc(size_t bytes, void **p);
int apemost_hip_host_free(void *p);

/* pair index `a` that tempering_interaction() will pick at swap-stream position
 * `round` (parallel_tempering_decide_swap_now, interaction.c:87-97); -1 if n_global==1 */
int64_t apemost_hip_swap_pair(uint64_t seed, uint64_t round, int64_t n_chains_global);
/* the same for this sampler's ladder and swap schedule (with APEMOST_HIP_FLAG_RANDOMSWAP the pair
 * comes from word 1 of the block; with APEMOST_HIP_FLAG_SWAP_EVEN_ODD the lowest lower chain of sweep
 * `round`: round % 2 if that is <= n_chains_global - 2, else -1) */
int64_t apemost_hip_sampler_swap_pair(const apemost_hip_sampler *s, uint64_t round);
/* how many of the swap attempts first_round, first_round + 1, ... (at most max_rounds) pick a pair
 * that lies inside this sampler's shard or outside it altogether, i.e. stops at the first pair that
 * straddles one of the shard's edges: the rounds a sharded ladder may put into one launch (even-odd
 * sweeps: stops at the first sweep whose parity puts a pair across one of the edges) */
int64_t apemost_hip_rounds_within_shard(const apemost_hip_sampler *s, uint64_t first_round, int64_t max_rounds);

/* sharded ladders: the swap partner across a shard edge.  side 0 = lower
 * neighbour (chain_offset-1), 1 = upper neighbour.  A record is
 * apemost_hip_edge_doubles(n_par) doubles: beta, prob, prob_best,
 * params[n_par], params_best[n_par].  d_buf is a DEVICE pointer (what RCCL
 * sends/receives).  export packs this shard's edge chain; import fills the
 * halo slot the next launch_round(apply_swap=1) reads. */
int32_t apemost_hip_edge_doubles(int32_t n_par);
int apemost_hip_edge_export(apemost_hip_sampler *s, int side, double *d_buf);
int apemost_hip_edge_import(apemost_hip_sampler *s, int side, const double *d_buf);

/* ---- one process, several devices (or several shards on one device) --------------------------
 * The same block-partitioned ladder as the one-process-per-GPU driver, for hosts that
 * stay a single process (the C host layer with APEMOST_DEVICES=0,1,...): shards[j] holds chains
 * [offset_j, offset_j + n_j) of the same ladder (same seed, same n_chains_global, offsets
 * ascending and contiguous), each on its own device and stream.
 *
 * apemost_hip_edge_exchange: the pending swap attempt picked the pair that straddles lower|upper:
 * both shards export their edge record, the records cross with hipMemcpyPeerAsync (xGMI between
 * devices, a device copy within one), and land in the halo rows the next launch reads -- all
 * stream-ordered with events, no host synchronisation.
 *
 * apemost_hip_run_shards: run_sampler() over all shards in lock step: rounds are batched into
 * multi-round launches up to the next swap attempt that needs a neighbour's record, exactly as
 * apemost_hip_run does on one device; d_samples[j] (may be NULL) receives shard j's rows,
 * [n_rounds*n_swap][n_j][n_par+2].  The result is bit-identical to the whole ladder on one
 * sampler. */
int apemost_hip_edge_exchange(apemost_hip_sampler *lower, apemost_hip_sampler *upper);
int apemost_hip_run_shards(apemost_hip_sampler **shards, int32_t n_shards, uint64_t n_rounds, uint32_t n_swap,
                           double **d_samples);

/* ---- calibration ---------------------------------------------------------- */
void apemost_hip_calib_defaults(apemost_hip_calib_config *c);
/* markov_chain_calibrate() (burn_in + calibrate_orig) on device for local chains
 * [first, first+count); status[count] (host) receives 0 / 1 step too large /
 * 2 iteration limit per chain, iters[count] the calibrate_orig sweep counts.
 * With burn_in_only != 0 only burn_in() runs (-DSKIP_CALIBRATE_ALLCHAINS). */
int apemost_hip_calibrate_chains(apemost_hip_sampler *s, int32_t first, int32_t count,
                                 const apemost_hip_calib_config *c, int burn_in_only,
                                 int32_t *status, uint64_t *iters);

/* The same in pieces.  The calibration runs as a sequence of launches ("segments"): a chain's trip
 * count is data-dependent, so every segment ends after a bounded number of likelihood evaluations per
 * chain, the chains that are done drop out, and the survivors are launched again -- with more
 * wavefronts per chain as they get fewer.  Results do not depend on where the segments are cut.
 *   begin  launches the first segment (asynchronous);
 *   poll   never blocks: if the segment in flight has ended, collects it and launches the next one;
 *          *active = chains still calibrating.  Hosts that drive several devices from one thread poll
 *          them in turn, and a host with a SIGINT handler polls between looks at its flag;
 *   cancel no further segments: end then returns with status -1 for the chains that were not done
 *          (their state is a consistent point of their calibration);
 *   end    polls and waits until no chain is left, then hands out status/iters of the chains begin named. */
int apemost_hip_calibrate_begin(apemost_hip_sampler *s, int32_t first, int32_t count,
                                const apemost_hip_calib_config *c, int burn_in_only);
int apemost_hip_calibrate_poll(apemost_hip_sampler *s, int32_t *active);
int apemost_hip_calibrate_cancel(apemost_hip_sampler *s);
/* several samplers (one per device) calibrating at once, driven by one thread: returns when a segment
 * of one of them has ended and been followed up, or none has chains left; *active_total = chains
 * still calibrating over all of them */
int apemost_hip_calibrate_wait_any(apemost_hip_sampler **samplers, int32_t n, int32_t *active_total);
int apemost_hip_calibrate_end(apemost_hip_sampler *s, int32_t *status, uint64_t *iters);
/* the readjustment log of apemost_hip_calib_config.progress_chain after calibrate_end: row k =
 * { iter, then per parameter (normalised step width, acceptance rate) } as the reference prints them
 * after its k-th readjustment; rows [capacity_rows][1 + 2 n_par], *n_rows = rows that exist */
int apemost_hip_calibrate_progress(apemost_hip_sampler *s, double *rows, int32_t capacity_rows, int32_t *n_rows);
/* the latest calibration in numbers: segments launched, likelihood evaluations of all its chains, and
 * launches and wall seconds per workgroup shape (index = likelihood wavefronts per chain) */
int apemost_hip_calibrate_stats(apemost_hip_sampler *s, uint64_t *segments, uint64_t *evaluations,
                                uint64_t launches_by_waves[9], double seconds_by_waves[9]);

/* ---- run summary: what `analyse` needs, folded on the device -------------------------------
 * The three quantities the analyse phase computes from the dump files (apemost_amd/host/src/analyse.c),
 * accumulated from the sample rows while they are still on the device:
 *   n             kept samples so far (the same for every chain);
 *   prob_sum[c]   sum of column n_par+1 (prob - prior) of chain c, a sequential `sum += v` in sample order
 *                 (analyse_data_probability);
 *   hist[h][p][b] counts of the values of parameter p of chain h < n_hist_chains in the nbins bins of
 *                 marginal_distribution() over [lo[p], hi[p]] (top edge widened by (hi-lo)/10000; values
 *                 outside, NaN included, are not counted);
 *   batch_sums[h][p][k]  sequential sums of the batches of batch_means_error(): sample n (counted from 1)
 *                 closes a batch when n % batch_size == batch_size - 1, so batch 0 holds batch_size - 1
 *                 samples and every later one batch_size; k < n_batches are closed, slot n_batches holds
 *                 the sum of the batch still open.  The array is [h][p][max_batches + 1].
 * Every sum is one thread's chain of additions in sample order: the results are bitwise equal to the host
 * loops, whatever the boundaries of the accumulate calls are.  Sharded ladders keep one summary per shard
 * (n_hist_chains = 0 on all but the shard that holds chain 0); the caller concatenates prob_sum. */
typedef struct {
    int32_t n_hist_chains; /* chains 0 .. n_hist_chains-1 get histograms and batch sums (0 .. n_chains) */
    int32_t nbins;         /* 1 .. 4096 */
    uint64_t batch_size;   /* >= 1 */
    uint64_t max_batches;  /* capacity: an accumulate that would close batch max_batches + 1 is invalid */
    const double *lo, *hi; /* host [n_par]: the histogram range, finite, lo < hi (may be NULL without histograms) */
} apemost_hip_summary_config;

/* host arrays; any pointer may be NULL (that part is skipped) */
typedef struct {
    uint64_t *n;
    double *prob_sum;   /* [n_chains] */
    uint64_t *hist;     /* [n_hist_chains][n_par][nbins] */
    double *batch_sums; /* [n_hist_chains][n_par][max_batches + 1] */
    uint64_t *n_batches;
} apemost_hip_summary_view;

/* allocates and zeroes the accumulator (a summary begun before is dropped) */
int apemost_hip_summary_begin(apemost_hip_sampler *s, const apemost_hip_summary_config *cfg);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2], the rows of
 * the launches issued so far) into the summary.  Asynchronous: queued behind those launches on the stream of
 * apemost_hip_samples_read_async, so launches issued afterwards overlap with it; apemost_hip_samples_wait (or
 * summary_get) must have returned before d_samples is written again. */
int apemost_hip_summary_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                   uint64_t thin);
/* copies the summary out (synchronises with the accumulates issued so far) */
int apemost_hip_summary_get(apemost_hip_sampler *s, const apemost_hip_summary_view *v);
/* loads a summary saved by summary_get into a summary begun with the same configuration (a resumed run):
 * n_batches, if given, must be the number that n closes */
int apemost_hip_summary_set(apemost_hip_sampler *s, const apemost_hip_summary_view *v);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_summary_end(apemost_hip_sampler *s);

/* ---- on-device peaks: exact medians and quartiles per mode, without dumps ---------------------
 * What the reference's peaks.exe (tools/peaks.c; the manual prefers it to reading the marginal histograms: "it is
 * exact") computes from the text dump of one chain's parameter, from columns that stay on the device: 8 bytes per
 * kept step, kept chain and parameter.  For `peaks.exe min max file`, column (k, p) being the file and
 * [lo[p], hi[p]] being [min, max]:
 *   1. filter   the values with v >= lo && v <= hi are kept, both ends inclusive; NaN is dropped (:101).  n_values
 *               of them.
 *   2. sort     ascending as numbers (:147).  The device sorts the keys bits ^ (bits >> 63 ? ~0 : 1 << 63), which
 *               order like the doubles; -0.0 comes before +0.0, one of the orders the tool's qsort may leave.
 *   3. cut      gap = (hi - lo) / 100; a new peak starts at sorted index i > 0 when v[i] - v[i-1] > gap, strictly,
 *               in fp64 as written (:151, :161-188).  n_peaks counts them all; the first 99 are described (the tool
 *               asserts npeaks < 100).  With n_values == 0 there is no peak (the tool reads uninitialised memory).
 *   4. select   peak c covers the sorted indices left[c] .. right[c], n = right - left + 1 values.  q[c][j], j = 0,
 *               1, 2, is v[left + n*(j+1)/4 - 1] (integer division): the left quartile, the median, the right
 *               quartile (:56-80).  Bit j of q_set[c] says that the index count n*(j+1)/4 is at least 1; where it is
 *               0 the statistic does not exist and q[c][j] is 0.
 * Peaks come in ascending order of position.  Slots of peaks that a column does not have are 0.
 * apemost_hip_peaks_table turns one column into the tool's printed table.
 * Sharded ladders: the caller begins peaks on the shard that holds the chain, as for n_hist_chains.  Ladder batches:
 * `chains` indexes the grid's local chains, ladder-major: b * n_chains is ladder b's chain 0. */
typedef struct {
    int32_t n_keep;          /* number of kept chains, 1 .. n_chains; n_keep * n_par <= 65535 */
    const int32_t *chains;   /* host [n_keep]: local chain indices, strictly increasing */
    uint64_t capacity;       /* kept samples per column, 1 .. 2^30 */
    const double *lo, *hi;   /* host [n_par]: peaks.exe's min and max per parameter, finite, lo < hi */
} apemost_hip_peaks_config;
typedef struct {
    uint64_t *n;             /* samples stored per column */
    uint64_t *n_values;      /* [n_keep][n_par] admitted by the filter */
    uint32_t *n_peaks;       /* [n_keep][n_par] peaks found (may exceed 99) */
    uint64_t *left, *right;  /* [n_keep][n_par][99] sorted-index bounds of each peak, in ascending order of position */
    double *q;               /* [n_keep][n_par][99][3] v[left+n/4-1], v[left+n*2/4-1], v[left+n*3/4-1] */
    uint8_t *q_set;          /* [n_keep][n_par][99] bit j: q[..][j] exists (its index count >= 1) */
} apemost_hip_peaks_view;    /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates cols[n_keep][n_par][capacity] on the device (columns begun before are dropped).  APEMOST_HIP_ERR_INVALID,
 * before any device work, for a NULL config, n_keep or a chain index out of range, chains not strictly increasing, a
 * capacity outside [1, 2^30], or a range that is not finite with lo < hi. */
int apemost_hip_peaks_begin(apemost_hip_sampler *s, const apemost_hip_peaks_config *cfg);
/* appends the parameter values of the kept chains at the kept steps skip, skip + thin, ... of d_samples (DEVICE
 * [n_steps][n_chains][n_par+2], the rows of the launches issued so far) to the columns.  Asynchronous and queued
 * like apemost_hip_summary_accumulate: the round kernels never wait for it, and apemost_hip_samples_wait (or
 * peaks_get) must have returned before d_samples is written again.  A call that would store more than `capacity`
 * samples is APEMOST_HIP_ERR_INVALID and stores nothing. */
int apemost_hip_peaks_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                 uint64_t thin);
/* steps 1 to 4 on the device for every column, in scratch memory of 8 bytes per column and stored sample rounded up
 * to a power of two (at least 4096), and the view filled (synchronises with the accumulates issued so far).  The
 * stored columns are only read: accumulates may go on, and a later get describes the longer columns.  When a column
 * has 100 peaks or more the view is still filled -- n_peaks with the true count, the rest for the first 99 peaks
 * -- and the call returns APEMOST_HIP_ERR_INVALID with a message that names (k, p): the reference aborts there. */
int apemost_hip_peaks_get(apemost_hip_sampler *s, const apemost_hip_peaks_view *v);
/* frees the columns (apemost_hip_destroy does too) */
int apemost_hip_peaks_end(apemost_hip_sampler *s);
/* Host arithmetic only, no device and no sampler: column (k, p) of a view of n_par parameters (n_values, n_peaks,
 * left, right, q and q_set all given) as the table peaks.exe prints.  In position order each statistic that does
 * not exist keeps the value it had after the peak before, 0 at the start (the tool's three variables live outside
 * its loop, :130); share = 1.0 * n / n_values; the rows are put in descending order of share by the selection
 * sort of src/gsl_helper.c:102-127 (strict >, rows j and best change places, so equal shares keep the order that
 * leaves).  table receives n_peaks rows of four doubles -- median, median - left quartile, right quartile - median,
 * share -- and must hold 99; *n_rows = n_peaks.  The tool prints "median\t-\t+\tpercent\n", then "%f\t%f\t%f\t%f\n"
 * per row.  APEMOST_HIP_ERR_INVALID for a column with 100 peaks or more. */
int apemost_hip_peaks_table(const apemost_hip_peaks_view *v, int32_t n_par, int32_t k, int32_t p, double *table,
                            uint32_t *n_rows);

/* ---- on-device joint marginals: pair histograms and covariance, without dumps ------------------
 * What a corner plot and a parameter covariance need and neither the 1-D bin counts of the run summary nor the
 * sorted columns of peaks can give: how the parameters of a kept chain depend on each other.  Accumulated from the
 * sample rows while they are still on the device, per kept chain k:
 *   n                   kept samples so far;
 *   counts[k][q][a][b]  for pair q = (i, j), i < j: the samples whose parameter i lies in bin a and whose parameter j
 *                       lies in bin b.  The bins are the run summary's: nbins bins over [lo[p], hi[p]] on the edges
 *                       ((nbins-b)/nbins)*lo + (b/nbins)*hi, the top one widened by (hi-lo)/10000, bin b holding
 *                       e[b] <= v < e[b+1], found by gsl_histogram_increment's bisection (one device function for
 *                       both).  A sample counts only if both values have a bin: anything outside a parameter's range,
 *                       NaN included, is dropped.  While every sample lies inside the box the sums of counts[k][q] over
 *                       b and over a are the summary's hist of parameters i and j;
 *   origin[k][p]        parameter p of the first sample ever accumulated for chain k (0 before there is one);
 *   sum[k][p]           the sequential sum, in sample order, of d_p = v_p - origin[k][p] over every kept sample;
 *   cross[k][i][j]      for i <= j the sequential sum of d_i * d_j, the product rounded to fp64 and then added, stored
 *                       as the upper triangle row by row: (0,0), (0,1), .., (0,n_par-1), (1,1), ...
 *                       No filter on the moments: every kept sample enters, so a non-finite value makes the sums of
 *                       its parameter non-finite.  mean = origin + sum / n, covariance = (cross_ij - sum_i sum_j / n)
 *                       / (n - 1): taken about the origin, which lies inside the sample, the subtraction cancels
 *                       digits of the spread, not of the position.
 * Every count is exact and every sum is one thread's chain of additions in sample order: the results are bitwise
 * equal to a sequential host loop, whatever the boundaries of the accumulate calls are.
 * Sharded ladders: the caller begins on the shard that holds the chain.  Ladder batches: `chains` indexes the grid's
 * local chains, ladder-major: b * n_chains is ladder b's chain 0.  Both as for peaks. */
typedef struct {
    int32_t n_keep;          /* number of kept chains, 1 .. n_chains; n_keep * n_par <= 65535 */
    const int32_t *chains;   /* host [n_keep]: local chain indices, strictly increasing */
    int32_t nbins;           /* 1 .. 512 */
    int32_t n_pairs;         /* pairs given; 0 with pairs != NULL: the moments alone; ignored with pairs == NULL */
    const int32_t *pairs;    /* host [n_pairs][2], i < j, no duplicates; NULL: all n_par (n_par - 1) / 2 pairs i < j in
                                lexicographic order */
    const double *lo, *hi;   /* host [n_par]: the histogram range, finite, lo < hi, hi - lo finite */
} apemost_hip_joint_config;
typedef struct {
    uint64_t *n;             /* kept samples */
    uint64_t *counts;        /* [n_keep][n_pairs][nbins][nbins] */
    double *origin, *sum;    /* [n_keep][n_par] */
    double *cross;           /* [n_keep][n_par (n_par + 1) / 2], upper triangle row-major */
} apemost_hip_joint_view;    /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates and zeroes the accumulator, and device scratch for one staged piece of the kept columns (10 bytes per
 * value, about 4 Mi values).  A joint begun before is dropped once the new configuration has been accepted; a begin
 * that is refused leaves it open and accumulating as it was.  APEMOST_HIP_ERR_INVALID, before any device work, for a
 * NULL config, n_keep or a chain index out of range, chains not strictly increasing, nbins outside 1 .. 512, a pair
 * with i >= j, an index out of range or a duplicate, missing lo or hi, a range that is not finite with lo < hi, or a
 * counts array above 2^30 bytes. */
int apemost_hip_joint_begin(apemost_hip_sampler *s, const apemost_hip_joint_config *cfg);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2], the rows of the
 * launches issued so far) into the accumulator.  Asynchronous and queued like apemost_hip_summary_accumulate: the
 * round kernels never wait for it, and apemost_hip_samples_wait (or joint_get) must have returned before d_samples is
 * written again.  APEMOST_HIP_ERR_INVALID without joint_begin or with thin == 0. */
int apemost_hip_joint_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                 uint64_t thin);
/* copies the accumulator out (synchronises with the accumulates issued so far) */
int apemost_hip_joint_get(apemost_hip_sampler *s, const apemost_hip_joint_view *v);
/* loads a view saved by joint_get into a joint begun with the same configuration (a resumed run); the origin is
 * loaded too, and with n > 0 the next sample does not replace it */
int apemost_hip_joint_set(apemost_hip_sampler *s, const apemost_hip_joint_view *v);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_joint_end(apemost_hip_sampler *s);

/* ---- on-device evidence fold: stepping stone, corrected trapezoid, error bars ------------------
 * What the estimators of ln p(D|M,I) beyond the rectangle rule of the run summary need, and what a run without sample
 * dumps cannot recompute: per chain the variance and the batch sums of column n_par+1 (v = prob - prior = beta *
 * loglike), and the log-mean-exp of multiples of it.  Accumulated from the sample rows while they are still on the
 * device, for EVERY local chain c of the sampler:
 *   n               kept samples so far, the same for every chain;
 *   origin[c]       v of the first sample ever accumulated (0 before there is one);
 *   sum[c], sq[c]   with d = v - origin[c] the sequential sums, in sample order, of d and of d * d (the product rounded
 *                   to fp64 and then added).  mean v = origin + sum / n, variance = (sq - sum^2 / n) / (n - 1): taken
 *                   about the origin, which lies inside the sample, the subtraction cancels digits of the spread, not
 *                   of the position (v is of the order of the log-likelihood, its spread of the order of n_par);
 *   batch[c][k]     batch sums of v under the closing rule of the summary's batch_sums: sample n, counted from 1,
 *                   closes a batch when n % batch_size == batch_size - 1; k < n_batches are closed, slot n_batches holds
 *                   the sum of the batch still open.  The array is [n_chains][max_batches + 1];
 *   m[s][c], S[s][c]   for s = 0 (up) and 1 (down) a running log-sum-exp of x = coef_s[c] * v (one rounded
 *                   multiply): the first sample sets m = x, S = 1; every later one
 *                       if (x > m) { S = S * exp(m - x) + 1; m = x; } else S += exp(x - m);
 *                   with the device library's fp64 exp, so that ln mean exp(x) = m + ln(S / n).  m is the running
 *                   maximum of x (exact); S carries one rounding of exp, of the multiply and of the add per sample.
 *                   The arrays are [2][n_chains].  With coef_up[c] = (beta_{c-1} - beta_c) / beta_c and
 *                   coef_down[c] = -(beta_c - beta_{c+1}) / beta_c these are the stepping-stone ratios
 *                   ln Z(beta_{c-1}) / Z(beta_c) and -ln Z(beta_{c+1}) / Z(beta_c) (Xie et al. 2011); the device
 *                   sees the coefficients only, never a beta (apemost_amd/evidence.py computes them).
 * No filter: every kept sample enters, so a non-finite v makes the sums of its chain non-finite.
 * Every quantity is one thread's chain of operations in sample order, its state carried in device memory between
 * calls: origin, sum, sq, batch and m are bitwise equal to a sequential host loop, S is equal to it up to exp,
 * whatever the boundaries of the accumulate calls are.
 * Ladder batches: the chains are the grid's local chains, ladder-major, and so are the coefficients the caller
 * supplies.  Sharded ladders: one accumulator per shard with that shard's slice of the coefficients; the caller
 * concatenates. */
typedef struct {
    uint64_t batch_size;      /* >= 1 */
    uint64_t max_batches;     /* capacity: an accumulate that would close batch max_batches + 1 is invalid */
    const double *coef_up;    /* host [n_chains], finite */
    const double *coef_down;  /* host [n_chains], finite */
} apemost_hip_evidence_config;
typedef struct {
    uint64_t *n;              /* kept samples */
    double *origin, *sum, *sq; /* [n_chains] */
    double *batch;            /* [n_chains][max_batches + 1] */
    double *m, *S;            /* [2][n_chains]: up, down */
} apemost_hip_evidence_view;  /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates and zeroes the accumulator, and device scratch for one staged piece of the column (about 1 Mi values).
 * An evidence fold begun before is dropped once the new configuration has been accepted; a begin that is refused
 * leaves it open and accumulating as it was.  APEMOST_HIP_ERR_INVALID, before any device work, for a NULL config,
 * batch_size == 0, a missing or non-finite coefficient, or a max_batches whose batch array would exceed 2^40 values. */
int apemost_hip_evidence_begin(apemost_hip_sampler *s, const apemost_hip_evidence_config *cfg);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2], the rows of the
 * launches issued so far) into the accumulator.  Asynchronous and queued like apemost_hip_summary_accumulate, on the
 * stream of apemost_hip_samples_read_async: the round kernels never wait for it, and apemost_hip_samples_wait (or
 * evidence_get) must have returned before d_samples is written again.  APEMOST_HIP_ERR_INVALID, before any device
 * work, without evidence_begin, with thin == 0, or when the kept steps would close batch max_batches + 1. */
int apemost_hip_evidence_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                    uint64_t thin);
/* copies the accumulator out (synchronises with the accumulates issued so far) */
int apemost_hip_evidence_get(apemost_hip_sampler *s, const apemost_hip_evidence_view *v);
/* loads a view saved by evidence_get into a fold begun with the same configuration (a resumed run); with n > 0 the
 * next sample replaces neither the origin nor m and S.  APEMOST_HIP_ERR_INVALID when n closes more than max_batches
 * batches. */
int apemost_hip_evidence_set(apemost_hip_sampler *s, const apemost_hip_evidence_view *v);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_evidence_end(apemost_hip_sampler *s);

/* ---- on-device MBAR: evidence and reweighting from every chain's samples ------------------------
 * The multistate Bennett acceptance ratio (Shirts & Chodera 2008) over a tempered ladder: the minimum-variance
 * estimate of every ln Z(beta_k) from the loglike of EVERY kept step of EVERY chain, and the weights that carry those
 * samples to any beta.  The fold stores, for every local chain c and kept step, l = v / beta_c (one IEEE division) of
 * column n_par+1 (v = prob - prior = beta * loglike) in ell[capacity][n_chains], and counts per ladder the stored
 * values that are not finite.  A ladder has K chains; its sample n = (kept step t, chain c) is taken in stored order
 * (step-major, the chain fastest).  With g_k the running estimate of ln Z(beta_k) and T kept steps in the range
 * [t0, t0 + t_count):
 *   lnD_n = ln sum_j exp(beta_j l_n + c_j),   c_j = ln T - g_j              (row pass)
 *   G_t   = ln sum_n exp(beta_t l_n - lnD_n)                                (column pass, any target beta_t >= 0)
 *   g <- G(g) at the sampled betas                                          (one self-consistent iteration)
 * G(g + a) = G(g) + a: the library never normalises, the caller subtracts g_0 and judges convergence.  The order of
 * every operation -- one rounded multiply and one rounded add per x, the exact maxima, tiles of 4096 samples counted
 * from the range's first, 64 lane partials through the adjacent-pairs tree, tile partials in tile order -- is stated
 * in csrc/pt_mbar.h and restated in apemost_amd/mbar.py: a range equals a fold that holds only its rows, a ladder of
 * a batch the sampler that holds it alone, n_iter updates n_iter calls, all on the bits.
 * Whole ladders, ladder batches and ragged batches (the ladders are independent; betas ladder-major).  The fold
 * evaluates no model, so every model is allowed.  A shard of a sharded ladder (n_chains_global > n_chains) is
 * APEMOST_HIP_ERR_UNSUPPORTED: the solve needs every chain on one device. */
typedef struct {
    uint64_t capacity;        /* kept steps the store has room for; capacity * n_chains <= 2^28 */
    const double *betas;      /* host [n_chains], ladder-major: finite, positive, strictly decreasing in every ladder */
} apemost_hip_mbar_config;
typedef struct {
    uint64_t *n;              /* kept steps stored */
    uint64_t *n_bad;          /* [n_ladders]: stored values that are not finite */
    double *ell;              /* [n][n_chains]: the first n rows of the store */
} apemost_hip_mbar_view;      /* host arrays; any pointer may be NULL (that part is skipped) */
typedef struct {
    double *m, *S0, *S1, *S2, *SS, *G; /* [n_ladders][n_t] */
    double *ell_first;        /* [n_ladders]: l of the range's first sample */
} apemost_hip_mbar_sums;      /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates the store, lnD and the tile-partial scratch.  An mbar fold begun before is dropped once the new
 * configuration has been accepted; a begin that is refused leaves it open as it was.  APEMOST_HIP_ERR_INVALID, before
 * any device work, for a NULL config, betas that are missing or break the rule above, capacity == 0 or capacity *
 * n_chains > 2^28 (the message names the largest capacity that fits). */
int apemost_hip_mbar_begin(apemost_hip_sampler *s, const apemost_hip_mbar_config *cfg);
/* appends l of the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2]) to the store.
 * Asynchronous and queued like apemost_hip_evidence_accumulate.  APEMOST_HIP_ERR_INVALID, before any device work,
 * without mbar_begin, with thin == 0, or when the kept steps go beyond capacity. */
int apemost_hip_mbar_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                uint64_t thin);
/* copies the store out (synchronises with the accumulates issued so far) */
int apemost_hip_mbar_get(apemost_hip_sampler *s, const apemost_hip_mbar_view *v);
/* loads a view saved by mbar_get into a fold begun with the same betas; APEMOST_HIP_ERR_INVALID when n > capacity */
int apemost_hip_mbar_set(apemost_hip_sampler *s, const apemost_hip_mbar_view *v);
/* frees the store (apemost_hip_destroy does too) */
int apemost_hip_mbar_end(apemost_hip_sampler *s);
/* n_iter updates g <- G(g) over the kept steps [t0, t0 + t_count); g_inout [n_chains] holds g before and after,
 * g_prev_out [n_chains] (may be NULL) g before the last update.  Synchronises.  APEMOST_HIP_ERR_INVALID for an empty
 * range, a range past n, n_iter < 1, or a ladder with stored non-finite values (the message gives the count). */
int apemost_hip_mbar_iterate(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, uint32_t n_iter, double *g_inout,
                             double *g_prev_out);
/* for the targets betas_t [n_t], each finite and >= 0 (0 included), shared by all ladders, and the free energies g
 * [n_chains]: m_t = max_n x_tn with x_tn = beta_t l_n - lnD_n, and with e = exp(x_tn - m_t), d = l_n - ell_first the
 * sums S0 = sum e, S1 = sum e d, S2 = sum (e d) d, SS = sum e e, and G = m + log(S0) with the device's log: ln Z(beta_t)
 * on the scale of g, and at a sampled beta the g the next mbar_iterate would give that chain, on the bits.
 * E[l] = ell_first + S1 / S0, Var[l] = S2 / S0 - (S1 / S0)^2, Kish's effective sample size S0^2 / SS.  The refusals of
 * mbar_iterate. */
int apemost_hip_mbar_evaluate(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g,
                              const double *betas_t, int32_t n_t, const apemost_hip_mbar_sums *out);
/* host_out [t_count][n_chains] = beta_t l_n - lnD_n - G_t (two rounded differences): the log weights, normalised per
 * ladder, with which a caller reweights whatever it kept of those rows to beta_t.  The refusals of mbar_iterate. */
int apemost_hip_mbar_log_weights(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g, double beta_t,
                                 double *host_out);

/* ---- on-device reweighted posteriors: moments and marginals at any beta from every chain --------
 * The posterior's moments and marginal histograms at any beta_t >= 0, sampled or not, estimated from EVERY kept step of
 * EVERY chain with the MBAR weights, without a sample dump.  The fold is attached to an open mbar fold with nothing
 * stored yet and keeps, for n_cols chosen columns of the sample row, the value of every kept step of every chain:
 * x[n_cols][capacity][n_chains], the capacity being the mbar fold's; n_cols * capacity * n_chains <= 2^30 values.
 * Per ladder over the kept steps [t0, t0 + t_count), N = t_count * K samples in mbar's stored order, for a target
 * beta_t: lnD_n, x_tn = beta_t l_n - lnD_n, the exact maximum m_t and e_n = exp(x_tn - m_t) are mbar_evaluate's.  With
 * origin_a the column's value at the range's first sample of the ladder and d_a = x_a,n - origin_a:
 *   S0 = sum e,  SS = sum e e,  S1[a] = sum e d_a,  cross[a][b] = sum (e d_a) d_b  (a <= b)
 * in mbar's fixed order (tiles of 4096, 64 lane partials, the adjacent-pairs tree, tiles in order; csrc/pt_reweight.h),
 * so m, S0 and SS equal mbar_evaluate's on the bits.  E[x_a] = origin_a + S1[a] / S0, Cov[x_a, x_b] = cross[a][b] / S0
 * - (S1[a] / S0)(S1[b] / S0), Kish's effective sample size S0^2 / SS.
 * Histograms: the run summary's bins over [lo[a], hi[a]] (values outside, NaN included, are not counted), weighted by
 * the fixed-point integers q_n = (uint64) rint(ldexp(e_n, shift)), shift = 63 - bit_length(N): exact scaling, one
 * rounding, sum q < 2^63, integer sums that do not depend on the grid or the order.  A bin differs from 2^shift sum e
 * by at most N_bin / 2; relative to the normalisation the error is at most N 2^-(shift+1) / ESS.
 * The two stores advance by separate calls: mbar_accumulate and reweight_accumulate (mbar_set and reweight_set) of
 * the same rows; evaluate and weights refuse with "stores out of step" while the kept counts differ.  mbar_begin and
 * mbar_end drop an attached reweight fold.  Whole ladders, ladder batches and ragged batches; every model (the fold
 * evaluates none); a shard of a sharded ladder is APEMOST_HIP_ERR_UNSUPPORTED. */
typedef struct {
    int32_t n_cols;           /* 1 .. 16 */
    const int32_t *cols;      /* host [n_cols]: columns of the row, 0 .. n_par+1, strictly increasing */
    int32_t nbins;            /* 0: no histograms; else 1 .. 4096 */
    const double *lo, *hi;    /* host [n_cols]: the histogram ranges (nbins > 0) */
} apemost_hip_reweight_config;
typedef struct {
    uint64_t *n;              /* kept steps stored */
    uint64_t *n_bad;          /* [n_ladders][n_cols]: stored values that are not finite */
    double *x;                /* [n_cols][n][n_chains]: the first n rows of every column */
} apemost_hip_reweight_view;  /* host arrays; any pointer may be NULL (that part is skipped) */
typedef struct {
    double *m, *S0, *SS;      /* [n_ladders][n_t] */
    double *origin;           /* [n_ladders][n_cols] */
    double *S1;               /* [n_ladders][n_t][n_cols] */
    double *cross;            /* [n_ladders][n_t][n_cols (n_cols + 1) / 2]: the upper triangle, row-major */
    int32_t *shift;           /* [1] */
    uint64_t *hist;           /* [n_ladders][n_t][n_cols][nbins] */
    uint64_t *q_total;        /* [n_ladders][n_t]: sum of q over all samples of the range */
} apemost_hip_reweight_sums;  /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates the columns' store and the scratch.  Needs an open mbar fold with nothing stored.  A reweight fold begun
 * before is dropped once the new configuration has been accepted.  APEMOST_HIP_ERR_INVALID, before any device work and
 * naming the offender, for a NULL config, columns out of range or not increasing, nbins outside [0, 4096], a bad
 * range, or a store above 2^30 values (the message gives the largest n_cols that fits). */
int apemost_hip_reweight_begin(apemost_hip_sampler *s, const apemost_hip_reweight_config *cfg);
/* appends the columns of the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2]).
 * Asynchronous and queued like apemost_hip_mbar_accumulate; refused beyond the mbar fold's capacity. */
int apemost_hip_reweight_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                    uint64_t thin);
/* copies the store out (synchronises with the accumulates issued so far) */
int apemost_hip_reweight_get(apemost_hip_sampler *s, const apemost_hip_reweight_view *v);
/* loads a view saved by reweight_get (after mbar_set: the resumed run); APEMOST_HIP_ERR_INVALID when n > capacity */
int apemost_hip_reweight_set(apemost_hip_sampler *s, const apemost_hip_reweight_view *v);
/* frees the store (mbar_begin, mbar_end and apemost_hip_destroy do too) */
int apemost_hip_reweight_end(apemost_hip_sampler *s);
/* the sums above for the targets betas_t [n_t], 1 <= n_t <= 64, each finite and >= 0, shared by all ladders, and the
 * free energies g [n_chains].  n_ladders * n_t * n_cols * nbins <= 2^24.  The refusals of mbar_iterate, "stores out of
 * step", and a non-zero n_bad of a column (the message gives the count).  Synchronises. */
int apemost_hip_reweight_evaluate(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g,
                                  const double *betas_t, int32_t n_t, const apemost_hip_reweight_sums *out);
/* host_e, host_q [t_count][n_chains] (either may be NULL): e_n and q_n of one target, those the evaluation uses, with
 * which a caller reweights rows of its own.  The refusals of reweight_evaluate. */
int apemost_hip_reweight_weights(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g, double beta_t,
                                 double *host_e, uint64_t *host_q);

/* Resampling: n_draws equally weighted draws per ladder from the weighted sample of one target, for whatever the sums
 * above do not answer (a corner plot, a credible region, the reference's own histogram and peak tools).  With q_n the
 * integers above, sample n = 0 .. N-1 in mbar's stored order, M = n_draws and the caller's u (csrc/pt_resample.h):
 *   C_n = q_0 + ... + q_n                          (uint64; Q = C_{N-1} = q_total < 2^63)
 *   a = Q div M,  b = Q mod M,  o = mulhi64(u, a)  (the high 64 bits of the 128-bit product; 0 <= o < a)
 *   p_m = m a + (m b) div M + o,  m = 0 .. M-1     (non-decreasing, below Q)
 *   draw m is the smallest n with C_n > p_m:
 * systematic resampling with an integer offset, in 64-bit integers alone (Q >= 2^shift >= 2^34 because the largest e
 * is 1, so a >= 2^10; m b < 2^48).  A sample with q_n = 0 is never drawn; sample n is drawn floor(M q_n / Q) or
 * ceil(M q_n / Q) times.  No floating point and no atomics: the same index on any grid.  The draws come out in stored
 * order (time-major, the chain fastest): they are equally weighted, not exchangeable in order. */
typedef struct {
    uint32_t *index;    /* [n_ladders][n_draws]: sample n of the ladder within the range; step t0 + n / K, chain n % K */
    double *x;          /* [n_ladders][n_draws][n_cols] */
    uint64_t *q_total;  /* [n_ladders] */
    int32_t *shift;     /* [1] */
} apemost_hip_reweight_draws;   /* host arrays; any pointer may be NULL (that part is skipped) */
/* the draws of the target beta_t (finite, >= 0) under the free energies g [n_chains]; q_total is reweight_evaluate's
 * for that target on the bits.  APEMOST_HIP_ERR_INVALID, before any device work and naming the offender, for a NULL g
 * or out, n_draws outside [1, 2^24] and n_ladders * n_draws * n_cols above 2^26; then the refusals of
 * reweight_evaluate.  The first call of a fold allocates 8 bytes per stored sample, which the fold's end frees.
 * Synchronises. */
int apemost_hip_reweight_resample(apemost_hip_sampler *s, uint64_t t0, uint64_t t_count, const double *g,
                                  double beta_t, uint32_t n_draws, uint64_t u,
                                  const apemost_hip_reweight_draws *out);

/* ---- on-device autocorrelation: lag sums, integrated times, effective sample size ---------------
 * How many independent samples a run holds: what the autocorrelation function of sample columns needs, accumulated
 * from the sample rows while they are still on the device.  A series is one (kept chain, column) pair, series
 * s = k * n_cols + c for kept chain k and listed column c; its samples are x_0, x_1, ... in kept order and
 * d_t = x_t - origin.  With L = max_lag, per series:
 *   n               kept samples so far, the same for every series;
 *   origin[s]       x_0 of the first sample ever accumulated (0 before there is one);
 *   sum[s]          the sequential sum of d_t;
 *   lag[s][l]       for l = 0 .. L-1 the sequential sum, in ascending t, of d_t * d_{t-l} over the pairs with t >= l
 *                   only (the product rounded to fp64 and then added);
 *   head[s][j]      for j = 0 .. L-2: d_j, and 0 where j >= n;
 *   tail[s][j]      for j = 0 .. L-2: d of sample n - (L-1) + j, and 0 where that index is negative.  It is the carry
 *                   the fold needs across calls.
 * Head and tail let the host remove the mean exactly: with m = sum / n,
 *   acov_l = (lag_l - m (sum - sum_{j<l} head_j) - m (sum - sum of the last l tail entries) + (n - l) m^2) / n.
 * Lags count kept samples: with thin they are in units of thin steps.
 * No filter: a non-finite value makes the sums of its own series non-finite and changes no other series.
 * Every quantity is one thread's chain of operations in sample order, its state carried in device memory between
 * calls: all of them are bitwise equal to a sequential host loop whatever the boundaries of the accumulate calls are,
 * pieces shorter than L-1 and the ramp-up while n < L included.
 * Ladder batches: chains are local chain indices of the grid, ladder-major.  Sharded ladders: begin on the shard that
 * holds the chain. */
typedef struct {
    int32_t n_keep;           /* 1 .. n_chains */
    const int32_t *chains;    /* host [n_keep], local chain indices, strictly increasing */
    int32_t max_lag;          /* L: 1 .. 4096 */
    int32_t n_cols;           /* 1 .. n_par+2; ignored when cols is NULL */
    const int32_t *cols;      /* host [n_cols], column indices in 0 .. n_par+1, strictly increasing; NULL: the n_par
                                 parameters and column n_par+1 (prob - prior), n_par+1 columns */
} apemost_hip_autocorr_config;
typedef struct {
    uint64_t *n;              /* kept samples */
    double *origin, *sum;     /* [n_series] */
    double *lag;              /* [n_series][L] */
    double *head, *tail;      /* [n_series][L-1] */
} apemost_hip_autocorr_view;  /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates and zeroes the accumulator, and device scratch for one staged piece: 2^20 / n_series kept steps, at least
 * 256 and at most 65536, behind L-1 history slots per series.  A fold begun before is dropped once the new
 * configuration has been accepted; a begin that is refused leaves it open and accumulating as it was.
 * APEMOST_HIP_ERR_INVALID, before any device work, for a NULL config, n_keep or an index out of range, indices not
 * strictly increasing, max_lag outside 1 .. 4096, more than 65535 series, or n_series * L above 2^24 lag sums
 * (128 MiB). */
int apemost_hip_autocorr_begin(apemost_hip_sampler *s, const apemost_hip_autocorr_config *cfg);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2], the rows of the
 * launches issued so far) into the accumulator.  Asynchronous and queued like apemost_hip_summary_accumulate, on the
 * stream of apemost_hip_samples_read_async: the round kernels never wait for it, and apemost_hip_samples_wait (or
 * autocorr_get) must have returned before d_samples is written again.  APEMOST_HIP_ERR_INVALID, before any device
 * work, without autocorr_begin or with thin == 0. */
int apemost_hip_autocorr_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                    uint64_t thin);
/* copies the accumulator out (synchronises with the accumulates issued so far) */
int apemost_hip_autocorr_get(apemost_hip_sampler *s, const apemost_hip_autocorr_view *v);
/* loads a view saved by autocorr_get into a fold begun with the same configuration (a resumed run); with n > 0 the
 * next sample replaces neither the origin nor the head. */
int apemost_hip_autocorr_set(apemost_hip_sampler *s, const apemost_hip_autocorr_view *v);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_autocorr_end(apemost_hip_sampler *s);

/* ---- on-device posterior predictive: the model curve's mean, bands and best fit ------------------
 * The fitted model itself: the curve of the built-in likelihood (simplesin and sine3: m(x); pulse and pulse_vrot: the
 * Lorentzian sum y(nu); the operation order is specified at the head of apemost_amd/csrc/pt_predict.h) evaluated at
 * n_x abscissae for every kept sample of the kept chains, while the sample rows are still on the device.  A series is
 * one (kept chain k, abscissa i) pair, series s = k * n_x + i, with the samples v_t = curve(parameters of kept sample
 * t of chain k, x_i).  Per series:
 *   n               kept samples so far, the same for every series;
 *   origin[s]       v_0 of the first sample ever accumulated (0 before there is one);
 *   sum[s], sq[s]   with d = v - origin the sequential sums of d and of d * d (the product rounded to fp64, then added);
 *   vmin[s], vmax[s]  from +inf and -inf by strict < and >: a NaN never enters;
 *   hist[s][b]      nbins counts over one range [lo, hi] shared by all series, on the run summary's edges (GSL's uniform
 *                   edges, the top one widened by (hi-lo)/10000, bin b = [e[b], e[b+1]), found by bisection); values
 *                   outside the range and NaN are not counted.  Medians and credible bands come from these counts.
 * and per kept chain the best sample:
 *   best_prob[k]    the largest column n_par (prob) over the kept samples, from -inf by strict >: the first occurrence
 *                   wins, a NaN (or -inf) never does;
 *   best_params[k][n_par]  the parameter row of that sample;  best_n[k]  its 1-based kept index, 0 before there is one.
 * No filter: a non-finite parameter makes the sums of its own chain's series non-finite and changes nothing else.
 * Every quantity is one thread's chain of operations in sample order, its state carried in device memory between
 * calls: all of them are bitwise equal to a sequential host loop whatever the boundaries of the accumulate calls are.
 * Ladder batches: chains are local chain indices of the grid, ladder-major; with x = NULL a kept chain takes the data
 * of its own ladder.  Sharded ladders: begin on the shard that holds the chain.
 * APEMOST_MODEL_USER: the curve is the device model's optional hook apemost_user_curve(ctx, i)
 * (include/apemost_device_model.h), and an abscissa is a whole row of n_cols values, because that is what a hook reads:
 *   x == NULL   the rows are all n_cols columns of the sampler's data as they are at begin (of the kept chain's own
 *               ladder in a batch), n_x = n_data;
 *   x != NULL   host [n_x][n_cols], row-major like m->data, every value finite; uploaded column-major as the ctx's data
 *               with ctx->n_data = n_x.  The same holds for apemost_hip_predict_curve, which needs no begin.
 * set / get / end, a resumed run, the limits and every APEMOST_HIP_ERR_INVALID rule are the built-in models'.  A device
 * model without the hook has no curve: every apemost_hip_predict_* entry point returns APEMOST_HIP_ERR_UNSUPPORTED for
 * such a sampler, with a message that names the hook (apemost_hip_user_hooks asks without failing). */
typedef struct {
    int32_t n_keep;           /* 1 .. n_chains */
    const int32_t *chains;    /* host [n_keep], local chain indices, strictly increasing */
    int32_t n_x;              /* >= 1; ignored when x is NULL */
    const double *x;          /* host [n_x], finite; NULL: column 0 of the sampler's data as it is at begin, n_x = n_data
                               * (APEMOST_MODEL_USER: host [n_x][n_cols]; NULL: the data's rows) */
    int32_t nbins;            /* 0: no histograms; else 1 .. 4096 */
    double lo, hi;            /* the histograms' range: finite, lo < hi (ignored when nbins is 0) */
} apemost_hip_predict_config;
typedef struct {
    uint64_t *n;              /* kept samples */
    double *origin, *sum, *sq, *vmin, *vmax; /* [n_keep][n_x] */
    uint64_t *hist;           /* [n_keep][n_x][nbins] */
    double *best_prob;        /* [n_keep] */
    double *best_params;      /* [n_keep][n_par] */
    uint64_t *best_n;         /* [n_keep] */
} apemost_hip_predict_view;   /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates and initialises the accumulator.  A fold begun before is dropped once the new configuration has been
 * accepted; a begin that is refused leaves it open and accumulating as it was.  APEMOST_HIP_ERR_INVALID, before any
 * device work, for a NULL config, n_keep or an index out of range, indices not strictly increasing, n_x < 1, a
 * non-finite x, nbins outside 0 .. 4096, a range that is not finite with lo < hi, n_keep * n_x above 2^20 series, or
 * n_keep * n_x * nbins above 2^26 counts (512 MiB). */
int apemost_hip_predict_begin(apemost_hip_sampler *s, const apemost_hip_predict_config *cfg);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2], the rows of the
 * launches issued so far) into the accumulator, in launches of at most 8192 kept steps.  Asynchronous and queued like
 * apemost_hip_autocorr_accumulate, on the stream of apemost_hip_samples_read_async.  APEMOST_HIP_ERR_INVALID, before
 * any device work, without predict_begin or with thin == 0. */
int apemost_hip_predict_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                   uint64_t thin);
/* copies the accumulator out (synchronises with the accumulates issued so far) */
int apemost_hip_predict_get(apemost_hip_sampler *s, const apemost_hip_predict_view *v);
/* loads a view saved by predict_get into a fold begun with the same configuration (a resumed run); with n > 0 the
 * next sample replaces neither the origins nor the best sample (unless its prob is larger) */
int apemost_hip_predict_set(apemost_hip_sampler *s, const apemost_hip_predict_view *v);
/* len[n_keep]: the abscissae kept chain k of the open fold really has -- n_x, except at the data's abscissae
 * (x == NULL) of a ragged batch (apemost_hip_create_batch_ragged), where it is the n_data of the chain's ladder and
 * n_x the largest of them.  Entries i >= len[k] of every [n_keep][n_x] array are never written by the fold: after
 * predict_get they hold their initial values (origin, sum, sq 0, vmin +inf, vmax -inf, hist 0). */
int apemost_hip_predict_lengths(apemost_hip_sampler *s, int32_t *len);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_predict_end(apemost_hip_sampler *s);
/* out[r][i] = the same curve for the caller's parameter rows: params host [n][n_par], x host [n_x] (NULL: column 0 of
 * the sampler's data -- of ladder 0 in a batch --, n_x = n_data, on a ragged batch n_data[0]), out host [n][n_x].  APEMOST_MODEL_USER: x host
 * [n_x][n_cols], finite (NULL: the data's rows).  Synchronous; needs no predict_begin.  APEMOST_HIP_ERR_INVALID for
 * n < 1, NULL params or out, n_x < 1 or n * n_x above 2^26. */
int apemost_hip_predict_curve(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x, const double *x,
                              double *out);

/* ---- on-device pointwise log-likelihood: WAIC, leave-one-out and DIC without dumps ------------------
 * The term l_i(theta) of every datum (x_i, y_i) -- columns 0 and 1 of the sampler's data as they are at begin -- under
 * every kept sample of the kept chains, while the sample rows are still on the device.  No sample dump holds it: a row
 * carries only the sum over the data.  With v the model curve of apemost_hip_predict_* at x_i (the operation order is
 * specified at the head of apemost_amd/csrc/pt_pointwise.h):
 *   simplesin, sine3    l = ((v - y_i) * (v - y_i)) * c with c = 1.0 / ((-2.0 * sigma) * sigma) from the sampler's sigma;
 *                       the constant -ln(sigma sqrt(2 pi)) is left out, as the reference's likelihood leaves it out: it
 *                       shifts every criterion by the same amount per datum;
 *   pulse, pulse_vrot   l = -(log(v) + y_i / v); the parameter-1 offset of the reference's sum is not a datum's term.
 * A series is one (kept chain k, datum i) pair, series s = k * n_data + i.  Per series:
 *   n                      kept samples so far, the same for every series;
 *   origin[s]              l of the first sample ever accumulated (0 before there is one);
 *   sum[s], sq[s]          with d = l - origin the sequential sums of d and of d * d (the product rounded, then added);
 *   m_up[s], S_up[s]       the running log-sum-exp of l, the recurrence of the evidence fold: ln mean exp(l) =
 *                          m_up + ln(S_up / n), the pointwise log predictive density;
 *   m_dn[s], S_dn[s], S2_dn[s]   the running log-sum-exp of -l and the running sum of the squares of the same
 *                          exponentials: -(m_dn + ln(S_dn / n)) is the importance-sampling leave-one-out density and
 *                          S_dn^2 / S2_dn the effective sample size of its weights.
 * and per kept chain  par_origin[k][p], par_sum[k][p]: the first sample's parameters and the sequential sums of the
 * parameters about them (the posterior mean that DIC needs).
 * No filter: a non-finite or non-positive v gives what IEEE arithmetic gives and touches its own chain's series only.
 * Every quantity is one thread's chain of operations in sample order, its state carried in device memory between
 * calls: all of them equal a sequential host loop whatever the boundaries of the accumulate calls are.
 * Ladder batches: chains are local chain indices of the grid, ladder-major; a kept chain takes the data of its own
 * ladder.  Sharded ladders: begin on the shard that holds the chain.
 * APEMOST_MODEL_USER: the term is the device model's optional hook apemost_user_pointwise(ctx, i)
 * (include/apemost_device_model.h) and a datum is a whole row: all n_cols columns of the sampler's data as they are at
 * begin (of the kept chain's own ladder in a batch), copied, so that a later set_data does not move them.
 * apemost_hip_pointwise_loglike[_ladder] read the data as it is at the call and need no begin.  set / get / end, a
 * resumed run, the limits (n_keep * n_data <= 2^20) and every APEMOST_HIP_ERR_INVALID rule are the built-in models'.
 * The engine cannot check the hook against term() and finish(): it is taken on trust.  A device model without the hook
 * has no datum's term (term() is a lane's share of a sum): every apemost_hip_pointwise_* entry point returns
 * APEMOST_HIP_ERR_UNSUPPORTED for such a sampler, with a message that names the hook. */
typedef struct {
    int32_t n_keep;           /* 1 .. n_chains */
    const int32_t *chains;    /* host [n_keep], local chain indices, strictly increasing */
} apemost_hip_pointwise_config;
typedef struct {
    uint64_t *n;              /* kept samples */
    double *origin, *sum, *sq, *m_up, *S_up, *m_dn, *S_dn, *S2_dn; /* [n_keep][n_data] */
    double *par_origin, *par_sum; /* [n_keep][n_par] */
} apemost_hip_pointwise_view; /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates and initialises the accumulator.  A fold begun before is dropped once the new configuration has been
 * accepted; a begin that is refused leaves it open and accumulating as it was.  APEMOST_HIP_ERR_INVALID, before any
 * device work, for a NULL config, n_keep or an index out of range, indices not strictly increasing, n_keep * n_data
 * above 2^20 series, or more than 512 parameters. */
int apemost_hip_pointwise_begin(apemost_hip_sampler *s, const apemost_hip_pointwise_config *cfg);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2], the rows of the
 * launches issued so far) into the accumulator, in launches of at most 8192 kept steps.  Asynchronous and queued like
 * apemost_hip_predict_accumulate, on the stream of apemost_hip_samples_read_async.  APEMOST_HIP_ERR_INVALID, before
 * any device work, without pointwise_begin or with thin == 0. */
int apemost_hip_pointwise_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                     uint64_t thin);
/* copies the accumulator out (synchronises with the accumulates issued so far) */
int apemost_hip_pointwise_get(apemost_hip_sampler *s, const apemost_hip_pointwise_view *v);
/* loads a view saved by pointwise_get into a fold begun with the same configuration (a resumed run); with n > 0 the
 * next sample replaces no origin */
int apemost_hip_pointwise_set(apemost_hip_sampler *s, const apemost_hip_pointwise_view *v);
/* len[n_keep]: the data kept chain k of the open fold really has.  The fold's arrays are [n_keep][n_data] with n_data
 * the longest data among the kept chains' ladders: the sampler's n_data, except on a ragged batch
 * (apemost_hip_create_batch_ragged).  Entries i >= len[k] are never written by the fold: after pointwise_get they hold
 * their initial values, 0 in all eight words. */
int apemost_hip_pointwise_lengths(apemost_hip_sampler *s, int32_t *len);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_pointwise_end(apemost_hip_sampler *s);
/* out[r][i] = l_i(params[r]), the same term for the caller's parameter rows: params host [n][n_par], out host
 * [n][n_data], over the sampler's data (of ladder 0 in a batch).  Synchronous; needs no pointwise_begin.
 * APEMOST_HIP_ERR_INVALID for n < 1, NULL params or out, or n * n_data above 2^26. */
int apemost_hip_pointwise_loglike(apemost_hip_sampler *s, int32_t n, const double *params, double *out);
/* the same over the data of ladder `ladder` of a batch (0 for an ordinary sampler); APEMOST_HIP_ERR_INVALID also for a
 * ladder out of range */
int apemost_hip_pointwise_loglike_ladder(apemost_hip_sampler *s, int32_t ladder, int32_t n, const double *params,
                                         double *out);

/* ---- the pointwise fold at the caller's data: held-out log predictive density, K-fold cross-validation ----
 * apemost_hip_pointwise_begin_at opens the same fold over data the sampler was not fitted to: kept chain k is scored on
 * the n_at[k] data (x, y) the caller hands in, packed kept chain after kept chain, instead of on columns 0 and 1 of its
 * own ladder.  After the call the fold is an ordinary pointwise fold whose series are (kept chain k, caller's datum i):
 * accumulate, get, set, lengths and end, the eight words, the limits (n_keep * max n_at <= 2^20 series, at most 512
 * parameters) and every rule are those above, and n_data of the fold is max n_at.  Where the lengths differ, the fold is
 * that of a ragged batch: series past n_at[k] keep their initial zeros and apemost_hip_pointwise_lengths reports n_at.
 * x and y are copied at begin; nothing of the sampler's data is read afterwards, and a later set_data moves nothing.
 *   m_up + ln(S_up / n)   is the log predictive density of held-out datum i under kept chain k's posterior, the elpd_i
 *                         of K-fold cross-validation where kept chain k was fitted without datum i;
 *   the _dn words         are still folded (the kernel is the same) and have no cross-validation meaning: leaving out a
 *                         datum that was never in is no estimate of anything.  apemost_amd/kfold.py ignores them.
 * The typical use is a ragged ladder batch (apemost_hip_create_batch_ragged) whose ladder b was fitted to the training
 * set of fold b, with chain 0 of every ladder (beta = 1) kept and scored on the block that ladder b left out
 * (apemost_amd/kfold.py).
 * The tail (apemost_hip_pointwise_tail_begin) keeps its own rule: allowed where all n_at are equal, refused where they
 * differ.  APEMOST_MODEL_USER: APEMOST_HIP_ERR_UNSUPPORTED -- a user model's datum is a whole row and it runs in no
 * batch; the hook on held-out rows is a follow-up.
 *
 * joint = 1: also the joint predictive density of every kept chain's block (apemost_amd/csrc/pt_pointwise_joint.h, new
 * kernels behind each piece of the fold on the same stream; the fold's own words are bitwise what they are without).
 * Per kept sample t of kept chain k, J_t = the sum of the block's L = n_at[k] terms in a fixed order: lane partial
 * p[j], j = 0 .. 63, starts at +0.0 and adds l_i for i = j, j + 64, ... < L ascending; the 64 partials are combined by
 * the adjacent-pairs tree p = p[0::2] + p[1::2] taken six times.  J_t depends on L and the terms and on nothing else.
 * Five words per kept chain, each a sequential loop in sample order whatever the calls' boundaries:
 *   origin[k]             J of the first sample ever;
 *   sum[k], sq[k]         with d = J - origin the sums of d and of d * d (the product rounded, then added);
 *   m[k], S[k]            the running log-sum-exp of J, the recurrence of the evidence fold:
 *                         ln mean_t exp(J_t) = m + ln(S / n) is the log predictive density of the block as a whole.
 * It is not the sum of the block's pointwise densities.  No filter: a non-finite term does what IEEE arithmetic does,
 * to its own kept chain's words only.  Device memory: 8192 doubles (64 KiB) of scratch per kept chain. */
typedef struct {
    const int32_t *n_at;  /* host [n_keep]: data that kept chain k is scored on, each >= 1 */
    const double *x, *y;  /* host, packed kept chain after kept chain: n_at[0] values, then n_at[1], ... */
    int32_t joint;        /* 1: also fold the joint predictive of each kept chain's block */
} apemost_hip_pointwise_at;
typedef struct {
    uint64_t *n;          /* kept samples: the fold's */
    double *origin, *sum, *sq, *m, *S; /* [n_keep] */
} apemost_hip_pointwise_joint_view; /* host arrays; any pointer may be NULL (that part is skipped) */
/* apemost_hip_pointwise_begin with the caller's data.  A fold begun before (and its tail and joint state) is dropped
 * once the new configuration has been accepted; a begin that is refused leaves it as it was.  APEMOST_HIP_ERR_INVALID,
 * before any device work and with a message that names the argument: what pointwise_begin refuses, a NULL at, a NULL
 * n_at, x or y, n_at[k] < 1, joint other than 0 or 1. */
int apemost_hip_pointwise_begin_at(apemost_hip_sampler *s, const apemost_hip_pointwise_config *cfg,
                                   const apemost_hip_pointwise_at *at);
/* copies the joint state out (synchronises with the accumulates issued so far) / loads it into a fold begun with the
 * same configuration (a resumed run).  After a pointwise_set that loaded samples, apemost_hip_pointwise_accumulate returns
 * APEMOST_HIP_ERR_INVALID until pointwise_joint_set has loaded the joint state of those samples; a view whose n differs
 * from the fold's is refused.  APEMOST_HIP_ERR_INVALID for a fold without joint = 1.  pointwise_begin, pointwise_begin_at
 * and pointwise_end drop the joint state. */
int apemost_hip_pointwise_joint_get(apemost_hip_sampler *s, const apemost_hip_pointwise_joint_view *v);
int apemost_hip_pointwise_joint_set(apemost_hip_sampler *s, const apemost_hip_pointwise_joint_view *v);
/* out[r][i] = l_i(params[r]) over the caller's data: params host [n][n_par], x and y host [n_x], out host [n][n_x]: the
 * term a fold begun with pointwise_begin_at folds, by the same device function.  Synchronous; needs no fold and reads
 * nothing of the sampler's data.  APEMOST_HIP_ERR_INVALID for n < 1, n_x < 1, a NULL array, or n * n_x above 2^26;
 * APEMOST_HIP_ERR_UNSUPPORTED for APEMOST_MODEL_USER. */
int apemost_hip_pointwise_loglike_at(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x,
                                     const double *x, const double *y, double *out);

/* ---- the tail of a pointwise fold (pt_pointwise_tail.h): what Pareto-smoothed leave-one-out needs ----
 * Per series s = (kept chain k, datum i) the `capacity` largest values of x = -l over the kept samples, exactly, where l
 * is the fold's own term of the same row (the same device function, so the same bits).  The order is the total order of
 * the bit patterns in which -0 lies below +0 and -inf and +inf are the ends; a NaN is never stored.  After any number of
 * accumulate calls
 *   count[s]              = min(capacity, samples so far whose term is not NaN),
 *   values[s][0 .. count) = the count[s] largest x, descending.
 * A selection under a total order does not depend on how the kept samples were cut into calls: the same kept samples
 * give the same bits.  With m_dn and S_dn of the fold this gives PSIS-LOO and the Pareto k of every datum
 * (apemost_amd/psis.py; the fit is not restated in C): the M + 1 largest log weights, M = ceil(min(0.2 n, 3 sqrt(n))),
 * so capacity = M + 1 (at most 4096: runs above 1.86e6 kept samples get a shorter tail).
 *
 * The tail attaches to an open fold: apemost_hip_pointwise_accumulate then launches two more kernels per piece behind the
 * fold's, on the same stream over the same kept steps; the fold's own results are bitwise what they are without a
 * tail, and a sampler without a tail launches nothing new.  pointwise_begin and pointwise_end drop the tail,
 * pointwise_set does not touch it.  Device memory: n_keep * ceil(n_data / 64) * 64 * B doubles with
 * B = 2 * max(1024, capacity rounded up to a power of two). */
typedef struct {
    uint64_t *count; /* [n_keep][n_data] */
    double *values;  /* [n_keep][n_data][capacity], descending; slots >= count are unspecified on get, ignored on set */
} apemost_hip_pointwise_tail_view; /* host arrays, both required */
/* Needs an open pointwise fold that has no sample yet, or whose state apemost_hip_pointwise_set has just loaded (nothing
 * accumulated since): the tail of those samples must then be loaded by pointwise_tail_set, and until it is
 * apemost_hip_pointwise_accumulate returns APEMOST_HIP_ERR_INVALID.  A tail begun before is replaced.
 * APEMOST_HIP_ERR_INVALID, before any device work: no pointwise_begin; a fold that has accumulated samples of its own;
 * capacity outside [2, 4096]; more than 2^28 buffer slots (2 GiB) -- the message names the largest capacity that fits.
 * APEMOST_HIP_ERR_UNSUPPORTED where pointwise_begin gives it.  A refused call leaves the fold, and a tail it has, as
 * they were. */
int apemost_hip_pointwise_tail_begin(apemost_hip_sampler *s, int32_t capacity);
/* sorts every series and copies count and values out (synchronises with the accumulates issued so far); the state's
 * selection is not changed by it.  APEMOST_HIP_ERR_INVALID without a tail or with a NULL array. */
int apemost_hip_pointwise_tail_get(apemost_hip_sampler *s, const apemost_hip_pointwise_tail_view *v);
/* loads a view saved by pointwise_tail_get into a tail begun with the same capacity on a fold of the same configuration
 * (a resumed run); the values need not be sorted, every threshold is recomputed from them.  APEMOST_HIP_ERR_INVALID, before
 * any device work, for a count above the capacity or a NaN among the first count values of a series. */
int apemost_hip_pointwise_tail_set(apemost_hip_sampler *s, const apemost_hip_pointwise_tail_view *v);
/* *capacity = the capacity of the open fold's tail, 0 where there is none */
int apemost_hip_pointwise_tail_capacity(apemost_hip_sampler *s, int32_t *capacity);

/* ---- on-device derived quantities: column programs folded without dumps ------------------------
 * What the reference's tools/matrix_man.c computes over the text dumps (add, mul, addc, mulc, invm, inva, ... piped
 * into histogram_tool) from rows that stay on the device: the posterior of functions of the parameters -- a splitting
 * f2 - f1, a ratio h2 / h1, A cos 2 pi phi, (prob - prior) / beta.
 *
 * A derived column is a small stack program over one sample row x[0 .. n_par+1], x[n_par] being prob and
 * x[n_par+1] prob - prior.  One int32 per instruction: the low 8 bits are the opcode, the high 24 bits the operand.
 * The programs of all columns are concatenated in code[]; column c is code[start[c] .. start[c+1]); constants are in
 * consts[].  "top" is the last value pushed, "second" the one below it:
 *   COL c      push x[c], 0 <= c <= n_par+1                  CONST k    push consts[k], 0 <= k < n_const
 *   DUP        push top                                       SWAP       top and second change places
 *   exact group -- every result is the correctly rounded IEEE fp64 operation, contraction off, so a program of this
 *   group alone gives the bits numpy gives:
 *   ADD SUB MUL DIV   second (op) top replaces both           NEG ABS    -top, |top| (the sign bit alone changes)
 *   INV        1.0 / top                                      SQRT FLOOR sqrt(top), floor(top)
 *   MIN        second < top ? second : top                    MAX        second > top ? second : top
 *              (literally: with a NaN among the two, or two zeros, the comparison is false and top stays)
 *   library group -- the device library's plain double-precision functions, not promised bit-equal to any host's:
 *   LOG EXP SIN COS   of top                                  ATAN2      atan2(second, top) replaces both
 * Limits: 1 .. 64 columns, 1 .. 256 instructions per column, at most 256 constants, stack depth at most 16; a program
 * leaves exactly one value. */
enum {
    APEMOST_DERIVED_COL = 0, APEMOST_DERIVED_CONST = 1, APEMOST_DERIVED_DUP = 2, APEMOST_DERIVED_SWAP = 3,
    APEMOST_DERIVED_ADD = 4, APEMOST_DERIVED_SUB = 5, APEMOST_DERIVED_MUL = 6, APEMOST_DERIVED_DIV = 7,
    APEMOST_DERIVED_NEG = 8, APEMOST_DERIVED_ABS = 9, APEMOST_DERIVED_INV = 10, APEMOST_DERIVED_SQRT = 11,
    APEMOST_DERIVED_FLOOR = 12, APEMOST_DERIVED_MIN = 13, APEMOST_DERIVED_MAX = 14,
    APEMOST_DERIVED_LOG = 15, APEMOST_DERIVED_EXP = 16, APEMOST_DERIVED_SIN = 17, APEMOST_DERIVED_COS = 18,
    APEMOST_DERIVED_ATAN2 = 19, APEMOST_DERIVED_N_OPCODES = 20
};
#define APEMOST_DERIVED_MAX_COLUMNS 64
#define APEMOST_DERIVED_MAX_CODE 256     /* instructions per column */
#define APEMOST_DERIVED_MAX_CONSTS 256
#define APEMOST_DERIVED_MAX_DEPTH 16
/* Host arithmetic only, no device and no sampler: verifies the n_col programs code[start[c] .. start[c+1]) over rows of
 * n_par + 2 values and n_const constants by abstract execution, and writes the stack depth each program reaches to
 * depth_out[n_col] (NULL: not wanted).  APEMOST_HIP_ERR_INVALID, the message naming column and instruction, for
 * n_col outside 1 .. 64, an empty program or one of more than 256 instructions, an unknown opcode, a COL operand
 * above n_par + 1, a CONST operand >= n_const, n_const outside 0 .. 256, a pop from too short a stack, a depth above
 * 16, or a final depth other than 1. */
int apemost_hip_derived_check(int32_t n_par, int32_t n_col, const int32_t *code, const int32_t *start, int32_t n_const,
                              int32_t *depth_out);

/* The fold.  Accumulated from the sample rows while they are still on the device, per kept chain k and column c, with
 * v the value the column's program gives for a kept row and n the kept samples so far:
 *   hist[k][c][nbins]      counts of v in the run summary's bins over [lo[c], hi[c]] (the edges and the bisection of
 *                          the summary and the joint fold: one device function for all three);
 *   batch[k][c][max_batches + 1]  the batch sums of batch_means_error() with the summary's rule: batch 0 holds
 *                          batch_size - 1 samples, every later one batch_size; slot n_batches is the open batch;
 *   counts[k][q][a][b], origin[k][c], sum[k][c], cross[k][c (c + 1) / 2]  exactly what the joint fold defines, with
 *                          "parameter" read as "column": the joint fold's own kernels run on the staged columns;
 *   nonfinite[k][c]        the count of values that are not finite;
 *   vmin[k][c], vmax[k][c] the least and the greatest v that is not a NaN, +inf and -inf before there is one; of the
 *                          two zeros -0.0 is the lesser (a derived quantity has no prior box: a pilot run reads these
 *                          to choose lo and hi).
 * Nothing is filtered from the sums: a non-finite v makes its column's sums non-finite, as in the joint and summary
 * folds, and nonfinite says why.  Every count is exact and every sum one thread's chain of additions in sample order:
 * the fold equals a sequential host loop over the values apemost_hip_derived_eval returns for the kept rows, bit for
 * bit, whatever the calls, the thinning and the staged pieces are.
 * Sharded ladders and ladder batches: `chains` as for the joint fold. */
typedef struct {
    int32_t n_keep;          /* number of kept chains, 1 .. n_chains; n_keep * n_col <= 65535 */
    const int32_t *chains;   /* host [n_keep]: local chain indices, strictly increasing */
    int32_t n_col;           /* columns, 1 .. 64 */
    const int32_t *code;     /* host [start[n_col]] */
    const int32_t *start;    /* host [n_col + 1], start[0] = 0 */
    int32_t n_const;         /* 0 .. 256 */
    const double *consts;    /* host [n_const] (may be NULL with n_const = 0) */
    int32_t nbins;           /* 1 .. 512 */
    int32_t n_pairs;         /* pairs of columns, with the joint fold's rules (ignored with pairs == NULL: all i < j) */
    const int32_t *pairs;    /* host [n_pairs][2] */
    const double *lo, *hi;   /* host [n_col]: the histogram range of every column, finite, lo < hi, hi - lo finite */
    uint64_t batch_size;     /* >= 1 */
    uint64_t max_batches;    /* batches there is room for; an accumulate that would close more is refused */
    uint64_t stage_steps;    /* kept steps per staged piece, 1 .. 2^18; 0: about 4 Mi values over all columns, as the
                                joint fold stages */
} apemost_hip_derived_config;
typedef struct {
    uint64_t *n;             /* kept samples */
    uint64_t *hist;          /* [n_keep][n_col][nbins] */
    double *batch;           /* [n_keep][n_col][max_batches + 1] */
    uint64_t *n_batches;     /* batches closed (get writes it; set checks it against n where both are given) */
    uint64_t *counts;        /* [n_keep][n_pairs][nbins][nbins] */
    double *origin, *sum;    /* [n_keep][n_col] */
    double *cross;           /* [n_keep][n_col (n_col + 1) / 2], upper triangle row-major */
    uint64_t *nonfinite;     /* [n_keep][n_col] */
    double *vmin, *vmax;     /* [n_keep][n_col] */
} apemost_hip_derived_view;  /* host arrays; any pointer may be NULL (that part is skipped) */

/* checks the programs with apemost_hip_derived_check and everything else before any device work, then allocates and
 * zeroes the accumulator and the scratch of one staged piece (10 bytes per value).  A fold begun before is dropped once
 * the new configuration has been accepted; a begin that is refused leaves it open and accumulating as it was. */
int apemost_hip_derived_begin(apemost_hip_sampler *s, const apemost_hip_derived_config *cfg);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2]); asynchronous and
 * queued like apemost_hip_joint_accumulate.  APEMOST_HIP_ERR_INVALID without derived_begin, with thin == 0, or where
 * the call would close more than max_batches batches (nothing is accumulated then). */
int apemost_hip_derived_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                   uint64_t thin);
/* copies the accumulator out (synchronises with the accumulates issued so far) */
int apemost_hip_derived_get(apemost_hip_sampler *s, const apemost_hip_derived_view *v);
/* loads a view saved by derived_get into a fold begun with the same configuration (a resumed run), origin included */
int apemost_hip_derived_set(apemost_hip_sampler *s, const apemost_hip_derived_view *v);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_derived_end(apemost_hip_sampler *s);
/* the open fold's programs on the caller's n rows (HOST rows[n][n_par+2], out[n][n_col]; n * (n_par + 2) and n * n_col
 * at most 2^26), by the device function the fold's gather kernel uses: how a program is checked, and what fixes the
 * fold's meaning.  APEMOST_HIP_ERR_INVALID without derived_begin. */
int apemost_hip_derived_eval(apemost_hip_sampler *s, uint64_t n, const double *rows, double *out);

/* ---- on-device predictive checks: PIT, leave-one-out PIT and discrepancy p-values without dumps ----
 * Is the model adequate for these data?  Per datum (x_i, y_i) -- columns 0 and 1 of the sampler's data as they are at
 * begin -- and kept sample of the kept chains, with v the model curve of apemost_hip_predict_* at x_i and l the term of
 * apemost_hip_pointwise_* (the operation order is specified at the head of apemost_amd/csrc/pt_check.h):
 *   simplesin, sine3    e = (y_i - v) * (1.0 / sigma), the standardised residual;  u = 0.5 * erfc(e * -sqrt(1/2));
 *   pulse, pulse_vrot   e = y_i / v, the ratio, Exp(1) under the model;  u = -expm1(-e);
 * u is the predictive CDF at y_i and a = u - 0.5.  A series is one (kept chain k, datum i) pair, s = k * n_data + i:
 *   n                      kept samples so far;
 *   origin[s], sum[s], sq[s]   e of the first sample and, with d = e - origin, the sequential sums of d and of d * d;
 *   sum_u[s]               the sequential sum of u: pit_i = sum_u / n, the posterior predictive PIT;
 *   m[s], S[s], SU[s]      the running log-sum-exp of -l (the pointwise fold's m_dn and S_dn, bit for bit) and the sum
 *                          of u under the same weights: loo_pit_i = SU / S, the leave-one-out PIT.
 * Per kept sample, three statistics T over the kept chain's L data, every sum in the fixed order of the joint
 * predictive (64 lane partials by i % 64, then the adjacent-pairs tree):
 *   APEMOST_CHECK_FIT      sine: sum e * e (null: chi^2 with L degrees of freedom); pulse: sum e (null: Gamma(L, 1));
 *   APEMOST_CHECK_EXTREME  sine: max |e_i|; pulse: max e_i (a NaN is skipped; -inf where every term is NaN);
 *   APEMOST_CHECK_SERIAL   sum over i >= 1 of a_i * a_{i-1}: null mean 0 and variance (L - 1) / 144; it sees an
 *                          unmodelled periodic signal.
 * Per kept chain and statistic q, at [k][q]: stat_origin, stat_sum, stat_sq (of T, as above), stat_min, stat_max (0
 * before there is a sample; a NaN is skipped), and with n_edges > 0 the exact counts [k][q][n_edges + 2]: slot
 * b = #{j : edges[q][j] <= T}, the last slot counts NaN.  With the edges at the null quantiles j / (n_edges + 1)
 * (apemost_hip_check_null_edges) slot b holds the samples whose null CDF lies in [b, b + 1) / (n_edges + 1): the
 * posterior predictive p-value of T to a half-width of 1 / (2 (n_edges + 1)).
 * No filter: a non-finite v gives what IEEE arithmetic gives and touches its own kept chain's words only.  Every word
 * equals a sequential host loop whatever the boundaries of the accumulate calls are.  Ladder batches, ragged batches and
 * sharded ladders: as apemost_hip_pointwise_* (a kept chain takes its own ladder's data; apemost_hip_check_lengths).
 * APEMOST_MODEL_USER: every entry point returns APEMOST_HIP_ERR_UNSUPPORTED, a user hook has no CDF. */
#define APEMOST_CHECK_FIT 0
#define APEMOST_CHECK_EXTREME 1
#define APEMOST_CHECK_SERIAL 2
#define APEMOST_CHECK_STATS 3
#define APEMOST_CHECK_MAX_EDGES 4095
typedef struct {
    uint64_t *n;              /* kept samples */
    double *origin, *sum, *sq, *sum_u, *m, *S, *SU; /* [n_keep][n_data] */
    double *stat_origin, *stat_sum, *stat_sq, *stat_min, *stat_max; /* [n_keep][3] */
    uint64_t *counts;         /* [n_keep][3][n_edges + 2] (nothing where n_edges == 0) */
} apemost_hip_check_view; /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates and initialises the accumulator.  chains: host [n_keep], local chain indices, strictly increasing.
 * edges: host [3][n_edges], per statistic finite and strictly ascending, or NULL with n_edges == 0 (no counts).  A fold
 * begun before is dropped once the new configuration has been accepted; a refused begin leaves it as it was.
 * APEMOST_HIP_ERR_INVALID, before any device work: n_keep or an index out of range, indices not strictly increasing,
 * n_keep * n_data above 2^20 series, more than 512 parameters, n_edges outside [0, 4095], edges NULL with n_edges > 0,
 * an edge that is not finite or not above the one before. */
int apemost_hip_check_begin(apemost_hip_sampler *s, int32_t n_keep, const int32_t *chains, int32_t n_edges,
                            const double *edges);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2]) in launches of at
 * most 8192 kept steps; asynchronous and queued like apemost_hip_pointwise_accumulate.  APEMOST_HIP_ERR_INVALID, before
 * any device work, without check_begin or with thin == 0. */
int apemost_hip_check_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                 uint64_t thin);
/* copies the accumulator out (synchronises with the accumulates issued so far) */
int apemost_hip_check_get(apemost_hip_sampler *s, const apemost_hip_check_view *v);
/* loads a view saved by check_get into a fold begun with the same configuration (a resumed run) */
int apemost_hip_check_set(apemost_hip_sampler *s, const apemost_hip_check_view *v);
/* len[n_keep]: the data kept chain k of the open fold really has (apemost_hip_pointwise_lengths' meaning): series past
 * them are never written and keep their initial zeros */
int apemost_hip_check_lengths(apemost_hip_sampler *s, int32_t *len);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_check_end(apemost_hip_sampler *s);
/* the stated meaning: e, u host [n][n_x] and T host [n][3] of the caller's parameter rows params host [n][n_par] over
 * the caller's data x, y host [n_x], by the fold's own device functions.  Synchronous; needs no fold and reads nothing
 * of the sampler's data.  APEMOST_HIP_ERR_INVALID for n < 1, n_x < 1, a NULL array or n * n_x above 2^26. */
int apemost_hip_check_values(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x, const double *x,
                             const double *y, double *e, double *u, double *T);
/* edges[j], j = 0 .. n_edges - 1: the null quantile (j + 1) / (n_edges + 1) of statistic `stat` of a built-in `model`
 * over n_data data.  A host function: no sampler, no device.
 *   FIT      exact: the regularised incomplete gamma function (series and continued fraction) inverted by bisection;
 *   EXTREME  exact: erf(t / sqrt 2)^L for the sine models (bisection), (1 - exp(-t))^L for the pulse models (closed form);
 *   SERIAL   approximate: the normal quantile with the exact null mean 0 and variance (L - 1) / 144; the statistic is
 *            a sum of L - 1 bounded, 1-dependent terms and the approximation is poor for small L.  For n_data == 1 the
 *            statistic is +0.0 whatever the data and has no null law: the edges are those of n_data == 2, so that a
 *            fold can be begun, and its p-value means nothing.
 * The edges are strictly ascending, SERIAL's symmetric about 0.  APEMOST_HIP_ERR_INVALID for n_data < 1, n_edges
 * outside [1, 4095], an unknown stat or NULL edges; APEMOST_HIP_ERR_UNSUPPORTED for APEMOST_MODEL_USER. */
int apemost_hip_check_null_edges(int32_t model, int32_t stat, int32_t n_data, int32_t n_edges, double *edges);

/* ---- on-device residual periodogram: posterior power on a frequency grid without dumps ----
 * What is left in the residuals, and at which frequency?  For APEMOST_MODEL_SIMPLESIN and APEMOST_MODEL_SINE3.  Per kept
 * sample of the kept chains, with (x_i, y_i) columns 0 and 1 of the kept chain's own ladder's data as they are at begin,
 * r_i = y_i - v the residual of apemost_hip_check_* before its scaling, and nu_j the caller's frequencies (the operation
 * order is specified at the head of apemost_amd/csrc/pt_periodogram.h):
 *   s_ij = sin(2 pi nu_j x_i), c_ij = sin(2 pi (nu_j x_i + 0.25)), the device sine of the likelihoods (NaN out of its range);
 *   C_j = sum_i r_i c_ij, S_j = sum_i r_i s_ij, fused multiply-adds from +0.0 in ascending i;
 *   P_j = ((wcc C) C + (wcs C) S) + (wss S) S with the caller's weights (wcc, wcs, wss) of [k][j]: a quadratic form, whose
 *   normalisation (Lomb-Scargle, Schuster, squared amplitude) is the host's (apemost_amd/periodogram.py).
 * A series is one (kept chain k, frequency j) pair, s = k * n_freq + j:
 *   n                      kept samples so far;
 *   origin[s], sum[s], sq[s]   P of the first sample and, with d = P - origin, the sequential sums of d and of d * d;
 *   pmin[s], pmax[s]       the extremes of P (a NaN is skipped; 0 before there is a sample);
 *   sum_c[s], sum_s[s]     the sequential sums of C and S: the periodogram of the mean residual follows by linearity;
 *   exceed[s]              #{t : P > level[k]} (a NaN P is not counted).
 * Per kept sample the highest peak m = max_j P_j and arg, the first j that holds it (n_freq where no P is above -inf; a
 * NaN never wins); per kept chain k: peak_origin, peak_sum, peak_sq, peak_min, peak_max of m, and peak_counts[k][arg]++
 * over [n_freq + 1] slots.
 * No filter: non-finite values touch their own kept chain's words only.  Every word equals a sequential host loop
 * whatever the boundaries of the accumulate calls are.  Ladder batches, ragged batches and sharded ladders: as
 * apemost_hip_check_* (a kept chain takes its own ladder's data; apemost_hip_periodogram_lengths).
 * APEMOST_MODEL_PULSE, APEMOST_MODEL_PULSE_VROT (their data already are a power spectrum) and APEMOST_MODEL_USER (no
 * residual law here): every entry point returns APEMOST_HIP_ERR_UNSUPPORTED. */
#define APEMOST_PERIODOGRAM_MAX_FREQ (1 << 20)
#define APEMOST_PERIODOGRAM_PIECE 512
typedef struct {
    uint64_t *n;              /* kept samples */
    double *origin, *sum, *sq, *pmin, *pmax, *sum_c, *sum_s; /* [n_keep][n_freq] */
    uint64_t *exceed;         /* [n_keep][n_freq] */
    double *peak_origin, *peak_sum, *peak_sq, *peak_min, *peak_max; /* [n_keep] */
    uint64_t *peak_counts;    /* [n_keep][n_freq + 1] */
} apemost_hip_periodogram_view; /* host arrays; any pointer may be NULL (that part is skipped) */

/* allocates and initialises the accumulator.  chains: host [n_keep], local chain indices, strictly increasing.  freqs:
 * host [n_freq], any doubles but NaN, in any order.  weights: host [n_keep][n_freq][3] = (wcc, wcs, wss); level: host
 * [n_keep].  A fold begun before is dropped once the new configuration has been accepted; a refused begin leaves it as
 * it was.  APEMOST_HIP_ERR_INVALID, before any device work: n_keep or an index out of range, indices not strictly
 * increasing, n_keep * n_data above 2^20 or n_keep * n_freq above 2^24 series, more than 512 parameters, n_freq outside
 * [1, 2^20], a NULL array, a NaN in freqs, weights or level (an infinite weight or level is allowed). */
int apemost_hip_periodogram_begin(apemost_hip_sampler *s, int32_t n_keep, const int32_t *chains, int32_t n_freq,
                                  const double *freqs, const double *weights, const double *level);
/* folds the kept steps skip, skip + thin, ... of d_samples (DEVICE [n_steps][n_chains][n_par+2]) in launches of at
 * most 512 kept steps; asynchronous and queued like apemost_hip_check_accumulate.  APEMOST_HIP_ERR_INVALID, before any
 * device work, without periodogram_begin or with thin == 0. */
int apemost_hip_periodogram_accumulate(apemost_hip_sampler *s, const double *d_samples, uint64_t n_steps, uint64_t skip,
                                       uint64_t thin);
/* copies the accumulator out (synchronises with the accumulates issued so far) */
int apemost_hip_periodogram_get(apemost_hip_sampler *s, const apemost_hip_periodogram_view *v);
/* loads a view saved by periodogram_get into a fold begun with the same configuration (a resumed run) */
int apemost_hip_periodogram_set(apemost_hip_sampler *s, const apemost_hip_periodogram_view *v);
/* len[n_keep]: the data kept chain k of the open fold really has (apemost_hip_check_lengths' meaning) */
int apemost_hip_periodogram_lengths(apemost_hip_sampler *s, int32_t *len);
/* frees the accumulator (apemost_hip_destroy does too) */
int apemost_hip_periodogram_end(apemost_hip_sampler *s);
/* the stated meaning: for the caller's parameter rows params host [n][n_par], data x, y host [n_x], freqs host [n_freq]
 * and weights w host [n_freq][3]: r host [n][n_x], the table c, s host [n_freq][n_x], C, S, P host [n][n_freq], peak host
 * [n] and arg host [n], by the fold's own device functions.  Synchronous; needs no fold and reads nothing of the sampler's
 * data.  APEMOST_HIP_ERR_INVALID for n < 1, n_x < 1, n_freq outside [1, 2^20], a NULL array, or one of n * n_x,
 * n_freq * n_x and n * n_freq above 2^26. */
int apemost_hip_periodogram_values(apemost_hip_sampler *s, int32_t n, const double *params, int32_t n_x, const double *x,
                                   const double *y, int32_t n_freq, const double *freqs, const double *w, double *r,
                                   double *c, double *s_out, double *C, double *S, double *P, double *peak, int32_t *arg);

/* ---- replica flow (APEMOST_HIP_FLAG_TRACK_REPLICAS; the specification is at the flag) ---------
 * Without the flag all three return APEMOST_HIP_ERR_UNSUPPORTED. */
typedef struct {
    uint32_t *replica, *heading;
    uint64_t *n_up, *n_down, *attempts, *round_trips;
} apemost_hip_replica_flow_view; /* host, [n_chains] each (grid-wide, ladder-major); any may be NULL */
/* synchronises like apemost_hip_get_state; after a timed-out hand-off the flow is void like the rest of the launch,
 * and the error is the one get_state gives */
int apemost_hip_replica_flow_get(apemost_hip_sampler *s, const apemost_hip_replica_flow_view *v);
/* a resumed run: every ladder's labels must be a permutation of 0 .. n-1 and headings <= 2 (APEMOST_HIP_ERR_INVALID) */
int apemost_hip_replica_flow_set(apemost_hip_sampler *s, const apemost_hip_replica_flow_view *v);
/* labels to identity, headings and counters to the initial state: after burn-in */
int apemost_hip_replica_flow_reset(apemost_hip_sampler *s);

/* ---- test hooks: device RNG conformance ------------------------------------ */
/* n raw 32-bit outputs of rocRAND philox4x32_10 (seed, subsequence, offset) */
int apemost_hip_rng_raw(int device, uint64_t seed, uint64_t subsequence, uint64_t offset, int32_t n,
                        uint32_t *out);
/* attempts q0..q0+n-1 of the proposal stream (chain, slot) at `tick`, exactly as the
 * step kernel evaluates them: valid[i] says whether the polar pair is usable, and then
 * the N(0,sigma) variate is (sigma*y[i])*s[i]; accept_log_u = ln(uniform) of the accept
 * test of that tick when slot == n_par */
int apemost_hip_rng_attempts(int device, uint64_t seed, uint64_t chain, int32_t slot, uint64_t tick,
                             uint64_t q0, int32_t n, double *y, double *s, int32_t *valid,
                             double *accept_log_u);

/* ---- timing ---------------------------------------------------------------- */
/* HIP events on the sampler's stream: begin/end bracket a region; elapsed ms and
 * the number of round-kernel launches inside it */
int apemost_hip_timer_begin(apemost_hip_sampler *s);
int apemost_hip_timer_end(apemost_hip_sampler *s, float *elapsed_ms, uint64_t *launches);

#ifdef __cplusplus
}
#endif
#endif /* APEMOST_HIP_H */
