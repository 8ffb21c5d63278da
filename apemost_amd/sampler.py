"""HipSampler: host-side mirror of the reference's parallel-tempering operators for one
device shard, implemented entirely by calls into libapemost_hip.so (include/apemost_hip.h).

Method names follow the reference functions they replace:
  run_sampler            src/parallel_tempering.c:347-419
  tempering_interaction  src/parallel_tempering_interaction.c:125-141 (fused into the next round)
  calc_model             apps/<model>.c (device re-implementation)
  markov_chain_calibrate src/markov_chain_calibrate.c:1182-1204
  calibrate_first/rest   src/parallel_tempering.c:78-207
"""
import ctypes as C

import numpy as np

from . import capi
from .state import LadderState

LADDER_CHEBYSHEV_BETA = 0
MODEL_USER = 4   # APEMOST_MODEL_USER (include/apemost_hip.h)


def ladder_beta(kind, i, n_beta, beta_0):
    """BETA_ALIGNMENT functions, src/parallel_tempering_beta.c:53-83 (host scalar math)."""
    import math
    d = n_beta - 1
    if kind == 0:
        return beta_0 + (1 - beta_0) / 2 * (1 - math.cos(i * math.pi / d))
    if kind == 1:
        return beta_0 + i * (1 - beta_0) / d
    if kind == 2:
        return 1 / (1 / beta_0 + i * (1 - 1 / beta_0) / d)
    if kind == 3:
        return 1 / (1 / beta_0 + (1 - 1 / beta_0) / 2 * (1 - math.cos(i * math.pi / d)))
    if kind == 4:
        return beta_0 + math.pow(i * 1.0 / d, 2) * (1 - beta_0)
    if kind == 5:
        return beta_0 + (1 - beta_0) * math.pow((1 - math.cos(i * math.pi / d)) / 2, 2)
    if kind == 6:
        return beta_0
    raise ValueError("unknown ladder kind %r" % kind)


def get_chain_beta(kind, i, n_beta, beta_0):
    """get_chain_beta, src/parallel_tempering_beta.c:85-90: chain 0 is beta = 1."""
    if n_beta == 1:
        return 1.0
    return ladder_beta(kind, n_beta - i - 1, n_beta, beta_0)


def calc_beta_0(state, chain, stepwidth_factors):
    """calc_beta_0, src/parallel_tempering_beta.c:92-102 (BETA_0_STEPWIDTH = 1.0)."""
    r = (state.pmax[chain] - state.pmin[chain]) * 1.0
    r = r / state.step[chain]
    r = r / np.asarray(stepwidth_factors)
    return float(np.max(r)) ** -0.5


def ladder_view(arr, b, n_ladders):
    """ladder b's part of a ladder-major array of a batch: the chain axis -- axis 1 of sample rows
    [n_steps][n_ladders * n_chains][n_par + 2], axis 0 of everything else ([n_ladders * n_chains] or
    [n_ladders * n_chains][n_par]) -- cut into n_ladders equal blocks.  A view, not a copy."""
    arr = np.asarray(arr)
    axis = 1 if arr.ndim == 3 else 0
    total = arr.shape[axis]
    if n_ladders < 1 or total % n_ladders or not 0 <= b < n_ladders:
        raise ValueError("ladder %r of %r in an axis of %d chains" % (b, n_ladders, total))
    per = total // n_ladders
    return arr[:, b * per:(b + 1) * per] if axis == 1 else arr[b * per:(b + 1) * per]


def _rectangle(rows):
    """1-D arrays of possibly different lengths as the rows of one [len(rows)][longest] array, zeros behind each"""
    out = np.zeros((len(rows), max([len(r) for r in rows] + [0])), dtype=np.float64)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out


class HipSampler:
    def __init__(self, model, n_par, n_chains, data, seed=0, device=0, chain_offset=0,
                 n_chains_global=None, waves_per_chain=0, sigma=0.5, hmin=1e-6, lds_policy=0, circular_params=0,
                 flags=0, adapt_target=0.0, device_model_source=None, seeds=None, ragged=False):
        """seeds=None: one ladder (a shard of it) of n_chains chains under `seed`.  seeds=[...]: a ladder batch
        (include/apemost_hip.h, apemost_hip_create_batch; HipSampler.batch reads better): len(seeds) independent
        ladders of n_chains chains EACH in one sampler, ladder b under seeds[b]; `data` is one matrix for every
        ladder, [n_ladders][n_data][n_cols], or a list of one [n_data_b][n_cols] matrix per ladder, whose lengths may
        differ (apemost_hip_create_batch_ragged); self.n_chains is then the total, self.chains_per_ladder the rest,
        self.n_data_per_ladder the ladders' data lengths.  ragged=True: through apemost_hip_create_batch_ragged even
        where the lengths are equal (the two give the same sampler)."""
        if seeds is not None and ragged and not isinstance(data, (list, tuple)):
            data = np.asarray(data, dtype=np.float64)
            data = [data] * len(seeds) if data.ndim == 2 else list(data)
        # (a list whose elements are matrices: one per ladder; a nested list that spells one matrix, or a 3-D array,
        # goes the way it always went)
        if seeds is not None and isinstance(data, (list, tuple)) and len(data) > 0 and np.ndim(data[0]) == 2:
            mats = [np.ascontiguousarray(m, dtype=np.float64) for m in data]
            if len(mats) != len(seeds) or any(m.ndim != 2 or m.shape[1:] != mats[0].shape[1:] for m in mats):
                raise ValueError("data: a list of one [n_data_b][n_cols] matrix per ladder, n_cols the same for all")
            # (equal lengths: the rectangular batch, as ever)
            data = np.stack(mats) if all(len(m) == len(mats[0]) for m in mats) and not ragged else mats
        else:
            data = np.ascontiguousarray(data, dtype=np.float64)
        if seeds is not None:
            self._init_batch(model, n_par, n_chains, data, [int(x) for x in seeds], device, chain_offset, n_chains_global,
                             waves_per_chain, sigma, hmin, lds_policy, circular_params, flags, adapt_target,
                             device_model_source)
            return
        assert data.ndim == 2
        self.cfg = capi.Config(abi_version=capi.ABI_VERSION, device=device, model=model, n_par=n_par,
                               n_chains=n_chains, n_data=data.shape[0], n_cols=data.shape[1],
                               waves_per_chain=waves_per_chain, lds_policy=lds_policy, chain_offset=chain_offset,
                               n_chains_global=n_chains if n_chains_global is None else n_chains_global,
                               seed=seed, sigma=sigma, hmin=hmin, circular_params=circular_params, flags=flags,
                               adapt_target=adapt_target,
                               device_model_source=None if device_model_source is None else str(device_model_source).encode())
        self._h = C.c_void_p()
        self.L = capi.lib()
        capi.check(self.L.apemost_hip_create(C.byref(self.cfg), C.byref(self._h)))
        capi.check(self.L.apemost_hip_set_data(self._h, data.ctypes.data_as(C.POINTER(C.c_double))))
        self.n_par, self.n_chains = n_par, n_chains
        self.n_chains_global = self.cfg.n_chains_global
        self.chain_offset = chain_offset
        self.seed = seed
        self.n_ladders, self.chains_per_ladder, self.seeds = 1, n_chains, [seed]
        self.n_data_per_ladder = [data.shape[0]]
        self._x0 = [data[:, 0].copy()]
        self._y0 = [data[:, 1].copy()]

    def _init_batch(self, model, n_par, n_chains, data, seeds, device, chain_offset, n_chains_global, waves_per_chain,
                    sigma, hmin, lds_policy, circular_params, flags, adapt_target, device_model_source):
        n_ladders = len(seeds)
        ragged = isinstance(data, list)   # one matrix per ladder, of different lengths
        if not ragged and (data.ndim not in (2, 3) or (data.ndim == 3 and data.shape[0] != n_ladders)):
            raise ValueError("data: [n_data][n_cols], or [n_ladders][n_data][n_cols] with one matrix per ladder")
        lengths = [len(m) for m in data] if ragged else [data.shape[-2]] * n_ladders
        self.cfg = capi.Config(abi_version=capi.ABI_VERSION, device=device, model=model, n_par=n_par,
                               n_chains=n_chains, n_data=max(lengths) if lengths else 0,
                               n_cols=data[0].shape[-1] if ragged else data.shape[-1],
                               waves_per_chain=waves_per_chain, lds_policy=lds_policy, chain_offset=chain_offset,
                               n_chains_global=n_chains if n_chains_global is None else n_chains_global,
                               seed=0, sigma=sigma, hmin=hmin, circular_params=circular_params, flags=flags,
                               adapt_target=adapt_target,
                               device_model_source=None if device_model_source is None else str(device_model_source).encode())
        self._h = C.c_void_p()
        self.L = capi.lib()
        arr = (C.c_uint64 * max(n_ladders, 1))(*seeds)
        if ragged:
            lens = (C.c_int32 * n_ladders)(*lengths)
            capi.check(self.L.apemost_hip_create_batch_ragged(C.byref(self.cfg), n_ladders, arr, lens, C.byref(self._h)))
        else:
            capi.check(self.L.apemost_hip_create_batch(C.byref(self.cfg), n_ladders, arr, C.byref(self._h)))
        self.n_data_per_ladder = lengths
        self.n_par, self.n_chains = n_par, n_chains * n_ladders
        self.n_chains_global = n_chains            # of the swap schedule: per ladder
        self.chain_offset = 0
        self.seed = seeds[0]
        self.n_ladders, self.chains_per_ladder, self.seeds = n_ladders, n_chains, seeds
        self._x0 = [None] * n_ladders
        self._y0 = [None] * n_ladders
        if not ragged and data.ndim == 2:
            self.set_data(data)
        else:
            for b in range(n_ladders):
                self.set_data(data[b], ladder=b)

    @classmethod
    def batch(cls, model, n_par, n_chains, data, seeds, **kw):
        """a ladder batch: len(seeds) independent ladders of n_chains chains each, stepped by one launch"""
        return cls(model, n_par, n_chains, data, seeds=seeds, **kw)

    def set_data(self, data, ladder=None):
        """the data matrix [n_data][n_cols] of every ladder (ladder=None) or of one ladder of a batch, in that
        ladder's own length (n_data_per_ladder)"""
        data = np.ascontiguousarray(data, dtype=np.float64)
        if ladder is None and len(set(self.n_data_per_ladder)) > 1:
            raise ValueError("the ladders of this batch differ in data length %s: set_data(data, ladder=b)"
                             % (self.n_data_per_ladder,))
        if ladder is not None and not 0 <= int(ladder) < self.n_ladders:
            raise ValueError("ladder %r outside [0,%d)" % (ladder, self.n_ladders))
        n_data = self.n_data_per_ladder[0 if ladder is None else int(ladder)]
        if data.shape != (n_data, self.cfg.n_cols):
            raise ValueError("data must be [%d][%d]" % (n_data, self.cfg.n_cols))
        p = data.ctypes.data_as(C.POINTER(C.c_double))
        if ladder is None:
            capi.check(self.L.apemost_hip_set_data(self._h, p))
        else:
            capi.check(self.L.apemost_hip_set_data_ladder(self._h, int(ladder), p))
        for b in range(self.n_ladders) if ladder is None else [int(ladder)]:
            self._x0[b] = data[:, 0].copy()   # the abscissae: what predict_begin(x=None) folds over
            self._y0[b] = data[:, 1].copy()   # with them the data of pointwise_begin

    def _user_rows(self, x):
        """a user model's abscissae are whole rows [n_x][n_cols]; a 1-D x is column 0, the other columns zero"""
        x = np.asarray(x, dtype=np.float64)
        if x.ndim == 1:
            rows = np.zeros((len(x), self.cfg.n_cols))
            rows[:, 0] = x
            return rows
        if x.ndim != 2 or x.shape[1] != self.cfg.n_cols:
            raise ValueError("x of a user model: [n_x] or [n_x][%d]" % self.cfg.n_cols)
        return np.ascontiguousarray(x)

    def ladder_view(self, arr, b):
        """ladder b's part of a ladder-major array or of sample rows of this sampler (module-level ladder_view)"""
        return ladder_view(arr, b, self.n_ladders)

    def close(self):
        if self._h:
            self.L.apemost_hip_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- plumbing -----------------------------------------------------------------
    def synchronize(self):
        capi.check(self.L.apemost_hip_synchronize(self._h))

    @property
    def stream(self):
        p = C.c_void_p()
        capi.check(self.L.apemost_hip_stream(self._h, C.byref(p)))
        return p.value or 0

    @property
    def geometry(self):
        w, l = C.c_int(0), C.c_int(0)
        capi.check(self.L.apemost_hip_waves_per_chain(self._h, C.byref(w), C.byref(l)))
        return w.value, bool(l.value)

    @property
    def user_model_compile_seconds(self):
        """hiprtc's time for this sampler's device model (0: the process had compiled the same source before)"""
        t = C.c_double(0)
        capi.check(self.L.apemost_hip_user_model_compile_seconds(self._h, C.byref(t)))
        return t.value

    @property
    def user_hooks(self):
        """(has the curve hook, has the pointwise hook, hiprtc's seconds for the analysis module -- 0: the process had
        compiled the same source's hooks before) of this sampler's device model (include/apemost_device_model.h); the
        first call, like the first predict_* or pointwise_* call, compiles that module"""
        c, p, t = C.c_int32(0), C.c_int32(0), C.c_double(0)
        capi.check(self.L.apemost_hip_user_hooks(self._h, C.byref(c), C.byref(p), C.byref(t)))
        return bool(c.value), bool(p.value), t.value

    @property
    def launch_policy(self):
        """(one-barrier kernel, cooperative multi-round launches, rounds one launch may hold)"""
        ob, co, mr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        capi.check(self.L.apemost_hip_launch_policy(self._h, C.byref(ob), C.byref(co), C.byref(mr)))
        return bool(ob.value), bool(co.value), mr.value

    @property
    def ob_helper(self):
        """the one-barrier kernel runs with a helper wavefront (the prior of the proposal in flight off the owner)"""
        ob = C.c_int32(0)
        capi.check(self.L.apemost_hip_launch_policy(self._h, C.byref(ob), None, None))
        return ob.value == 2

    def set_state(self, state, fields=None):
        v = state.view(fields) if fields else state.view()
        capi.check(self.L.apemost_hip_set_state(self._h, C.byref(v)))

    def get_state(self, state=None, fields=None):
        state = state or LadderState(self.n_chains, self.n_par)
        v = state.view(fields) if fields else state.view()
        capi.check(self.L.apemost_hip_get_state(self._h, C.byref(v)))
        return state

    @property
    def round(self):
        r, p = C.c_uint64(0), C.c_int(0)
        capi.check(self.L.apemost_hip_get_round(self._h, C.byref(r), C.byref(p)))
        return r.value, bool(p.value)

    def set_round(self, round_, swap_pending=False):
        capi.check(self.L.apemost_hip_set_round(self._h, round_, int(swap_pending)))

    # -- hot path -----------------------------------------------------------------
    def calc_model(self, first=0, count=-1):
        capi.check(self.L.apemost_hip_calc_model(self._h, first, count))

    def loglike(self, params, beta):
        params = np.ascontiguousarray(params, dtype=np.float64).reshape(-1, self.n_par)
        n = params.shape[0]
        beta = np.ascontiguousarray(np.broadcast_to(np.asarray(beta, dtype=np.float64), (n,)))
        prob, prior = np.zeros(n), np.zeros(n)
        dp = C.POINTER(C.c_double)
        capi.check(self.L.apemost_hip_loglike(self._h, n, params.ctypes.data_as(dp), beta.ctypes.data_as(dp),
                                              prob.ctypes.data_as(dp), prior.ctypes.data_as(dp)))
        return prob, prior

    def _adopt(self, d_samples):
        """The sampler launches on its own stream.  A sample buffer that torch has just created
        (torch.zeros fills it on torch's current stream) must be complete before the first kernel
        writes rows into it, or the fill may land on top of them."""
        if d_samples and d_samples != getattr(self, "_last_samples", 0):
            import sys
            torch = sys.modules.get("torch")    # (a process without torch has no torch buffer to wait for)
            if torch is not None and torch.cuda.is_available():
                torch.cuda.current_stream().synchronize()
        self._last_samples = d_samples

    def launch_round(self, n_steps, apply_swap, d_samples=0):
        self._adopt(d_samples)
        capi.check(self.L.apemost_hip_launch_round(self._h, n_steps, int(apply_swap), d_samples))

    def launch_rounds(self, n_rounds, n_steps, apply_swap, d_samples=0):
        self._adopt(d_samples)
        capi.check(self.L.apemost_hip_launch_rounds(self._h, n_rounds, n_steps, int(apply_swap), d_samples))

    def swap_pair(self, round_, ladder=None):
        """lower chain of the pair swap attempt `round_` picks under this sampler's swap schedule; on a batch the
        pair inside ladder `ladder` (each ladder draws its own)"""
        if self.n_ladders == 1 and ladder is None:
            return int(self.L.apemost_hip_sampler_swap_pair(self._h, round_))
        if ladder is None or not 0 <= ladder < self.n_ladders:
            raise ValueError("swap_pair on a batch of %d ladders needs ladder=" % self.n_ladders)
        if self.chains_per_ladder <= 1:
            return -1
        if self.cfg.flags & capi.FLAG_SWAP_EVEN_ODD:
            return round_ % 2 if round_ % 2 <= self.chains_per_ladder - 2 else -1
        return capi.swap_pair(self.seeds[ladder], round_, self.chains_per_ladder)

    def swap_attempts(self, pair, first_round, n_rounds, ladder=None):
        """how often the pair (pair, pair + 1) of the global ladder is attempted in the swap attempts first_round ..
        first_round + n_rounds - 1: a pure function of the schedule, so that swapcount / attempts is the per-pair
        swap rate a ladder is tuned with.  Even-odd sweeps: the sweeps of the pair's parity.  On a batch: the pair
        (pair, pair + 1) inside ladder `ladder`, under that ladder's seed."""
        if not 0 <= pair <= self.n_chains_global - 2 or n_rounds <= 0:
            return 0
        if self.cfg.flags & capi.FLAG_SWAP_EVEN_ODD:
            first = first_round + ((pair - first_round) % 2)     # the first sweep of the pair's parity
            return max(0, (first_round + n_rounds - first + 1) // 2)
        return sum(1 for r in range(first_round, first_round + n_rounds) if self.swap_pair(r, ladder) == pair)

    def rounds_within_shard(self, first_round, max_rounds):
        """how many swap attempts from `first_round` on (at most max_rounds) do not straddle an edge of this shard"""
        return int(self.L.apemost_hip_rounds_within_shard(self._h, first_round, max_rounds))

    @property
    def max_rounds_per_launch(self):
        v = C.c_int32(0)
        capi.check(self.L.apemost_hip_max_rounds_per_launch(self._h, C.byref(v)))
        return v.value

    def markov_chain_step_for(self, param, n_steps=1, d_samples=0):
        self._adopt(d_samples)
        capi.check(self.L.apemost_hip_launch_round_for(self._h, n_steps, param, d_samples))

    def run_sampler(self, n_rounds, n_swap, d_samples=0):
        """n_rounds x {n_swap steps per chain, one swap attempt}; asynchronous."""
        self._adopt(d_samples)
        capi.check(self.L.apemost_hip_run(self._h, n_rounds, n_swap, d_samples))

    # -- replica flow (apemost_amd/replica_flow.py; flags=capi.FLAG_TRACK_REPLICAS) -----------
    def replica_flow(self, ladder=None):
        """the replica flow so far as a ReplicaFlow, with the chains' betas and swap counts (synchronises like
        get_state).  A batch gives a list, one per ladder, or the one of ladder `ladder`."""
        from .replica_flow import FIELDS, ReplicaFlow
        a = {k: np.zeros(self.n_chains, dtype=t) for k, t in FIELDS}
        v = capi.ReplicaFlowView(**{k: a[k].ctypes.data_as(C.POINTER(C.c_uint32 if t == np.uint32 else C.c_uint64))
                                    for k, t in FIELDS})
        capi.check(self.L.apemost_hip_replica_flow_get(self._h, C.byref(v)))
        st = self.get_state(fields=("beta", "swapcount"))
        flows = [ReplicaFlow(beta=self.ladder_view(st.beta, b).copy(), swapcount=self.ladder_view(st.swapcount, b).copy(),
                             **{k: self.ladder_view(a[k], b).copy() for k, _ in FIELDS}) for b in range(self.n_ladders)]
        if ladder is not None:
            return flows[ladder]
        return flows[0] if self.n_ladders == 1 else flows

    def replica_flow_set(self, rf):
        """load a ReplicaFlow (a list of them, one per ladder, on a batch) saved by replica_flow(): a resumed run.
        betas and swap counts are state and travel with set_state."""
        from .replica_flow import FIELDS
        flows = list(rf) if isinstance(rf, (list, tuple)) else [rf]
        if len(flows) != self.n_ladders or any(len(f.replica) != self.chains_per_ladder for f in flows):
            raise ValueError("replica_flow_set: %d ladders of %d chains are needed" % (self.n_ladders, self.chains_per_ladder))
        a = {k: np.ascontiguousarray(np.concatenate([getattr(f, k) for f in flows]), dtype=t) for k, t in FIELDS}
        v = capi.ReplicaFlowView(**{k: a[k].ctypes.data_as(C.POINTER(C.c_uint32 if t == np.uint32 else C.c_uint64))
                                    for k, t in FIELDS})
        capi.check(self.L.apemost_hip_replica_flow_set(self._h, C.byref(v)))

    def replica_flow_reset(self):
        """labels to identity, headings and counters to the initial state (after burn-in)"""
        capi.check(self.L.apemost_hip_replica_flow_reset(self._h))

    # -- run summary (apemost_amd/summary.py) ------------------------------------------------
    def summary_begin(self, lo=None, hi=None, n_hist_chains=1, nbins=200, batch_size=1, max_batches=0, thin=1):
        """start an on-device summary: prob - prior sums of every chain, and histograms over [lo, hi] and
        batch sums of batch_size (batch_means_error()) for chains 0 .. n_hist_chains-1.  `thin` is only
        recorded with the summary (accumulate takes the rows' own skip/thin)."""
        cfg = capi.SummaryConfig(n_hist_chains=n_hist_chains, nbins=nbins, batch_size=batch_size, max_batches=max_batches)
        dp = C.POINTER(C.c_double)
        self._sum_lo = None if lo is None else np.ascontiguousarray(lo, dtype=np.float64)
        self._sum_hi = None if hi is None else np.ascontiguousarray(hi, dtype=np.float64)
        if self._sum_lo is not None:
            assert self._sum_lo.shape == (self.n_par,) and self._sum_hi.shape == (self.n_par,)
            cfg.lo, cfg.hi = self._sum_lo.ctypes.data_as(dp), self._sum_hi.ctypes.data_as(dp)
        capi.check(self.L.apemost_hip_summary_begin(self._h, C.byref(cfg)))
        self._sum_cfg = dict(n_hist_chains=n_hist_chains, nbins=nbins, batch_size=batch_size, max_batches=max_batches,
                             thin=thin)

    def summary_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2] into the
        summary; asynchronous (summary() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_summary_accumulate(self._h, d_samples, n_steps, skip, thin))

    def _summary_view(self, arrays):
        return capi.SummaryView(n=arrays["n"].ctypes.data_as(capi._up), prob_sum=arrays["prob_sum"].ctypes.data_as(C.POINTER(C.c_double)),
                                hist=arrays["hist"].ctypes.data_as(capi._up),
                                batch_sums=arrays["batch_sums"].ctypes.data_as(C.POINTER(C.c_double)),
                                n_batches=arrays["n_batches"].ctypes.data_as(capi._up))

    def summary(self):
        """the summary so far as a RunSummary (synchronises with the accumulates issued so far)"""
        from .summary import RunSummary
        c = self._sum_cfg
        a = dict(n=np.zeros(1, dtype=np.uint64), prob_sum=np.zeros(self.n_chains),
                 hist=np.zeros((c["n_hist_chains"], self.n_par, c["nbins"]), dtype=np.uint64),
                 batch_sums=np.zeros((c["n_hist_chains"], self.n_par, c["max_batches"] + 1)),
                 n_batches=np.zeros(1, dtype=np.uint64))
        capi.check(self.L.apemost_hip_summary_get(self._h, C.byref(self._summary_view(a))))
        lo = self._sum_lo if self._sum_lo is not None else np.zeros(self.n_par)
        hi = self._sum_hi if self._sum_hi is not None else np.zeros(self.n_par)
        return RunSummary(int(a["n"][0]), a["prob_sum"], a["hist"], a["batch_sums"], int(a["n_batches"][0]), lo, hi,
                          c["batch_size"], c["thin"])

    def summary_set(self, rs):
        """load a RunSummary (a resumed run) into the summary begun with the same configuration"""
        a = dict(n=np.array([rs.n], dtype=np.uint64), prob_sum=np.ascontiguousarray(rs.prob_sum, dtype=np.float64),
                 hist=np.ascontiguousarray(rs.hist, dtype=np.uint64),
                 batch_sums=np.ascontiguousarray(rs.batch_sums, dtype=np.float64),
                 n_batches=np.array([rs.n_batches], dtype=np.uint64))
        c = self._sum_cfg
        assert a["prob_sum"].shape == (self.n_chains,)
        assert a["hist"].shape == (c["n_hist_chains"], self.n_par, c["nbins"])
        assert a["batch_sums"].shape == (c["n_hist_chains"], self.n_par, c["max_batches"] + 1)
        capi.check(self.L.apemost_hip_summary_set(self._h, C.byref(self._summary_view(a))))

    def summary_end(self):
        capi.check(self.L.apemost_hip_summary_end(self._h))

    # -- on-device peaks (apemost_amd/peaks.py) -------------------------------------------------
    def peaks_begin(self, lo, hi, chains=(0,), capacity=1 << 20):
        """keep the parameter columns of the local chains `chains` (strictly increasing; b * chains_per_ladder is
        ladder b's chain 0) on the device, up to `capacity` kept samples each, for the peaks of the reference's
        peaks.exe over [lo[p], hi[p]]"""
        self._pk_lo = np.ascontiguousarray(lo, dtype=np.float64)
        self._pk_hi = np.ascontiguousarray(hi, dtype=np.float64)
        self._pk_chains = np.ascontiguousarray(chains, dtype=np.int32)
        assert self._pk_lo.shape == (self.n_par,) and self._pk_hi.shape == (self.n_par,) and self._pk_chains.ndim == 1
        dp = C.POINTER(C.c_double)
        cfg = capi.PeaksConfig(n_keep=len(self._pk_chains), chains=self._pk_chains.ctypes.data_as(C.POINTER(C.c_int32)),
                               capacity=capacity, lo=self._pk_lo.ctypes.data_as(dp), hi=self._pk_hi.ctypes.data_as(dp))
        capi.check(self.L.apemost_hip_peaks_begin(self._h, C.byref(cfg)))

    def peaks_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """append the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2] to the
        columns; asynchronous (peaks() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_peaks_accumulate(self._h, d_samples, n_steps, skip, thin))

    def peaks(self):
        """the peaks of the columns stored so far as a Peaks object (sorts on the device; synchronises with the
        accumulates issued so far).  A column with 100 peaks or more raises ApemostHipError, as the tool aborts."""
        from .peaks import Peaks
        pk = Peaks.empty(len(self._pk_chains), self.n_par, self._pk_lo, self._pk_hi, self._pk_chains)
        capi.check(self.L.apemost_hip_peaks_get(self._h, C.byref(pk.view())))
        return pk

    def peaks_end(self):
        capi.check(self.L.apemost_hip_peaks_end(self._h))

    # -- on-device joint marginals (apemost_amd/joint.py) ------------------------------------------
    def joint_begin(self, lo, hi, chains=(0,), nbins=200, pairs=None):
        """start pair histograms (nbins x nbins over [lo, hi], the summary's bins) and moments about the first
        sample for the local chains `chains` (strictly increasing; b * chains_per_ladder is ladder b's chain 0).
        pairs: a list of (i, j), i < j; None: all of them in lexicographic order; []: the moments alone."""
        from .joint import all_pairs
        self._jt_lo = np.ascontiguousarray(lo, dtype=np.float64)
        self._jt_hi = np.ascontiguousarray(hi, dtype=np.float64)
        self._jt_chains = np.ascontiguousarray(chains, dtype=np.int32)
        assert self._jt_lo.shape == (self.n_par,) and self._jt_hi.shape == (self.n_par,) and self._jt_chains.ndim == 1
        self._jt_pairs = np.ascontiguousarray(all_pairs(self.n_par) if pairs is None else pairs,
                                              dtype=np.int32).reshape(-1, 2)
        self._jt_nbins = int(nbins)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        given = np.zeros((max(len(self._jt_pairs), 1), 2), dtype=np.int32)    # (never a NULL pointer for an empty list)
        given[:len(self._jt_pairs)] = self._jt_pairs
        cfg = capi.JointConfig(n_keep=len(self._jt_chains), chains=self._jt_chains.ctypes.data_as(ip), nbins=nbins,
                               n_pairs=len(self._jt_pairs), pairs=None if pairs is None else given.ctypes.data_as(ip),
                               lo=self._jt_lo.ctypes.data_as(dp), hi=self._jt_hi.ctypes.data_as(dp))
        capi.check(self.L.apemost_hip_joint_begin(self._h, C.byref(cfg)))

    def joint_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2] into the joint
        marginals; asynchronous (joint() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_joint_accumulate(self._h, d_samples, n_steps, skip, thin))

    def joint(self):
        """the joint marginals so far as a Joint object (synchronises with the accumulates issued so far)"""
        from .joint import Joint
        jt = Joint.empty(len(self._jt_chains), self.n_par, self._jt_nbins, self._jt_pairs, self._jt_lo, self._jt_hi,
                         self._jt_chains)
        capi.check(self.L.apemost_hip_joint_get(self._h, C.byref(jt.view())))
        return jt

    def joint_set(self, jt):
        """load a Joint (a resumed run) into the joint begun with the same configuration"""
        assert jt.counts.shape == (len(self._jt_chains), len(self._jt_pairs), self._jt_nbins, self._jt_nbins)
        assert jt.sum.shape == (len(self._jt_chains), self.n_par) and np.array_equal(jt.pairs, self._jt_pairs)
        capi.check(self.L.apemost_hip_joint_set(self._h, C.byref(jt.view())))

    def joint_end(self):
        capi.check(self.L.apemost_hip_joint_end(self._h))

    # -- on-device derived quantities (apemost_amd/derived.py) --------------------------------------
    def derived_begin(self, columns, lo, hi, chains=(0,), nbins=200, pairs=None, batch_size=1, max_batches=0, names=None,
                      stage_steps=0, thin=1):
        """start the fold of computed columns for the local chains `chains`: histograms over [lo[c], hi[c]] on the
        summary's bins, batch sums, the joint fold's pair counts and moments over the columns, non-finite counts, min
        and max.  columns: each a derived.Program, an infix expression (derived.compile) or a (name, either) pair;
        names: the parameters' names in expressions (default p0, p1, ...).  stage_steps: kept steps per staged piece,
        0 for the joint fold's choice.  `thin` is only recorded with the result."""
        from . import derived as dv
        row_names = ["p%d" % i for i in range(self.n_par)] if names is None else list(names)
        assert len(row_names) == self.n_par
        col_names, programs = [], []
        for c, col in enumerate(columns):
            name, col = col if isinstance(col, tuple) else ("d%d" % c, col)
            col_names.append(name)
            programs.append(col if isinstance(col, dv.Program) else dv.compile(col, row_names))
        code, start, consts = dv.pack(programs)
        lo, hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        chains = np.ascontiguousarray(chains, dtype=np.int32)
        assert lo.shape == hi.shape == (len(programs),) and chains.ndim == 1
        use_pairs = np.ascontiguousarray(dv.all_pairs(len(programs)) if pairs is None else pairs, dtype=np.int32).reshape(-1, 2)
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
        given = np.zeros((max(len(use_pairs), 1), 2), dtype=np.int32)    # (never a NULL pointer for an empty list)
        given[:len(use_pairs)] = use_pairs
        code_arg = code if len(code) else np.zeros(1, dtype=np.int32)
        consts_arg = consts if len(consts) else np.zeros(1)
        cfg = capi.DerivedConfig(n_keep=len(chains), chains=chains.ctypes.data_as(ip), n_col=len(programs),
                                 code=code_arg.ctypes.data_as(ip), start=start.ctypes.data_as(ip), n_const=len(consts),
                                 consts=consts_arg.ctypes.data_as(dp), nbins=nbins, n_pairs=len(use_pairs),
                                 pairs=None if pairs is None else given.ctypes.data_as(ip), lo=lo.ctypes.data_as(dp),
                                 hi=hi.ctypes.data_as(dp), batch_size=batch_size, max_batches=max_batches,
                                 stage_steps=stage_steps)
        capi.check(self.L.apemost_hip_derived_begin(self._h, C.byref(cfg)))
        self._dv_cfg = dict(programs=programs, lo=lo, hi=hi, chains=chains, nbins=int(nbins), pairs=use_pairs,
                            batch_size=int(batch_size), max_batches=int(max_batches), names=col_names,
                            row_names=row_names, thin=thin)

    def derived_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2]; asynchronous
        (derived() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_derived_accumulate(self._h, d_samples, n_steps, skip, thin))

    def derived(self):
        """the fold so far as a Derived object (synchronises with the accumulates issued so far)"""
        from .derived import Derived
        dv = Derived.empty(**self._dv_cfg)
        capi.check(self.L.apemost_hip_derived_get(self._h, C.byref(dv.view())))
        return dv

    def derived_set(self, dv):
        """load a Derived (a resumed run) into the fold begun with the same configuration"""
        c = self._dv_cfg
        assert dv.hist.shape == (len(c["chains"]), len(c["programs"]), c["nbins"]) and np.array_equal(dv.pairs, c["pairs"])
        assert dv.batch.shape[2] == c["max_batches"] + 1 and dv.batch_size == c["batch_size"]
        dv.n_batches_[0] = dv.n_batches
        capi.check(self.L.apemost_hip_derived_set(self._h, C.byref(dv.view())))

    def derived_end(self):
        capi.check(self.L.apemost_hip_derived_end(self._h))

    def derived_eval(self, rows):
        """[n][n_col]: the open fold's programs on the host rows [n][n_par+2], by the device function the fold uses"""
        rows = np.ascontiguousarray(rows, dtype=np.float64)
        assert rows.ndim == 2 and rows.shape[1] == self.n_par + 2
        out = np.zeros((len(rows), len(self._dv_cfg["programs"])))
        dp = C.POINTER(C.c_double)
        capi.check(self.L.apemost_hip_derived_eval(self._h, len(rows), rows.ctypes.data_as(dp), out.ctypes.data_as(dp)))
        return out

    # -- on-device evidence fold (apemost_amd/evidence.py) ------------------------------------------
    def evidence_begin(self, betas=None, batch_size=1, max_batches=0, coef_up=None, coef_down=None, thin=1):
        """start the fold of column n_par+1 of every local chain: moments about the first sample, batch sums and the
        two log-sum-exps of the stepping-stone estimators.  betas: the ladder-major betas of the local chains (None:
        the sampler's own); the coefficients follow from them (Evidence.coefficients) unless coef_up and coef_down
        [n_chains] are given, which a shard of a sharded ladder needs: its neighbours' betas live elsewhere."""
        from .evidence import Evidence
        if betas is None:
            betas = self.get_state(fields=("beta",)).beta
        self._ev_betas = np.ascontiguousarray(betas, dtype=np.float64)
        assert self._ev_betas.shape == (self.n_chains,)
        if coef_up is None or coef_down is None:
            coef_up, coef_down = Evidence.coefficients(self._ev_betas, self.n_ladders)
        self._ev_coef = np.ascontiguousarray([coef_up, coef_down], dtype=np.float64)
        assert self._ev_coef.shape == (2, self.n_chains)
        self._ev_bs, self._ev_max, self._ev_thin = int(batch_size), int(max_batches), int(thin)
        cfg = capi.EvidenceConfig(batch_size=batch_size, max_batches=max_batches,
                                  coef_up=self._ev_coef[0].ctypes.data_as(capi._dp),
                                  coef_down=self._ev_coef[1].ctypes.data_as(capi._dp))
        capi.check(self.L.apemost_hip_evidence_begin(self._h, C.byref(cfg)))

    def evidence_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2]; asynchronous
        (evidence() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_evidence_accumulate(self._h, d_samples, n_steps, skip, thin))

    def evidence(self):
        """the fold so far as an Evidence object (synchronises with the accumulates issued so far)"""
        from .evidence import Evidence
        ev = Evidence.empty(self._ev_betas, self._ev_bs, self._ev_max, self._ev_coef[0], self._ev_coef[1],
                            self.n_ladders, self._ev_thin)
        capi.check(self.L.apemost_hip_evidence_get(self._h, C.byref(ev.view())))
        return ev

    def evidence_set(self, ev):
        """load an Evidence (a resumed run) into the fold begun with the same configuration"""
        assert ev.batch.shape == (self.n_chains, self._ev_max + 1) and ev.batch_size == self._ev_bs
        capi.check(self.L.apemost_hip_evidence_set(self._h, C.byref(ev.view())))

    def evidence_end(self):
        capi.check(self.L.apemost_hip_evidence_end(self._h))

    # -- on-device MBAR (apemost_amd/mbar.py) -------------------------------------------------------
    def mbar_begin(self, capacity, betas=None, thin=1):
        """start the store of loglike = column n_par+1 / beta of every kept step of every local chain, with room for
        `capacity` kept steps (capacity * n_chains <= 2^28).  betas: the ladder-major betas of the local chains (None:
        the sampler's own), positive and strictly decreasing in every ladder.  Not for a shard of a sharded ladder."""
        from .mbar import check_betas
        if betas is None:
            betas = self.get_state(fields=("beta",)).beta
        self._mb_betas = check_betas(betas, self.n_ladders)
        assert self._mb_betas.shape == (self.n_chains,)
        self._mb_thin = int(thin)
        cfg = capi.MbarConfig(capacity=capacity, betas=self._mb_betas.ctypes.data_as(capi._dp))
        capi.check(self.L.apemost_hip_mbar_begin(self._h, C.byref(cfg)))
        self._mb_capacity = int(capacity)

    def mbar_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """append the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2]; asynchronous
        (mbar() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_mbar_accumulate(self._h, d_samples, n_steps, skip, thin))

    def mbar(self):
        """the store so far as an Mbar whose passes run on this sampler's device (synchronises with the accumulates
        issued so far); it computes on the open fold, so it is good until the next mbar_begin, mbar_set or mbar_end"""
        from .mbar import Mbar
        n = np.zeros(1, dtype=np.uint64)
        capi.check(self.L.apemost_hip_mbar_get(self._h, C.byref(capi.MbarView(n=n.ctypes.data_as(capi._up)))))
        mb = Mbar(np.zeros((int(n[0]), self.n_chains)), self._mb_betas, self.n_ladders, None, self._mb_thin, self)
        capi.check(self.L.apemost_hip_mbar_get(self._h, C.byref(mb.view())))
        return mb

    def mbar_set(self, mb):
        """load an Mbar's store (a resumed run) into the fold begun with the same betas"""
        assert mb.betas.tobytes() == self._mb_betas.tobytes() and mb.n <= self._mb_capacity
        capi.check(self.L.apemost_hip_mbar_set(self._h, C.byref(mb.view())))

    def mbar_end(self):
        capi.check(self.L.apemost_hip_mbar_end(self._h))

    # -- on-device reweighted posteriors (apemost_amd/reweight.py) ----------------------------------
    def reweight_begin(self, cols=None, lo=None, hi=None, nbins=200):
        """start the store of the columns `cols` (None: the parameters; at most 16, strictly increasing) of every kept
        step of every local chain beside the open mbar fold, before its first mbar_accumulate: the capacity is that
        fold's.  lo, hi [n_cols]: the histogram ranges (nbins = 0: no histograms)."""
        from .reweight import check_cols
        self._rw_cols = check_cols(np.arange(self.n_par) if cols is None else cols, self.n_par)
        k = len(self._rw_cols)
        self._rw_nbins = int(nbins)
        self._rw_lo = np.zeros(k) if lo is None else np.ascontiguousarray(lo, dtype=np.float64).reshape(k)
        self._rw_hi = np.zeros(k) if hi is None else np.ascontiguousarray(hi, dtype=np.float64).reshape(k)
        cfg = capi.ReweightConfig(n_cols=k, cols=self._rw_cols.ctypes.data_as(C.POINTER(C.c_int32)), nbins=self._rw_nbins,
                                  lo=self._rw_lo.ctypes.data_as(capi._dp), hi=self._rw_hi.ctypes.data_as(capi._dp))
        capi.check(self.L.apemost_hip_reweight_begin(self._h, C.byref(cfg)))

    def reweight_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """append the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2]: the rows
        mbar_accumulate is given, by a call of its own; asynchronous like it"""
        capi.check(self.L.apemost_hip_reweight_accumulate(self._h, d_samples, n_steps, skip, thin))

    def reweight(self):
        """the store so far as a Reweight whose sums run on this sampler's device (synchronises with the accumulates
        issued so far); good until the next mbar_begin, reweight_begin, reweight_set or either end"""
        from .reweight import Reweight
        n = np.zeros(1, dtype=np.uint64)
        capi.check(self.L.apemost_hip_reweight_get(self._h, C.byref(capi.ReweightView(n=n.ctypes.data_as(capi._up)))))
        rw = Reweight(np.zeros((len(self._rw_cols), int(n[0]), self.n_chains)), self._rw_cols, self._rw_lo, self._rw_hi,
                      self._rw_nbins, self.n_ladders, None, self._mb_thin, self)
        capi.check(self.L.apemost_hip_reweight_get(self._h, C.byref(rw.view())))
        return rw

    def reweight_set(self, rw):
        """load a Reweight's store (a resumed run, after mbar_set) into the fold begun with the same columns"""
        assert rw.cols.tobytes() == self._rw_cols.tobytes() and rw.n <= self._mb_capacity
        capi.check(self.L.apemost_hip_reweight_set(self._h, C.byref(rw.view())))

    def reweight_resample(self, g, beta=1.0, n_draws=4096, u=0, t0=0, t_count=None):
        """n_draws equally weighted draws per ladder at the target `beta` from the stores as they are on the device,
        under the free energies g [n_chains] over the kept steps [t0, t0 + t_count) (None: to the last stored): a
        Resampled, without the copy of the store that reweight() makes for Reweight.resample"""
        from .reweight import Reweight
        n = np.zeros(1, dtype=np.uint64)
        capi.check(self.L.apemost_hip_reweight_get(self._h, C.byref(capi.ReweightView(n=n.ctypes.data_as(capi._up)))))
        head = Reweight(np.zeros((len(self._rw_cols), 0, self.n_chains)), self._rw_cols, n_ladders=self.n_ladders,
                        thin=self._mb_thin)
        t_count = int(n[0]) - t0 if t_count is None else t_count
        r = head._draws(float(beta), n_draws, u, t0, t_count)
        r.n = int(n[0])
        g = np.ascontiguousarray(g, dtype=np.float64).reshape(self.n_chains)
        shift = np.zeros(1, dtype=np.int32)
        out = capi.ReweightDraws(index=r.index.ctypes.data_as(C.POINTER(C.c_uint32)), x=r.x.ctypes.data_as(capi._dp),
                                 q_total=r.q_total.ctypes.data_as(capi._up),
                                 shift=shift.ctypes.data_as(C.POINTER(C.c_int32)))
        capi.check(self.L.apemost_hip_reweight_resample(self._h, t0, t_count, g.ctypes.data_as(capi._dp), float(beta),
                                                        r.n_draws, r.u, C.byref(out)))
        return r

    def reweight_end(self):
        capi.check(self.L.apemost_hip_reweight_end(self._h))

    # -- on-device autocorrelation (apemost_amd/autocorr.py) ----------------------------------------
    def autocorr_begin(self, chains=(0,), max_lag=1024, cols=None, thin=1):
        """start the lag sums of the columns `cols` (None: the parameters and prob - prior) of the local chains
        `chains` (strictly increasing; b * chains_per_ladder is ladder b's chain 0) for the lags 0 .. max_lag - 1.
        thin is recorded in the result: lags count kept samples."""
        from .autocorr import default_cols
        self._ac_chains = np.ascontiguousarray(chains, dtype=np.int32)
        self._ac_cols = np.ascontiguousarray(default_cols(self.n_par) if cols is None else cols, dtype=np.int32)
        assert self._ac_chains.ndim == 1 and self._ac_cols.ndim == 1
        self._ac_lag, self._ac_thin = int(max_lag), int(thin)
        ip = C.POINTER(C.c_int32)
        cfg = capi.AutocorrConfig(n_keep=len(self._ac_chains), chains=self._ac_chains.ctypes.data_as(ip),
                                  max_lag=self._ac_lag, n_cols=len(self._ac_cols),
                                  cols=None if cols is None else self._ac_cols.ctypes.data_as(ip))
        capi.check(self.L.apemost_hip_autocorr_begin(self._h, C.byref(cfg)))

    def autocorr_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2] into the lag
        sums; asynchronous (autocorr() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_autocorr_accumulate(self._h, d_samples, n_steps, skip, thin))

    def autocorr(self):
        """the fold so far as an Autocorr object (synchronises with the accumulates issued so far)"""
        from .autocorr import Autocorr
        ac = Autocorr.empty(self._ac_chains, self._ac_lag, self.n_par, self._ac_cols, self._ac_thin, self.n_ladders)
        capi.check(self.L.apemost_hip_autocorr_get(self._h, C.byref(ac.view())))
        return ac

    def autocorr_set(self, ac):
        """load an Autocorr (a resumed run) into the fold begun with the same configuration"""
        assert ac.lag.shape == (len(self._ac_chains), len(self._ac_cols), self._ac_lag)
        assert np.array_equal(ac.chains, self._ac_chains) and np.array_equal(ac.cols, self._ac_cols)
        capi.check(self.L.apemost_hip_autocorr_set(self._h, C.byref(ac.view())))

    def autocorr_end(self):
        capi.check(self.L.apemost_hip_autocorr_end(self._h))

    # -- on-device posterior predictive (apemost_amd/predict.py) ------------------------------------
    def predict_begin(self, chains=(0,), x=None, nbins=0, lo=None, hi=None, thin=1):
        """start the fold of the model curve at the abscissae x (None: column 0 of the data, for every kept chain that
        of its own ladder; a user model with the curve hook: rows [n_x][n_cols], a 1-D x being column 0 with the other
        columns zero, None: the data's rows) over the kept samples of the local chains `chains` (strictly increasing).  nbins > 0 adds a
        histogram of the curve's values over [lo, hi] at every abscissa: medians and credible bands.  thin is recorded
        in the result."""
        self._pr_chains = np.ascontiguousarray(chains, dtype=np.int32)
        assert self._pr_chains.ndim == 1
        self._pr_nbins, self._pr_thin = int(nbins), int(thin)
        self._pr_lo, self._pr_hi = (0.0, 0.0) if nbins == 0 else (float(lo), float(hi))
        if x is None:
            xs = [self._x0[int(c) // self.chains_per_ladder if self.n_ladders > 1 else 0]
                  for c in self._pr_chains.tolist() if 0 <= c < self.n_chains]
            xs = xs if len(xs) == len(self._pr_chains) else [self._x0[0]] * len(self._pr_chains)
            self._pr_x = _rectangle(xs)   # (a ragged batch: every row in its own length, zeros behind it)
            xp, n_x = None, 0
        elif self.cfg.model == MODEL_USER:   # whole rows [n_x][n_cols]; the result's x is their column 0
            x = self._user_rows(x)
            self._pr_x = np.tile(x[:, 0], (len(self._pr_chains), 1))
            xp, n_x = x.ctypes.data_as(capi._dp), len(x)
        else:
            x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
            self._pr_x = np.tile(x, (len(self._pr_chains), 1))
            xp, n_x = x.ctypes.data_as(capi._dp), len(x)
        cfg = capi.PredictConfig(n_keep=len(self._pr_chains), chains=self._pr_chains.ctypes.data_as(C.POINTER(C.c_int32)),
                                 n_x=n_x, x=xp, nbins=self._pr_nbins, lo=self._pr_lo, hi=self._pr_hi)
        capi.check(self.L.apemost_hip_predict_begin(self._h, C.byref(cfg)))

    def predict_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2]; asynchronous
        (predict() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_predict_accumulate(self._h, d_samples, n_steps, skip, thin))

    def predict(self):
        """the fold so far as a Predict object (synchronises with the accumulates issued so far)"""
        from .predict import Predict
        pr = Predict.empty(self._pr_chains, self._pr_x, self.n_par, self.cfg.model, self._pr_nbins, self._pr_lo,
                           self._pr_hi, self._pr_thin, self.n_ladders)
        capi.check(self.L.apemost_hip_predict_get(self._h, C.byref(pr.view())))
        pr.lengths = self._fold_lengths(self.L.apemost_hip_predict_lengths, pr.n_keep, pr.n_x)
        return pr

    def _fold_lengths(self, call, n_keep, width):
        """a fold's lengths [n_keep] where they are not all the width of its arrays (a ragged batch), else None"""
        lens = np.zeros(n_keep, dtype=np.int32)
        capi.check(call(self._h, lens.ctypes.data_as(C.POINTER(C.c_int32))))
        return lens if np.any(lens != width) else None

    def predict_set(self, pr):
        """load a Predict (a resumed run) into the fold begun with the same configuration"""
        assert pr.hist.shape == self._pr_x.shape + (self._pr_nbins,) and pr.n_par == self.n_par
        assert np.array_equal(pr.chains, self._pr_chains)
        capi.check(self.L.apemost_hip_predict_set(self._h, C.byref(pr.view())))

    def predict_end(self):
        capi.check(self.L.apemost_hip_predict_end(self._h))

    def predict_curve(self, params, x=None):
        """the model curve [n][n_x] of the parameter rows params [n][n_par] (or one row) at x (None: column 0 of the
        data, of ladder 0 in a batch), evaluated on the device by the fold's own curve function"""
        params = np.ascontiguousarray(params, dtype=np.float64)
        one = params.ndim == 1
        params = params.reshape(-1, self.n_par)
        if x is None:
            xp, n_x = None, self.n_data_per_ladder[0]
        elif self.cfg.model == MODEL_USER:
            x = self._user_rows(x)
            xp, n_x = x.ctypes.data_as(capi._dp), len(x)
        else:
            x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
            xp, n_x = x.ctypes.data_as(capi._dp), len(x)
        out = np.zeros((len(params), n_x))
        capi.check(self.L.apemost_hip_predict_curve(self._h, len(params), params.ctypes.data_as(capi._dp), n_x, xp,
                                                    out.ctypes.data_as(capi._dp)))
        return out[0] if one else out

    # -- on-device pointwise log-likelihood (apemost_amd/pointwise.py) -------------------------------
    def pointwise_begin(self, chains=(0,), thin=1, tail=None, at=None, joint=False):
        """start the fold of the pointwise log-likelihood of every datum (columns 0 and 1 of the data as they are now,
        for every kept chain those of its own ladder) over the kept samples of the local chains `chains` (strictly
        increasing).  The criteria mean what they say for a chain at beta = 1: chain 0, the default.  thin is recorded
        in the result.  tail: also keep, per kept chain and datum, the largest leave-one-out log weights
        (pointwise_tail(), apemost_amd/psis.py): a capacity (2 .. 4096), or "auto:<expected kept samples>" for
        psis.capacity_for of that many; None keeps none.
        at: score the kept chains on the caller's data instead, held-out data the sampler was not fitted to
        (apemost_hip_pointwise_begin_at, apemost_amd/kfold.py): a list of one [n_at][2] matrix (x, y) per kept chain, or
        one matrix for all of them.  m_up + ln(S_up / n) is then the held-out log predictive density of every datum;
        the _dn words and DIC have no meaning there.  joint (with at): also the joint predictive density of every
        kept chain's block (pointwise_joint())."""
        self._pw_chains = np.ascontiguousarray(chains, dtype=np.int32)
        assert self._pw_chains.ndim == 1
        self._pw_thin = int(thin)
        cfg = capi.PointwiseConfig(n_keep=len(self._pw_chains),
                                   chains=self._pw_chains.ctypes.data_as(C.POINTER(C.c_int32)))
        self._pw_at = at is not None
        self._pw_joint = bool(joint)
        if at is None:
            if joint:
                raise ValueError("joint: the joint predictive of a block needs the block: pass at")
            lads = [int(c) // self.chains_per_ladder if self.n_ladders > 1 else 0
                    for c in self._pw_chains.tolist() if 0 <= c < self.n_chains]
            lads = lads if len(lads) == len(self._pw_chains) else [0] * len(self._pw_chains)
            # ([n_keep][2][n_data]; a ragged batch: every row in its own length, zeros behind it)
            self._pw_data = np.stack([_rectangle([self._x0[b] for b in lads]), _rectangle([self._y0[b] for b in lads])],
                                     axis=1)
            capi.check(self.L.apemost_hip_pointwise_begin(self._h, C.byref(cfg)))
        else:
            mats = [at] * len(self._pw_chains) if not isinstance(at, (list, tuple)) else list(at)
            mats = [np.ascontiguousarray(m, dtype=np.float64) for m in mats]
            if len(mats) != len(self._pw_chains) or any(m.ndim != 2 or m.shape[1] < 2 for m in mats):
                raise ValueError("at: one [n_at][2] matrix per kept chain (%d), or one matrix for all"
                                 % len(self._pw_chains))
            n_at = np.array([len(m) for m in mats], dtype=np.int32)
            x = np.ascontiguousarray(np.concatenate([m[:, 0] for m in mats])) if mats else np.zeros(0)
            y = np.ascontiguousarray(np.concatenate([m[:, 1] for m in mats])) if mats else np.zeros(0)
            self._pw_data = np.stack([_rectangle([m[:, 0] for m in mats]), _rectangle([m[:, 1] for m in mats])], axis=1)
            where = capi.PointwiseAt(n_at=n_at.ctypes.data_as(C.POINTER(C.c_int32)), x=x.ctypes.data_as(capi._dp),
                                     y=y.ctypes.data_as(capi._dp), joint=1 if joint else 0)
            capi.check(self.L.apemost_hip_pointwise_begin_at(self._h, C.byref(cfg), C.byref(where)))
        if tail is not None:
            self.pointwise_tail_begin(tail)

    def pointwise_tail_begin(self, tail):
        """attach a tail to the open fold, before its first accumulate or right behind pointwise_set (then
        pointwise_tail_set must follow); `tail` as in pointwise_begin"""
        from . import psis
        if isinstance(tail, str):
            kind, _, expected = tail.partition(":")
            if kind != "auto" or not expected.strip().isdigit():
                raise ValueError("tail %r: a capacity or \"auto:<expected kept samples>\"" % (tail,))
            tail = psis.capacity_for(int(expected))
        capi.check(self.L.apemost_hip_pointwise_tail_begin(self._h, int(tail)))

    def pointwise_tail_capacity(self):
        """the capacity of the open fold's tail, 0 where there is none"""
        c = C.c_int32(0)
        capi.check(self.L.apemost_hip_pointwise_tail_capacity(self._h, C.byref(c)))
        return c.value

    def pointwise_tail(self):
        """the tail so far as a psis.PointwiseTail (synchronises with the accumulates issued so far)"""
        from .psis import PointwiseTail
        n = C.c_uint64(0)
        capi.check(self.L.apemost_hip_pointwise_get(self._h, C.byref(capi.PointwiseView(n=C.pointer(n)))))
        t = PointwiseTail.empty(self._pw_chains, self._pw_data.shape[2], self.pointwise_tail_capacity(), n.value, self._pw_thin,
                                self.n_ladders)
        capi.check(self.L.apemost_hip_pointwise_tail_get(self._h, C.byref(t.view())))
        t.clear_unused()
        return t

    def pointwise_tail_set(self, tail):
        """load a PointwiseTail (a resumed run) into the tail begun with the same capacity"""
        assert tail.count.shape == self._pw_data[:, 0].shape and np.array_equal(tail.chains, self._pw_chains)
        assert tail.capacity == self.pointwise_tail_capacity()
        capi.check(self.L.apemost_hip_pointwise_tail_set(self._h, C.byref(tail.view())))

    def pointwise_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2]; asynchronous
        (pointwise() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_pointwise_accumulate(self._h, d_samples, n_steps, skip, thin))

    def pointwise(self, at_mean=True):
        """the fold so far as a Pointwise object (synchronises with the accumulates issued so far).  at_mean: also
        evaluate the term at every kept chain's posterior mean parameters, which DIC needs, on the device: one
        pointwise_loglike call, or in a batch one per kept chain over its own ladder's data (not part of the device
        state)."""
        from .pointwise import Pointwise
        pw = Pointwise.empty(self._pw_chains, self._pw_data[:, 0], self._pw_data[:, 1], self.n_par, self.cfg.model,
                             self.cfg.sigma, self._pw_thin, self.n_ladders)
        capi.check(self.L.apemost_hip_pointwise_get(self._h, C.byref(pw.view())))
        pw.lengths = self._fold_lengths(self.L.apemost_hip_pointwise_lengths, pw.n_keep, pw.n_data)
        pw.heldout = getattr(self, "_pw_at", False)   # (DIC has no held-out meaning: at_mean stays NaN, dic raises)
        if at_mean and int(pw.n[0]) > 0 and not pw.heldout:
            if self.n_ladders == 1:
                pw.at_mean = self.pointwise_loglike(pw.par_mean_all()).reshape(pw.n_keep, pw.n_data)
            else:
                for k in range(pw.n_keep):
                    b = int(pw.chains[k]) // self.chains_per_ladder
                    pw.at_mean[k, :self.n_data_per_ladder[b]] = self.pointwise_loglike(pw.par_mean(k), b)
        return pw

    def pointwise_set(self, pw):
        """load a Pointwise (a resumed run) into the fold begun with the same configuration"""
        assert pw.origin.shape == self._pw_data[:, 0].shape and pw.n_par == self.n_par
        assert np.array_equal(pw.chains, self._pw_chains)
        capi.check(self.L.apemost_hip_pointwise_set(self._h, C.byref(pw.view())))

    def pointwise_end(self):
        capi.check(self.L.apemost_hip_pointwise_end(self._h))

    def pointwise_joint(self):
        """the joint predictive state of every kept chain's block so far, a kfold.Joint (a fold begun with at and
        joint=True; synchronises with the accumulates issued so far)"""
        from .kfold import Joint
        jt = Joint.empty(self._pw_chains, self._pw_lengths(), self._pw_thin)
        capi.check(self.L.apemost_hip_pointwise_joint_get(self._h, C.byref(jt.view())))
        return jt

    def _pw_lengths(self):
        lens = np.zeros(len(self._pw_chains), dtype=np.int32)
        capi.check(self.L.apemost_hip_pointwise_lengths(self._h, lens.ctypes.data_as(C.POINTER(C.c_int32))))
        return lens

    def pointwise_joint_set(self, jt):
        """load a kfold.Joint (a resumed run) behind pointwise_set, into a fold begun with the same configuration"""
        assert np.array_equal(jt.chains, self._pw_chains)
        capi.check(self.L.apemost_hip_pointwise_joint_set(self._h, C.byref(jt.view())))

    def pointwise_loglike_at(self, params, x, y):
        """the pointwise log-likelihood [n][n_x] of the parameter rows params [n][n_par] (or one row) over the caller's
        data x, y [n_x], evaluated on the device by the fold's own term: what a fold begun with `at` folds"""
        params = np.ascontiguousarray(params, dtype=np.float64)
        one = params.ndim == 1
        params = np.ascontiguousarray(params.reshape(-1, self.n_par))
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if len(x) != len(y):
            raise ValueError("x holds %d values, y %d" % (len(x), len(y)))
        out = np.zeros((len(params), len(x)))
        capi.check(self.L.apemost_hip_pointwise_loglike_at(self._h, len(params), params.ctypes.data_as(capi._dp), len(x),
                                                           x.ctypes.data_as(capi._dp), y.ctypes.data_as(capi._dp),
                                                           out.ctypes.data_as(capi._dp)))
        return out[0] if one else out

    def pointwise_loglike(self, params, ladder=0):
        """the pointwise log-likelihood [n][n_data] of the parameter rows params [n][n_par] (or one row) over the
        sampler's data (of ladder `ladder` in a batch), evaluated on the device by the fold's own term"""
        params = np.ascontiguousarray(params, dtype=np.float64)
        one = params.ndim == 1
        params = np.ascontiguousarray(params.reshape(-1, self.n_par))
        out = np.zeros((len(params), self.n_data_per_ladder[ladder if 0 <= ladder < self.n_ladders else 0]))
        capi.check(self.L.apemost_hip_pointwise_loglike_ladder(self._h, int(ladder), len(params),
                                                               params.ctypes.data_as(capi._dp),
                                                               out.ctypes.data_as(capi._dp)))
        return out[0] if one else out

    # -- on-device predictive checks (apemost_amd/check.py) ---------------------------------------------
    def check_begin(self, chains=(0,), nbins=256, edges=None, thin=1):
        """start the fold of the predictive checks (apemost_amd/check.py, apemost_amd/csrc/pt_check.h) over the kept samples
        of the local chains `chains` (strictly increasing), each on columns 0 and 1 of its own ladder's data as they are
        now: per datum the predictive CDF at the observed value (PIT, leave-one-out PIT, the residual's moments), per
        kept sample the three discrepancy statistics FIT, EXTREME and SERIAL, histogrammed over nbins slots.  edges
        [3][nbins - 1]: the slots' edges per statistic; None: the null quantiles j / nbins of check.null_edges for the
        kept chains' data length, so that the histogram is that of the posterior predictive p-value.  nbins = 1 keeps no
        histogram.  The checks mean what they say for a chain at beta = 1: chain 0, the default."""
        from . import check as ck
        self._ck_chains = np.ascontiguousarray(chains, dtype=np.int32)
        assert self._ck_chains.ndim == 1
        self._ck_thin = int(thin)
        lads = [int(c) // self.chains_per_ladder if self.n_ladders > 1 else 0
                for c in self._ck_chains.tolist() if 0 <= c < self.n_chains]
        lads = lads if len(lads) == len(self._ck_chains) else [0] * len(self._ck_chains)
        self._ck_data = np.stack([_rectangle([self._x0[b] for b in lads]), _rectangle([self._y0[b] for b in lads])], axis=1)
        if edges is None:
            n_edges = int(nbins) - 1
            lens = sorted({len(self._x0[b]) for b in lads})
            if n_edges > 0 and len(lens) > 1:
                raise ValueError("the kept chains' ladders hold %s data: the null quantiles depend on the length; pass "
                                 "edges, or begin one fold per length" % lens)
            edges = (np.stack([ck.null_edges(self.cfg.model, q, lens[0], n_edges) for q in range(ck.N_STATS)])
                     if n_edges > 0 and lens else np.zeros((ck.N_STATS, 0)))
        edges = np.ascontiguousarray(edges, dtype=np.float64)
        if edges.ndim != 2 or edges.shape[0] != ck.N_STATS:
            raise ValueError("edges: [3][n_edges], one ascending row per statistic")
        self._ck_edges = edges
        capi.check(self.L.apemost_hip_check_begin(self._h, len(self._ck_chains),
                                                  self._ck_chains.ctypes.data_as(C.POINTER(C.c_int32)), edges.shape[1],
                                                  edges.ctypes.data_as(capi._dp) if edges.shape[1] else None))

    def check_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2]; asynchronous
        (check() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_check_accumulate(self._h, d_samples, n_steps, skip, thin))

    def check(self):
        """the fold so far as a check.Check (synchronises with the accumulates issued so far)"""
        from .check import Check
        c = Check.empty(self._ck_chains, self._ck_data[:, 0], self._ck_data[:, 1], self._ck_edges, self.cfg.model,
                        self.cfg.sigma, self._ck_thin, self.n_ladders)
        capi.check(self.L.apemost_hip_check_get(self._h, C.byref(c.view())))
        c.lengths = self._fold_lengths(self.L.apemost_hip_check_lengths, c.n_keep, c.n_data)
        return c

    def check_set(self, c):
        """load a Check (a resumed run) into the fold begun with the same configuration"""
        assert c.origin.shape == self._ck_data[:, 0].shape and np.array_equal(c.chains, self._ck_chains)
        assert c.edges.tobytes() == self._ck_edges.tobytes()
        capi.check(self.L.apemost_hip_check_set(self._h, C.byref(c.view())))

    def check_end(self):
        capi.check(self.L.apemost_hip_check_end(self._h))

    def check_values(self, params, x, y):
        """(e, u, T): the residual e and the predictive CDF u, [n][n_x] each, and the three statistics T [n][3] of the
        parameter rows params [n][n_par] (or one row) over the caller's data x, y [n_x], by the fold's own device
        functions: the stated meaning of what check_accumulate folds"""
        params = np.ascontiguousarray(params, dtype=np.float64)
        one = params.ndim == 1
        params = np.ascontiguousarray(params.reshape(-1, self.n_par))
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        if len(x) != len(y):
            raise ValueError("x holds %d values, y %d" % (len(x), len(y)))
        e, u, T = np.zeros((len(params), len(x))), np.zeros((len(params), len(x))), np.zeros((len(params), 3))
        capi.check(self.L.apemost_hip_check_values(self._h, len(params), params.ctypes.data_as(capi._dp), len(x),
                                                   x.ctypes.data_as(capi._dp), y.ctypes.data_as(capi._dp),
                                                   e.ctypes.data_as(capi._dp), u.ctypes.data_as(capi._dp),
                                                   T.ctypes.data_as(capi._dp)))
        return (e[0], u[0], T[0]) if one else (e, u, T)

    # -- on-device residual periodogram (apemost_amd/periodogram.py) -------------------------------------
    def periodogram_begin(self, chains=(0,), freqs=None, kind="lomb_scargle", sigma=None, weights=None, level=np.inf,
                          thin=1):
        """start the fold of the residual periodogram (apemost_amd/periodogram.py, apemost_amd/csrc/pt_periodogram.h) over
        the kept samples of the local chains `chains` (strictly increasing), each on columns 0 and 1 of its own ladder's
        data as they are now: per kept sample the power of y - model on the frequencies `freqs` [n_freq] (any doubles, in
        any order), folded per frequency into moments, extremes, the coherent amplitude and the count above `level` (one
        number, or one per kept chain), and per kept chain into the histogram of the highest peak's frequency.  weights
        [n_keep][n_freq][3] (or [n_freq][3] for every kept chain): the quadratic form's; None: periodogram.weights of
        `kind` over each kept chain's abscissae with `sigma` (None: the sampler's).  simplesin and sine3 only."""
        from . import periodogram as pg
        if freqs is None:
            raise ValueError("freqs: the frequency grid [n_freq]")
        self._pg_chains = np.ascontiguousarray(chains, dtype=np.int32)
        assert self._pg_chains.ndim == 1
        self._pg_thin = int(thin)
        n_keep = len(self._pg_chains)
        self._pg_freqs = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        lads = [int(c) // self.chains_per_ladder if self.n_ladders > 1 else 0
                for c in self._pg_chains.tolist() if 0 <= c < self.n_chains]
        lads = lads if len(lads) == n_keep else [0] * n_keep
        sigma = self.cfg.sigma if sigma is None else float(sigma)
        if weights is None:
            by_ladder = {b: pg.weights(self._x0[b], self._pg_freqs, kind, sigma) for b in sorted(set(lads))}
            weights = np.stack([by_ladder[b] for b in lads]) if lads else np.zeros((0, len(self._pg_freqs), 3))
        weights = np.asarray(weights, dtype=np.float64)
        if weights.ndim == 2:
            weights = np.broadcast_to(weights, (n_keep,) + weights.shape)
        if weights.shape != (n_keep, len(self._pg_freqs), 3):
            raise ValueError("weights: [n_keep][n_freq][3], here %r for %d kept chains and %d frequencies"
                             % (weights.shape, n_keep, len(self._pg_freqs)))
        self._pg_weights = np.ascontiguousarray(weights)
        self._pg_level = np.ascontiguousarray(np.broadcast_to(np.asarray(level, dtype=np.float64), (n_keep,)))
        self._pg_sigma = sigma
        capi.check(self.L.apemost_hip_periodogram_begin(self._h, n_keep, self._pg_chains.ctypes.data_as(C.POINTER(C.c_int32)),
                                                        len(self._pg_freqs), self._pg_freqs.ctypes.data_as(capi._dp),
                                                        self._pg_weights.ctypes.data_as(capi._dp),
                                                        self._pg_level.ctypes.data_as(capi._dp)))

    def periodogram_accumulate(self, d_samples, n_steps, skip=0, thin=1):
        """fold the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2]; asynchronous
        (periodogram() or a sample read's wait before the rows are overwritten)"""
        capi.check(self.L.apemost_hip_periodogram_accumulate(self._h, d_samples, n_steps, skip, thin))

    def periodogram(self):
        """the fold so far as a periodogram.Periodogram (synchronises with the accumulates issued so far)"""
        from .periodogram import Periodogram
        lens = np.zeros(len(self._pg_chains), dtype=np.int32)
        capi.check(self.L.apemost_hip_periodogram_lengths(self._h, lens.ctypes.data_as(C.POINTER(C.c_int32))))
        p = Periodogram.empty(self._pg_chains, self._pg_freqs, self._pg_weights, self._pg_level, lens, self.cfg.model,
                              self._pg_sigma, self._pg_thin, self.n_ladders)
        capi.check(self.L.apemost_hip_periodogram_get(self._h, C.byref(p.view())))
        return p

    def periodogram_set(self, p):
        """load a Periodogram (a resumed run) into the fold begun with the same configuration"""
        assert np.array_equal(p.chains, self._pg_chains) and p.freqs.tobytes() == self._pg_freqs.tobytes()
        assert p.weights.tobytes() == self._pg_weights.tobytes() and p.level.tobytes() == self._pg_level.tobytes()
        capi.check(self.L.apemost_hip_periodogram_set(self._h, C.byref(p.view())))

    def periodogram_end(self):
        capi.check(self.L.apemost_hip_periodogram_end(self._h))

    def periodogram_values(self, params, x, y, freqs, weights):
        """a dict of r [n][n_x], the table c, s [n_freq][n_x], C, S, P [n][n_freq], peak [n] and arg [n] (int32) of the
        parameter rows params [n][n_par] over the caller's data x, y [n_x], frequencies [n_freq] and weights
        [n_freq][3], by the fold's own device functions: the stated meaning of what periodogram_accumulate folds"""
        params = np.ascontiguousarray(np.asarray(params, dtype=np.float64).reshape(-1, self.n_par))
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1)
        y = np.ascontiguousarray(y, dtype=np.float64).reshape(-1)
        freqs = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        weights = np.ascontiguousarray(weights, dtype=np.float64)
        if len(x) != len(y):
            raise ValueError("x holds %d values, y %d" % (len(x), len(y)))
        if weights.shape != (len(freqs), 3):
            raise ValueError("weights: [n_freq][3], here %r for %d frequencies" % (weights.shape, len(freqs)))
        n, nx, nf = len(params), len(x), len(freqs)
        out = dict(r=np.zeros((n, nx)), c=np.zeros((nf, nx)), s=np.zeros((nf, nx)), C=np.zeros((n, nf)), S=np.zeros((n, nf)),
                   P=np.zeros((n, nf)), peak=np.zeros(n), arg=np.zeros(n, dtype=np.int32))
        dp = capi._dp
        capi.check(self.L.apemost_hip_periodogram_values(
            self._h, n, params.ctypes.data_as(dp), nx, x.ctypes.data_as(dp), y.ctypes.data_as(dp), nf,
            freqs.ctypes.data_as(dp), weights.ctypes.data_as(dp), *[out[f].ctypes.data_as(dp) for f in "rcsCSP"],
            out["peak"].ctypes.data_as(dp), out["arg"].ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    # -- the reference's text dumps, formatted on the device (apemost_amd/csrc/pt_text.h) -----------------
    def samples_text_bound(self, n_steps, skip=0, thin=1, n_param_chains=1):
        """(streams, host text bytes, device scratch bytes) of one samples_text batch"""
        v = [C.c_uint64(0) for _ in range(3)]
        capi.check(self.L.apemost_hip_samples_text_bound(self._h, n_steps, skip, thin, n_param_chains,
                                                         *[C.byref(x) for x in v]))
        return tuple(x.value for x in v)

    def samples_text(self, d_samples, n_steps, skip=0, thin=1, n_param_chains=1):
        """the kept steps skip, skip + thin, ... of the device rows [n_steps][n_chains][n_par+2] as the lines of
        the reference's text dumps, formatted on the device: one bytes object per file -- "%.15e\\n" of parameter
        p of chain c at index c*n_par + p for the chains 0 .. n_param_chains-1, then "%6e\\t%6e\\n" (prob,
        prob - prior) of every chain.  Synchronous."""
        import sys
        torch = sys.modules.get("torch")        # rows that torch has just written must be complete
        if torch is not None and torch.cuda.is_available():
            torch.cuda.current_stream().synchronize()
        n_streams, text_bytes, scratch_bytes = self.samples_text_bound(n_steps, skip, thin, n_param_chains)
        scratch = C.c_void_p()
        capi.check(self.L.apemost_hip_device_alloc(self._h, scratch_bytes, C.byref(scratch)))
        text = np.zeros(max(text_bytes, 1), dtype=np.uint8)
        offsets = np.zeros(n_streams + 1, dtype=np.uint64)
        try:
            capi.check(self.L.apemost_hip_samples_text_read_async(
                self._h, d_samples, n_steps, skip, thin, n_param_chains, scratch, scratch_bytes,
                text.ctypes.data, text_bytes, offsets.ctypes.data_as(capi._up), n_streams + 1))
            capi.check(self.L.apemost_hip_samples_wait(self._h))
        finally:
            capi.check(self.L.apemost_hip_device_free(self._h, scratch))
        raw = text.tobytes()
        return [raw[int(offsets[i]):int(offsets[i + 1])] for i in range(n_streams)]

    def edge_export(self, side, d_buf):
        capi.check(self.L.apemost_hip_edge_export(self._h, side, d_buf))

    def edge_import(self, side, d_buf):
        capi.check(self.L.apemost_hip_edge_import(self._h, side, d_buf))

    # -- calibration ----------------------------------------------------------------
    def markov_chain_calibrate(self, first, count, cfg=None, burn_in_only=False):
        """markov_chain_calibrate() for chains [first, first+count).  Unless cfg names another chain
        (progress_chain >= 0), the readjustments of the LAST chain of the range are logged: the
        reference reopens calibration_progress.data "w" for every chain it calibrates
        (src/markov_chain_calibrate.c:1052), so that chain's lines are the ones a single-threaded
        run leaves behind (calibration_progress_text)."""
        src = cfg or capi.calib_defaults()
        cfg = capi.CalibConfig()
        C.pointer(cfg)[0] = src
        if cfg.progress_chain < 0 and not burn_in_only:
            cfg.progress_chain = first + count - 1
        status = np.zeros(count, dtype=np.int32)
        iters = np.zeros(count, dtype=np.uint64)
        rc = self.L.apemost_hip_calibrate_chains(self._h, first, count, C.byref(cfg), int(burn_in_only),
                                                 status.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 iters.ctypes.data_as(C.POINTER(C.c_uint64)))
        if rc not in (capi.OK, capi.ERR_CALIBRATION):
            capi.check(rc)
        if not burn_in_only:
            self._progress_text = self._format_progress(self.calibrate_progress())
        return status, iters

    def _format_progress(self, rows):
        """the line format of src/markov_chain_calibrate.c:1143-1146: "%d\t%lu\t%f\t%f\t%f\n" of
        (parameter, iter, normalised step, accept rate, -1.)"""
        return "".join("%d\t%d\t%f\t%f\t%f\n" % (i, int(r[0]), r[1 + 2 * i], r[2 + 2 * i], -1.0)
                       for r in rows for i in range(self.n_par))

    def calibration_progress_text(self):
        """contents of calibration_progress.data after the calibrations made so far"""
        return getattr(self, "_progress_text", "")

    def calibrate_progress(self):
        """rows (iter, then (normalised step, accept rate) per parameter) of the chain named by
        cfg.progress_chain in the latest calibration: what the reference writes to
        calibration_progress.data (src/markov_chain_calibrate.c:1143-1146)"""
        n = C.c_int32(0)
        capi.check(self.L.apemost_hip_calibrate_progress(self._h, None, 0, C.byref(n)))
        rows = np.zeros((n.value, 1 + 2 * self.n_par))
        if n.value:
            capi.check(self.L.apemost_hip_calibrate_progress(self._h, rows.ctypes.data_as(C.POINTER(C.c_double)),
                                                             n.value, C.byref(n)))
        return rows

    def calibrate_stats(self):
        """(segments, likelihood evaluations, launches per waves-per-chain) of the latest calibration;
        self.calibrate_seconds_by_waves holds the wall seconds per waves-per-chain"""
        seg, ev = C.c_uint64(0), C.c_uint64(0)
        by = (C.c_uint64 * 9)()
        sec = (C.c_double * 9)()
        capi.check(self.L.apemost_hip_calibrate_stats(self._h, C.byref(seg), C.byref(ev), by, sec))
        self.calibrate_seconds_by_waves = {w: float(sec[w]) for w in range(9) if by[w]}
        return seg.value, ev.value, {w: int(by[w]) for w in range(9) if by[w]}

    def calibrate_first(self, cfg=None):
        """calibrate_first(): calc_model(chain 0) then markov_chain_calibrate(chain 0)."""
        self.calc_model(0, 1)
        status, _ = self.markov_chain_calibrate(0, 1, cfg)
        return int(status[0])

    def calibrate_rest(self, cfg=None, ladder_kind=LADDER_CHEBYSHEV_BETA, beta_0=-0.001,
                       skip_calibrate_allchains=False):
        """calibrate_rest() for a whole ladder on this device.  Entry state: chain 0 carries the
        calibrated steps/params (read_calibration_file(chains, 1)), every beta = 1."""
        assert self.n_ladders == 1 and self.n_chains == self.n_chains_global and self.chain_offset == 0
        from .distributed import calibrate_rest_sharded
        return calibrate_rest_sharded(self, self.n_chains, 0, cfg, ladder_kind, beta_0, skip_calibrate_allchains)
