"""ctypes binding of the C ABI in include/apemost_hip.h (libapemost_hip.so).

This is plumbing only: every call goes straight to the HIP library.  There is no
Python or CPU implementation behind it -- if the library is missing or no gfx950
device is present, calls raise ApemostHipError.
"""
import ctypes as C
import os

import numpy as np

from . import build as _build

ABI_VERSION = 3
FLAG_SINGLE_ROUND_LAUNCHES, FLAG_COOPERATIVE_LAUNCH, FLAG_TWO_BARRIER_STEP = 1, 2, 4
# the reference's compile-time variants (-DPROPOSAL_LOGISTIC, -DPROPOSAL_UNIFORM, -DRANDOMSWAP, -DADAPT)
FLAG_PROPOSAL_LOGISTIC, FLAG_PROPOSAL_UNIFORM, FLAG_RANDOMSWAP, FLAG_ADAPT = 8, 16, 32, 64
FLAG_TEST_REFUSE_COOPERATIVE, FLAG_TEST_WITHHOLD_PUBLISH = 128, 256   # test hooks (include/apemost_hip.h)
FLAG_RWM = 512
FLAG_USER_ONE_BARRIER = 1024   # APEMOST_MODEL_USER in the one-barrier kernels (include/apemost_hip.h)
FLAG_SWAP_EVEN_ODD = 2048      # even-odd swap sweeps: every pair of the sweep's parity each round (include/apemost_hip.h)
FLAG_TRACK_REPLICAS = 4096     # replica-flow tracking: round trips and up / down moves per rung (include/apemost_hip.h)
OK, ERR_INVALID, ERR_NO_DEVICE, ERR_RUNTIME, ERR_UNSUPPORTED, ERR_CALIBRATION = 0, -1, -2, -3, -4, -5

_dp = C.POINTER(C.c_double)
_up = C.POINTER(C.c_uint64)


class ApemostHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("apemost_hip error %d: %s" % (code, msg))
        self.code = code


class Config(C.Structure):
    _fields_ = [("abi_version", C.c_int32), ("device", C.c_int32), ("model", C.c_int32),
                ("n_par", C.c_int32), ("n_chains", C.c_int32), ("n_data", C.c_int32),
                ("n_cols", C.c_int32), ("waves_per_chain", C.c_int32), ("lds_policy", C.c_int32),
                ("flags", C.c_int32), ("chain_offset", C.c_int64),
                ("n_chains_global", C.c_int64), ("seed", C.c_uint64), ("sigma", C.c_double),
                ("hmin", C.c_double), ("circular_params", C.c_uint64), ("adapt_target", C.c_double),
                ("device_model_source", C.c_char_p)]


class StateView(C.Structure):
    _fields_ = [("params", _dp), ("params_best", _dp), ("step", _dp), ("pmin", _dp), ("pmax", _dp),
                ("params_accepts", _up), ("params_rejects", _up), ("beta", _dp), ("prob", _dp),
                ("prior", _dp), ("prob_best", _dp), ("accept", _up), ("reject", _up), ("n_iter", _up),
                ("swapcount", _up), ("ticks", _up)]


class CalibConfig(C.Structure):
    _fields_ = [("burn_in_iterations", C.c_uint32), ("iter_limit", C.c_uint32),
                ("iter_readjust", C.c_uint32), ("no_rescaling_limit", C.c_int32),
                ("rat_limit", C.c_double), ("target_global", C.c_double),
                ("max_ar_deviation", C.c_double), ("mul", C.c_double), ("adjust_step", C.c_double),
                ("progress_chain", C.c_int32), ("reserved", C.c_int32)]


class SummaryConfig(C.Structure):
    _fields_ = [("n_hist_chains", C.c_int32), ("nbins", C.c_int32), ("batch_size", C.c_uint64),
                ("max_batches", C.c_uint64), ("lo", _dp), ("hi", _dp)]


class SummaryView(C.Structure):
    _fields_ = [("n", _up), ("prob_sum", _dp), ("hist", _up), ("batch_sums", _dp), ("n_batches", _up)]


class PeaksConfig(C.Structure):
    _fields_ = [("n_keep", C.c_int32), ("chains", C.POINTER(C.c_int32)), ("capacity", C.c_uint64), ("lo", _dp), ("hi", _dp)]


class PeaksView(C.Structure):
    _fields_ = [("n", _up), ("n_values", _up), ("n_peaks", C.POINTER(C.c_uint32)), ("left", _up), ("right", _up),
                ("q", _dp), ("q_set", C.POINTER(C.c_uint8))]


class JointConfig(C.Structure):
    _fields_ = [("n_keep", C.c_int32), ("chains", C.POINTER(C.c_int32)), ("nbins", C.c_int32), ("n_pairs", C.c_int32),
                ("pairs", C.POINTER(C.c_int32)), ("lo", _dp), ("hi", _dp)]


class JointView(C.Structure):
    _fields_ = [("n", _up), ("counts", _up), ("origin", _dp), ("sum", _dp), ("cross", _dp)]


class EvidenceConfig(C.Structure):
    _fields_ = [("batch_size", C.c_uint64), ("max_batches", C.c_uint64), ("coef_up", _dp), ("coef_down", _dp)]


class EvidenceView(C.Structure):
    _fields_ = [("n", _up), ("origin", _dp), ("sum", _dp), ("sq", _dp), ("batch", _dp), ("m", _dp), ("S", _dp)]


class MbarConfig(C.Structure):
    _fields_ = [("capacity", C.c_uint64), ("betas", _dp)]


class MbarView(C.Structure):
    _fields_ = [("n", _up), ("n_bad", _up), ("ell", _dp)]


class MbarSums(C.Structure):
    _fields_ = [("m", _dp), ("S0", _dp), ("S1", _dp), ("S2", _dp), ("SS", _dp), ("G", _dp), ("ell_first", _dp)]


class ReweightConfig(C.Structure):
    _fields_ = [("n_cols", C.c_int32), ("cols", C.POINTER(C.c_int32)), ("nbins", C.c_int32), ("lo", _dp), ("hi", _dp)]


class ReweightView(C.Structure):
    _fields_ = [("n", _up), ("n_bad", _up), ("x", _dp)]


class ReweightSums(C.Structure):
    _fields_ = [("m", _dp), ("S0", _dp), ("SS", _dp), ("origin", _dp), ("S1", _dp), ("cross", _dp),
                ("shift", C.POINTER(C.c_int32)), ("hist", _up), ("q_total", _up)]


class ReweightDraws(C.Structure):
    _fields_ = [("index", C.POINTER(C.c_uint32)), ("x", _dp), ("q_total", _up), ("shift", C.POINTER(C.c_int32))]


class AutocorrConfig(C.Structure):
    _fields_ = [("n_keep", C.c_int32), ("chains", C.POINTER(C.c_int32)), ("max_lag", C.c_int32), ("n_cols", C.c_int32),
                ("cols", C.POINTER(C.c_int32))]


class AutocorrView(C.Structure):
    _fields_ = [("n", _up), ("origin", _dp), ("sum", _dp), ("lag", _dp), ("head", _dp), ("tail", _dp)]


class PredictConfig(C.Structure):
    _fields_ = [("n_keep", C.c_int32), ("chains", C.POINTER(C.c_int32)), ("n_x", C.c_int32), ("x", _dp),
                ("nbins", C.c_int32), ("lo", C.c_double), ("hi", C.c_double)]


class PredictView(C.Structure):
    _fields_ = [("n", _up), ("origin", _dp), ("sum", _dp), ("sq", _dp), ("vmin", _dp), ("vmax", _dp), ("hist", _up),
                ("best_prob", _dp), ("best_params", _dp), ("best_n", _up)]


class PointwiseConfig(C.Structure):
    _fields_ = [("n_keep", C.c_int32), ("chains", C.POINTER(C.c_int32))]


class PointwiseView(C.Structure):
    _fields_ = [("n", _up), ("origin", _dp), ("sum", _dp), ("sq", _dp), ("m_up", _dp), ("S_up", _dp), ("m_dn", _dp),
                ("S_dn", _dp), ("S2_dn", _dp), ("par_origin", _dp), ("par_sum", _dp)]


class PointwiseTailView(C.Structure):
    _fields_ = [("count", _up), ("values", _dp)]


class PointwiseAt(C.Structure):
    _fields_ = [("n_at", C.POINTER(C.c_int32)), ("x", _dp), ("y", _dp), ("joint", C.c_int32)]


class PointwiseJointView(C.Structure):
    _fields_ = [("n", _up), ("origin", _dp), ("sum", _dp), ("sq", _dp), ("m", _dp), ("S", _dp)]


class CheckView(C.Structure):
    _fields_ = [("n", _up), ("origin", _dp), ("sum", _dp), ("sq", _dp), ("sum_u", _dp), ("m", _dp), ("S", _dp), ("SU", _dp),
                ("stat_origin", _dp), ("stat_sum", _dp), ("stat_sq", _dp), ("stat_min", _dp), ("stat_max", _dp),
                ("counts", _up)]


class PeriodogramView(C.Structure):
    _fields_ = [("n", _up), ("origin", _dp), ("sum", _dp), ("sq", _dp), ("pmin", _dp), ("pmax", _dp), ("sum_c", _dp),
                ("sum_s", _dp), ("exceed", _up), ("peak_origin", _dp), ("peak_sum", _dp), ("peak_sq", _dp), ("peak_min", _dp),
                ("peak_max", _dp), ("peak_counts", _up)]


class DerivedConfig(C.Structure):
    _fields_ = [("n_keep", C.c_int32), ("chains", C.POINTER(C.c_int32)), ("n_col", C.c_int32),
                ("code", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32)), ("n_const", C.c_int32), ("consts", _dp),
                ("nbins", C.c_int32), ("n_pairs", C.c_int32), ("pairs", C.POINTER(C.c_int32)), ("lo", _dp), ("hi", _dp),
                ("batch_size", C.c_uint64), ("max_batches", C.c_uint64), ("stage_steps", C.c_uint64)]


class DerivedView(C.Structure):
    _fields_ = [("n", _up), ("hist", _up), ("batch", _dp), ("n_batches", _up), ("counts", _up), ("origin", _dp),
                ("sum", _dp), ("cross", _dp), ("nonfinite", _up), ("vmin", _dp), ("vmax", _dp)]


PEAKS_MAX = 99  # peaks described per column (include/apemost_hip.h)


class ReplicaFlowView(C.Structure):
    _fields_ = [("replica", C.POINTER(C.c_uint32)), ("heading", C.POINTER(C.c_uint32)), ("n_up", _up), ("n_down", _up),
                ("attempts", _up), ("round_trips", _up)]


# every symbol include/apemost_hip.h declares
EXPORTS = [
    "apemost_hip_last_error", "apemost_hip_abi_version", "apemost_hip_device_count",
    "apemost_hip_device_info", "apemost_hip_create", "apemost_hip_destroy", "apemost_hip_synchronize",
    "apemost_hip_stream", "apemost_hip_waves_per_chain", "apemost_hip_launch_policy", "apemost_hip_user_model_compile_seconds", "apemost_hip_user_hooks", "apemost_hip_set_chain_offset", "apemost_hip_set_data", "apemost_hip_set_state",
    "apemost_hip_get_state", "apemost_hip_set_round", "apemost_hip_get_round", "apemost_hip_calc_model",
    "apemost_hip_loglike", "apemost_hip_launch_round", "apemost_hip_launch_rounds", "apemost_hip_max_rounds_per_launch",
    "apemost_hip_launch_round_for", "apemost_hip_run", "apemost_hip_samples_alloc",
    "apemost_hip_samples_read", "apemost_hip_samples_free", "apemost_hip_samples_read_async",
    "apemost_hip_samples_wait", "apemost_hip_samples_pack_read_async", "apemost_hip_host_alloc", "apemost_hip_host_free", "apemost_hip_swap_pair",
    "apemost_hip_sampler_swap_pair", "apemost_hip_rounds_within_shard",
    "apemost_hip_edge_doubles", "apemost_hip_edge_export", "apemost_hip_edge_import",
    "apemost_hip_edge_exchange", "apemost_hip_run_shards",
    "apemost_hip_calib_defaults", "apemost_hip_calibrate_chains", "apemost_hip_calibrate_begin",
    "apemost_hip_calibrate_end", "apemost_hip_calibrate_poll", "apemost_hip_calibrate_cancel", "apemost_hip_calibrate_wait_any",
    "apemost_hip_calibrate_progress", "apemost_hip_calibrate_stats", "apemost_hip_rng_raw",
    "apemost_hip_rng_attempts", "apemost_hip_timer_begin", "apemost_hip_timer_end",
    "apemost_hip_summary_begin", "apemost_hip_summary_accumulate", "apemost_hip_summary_get",
    "apemost_hip_summary_set", "apemost_hip_summary_end",
    "apemost_hip_samples_text_bound", "apemost_hip_samples_text_read_async", "apemost_hip_device_alloc",
    "apemost_hip_device_free",
    "apemost_hip_create_batch", "apemost_hip_n_ladders", "apemost_hip_set_data_ladder",
    "apemost_hip_create_batch_ragged", "apemost_hip_ragged_layout", "apemost_hip_ladder_n_data",
    "apemost_hip_predict_lengths", "apemost_hip_pointwise_lengths",
    "apemost_hip_replica_flow_get", "apemost_hip_replica_flow_set", "apemost_hip_replica_flow_reset",
    "apemost_hip_peaks_begin", "apemost_hip_peaks_accumulate", "apemost_hip_peaks_get", "apemost_hip_peaks_end",
    "apemost_hip_peaks_table",
    "apemost_hip_joint_begin", "apemost_hip_joint_accumulate", "apemost_hip_joint_get", "apemost_hip_joint_set",
    "apemost_hip_joint_end",
    "apemost_hip_evidence_begin", "apemost_hip_evidence_accumulate", "apemost_hip_evidence_get",
    "apemost_hip_evidence_set", "apemost_hip_evidence_end",
    "apemost_hip_mbar_begin", "apemost_hip_mbar_accumulate", "apemost_hip_mbar_get", "apemost_hip_mbar_set",
    "apemost_hip_mbar_end", "apemost_hip_mbar_iterate", "apemost_hip_mbar_evaluate", "apemost_hip_mbar_log_weights",
    "apemost_hip_reweight_begin", "apemost_hip_reweight_accumulate", "apemost_hip_reweight_get",
    "apemost_hip_reweight_set", "apemost_hip_reweight_end", "apemost_hip_reweight_evaluate",
    "apemost_hip_reweight_weights", "apemost_hip_reweight_resample",
    "apemost_hip_autocorr_begin", "apemost_hip_autocorr_accumulate", "apemost_hip_autocorr_get",
    "apemost_hip_autocorr_set", "apemost_hip_autocorr_end",
    "apemost_hip_predict_begin", "apemost_hip_predict_accumulate", "apemost_hip_predict_get",
    "apemost_hip_predict_set", "apemost_hip_predict_end", "apemost_hip_predict_curve",
    "apemost_hip_pointwise_begin", "apemost_hip_pointwise_accumulate", "apemost_hip_pointwise_get",
    "apemost_hip_pointwise_set", "apemost_hip_pointwise_end", "apemost_hip_pointwise_loglike",
    "apemost_hip_pointwise_loglike_ladder",
    "apemost_hip_pointwise_tail_begin", "apemost_hip_pointwise_tail_get", "apemost_hip_pointwise_tail_set",
    "apemost_hip_pointwise_tail_capacity",
    "apemost_hip_pointwise_begin_at", "apemost_hip_pointwise_joint_get", "apemost_hip_pointwise_joint_set",
    "apemost_hip_pointwise_loglike_at",
    "apemost_hip_derived_check", "apemost_hip_derived_begin", "apemost_hip_derived_accumulate",
    "apemost_hip_derived_get", "apemost_hip_derived_set", "apemost_hip_derived_end", "apemost_hip_derived_eval",
    "apemost_hip_check_begin", "apemost_hip_check_accumulate", "apemost_hip_check_get", "apemost_hip_check_set",
    "apemost_hip_check_lengths", "apemost_hip_check_end", "apemost_hip_check_values", "apemost_hip_check_null_edges",
    "apemost_hip_periodogram_begin", "apemost_hip_periodogram_accumulate", "apemost_hip_periodogram_get",
    "apemost_hip_periodogram_set", "apemost_hip_periodogram_lengths", "apemost_hip_periodogram_end",
    "apemost_hip_periodogram_values",
]

_lib = None


def library_path():
    return _build.HIP_LIB


def lib():
    """Load libapemost_hip.so (must have been built by apemost_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP runtime per process: PyTorch bundles its own libamdhip64 (same SONAME as the system
    # one this library links).  If torch is going to be used for device memory / RCCL plumbing it
    # must be loaded FIRST so that the dynamic linker resolves our DT_NEEDED to the copy already
    # in the process; two runtimes in one process cannot both open the GPU.
    # APEMOST_NO_TORCH=1: the caller will not use torch in this process (bench.py --no-torch, the profile
    # scripts): nothing to order, and the process then holds ONE HIP / HSA runtime -- under rocprofv3,
    # torch's bundled runtime next to the tool's was what aborted at exit (profiles/README.md).
    if not os.environ.get("APEMOST_NO_TORCH"):
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    path = library_path()
    if not os.path.exists(path):
        raise ApemostHipError(ERR_NO_DEVICE, "%s not built; run `python -m apemost_amd.build`" % path)
    L = C.CDLL(path)
    vp = C.c_void_p
    L.apemost_hip_last_error.restype = C.c_char_p
    L.apemost_hip_device_count.argtypes = [C.POINTER(C.c_int)]
    L.apemost_hip_device_info.argtypes = [C.c_int, C.c_char_p, C.c_size_t, C.POINTER(C.c_int), _up]
    L.apemost_hip_create.argtypes = [C.POINTER(Config), C.POINTER(vp)]
    L.apemost_hip_create_batch.argtypes = [C.POINTER(Config), C.c_int32, _up, C.POINTER(vp)]
    L.apemost_hip_create_batch_ragged.argtypes = [C.POINTER(Config), C.c_int32, _up, C.POINTER(C.c_int32), C.POINTER(vp)]
    L.apemost_hip_ragged_layout.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32), _up, C.POINTER(C.c_int32), _up]
    L.apemost_hip_ladder_n_data.argtypes = [vp, C.c_int32, C.POINTER(C.c_int32)]
    L.apemost_hip_predict_lengths.argtypes = [vp, C.POINTER(C.c_int32)]
    L.apemost_hip_pointwise_lengths.argtypes = [vp, C.POINTER(C.c_int32)]
    L.apemost_hip_n_ladders.argtypes = [vp, C.POINTER(C.c_int32)]
    L.apemost_hip_set_data_ladder.argtypes = [vp, C.c_int32, _dp]
    L.apemost_hip_destroy.argtypes = [vp]
    L.apemost_hip_synchronize.argtypes = [vp]
    L.apemost_hip_stream.argtypes = [vp, C.POINTER(vp)]
    L.apemost_hip_waves_per_chain.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.apemost_hip_launch_policy.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.apemost_hip_set_data.argtypes = [vp, _dp]
    L.apemost_hip_set_state.argtypes = [vp, C.POINTER(StateView)]
    L.apemost_hip_get_state.argtypes = [vp, C.POINTER(StateView)]
    L.apemost_hip_set_round.argtypes = [vp, C.c_uint64, C.c_int]
    L.apemost_hip_get_round.argtypes = [vp, _up, C.POINTER(C.c_int)]
    L.apemost_hip_calc_model.argtypes = [vp, C.c_int32, C.c_int32]
    L.apemost_hip_loglike.argtypes = [vp, C.c_int32, _dp, _dp, _dp, _dp]
    L.apemost_hip_launch_round.argtypes = [vp, C.c_uint32, C.c_int, vp]
    L.apemost_hip_launch_round_for.argtypes = [vp, C.c_uint32, C.c_int32, vp]
    L.apemost_hip_launch_rounds.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, vp]
    L.apemost_hip_max_rounds_per_launch.argtypes = [vp, C.POINTER(C.c_int32)]
    L.apemost_hip_run.argtypes = [vp, C.c_uint64, C.c_uint32, vp]
    L.apemost_hip_samples_alloc.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    L.apemost_hip_samples_read.argtypes = [vp, vp, C.c_uint64, _dp]
    L.apemost_hip_samples_free.argtypes = [vp, vp]
    L.apemost_hip_samples_read_async.argtypes = [vp, vp, C.c_uint64, vp, vp]
    L.apemost_hip_samples_pack_read_async.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, C.c_int32,
                                                      vp, vp, vp, _up]
    L.apemost_hip_samples_wait.argtypes = [vp]
    L.apemost_hip_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.apemost_hip_host_free.argtypes = [vp]
    L.apemost_hip_swap_pair.argtypes = [C.c_uint64, C.c_uint64, C.c_int64]
    L.apemost_hip_swap_pair.restype = C.c_int64
    L.apemost_hip_sampler_swap_pair.argtypes = [C.c_void_p, C.c_uint64]
    L.apemost_hip_sampler_swap_pair.restype = C.c_int64
    L.apemost_hip_rounds_within_shard.argtypes = [C.c_void_p, C.c_uint64, C.c_int64]
    L.apemost_hip_rounds_within_shard.restype = C.c_int64
    L.apemost_hip_edge_doubles.argtypes = [C.c_int32]
    L.apemost_hip_edge_doubles.restype = C.c_int32
    L.apemost_hip_edge_export.argtypes = [vp, C.c_int, vp]
    L.apemost_hip_edge_import.argtypes = [vp, C.c_int, vp]
    L.apemost_hip_edge_exchange.argtypes = [vp, vp]
    L.apemost_hip_run_shards.argtypes = [C.POINTER(vp), C.c_int32, C.c_uint64, C.c_uint32, C.POINTER(vp)]
    L.apemost_hip_calib_defaults.argtypes = [C.POINTER(CalibConfig)]
    L.apemost_hip_calib_defaults.restype = None
    L.apemost_hip_calibrate_chains.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(CalibConfig), C.c_int,
                                               C.POINTER(C.c_int32), _up]
    L.apemost_hip_calibrate_begin.argtypes = [vp, C.c_int32, C.c_int32, C.POINTER(CalibConfig), C.c_int]
    L.apemost_hip_calibrate_end.argtypes = [vp, C.POINTER(C.c_int32), _up]
    L.apemost_hip_calibrate_poll.argtypes = [vp, C.POINTER(C.c_int32)]
    L.apemost_hip_calibrate_cancel.argtypes = [vp]
    L.apemost_hip_calibrate_wait_any.argtypes = [C.POINTER(vp), C.c_int32, C.POINTER(C.c_int32)]
    L.apemost_hip_calibrate_progress.argtypes = [vp, _dp, C.c_int32, C.POINTER(C.c_int32)]
    L.apemost_hip_calibrate_stats.argtypes = [vp, _up, _up, _up, _dp]
    L.apemost_hip_rng_raw.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32,
                                      C.POINTER(C.c_uint32)]
    L.apemost_hip_rng_attempts.argtypes = [C.c_int, C.c_uint64, C.c_uint64, C.c_int32, C.c_uint64, C.c_uint64,
                                           C.c_int32, _dp, _dp, C.POINTER(C.c_int32), _dp]
    L.apemost_hip_user_model_compile_seconds.argtypes = [vp, _dp]
    L.apemost_hip_user_hooks.argtypes = [vp, C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp]
    L.apemost_hip_summary_begin.argtypes = [vp, C.POINTER(SummaryConfig)]
    L.apemost_hip_summary_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_summary_get.argtypes = [vp, C.POINTER(SummaryView)]
    L.apemost_hip_summary_set.argtypes = [vp, C.POINTER(SummaryView)]
    L.apemost_hip_summary_end.argtypes = [vp]
    L.apemost_hip_samples_text_bound.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, _up, _up, _up]
    L.apemost_hip_samples_text_read_async.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_int32, vp,
                                                      C.c_uint64, vp, C.c_uint64, _up, C.c_uint64]
    L.apemost_hip_device_alloc.argtypes = [vp, C.c_uint64, C.POINTER(vp)]
    L.apemost_hip_device_free.argtypes = [vp, vp]
    L.apemost_hip_replica_flow_get.argtypes = [vp, C.POINTER(ReplicaFlowView)]
    L.apemost_hip_replica_flow_set.argtypes = [vp, C.POINTER(ReplicaFlowView)]
    L.apemost_hip_replica_flow_reset.argtypes = [vp]
    L.apemost_hip_peaks_begin.argtypes = [vp, C.POINTER(PeaksConfig)]
    L.apemost_hip_peaks_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_peaks_get.argtypes = [vp, C.POINTER(PeaksView)]
    L.apemost_hip_peaks_end.argtypes = [vp]
    L.apemost_hip_peaks_table.argtypes = [C.POINTER(PeaksView), C.c_int32, C.c_int32, C.c_int32, _dp,
                                          C.POINTER(C.c_uint32)]
    L.apemost_hip_joint_begin.argtypes = [vp, C.POINTER(JointConfig)]
    L.apemost_hip_joint_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_joint_get.argtypes = [vp, C.POINTER(JointView)]
    L.apemost_hip_joint_set.argtypes = [vp, C.POINTER(JointView)]
    L.apemost_hip_joint_end.argtypes = [vp]
    L.apemost_hip_evidence_begin.argtypes = [vp, C.POINTER(EvidenceConfig)]
    L.apemost_hip_evidence_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_evidence_get.argtypes = [vp, C.POINTER(EvidenceView)]
    L.apemost_hip_evidence_set.argtypes = [vp, C.POINTER(EvidenceView)]
    L.apemost_hip_evidence_end.argtypes = [vp]
    L.apemost_hip_mbar_begin.argtypes = [vp, C.POINTER(MbarConfig)]
    L.apemost_hip_mbar_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_mbar_get.argtypes = [vp, C.POINTER(MbarView)]
    L.apemost_hip_mbar_set.argtypes = [vp, C.POINTER(MbarView)]
    L.apemost_hip_mbar_end.argtypes = [vp]
    L.apemost_hip_mbar_iterate.argtypes = [vp, C.c_uint64, C.c_uint64, C.c_uint32, _dp, _dp]
    L.apemost_hip_mbar_evaluate.argtypes = [vp, C.c_uint64, C.c_uint64, _dp, _dp, C.c_int32, C.POINTER(MbarSums)]
    L.apemost_hip_mbar_log_weights.argtypes = [vp, C.c_uint64, C.c_uint64, _dp, C.c_double, _dp]
    L.apemost_hip_reweight_begin.argtypes = [vp, C.POINTER(ReweightConfig)]
    L.apemost_hip_reweight_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_reweight_get.argtypes = [vp, C.POINTER(ReweightView)]
    L.apemost_hip_reweight_set.argtypes = [vp, C.POINTER(ReweightView)]
    L.apemost_hip_reweight_end.argtypes = [vp]
    L.apemost_hip_reweight_evaluate.argtypes = [vp, C.c_uint64, C.c_uint64, _dp, _dp, C.c_int32, C.POINTER(ReweightSums)]
    L.apemost_hip_reweight_weights.argtypes = [vp, C.c_uint64, C.c_uint64, _dp, C.c_double, _dp, _up]
    L.apemost_hip_reweight_resample.argtypes = [vp, C.c_uint64, C.c_uint64, _dp, C.c_double, C.c_uint32, C.c_uint64,
                                                C.POINTER(ReweightDraws)]
    L.apemost_hip_autocorr_begin.argtypes = [vp, C.POINTER(AutocorrConfig)]
    L.apemost_hip_autocorr_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_autocorr_get.argtypes = [vp, C.POINTER(AutocorrView)]
    L.apemost_hip_autocorr_set.argtypes = [vp, C.POINTER(AutocorrView)]
    L.apemost_hip_autocorr_end.argtypes = [vp]
    L.apemost_hip_predict_begin.argtypes = [vp, C.POINTER(PredictConfig)]
    L.apemost_hip_predict_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_predict_get.argtypes = [vp, C.POINTER(PredictView)]
    L.apemost_hip_predict_set.argtypes = [vp, C.POINTER(PredictView)]
    L.apemost_hip_predict_end.argtypes = [vp]
    L.apemost_hip_predict_curve.argtypes = [vp, C.c_int32, _dp, C.c_int32, _dp, _dp]
    L.apemost_hip_pointwise_begin.argtypes = [vp, C.POINTER(PointwiseConfig)]
    L.apemost_hip_pointwise_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_pointwise_get.argtypes = [vp, C.POINTER(PointwiseView)]
    L.apemost_hip_pointwise_set.argtypes = [vp, C.POINTER(PointwiseView)]
    L.apemost_hip_pointwise_end.argtypes = [vp]
    L.apemost_hip_pointwise_loglike.argtypes = [vp, C.c_int32, _dp, _dp]
    L.apemost_hip_pointwise_loglike_ladder.argtypes = [vp, C.c_int32, C.c_int32, _dp, _dp]
    L.apemost_hip_pointwise_tail_begin.argtypes = [vp, C.c_int32]
    L.apemost_hip_pointwise_tail_get.argtypes = [vp, C.POINTER(PointwiseTailView)]
    L.apemost_hip_pointwise_tail_set.argtypes = [vp, C.POINTER(PointwiseTailView)]
    L.apemost_hip_pointwise_tail_capacity.argtypes = [vp, C.POINTER(C.c_int32)]
    L.apemost_hip_pointwise_begin_at.argtypes = [vp, C.POINTER(PointwiseConfig), C.POINTER(PointwiseAt)]
    L.apemost_hip_pointwise_joint_get.argtypes = [vp, C.POINTER(PointwiseJointView)]
    L.apemost_hip_pointwise_joint_set.argtypes = [vp, C.POINTER(PointwiseJointView)]
    L.apemost_hip_pointwise_loglike_at.argtypes = [vp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp]
    ip = C.POINTER(C.c_int32)
    L.apemost_hip_check_begin.argtypes = [vp, C.c_int32, ip, C.c_int32, _dp]
    L.apemost_hip_check_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_check_get.argtypes = [vp, C.POINTER(CheckView)]
    L.apemost_hip_check_set.argtypes = [vp, C.POINTER(CheckView)]
    L.apemost_hip_check_lengths.argtypes = [vp, C.POINTER(C.c_int32)]
    L.apemost_hip_check_end.argtypes = [vp]
    L.apemost_hip_check_values.argtypes = [vp, C.c_int32, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp]
    L.apemost_hip_check_null_edges.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _dp]
    L.apemost_hip_periodogram_begin.argtypes = [vp, C.c_int32, ip, C.c_int32, _dp, _dp, _dp]
    L.apemost_hip_periodogram_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_periodogram_get.argtypes = [vp, C.POINTER(PeriodogramView)]
    L.apemost_hip_periodogram_set.argtypes = [vp, C.POINTER(PeriodogramView)]
    L.apemost_hip_periodogram_lengths.argtypes = [vp, C.POINTER(C.c_int32)]
    L.apemost_hip_periodogram_end.argtypes = [vp]
    L.apemost_hip_periodogram_values.argtypes = [vp, C.c_int32, _dp, C.c_int32, _dp, _dp, C.c_int32, _dp, _dp, _dp, _dp, _dp,
                                                 _dp, _dp, _dp, _dp, C.POINTER(C.c_int32)]
    L.apemost_hip_derived_check.argtypes = [C.c_int32, C.c_int32, ip, ip, C.c_int32, ip]
    L.apemost_hip_derived_begin.argtypes = [vp, C.POINTER(DerivedConfig)]
    L.apemost_hip_derived_accumulate.argtypes = [vp, vp, C.c_uint64, C.c_uint64, C.c_uint64]
    L.apemost_hip_derived_get.argtypes = [vp, C.POINTER(DerivedView)]
    L.apemost_hip_derived_set.argtypes = [vp, C.POINTER(DerivedView)]
    L.apemost_hip_derived_end.argtypes = [vp]
    L.apemost_hip_derived_eval.argtypes = [vp, C.c_uint64, _dp, _dp]
    L.apemost_hip_timer_begin.argtypes = [vp]
    L.apemost_hip_timer_end.argtypes = [vp, C.POINTER(C.c_float), _up]
    _lib = L
    return L


def check(rc):
    if rc != OK:
        raise ApemostHipError(rc, lib().apemost_hip_last_error().decode("utf-8", "replace"))


def device_count():
    n = C.c_int(0)
    check(lib().apemost_hip_device_count(C.byref(n)))
    return n.value


def device_info(device=0):
    name = C.create_string_buffer(256)
    cus, mem = C.c_int(0), C.c_uint64(0)
    check(lib().apemost_hip_device_info(device, name, 256, C.byref(cus), C.byref(mem)))
    return name.value.decode(), cus.value, mem.value


def calib_defaults(**overrides):
    c = CalibConfig()
    lib().apemost_hip_calib_defaults(C.byref(c))
    for k, v in overrides.items():
        setattr(c, k, v)
    return c


def ragged_layout(n_data, n_cols):
    """Where the ladders' data matrices of a ragged batch start, in doubles: (offsets [n_ladders + 1], the longest
    length, the total).  Host arithmetic only (apemost_hip_ragged_layout): no device is touched."""
    lens = np.ascontiguousarray(n_data, dtype=np.int32)
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    longest, total = C.c_int32(0), C.c_uint64(0)
    check(lib().apemost_hip_ragged_layout(len(lens), n_cols, lens.ctypes.data_as(C.POINTER(C.c_int32)),
                                          off.ctypes.data_as(_up), C.byref(longest), C.byref(total)))
    return off, longest.value, total.value


def swap_pair(seed, round_, n_global):
    return int(lib().apemost_hip_swap_pair(seed, round_, n_global))


def rng_raw(seed, subsequence, offset, n, device=0):
    out = np.zeros(n, dtype=np.uint32)
    check(lib().apemost_hip_rng_raw(device, seed, subsequence, offset, n,
                                    out.ctypes.data_as(C.POINTER(C.c_uint32))))
    return out


def rng_attempts(seed, chain, slot, tick, q0, n, device=0):
    y, s, valid = np.zeros(n), np.zeros(n), np.zeros(n, dtype=np.int32)
    lu = C.c_double(0)
    check(lib().apemost_hip_rng_attempts(device, seed, chain, slot, tick, q0, n, y.ctypes.data_as(_dp),
                                         s.ctypes.data_as(_dp), valid.ctypes.data_as(C.POINTER(C.c_int32)),
                                         C.byref(lu)))
    return y, s, valid.astype(bool), lu.value
