"""Which data lengths walk which part of the likelihood loops, and the inputs the data-length tests share.

The data sum of a Metropolis step is written twice and splits into regimes by n_data.  With T = 64 * waves lanes
per chain:

  * Engine::cache_rows and Engine::lane_sum (apemost_amd/csrc/pt_device.h:1763-1783 and 1832-1937): rows held in
    registers when n_data == kWide * T exactly (kWide = 4 below eight waves, 2 at eight); the software-pipelined
    loop of n_data // (4 T) passes for waves <= 2 and the kPrefetch models (simplesin, sine3, pulse_vrot: two
    passes per trip, the second one advancing only while k + 1 < passes, an odd count leaving one pass behind
    the loop); the 4-wide loop for waves < 8 where the pipelined loop does not exist; the 2-wide loop; the
    1-wide tail.
  * ObEngine::cache_rows and ObEngine::lik_partial (apemost_amd/csrc/pt_onebarrier.h:480-550): the same without
    the pipelined loop, for the four and eight likelihood waves of the one-barrier kernels.

regimes() restates both as a walk over the lanes; lengths() is the list of lengths the GPU tests run, chosen so
that every regime a (model, waves) pair can reach is reached (tests/test_data_lengths_cpu.py holds that against
this restatement, so a constant that moves there without moving here fails a test instead of thinning the
matrix).  case() is the shared, read-only input of a (model, length): data, six parameter points, their betas,
the extended-precision reference (tests/loglike_ref.py) and the oracle's values, computed once per process."""
import functools
import types

import numpy as np

from apemost_amd import workloads as wl
from oracle import oracle as orc
from tests import loglike_ref

K_WAVE = 64
MODELS = ("simplesin", "sine3", "pulse", "pulse_vrot")
WAVES = (1, 2, 4, 6, 8)
PREFETCH_MODELS = ("simplesin", "sine3", "pulse_vrot")      # Model::kPrefetch, pt_device.h:540, 668, 1099
ONE_BARRIER_WAVES = (4, 8)                                  # kObWavesMask, pt_kernels.h:47-48
BIG_LDS = 64 * 1024                                         # beyond it a kernel opts in (enable_big_lds)


def threads(waves):
    return K_WAVE * waves


def k_wide(waves):
    """Engine::kWide (pt_device.h:1766) and ObEngine::kWide (pt_onebarrier.h:170)"""
    return 4 if waves < 8 else 2


def pipelined(waves, model):
    """Engine::kPipelined (pt_device.h:1772)"""
    return waves <= 2 and model in PREFETCH_MODELS


def pipe_passes(n_data, waves, model):
    """passes of the software-pipelined loop (pt_device.h:1853); 0 where it does not run"""
    if not pipelined(waves, model) or n_data == k_wide(waves) * threads(waves):
        return 0
    return n_data // (4 * threads(waves))


def _walk(n_data, t, kw, pipe, wide4):
    """(regime names, how often each point is evaluated) of one data sum: `pipe` the pipelined loop exists,
    `wide4` the 4-wide loop exists"""
    hit, seen = set(), np.zeros(n_data, dtype=np.int64)
    if n_data == kw * t:                         # rows_in_regs: i = n_data, every loop below is empty
        for tid in range(t):
            seen[tid:n_data:t] += 1
        return {"rows_in_regs"}, seen
    base = 0
    if pipe:
        passes = n_data // (4 * t)
        if passes > 0:
            hit.add("pipe_passes_1" if passes == 1 else "pipe_passes_2" if passes == 2 else
                    "pipe_passes_odd_ge3" if passes % 2 else "pipe_passes_even_ge4")
            base = passes * 4 * t
            seen[:base] += 1
    for tid in range(t):
        i, trips = base + tid, 0
        if wide4:
            while i + 3 * t < n_data:
                seen[[i, i + t, i + 2 * t, i + 3 * t]] += 1
                i += 4 * t
                trips += 1
            if trips:
                hit.add("wide4")
            if trips > 1:
                hit.add("wide4_trips_ge2")
        while i + t < n_data:
            seen[[i, i + t]] += 1
            i += 2 * t
            hit.add("wide2")
        while i < n_data:
            seen[i] += 1
            i += t
            hit.add("tail1")
    return hit, seen


def two_phase_walk(n_data, waves, model):
    """Engine::lane_sum, pt_device.h:1832-1937"""
    pipe = pipelined(waves, model)
    return _walk(n_data, threads(waves), k_wide(waves), pipe, waves < 8 and not pipe)


def one_barrier_walk(n_data, waves):
    """ObEngine::lik_partial, pt_onebarrier.h:492-550 (LW = waves likelihood wavefronts)"""
    assert waves in ONE_BARRIER_WAVES
    return _walk(n_data, threads(waves), k_wide(waves), False, waves < 8)


def regimes(n_data, waves, model):
    """the names of the regimes a data vector of n_data points exercises at `waves` wavefronts per chain"""
    t = threads(waves)
    hit, _ = two_phase_walk(n_data, waves, model)
    if waves in ONE_BARRIER_WAVES:
        hit = hit | one_barrier_walk(n_data, waves)[0]
    if n_data % K_WAVE:
        hit.add("partial_wave")                  # a wavefront with some lanes past the end
    if n_data <= t - K_WAVE:
        hit.add("idle_waves")                    # a whole wavefront without a point (its partial sum is 0)
    if 16 * n_data > BIG_LDS:
        hit.add("stage_over_64k")                # the staged vector alone is more than 64 KiB of LDS
    return hit


def reachable(waves, model):
    """every regime some length can reach at this (model, waves)"""
    out = {"rows_in_regs", "wide2", "tail1", "partial_wave", "stage_over_64k"}
    if waves > 1:
        out.add("idle_waves")
    if pipelined(waves, model):
        out |= {"pipe_passes_1", "pipe_passes_2", "pipe_passes_odd_ge3", "pipe_passes_even_ge4"}
    elif waves < 8:
        out |= {"wide4", "wide4_trips_ge2"}
    return out


def lengths(waves, model):
    """the data lengths the GPU tests run at this (model, waves), ascending"""
    t = threads(waves)
    out = {1, 2, 63, 64, 65, t - 1, t, t + 1, 2 * t - 1, 2 * t, 2 * t + 1, 3 * t + 1, 4 * t - 1, 4 * t, 4 * t + 1,
           5 * t + 1, 7 * t + 1}
    out |= {k_wide(waves) * t - 1, k_wide(waves) * t, k_wide(waves) * t + 1}
    if waves <= 2:
        out |= {8 * t, 8 * t + 1, 12 * t, 15 * t + 1, 16 * t, 21 * t + 1}
    else:
        out.add(9 * t + 1)
    out.add(4100)                                # staged: more than 64 KiB at every shape
    return sorted(n for n in out if n >= 1)


def sampling_lengths(waves, model):
    """the reduced set the sampling tests run: the shortest length of every regime, and T + 1"""
    all_lengths = lengths(waves, model)
    out = {threads(waves) + 1}
    for r in sorted(reachable(waves, model)):
        out.add(min(n for n in all_lengths if r in regimes(n, waves, model)))
    return sorted(out)


def calibration_lengths(waves, model):
    t = threads(waves)
    return sorted({t + 1, k_wide(waves) * t, max(lengths(waves, model))})


# (model, n_data): added to the seed where the drawn points are ill-conditioned -- the oracle's own fp64 sum is then
# further than 1e-13 from the extended reference (test_data_lengths_cpu.py), so no fp64 kernel can be held to 1e-12
# (one and two points of a sine model: the residual at w.start is the noise of a single point, and where it is small
# the rounding of the phase 2 pi (f x + phi) ~ 128 rad is 1e-12 of its square; the data noise is redrawn with the points)
RESEED = {("simplesin", 1): 11, ("simplesin", 2): 3, ("sine3", 1): 7, ("sine3", 2): 3}


@functools.lru_cache(maxsize=None)
def case(model, n_data):
    """the shared input of (model, n_data): w (the workload), params [6][n_par] (w.start and five points uniform in
    the inner 90 % of the prior box), beta [6] uniform in [0.01, 1], ext_prob / ext_prior (numpy.longdouble,
    tests/loglike_ref.py), orc_prob / orc_prior (the oracle).  Read-only: every test sees the same arrays."""
    bump = RESEED.get((model, n_data), 0)
    w = wl.by_name(model, n_data=n_data, n_chain=2, **({"seed": 1000 + bump} if bump else {}))   # (w.start is a point too)
    rs = np.random.RandomState([w.model, n_data, bump])
    params = np.vstack([w.start, w.pmin + (w.pmax - w.pmin) * rs.uniform(0.05, 0.95, size=(5, w.n_par))])
    beta = rs.uniform(0.01, 1.0, len(params))
    ext = [loglike_ref.loglike(model, p, w.data, b) for p, b in zip(params, beta)]
    ref = [orc.loglike(w.model, p, w.data, beta=b) for p, b in zip(params, beta)]
    c = types.SimpleNamespace(w=w, params=params, beta=beta,
                              ext_prob=np.array([e[0] for e in ext], dtype=np.longdouble),
                              ext_prior=np.array([e[1] for e in ext], dtype=np.longdouble),
                              orc_prob=np.array([r[0] for r in ref]), orc_prior=np.array([r[1] for r in ref]))
    for a in (w.data, params, beta, c.ext_prob, c.ext_prior, c.orc_prob, c.orc_prior):
        a.setflags(write=False)
    return c


def rel_err(got, want):
    """|got - want| / |want| in extended precision (0 where both are 0)"""
    got, want = np.asarray(got, dtype=np.longdouble), np.asarray(want, dtype=np.longdouble)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.abs(got - want) / np.abs(want)
    return np.where(got == want, np.longdouble(0), r)
