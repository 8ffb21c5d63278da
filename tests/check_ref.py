"""A restatement of the predictive checks' rule (apemost_amd/csrc/pt_check.h; include/apemost_hip.h,
apemost_hip_check_*) that shares nothing with the kernels or with apemost_amd/check.py.

It starts from e and u, the residual and the predictive CDF of every (sample, datum) pair, and from l, the pointwise
term: those are the device's own values (HipSampler.check_values, pointwise_loglike_at) or synthetic ones.  What the
rule does with them is plain IEEE arithmetic, which numpy and Python floats state bit for bit:

  stats       FIT and SERIAL through the two-stage sum (64 lane partials, each from +0.0 over the terms i = j, j + 64,
              ... in ascending order, then the adjacent-pairs tree taken six times); numpy adds two float64 arrays
              element by element with one rounding each, so both stages are whole-array additions.  EXTREME is the
              maximum of the terms that are not NaN, from -inf, plus 0.0.
  RefSeries   the seven words of one series, folded one sample after the other in Python with math.exp; beside the
              sequential S and SU it keeps their sums about the final maximum without summation error (math.fsum), which
              the comparison rule of tests/test_gpu_pointwise.py needs.
  RefStat     the five words and the counts of one statistic of one kept chain.
Test infrastructure only."""
import math

import numpy as np

LANES = 64
SINE = (0, 3)          # APEMOST_MODEL_SIMPLESIN, APEMOST_MODEL_SINE3 (include/apemost_hip.h)


def two_stage_sum(terms):
    """the rule's sum of the terms [..., L] over the last axis"""
    terms = np.asarray(terms, dtype=np.float64)
    L = terms.shape[-1]
    p = np.zeros(terms.shape[:-1] + (LANES,))
    with np.errstate(all="ignore"):
        for i0 in range(0, L, LANES):
            chunk = terms[..., i0:i0 + LANES]
            m = chunk.shape[-1]
            p[..., :m] = p[..., :m] + chunk
        for _ in range(6):
            p = p[..., 0::2] + p[..., 1::2]
    return p[..., 0]


def serial_terms(u):
    """g [..., L] of SERIAL from u [..., L]: g_0 = +0.0, g_i = a_i * a_{i-1} with a = u - 0.5"""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(all="ignore"):
        a = u - np.float64(0.5)
        g = np.zeros(a.shape)
        g[..., 1:] = a[..., 1:] * a[..., :-1]
    return g


def stats(e, u, sine):
    """T [..., 3] (FIT, EXTREME, SERIAL) of e, u [..., L]"""
    e, u = np.asarray(e, dtype=np.float64), np.asarray(u, dtype=np.float64)
    with np.errstate(all="ignore"):
        fit = two_stage_sum(e * e if sine else e)
        t = np.abs(e) if sine else e
        ext = np.where(np.isnan(t), -np.inf, t).max(axis=-1) + np.float64(0.0)
        ser = two_stage_sum(serial_terms(u))
    return np.stack([fit, ext, ser], axis=-1)


def exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


class RefSeries:
    """the seven words of the samples e, u, l [n] of one series, folded sequentially"""

    def __init__(self, e, u, l):
        e, u, l = ([float(v) for v in np.asarray(a, dtype=np.float64).reshape(-1).tolist()] for a in (e, u, l))
        self.n = len(e)
        origin = e[0]
        total = sq = sum_u = 0.0
        m, S, SU = -l[0], 1.0, u[0]
        for t in range(self.n):
            d = e[t] - origin
            total = total + d
            dd = d * d
            sq = sq + dd
            sum_u = sum_u + u[t]
            if t == 0:
                continue
            x = -l[t]
            if x > m:
                w = exp(m - x)
                S = S * w + 1.0
                SU = SU * w + u[t]
                m = x
            else:
                w = exp(x - m)
                S = S + w
                uw = u[t] * w
                SU = SU + uw
        self.origin, self.sum, self.sq, self.sum_u, self.m, self.S, self.SU = origin, total, sq, sum_u, m, S, SU
        self.finite = all(math.isfinite(v) for v in l) and all(math.isfinite(v) for v in u)
        if self.finite:
            self.S_exact = math.fsum(exp(-v - m) for v in l)
            self.SU_exact = math.fsum(uu * exp(-v - m) for uu, v in zip(u, l))


class RefStat:
    """origin, sum, sq, min, max and the counts [len(edges) + 2] of the samples T [n] of one statistic"""

    def __init__(self, T, edges):
        T = [float(v) for v in np.asarray(T, dtype=np.float64).reshape(-1).tolist()]
        edges = [float(v) for v in edges]
        self.n = len(T)
        origin = T[0]
        total = sq = 0.0
        mn, mx = math.inf, -math.inf
        counts = [0] * (len(edges) + 2)
        for v in T:
            d = v - origin
            total = total + d
            dd = d * d
            sq = sq + dd
            mn = v if v < mn else mn
            mx = v if v > mx else mx
            counts[len(edges) + 1 if v != v else sum(1 for b in edges if b <= v)] += 1
        self.origin, self.sum, self.sq, self.min, self.max = origin, total, sq, mn, mx
        self.counts = np.array(counts, dtype=np.uint64)
