"""The rule of the residual periodogram (apemost_amd/csrc/pt_periodogram.h) restated in Python: a reference for the fold
(apemost_hip_periodogram_*) that shares nothing with the kernels or with apemost_amd/periodogram.py.

Python 3.10 has no math.fma: the fused multiply-add is taken exactly in fractions.Fraction and rounded once by float(),
which is correctly rounded; non-finite operands, exact zeros and overflow are handled by hand."""
import math
from fractions import Fraction

import numpy as np

TWO_PI = 2.0 * 3.14159265358979323846264338328
RANGE = 35184372088832.0      # 2^45


def fma(a, b, c):
    """fl(a * b + c), one rounding"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b)):
        with np.errstate(all="ignore"):
            return float(np.float64(a) * np.float64(b) + np.float64(c))   # (the product is NaN or inf as it stands)
    if not math.isfinite(c):
        return c                     # (the exact product is finite, whatever its rounded value would be)
    exact = Fraction(a) * Fraction(b) + Fraction(c)
    if exact == 0:
        if a == 0.0 or b == 0.0:     # an exact zero product keeps its sign: (+-0) + c by IEEE addition
            return math.copysign(0.0, a) * math.copysign(1.0, b) + c
        return 0.0                   # exact cancellation: +0 under round-to-nearest
    try:
        return float(exact)
    except OverflowError:
        return math.inf if exact > 0 else -math.inf


def in_range(nu, x):
    """the trig is NaN unless this holds: predict_sine_in_range with ph = 0.25"""
    with np.errstate(all="ignore"):
        return bool(np.float64(TWO_PI) * (np.float64(abs(nu)) * np.float64(abs(x)) + np.float64(0.25)) < RANGE)


def sums(r, c, s):
    """(C, S) of one frequency: fused multiply-adds from +0.0 in ascending i"""
    C = S = 0.0
    for ri, ci, si in zip(np.asarray(r, dtype=np.float64).tolist(), np.asarray(c, dtype=np.float64).tolist(),
                          np.asarray(s, dtype=np.float64).tolist()):
        C = fma(ri, ci, C)
        S = fma(ri, si, S)
    return C, S


def power(w, C, S):
    """((wcc C) C + (wcs C) S) + (wss S) S, every operation rounded"""
    with np.errstate(all="ignore"):
        wcc, wcs, wss, C, S = (np.float64(v) for v in (w[0], w[1], w[2], C, S))
        return float(((wcc * C) * C + (wcs * C) * S) + (wss * S) * S)


def peak(P):
    """(m, arg): the first occurrence of the largest P; a NaN never wins; (-inf, n_freq) where nothing is above -inf"""
    m, arg = -math.inf, len(P)
    for j, p in enumerate(np.asarray(P, dtype=np.float64).tolist()):
        if p > m:
            m, arg = p, j
    return m, arg


def row(r, c, s, w):
    """C, S, P [n_freq], peak and arg of one sample: r [L], c, s [n_freq][L], w [n_freq][3]"""
    n_freq = len(c)
    C, S, P = np.zeros(n_freq), np.zeros(n_freq), np.zeros(n_freq)
    for j in range(n_freq):
        C[j], S[j] = sums(r, c[j], s[j])
        P[j] = power(w[j], C[j], S[j])
    m, arg = peak(P)
    return C, S, P, m, arg


class Moments:
    """origin, sum, sq, min, max of a sequence, as the device folds them"""

    def __init__(self, values):
        self.origin = self.sum = self.sq = self.min = self.max = 0.0
        with np.errstate(all="ignore"):
            for t, v in enumerate(np.asarray(values, dtype=np.float64)):
                if t == 0:
                    self.origin, self.min, self.max = v, np.float64(math.inf), np.float64(-math.inf)
                    self.sum, self.sq = np.float64(0.0), np.float64(0.0)
                d = v - self.origin
                self.sum = self.sum + d
                self.sq = self.sq + d * d
                self.min = v if v < self.min else self.min
                self.max = v if v > self.max else self.max


class RefSeries(Moments):
    """the words of one series (kept chain, frequency) over its samples' P, C and S in order"""

    def __init__(self, P, C, S, level):
        Moments.__init__(self, P)
        self.sum_c = self.sum_s = np.float64(0.0)
        self.exceed = 0
        with np.errstate(all="ignore"):
            for p, c, s in zip(np.asarray(P, dtype=np.float64), np.asarray(C, dtype=np.float64), np.asarray(S, dtype=np.float64)):
                self.sum_c = self.sum_c + c
                self.sum_s = self.sum_s + s
                self.exceed += 1 if p > level else 0


class RefPeak(Moments):
    """the words of one kept chain's highest peak over its samples' (m, arg) in order"""

    def __init__(self, m, arg, n_freq):
        Moments.__init__(self, m)
        self.counts = np.zeros(n_freq + 1, dtype=np.uint64)
        for a in arg:
            self.counts[int(a)] += np.uint64(1)
