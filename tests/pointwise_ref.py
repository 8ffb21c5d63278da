"""A restatement of the pointwise log-likelihood fold (include/apemost_hip.h, apemost_hip_pointwise_*; the
specification is the head of apemost_amd/csrc/pt_pointwise.h) that shares nothing with the kernels or with
apemost_amd/pointwise.py.

The term is built on the rational-arithmetic `curve` of tests/predict_ref.py and its sub / mul / div / add, every
operation rounded once from exact rational arithmetic; the pulse logarithm is math.log.  RefPointwise is the sequential
fold with Python's math.exp.  Beside the sequential S words it keeps what the comparison rule of
tests/test_gpu_pointwise.py needs: the sums of the reference's exponentials about the final maximum, taken without
summation error (math.fsum, and exact rationals for the squares).  An exact zero result is +0 here whatever IEEE's sign
would be: the tests' inputs avoid exact cancellations (a curve value equal to its datum).  Test infrastructure only."""
import math
from fractions import Fraction

import numpy as np

from tests.predict_ref import (MODEL_PULSE, MODEL_PULSE_VROT, MODEL_SIMPLESIN, MODEL_SINE3, add, curve, div, mul,
                               same_floats, sub)

SINE = (MODEL_SIMPLESIN, MODEL_SINE3)
STATE = ("origin", "sum", "sq", "m_up", "S_up", "m_dn", "S_dn", "S2_dn")
EXACT = ("origin", "sum", "sq", "m_up", "m_dn", "par_origin", "par_sum")


def sine_constant(sigma):
    return div(1.0, mul(mul(-2.0, float(sigma)), float(sigma)))


def ln(v):
    """math.log with IEEE's answers at the edges"""
    if v != v or v < 0:
        return math.nan
    if v == 0:
        return -math.inf
    return math.inf if v == math.inf else math.log(v)


def term_of(model, v, y, c):
    """the term of one datum from the curve's value v"""
    if model in SINE:
        r = sub(v, y)
        return mul(mul(r, r), c)
    return -add(ln(v), div(y, v))


def term(model, par, x, y, sigma):
    return term_of(model, curve(model, par, x), float(y), sine_constant(sigma))


def terms(model, params, data, sigma):
    """[n][n_data] of term()"""
    c = sine_constant(sigma)
    return np.array([[term_of(model, curve(model, p, xi), float(yi), c) for xi, yi in data[:, :2]] for p in params],
                    dtype=np.float64).reshape(len(params), len(data))


def exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def _exact_sum_of_squares(es):
    try:
        return float(sum(Fraction(e) * Fraction(e) for e in es))
    except OverflowError:
        return math.inf


class RefPointwise:
    """the fold of kept rows [n][n_chains][n_par+2] for the kept chains over their data ([n_data][2], or one matrix
    per kept chain), one sample after the other.  values: the terms [n][n_keep][n_data] where the caller has them."""

    def __init__(self, model, rows, chains, data, sigma=0.5, values=None):
        rows = np.asarray(rows, dtype=np.float64)
        n, _, w = rows.shape
        n_par, K = w - 2, len(chains)
        data = np.asarray(data, dtype=np.float64)
        data = np.tile(data, (K, 1, 1)) if data.ndim == 2 else data
        D = data.shape[1]
        if values is None:
            values = np.array([terms(model, rows[:, c, :n_par], data[k], sigma) for k, c in enumerate(chains)],
                              dtype=np.float64).reshape(K, n, D).transpose(1, 0, 2)
        values = np.asarray(values, dtype=np.float64).reshape(n, K, D)
        self.n, self.values = n, values
        for f in STATE + ("S_up_exact", "S_dn_exact", "S2_dn_exact"):
            setattr(self, f, np.zeros((K, D)))
        self.finite = np.isfinite(values).all(axis=0) if n else np.ones((K, D), dtype=bool)
        self.par_origin, self.par_sum = np.zeros((K, n_par)), np.zeros((K, n_par))
        for k, chain in enumerate(chains):
            for p in range(n_par):
                col = rows[:, chain, p].tolist()
                origin, total = (col[0] if n else 0.0), 0.0
                for v in col:
                    total = total + (v - origin)
                self.par_origin[k, p], self.par_sum[k, p] = origin, total
            for i in range(D):
                col = values[:, k, i].tolist()
                if not n:
                    continue
                origin = col[0]
                total = sq = 0.0
                m_up, S_up, m_dn, S_dn, S2_dn = origin, 1.0, -origin, 1.0, 1.0
                for t, l in enumerate(col):
                    d = l - origin
                    total = total + d
                    dd = d * d
                    sq = sq + dd
                    if t == 0:
                        continue
                    if l > m_up:
                        S_up = S_up * exp(m_up - l) + 1.0
                        m_up = l
                    else:
                        S_up = S_up + exp(l - m_up)
                    x = -l
                    if x > m_dn:
                        e = exp(m_dn - x)
                        S_dn = S_dn * e + 1.0
                        S2_dn = S2_dn * (e * e) + 1.0
                        m_dn = x
                    else:
                        e = exp(x - m_dn)
                        S_dn = S_dn + e
                        S2_dn = S2_dn + e * e
                for f, v in zip(STATE, (origin, total, sq, m_up, S_up, m_dn, S_dn, S2_dn)):
                    getattr(self, f)[k, i] = v
                if self.finite[k, i]:
                    self.S_up_exact[k, i] = math.fsum(exp(l - m_up) for l in col)
                    down = [exp(-l - m_dn) for l in col]
                    self.S_dn_exact[k, i] = math.fsum(down)
                    self.S2_dn_exact[k, i] = _exact_sum_of_squares(down)


def nan_positions_agree(a, b):
    return bool(np.array_equal(np.isnan(np.asarray(a)), np.isnan(np.asarray(b))))


def assert_same_state(got, ref, what=""):
    """two device results (or files): every word of the state bit for bit, a NaN by its position"""
    assert int(np.asarray(got.n).reshape(-1)[0]) == int(np.asarray(ref.n).reshape(-1)[0]), what
    for f in STATE + ("par_origin", "par_sum"):
        assert same_floats(getattr(got, f), getattr(ref, f)), (what, f)
