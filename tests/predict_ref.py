"""A restatement of the posterior predictive fold (include/apemost_hip.h, apemost_hip_predict_*; the specification is
the head of apemost_amd/csrc/pt_predict.h) that shares nothing with the kernels or with apemost_amd/predict.py.

The four curves are restated with every operation -- every FMA included -- rounded once from exact rational arithmetic
(fractions.Fraction; int / int true division rounds correctly, to nearest even).  sin_cw is restated step by step as
tools/check_sine.py does, in the form that ships (sin_multiple): fm = fma(u, 2.0, magic), the parity is the low
bit of fm.  Where an operand is not finite the operation is Python's own float arithmetic, which gives IEEE's inf and
NaN.  An exact zero result is +0 here whatever IEEE's sign would be: the tests' inputs avoid exact cancellations.
The pulse curves are plain IEEE operations: `pulse_numpy` states them with numpy for tests that need many samples.
RefPredict is the sequential loops of the fold.  Test infrastructure only."""
import math
from fractions import Fraction

import numpy as np

MODEL_SIMPLESIN, MODEL_PULSE, MODEL_PULSE_VROT, MODEL_SINE3 = 0, 1, 2, 3
TWO_PI = 2.0 * 3.14159265358979323846264338328
MAGIC = 6755399441055744.0
NPI_HI, NPI_MID = -3.14159265358979311600e+00, -1.22464679914735320717e-16
S = (-1.66666666666666657415e-01, 8.33333333333331587045e-03, -1.98412698412549659988e-04, 2.75573192191608328544e-06,
     -2.50521076166904495328e-08, 1.60589772926427431318e-10, -7.64396966398807388923e-13, 2.73143687693798929796e-15)
RANGE = 35184372088832.0    # 2^45


def _rnd(q):
    try:
        return q.numerator / q.denominator
    except OverflowError:
        return math.inf if q > 0 else -math.inf


def _finite(*v):
    return all(math.isfinite(a) for a in v)


def _float_op(f):
    try:
        return f()
    except (OverflowError, ZeroDivisionError):
        return math.nan


def mul(a, b):
    return _rnd(Fraction(a) * Fraction(b)) if _finite(a, b) else _float_op(lambda: a * b)


def add(a, b):
    return _rnd(Fraction(a) + Fraction(b)) if _finite(a, b) else _float_op(lambda: a + b)


def sub(a, b):
    return _rnd(Fraction(a) - Fraction(b)) if _finite(a, b) else _float_op(lambda: a - b)


def div(a, b):
    if _finite(a, b) and b != 0:
        return _rnd(Fraction(a) / Fraction(b))
    if b == 0:
        return math.nan if (a == 0 or a != a) else math.copysign(math.inf, a) * math.copysign(1.0, b)
    return _float_op(lambda: a / b)


def fma(a, b, c):
    return _rnd(Fraction(a) * Fraction(b) + Fraction(c)) if _finite(a, b, c) else _float_op(lambda: a * b + c)


def sin_cw(x, u):
    """the device's sine of x = kTwoPi * u (rounded), for finite arguments inside the range"""
    fm = fma(u, 2.0, MAGIC)
    odd = int(np.float64(fm).view(np.uint64)) & 1
    fn = sub(fm, MAGIC)
    r = fma(fn, NPI_HI, x)
    r = fma(fn, NPI_MID, r)
    z = mul(r, r)
    q = fma(z, S[7], S[6])
    for c in (S[5], S[4], S[3], S[2], S[1], S[0]):
        q = fma(z, q, c)
    v = fma(mul(r, z), q, r)
    return -v if odd else v


def sine_in_range(f, ph, x):
    return mul(TWO_PI, add(mul(abs(f), abs(x)), abs(ph))) < RANGE    # False for NaN


def _sine_term(a, f, ph, x):
    u = add(mul(f, x), ph)
    return mul(a, sin_cw(mul(TWO_PI, u), u))


def _lorentz(h, d, lifetime):
    t = mul(mul(TWO_PI, d), lifetime)
    return div(h, add(1.0, mul(t, t)))


def curve(model, par, x):
    """one value of the model curve for the parameter row par at x"""
    par = [float(v) for v in par]
    x = float(x)
    if model == MODEL_SIMPLESIN:
        a, f, ph, o = par[:4]
        if not sine_in_range(f, ph, x):
            return math.nan
        return add(_sine_term(a, f, ph, x), o)
    if model == MODEL_SINE3:
        if not all(sine_in_range(par[3 * c + 1], par[3 * c + 2], x) for c in range(3)):
            return math.nan
        m = 0.0
        for c in range(3):
            m = add(m, _sine_term(par[3 * c], par[3 * c + 1], par[3 * c + 2], x))
        return add(m, par[9])
    if model == MODEL_PULSE:
        y = 0.0
        for j in range(2, len(par) - 1, 2):
            y = add(y, _lorentz(par[j + 1], sub(par[j], x), par[0]))
        return y
    if model == MODEL_PULSE_VROT:
        vrot = par[2]
        d = sub(par[5], x)
        y = add(0.0, _lorentz(par[4], sub(par[3], x), par[0]))
        y = add(y, _lorentz(par[6], add(d, -vrot), par[0]))
        y = add(y, _lorentz(par[6], d, par[0]))
        return add(y, _lorentz(par[6], add(d, vrot), par[0]))
    raise ValueError(model)


def curves(model, params, x):
    """[n][n_x] of curve()"""
    return np.array([[curve(model, p, xi) for xi in x] for p in params], dtype=np.float64).reshape(len(params), len(x))


def pulse_numpy(params, x):
    """the pulse curve [n][n_x] in numpy's IEEE operations, mode after mode"""
    p = np.asarray(params, dtype=np.float64)
    x = np.asarray(x, dtype=np.float64)[None, :]
    y = np.zeros((p.shape[0], x.shape[1]))
    with np.errstate(all="ignore"):
        for j in range(2, p.shape[1] - 1, 2):
            t = (TWO_PI * (p[:, j, None] - x)) * p[:, 0, None]
            y = y + p[:, j + 1, None] / (1 + t * t)
    return y


def edges(lo, hi, nbins):
    e = [((nbins - b) / nbins) * lo + (b / nbins) * hi for b in range(nbins + 1)]
    e[nbins] += (hi - lo) / 10000
    return e


def bin_of(v, e):
    """the host's bisection; -1 outside [e[0], e[-1]) and for NaN"""
    left, right = 0, len(e) - 1
    if not (v >= e[0] and v < e[right]):
        return -1
    while right - left > 1:
        mid = (left + right) // 2
        if v >= e[mid]:
            left = mid
        else:
            right = mid
    return left


class RefPredict:
    """the fold of kept rows [n][n_chains][n_par+2] for the kept chains at the abscissae x ([n_x], or [n_keep][n_x]),
    one sample after the other.  values: the curves [n][n_keep][n_x] where the caller has them already."""

    def __init__(self, model, rows, chains, x, nbins=0, lo=0.0, hi=0.0, values=None):
        rows = np.asarray(rows, dtype=np.float64)
        n, _, w = rows.shape
        n_par, K = w - 2, len(chains)
        x = np.asarray(x, dtype=np.float64)
        x = np.tile(x, (K, 1)) if x.ndim == 1 else x
        X = x.shape[1]
        self.n = n
        self.origin, self.sum, self.sq = np.zeros((K, X)), np.zeros((K, X)), np.zeros((K, X))
        self.vmin, self.vmax = np.full((K, X), np.inf), np.full((K, X), -np.inf)
        self.hist = np.zeros((K, X, nbins), dtype=np.uint64)
        self.best_prob, self.best_params = np.full(K, -np.inf), np.zeros((K, n_par))
        self.best_n = np.zeros(K, dtype=np.uint64)
        e = edges(lo, hi, nbins) if nbins else None
        if values is None:
            values = np.array([[[curve(model, rows[t, c, :n_par], xi) for xi in x[k]] for k, c in enumerate(chains)]
                               for t in range(n)], dtype=np.float64).reshape(n, K, X)
        with np.errstate(all="ignore"):
            for k, chain in enumerate(chains):
                for t in range(n):
                    p = rows[t, chain, n_par]
                    if p > self.best_prob[k]:
                        self.best_prob[k], self.best_n[k] = p, t + 1
                        self.best_params[k] = rows[t, chain, :n_par]
                for i in range(X):
                    v = values[:, k, i]
                    origin = v[0] if n else 0.0
                    total = sq = np.float64(0.0)
                    vmin, vmax = np.inf, -np.inf
                    for t in range(n):
                        d = v[t] - origin
                        total = total + d
                        dd = d * d
                        sq = sq + dd
                        if v[t] < vmin:
                            vmin = v[t]
                        if v[t] > vmax:
                            vmax = v[t]
                        if nbins:
                            b = bin_of(v[t], e)
                            if b >= 0:
                                self.hist[k, i, b] += np.uint64(1)
                    self.origin[k, i], self.sum[k, i], self.sq[k, i] = origin, total, sq
                    self.vmin[k, i], self.vmax[k, i] = vmin, vmax


def same_floats(a, b):
    """bit for bit, except that a NaN equals a NaN of any sign and payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


FLOAT_FIELDS = ("origin", "sum", "sq", "vmin", "vmax", "best_prob", "best_params")
INT_FIELDS = ("hist", "best_n")
FIELDS = FLOAT_FIELDS + INT_FIELDS


def assert_equals(got, ref, what=""):
    """a Predict (or RefPredict) against another, every field with == on the bits"""
    n = int(got.n[0]) if hasattr(got.n, "__len__") else int(got.n)
    m = int(ref.n[0]) if hasattr(ref.n, "__len__") else int(ref.n)
    assert n == m, (what, n, m)
    for f in FLOAT_FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        if not same_floats(a, b):
            a, b = np.asarray(a), np.asarray(b)
            with np.errstate(all="ignore"):
                bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
            at = tuple(bad[0]) if len(bad) else ()
            raise AssertionError("%s %s: %d entries differ (signs of zero included), first at %s: %r against %r" % (
                what, f, len(bad), at, a[at] if len(bad) else None, b[at] if len(bad) else None))
    for f in INT_FIELDS:
        a, b = np.asarray(getattr(got, f)), np.asarray(getattr(ref, f))
        assert a.shape == b.shape and np.array_equal(a, b), (what, f, np.argwhere(a != b)[:3].tolist())
