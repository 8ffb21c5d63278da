"""The four built-in log-likelihoods and priors in numpy.longdouble (x87 extended: 64 bits of significand), restated
from the formulas of the project's own oracle (oracle/apemost_oracle.c ll_simplesin, ll_sine3, ll_pulse,
ll_pulse_vrot): one term per data point, the terms added in index order.  None of the kernels' shortcuts: no running
product under one logarithm, no reciprocal shared between points, no tree of partial sums.

2 pi is the reference's `2.0 * M_PI`, the fp64 constant: the models are defined with it (apps/simplesin.c, apps/pulse.c),
and the phase 2 pi (f x + phi) of a sine model is of the order of 1e2..1e3 rad, so the true pi in its place would move
a term by 1e-14 relative -- another model, not a better sum."""
import numpy as np

# the x87 format: without it this reference is the oracle's own arithmetic and checks nothing
assert np.finfo(np.longdouble).nmant >= 63, "numpy.longdouble is not an extended-precision type on this host"

L = np.longdouble
TWO_PI = L(2.0) * L(np.pi)           # (exact in either format: a power of two times the fp64 constant)


def _sum(terms):
    """the terms added one by one in index order (ufunc.accumulate is a serial loop, unlike the pairwise np.sum)"""
    terms = np.asarray(terms, dtype=L)
    return np.add.accumulate(terms)[-1] if len(terms) else L(0)


def _sines(p, x, count):
    m = np.zeros_like(x)
    for k in range(count):
        m = m + p[3 * k] * np.sin(TWO_PI * (p[3 * k + 1] * x + p[3 * k + 2]))
    return m


def simplesin(p, x, y, beta, sigma):
    d = _sines(p, x, 1) + p[3] - y
    return beta * _sum(d * d) / (-2 * sigma * sigma), L(0)


def sine3(p, x, y, beta, sigma):
    d = _sines(p, x, 3) + p[9] - y
    return beta * _sum(d * d) / (-2 * sigma * sigma), L(0)


def _lorentz(freq, height, nu, lifetime):
    q = TWO_PI * (freq - nu) * lifetime
    return height / (1 + q * q)


def pulse(p, nu, d, beta, hmin):
    n_modes = (len(p) - 2) // 2
    prior = -_sum([np.log(p[j + 1] + hmin) for j in range(2, len(p), 2)]) / n_modes
    y = np.zeros_like(nu)
    for j in range(2, len(p), 2):
        y = y + _lorentz(p[j], p[j + 1], nu, p[0])
    prob = p[1] + _sum(np.log(y) + d / y)
    return prior + -beta * prob, prior


def pulse_vrot(p, nu, d, beta, hmin):
    prior = -(np.log(p[4] + hmin) + np.log(p[6] + hmin)) / 2
    y = _lorentz(p[3], p[4], nu, p[0])
    for k in (-1, 0, 1):
        y = y + _lorentz(p[5] + k * p[2], p[6], nu, p[0])
    prob = p[1] + _sum(np.log(y) + d / y)
    return prior + -beta * prob, prior


def loglike(model, params, data, beta=1.0, sigma=0.5, hmin=1e-6):
    """(prob, prior) of the built-in model `model` (its name) as numpy.longdouble"""
    p = np.asarray(params, dtype=np.float64).astype(L)
    data = np.asarray(data, dtype=np.float64)
    x, y = data[:, 0].astype(L), data[:, 1].astype(L)
    if model == "simplesin":
        return simplesin(p, x, y, L(beta), L(sigma))
    if model == "sine3":
        return sine3(p, x, y, L(beta), L(sigma))
    if model == "pulse":
        return pulse(p, x, y, L(beta), L(hmin))
    if model == "pulse_vrot":
        return pulse_vrot(p, x, y, L(beta), L(hmin))
    raise ValueError("no built-in model %r" % (model,))
