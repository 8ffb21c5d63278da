"""A dense restatement of what apemost_amd/psis.py and the device tail (pt_pointwise_tail.h) compute, sharing nothing with
either: the top-capacity selection as a sort of int64 keys over a dense [n][n_data] matrix, the PSIS algorithm over all n
log ratios of a datum (sort, cut the tail, fit, replace, truncate at the maximum, normalise), the generalised Pareto fit
in mpmath at 50 digits, and a sequential host fold of the words psis() reads from a Pointwise."""
import math

import mpmath
import numpy as np


# ---- the selection ------------------------------------------------------------------------------------------------
def order_keys(x):
    """int64 keys that order like the doubles' bit patterns under the total order: -inf < ... < -0 < +0 < ... < +inf"""
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.int64)
    return np.where(b < 0, b ^ np.int64(0x7FFFFFFFFFFFFFFF), b)


def select(x, capacity):
    """x [n][n_data] (NaN allowed) -> (count [n_data] uint64, values [n_data][capacity]): per column the `capacity`
    largest non-NaN values in the key order, descending; 0.0 behind count"""
    x = np.asarray(x, dtype=np.float64)
    n, nd = x.shape
    count, values = np.zeros(nd, dtype=np.uint64), np.zeros((nd, capacity))
    for i in range(nd):
        col = x[:, i]
        col = col[~np.isnan(col)]
        keys = np.sort(order_keys(col))[::-1][:capacity]
        back = np.where(keys < 0, keys ^ np.int64(0x7FFFFFFFFFFFFFFF), keys).view(np.float64)
        count[i] = len(back)
        values[i, :len(back)] = back
    return count, values


def select_chains(x, capacity):
    """x [n][n_keep][n_data] -> (count [n_keep][n_data], values [n_keep][n_data][capacity])"""
    parts = [select(x[:, k], capacity) for k in range(x.shape[1])]
    return np.stack([p[0] for p in parts]), np.stack([p[1] for p in parts])


# ---- the sequential fold of the words psis() reads -------------------------------------------------------------------
def fold_state(l):
    """l [n][n_data] -> dict of the eight state words of pt_pointwise.h's recurrence, on the host in float64"""
    l = np.asarray(l, dtype=np.float64)
    n, nd = l.shape
    origin = l[0].copy()
    out = dict(origin=origin, sum=np.zeros(nd), sq=np.zeros(nd), m_up=l[0].copy(), S_up=np.ones(nd), m_dn=-l[0],
               S_dn=np.ones(nd), S2_dn=np.ones(nd))
    with np.errstate(all="ignore"):
        for t in range(1, n):
            d = l[t] - origin
            out["sum"] += d
            out["sq"] += d * d
            for m, S, S2, x in (("m_up", "S_up", None, l[t]), ("m_dn", "S_dn", "S2_dn", -l[t])):
                up = x > out[m]
                tt = np.exp(np.where(up, out[m] - x, x - out[m]))
                out[S] = np.where(up, out[S] * tt + 1.0, out[S] + tt)
                if S2:
                    out[S2] = np.where(up, out[S2] * (tt * tt) + 1.0, out[S2] + tt * tt)
                out[m] = np.where(up, x, out[m])
    return out


# ---- the fit in mpmath ---------------------------------------------------------------------------------------------
def gpdfit_mp(x, digits=50):
    """(k, sigma, kappa) by the Zhang-Stephens estimator with the loo package's settings, in `digits` digits; kappa =
    mean |theta x / (1 - theta x)| is the sensitivity of k to a relative change of theta"""
    with mpmath.workdps(digits):
        xs = [mpmath.mpf(float(v)) for v in x]
        N = len(xs)
        G = 30 + int(math.floor(math.sqrt(N)))
        star = xs[int(math.floor(N / 4 + 0.5)) - 1]
        theta = [1 / xs[-1] + (1 - mpmath.sqrt(mpmath.mpf(G) / (j - mpmath.mpf(1) / 2))) / 3 / star for j in range(1, G + 1)]
        kj = [mpmath.fsum(mpmath.log1p(-th * v) for v in xs) / N for th in theta]
        lj = [N * (mpmath.log(-th / k) - k - 1) for th, k in zip(theta, kj)]
        w = [1 / mpmath.fsum(mpmath.exp(li - lv) for li in lj) for lv in lj]
        th = mpmath.fsum(a * b for a, b in zip(theta, w))
        k = mpmath.fsum(mpmath.log1p(-th * v) for v in xs) / N
        sigma = -k / th
        kappa = mpmath.fsum(abs(th * v / (1 - th * v)) for v in xs) / N
        k = (k * N + 5) / (N + 10)
        return float(k), float(sigma), float(kappa)


# ---- dense PSIS ---------------------------------------------------------------------------------------------------
def psis_dense(l, fit, smooth=True):
    """l [n]: a datum's terms under all n samples (no NaN).  Returns (elpd, k_hat, M): the log ratios -l are sorted, the M
    largest cut off at the (M+1)-th, fitted by `fit` (exceedances of the ratios about the cutoff, after the shift by the
    maximum), replaced by the fitted distribution's quantiles at (j + 1/2) / M, truncated at the largest raw ratio, and
    elpd = ln(sum w exp(l)) - ln(sum w) over all n samples"""
    l = np.asarray(l, dtype=np.float64)
    n = len(l)
    order = np.argsort(order_keys(-l), kind="stable")
    lw = (-l)[order]                                        # ascending
    top = lw[-1]
    raw = lw - top
    new = raw.copy()
    M = int(math.ceil(min(0.2 * n, 3.0 * math.sqrt(n))))
    M = min(M, n - 1)
    k_hat = math.inf
    if M >= 5 and raw[-1] - raw[n - M] >= 2.0 ** -52 / 100:
        cut = float(np.exp(raw[n - M - 1]))
        k_hat, sigma = fit(np.exp(raw[n - M:]) - cut)[:2]
        if k_hat != k_hat:
            k_hat = math.inf
        if smooth and math.isfinite(k_hat):
            for j in range(M):
                p = (j + 0.5) / M
                q = -sigma * math.log1p(-p) if k_hat == 0 else sigma * math.expm1(-k_hat * math.log1p(-p)) / k_hat
                new[n - M + j] = min(0.0, math.log(q + cut))
    num = math.fsum(math.exp(a - b) for a, b in zip(new.tolist(), raw.tolist()))
    den = math.fsum(math.exp(a) for a in new.tolist())
    return math.log(num) - top - math.log(den), k_hat, M
