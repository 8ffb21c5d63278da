"""Reweighted posteriors restated for the tests: it shares nothing with apemost_amd/reweight.py or the kernels.  The
weights are numpy's exp of the arguments tests/mbar_ref.py forms, every floating-point sum is math.fsum (exact
summation of the rounded products) and every fixed-point sum is a sum of Python integers.  One ladder at a time:
ell [T][K] (kept step, chain), x [k][T][K] the columns, betas [K]."""
import math

import numpy as np

from tests.summary_rows import gsl_edges


def conjugate(K=8, T=2000, d=4, seed=20080614, beta_max=1.0, beta_min=0.01):
    """mbar_ref.conjugate with its draws: the same generator calls, so betas and ell are its own on the bits.  Returns
    (betas [K], ell [T][K], x [d][T][K]): the chain at beta draws x ~ N(0, I / (1 + beta)), and so does the posterior at
    any beta: mean 0 and variance 1 / (1 + beta) in every coordinate."""
    rng = np.random.default_rng(seed)
    betas = beta_max * (beta_min / beta_max) ** (np.arange(K) / max(K - 1, 1)) if K > 1 else np.array([beta_max])
    x = rng.standard_normal((T, K, d)) / np.sqrt(1.0 + betas)[None, :, None]
    return betas, -0.5 * (x * x).sum(axis=2), np.ascontiguousarray(np.moveaxis(x, 2, 0))


def shift_of(N):
    return 63 - int(N).bit_length()


def bin_of(v, e):
    """gsl_histogram_increment over the edges e: the bin of v, or -1 outside [e[0], e[n]) and for NaN"""
    n = len(e) - 1
    if not (v >= e[0] and v < e[n]):
        return -1
    left, right = 0, n
    while right - left > 1:
        mid = (left + right) // 2
        if v >= e[mid]:
            left = mid
        else:
            right = mid
    return left


def weights(ell, lnD, beta_t):
    """(m, e [N]) of one target: e = exp((beta_t l - lnD) - m)"""
    x = beta_t * ell.reshape(-1) - lnD
    m = float(x.max())
    return m, np.exp(x - m), float(np.abs(x).max())


def sums(x, ell, lnD, beta_t, lo=None, hi=None, nbins=0):
    """dict of one target over the columns x [k][T][K]: m, S0, SS, origin [k], S1 [k], cross {(a, b)}, the scales
    A1 [k] = sum e |d_a| and A2 {(a, b)} = sum e |d_a d_b|, e [N], q [N] (Python integers), hist [k][nbins] and q_total
    (Python integers), shift, x_abs_max"""
    k = len(x)
    m, e, x_abs_max = weights(ell, lnD, beta_t)
    N = len(e)
    cols = [np.ascontiguousarray(x[a]).reshape(-1) for a in range(k)]
    d = [c - c[0] for c in cols]
    s = shift_of(N)
    q = [int(v) for v in np.rint(np.ldexp(e, s)).tolist()]
    out = dict(m=m, S0=math.fsum(e.tolist()), SS=math.fsum((e * e).tolist()), origin=[float(c[0]) for c in cols],
               S1=[math.fsum((e * d[a]).tolist()) for a in range(k)], A1=[math.fsum((e * np.abs(d[a])).tolist()) for a in range(k)],
               cross={}, A2={}, e=e, q=q, q_total=sum(q), shift=s, x_abs_max=x_abs_max, hist=[], bins=[])
    for a in range(k):
        ed = e * d[a]
        for b in range(a, k):
            out["cross"][a, b] = math.fsum((ed * d[b]).tolist())
            out["A2"][a, b] = math.fsum((e * np.abs(d[a] * d[b])).tolist())
    for a in range(k if nbins else 0):
        edges = gsl_edges(float(lo[a]), float(hi[a]), nbins)
        bins = [bin_of(v, edges) for v in cols[a].tolist()]
        h = [0] * nbins
        for b, w in zip(bins, q):
            if b >= 0:
                h[b] += w
        out["hist"].append(h)
        out["bins"].append(bins)
    return out


def errors_over_bounds(got, b, t, ref, E_x, R0, nbins):
    """every word of target t of ladder b of `got` (a Reweighted: m, S0, SS, S1, cross, hist, q_total) against the
    sums() dict `ref`, as error / bound, with (E_x, R0) of mbar_ref.bounds.  With u = 2^-53: two evaluations that follow
    the stated operations differ in e_n by at most (2 E_x + 4 u) e_n (the argument by 2 E_x, one ulp per exp on either
    side), hence |q - q_ref| <= 2^s (2 E_x + 4 u) e + 1 per sample (half a unit per rint), and a bin or q_total by the
    sum of that over its samples.  m, S0 and SS are MBAR's (E_x, R0, 2 R0 + 2 u).  d is the same subtraction on both
    sides; a term of S1 carries one product on either side and changes sign: (R0 + 2 u) sum e |d_a|; a term of cross
    two products: (R0 + 4 u) sum e |d_a d_b|."""
    u = 2.0 ** -53
    k = len(ref["S1"])
    per_q = 2.0 ** ref["shift"] * (2 * E_x + 4 * u)
    e = ref["e"]
    out = {"m": abs(got.m[b, t] - ref["m"]) / E_x,
           "S0": abs(got.S0[b, t] / ref["S0"] - 1) / R0,
           "SS": abs(got.SS[b, t] / ref["SS"] - 1) / (2 * R0 + 2 * u),
           "q_total": abs(int(got.q_total[b, t]) - ref["q_total"]) / (per_q * ref["S0"] + len(e))}
    s1 = c = h = 0.0
    for a in range(k):
        if ref["A1"][a] > 0:
            s1 = max(s1, abs(got.S1[b, t, a] - ref["S1"][a]) / ((R0 + 2 * u) * ref["A1"][a]))
        else:
            s1 = max(s1, float(got.S1[b, t, a] != 0))
        for a2 in range(a, k):
            at = a * k - a * (a - 1) // 2 + (a2 - a)
            if ref["A2"][a, a2] > 0:
                c = max(c, abs(got.cross[b, t, at] - ref["cross"][a, a2]) / ((R0 + 4 * u) * ref["A2"][a, a2]))
            else:
                c = max(c, float(got.cross[b, t, at] != 0))
        if nbins:
            bins = np.array(ref["bins"][a])
            for bin_ in range(nbins):
                inside = bins == bin_
                bound = per_q * math.fsum(e[inside].tolist()) + int(inside.sum())
                diff = abs(int(got.hist[b, t, a, bin_]) - ref["hist"][a][bin_])
                h = max(h, diff / bound if bound > 0 else float(diff != 0))
    out.update(S1=s1, cross=c, hist=h)
    return out


def estimates(ref, a):
    """(mean, variance, ESS) of column slot a from a sums() dict"""
    r = ref["S1"][a] / ref["S0"]
    return ref["origin"][a] + r, ref["cross"][a, a] / ref["S0"] - r * r, ref["S0"] ** 2 / ref["SS"]
