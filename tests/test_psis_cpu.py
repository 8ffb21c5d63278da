"""apemost_amd/psis.py against tests/psis_ref.py, a dense restatement that shares nothing with it (no GPU).

The bounds (u = 2^-53):

Fit.  k_j is a mean of N terms log1p(-theta_j x), each good to an ulp, summed pairwise: a few ulps of the mean of their
magnitudes.  l_j = N (...) multiplies that by N, so the G weights, and theta-hat with them, carry a relative error of
about N ulps plus G ulps of their own sums.  k is a mean of log1p(-theta-hat x): a relative change e of theta-hat moves
it by e * kappa, kappa = mean |theta x / (1 - theta x)| (taken from the restatement), and its own N-term mean adds ulps
of |k|; the adjustment (k N + 5) / (N + 10) shrinks both.  Allowing 8 ulps for every one counted:
    |k - k_ref| <= 8 (N + G) 2^-52 (kappa + |k| + 1),     sigma to the same bound, relative,
and the test gives it the project's factor 2.  Worst observed fraction of the doubled bound over the arrays below:
0.00084 (k), 0.0012 (sigma).

Decomposition.  psis() works from S_dn, a sequential sum of n exponentials good to n 2^-50 relative (the rule of
tests/test_gpu_pointwise.py), which the smoothed denominator S_dn - sum exp(t) + sum exp(s) carries as n 2^-50 * ratio
relative, ratio being what psis() reports.  Beside it stand at most 64 roundings of the magnitudes involved (two
logarithms, the subtractions of m, the exponentials of t, s and s - t with |s - t| < 40, the quantile's log, expm1 and
log1p): 64 * 2^-52 (1 + |m| + |elpd|).  With the factor 2:
    |elpd - elpd_dense| <= 2 (n 2^-50 ratio + 2^-46 (1 + |m| + |elpd|)).
Worst observed fraction: 0.00056 (n = 20000, M = 425, k-hat 0.44, 1.89, 4.52).

Recovery (recorded, not asserted as a distance): k = -0.3, 0.1, 0.3, 0.7, 1.2 give k-hat = -0.28899, 0.10561, 0.30303,
0.69773, 1.19098 on the exact quantiles at (j - 1/2) / 1000.

A series with a NaN term: the fold's S_dn is NaN there (pt_pointwise.h has no filter), so elpd_loo is NaN exactly as
Pointwise.elpd_loo is; what must be finite is pareto_k and tail_len, which come from the tail alone."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import psis, workloads as wl
from apemost_amd.pointwise import Pointwise
from apemost_amd.psis import PointwiseTail, capacity_for, gpdfit, k_threshold, tail_length
from tests import psis_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_pair(l, capacity=None, chains=(0,)):
    """l [n][n_data] (one kept chain) -> the Pointwise and PointwiseTail a device fold of these terms would give"""
    l = np.asarray(l, dtype=np.float64)
    n, nd = l.shape
    st = psis_ref.fold_state(l)
    pw = Pointwise([n], *[st[f] for f in ("origin", "sum", "sq", "m_up", "S_up", "m_dn", "S_dn", "S2_dn")], np.zeros((1, 4)),
                   np.zeros((1, 4)), list(chains), np.arange(nd, dtype=float), np.zeros(nd), 4, wl.MODEL_SIMPLESIN)
    capacity = capacity_for(n) if capacity is None else capacity
    count, values = psis_ref.select(-l, capacity)
    return pw, PointwiseTail(count, values, capacity, list(chains), n)


# ---- the fit ----------------------------------------------------------------------------------------------------------
def fit_arrays():
    rng = np.random.default_rng(7)
    out = []
    for N, shapes in ((5, (0.2, 0.9, 3.0)), (20, (0.2, 0.9, 3.0)), (425, (0.2, 0.9, 3.0)), (4095, (0.9,))):
        for kk in shapes:
            out.append(np.sort(np.expm1(kk * rng.exponential(size=N)) / kk))
    return out


def test_fit_against_mpmath():
    worst_k = worst_s = 0.0
    for x in fit_arrays():
        N = len(x)
        G = 30 + int(math.sqrt(N))
        k, sigma = gpdfit(x)
        k_ref, s_ref, kappa = psis_ref.gpdfit_mp(x)
        bound = 2 * 8 * (N + G) * 2.0 ** -52 * (kappa + abs(k_ref) + 1)
        fk, fs = abs(k - k_ref) / bound, abs(sigma - s_ref) / abs(s_ref) / bound
        print("N %d: k %.17g (ref %.17g) %.3g of the bound, sigma %.3g of it" % (N, k, k_ref, fk, fs))
        worst_k, worst_s = max(worst_k, fk), max(worst_s, fs)
        assert fk <= 1 and fs <= 1, (N, k, k_ref, sigma, s_ref)
    print("worst fractions: k %.3g, sigma %.3g" % (worst_k, worst_s))


def test_fit_recovers_the_shape_of_exact_quantiles():
    p = (np.arange(1, 1001) - 0.5) / 1000
    thr = k_threshold(10 ** 5)
    assert thr == 0.7
    got = []
    for k in (-0.3, 0.1, 0.3, 0.7, 1.2):
        k_hat, sigma = gpdfit(1.0 * np.expm1(-k * np.log1p(-p)) / k)
        print("k %g: k-hat %.5f (off by %.5f), sigma %.5f" % (k, k_hat, k_hat - k, sigma))
        assert (k_hat <= thr) == (k <= thr) and (k_hat <= 1) == (k <= 1), (k, k_hat)
        got.append(k_hat)
    assert all(a < b for a, b in zip(got, got[1:])), got


def test_fit_of_nan_is_infinite():
    assert gpdfit(np.zeros(8))[0] == math.inf                 # 0 / 0 all the way


# ---- the decomposition ---------------------------------------------------------------------------------------------------
CACHE = {}


def heavy_case():
    """20000 samples of three data whose leave-one-out ratios are Pareto with shapes 0.5, 2 and 4.4"""
    if "heavy" not in CACHE:
        rng = np.random.default_rng(11)
        n = 20000
        l = -(np.array([0.5, 2.0, 4.4]) * rng.exponential(size=(n, 3))) - 3.0
        CACHE["heavy"] = l, host_pair(l)
    return CACHE["heavy"]


def elpd_bound(n, ratio, m, elpd):
    return 2 * (n * 2.0 ** -50 * ratio + 2.0 ** -46 * (1 + abs(m) + abs(elpd)))


def test_decomposition_against_the_dense_algorithm():
    l, (pw, tail) = heavy_case()
    n = len(l)
    assert tail_length(n) == 425 and tail.capacity == 426 and (tail.count == 426).all()
    res = psis.psis(pw, tail)
    raw = psis.psis(pw, tail, smooth=False)
    plain = pw.elpd_loo()
    worst = 0.0
    for i in range(3):
        elpd, k_hat, M = psis_ref.psis_dense(l[:, i], gpdfit)
        assert M == 425 == res.tail_len[i] and not res.tail_short[i]
        assert np.float64(k_hat).tobytes() == np.float64(res.k[i]).tobytes(), (i, k_hat, res.k[i])
        b = elpd_bound(n, res.ratio[i], pw.m_dn[0, i], elpd)
        f = abs(res.elpd[i] - elpd) / b
        print("datum %d: k-hat %.4f, elpd %.15g (dense %.15g), ratio %.4g, %.3g of the bound" % (i, k_hat, res.elpd[i], elpd,
                                                                                                 res.ratio[i], f))
        worst = max(worst, f)
        assert f <= 1
        # the restatement's own fit agrees about k-hat to the fit test's bound
        k_mp = psis_ref.psis_dense(l[:, i], psis_ref.gpdfit_mp)[1]
        assert abs(k_mp - k_hat) < 1e-9
        # unsmoothed: the plain importance-sampling estimate, from the formula with s = t
        dense_raw = psis_ref.psis_dense(l[:, i], gpdfit, smooth=False)[0]
        for other in (plain[i], dense_raw):
            assert abs(raw.elpd[i] - other) <= elpd_bound(n, raw.ratio[i], pw.m_dn[0, i], other)
        assert raw.ratio[i] == pytest.approx(1.0, abs=1e-9) and raw.k[i] == res.k[i]
    assert abs(res.k[0] - 0.5) < 0.15 and abs(res.k[1] - 2.0) < 0.3 and abs(res.k[2] - 4.4) < 0.6, res.k
    print("worst fraction %.3g" % worst)
    tab = res.k_table()
    assert tab["good"].tolist() == [0] and tab["bad"].tolist() == [] and tab["very bad"].tolist() == [1, 2]
    assert res.k_threshold() == k_threshold(n) == 0.7
    assert res.looic() == -2.0 * (res.elpd[0] + res.elpd[1] + res.elpd[2])
    assert res.p_loo() == pytest.approx(float(np.sum(pw.lppd()) - np.sum(res.elpd)))
    assert res.se() > 0 and res.compare(raw)[0] == pytest.approx(float(np.sum(res.elpd - raw.elpd)))
    assert res.text().splitlines()[0] == "n\t20000" and len(res.text().splitlines()) == 10 + 3


# ---- the edges -------------------------------------------------------------------------------------------------------
def run(l, capacity=None):
    pw, tail = host_pair(np.asarray(l, dtype=np.float64), capacity)
    return pw, tail, psis.psis(pw, tail)


def test_edges():
    rng = np.random.default_rng(3)
    # M < 5: 20 samples give M = 4
    pw, tail, r = run(-rng.exponential(size=(20, 2)))
    assert r.tail_len.tolist() == [4, 4] and (r.k == math.inf).all() and np.isfinite(r.elpd).all()
    assert np.allclose(r.elpd, pw.elpd_loo(), rtol=0, atol=1e-13)
    # the capacity cuts the tail short: 1000 samples want M = 95, a capacity of 40 gives 39
    l = -rng.exponential(size=(1000, 2))
    pw, tail, r = run(l, capacity=40)
    assert tail_length(1000) == 95 and r.tail_len.tolist() == [39, 39] and r.tail_short.all()
    assert np.isfinite(r.k).all() and np.isfinite(r.elpd).all()
    full = run(l)[2]
    assert not full.tail_short.any() and full.tail_len.tolist() == [95, 95]
    # all tail values equal
    l = -rng.exponential(size=(1000, 1))
    l[:200, 0] = -7.5                                          # the 200 largest ratios are one value
    pw, tail, r = run(l)
    assert r.k[0] == math.inf and r.tail_len[0] == 95 and abs(r.elpd[0] - pw.elpd_loo()[0]) < 1e-12
    # a series with NaN terms: the count is short, k comes from the tail, elpd is the fold's NaN
    l = -rng.exponential(size=(1000, 2))
    l[5::7, 1] = np.nan
    pw, tail, r = run(l)
    assert int(tail.count[0, 1]) == 96 and np.isfinite(r.k).all() and r.tail_len.tolist() == [95, 95]
    assert np.isfinite(r.elpd[0]) and np.isnan(r.elpd[1]) and np.isnan(pw.elpd_loo()[1])
    l[:, 1] = np.nan                                           # nothing but NaN: an empty tail
    pw, tail, r = run(l)
    assert int(tail.count[0, 1]) == 0 and r.tail_len[1] == 0 and r.k[1] == math.inf and r.tail_short[1]
    # +inf among the ratios (a term of -inf): no fit, and the elpd of a sample that excludes the datum
    l = -rng.exponential(size=(1000, 2))
    l[17, 0] = -math.inf
    pw, tail, r = run(l)
    assert tail.values[0, 0, 0] == math.inf and r.k[0] == math.inf and math.isfinite(r.k[1]) and math.isfinite(r.elpd[1])
    assert not math.isfinite(r.elpd[0])
    l[17, 0] = math.inf                                        # -inf among the ratios, far below the tail
    pw, tail, r = run(l)
    assert math.isfinite(r.k[0]) and math.isfinite(r.elpd[0])
    # one sample
    pw, tail, r = run([[-1.25, -0.5]])
    assert capacity_for(1) == 2 and r.tail_len.tolist() == [0, 0] and (r.k == math.inf).all()
    assert r.elpd.tolist() == [-1.25, -0.5] and not r.tail_short.any()


# ---- files, mismatches, the command line ---------------------------------------------------------------------------------------
def test_capacity_rule():
    assert [tail_length(n) for n in (1, 10, 100, 225, 1000, 20000, 10 ** 6)] == [1, 2, 20, 45, 95, 425, 3000]
    assert tail_length(1000, r_eff=0.25) == 190
    assert [capacity_for(n) for n in (1, 100, 10 ** 6, 1860000, 1870000, 10 ** 8)] == [2, 21, 3001, 4093, 4096, 4096]
    assert k_threshold(100) == 0.5 and k_threshold(10 ** 6) == 0.7 and k_threshold(1) == -math.inf


def test_round_trip_mismatches_and_command_line(tmp_path):
    l, (pw, tail) = heavy_case()
    path = str(tmp_path / "pointwise_tail.bin")
    tail.write(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"APEMOSTT" and len(raw) == 56 + 4 + 8 * 3 + 8 * 3 * 426
    back = PointwiseTail.read(path)
    back.write(str(tmp_path / "again.bin"))
    assert open(str(tmp_path / "again.bin"), "rb").read() == raw
    assert back.n == 20000 and back.capacity == 426 and back.values.tobytes() == tail.values.tobytes()
    assert [t.n_keep for t in back.per_ladder(1)] == [1]
    (tmp_path / "bad.bin").write_bytes(b"APEMOSTW" + raw[8:])                # the pointwise fold's magic
    (tmp_path / "short.bin").write_bytes(raw[:-8])
    for name in ("bad.bin", "short.bin"):
        with pytest.raises(ValueError):
            PointwiseTail.read(str(tmp_path / name))
    with pytest.raises(ValueError):
        PointwiseTail(np.full((1, 3), 9), np.zeros((1, 3, 4)), 4, [0], 10)  # a count above the capacity
    for other in (PointwiseTail(tail.count, tail.values, 426, [0], 19999),
                  PointwiseTail(tail.count, tail.values, 426, [1], 20000),
                  PointwiseTail(tail.count[:, :2], tail.values[:, :2], 426, [0], 20000)):
        with pytest.raises(ValueError):
            psis.psis(pw, other)
    pw.write(str(tmp_path / "pointwise.bin"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, "-m", "apemost_amd.psis", str(tmp_path)], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=120)
    assert out.returncode == 0 and out.stdout == psis.psis(pw, tail).text(), out.stderr
    out = subprocess.run([sys.executable, "-m", "apemost_amd.psis", str(tmp_path / "nowhere")], stdout=subprocess.PIPE,
                         stderr=subprocess.PIPE, universal_newlines=True, env=env, timeout=120)
    assert out.returncode == 1 and "psis:" in out.stderr
