"""The residual periodogram without a device: the ABI declares and exports the entry points, tests/periodogram_ref.py
restates the rule, the header's helpers built by the host compiler under the sanitizers give its bits
(tests/periodogram_rule.cpp, a program of its own), and apemost_amd/periodogram.py's weights and file on synthetic state."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi, periodogram as pg
from tests import periodogram_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "apemost_amd", "csrc")
ENTRIES = ["apemost_hip_periodogram_begin", "apemost_hip_periodogram_accumulate", "apemost_hip_periodogram_get",
           "apemost_hip_periodogram_set", "apemost_hip_periodogram_lengths", "apemost_hip_periodogram_end",
           "apemost_hip_periodogram_values"]
NAN, INF = math.nan, math.inf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in ENTRIES:
        assert "int %s(" % name in header, name
        assert name in capi.EXPORTS and getattr(L, name), name
    assert "apemost_hip_periodogram_view" in header
    assert "#define APEMOST_PERIODOGRAM_PIECE %d\n" % pg.PIECE in header
    assert "#define APEMOST_HIP_ABI_VERSION 3" in header and L.apemost_hip_abi_version() == capi.ABI_VERSION == 3
    assert [f for f, _ in capi.PeriodogramView._fields_] == ["n"] + list(pg.STATE) + ["exceed"] + list(pg.PEAK_STATE) + ["peak_counts"]


# ---- 1. the rule on values worked out by hand --------------------------------------------------------------------------------
def test_the_fused_multiply_add_of_the_reference():
    assert ref.fma(3.0, 4.0, 5.0) == 17.0
    # 1 + 2^-52 squared is 1 + 2^-51 + 2^-104: the product rounded first loses the last term, the fused form keeps it
    a = 1.0 + 2.0 ** -52
    assert a * a - (1.0 + 2.0 ** -51) == 0.0 and ref.fma(a, a, -(1.0 + 2.0 ** -51)) == 2.0 ** -104
    assert bits(ref.fma(0.0, -1.0, 0.0))[0] == bits(0.0)[0] and bits(ref.fma(0.0, -1.0, -0.0))[0] == bits(-0.0)[0]
    assert bits(ref.fma(2.0, 3.0, -6.0))[0] == bits(0.0)[0]
    assert math.isnan(ref.fma(INF, 0.0, 1.0)) and math.isnan(ref.fma(INF, 1.0, -INF)) and ref.fma(-INF, 2.0, 1.0) == -INF
    assert ref.fma(1e308, 10.0, 0.0) == INF and ref.fma(1e308, 10.0, -INF) == -INF


def test_the_rule_on_values_taken_by_hand():
    r = np.array([1.0, -2.0, 0.5])
    c = np.array([[1.0, 0.5, -1.0], [0.0, 1.0, 1.0]])
    s = np.array([[0.0, 1.0, 2.0], [1.0, 0.0, 0.0]])
    w = np.array([[1.0, 0.0, 1.0], [0.5, 2.0, 0.25]])
    C, S, P, m, arg = ref.row(r, c, s, w)
    assert C.tolist() == [1.0 - 1.0 - 0.5, -2.0 + 0.5] and S.tolist() == [-2.0 + 1.0, 1.0]
    assert P.tolist() == [(0.25 + 0.0) + 1.0, ((0.5 * -1.5) * -1.5 + (2.0 * -1.5) * 1.0) + 0.25]
    assert (m, arg) == (1.25, 0)
    # a tie: the first occurrence wins; NaN in the middle never does; nothing above -inf: arg = n_freq
    assert ref.peak([1.0, 3.0, 3.0, 2.0]) == (3.0, 1)
    assert ref.peak([1.0, NAN, 0.5]) == (1.0, 0) and ref.peak([NAN, 2.0, NAN, 2.0]) == (2.0, 1)
    assert ref.peak([NAN, NAN, NAN]) == (-INF, 3) and ref.peak([-INF, -INF]) == (-INF, 2) and ref.peak([-INF, INF]) == (INF, 1)
    # a NaN residual reaches every frequency's sums; the peak then has no frequency
    C, S, P, m, arg = ref.row(np.array([1.0, NAN]), c[:, :2], s[:, :2], w)
    assert np.isnan(C).all() and np.isnan(P).all() and (m, arg) == (-INF, 2)
    # the range of the trig: predict_sine_in_range with ph = 0.25
    assert ref.in_range(1.0, 5.5e12) and not ref.in_range(1.0, 5.7e12) and not ref.in_range(NAN, 1.0) and not ref.in_range(INF, 0.0)


def test_the_sequential_words():
    P = [2.0, NAN, 1.0, 2.5, INF]
    C = [1.0, 2.0, 3.0, 4.0, 5.0]
    S = [-1.0, 0.5, 0.25, 0.0, 1.0]
    q = ref.RefSeries(P[:4], C[:4], S[:4], 1.5)
    assert q.origin == 2.0 and math.isnan(q.sum) and math.isnan(q.sq) and (q.min, q.max) == (1.0, 2.5)
    assert (q.sum_c, q.sum_s, q.exceed) == (10.0, -0.25, 2)
    q = ref.RefSeries([P[0]] + P[2:], [C[0]] + C[2:], [S[0]] + S[2:], INF)
    assert (q.origin, q.min, q.max, q.exceed) == (2.0, 1.0, INF, 0) and q.sum == INF
    # a plain Python loop gives the same words
    vals = [0.1 * t * t - t for t in range(11)]
    origin, total, sq, mn, mx = vals[0], 0.0, 0.0, INF, -INF
    for v in vals:
        d = v - origin
        total += d
        sq += d * d
        mn, mx = (v if v < mn else mn), (v if v > mx else mx)
    q = ref.RefSeries(vals, vals, vals, 0.0)
    assert (q.origin, q.sum, q.sq, q.min, q.max) == (origin, total, sq, mn, mx) and q.exceed == sum(v > 0.0 for v in vals)
    e = ref.RefSeries([], [], [], 0.0)
    assert (e.origin, e.sum, e.sq, e.min, e.max, e.sum_c, e.exceed) == (0.0,) * 6 + (0,)
    pk = ref.RefPeak([3.0, -INF, 2.0], [1, 4, 1], 4)
    assert pk.origin == 3.0 and pk.sum == -INF and (pk.min, pk.max) == (-INF, 3.0) and pk.counts.tolist() == [0, 2, 0, 0, 1]


# ---- 2. the helpers under the sanitizers ------------------------------------------------------------------------------------
def test_helpers_built_by_the_host_compiler_under_the_sanitizers(tmp_path):
    """the header's helpers, compiled for the host, give periodogram_ref's bits for every length the kernels treat
    differently, with ties, zeros of both signs and non-finite values"""
    rng = np.random.default_rng(21)
    blocks = []
    for L in (1, 2, 63, 64, 65):
        for n_freq in (1, 64, 65):
            r = rng.standard_normal(L) * 10.0 ** rng.integers(-3, 4, L)
            blocks.append((r, rng.uniform(-1, 1, (n_freq, L)), rng.uniform(-1, 1, (n_freq, L)),
                           rng.standard_normal((n_freq, 3)) * 10.0 ** rng.integers(-2, 3, (n_freq, 1))))
    one = np.ones((3, 2))
    blocks.append((np.array([1.0, 1.0]), one, one, np.array([[1.0, 0.0, 0.0]] * 3)))                 # a tie in P
    blocks.append((np.array([NAN, 1.0]), one, one, np.ones((3, 3))))                                # all NaN
    blocks.append((np.array([1.0, 2.0]), np.array([[1.0, 1.0], [NAN, 1.0], [1.0, 1.0]]), one, np.ones((3, 3))))  # NaN amid
    blocks.append((np.array([-0.0, 0.0]), one, -one, np.array([[INF, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, 0.0, 0.0]])))
    blocks.append((np.array([1e200, 1e200]), 1e200 * one, one, np.array([[1.0, 0.0, 0.0], [-1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])))
    src = tmp_path / "blocks.txt"
    src.write_text("".join("%d %d " % (len(r), len(c)) + " ".join(
        "%016x" % int(b) for b in np.concatenate([bits(r), bits(c).ravel(), bits(s).ravel(), bits(w).ravel()])) + "\n"
        for r, c, s, w in blocks))
    exe = str(tmp_path / "periodogram_rule")
    subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(HERE, "periodogram_rule.cpp"), "-o", exe])
    run = subprocess.run([exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    lines = run.stdout.splitlines()
    assert len(lines) == len(blocks)
    for (r, c, s, w), line in zip(blocks, lines):
        words = line.split()
        n_freq = len(c)
        got = np.array([int(v, 16) for v in words[:-1]], dtype=np.uint64).view(np.float64)
        C, S, P, m, arg = ref.row(r, c, s, w)
        want = np.concatenate([C, S, P, [m]])
        same = (bits(got) == bits(want)) | (np.isnan(got) & np.isnan(want))
        assert same.all(), (len(r), n_freq, np.flatnonzero(~same)[:5], got[~same][:5], want[~same][:5])
        assert int(words[-1]) == arg, (len(r), n_freq, words[-1], arg)


# ---- 3. the weights (host policy) ---------------------------------------------------------------------------------------------
def uneven(rng, L=120):
    return np.sort(rng.uniform(0.0, 40.0, L))


def test_amplitude2_returns_the_squared_amplitude_of_a_pure_sinusoid():
    rng = np.random.default_rng(3)
    x = uneven(rng)
    nu, amp, phase = 0.731, 1.7, 0.4
    y = amp * np.sin(2 * np.pi * (nu * x + phase))
    freqs = np.array([0.2, nu, 1.3])
    w = pg.weights(x, freqs, "amplitude2")
    arg = 2 * np.pi * np.outer(freqs, x)
    Cs, Ss = (y * np.cos(arg)).sum(1), (y * np.sin(arg)).sum(1)
    P = pg.power(w, Cs, Ss)
    assert P[1] == pytest.approx(amp * amp, rel=1e-9)
    assert P[0] < 0.5 * amp * amp and P[2] < 0.5 * amp * amp


def test_lomb_scargle_is_half_the_drop_in_chi2_of_the_least_squares_sinusoid():
    rng = np.random.default_rng(4)
    x = uneven(rng)
    sigma = 0.3
    y = 0.8 * np.sin(2 * np.pi * 0.41 * x + 1.0) + sigma * rng.standard_normal(len(x))
    freqs = np.array([0.05, 0.41, 0.9, 2.2])
    w = pg.weights(x, freqs, "lomb_scargle", sigma)
    for j, nu in enumerate(freqs):
        A = np.stack([np.cos(2 * np.pi * nu * x), np.sin(2 * np.pi * nu * x)], 1)
        coef = np.linalg.lstsq(A, y, rcond=None)[0]
        drop = (np.sum(y * y) - np.sum((y - A @ coef) ** 2)) / (sigma * sigma)
        P = pg.power(w[j], np.sum(y * A[:, 0]), np.sum(y * A[:, 1]))
        assert P == pytest.approx(0.5 * drop, rel=1e-9), (j, P, drop)


def test_schuster_and_singular_grams():
    x = np.arange(16.0)
    w = pg.weights(x, [0.0, 0.1, 0.5], "schuster", 2.0)
    assert w.tolist() == [[1.0 / 64.0, 0.0, 1.0 / 64.0]] * 3
    for kind in ("lomb_scargle", "amplitude2"):
        w = pg.weights(x, [0.0, 0.1, 0.5], kind, 2.0)       # nu = 0 and the Nyquist frequency of an even grid: sin is 0
        assert w[0].tolist() == [0.0, 0.0, 0.0] and np.all(w[1] != 0.0), kind
        assert np.abs(w[2]).max() == 0.0, kind
    with pytest.raises(ValueError):
        pg.weights(x, [0.1], "fourier")
    with pytest.raises(ValueError):
        pg.weights(x, [0.1], "schuster", 0.0)


def test_lomb_scargle_power_of_white_noise_has_mean_one():
    """2000 seeded draws of white noise of known sigma: the reference-rule LS power at a fixed frequency is Exp(1), so
    its mean lies within 4 standard errors (4 / sqrt(2000)) of 1"""
    rng = np.random.default_rng(5)
    x = uneven(rng, 40)
    sigma, nu = 0.5, 0.37
    w = pg.weights(x, [nu], "lomb_scargle", sigma)[0]
    c, s = np.cos(2 * np.pi * nu * x), np.sin(2 * np.pi * nu * x)
    P = []
    for _ in range(2000):
        C_, S_ = ref.sums(sigma * rng.standard_normal(len(x)), c, s)
        P.append(ref.power(w, C_, S_))
    P = np.array(P)
    se = P.std(ddof=1) / math.sqrt(len(P))
    assert abs(P.mean() - 1.0) < 4 * se and 0.8 < P.std(ddof=1) < 1.2, (P.mean(), se, P.std(ddof=1))


# ---- 4. the Python object -----------------------------------------------------------------------------------------------------
def synthetic(n_keep=2, n_freq=5, n=7, seed=0):
    rng = np.random.default_rng(seed)
    freqs = np.linspace(0.1, 0.5, n_freq)
    w = rng.uniform(0.5, 1.5, (n_keep, n_freq, 3))
    level = np.array([1.0, INF][:n_keep])
    p = pg.Periodogram.empty(np.arange(n_keep) * 3, freqs, w, level, [11] * n_keep, model=3, sigma=0.4, thin=2, n_ladders=1)
    Ps = rng.exponential(1.0, (n, n_keep, n_freq))
    Cs, Ss = rng.standard_normal((n, n_keep, n_freq)), rng.standard_normal((n, n_keep, n_freq))
    for k in range(n_keep):
        for j in range(n_freq):
            q = ref.RefSeries(Ps[:, k, j], Cs[:, k, j], Ss[:, k, j], level[k])
            for f, v in zip(pg.STATE, (q.origin, q.sum, q.sq, q.min, q.max, q.sum_c, q.sum_s)):
                getattr(p, f)[k, j] = v
            p.exceed[k, j] = q.exceed
        peaks = [ref.peak(Ps[t, k]) for t in range(n)]
        q = ref.RefPeak([m for m, _ in peaks], [a for _, a in peaks], n_freq)
        for f, v in zip(pg.PEAK_STATE, (q.origin, q.sum, q.sq, q.min, q.max)):
            getattr(p, f)[k] = v
        p.peak_counts[k] = q.counts
    p.n[0] = n
    return p, Ps, Cs, Ss


def test_what_the_object_says():
    p, Ps, Cs, Ss = synthetic()
    for k in range(2):
        assert p.mean(k) == pytest.approx(Ps[:, k].mean(0), rel=1e-12)
        assert p.var(k) == pytest.approx(Ps[:, k].var(0, ddof=1), rel=1e-10) and p.sd(k) == pytest.approx(Ps[:, k].std(0, ddof=1), rel=1e-10)
        assert p.min(k).tolist() == Ps[:, k].min(0).tolist() and p.max(k).tolist() == Ps[:, k].max(0).tolist()
        assert p.coherent(k) == pytest.approx(pg.power(p.weights[k], Cs[:, k].mean(0), Ss[:, k].mean(0)), rel=1e-12)
        top = np.array([Ps[t, k].max() for t in range(len(Ps))])
        assert p.peak_mean(k) == pytest.approx(top.mean(), rel=1e-12) and p.peak_sd(k) == pytest.approx(top.std(ddof=1), rel=1e-10)
        hist = np.bincount(Ps[:, k].argmax(1), minlength=5)
        assert p.peak_hist(k).tolist() == hist.tolist() and p.n_no_peak(k) == 0
        assert p.peak_frequency(k) == (float(p.freqs[int(hist.argmax())]), hist.max() / 7.0)
    assert p.exceed_fraction(0).tolist() == ((Ps[:, 0] > 1.0).sum(0) / 7.0).tolist() and not p.exceed_fraction(1).any()
    lines = p.text(0).splitlines()
    assert len(lines) == 5 and all(len(l.split("\t")) == 7 for l in lines) and lines[2].split("\t")[0] == "%.15e" % p.freqs[2]
    halves = p.per_ladder(2)
    assert [h.n_keep for h in halves] == [1, 1] and halves[1].sum.tobytes() == p.sum[1:].tobytes()
    back = pg.Periodogram.concat(halves)
    assert back.peak_counts.tobytes() == p.peak_counts.tobytes() and back.chains.tolist() == p.chains.tolist()
    empty = pg.Periodogram.empty([0], p.freqs, p.weights[0], [0.0], [4])
    assert math.isnan(empty.peak_frequency()[0]) and empty.peak_frequency()[1] == 0.0


def test_write_read_round_trip(tmp_path):
    p, _, _, _ = synthetic(seed=2)
    path = str(tmp_path / "periodogram.bin")
    p.write(path)
    q = pg.Periodogram.read(path)
    for f in pg.STATE + pg.PEAK_STATE + ("exceed", "peak_counts", "chains", "freqs", "weights", "level", "lengths", "n"):
        assert getattr(q, f).tobytes() == getattr(p, f).tobytes() and getattr(q, f).dtype == getattr(p, f).dtype, f
    assert (q.model, q.sigma, q.thin, q.n_ladders) == (3, 0.4, 2, 1) and q.text(1) == p.text(1)
    open(path, "ab").write(b"\0")
    with pytest.raises(ValueError):
        pg.Periodogram.read(path)
    open(path, "wb").write(b"APEMOSTK" + bytes(64))
    with pytest.raises(ValueError):
        pg.Periodogram.read(path)


# ---- 5. refusals that need no device ----------------------------------------------------------------------------------------
def test_a_null_sampler_is_refused_by_every_entry_point():
    L = capi.lib()
    ip = C.POINTER(C.c_int32)
    ch = np.zeros(1, dtype=np.int32)
    one = np.zeros(3)
    dp = one.ctypes.data_as(capi._dp)
    view = capi.PeriodogramView()
    calls = [lambda: L.apemost_hip_periodogram_begin(None, 1, ch.ctypes.data_as(ip), 1, dp, dp, dp),
             lambda: L.apemost_hip_periodogram_accumulate(None, None, 0, 0, 1),
             lambda: L.apemost_hip_periodogram_get(None, C.byref(view)),
             lambda: L.apemost_hip_periodogram_set(None, C.byref(view)),
             lambda: L.apemost_hip_periodogram_lengths(None, ch.ctypes.data_as(ip)),
             lambda: L.apemost_hip_periodogram_end(None),
             lambda: L.apemost_hip_periodogram_values(None, 1, dp, 1, dp, dp, 1, dp, dp, dp, dp, dp, dp, dp, dp, dp,
                                                      ch.ctypes.data_as(ip))]
    for call in calls:
        assert call() == capi.ERR_INVALID
        assert b"sampler is NULL" in L.apemost_hip_last_error()
