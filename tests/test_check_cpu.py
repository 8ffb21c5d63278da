"""Predictive checks without a device: the ABI declares and exports the entry points, tests/check_ref.py restates the rule,
the header's helpers built by the host compiler under the sanitizers give its bits (tests/check_rule.cpp, a program of
its own), apemost_hip_check_null_edges against mpmath, and apemost_amd/check.py on synthetic state."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi, check as ck
from tests import check_ref as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "apemost_amd", "csrc")
ENTRIES = ["apemost_hip_check_begin", "apemost_hip_check_accumulate", "apemost_hip_check_get", "apemost_hip_check_set",
           "apemost_hip_check_lengths", "apemost_hip_check_end", "apemost_hip_check_values", "apemost_hip_check_null_edges"]
SIMPLESIN, PULSE, PULSE_VROT, SINE3, USER = 0, 1, 2, 3, 4


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_entry_points_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in ENTRIES:
        assert "int %s(" % name in header, name
        assert name in capi.EXPORTS and getattr(L, name), name
    assert "#define APEMOST_HIP_ABI_VERSION" in header and L.apemost_hip_abi_version() == capi.ABI_VERSION


# ---- 1. the rule in numpy ---------------------------------------------------------------------------------------------------
def test_the_rule_on_values_taken_by_hand():
    e = np.array([1.5, -2.0, 0.5])
    u = np.array([0.75, 0.25, 1.0])
    T = ref.stats(e, u, True)
    assert T.tolist() == [(0.0 + 2.25) + (0.0 + 4.0) + ((0.0 + 0.25) + 0.0), 2.0, (0.0 + 0.0) + (0.25 * -0.25) + (0.5 * -0.25) + 0.0]
    T = ref.stats(e, u, False)
    assert T[0] == (1.5 + -2.0) + 0.5 and T[1] == 1.5
    one = ref.stats(np.array([-0.0]), np.array([0.3]), False)
    assert bits(one).tolist() == bits(np.array([0.0, 0.0, 0.0])).tolist()       # L = 1: SERIAL is +0.0, EXTREME -0.0 + 0.0
    nan = ref.stats(np.array([np.nan, 1.0, -3.0]), np.array([0.5, np.nan, 0.5]), True)
    assert math.isnan(nan[0]) and nan[1] == 3.0 and math.isnan(nan[2])          # a NaN term is skipped by EXTREME alone
    assert ref.stats(np.array([np.nan]), np.array([0.5]), True)[1] == -math.inf
    # 65 data: datum 64 is lane 0's second term, and its predecessor is lane 63's
    u = np.linspace(0.01, 0.99, 65)
    a = u - 0.5
    g = np.concatenate([[0.0], a[1:] * a[:-1]])
    p = g[:64].copy()
    p[0] = p[0] + g[64]
    for _ in range(6):
        p = p[0::2] + p[1::2]
    assert ref.stats(np.zeros(65), u, True)[2] == p[0]


def test_the_sequential_words():
    r = ref.RefSeries([1.0, 3.0, 2.0], [0.5, 0.25, 1.0], [-1.0, -3.0, -2.0])
    assert (r.origin, r.sum, r.sq, r.sum_u, r.m) == (1.0, 0.0 + 2.0 + 1.0, 4.0 + 1.0, 0.5 + 0.25 + 1.0, 3.0)
    w = math.exp(1.0 - 3.0)
    assert r.S == (1.0 * w + 1.0) + math.exp(2.0 - 3.0) and r.SU == (0.5 * w + 0.25) + 1.0 * math.exp(2.0 - 3.0)
    assert r.S_exact == pytest.approx(r.S, rel=1e-15) and r.SU_exact == pytest.approx(r.SU, rel=1e-15)
    s = ref.RefStat([2.0, math.nan, 1.0, 2.5], [1.0, 2.0])
    assert s.origin == 2.0 and math.isnan(s.sum) and (s.min, s.max) == (1.0, 2.5) and s.counts.tolist() == [0, 1, 2, 1]
    assert ck.slots([2.0, math.nan, 1.0, 2.5, 0.0], [1.0, 2.0]).tolist() == [2, 3, 1, 2, 0]


# ---- 2. the helpers under the sanitizers ------------------------------------------------------------------------------------
def test_helpers_built_by_the_host_compiler_under_the_sanitizers(tmp_path):
    """the header's helpers, compiled for the host, give check_ref's bits for every length the kernels treat differently,
    with zeros of both signs and non-finite values"""
    rng = np.random.default_rng(12)
    blocks = []
    for sine in (True, False):
        for L in (1, 2, 64, 65, 130):
            e = rng.standard_normal(L) * 10.0 ** rng.integers(-3, 4, L)
            blocks.append((sine, e if sine else np.abs(e), rng.uniform(size=L)))
        blocks.append((sine, np.array([-0.0]), np.array([0.5])))
        blocks.append((sine, np.array([np.nan, 1.0, -3.0]), np.array([0.5, np.nan, 0.25])))
        blocks.append((sine, np.array([np.nan, np.nan]), np.array([1.0, 0.0])))
        blocks.append((sine, np.array([np.inf] + [1.0] * 64), np.array([1.0] * 64 + [0.0])))
    src = tmp_path / "blocks.txt"
    src.write_text("".join(("s " if sine else "p ") + " ".join("%016x" % int(b) for b in np.concatenate([bits(e), bits(u)])) + "\n"
                           for sine, e, u in blocks))
    exe = str(tmp_path / "check_rule")
    subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(HERE, "check_rule.cpp"), "-o", exe])
    run = subprocess.run([exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert run.returncode == 0, (run.returncode, run.stderr[-2000:])
    got = [[int(w, 16) for w in line.split()] for line in run.stdout.splitlines()]
    assert len(got) == len(blocks)
    for (sine, e, u), g in zip(blocks, got):
        want = ref.stats(e, u, sine)
        for q in range(3):
            if math.isnan(want[q]):
                assert math.isnan(np.uint64(g[q]).view(np.float64)), (sine, len(e), q)
            else:
                assert g[q] == int(bits(want[q])[0]), (sine, len(e), q, g[q], want[q])


# ---- 3. the null quantiles ---------------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 10, 1000, 65536)


@pytest.mark.parametrize("model", [SIMPLESIN, PULSE])
@pytest.mark.parametrize("L", LENGTHS)
def test_null_edges_against_mpmath(model, L):
    """the null CDF at edge j is (j + 1) / (n_edges + 1) within 1e-9: the p-value's resolution is >= 1.2e-4 and bisection
    in fp64 reaches 1e-15, so 1e-9 separates a wrong formula from rounding"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    n_edges = 63
    sine = model == SIMPLESIN
    fit, ext = ck.null_edges(model, ck.FIT, L, n_edges), ck.null_edges(model, ck.EXTREME, L, n_edges)
    worst = 0.0
    for j in range(n_edges):
        p = mp.mpf(j + 1) / (n_edges + 1)
        x = mp.mpf(float(fit[j]))
        cdf = mp.gammainc(mp.mpf(L) / 2, 0, x / 2, regularized=True) if sine else mp.gammainc(mp.mpf(L), 0, x, regularized=True)
        t = mp.mpf(float(ext[j]))
        cdf_ext = (mp.erf(t / mp.sqrt(2)) if sine else 1 - mp.exp(-t)) ** L
        worst = max(worst, abs(float(cdf - p)), abs(float(cdf_ext - p)))
    print("model %d, L %d: worst CDF error %.3g" % (model, L, worst))
    assert worst <= 1e-9


@pytest.mark.parametrize("model", [SIMPLESIN, SINE3, PULSE, PULSE_VROT])
def test_null_edges_ascend_and_serial_is_symmetric(model):
    for L in LENGTHS:
        for n_edges in (1, 2, 255, 256):
            for stat in range(3):
                e = ck.null_edges(model, stat, L, n_edges)
                assert np.isfinite(e).all() and (np.diff(e) > 0).all(), (L, n_edges, stat)
            assert (e == -e[::-1]).all() and (n_edges % 2 == 0 or e[n_edges // 2] == 0.0), (L, n_edges)
    # the normal quantile with the exact null variance (L - 1) / 144
    e = ck.null_edges(model, ck.SERIAL, 145, 3)
    assert e[2] == pytest.approx(0.6744897501960817, rel=1e-14) and e[1] == 0.0
    # the families share their laws
    sine = model in (SIMPLESIN, SINE3)
    for stat in range(3):
        assert ck.null_edges(model, stat, 10, 7).tobytes() == ck.null_edges(SIMPLESIN if sine else PULSE, stat, 10, 7).tobytes()
    # L = 1: EXTREME and FIT are the law of one datum
    one = ck.null_edges(model, ck.FIT, 1, 3), ck.null_edges(model, ck.EXTREME, 1, 3)
    want = [0.6744897501960817 ** 2 if sine else -math.log(0.5), 0.6744897501960817 if sine else -math.log(0.5)]
    assert one[0][1] == pytest.approx(want[0], rel=1e-12) and one[1][1] == pytest.approx(want[1], rel=1e-12)


def test_null_edges_refusals():
    L = capi.lib()
    out = np.zeros(4096)
    dp = out.ctypes.data_as(capi._dp)
    call = L.apemost_hip_check_null_edges
    assert call(SIMPLESIN, 0, 10, 4, dp) == capi.OK
    for args in ((SIMPLESIN, 3, 10, 4), (SIMPLESIN, -1, 10, 4), (SIMPLESIN, 0, 0, 4), (SIMPLESIN, 0, 10, 0),
                 (SIMPLESIN, 0, 10, 4096), (7, 0, 10, 4), (-1, 0, 10, 4)):
        assert call(*args, dp) == capi.ERR_INVALID and b"check_null_edges" in L.apemost_hip_last_error(), args
    assert call(SIMPLESIN, 0, 10, 4, None) == capi.ERR_INVALID
    assert call(USER, 0, 10, 4, dp) == capi.ERR_UNSUPPORTED and b"user-supplied" in L.apemost_hip_last_error()
    assert call(PULSE, 2, 10, 4095, dp) == capi.OK and (np.diff(out[:4095]) > 0).all()
    with pytest.raises(capi.ApemostHipError):
        ck.null_edges(SIMPLESIN, 5, 10, 4)


# ---- 4. p_value on a synthetic null -------------------------------------------------------------------------------------------
def synthetic(n=4000, L=50, nbins=256, seed=77):
    """a Check of one kept chain of a pulse model whose u are iid uniform: e = -log(1 - u) is Exp(1), T by check_ref"""
    rng = np.random.default_rng(seed)
    u = rng.uniform(size=(n, L))
    e = -np.log1p(-u)
    T = ref.stats(e, u, False)
    edges = np.stack([ck.null_edges(PULSE, q, L, nbins - 1) for q in range(3)])
    c = ck.Check.empty([0], np.arange(L, dtype=float), e[0], edges, PULSE)
    c.n[0] = n
    for q in range(3):
        r = ref.RefStat(T[:, q], edges[q])
        c.counts[0, q] = r.counts
        c.stat_origin[0, q], c.stat_sum[0, q], c.stat_sq[0, q], c.stat_min[0, q], c.stat_max[0, q] = r.origin, r.sum, r.sq, r.min, r.max
        assert r.counts.tolist() == np.bincount(ck.slots(T[:, q], edges[q]), minlength=nbins + 1).tolist()
    c.origin[0] = e[0]
    c.sum[0] = (e - e[0]).sum(axis=0)
    c.sq[0] = ((e - e[0]) ** 2).sum(axis=0)
    c.sum_u[0] = u.sum(axis=0)
    c.S[0] = n
    c.SU[0] = u.sum(axis=0)
    return c, T


def test_p_value_on_a_synthetic_null():
    """4000 samples of L = 50 iid uniform u: a p-value is uniform under the null, variance 1/12, so the mean of the 4000
    FIT p-values lies within 4 standard errors of 1/2; the histogram's midpoints add at most its half-width"""
    c, T = synthetic()
    p, half = c.p_value("fit")
    se = math.sqrt(1.0 / 12.0 / 4000)
    print("mean FIT p-value %.5f, standard error %.5f" % (p, se))
    assert half == 1.0 / 512 and abs(p - 0.5) <= 4 * se
    for stat in ("extreme", ck.SERIAL):
        q, _ = c.p_value(stat)
        assert abs(q - 0.5) <= 4 * se + (0.02 if stat == ck.SERIAL else 0), (stat, q)        # (SERIAL's law is approximate)
    lo, _ = c.p_value("fit", "lower")
    two, w = c.p_value("fit", "two")
    assert lo == 1.0 - p and two == 2 * min(p, lo) and w == 2 * half
    assert int(c.p_hist("fit").sum()) == 4000 and c.n_nan("fit") == 0 and c.p_hist(0).shape == (256,)
    assert c.stat_mean()[0] == pytest.approx(T[:, 0].mean(), rel=1e-12) and c.stat_sd()[0] == pytest.approx(T[:, 0].std(ddof=1), rel=1e-9)
    assert c.stat_mean()[0] == pytest.approx(50.0, abs=4 * math.sqrt(50.0 / 4000))
    assert np.abs(c.pit() - 0.5).max() < 5 * math.sqrt(1 / 12 / 4000) and c.outliers(0.01).size == 0
    assert c.resid_mean() == pytest.approx(1.0, abs=0.1) and c.resid_sd() == pytest.approx(1.0, abs=0.15)
    with pytest.raises(ValueError):
        c.p_value("fit", "both")
    with pytest.raises(ValueError):
        c.p_value("chi2")
    # a model that misses: every T far in the upper tail
    c.counts[0, 0] = 0
    c.counts[0, 0, 255] = 4000
    assert c.p_value("fit")[0] == pytest.approx(1.0 / 512) and c.p_value("fit", "two")[0] == pytest.approx(1.0 / 256)
    # no histogram, no p-value
    bare = ck.Check.empty([0], np.zeros(3), np.zeros(3), np.zeros((3, 0)), PULSE)
    assert math.isnan(bare.p_value("fit")[0]) and bare.counts.shape == (1, 3, 2)


# ---- 5. check.bin ---------------------------------------------------------------------------------------------------------------
def test_write_read_round_trip(tmp_path):
    c, _ = synthetic(n=40, L=5, nbins=8)
    c.thin = 3
    c.counts[0, 2, 8] = 2                                     # the NaN slot
    path = str(tmp_path / "check.bin")
    c.write(path)
    back = ck.Check.read(path)
    for f in ck.STATE + ck.STAT_STATE + ("n", "chains", "x", "y", "edges", "counts"):
        assert getattr(back, f).tobytes() == getattr(c, f).tobytes() and getattr(back, f).dtype == getattr(c, f).dtype, f
    assert (back.model, back.sigma, back.thin, back.n_ladders, back.nbins) == (PULSE, 0.5, 3, 1, 8) and back.n_nan(2) == 2
    assert back.text() == c.text() and back.stats_text() == c.stats_text()
    assert len(c.text().splitlines()) == 5 and len(c.text().splitlines()[0].split("\t")) == 6
    rows = [line.split("\t") for line in c.stats_text().splitlines()]
    assert [r[0] for r in rows] == ["fit", "extreme", "serial"] and all(len(r) == 8 for r in rows)
    raw = open(path, "rb").read()
    assert raw[:8] == b"APEMOSTK"
    for bad in (raw[:-1], b"APEMOSTW" + raw[8:], raw[:20]):
        open(path, "wb").write(bad)
        with pytest.raises(ValueError):
            ck.Check.read(path)
    # a ragged fold's padding is not data
    c.lengths = np.array([3], dtype=np.int32)
    with pytest.raises(ValueError, match="per_ladder"):
        c.write(path)
    with pytest.raises(ValueError, match="per_ladder"):
        c.text()
    one = c.per_ladder(1)[0]
    assert one.n_data == 3 and one.sum_u.tobytes() == np.ascontiguousarray(c.sum_u[:, :3]).tobytes() and one.lengths is None
    assert one.counts.tobytes() == c.counts.tobytes() and len(one.text().splitlines()) == 3


# ---- 6. refusals that need no device ----------------------------------------------------------------------------------------------
def test_a_null_sampler_is_refused_by_every_entry_point():
    L = capi.lib()
    ch = np.zeros(1, dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    out = np.zeros(8)
    dp = out.ctypes.data_as(capi._dp)
    view = capi.CheckView()
    calls = [lambda: L.apemost_hip_check_begin(None, 1, ch.ctypes.data_as(ip), 0, None),
             lambda: L.apemost_hip_check_accumulate(None, None, 0, 0, 1),
             lambda: L.apemost_hip_check_get(None, C.byref(view)), lambda: L.apemost_hip_check_set(None, C.byref(view)),
             lambda: L.apemost_hip_check_lengths(None, ch.ctypes.data_as(ip)), lambda: L.apemost_hip_check_end(None),
             lambda: L.apemost_hip_check_values(None, 1, dp, 1, dp, dp, dp, dp, dp)]
    for call in calls:
        assert call() == capi.ERR_INVALID and b"sampler is NULL" in L.apemost_hip_last_error()
