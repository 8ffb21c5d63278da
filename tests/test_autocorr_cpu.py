"""The autocorrelation fold without a device (apemost_amd/autocorr.py): the entry points exist, Autocorr.from_rows
equals the restatement of tests/autocorr_ref.py, the mean-removed autocovariance from the state equals a direct
two-pass one, the integrated times of AR(1) series land where their theory says, autocorr.bin round-trips, and the C
host's writer, built alone under the sanitizers, prints what Autocorr.text() prints."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi
from apemost_amd.autocorr import Autocorr, default_cols
from tests.autocorr_ref import RefAutocorr, assert_equals, same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["apemost_hip_autocorr_begin", "apemost_hip_autocorr_accumulate", "apemost_hip_autocorr_get",
           "apemost_hip_autocorr_set", "apemost_hip_autocorr_end"]


def test_header_declares_and_library_exports_the_entry_points():
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTS and getattr(L, name).argtypes, name
    assert "apemost_hip_autocorr_config;" in header and "apemost_hip_autocorr_view;" in header
    assert re.search(r"#define APEMOST_HIP_ABI_VERSION 3\b", header)
    assert capi.ABI_VERSION == 3 and L.apemost_hip_abi_version() == 3
    csrc = os.path.join(ROOT, "apemost_amd", "csrc")
    assert '#include "pt_autocorr.h"' in open(os.path.join(csrc, "apemost_hip.hip")).read()
    for f in ("pt_device.h", "pt_onebarrier.h", "pt_kernels.h", "apemost_model.hip"):    # the round kernels do not see it
        assert "autocorr" not in open(os.path.join(csrc, f)).read(), f
    from apemost_amd.sampler import HipSampler
    for m in ("autocorr_begin", "autocorr_accumulate", "autocorr", "autocorr_set", "autocorr_end"):
        assert callable(getattr(HipSampler, m)), m


def _rows(seed, n, n_chains=3, n_par=2):
    """rows [n][n_chains][n_par+2]: correlated columns away from zero, so that the origin matters"""
    rng = np.random.default_rng(seed)
    rows = np.cumsum(rng.standard_normal((n, n_chains, n_par + 2)), axis=0) * 0.1 + rng.standard_normal((n, n_chains, n_par + 2))
    return rows + np.array([100.0, -3.0, 0.5, -1000.0, 7.0, 2e4])[:n_par + 2]


L_CPU = 9


@pytest.mark.parametrize("thin", [1, 3])
@pytest.mark.parametrize("n", [0, 1, 2, L_CPU - 2, L_CPU - 1, L_CPU, L_CPU + 1, 40 * L_CPU])
def test_from_rows_equals_the_restatement(n, thin):
    """n < L, n = L - 1, n = L, n >> L, with the kept steps of thin 1 and 3"""
    rows = _rows(n + thin, n * thin)[::thin]
    assert len(rows) == n
    ac = Autocorr.from_rows(rows, (0, 2), L_CPU, thin=thin)
    assert ac.cols.tolist() == [0, 1, 3] == default_cols(2) and ac.thin == thin and ac.lag.shape == (2, 3, L_CPU)
    assert_equals(ac, RefAutocorr(rows, (0, 2), L_CPU, [0, 1, 3]), "from_rows %d/%d" % (n, thin))
    some = Autocorr.from_rows(rows, (1,), L_CPU, cols=(2,), thin=thin)
    assert_equals(some, RefAutocorr(rows, (1,), L_CPU, [2]), "one column %d" % n)
    if n > L_CPU:
        assert ac.lag[0, 0, L_CPU - 1] != 0 and ac.tail[0, 0].tobytes() == (rows[-(L_CPU - 1):, 0, 0] - rows[0, 0, 0]).tobytes()


def test_from_rows_with_one_lag_and_per_ladder():
    rows = _rows(5, 30, n_chains=4)
    ac = Autocorr.from_rows(rows, (0, 2), 1)
    assert ac.head.shape == ac.tail.shape == (2, 3, 0)
    assert_equals(ac, RefAutocorr(rows, (0, 2), 1, [0, 1, 3]))
    ac = Autocorr.from_rows(rows, (0, 2), 5)
    ac.n_ladders = 2
    lads = ac.per_ladder()
    assert len(lads) == 2 and lads[1].chains.tolist() == [2] and lads[1].lag.tobytes() == ac.lag[1:].tobytes()
    assert_equals(lads[1], Autocorr.from_rows(rows, (2,), 5))
    with pytest.raises(ValueError):
        ac.per_ladder(3)


def test_a_non_finite_value_stays_in_its_series():
    rows = _rows(6, 50)
    clean = Autocorr.from_rows(rows, (0, 1), 7)
    rows[20, 1, 1] = np.inf
    rows[31, 0, 3] = np.nan
    ac = Autocorr.from_rows(rows, (0, 1), 7)
    assert_equals(ac, RefAutocorr(rows, (0, 1), 7, [0, 1, 3]))
    assert not np.isfinite(ac.lag[1, 1]).any() and np.isnan(ac.lag[0, 2]).all() and not np.isfinite(ac.sum[1, 1])
    for k, c in ((0, 0), (0, 1), (1, 0), (1, 2)):
        assert ac.lag[k, c].tobytes() == clean.lag[k, c].tobytes() and ac.sum[k, c] == clean.sum[k, c]


def direct_acov(x, L):
    """two passes: the mean first, then the products of the residuals, in extended precision where numpy has it"""
    x = np.asarray(x, dtype=np.longdouble)
    r = x - x.mean()
    return np.array([float(np.sum(r[l:] * r[:len(x) - l]) / len(x)) for l in range(L)])


def test_acov_from_the_state_equals_a_two_pass_autocovariance():
    """20 000 samples of an AR(1) series around 1000 whose first sample -- the origin -- lies inside the sample: the
    rounding bound n 2^-53 (1 + m^2 / acov_0) with |m| <= 3 sigma is about 2e-11 acov_0; the tolerance is 1e-10
    acov_0."""
    rng = np.random.default_rng(11)
    n, L = 20000, 200
    e = rng.standard_normal(n)
    x = np.zeros(n)
    for t in range(1, n):
        x[t] = 0.8 * x[t - 1] + e[t]
    x += 1000.0
    rows = np.zeros((n, 1, 3))
    rows[:, 0, 0] = x
    ac = Autocorr.from_rows(rows, (0,), L, cols=(0,))
    assert x.min() < ac.origin[0, 0] < x.max()
    m = ac.sum[0, 0] / n
    got, want = ac.acov(0)[0], direct_acov(x, L)
    assert abs(m) <= 3 * math.sqrt(want[0]), (m, want[0])
    worst = float(np.max(np.abs(got - want))) / want[0]
    print("acov: worst difference %.3g acov_0" % worst)
    assert worst <= 1e-10
    assert ac.acf(0)[0, 0] == 1.0 and abs(ac.acf(0)[0, 1] - 0.8) < 0.02
    assert ac.mean(0)[0] == pytest.approx(x.mean(), rel=1e-14)


def ar1(phi, n, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal(n + 1000)
    x = np.zeros(n + 1000)
    for t in range(1, len(x)):
        x[t] = phi * x[t - 1] + e[t]
    rows = np.zeros((n, 1, 3))
    rows[:, 0, 0] = x[1000:]                                  # past the start-up
    return rows


AR1 = {}


def ar1_autocorr(phi, n, L, seed):
    key = (phi, n, L, seed)
    if key not in AR1:
        AR1[key] = Autocorr.from_rows(ar1(phi, n, seed), (0,), L, cols=(0,))
    return AR1[key]


@pytest.mark.parametrize("phi,n,L,seed", [(0.9, 200000, 512, 1), (0.5, 50000, 64, 2), (0.0, 50000, 64, 3)])
def test_sokal_tau_of_ar1(phi, n, L, seed):
    """tau = (1 + phi) / (1 - phi) within 4 standard errors tau sqrt(2 (2 M + 1) / n) (Sokal 1989)"""
    ac = ar1_autocorr(phi, n, L, seed)
    tau, window = ac.tau(0)
    tau, M = float(tau[0]), int(window[0])
    truth = (1 + phi) / (1 - phi)
    se = tau * math.sqrt(2.0 * (2 * M + 1) / n)
    print("phi %.1f: tau %.4f (truth %.4f), window %d, %.2f standard errors" % (phi, tau, truth, M, (tau - truth) / se))
    assert M >= 5 * tau and M > 0 and bool(ac.converged(0)[0])
    assert abs(tau - truth) <= 4 * se, (tau, truth, se)
    assert ac.ess(0)[0] == n / tau
    assert ac.mcse(0)[0] == math.sqrt(ac.variance(0)[0] * tau / n)


def test_a_window_that_does_not_close():
    ac = ar1_autocorr(0.999, 50000, 16, 4)
    tau, window = ac.tau(0)
    assert int(window[0]) == -1 and not ac.converged(0)[0]
    assert tau[0] == 1.0 + 2.0 * float(np.cumsum(ac.acf(0)[0, 1:])[-1]) and 25 < tau[0] < 31    # all 15 lags: a lower bound
    tg, wg = ac.tau(0, method="geyer")
    assert int(wg[0]) == -1 and not ac.converged(0, "geyer")[0] and tg[0] > 25
    with pytest.raises(ValueError):
        ac.tau(0, method="fft")


def test_geyer_tau_agrees_with_sokal():
    phi, n = 0.5, 50000
    ac = ar1_autocorr(phi, n, 64, 2)
    (ts, ws), (tg, wg) = ac.tau(0), ac.tau(0, method="geyer")
    se = float(ts[0]) * math.sqrt(2.0 * (2 * int(ws[0]) + 1) / n)
    print("geyer %.4f (window %d) against sokal %.4f" % (tg[0], wg[0], ts[0]))
    assert wg[0] >= 0 and abs(tg[0] - 3.0) <= 4 * se and abs(tg[0] - ts[0]) <= 4 * se


def _state(seed=9, n=300, L=12, thin=4):
    rows = _rows(seed, n, n_chains=2, n_par=3)
    return Autocorr.from_rows(rows, (0,), L, thin=thin)


def test_files_round_trip(tmp_path):
    ac = Autocorr.from_rows(_rows(3, 90), (0, 2), 12, thin=5)
    path = str(tmp_path / "autocorr.bin")
    ac.write(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"APEMOSTA" and len(raw) == 48 + 4 * (2 + 3) + 8 * 6 * (2 + 12 + 22)
    back = Autocorr.read(path)
    back.write(str(tmp_path / "again.bin"))
    assert open(str(tmp_path / "again.bin"), "rb").read() == raw
    for f in ("n", "origin", "sum", "lag", "head", "tail", "chains", "cols"):
        assert getattr(back, f).tobytes() == getattr(ac, f).tobytes() and getattr(back, f).shape == getattr(ac, f).shape, f
    assert (back.max_lag, back.n_par, back.thin, back.n_ladders) == (12, 2, 5, 1)
    (tmp_path / "bad.bin").write_bytes(b"APEMOSTJ" + raw[8:])
    with pytest.raises(ValueError):
        Autocorr.read(str(tmp_path / "bad.bin"))
    (tmp_path / "short.bin").write_bytes(raw[:-8])
    with pytest.raises(ValueError):
        Autocorr.read(str(tmp_path / "short.bin"))


def test_text_is_stable():
    ac = _state()
    text = ac.text(["a", "b", "c"])
    assert text == ac.text(["a", "b", "c"]) == Autocorr.from_rows(_rows(9, 300, 2, 3), (0,), 12, thin=4).text(["a", "b", "c"])
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) == 5 and [ln.split("\t")[0] for ln in lines[:4]] == ["a", "b", "c", "prob-prior"]
    f = lines[0].split("\t")
    assert len(f) == 8 and re.fullmatch(r"-?\d\.\d{15}e[+-]\d\d", f[1]) and re.fullmatch(r"-?\d+", f[4])
    tau, window = ac.tau(0)
    assert float(f[3]) == float("%.15e" % tau[0]) and int(f[4]) == window[0]
    assert float(f[1]) == float("%.15e" % ac.mean(0)[0]) and float(f[2]) == float("%.15e" % ac.variance(0)[0])
    assert float(f[5]) == float("%.15e" % ac.ess(0)[0]) and float(f[6]) == float("%.15e" % ac.mcse(0)[0])
    assert float(f[7]) == float("%.15e" % ac.tau(0, "geyer")[0][0])
    assert ac.text().startswith("p0\t")


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """the C host's writer with its own main, under the address and undefined-behaviour sanitizers"""
    host = os.path.join(ROOT, "apemost_amd", "host")
    exe = str(tmp_path_factory.mktemp("autocorr_check") / "autocorr_check")
    subprocess.check_call(["gcc", "-std=c99", "-ansi", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(host, "include"),
                           os.path.join(ROOT, "tests", "autocorr_check.c"), os.path.join(host, "src", "run_autocorr.c"),
                           "-o", exe, "-lm"])
    return exe


def _with_nan():
    ac = _state(seed=10)
    ac.lag[0, 1, 3] = np.nan
    return ac


def _constant():
    rows = np.zeros((40, 1, 5))
    rows[:, 0, 1] = np.arange(40.0)
    return Autocorr.from_rows(rows, (0,), 6)


@pytest.mark.parametrize("make", [_state, lambda: _state(n=5, L=12), lambda: _state(n=0), lambda: _state(L=1),
                                  lambda: ar1_autocorr(0.999, 50000, 16, 4), lambda: ar1_autocorr(0.5, 50000, 64, 2),
                                  _with_nan, _constant],
                         ids=["plain", "fewer_samples_than_lags", "empty", "one_lag", "open_window", "ar1", "nan", "constant"])
def test_c_host_writer_stands_alone(checker, tmp_path, make):
    ac = make()
    names = ["alpha", "beta", "gamma"][:ac.n_par]
    ac.write(str(tmp_path / "autocorr.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([checker, str(tmp_path / "autocorr.bin"), str(tmp_path / "autocorr.txt"),
                           str(tmp_path / "again.bin")] + names, env=env)
    assert (tmp_path / "autocorr.txt").read_text() == ac.text(names)
    assert (tmp_path / "again.bin").read_bytes() == (tmp_path / "autocorr.bin").read_bytes()
