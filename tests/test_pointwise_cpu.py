"""The pointwise log-likelihood without a device (apemost_amd/pointwise.py): the entry points exist, the model
translation units do not mention the feature, hand cases with known answers, compare and its refusal, DIC from at_mean,
pointwise.bin round-trips, the text is stable, loglike_numpy agrees with the rational restatement of
tests/pointwise_ref.py, and the C host's writer, built alone under the sanitizers, prints what Pointwise prints."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi
from apemost_amd import workloads as wl
from apemost_amd.pointwise import CRITERIA, STATE, Pointwise, loglike_numpy, sine_constant
from tests import pointwise_ref as ref
from tests.pointwise_ref import RefPointwise
from tests.test_predict_cpu import sine_bound

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["apemost_hip_pointwise_begin", "apemost_hip_pointwise_accumulate", "apemost_hip_pointwise_get",
           "apemost_hip_pointwise_set", "apemost_hip_pointwise_end", "apemost_hip_pointwise_loglike"]
U = 2.0 ** -53


def test_header_declares_and_library_exports_the_entry_points():
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTS and getattr(L, name).argtypes, name
    assert "apemost_hip_pointwise_config;" in header and "apemost_hip_pointwise_view;" in header
    assert re.search(r"#define APEMOST_HIP_ABI_VERSION 3\b", header)
    assert capi.ABI_VERSION == 3 and L.apemost_hip_abi_version() == 3
    from apemost_amd.sampler import HipSampler
    for m in ("pointwise_begin", "pointwise_accumulate", "pointwise", "pointwise_set", "pointwise_end",
              "pointwise_loglike"):
        assert callable(getattr(HipSampler, m)), m


def test_the_model_translation_units_do_not_mention_it():
    csrc = os.path.join(ROOT, "apemost_amd", "csrc")
    assert '#include "pt_pointwise.h"' in open(os.path.join(csrc, "apemost_hip.hip")).read()
    for f in ("pt_device.h", "pt_onebarrier.h", "pt_kernels.h", "apemost_model.hip"):
        assert "pointwise" not in open(os.path.join(csrc, f)).read().lower(), f


# ---- Pointwise's arithmetic -------------------------------------------------------------------------------------------
def from_values(values, model=wl.MODEL_SIMPLESIN, n_par=4, thin=1, params=None, seed=0):
    """a Pointwise of one kept chain from the terms values [n][n_data], folded by the restatement's sequential loops"""
    values = np.asarray(values, dtype=np.float64)
    n, D = values.shape
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 1, n_par + 2))
    rows[:, 0, :n_par] = rng.uniform(0.1, 1.0, (n, n_par)) if params is None else params
    data = np.stack([100 + 0.5 * np.arange(D), rng.uniform(-1, 2, D)], 1)
    r = RefPointwise(model, rows, [0], data, 0.5, values=values.reshape(n, 1, D))
    pw = Pointwise([n], *[getattr(r, f) for f in STATE], r.par_origin, r.par_sum, [0], data[:, 0], data[:, 1], n_par,
                   model, 0.5, thin)
    return pw, rows


def test_all_samples_identical():
    """every sample the same: S_up = S_dn = S2_dn = n exactly (exp(0) = 1), so ln(S / n) = 0 and lppd = elpd_loo = l
    bit for bit, both p_waic are 0 and the weights' effective sample size is n"""
    L = np.array([-1.25, -0.5, -33.0])
    pw, _ = from_values(np.tile(L, (7, 1)))
    assert pw.lppd().tolist() == L.tolist() == pw.elpd_loo().tolist() == pw.mean_loglike().tolist()
    assert pw.p_waic(1).tolist() == [0.0] * 3 == pw.p_waic(2).tolist() == pw.var_loglike().tolist()
    assert pw.loo_ess().tolist() == [7.0] * 3 and len(pw.loo_unreliable(7.0)) == 0
    assert pw.loo_unreliable(7.5).tolist() == [0, 1, 2]
    c = pw.criteria()
    assert c["lppd"] == c["elpd_loo"] == c["elpd_waic"] == float(np.cumsum(L)[-1]) and c["p_loo"] == 0.0
    assert c["waic"] == c["looic"] == -2 * c["lppd"] and c["n"] == 7.0
    with pytest.raises(ValueError):
        pw.p_waic(3)


def test_two_samples_two_data_by_hand():
    """datum 0 has the likelihoods 1/2 and 1/4 under the two samples, datum 1 has e^-1 under both.
    datum 0: the mean likelihood is 3/8, so lppd = ln(3/8); the harmonic mean is 1 / ((2 + 4) / 2) = 1/3, so elpd_loo =
    -ln 3; the mean of l is -(3/2) ln 2, its sample variance (ln 2)^2 / 2 (two values ln 2 apart); the leave-one-out
    weights are proportional to 2 and 4: (2 + 4)^2 / (4 + 16) = 1.8.
    datum 1: lppd = elpd_loo = mean = -1, variance 0, effective sample size 2.
    So lppd = ln(3/8) - 1, p_waic2 = (ln 2)^2 / 2, p_waic1 = 2 (ln(3/8) + (3/2) ln 2) = 2 ln(3 / 2^1.5), elpd_waic =
    lppd - p_waic2, elpd_loo = -ln 3 - 1 and p_loo = ln(3/8) + ln 3 = ln(9/8).  Each figure is a handful of roundings
    of numbers of order 1 away from these: 1e-14."""
    ln2, ln3 = math.log(2.0), math.log(3.0)
    pw, _ = from_values([[math.log(0.5), -1.0], [math.log(0.25), -1.0]])
    tol = dict(rel=0, abs=1e-14)
    assert pw.lppd().tolist() == pytest.approx([math.log(0.375), -1.0], **tol)
    assert pw.elpd_loo().tolist() == pytest.approx([-ln3, -1.0], **tol)
    assert pw.mean_loglike().tolist() == pytest.approx([-1.5 * ln2, -1.0], **tol)
    assert pw.var_loglike().tolist() == pytest.approx([ln2 * ln2 / 2, 0.0], **tol)
    assert pw.loo_ess().tolist() == pytest.approx([1.8, 2.0], **tol)
    c = pw.criteria()
    assert c["lppd"] == pytest.approx(math.log(0.375) - 1, **tol)
    assert c["p_waic2"] == pytest.approx(ln2 * ln2 / 2, **tol)
    assert c["p_waic1"] == pytest.approx(2 * math.log(3 / 2 ** 1.5), **tol)
    assert c["elpd_waic"] == pytest.approx(math.log(0.375) - 1 - ln2 * ln2 / 2, **tol)
    assert c["waic"] == -2 * c["elpd_waic"] and c["looic"] == -2 * c["elpd_loo"]
    assert c["elpd_loo"] == pytest.approx(-ln3 - 1, **tol) and c["p_loo"] == pytest.approx(math.log(9 / 8), **tol)
    # the standard error: the two pointwise elpd_waic e0, e1 have the variance (e0 - e1)^2 / 2 about their mean
    e = pw.elpd_waic()
    assert c["waic_se"] == pytest.approx(math.sqrt(2 * (e[0] - e[1]) ** 2 / 2), **tol)


def test_one_sample_dominates_the_weights():
    """l = 0 then -800: the weight exp(800) of the second sample makes the first's exp(-800) = 0 in fp64: S_dn = S2_dn
    = 1, an effective sample size of exactly 1, and elpd_loo = -(800 + ln(1/2))"""
    pw, _ = from_values([[0.0, -1.0], [-800.0, -1.0]])
    assert pw.loo_ess().tolist() == [1.0, 2.0] and pw.loo_unreliable(1.5).tolist() == [0]
    assert pw.elpd_loo()[0] == -(800.0 + math.log(0.5)) and pw.lppd()[0] == 0.0 + math.log(0.5)


def test_compare_and_its_refusal():
    rng = np.random.default_rng(3)
    a, _ = from_values(-1 + 0.1 * rng.standard_normal((30, 5)))
    b, _ = from_values(-1.5 + 0.1 * rng.standard_normal((30, 5)))
    for kind, fa, fb in (("loo", a.elpd_loo(), b.elpd_loo()), ("waic", a.elpd_waic(), b.elpd_waic())):
        diff, se = a.compare(b, kind)
        d = fa - fb
        assert diff == pytest.approx(float(d.sum()), rel=1e-13) and diff > 0
        assert se == pytest.approx(math.sqrt(5 * d.var(ddof=1)), rel=1e-12)
        back, se_back = b.compare(a, kind)
        assert back == -diff and se_back == se
    assert a.compare(a)[0] == 0.0 and a.compare(a)[1] == 0.0
    other, _ = from_values(-1 + 0.1 * rng.standard_normal((30, 5)), seed=9)      # other data
    with pytest.raises(ValueError):
        a.compare(other)
    with pytest.raises(ValueError):
        a.compare(b, "psis")


def test_dic_from_at_mean():
    """par_mean is origin + sum / n of the stored samples; p_D = 2 (sum l(mean parameters) - sum mean l) and
    DIC = -2 sum l(mean parameters) + 2 p_D"""
    rng = np.random.default_rng(4)
    values = -2 + 0.3 * rng.standard_normal((40, 6))
    pw, rows = from_values(values)
    assert np.allclose(pw.par_mean(), rows[:, 0, :4].mean(axis=0), rtol=1e-14, atol=0)
    assert pw.par_mean_all().shape == (1, 4)
    assert np.isnan(pw.at_mean).all() and np.isnan(pw.dic())              # nobody filled it yet
    pw.at_mean[0] = values.mean(axis=0) + 0.125
    assert pw.p_dic() == pytest.approx(2 * 6 * 0.125, rel=1e-12)
    assert pw.dic() == pytest.approx(-2 * float(pw.at_mean.sum()) + 2 * pw.p_dic(), rel=1e-14)
    assert pw.criteria()["dic"] == pw.dic() and pw.criteria()["p_dic"] == pw.p_dic()


def _state(n=50, n_data=7, model=wl.MODEL_SIMPLESIN, seed=4, at_mean=True):
    rng = np.random.default_rng(seed)
    n_par = {wl.MODEL_SIMPLESIN: 4, wl.MODEL_PULSE: 6}[model]
    values = -1.5 + 0.4 * rng.standard_normal((n, n_data))
    pw, _ = from_values(values, model, n_par, thin=3, seed=seed)
    if at_mean and n:
        pw.at_mean[0] = values.mean(axis=0) + 0.01
    return pw


def test_files_round_trip(tmp_path):
    pw = _state()
    path = str(tmp_path / "pointwise.bin")
    pw.write(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"APEMOSTW" and len(raw) == 64 + 4 + 8 * (11 * 7 + 2 * 4)
    back = Pointwise.read(path)
    back.write(str(tmp_path / "again.bin"))
    assert open(str(tmp_path / "again.bin"), "rb").read() == raw
    for f in ("n", "x", "y", "chains", "par_origin", "par_sum", "at_mean") + STATE:
        assert getattr(back, f).tobytes() == getattr(pw, f).tobytes() and getattr(back, f).shape == getattr(pw, f).shape, f
    assert (back.n_par, back.thin, back.n_ladders, back.model, back.sigma, back.n_data) == (4, 3, 1, 0, 0.5, 7)
    (tmp_path / "bad.bin").write_bytes(b"APEMOSTP" + raw[8:])               # the posterior predictive's magic
    with pytest.raises(ValueError):
        Pointwise.read(str(tmp_path / "bad.bin"))
    (tmp_path / "short.bin").write_bytes(raw[:-8])
    with pytest.raises(ValueError):
        Pointwise.read(str(tmp_path / "short.bin"))
    from apemost_amd.predict import Predict
    with pytest.raises(ValueError):
        Predict.read(path)                                                # and the other way round


def test_per_ladder():
    a, b = _state(seed=1), _state(seed=2)
    cat = [np.concatenate([getattr(a, f), getattr(b, f)]) for f in STATE]
    both = Pointwise(a.n, *cat, np.concatenate([a.par_origin, b.par_origin]), np.concatenate([a.par_sum, b.par_sum]),
                     [0, 8], np.concatenate([a.x, b.x]), np.concatenate([a.y, b.y]), 4, 0, 0.5, 3, 2,
                     np.concatenate([a.at_mean, b.at_mean]))
    lads = both.per_ladder()
    assert len(lads) == 2 and lads[1].chains.tolist() == [8] and lads[1].n_ladders == 1
    for f in STATE + ("par_origin", "par_sum", "at_mean", "x", "y"):
        assert getattr(lads[1], f).tobytes() == getattr(b, f).tobytes(), f
    assert lads[1].criteria_text() == b.criteria_text() == both.criteria_text(k=1)
    with pytest.raises(ValueError):
        both.per_ladder(3)


def test_text_is_stable():
    pw = _state()
    text = pw.text()
    assert text == pw.text() == _state().text()
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) == 8
    f = lines[2].split("\t")
    assert len(f) == 8 and all(re.fullmatch(r"-?\d\.\d{15}e[+-]\d\d", v) for v in f)
    want = [pw.x[0][2], pw.y[0][2], pw.mean_loglike()[2], math.sqrt(pw.var_loglike()[2]), pw.lppd()[2], pw.p_waic(2)[2],
            pw.elpd_loo()[2], pw.loo_ess()[2]]
    assert [float(v) for v in f] == [float("%.15e" % v) for v in want]
    crit = pw.criteria_text()
    assert crit == _state().criteria_text()
    rows = [ln.split("\t") for ln in crit.split("\n")[:-1]]
    assert [r[0] for r in rows] == list(CRITERIA) and rows[0][1] == "%.15e" % 50.0
    assert [float(r[1]) for r in rows] == [float("%.15e" % pw.criteria()[name]) for name in CRITERIA]
    assert 1.0 <= pw.loo_ess().min() and pw.loo_ess().max() <= 50.0


# ---- loglike_numpy against the restatement ------------------------------------------------------------------------------
def test_loglike_numpy_agrees_with_the_restatement():
    """Sine models: the two curves differ by at most e_v = sine_bound (tests/test_predict_cpu.py).  Carried through
    r = v - y, q = r * r, l = q * c, each rounded once per side (u = 2^-53):
        |dr| <= e_v + 2 u |r|;   |dq| <= 2 |r| |dr| + dr^2 + 2 u q;   |dl| <= |c| |dq| + 2 u |l|.
    Pulse models: the curves are equal bit for bit (plain IEEE operations) and so is w = y / v; both logarithms are within
    one ulp of ln v, so L differs by at most 2 * 2^-52 |ln v|, L + w by that and one rounding per side, and the negation
    is exact:  |dl| <= 2^-51 |ln v| + 2 u |l|."""
    rng = np.random.default_rng(5)
    x = np.concatenate([100 + 0.5 * np.arange(40), [2.45e6 + 0.37, -77.7, 0.0, 1e13]])
    sigma = 0.37
    c = float(sine_constant(sigma))
    assert c == ref.sine_constant(sigma) == 1.0 / ((-2.0 * sigma) * sigma)
    for model, n_par, n_adds in ((wl.MODEL_SIMPLESIN, 4, 1), (wl.MODEL_SINE3, 10, 4)):
        data = np.stack([x, rng.uniform(-1, 2, len(x))], 1)
        hi = np.array([2, 0.3, 1, 2] if n_par == 4 else [2, 0.3, 1] * 3 + [2], dtype=float)
        rows = hi * rng.uniform(size=(6, n_par))
        rows[5, 1] = 1e3                                      # 2 pi f x = 6e16 at x = 1e13: past the guard
        got, want = loglike_numpy(model, rows, data, sigma), ref.terms(model, rows, data, sigma)
        assert np.isnan(want[5, -1]) and np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == 1
        worst = 0.0
        for r in range(6):
            amps = rows[r, 0:1] if n_par == 4 else rows[r, 0:9:3]
            e_v = sine_bound(amps, rows[r, -1], n_adds)
            with np.errstate(all="ignore"):
                res = np.abs(np.sqrt(want[r] / c))            # |r| of the restatement
                dr = e_v + 2 * U * res
                dq = 2 * res * dr + dr * dr + 2 * U * res * res
                bound = abs(c) * dq + 2 * U * np.abs(want[r])
                frac = np.nanmax(np.abs(got[r] - want[r]) / bound)
            worst = max(worst, frac)
            assert frac <= 1, (model, r, frac)
        print("model %d: worst difference %.3g of its bound" % (model, worst))
    nu = np.linspace(10, 12, 41)
    for model, base in ((wl.MODEL_PULSE, [5.0, 0.05, 10.6, 4.0, 11.3, 2.5]),
                        (wl.MODEL_PULSE_VROT, [5.0, 0.05, 0.05, 10.6, 4.0, 11.3, 2.5])):
        data = np.stack([nu, rng.exponential(1.0, 41)], 1)
        rows = np.array(base) * (1 + 0.1 * rng.uniform(size=(5, len(base))))
        got, want = loglike_numpy(model, rows, data, sigma, hmin=1e-6), ref.terms(model, rows, data, sigma)
        v = np.array([[ref.curve(model, p, xi) for xi in nu] for p in rows])
        bound = 2.0 ** -51 * np.abs(np.log(v)) + 2 * U * np.abs(want)
        frac = float(np.max(np.abs(got - want) / bound))
        print("model %d: worst difference %.3g of its bound" % (model, frac))
        assert np.isfinite(want).all() and frac <= 1, (model, frac)
    assert loglike_numpy(wl.MODEL_PULSE, rows[0, :6], data).shape == (41,)
    with pytest.raises(ValueError):
        loglike_numpy(wl.MODEL_USER, rows, data)


# ---- the C host's writer ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """the C host's writer with its own main, under the address and undefined-behaviour sanitizers"""
    host = os.path.join(ROOT, "apemost_amd", "host")
    exe = str(tmp_path_factory.mktemp("pointwise_check") / "pointwise_check")
    subprocess.check_call(["gcc", "-std=c99", "-ansi", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(host, "include"),
                           os.path.join(ROOT, "tests", "pointwise_check.c"), os.path.join(host, "src", "run_pointwise.c"),
                           "-o", exe, "-lm"])
    return exe


def _with_nan():
    pw = _state(seed=10)
    pw.sum[0, 1] = np.nan
    pw.S_dn[0, 2] = np.inf
    pw.S_up[0, 3] = -1.0                                      # a logarithm of a negative number
    pw.S2_dn[0, 4] = 0.0
    return pw


@pytest.mark.parametrize("make", [_state, lambda: _state(at_mean=False), lambda: _state(n=0), lambda: _state(n=1),
                                  lambda: _state(n_data=1), lambda: _state(model=wl.MODEL_PULSE), _with_nan],
                         ids=["plain", "no_at_mean", "empty", "one_sample", "one_datum", "pulse", "nan"])
def test_c_host_writer_stands_alone(checker, tmp_path, make):
    pw = make()
    pw.write(str(tmp_path / "pointwise.bin"))
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([checker, str(tmp_path / "pointwise.bin"), str(tmp_path / "pointwise.txt"),
                           str(tmp_path / "criteria.txt"), str(tmp_path / "again.bin")], env=env)
    assert (tmp_path / "pointwise.txt").read_text() == pw.text()
    assert (tmp_path / "criteria.txt").read_text() == pw.criteria_text()
    assert (tmp_path / "again.bin").read_bytes() == (tmp_path / "pointwise.bin").read_bytes()
