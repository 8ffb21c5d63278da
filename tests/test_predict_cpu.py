"""The posterior predictive without a device (apemost_amd/predict.py): the entry points exist, Predict's mean and variance
from origin, sum and sq equal a two-pass variance, quantiles come from the counts, residuals follow the model,
predict.bin round-trips, the text is stable, curve_numpy agrees with the rational restatement of tests/predict_ref.py,
and the C host's writer, built alone under the sanitizers, prints what Predict.text() prints."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi
from apemost_amd import workloads as wl
from apemost_amd.predict import Predict, curve_numpy
from tests import predict_ref as ref
from tests.predict_ref import RefPredict, assert_equals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["apemost_hip_predict_begin", "apemost_hip_predict_accumulate", "apemost_hip_predict_get",
           "apemost_hip_predict_set", "apemost_hip_predict_end", "apemost_hip_predict_curve"]


def test_header_declares_and_library_exports_the_entry_points():
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTS and getattr(L, name).argtypes, name
    assert "apemost_hip_predict_config;" in header and "apemost_hip_predict_view;" in header
    assert re.search(r"#define APEMOST_HIP_ABI_VERSION 3\b", header)
    assert capi.ABI_VERSION == 3 and L.apemost_hip_abi_version() == 3
    csrc = os.path.join(ROOT, "apemost_amd", "csrc")
    assert '#include "pt_predict.h"' in open(os.path.join(csrc, "apemost_hip.hip")).read()
    for f in ("pt_device.h", "pt_onebarrier.h", "pt_kernels.h", "apemost_model.hip"):    # the round kernels do not see it
        assert "predict" not in open(os.path.join(csrc, f)).read(), f
    from apemost_amd.sampler import HipSampler
    for m in ("predict_begin", "predict_accumulate", "predict", "predict_set", "predict_end", "predict_curve"):
        assert callable(getattr(HipSampler, m)), m


# ---- Predict's arithmetic ---------------------------------------------------------------------------------------------
def from_values(values, x, model=wl.MODEL_SIMPLESIN, nbins=0, lo=0.0, hi=0.0, n_par=4, thin=1):
    """a Predict of one kept chain from the curve's samples values [n][n_x], by numpy's cumulative sums (which add in
    index order) and the restatement's bisection"""
    values = np.asarray(values, dtype=np.float64)
    n, X = values.shape
    pr = Predict.empty((0,), x, n_par, model, nbins, lo, hi, thin)
    pr.n[0] = n
    if n == 0:
        return pr
    with np.errstate(all="ignore"):
        d = values - values[0]
        pr.origin[0] = values[0]
        pr.sum[0] = np.cumsum(np.concatenate((np.zeros((1, X)), d)), axis=0)[-1]
        pr.sq[0] = np.cumsum(np.concatenate((np.zeros((1, X)), d * d)), axis=0)[-1]
        pr.vmin[0], pr.vmax[0] = np.fmin.reduce(values, axis=0), np.fmax.reduce(values, axis=0)
    if nbins:
        e = ref.edges(lo, hi, nbins)
        for i in range(X):
            for v in values[:, i].tolist():
                b = ref.bin_of(v, e)
                if b >= 0:
                    pr.hist[0, i, b] += np.uint64(1)
    return pr


def test_variance_from_the_state_equals_a_two_pass_variance():
    """20 000 samples around 1000 whose first -- the origin -- lies inside the sample.  With u = 2^-53, d = v - origin
    and m the mean of d: a sequential sum of n terms errs by at most n u sum |d|, so sq errs by n^2 u (var + m^2) and
    sum^2 / n by 2 n^2 u |m| mean|d| <= 2 n^2 u (var + m^2); var = (sq - sum^2 / n) / n then errs by
    3 n u (var + m^2).  With |m| <= 3 sd that is 30 n u var = 6.7e-11 var; the tolerance is 1e-10 var."""
    rng = np.random.default_rng(11)
    n = 20000
    values = 1000.0 + rng.standard_normal((n, 3)) * np.array([1.0, 0.01, 50.0])
    pr = from_values(values, [1.0, 2.0, 3.0])
    ld = values.astype(np.longdouble)
    mean = ld.mean(axis=0)
    want = np.array(((ld - mean) ** 2).mean(axis=0), dtype=np.float64)
    m = pr.sum[0] / n
    assert np.all(np.abs(m) <= 3 * np.sqrt(want)), (m, want)
    worst = float(np.max(np.abs(pr.var(0) - want) / want))
    print("var: worst relative difference %.3g" % worst)
    assert worst <= 1e-10
    assert np.allclose(pr.mean(0), np.array(mean, dtype=np.float64), rtol=1e-14, atol=0)
    assert np.array_equal(pr.sd(0), np.sqrt(pr.var(0)))
    assert pr.vmin[0].tolist() == values.min(axis=0).tolist() and pr.vmax[0].tolist() == values.max(axis=0).tolist()


def test_quantiles_come_from_the_counts():
    """100 values 0.5, 1.5, ..., 99.5 in 100 bins over [0, 100]: one per bin, so the q-quantile is 100 q up to the
    rounding of the edges; a second abscissa with everything in one bin interpolates inside it; a third has nothing"""
    v = np.arange(100.0) + 0.5
    values = np.stack([v, np.full(100, 42.25), np.full(100, np.nan)], axis=1)
    pr = from_values(values, [0.0, 1.0, 2.0], nbins=100, lo=0.0, hi=100.0)
    assert pr.counted(0).tolist() == [100, 100, 0]
    top = pr.quantile(1.0)
    assert top[0] == pr.edges()[100] == 100.0 + 100.0 / 10000 and top[1] == 43.0    # the top edge is the widened one
    for q in (0.0, 0.16, 0.5, 0.84, 0.975):
        got = pr.quantile(q)
        assert got[0] == pytest.approx(100 * q, abs=1e-11) and np.isnan(got[2])
        assert got[1] == pytest.approx(42 + q, abs=1e-11)          # all of bin [42, 43): rank q n of n inside it
    lo68, hi68 = pr.band(0.68)
    assert lo68[0] == pytest.approx(16.0, abs=1e-11) and hi68[0] == pytest.approx(84.0, abs=1e-11)
    assert pr.median()[0] == pytest.approx(50.0, abs=1e-11)
    with pytest.raises(ValueError):
        pr.quantile(1.5)
    with pytest.raises(ValueError):
        from_values(values, [0.0, 1.0, 2.0]).quantile(0.5)         # no histograms


def test_residuals_follow_the_model_and_chi2():
    values = np.array([[2.0, 4.0], [4.0, 4.0]])
    y = np.array([6.0, 2.0])
    sine = from_values(values, [0.0, 1.0], model=wl.MODEL_SINE3, n_par=10)
    pulse = from_values(values, [0.0, 1.0], model=wl.MODEL_PULSE_VROT, n_par=7)
    assert sine.mean(0).tolist() == [3.0, 4.0] and sine.var(0).tolist() == [1.0, 0.0]
    assert sine.default_kind() == "difference" and pulse.default_kind() == "ratio"
    assert sine.residuals(y).tolist() == [3.0, -2.0] == sine.residuals(y, "difference").tolist()
    assert pulse.residuals(y).tolist() == [2.0, 0.5] == sine.residuals(y, "ratio").tolist()
    assert sine.chi2(y, 2.0) == (1.5 ** 2 + 1.0)
    with pytest.raises(ValueError):
        sine.residuals(y, "quotient")


def _state(n=50, nbins=16, model=wl.MODEL_SIMPLESIN, seed=4):
    rng = np.random.default_rng(seed)
    x = np.linspace(100.0, 110.0, 7)
    n_par = {wl.MODEL_SIMPLESIN: 4, wl.MODEL_PULSE: 6}[model]
    par = np.array(wl.SIMPLESIN_PARAMS)[:, 0].astype(float) if model == wl.MODEL_SIMPLESIN else np.array(
        [5.0, 0.05, 104.0, 4.0, 107.0, 2.5])
    rows = par + 0.01 * rng.standard_normal((n, n_par))
    values = curve_numpy(model, rows, x) if n else np.zeros((0, 7))
    pr = from_values(values, x, model, nbins, -0.5, 1.5, n_par, thin=3)
    if n:
        pr.best_prob[0], pr.best_n[0], pr.best_params[0] = -12.5, min(n, 7), rows[min(n, 7) - 1]
    return pr


def test_files_round_trip(tmp_path):
    pr = _state()
    path = str(tmp_path / "predict.bin")
    pr.write(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"APEMOSTP" and len(raw) == 72 + 4 + 8 * (6 * 7 + 7 * 16 + 2 + 4)
    back = Predict.read(path)
    back.write(str(tmp_path / "again.bin"))
    assert open(str(tmp_path / "again.bin"), "rb").read() == raw
    for f in ("n", "x", "origin", "sum", "sq", "vmin", "vmax", "hist", "best_prob", "best_params", "best_n", "chains"):
        assert getattr(back, f).tobytes() == getattr(pr, f).tobytes() and getattr(back, f).shape == getattr(pr, f).shape, f
    assert (back.nbins, back.n_par, back.thin, back.n_ladders, back.model, back.lo, back.hi) == (16, 4, 3, 1, 0, -0.5, 1.5)
    (tmp_path / "bad.bin").write_bytes(b"APEMOSTA" + raw[8:])
    with pytest.raises(ValueError):
        Predict.read(str(tmp_path / "bad.bin"))
    (tmp_path / "short.bin").write_bytes(raw[:-8])
    with pytest.raises(ValueError):
        Predict.read(str(tmp_path / "short.bin"))


def test_per_ladder():
    a, b = _state(seed=1), _state(seed=2)
    both = Predict(a.n, np.concatenate([a.origin, b.origin]), np.concatenate([a.sum, b.sum]), np.concatenate([a.sq, b.sq]),
                   np.concatenate([a.vmin, b.vmin]), np.concatenate([a.vmax, b.vmax]), np.concatenate([a.hist, b.hist]),
                   np.concatenate([a.best_prob, b.best_prob]), np.concatenate([a.best_params, b.best_params]),
                   np.concatenate([a.best_n, b.best_n]), [0, 8], np.concatenate([a.x, b.x]), 4, 0, -0.5, 1.5, 3, 2)
    lads = both.per_ladder()
    assert len(lads) == 2 and lads[1].chains.tolist() == [8] and lads[1].n_ladders == 1
    for f in ref.FIELDS:
        assert getattr(lads[1], f).tobytes() == getattr(b, f).tobytes(), f
    with pytest.raises(ValueError):
        both.per_ladder(3)


def test_text_is_stable():
    pr = _state()
    y = np.linspace(0.0, 1.0, 7)
    text = pr.text(y)
    assert text == pr.text(y) == _state().text(y)
    lines = text.split("\n")
    assert lines[-1] == "" and len(lines) == 8
    f = lines[2].split("\t")
    assert len(f) == 11 and all(re.fullmatch(r"-?\d\.\d{15}e[+-]\d\d", v) for v in f)
    want = [pr.x[0][2], y[2], pr.mean()[2], pr.sd()[2], y[2] - pr.mean()[2], pr.vmin[0][2], pr.vmax[0][2],
            pr.best_curve()[2], pr.median()[2], pr.band(0.68)[0][2], pr.band(0.68)[1][2]]
    assert [float(v) for v in f] == [float("%.15e" % v) for v in want]
    assert len(_state(nbins=0).text(y).split("\n")[0].split("\t")) == 8
    assert np.array_equal(pr.best_curve(), curve_numpy(0, pr.best_params[0], pr.x[0]))


# ---- curve_numpy against the restatement --------------------------------------------------------------------------------
U = 2.0 ** -53


def sine_bound(amplitudes, offset, n_adds):
    """both sides take the sine of the same rounded argument.  The device's sin_cw is within 2.3e-16 of it (documented
    at pt_device.h), numpy's within one ulp of a value below 1 (2^-52); each product a * s rounds once per side
    (2 u |a|), and each of the n_adds additions rounds once per side on a partial sum of at most sum |a| + |o|"""
    A = float(np.sum(np.abs(amplitudes)))
    return A * (2.3e-16 + 2.0 ** -52 + 2 * U) + 2 * n_adds * U * (A + abs(offset))


def test_curve_numpy_agrees_with_the_restatement():
    rng = np.random.default_rng(5)
    x = np.concatenate([100 + 0.5 * np.arange(40), [2.45e6 + 0.37, -77.7, 0.0, 1e13]])
    for model, n_par, n_adds in ((wl.MODEL_SIMPLESIN, 4, 1), (wl.MODEL_SINE3, 10, 4)):
        lo = np.zeros(n_par)
        hi = np.array([2, 0.3, 1, 2] if n_par == 4 else [2, 0.3, 1] * 3 + [2], dtype=float)
        rows = lo + (hi - lo) * rng.uniform(size=(6, n_par))
        rows[5, 1] = 1e3                                      # 2 pi f x = 6e16 at x = 1e13: past the guard
        got, want = curve_numpy(model, rows, x), ref.curves(model, rows, x)
        assert np.isnan(want[5, -1]) and np.isnan(got[5, -1]) and np.array_equal(np.isnan(got), np.isnan(want))
        worst = 0.0
        for r in range(6):
            amps = rows[r, 0:1] if n_par == 4 else rows[r, 0:9:3]
            bound = sine_bound(amps, rows[r, -1], n_adds)
            err = np.nanmax(np.abs(got[r] - want[r]))
            worst = max(worst, err / bound)
            assert err <= bound, (model, r, err, bound)
        print("model %d: worst difference %.3g of its bound" % (model, worst))
    # the pulse curves are plain IEEE operations: bit for bit
    nu = np.linspace(10, 12, 41)
    rows = np.array([5.0, 0.05, 10.6, 4.0, 11.3, 2.5]) * (1 + 0.1 * rng.uniform(size=(5, 6)))
    assert curve_numpy(wl.MODEL_PULSE, rows, nu).tobytes() == ref.curves(wl.MODEL_PULSE, rows, nu).tobytes()
    assert ref.pulse_numpy(rows, nu).tobytes() == ref.curves(wl.MODEL_PULSE, rows, nu).tobytes()
    rows = np.array([5.0, 0.05, 0.05, 10.6, 4.0, 11.3, 2.5]) * (1 + 0.1 * rng.uniform(size=(5, 7)))
    assert curve_numpy(wl.MODEL_PULSE_VROT, rows, nu).tobytes() == ref.curves(wl.MODEL_PULSE_VROT, rows, nu).tobytes()
    assert curve_numpy(wl.MODEL_PULSE, rows[0, :6], nu).shape == (41,)
    with pytest.raises(ValueError):
        curve_numpy(wl.MODEL_USER, rows, nu)


def test_the_restatement_of_the_fold_is_sequential():
    """RefPredict against from_values on rows small enough for both; a tie in prob keeps the first occurrence, a NaN
    prob never wins and best_n is 1-based"""
    rng = np.random.default_rng(8)
    x = np.array([100.0, 100.5, 101.0])
    rows = np.zeros((9, 2, 6))
    rows[:, :, :4] = np.array([0.9, 0.2, 0.4, 0.5]) + 0.05 * rng.standard_normal((9, 2, 4))
    rows[:, 1, 4] = [-5, np.nan, -3, -4, -3, -9, -3, -8, -7]
    rows[:, 0, 4] = np.nan
    got = RefPredict(wl.MODEL_SIMPLESIN, rows, [1], x, 8, 0.0, 1.5)
    want = from_values(ref.curves(wl.MODEL_SIMPLESIN, rows[:, 1, :4], x), x, nbins=8, lo=0.0, hi=1.5)
    want.best_prob[0], want.best_n[0], want.best_params[0] = -3.0, 3, rows[2, 1, :4]
    assert_equals(got, want)
    none = RefPredict(wl.MODEL_SIMPLESIN, rows, [0], x)
    assert none.best_n[0] == 0 and none.best_prob[0] == -np.inf and not none.best_params.any()
    assert 0 < got.hist.sum() <= 27 and got.hist.shape == (1, 3, 8)


# ---- the C host's writer ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    """the C host's writer with its own main, under the address and undefined-behaviour sanitizers"""
    host = os.path.join(ROOT, "apemost_amd", "host")
    exe = str(tmp_path_factory.mktemp("predict_check") / "predict_check")
    subprocess.check_call(["gcc", "-std=c99", "-ansi", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(host, "include"),
                           os.path.join(ROOT, "tests", "predict_check.c"), os.path.join(host, "src", "run_predict.c"),
                           "-o", exe, "-lm"])
    return exe


def _with_nan():
    pr = _state(seed=10)
    pr.sum[0, 1] = np.nan
    pr.vmin[0, 2] = np.inf
    return pr


def _empty_bins():
    pr = _state(seed=11)
    pr.hist[0, 3] = 0                                         # nothing counted at one abscissa
    pr.hist[0, 4, :8] = 0                                     # empty leading bins
    return pr


@pytest.mark.parametrize("make", [_state, lambda: _state(nbins=0), lambda: _state(n=0), lambda: _state(n=1, nbins=1),
                                  lambda: _state(model=wl.MODEL_PULSE), _with_nan, _empty_bins],
                         ids=["plain", "no_histograms", "empty", "one_sample_one_bin", "pulse_ratio", "nan", "empty_bins"])
def test_c_host_writer_stands_alone(checker, tmp_path, make):
    pr = make()
    y = np.linspace(0.1, 1.3, pr.n_x)
    best = pr.best_curve()
    pr.write(str(tmp_path / "predict.bin"))
    (tmp_path / "curves.bin").write_bytes(np.concatenate([y, best]).astype("<f8").tobytes())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
    subprocess.check_call([checker, str(tmp_path / "predict.bin"), str(tmp_path / "curves.bin"),
                           str(tmp_path / "predict.txt"), str(tmp_path / "again.bin")], env=env)
    assert (tmp_path / "predict.txt").read_text() == pr.text(y, best)
    assert (tmp_path / "again.bin").read_bytes() == (tmp_path / "predict.bin").read_bytes()
