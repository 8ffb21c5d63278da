"""The shipped form of the device sine (tests/predict_ref.sin_cw: n = rint(2 u) from the phase in turns) against a true
sine over its whole argument range, the reduced argument against the interval the polynomial was fitted on, the range
guard against its exact statement, and the loglike probe of tests/test_gpu_sine_domain.py against a CPU model of the
kernels' data sum.  No GPU."""
import math
from fractions import Fraction

import numpy as np
import pytest

from tests import predict_ref as ref
from tests import sine_domain as sd


@pytest.fixture(scope="module")
def errors():
    """{class: [(u, sin_cw - sin)]} over the whole list, computed once"""
    return {name: [(u, sd.sine_error(u)) for u in us] for name, us in sd.phases().items()}


def test_the_list_is_what_the_number_was_measured_on():
    p = sd.phases()
    total = sum(len(v) for v in p.values())
    assert 15000 <= total <= 20000, total
    assert sd.WORST_PHASE in p["half_integer"]
    assert max(abs(u) for u in p["guard_edge"]) == sd.largest_phase()
    assert all(2.0 ** 44 <= abs(sd.argument(u)) < 2.0 ** 45 for u in p["top_octave"])
    # every binary decade of k, both signs and all five offsets among the half integers
    decades = {(int(math.log2(abs(2 * u))), u > 0) for u in p["half_integer"]}
    assert decades == {(e, s) for e in range(44) for s in (True, False)}     # 2 u < 2^45 / pi = 2^43.35
    for f, ph, u in sd.phases_inexact():
        assert 0.1 <= f <= 0.3 and 0 <= ph <= 1 and u == ref.add(ref.mul(f, sd.X0_INEXACT), ph) != ref.fma(f, sd.X0_INEXACT, ph)
    assert len(sd.probe_points("exact")) <= sd.MAX_PROBE_POINTS and len(sd.probe_points("inexact")) <= sd.MAX_PROBE_POINTS
    classes = {name: set(us) for name, us in p.items()}
    probed = {u for _, _, u in sd.probe_points("exact")}
    assert all(probed & classes[c] for c in ("small", "medium", "log_uniform", "half_integer", "integer", "top_octave",
                                             "guard_edge")) and sd.WORST_PHASE in probed
    probed_decades = {int(math.log2(abs(2 * u))) for u in probed & classes["half_integer"]}
    assert probed_decades >= set(range(44)), sorted(set(range(44)) - probed_decades)


def test_shipped_sine_against_a_true_sine_over_the_whole_range(errors):
    """|sin_cw - sin| <= SIN_CW_ABS_ERR at every argument of the list, and SIN_CW_ABS_ERR is the list's worst error plus
    2^-53 -- not more.  Above 4 ulp of 1 the shipped reduction itself would be the finding."""
    worst = (0.0, None, None)
    for name, es in errors.items():
        e, u = max((abs(e), u) for u, e in es)
        print("%-13s %5d arguments, worst error %.4g at u = %r" % (name, len(es), e, u))
        worst = max(worst, (e, u, name))
    print("worst of the list: %.9g at u = %r (%s); SIN_CW_ABS_ERR = %.4g" % (worst + (sd.SIN_CW_ABS_ERR,)))
    assert worst[0] <= sd.SIN_CW_ABS_ERR
    assert worst[0] <= 4 * 2.0 ** -52
    assert worst[1] == sd.WORST_PHASE and 0.999 * sd.WORST_ERR <= worst[0] <= sd.WORST_ERR, worst
    assert sd.SIN_CW_ABS_ERR == sd.WORST_ERR + 2.0 ** -53
    # where 2 u is not next to a half integer the form that ships is the form the fit was checked in
    away = max(abs(e) for name, es in errors.items() if name not in ("half_integer",) for _, e in es)
    assert away <= 2.3e-16, away


def test_the_reduced_argument_stays_next_to_the_fitted_interval():
    """|r| <= pi/2 + 2^-8 (sine_domain.reduced derives it): an argument cannot walk far outside [-pi/2, pi/2]"""
    p = sd.phases()
    excess = {}
    for name in ("half_integer", "integer", "guard_edge", "top_octave"):
        for u in p[name]:
            over = abs(sd.reduced(sd.argument(u), u)) - sd.HALF_PI
            if name in ("half_integer", "guard_edge", "top_octave"):
                assert over <= sd.R_EXCESS_BOUND, (name, u, over)
            e = int(math.log2(abs(2 * u))) if abs(2 * u) >= 1 else 0
            if name == "half_integer":
                excess[e] = max(excess.get(e, -1.0), over)
    for e in sorted(excess):
        print("2u in [2^%d, 2^%d): largest |r| - pi/2 = %.3g" % (e, e + 1, excess[e]))
    assert max(excess.values()) > 1e-3          # the list does reach the arguments that leave the interval
    assert all(excess[e] <= 2.0 ** (e - 52) * 4 for e in excess if e < 40)   # and below 2^40 only by the ulps of x


def test_the_range_guard_at_the_doubles_around_its_edge():
    """predict_ref.sine_in_range against the predicate written out in Fraction, at the doubles on both sides of 2^45"""
    top = sd.largest_phase()
    assert ref.mul(ref.TWO_PI, top) < 2.0 ** 45 <= ref.mul(ref.TWO_PI, math.nextafter(top, math.inf))
    seen = set()
    for x in (1.0, 2.45e6, 1e13, 3.0, 12345.678):
        for ph in (0.0, 0.25, 1.0, top / 2):
            for k in range(-3, 4):
                f = sd.step_ulps((top - ph) / x, k)         # f x + ph within a few ulps of the edge
                for sf in (1.0, -1.0):
                    for sp in (1.0, -1.0):
                        got = ref.sine_in_range(sf * f, sp * ph, x)
                        assert got == sd.exact_in_range(sf * f, sp * ph, x), (f, ph, x)
                        # the unrounded value: at the edge, and on the guard's side of it wherever it is further from
                        # the edge than the predicate's three roundings
                        exact = Fraction(ref.TWO_PI) * (Fraction(f) * Fraction(x) + Fraction(ph))
                        assert abs(exact - 2 ** 45) < 2 ** 45 * Fraction(16, 2 ** 53), (f, ph, x)
                        if abs(exact - 2 ** 45) > 2 ** 45 * Fraction(3, 2 ** 53):
                            assert got == (exact < 2 ** 45), (f, ph, x)
                        seen.add(got)
    assert seen == {True, False}
    v = ref.mul(ref.TWO_PI, top)
    assert v == math.nextafter(2.0 ** 45, 0.0) or v < 2.0 ** 45
    for bad in (math.nan, math.inf, -math.inf):
        assert not ref.sine_in_range(bad, 0.0, 1.0) and not ref.sine_in_range(0.1, bad, 1.0)
        assert not ref.sine_in_range(0.1, 0.0, bad)


@pytest.mark.parametrize("n_data,waves", [(1, 1), (65, 1), (4100, 1), (1025, 4), (4100, 8)])
def test_the_probe_recovers_the_modelled_sine_error(n_data, waves):
    """the probe on a CPU model of the data sum (equal squares added lane by lane, a tree over the lanes, the waves'
    partial sums one after the other): the error it infers is the modelled sine's true error within resolution(), and
    the resolution is below 4e-17"""
    res = sd.resolution(n_data, waves)
    assert res < 4e-17
    t = 64 * waves
    for group in ("exact", "inexact"):
        pts = sd.probe_points(group)[::4]
        data, params, info = sd.probe_inputs(group, n_data, points=pts)
        assert data.shape == (n_data, 2) and len(set(map(tuple, data))) == 1
        prob = np.zeros(len(info))
        for i, h in enumerate(info):
            d = np.float64(h["d_model"])
            lanes = np.zeros(t)
            for lane in range(t):
                for _ in range(len(range(lane, n_data, t))):
                    lanes[lane] = lanes[lane] + d * d
            per_wave = lanes.reshape(waves, 64)
            for width in (32, 16, 8, 4, 2, 1):
                per_wave = per_wave[:, :width] + per_wave[:, width:2 * width]
            total = np.float64(0)
            for w in range(waves):
                total = total + per_wave[w, 0]
            prob[i] = total / -0.5
        err, off = sd.probe_sine_error(prob, info, n_data)
        true_err = np.array([sd.sine_error(h["u"], h["x"]) for h in info])
        assert np.abs(err - true_err).max() <= res, (group, np.abs(err - true_err).max(), res)
        assert np.abs(off).max() <= res
        assert np.abs(err).max() <= sd.SIN_CW_ABS_ERR + res


def test_sine3_probe_parameters_leave_the_other_components_at_zero():
    for c in range(3):
        _, params, info = sd.probe_inputs("exact", 3, model="sine3", component=c, points=sd.probe_points("exact")[:5])
        rest = [j for j in range(9) if j // 3 != c]
        assert params.shape == (5, 10) and not params[:, rest].any()
        assert np.array_equal(params[:, 3 * c], np.ones(5)) and np.array_equal(params[:, 9], [h["o"] for h in info])
        for row, h in zip(params, info):
            assert ref.curve(ref.MODEL_SINE3, row, 1.0) == h["d_model"]
