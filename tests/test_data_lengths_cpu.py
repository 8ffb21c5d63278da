"""The matrix of data lengths (tests/data_lengths.py) against its own restatement of the likelihood loops, and the
extended-precision reference (tests/loglike_ref.py) against known values and against the oracle at every input that
tests/test_gpu_data_lengths.py hands to a kernel.  No GPU."""
import os

import numpy as np
import pytest

from oracle import oracle as orc
from tests import data_lengths as dl
from tests import loglike_ref

SHAPES = [(m, w) for m in dl.MODELS for w in dl.WAVES]


@pytest.mark.parametrize("model,waves", SHAPES)
def test_lengths_reach_every_regime(model, waves):
    t, kw = dl.threads(waves), dl.k_wide(waves)
    lengths = dl.lengths(waves, model)
    assert lengths == sorted(set(lengths)) and lengths[0] == 1
    hit = {n: dl.regimes(n, waves, model) for n in lengths}
    union = set().union(*hit.values())
    assert union == dl.reachable(waves, model), (sorted(union), sorted(dl.reachable(waves, model)))
    # rows in registers: the one length that is exactly kWide * T, and not its neighbours
    assert [n for n in lengths if "rows_in_regs" in hit[n]] == [kw * t]
    assert hit[kw * t] - {"stage_over_64k"} == {"rows_in_regs"}
    for n in (kw * t - 1, kw * t + 1):
        assert n in lengths and "rows_in_regs" not in hit[n]
    if waves <= 2:
        # the pipelined loop: 1 pass (the resident one alone), 2 (one trip, no advance in its second pass), 3 (a trip
        # and the leftover pass), 4 (the second pass of the first trip advances), 5
        counts = {dl.pipe_passes(n, waves, model) for n in lengths}
        if dl.pipelined(waves, model):
            assert {1, 2, 3, 4, 5} <= counts, sorted(counts)
        else:
            assert counts == {0}
    else:
        assert not dl.pipelined(waves, model)
        assert any(16 * n > dl.BIG_LDS for n in lengths)


@pytest.mark.parametrize("model,waves", SHAPES)
def test_every_point_is_evaluated_once_in_the_restated_loops(model, waves):
    """the walk behind regimes() is a partition of the data vector at every length: a restatement that dropped or
    repeated a point would name the wrong regimes"""
    for n in dl.lengths(waves, model):
        _, seen = dl.two_phase_walk(n, waves, model)
        assert seen.tolist() == [1] * n, (n, "two-phase")
        if waves in dl.ONE_BARRIER_WAVES:
            hit, seen = dl.one_barrier_walk(n, waves)
            assert seen.tolist() == [1] * n, (n, "one-barrier")
            assert hit == dl.two_phase_walk(n, waves, model)[0], n   # never pipelined: the same regimes


@pytest.mark.parametrize("model,waves", SHAPES)
def test_reduced_sets_come_from_the_regimes(model, waves):
    t = dl.threads(waves)
    lengths = dl.lengths(waves, model)
    sampled = dl.sampling_lengths(waves, model)
    assert set(sampled) <= set(lengths) and t + 1 in sampled and len(sampled) <= 9
    assert set().union(*(dl.regimes(n, waves, model) for n in sampled)) == dl.reachable(waves, model)
    cal = dl.calibration_lengths(waves, model)
    assert cal == sorted({t + 1, dl.k_wide(waves) * t, lengths[-1]}) and len(cal) == 3


def test_the_regimes_at_known_lengths():
    """spot checks of the restatement against the kernels' code read by hand"""
    assert dl.regimes(256, 1, "simplesin") == {"rows_in_regs"}
    assert dl.regimes(257, 1, "simplesin") == {"pipe_passes_1", "tail1", "partial_wave"}
    assert dl.regimes(257, 1, "pulse") == {"wide4", "tail1", "partial_wave"}           # pulse has no pipelined loop
    assert dl.regimes(768, 1, "sine3") == {"pipe_passes_odd_ge3"}
    assert dl.regimes(1345, 1, "pulse_vrot") == {"pipe_passes_odd_ge3", "wide2", "tail1", "partial_wave"}
    assert dl.regimes(2 * 128 + 1, 2, "simplesin") == {"wide2", "tail1", "partial_wave"}
    assert dl.regimes(1024, 8, "pulse") == {"rows_in_regs"}
    assert dl.regimes(1024, 4, "pulse") == {"rows_in_regs"}
    assert dl.regimes(2048, 8, "pulse") == {"wide2"}                                     # eight waves: no 4-wide loop
    assert dl.regimes(1, 6, "sine3") == {"tail1", "partial_wave", "idle_waves"}
    assert dl.regimes(9 * 384 + 1, 6, "sine3") == {"wide4", "wide4_trips_ge2", "wide2", "tail1", "partial_wave"}
    assert dl.regimes(4100, 4, "simplesin") == {"wide4", "wide4_trips_ge2", "tail1", "partial_wave", "stage_over_64k"}


# ---- the extended-precision reference ---------------------------------------------------------------------------------
def test_extended_reference_is_extended():
    assert np.finfo(np.longdouble).nmant >= 63
    assert loglike_ref.TWO_PI == np.longdouble(2 * np.pi)


def test_extended_reference_reproduces_the_manual_value():
    # doc/manual.rst:190-213 (tests/test_gpu_parity.py::test_loglike_golden_vectors)
    data = np.array([[101, 0.67], [102, 1.01], [103, 7.9e-1], [104, 1.34]])
    prob, prior = loglike_ref.loglike("simplesin", [1, 0.2, 1, 0], data, 1.0)
    assert abs(prob - np.longdouble(-1.480898044165363e+01)) < 1e-12 * 14.8 and prior == 0


def test_extended_reference_reproduces_the_testlc_values(golden_dir):
    d = np.loadtxt(os.path.join(golden_dir, "testlc.dat"))
    got = [loglike_ref.loglike("simplesin", p, d, 1.0)[0] for p in ([0.7, 5.2, 5.4, 0.0], [1.0, 10.0, 0.25, 0.1])]
    np.testing.assert_allclose(np.array(got, dtype=np.float64), [-3.187159885063915e+03, -3.271718790429034e+03],
                               rtol=1e-12)


def test_extended_reference_has_the_oracles_prior_convention():
    w = dl.case("pulse", 65).w
    prob, prior = loglike_ref.loglike("pulse", w.start, w.data, 0.3)
    o_prob, o_prior = orc.loglike(w.model, w.start, w.data, beta=0.3)
    assert dl.rel_err(o_prob, prob) < 1e-13 and dl.rel_err(o_prior, prior) < 1e-13 and prior != 0


@pytest.mark.parametrize("model,waves", SHAPES)
def test_inputs_are_well_conditioned(model, waves):
    """A condition on the inputs of tests/test_gpu_data_lengths.py, not a measurement: at every (length, parameter
    point) a kernel will be held to 1e-12 at, the oracle's plain fp64 sum agrees with the extended reference to 1e-13.
    A point that does not -- a one-point data set whose residual nearly vanishes, a pulse posterior whose prior
    cancels the data sum -- is replaced by another seed (data_lengths.RESEED), never given a wider bound."""
    bad = []
    for n in dl.lengths(waves, model):
        c = dl.case(model, n)
        assert c.params.shape == (6, c.w.n_par) and np.array_equal(c.params[0], c.w.start)
        assert np.all(c.params >= c.w.pmin) and np.all(c.params <= c.w.pmax)
        assert np.all((c.beta >= 0.01) & (c.beta <= 1)) and c.w.n_data == n
        assert np.all(np.isfinite(c.ext_prob.astype(np.float64))) and np.all(np.isfinite(c.orc_prob))
        e_prob, e_prior = dl.rel_err(c.orc_prob, c.ext_prob), dl.rel_err(c.orc_prior, c.ext_prior)
        if e_prob.max() > 1e-13 or e_prior.max() > 1e-13:
            bad.append((n, float(e_prob.max()), float(e_prior.max())))
    assert not bad, bad
