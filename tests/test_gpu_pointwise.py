"""On-device pointwise log-likelihood (apemost_hip_pointwise_*, pt_pointwise.h) against tests/pointwise_ref.py, a
restatement that shares nothing with the kernels.

The comparison rule, for every test (u = 2^-53, one ulp = 2^-52 relative, n the kept samples):

Sine models.  The restatement gives the term bit for bit (rational arithmetic rounded once per operation), so origin,
sum, sq, m_up, m_dn, par_origin and par_sum compare with == on the bits, a NaN by its position.  S_up and S_dn compare
to the rule of tests/test_gpu_evidence.py: each step adds at most one ulp from exp (the device library's bound) and one
from its multiply and add, under n 2^-51 in all; the tolerance is n 2^-50 relative against math.fsum of the
reference's exponentials about the final maximum (itself within an ulp of the exact sum).  S2_dn squares the same
exponential: the exp error counts twice (2 ulps), the multiply and add as before (1 ulp), and the two extra roundings
e * e and S2 * tt (or its addition) half an ulp each (1 ulp): 4 ulps = 2^-50 a step, n 2^-50 in all, and with the same
factor 2 the tolerance is n 2^-49 against the exact sum of the squares of the reference's exponentials.

Pulse models.  The curve v is bit for bit (plain IEEE operations) and so is w = y / v.  The device's log is within one
ulp of ln v (the device library's bound, taken as the evidence test takes exp's) and so is math.log: the two L differ by
at most 2 * 2^-52 |ln v|; L + w rounds once per side and the negation is exact.  Per term
    delta = 2^-51 |ln v| + 2 u |l|.
From it, with delta_t the bound of sample t, delta_0 that of the first and d_t = l_t - origin:
    origin   delta_0
    d_t      e_t = delta_t + delta_0 + 2 u |d_t|                     (one rounding per side)
    sum      sum_t e_t + 2 (n - 1) u sum_t |d_t|                     (n - 1 additions per side)
    sq       sum_t (2 |d_t| e_t + e_t^2 + 2 u d_t^2) + 2 (n - 1) u sum_t d_t^2
    m        max_t delta_t      (the maximum of perturbed values moves by at most the largest perturbation)
    S words  every exponent x_t - m moves by at most 2 max delta (x and m both): a relative perturbation of
             exp(2 max delta) - 1, to first order 2 max delta, of S_up and S_dn and twice that of S2_dn, on top of the
             sine models' n 2^-50 and n 2^-49.
Each of these gets the factor 2 that the evidence test gives its bound.  The worst observed fraction of each bound is
printed.  A series with a non-finite term has no such reference: its NaNs must sit where the restatement's sit, and
what is not NaN compares against the restatement's own sequential S to the same tolerances (both sides then carry the
per-step error, n 2^-51 each).

The real-run tests hold the project's own 1e-12 relative (tests/test_gpu_parity.py::test_loglike_matches_oracle)
between the sum of a kept sample's terms and the engine's own log-likelihood in the row."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.pointwise import PIECE, STATE, Pointwise
from apemost_amd.sampler import HipSampler
from apemost_amd.summary import batches_closed
from tests import hostlib
from tests import pointwise_ref as ref
from tests import predict_ref
from tests.helpers import make_pair
from tests.pointwise_ref import EXACT, RefPointwise, assert_same_state, nan_positions_agree
from tests.predict_ref import same_floats

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SINE = (wl.MODEL_SIMPLESIN, wl.MODEL_SINE3)


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def feed(s, d, calls, skip0=0, thin=1):
    """accumulate d in calls of the given numbers of steps; the kept steps are skip0, skip0 + thin, ... of the whole"""
    off = 0
    for n in calls:
        skip = skip0 - off if off < skip0 else (thin - (off - skip0) % thin) % thin
        s.pointwise_accumulate(d[off:].data_ptr(), n, skip, thin)
        off += n
    assert off == d.shape[0]


def fold(s, rows, chains, calls=None, skip0=0, thin=1, at_mean=False):
    d = on_device(rows)
    s.pointwise_begin(chains=chains, thin=thin)
    feed(s, d, calls or [len(rows)], skip0, thin)
    got = s.pointwise(at_mean=at_mean)
    s.pointwise_end()
    return got


def pulse_delta(model, rows, chains, data, values):
    """delta [n][n_keep][n_data] of the rule for kept rows"""
    n_par = rows.shape[2] - 2
    data = np.asarray(data)
    data = np.tile(data, (len(chains), 1, 1)) if data.ndim == 2 else data
    v = np.array([[[predict_ref.curve(model, rows[t, c, :n_par], xi) for xi in data[k][:, 0]]
                   for k, c in enumerate(chains)] for t in range(len(rows))])
    with np.errstate(all="ignore"):
        return 2.0 ** -51 * np.abs(np.log(v)) + 2 * U * np.abs(values)


def check(got, r, model, what, delta=None):
    """a Pointwise against a RefPointwise by the module's rule; returns the worst fractions of the bounds"""
    n = r.n
    assert int(got.n[0]) == n, (what, int(got.n[0]), n)
    assert same_floats(got.par_origin, r.par_origin) and same_floats(got.par_sum, r.par_sum), what
    worst = {}
    fin = r.finite
    if model in SINE:
        for f in EXACT:
            a, b = getattr(got, f), getattr(r, f)
            if not same_floats(a, b):
                with np.errstate(all="ignore"):
                    bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
                raise AssertionError("%s %s: %d entries differ, first at %s: %r against %r" % (
                    what, f, len(bad), tuple(bad[0]), a[tuple(bad[0])], b[tuple(bad[0])]))
        extra = np.zeros(fin.shape)
    else:
        assert delta is not None and delta.shape == r.values.shape
        for f in EXACT[:5]:
            assert nan_positions_agree(getattr(got, f), getattr(r, f)), (what, f)
        with np.errstate(all="ignore"):
            d = r.values - r.values[0]
            e = delta + delta[0] + 2 * U * np.abs(d)
            bounds = {"origin": delta[0], "sum": e.sum(axis=0) + 2 * (n - 1) * U * np.abs(d).sum(axis=0),
                      "sq": (2 * np.abs(d) * e + e * e + 2 * U * d * d).sum(axis=0) + 2 * (n - 1) * U * (d * d).sum(axis=0),
                      "m_up": delta.max(axis=0), "m_dn": delta.max(axis=0)}
            for f, b in bounds.items():
                diff = np.abs(getattr(got, f) - getattr(r, f))[fin]
                frac = float(np.max(diff / (2 * b[fin]))) if fin.any() else 0.0
                worst[f] = frac
                assert frac <= 1, (what, f, frac)
            # a series with a non-finite term: sum and sq are non-finite with it (checked by position above); origin
            # and the two maxima -- a NaN never moves a maximum, on either side -- keep their bounds over the terms
            # that are not NaN, and an infinite word is the same infinity
            dl = np.where(np.isnan(r.values), -np.inf, delta)
            for f, b in (("origin", delta[0]), ("m_up", dl.max(axis=0)), ("m_dn", dl.max(axis=0))):
                a, w = getattr(got, f), getattr(r, f)
                inf = ~fin & np.isinf(w)
                assert np.array_equal(a[inf], w[inf]), (what, f)
                at = ~fin & np.isfinite(w) & np.isfinite(b)
                diff = np.abs(a - w)[at]
                frac = float(np.max(np.where(diff == 0, 0.0, diff / (2 * b[at])))) if at.any() else 0.0
                worst[f] = max(worst[f], frac)
                assert frac <= 1, (what, f, "beside a non-finite term", frac)
            extra = 2 * (2 * delta.max(axis=0))
    for f, per_step, doubled in (("S_up", 2.0 ** -50, 1), ("S_dn", 2.0 ** -50, 1), ("S2_dn", 2.0 ** -49, 2)):
        a, seq, exact = getattr(got, f), getattr(r, f), getattr(r, f + "_exact")
        assert nan_positions_agree(a, seq), (what, f)
        with np.errstate(all="ignore"):
            want = np.where(fin, exact, seq)
            tol = n * per_step + doubled * extra
            ok = ~np.isnan(seq)
            rel = np.where(a[ok] == want[ok], 0.0, np.abs(a[ok] - want[ok]) / np.abs(want[ok]))
            frac = float(np.max(rel / tol[ok])) if ok.any() else 0.0
        worst[f] = frac
        assert frac <= 1, (what, f, frac)
    print("%s: n = %d, worst fractions of the bounds: %s" % (what, n, ", ".join("%s %.3g" % kv for kv in worst.items())))
    return worst


# ---- 1. pointwise_loglike alone -------------------------------------------------------------------------------------------
def loglike_x():
    return np.concatenate([100 + 0.5 * np.arange(40), [2.45e6 + 0.37, -77.7, 0.0, 1e13]])


@pytest.mark.parametrize("model,n_par", [(wl.MODEL_SIMPLESIN, 4), (wl.MODEL_SINE3, 10)])
def test_sine_terms_bit_for_bit(model, n_par):
    """6 rows x 44 data; row 5 lies past the sine's range guard at the last datum; sigma is not the default"""
    rng = np.random.default_rng(40 + model)
    x = loglike_x()
    data = np.stack([x, rng.uniform(-1, 2, len(x))], 1)
    hi = np.array([2, 0.3, 1, 2] if n_par == 4 else [2, 0.3, 1] * 3 + [2], dtype=float)
    rows = 0.02 + (hi - 0.02) * rng.uniform(size=(6, n_par))
    rows[4, 0] = -1.25                                        # a negative amplitude
    rows[5, 1] = 1e3                                          # 2 pi f x = 6e16 at x = 1e13
    s = HipSampler(model, n_par, 1, data, seed=1, sigma=0.37)
    got = s.pointwise_loglike(rows)
    one = s.pointwise_loglike(rows[2])
    s.close()
    want = ref.terms(model, rows, data, 0.37)
    assert got.shape == (6, 44) and one.tobytes() == got[2].tobytes()
    assert np.isnan(want[5, -1]) and np.isnan(want).sum() == 1 and (want[~np.isnan(want)] < 0).all()
    assert same_floats(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5].tolist()


@pytest.mark.parametrize("model,n_par", [(wl.MODEL_PULSE, 6), (wl.MODEL_PULSE_VROT, 7)])
def test_pulse_terms_to_their_bound(model, n_par):
    """5 rows x 41 data to delta of the rule, with its factor 2"""
    rng = np.random.default_rng(50 + model)
    nu = np.linspace(10, 12, 41)
    data = np.stack([nu, rng.exponential(1.0, 41)], 1)
    base = np.array([5.0, 0.05, 10.6, 4.0, 11.3, 2.5] if n_par == 6 else [5.0, 0.05, 0.05, 10.6, 4.0, 11.3, 2.5])
    rows = base * (1 + 0.1 * rng.uniform(size=(5, n_par)))
    s = HipSampler(model, n_par, 1, data, seed=1)
    got = s.pointwise_loglike(rows)
    s.close()
    want = ref.terms(model, rows, data, 0.5)
    full = np.zeros((5, 1, n_par + 2))
    full[:, 0, :n_par] = rows
    delta = pulse_delta(model, full, [0], data, want.reshape(5, 1, 41)).reshape(5, 41)
    frac = float(np.max(np.abs(got - want) / (2 * delta)))
    print("model %d: worst difference %.3g of its bound" % (model, frac))
    assert np.isfinite(want).all() and frac <= 1


# ---- 2. the fold on hand-built rows: the data sizes ---------------------------------------------------------------------
CHAINS = [0, 3]                                               # two non-adjacent kept chains of five
CACHE = {}


def size_case():
    """12 steps of 5 chains of simplesin parameters around the workload's start, 130 data; the terms of the kept chains
    once per module (the smaller data sets are the first n_data of these)"""
    if "size" not in CACHE:
        rng = np.random.default_rng(1)
        rows = np.zeros((12, 5, 6))
        rows[:, :, :4] = np.array([0.9, 0.2, 0.4, 0.5]) + np.array([0.05, 1e-4, 0.02, 0.05]) * rng.standard_normal((12, 5, 4))
        data = np.stack([np.concatenate([100 + 0.5 * np.arange(128), [2.45e6 + 0.5, -3.25]]), rng.uniform(-1, 2, 130)], 1)
        values = np.stack([ref.terms(wl.MODEL_SIMPLESIN, rows[:, c, :4], data, 0.5) for c in CHAINS], axis=1)
        CACHE["size"] = rows, data, values
    return CACHE["size"]


@pytest.mark.parametrize("n_data", [1, 63, 64, 65, 130])
def test_hand_built_rows_at_every_data_size(n_data):
    """one lane, a wave less one, a full wave, a wave and one, and three data workgroups with a ragged last one; calls
    of 1, 2 and 9 steps against one call"""
    rows, data, values = size_case()
    data, values = data[:n_data], values[:, :, :n_data]
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 5, data, seed=1)
    got = fold(s, rows, CHAINS, [1, 2, 9])
    whole = fold(s, rows, CHAINS)
    s.close()
    r = RefPointwise(wl.MODEL_SIMPLESIN, rows, CHAINS, data, values=values)
    assert got.origin.shape == (2, n_data) and got.x[1].tobytes() == data[:, 0].tobytes() and r.finite.all()
    check(got, r, wl.MODEL_SIMPLESIN, "n_data %d" % n_data)
    assert_same_state(whole, got, "one call")
    assert got.origin.tobytes() == values[0].tobytes()


# ---- 3. the fold on hand-built rows: call boundaries, remainders, tiles and the kinds of series ---------------------------------
HAND_STEPS = 140
HAND_DATA = np.array([[100.5, 0.7], [101.0, 1000.0], [103.5, -1000.0], [2.45e6 + 0.5, 1e5]])


def hand_case(model):
    """140 steps of 5 chains at 4 data whose y are 0.7, 1000, -1000 and 1e5.
    simplesin (4 parameters, 128 rows to an LDS tile): chain 0 has the amplitude 0 and an offset that rises by 0.01 a
    step, so v is the offset: at y = 1000 the term rises at every step (the maximum moves every time), at y = -1000 it
    falls at every step (never), at y = 1e5 it rises by 4000 a step (every exp underflows), at y = 0.7 it rises, then
    falls.  Chain 3 has realistic parameters with noise: at y = 1e5 the term jumps by tens of thousands either way.
    sine3 (10 parameters, 51 rows to a tile): chain 0 is constant, chain 3 realistic with noise."""
    if model not in CACHE:
        rng = np.random.default_rng(2 + model)
        if model == wl.MODEL_SIMPLESIN:
            n_par = 4
            rows = np.zeros((HAND_STEPS, 5, 6))
            rows[:, :, :4] = np.array([0.9, 0.2, 0.4, 0.5]) + np.array([0.05, 1e-4, 0.02, 0.05]) * rng.standard_normal((HAND_STEPS, 5, 4))
            rows[:, 0, 0] = 0.0
            rows[:, 0, 3] = 0.0037 + 0.01 * np.arange(HAND_STEPS)
        else:
            n_par = 10
            start = np.array([0.9, 0.2, 0.4, 0.54, 0.11, 0.1, 0.27, 0.27, 0.7, 0.5])
            rows = np.zeros((HAND_STEPS, 5, 12))
            rows[:, :, :10] = start + 0.02 * np.array([1, 1e-3, 1] * 3 + [1]) * rng.standard_normal((HAND_STEPS, 5, 10))
            rows[:, 0, :10] = start
        values = np.stack([ref.terms(model, rows[:, c, :n_par], HAND_DATA, 0.5) if (c or model == wl.MODEL_SIMPLESIN)
                           else np.tile(ref.terms(model, rows[:1, c, :n_par], HAND_DATA, 0.5), (HAND_STEPS, 1))
                           for c in CHAINS], axis=1)
        CACHE[model] = rows, n_par, values
    return CACHE[model]


@pytest.mark.parametrize("skip0,thin", [(0, 1), (2, 1), (1, 3)])
@pytest.mark.parametrize("model", [wl.MODEL_SIMPLESIN, wl.MODEL_SINE3], ids=["n_par4", "n_par10"])
def test_hand_built_rows_over_every_call_boundary(model, skip0, thin):
    """kept counts 140, 138 and 47: after the first sample the first tile leaves 127 = 31 x 4 + 3 (4 parameters) or
    50 = 12 x 4 + 2 (10 parameters) samples, the later tiles 12 / 10 or 51, 38 / 36: every remainder of the side-by-side
    width, and one or two tile boundaries.  Calls of 1, 2 and 33 steps and the rest, against one call."""
    rows, n_par, values = hand_case(model)
    s = HipSampler(model, n_par, 5, HAND_DATA, seed=1)
    got = fold(s, rows, CHAINS, [1, 2, 33, HAND_STEPS - 36], skip0, thin)
    whole = fold(s, rows, CHAINS, None, skip0, thin)
    s.close()
    kept, v = rows[skip0::thin], values[skip0::thin]
    r = RefPointwise(model, kept, CHAINS, HAND_DATA, values=v)
    assert got.thin == thin and r.finite.all()
    check(got, r, model, "model %d calls %d/%d" % (model, skip0, thin))
    assert_same_state(whole, got, "one call")
    if model == wl.MODEL_SIMPLESIN:
        assert (np.diff(v[:, 0, 1]) > 0).all() and got.m_up[0, 1] == v[-1, 0, 1] and got.m_dn[0, 1] == -v[0, 0, 1]
        assert (np.diff(v[:, 0, 2]) < 0).all() and got.m_up[0, 2] == v[0, 0, 2] and got.m_dn[0, 2] == -v[-1, 0, 2]
        assert (np.diff(v[:, 0, 3]) > 700 * thin).all() and got.S_up[0, 3] == 1.0 and got.S_dn[0, 3] == 1.0
        assert got.S2_dn[0, 3] == 1.0 and np.abs(np.diff(v[:, 1, 3])).min() > 0 and np.abs(np.diff(v[:, 1, 3])).max() > 1e4
        assert got.loo_ess(0)[3] == 1.0
    else:                                                     # the constant chain: S = n exactly, no spread
        n = len(kept)
        assert not got.sum[0].any() and not got.sq[0].any() and got.S_up[0].tolist() == [float(n)] * 4
        assert got.S_dn[0].tolist() == [float(n)] * 4 == got.S2_dn[0].tolist() and got.loo_ess(0).tolist() == [float(n)] * 4
        assert got.lppd(0).tolist() == v[0, 0].tolist() == got.elpd_loo(0).tolist()


# ---- 4. several pieces in one call ----------------------------------------------------------------------------------------------
def test_several_pieces_in_one_call():
    """8192 + 37 kept steps of simplesin at 3 data.  The amplitude is exactly 0, so the curve is the offset whatever the
    sine is (0 * s + o = o) and the term is ((o - y) * (o - y)) * c in plain IEEE operations: numpy states it bit for
    bit, and 24 samples spread over both pieces are confirmed against the rational restatement."""
    n = PIECE + 37
    rng = np.random.default_rng(6)
    data = np.array([[100.0, 0.31], [100.5, 1.77], [2.45e6, -0.4]])
    rows = np.zeros((n, 1, 6))
    rows[:, 0, :4] = [0.0, 0.2, 0.4, 0.0]
    rows[:, 0, 3] = 0.5 + 0.3 * rng.standard_normal(n)
    r0 = rows[:, 0, 3, None] - data[None, :, 1]
    values = ((r0 * r0) * ref.sine_constant(0.5)).reshape(n, 1, 3)
    some = np.concatenate([np.arange(8), PIECE - 4 + np.arange(8), n - 8 + np.arange(8)])
    assert values[some, 0].tobytes() == ref.terms(wl.MODEL_SIMPLESIN, rows[some, 0, :4], data, 0.5).tobytes()
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 1, data, seed=1)
    got = fold(s, rows, (0,))
    again = fold(s, rows, (0,), [PIECE - 3, 5, n - PIECE - 2])
    s.close()
    r = RefPointwise(wl.MODEL_SIMPLESIN, rows, [0], data, values=values)
    check(got, r, wl.MODEL_SIMPLESIN, "two pieces")
    assert_same_state(again, got, "cut elsewhere")
    assert np.all(got.loo_ess() > 1) and np.all(got.loo_ess() < n)


# ---- 5. non-finite parameters and non-positive curves ----------------------------------------------------------------------------
def test_a_non_finite_parameter_stays_in_its_chain():
    rows, data, values = size_case()
    data, values = data[:65], values[:, :, :65]
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 5, data, seed=1)
    clean = fold(s, rows, CHAINS, [1, 2, 9])
    bad = rows.copy()
    bad[7, 3, 1] = np.nan                                     # a NaN frequency in one sample of chain 3
    got = fold(s, bad, CHAINS, [1, 2, 9])
    s.close()
    v = values.copy()
    v[7, 1] = np.nan
    r = RefPointwise(wl.MODEL_SIMPLESIN, bad, CHAINS, data, values=v)
    check(got, r, wl.MODEL_SIMPLESIN, "a NaN frequency")
    for f in STATE:
        assert getattr(got, f)[0].tobytes() == getattr(clean, f)[0].tobytes(), f
    assert got.par_sum[0].tobytes() == clean.par_sum[0].tobytes()
    for f in ("sum", "sq", "S_up", "S_dn", "S2_dn"):
        assert np.isnan(getattr(got, f)[1]).all(), f
    assert np.isnan(got.par_sum[1, 1]) and np.isfinite(got.par_sum[1, [0, 2, 3]]).all()
    assert got.origin[1].tobytes() == clean.origin[1].tobytes()


def test_a_negative_pulse_height_gives_the_restatements_nan():
    """30 steps of a one-mode pulse at 5 data; one row of chain 1 has a negative height, so v < 0 and ln v is NaN: the
    series of that chain are NaN where the restatement's are, the other chain's hold their bounds"""
    rng = np.random.default_rng(7)
    nu = np.array([10.3, 10.55, 10.6, 10.7, 11.9])
    data = np.stack([nu, rng.exponential(1.0, 5)], 1)
    rows = np.zeros((30, 2, 6))
    rows[:, :, :4] = np.array([5.0, 0.05, 10.6, 4.0]) * (1 + 0.02 * rng.standard_normal((30, 2, 4)))
    rows[11, 1, 3] = -4.0
    s = HipSampler(wl.MODEL_PULSE, 4, 2, data, seed=1)
    got = fold(s, rows, (0, 1), [7, 23])
    s.close()
    r = RefPointwise(wl.MODEL_PULSE, rows, [0, 1], data)
    assert np.isnan(r.values[11, 1]).all() and r.finite[0].all() and not r.finite[1].any()
    check(got, r, wl.MODEL_PULSE, "a negative height", pulse_delta(wl.MODEL_PULSE, rows, [0, 1], data, r.values))
    assert np.isnan(got.sum[1]).all() and np.isnan(got.S_dn[1]).all() and np.isfinite(got.sum[0]).all()


# ---- 6. a ladder batch --------------------------------------------------------------------------------------------------------
def test_a_batch_of_three_ladders():
    """three ladders with different data: every kept chain folds over its own ladder's, and each ladder's result equals
    a stand-alone sampler's over that ladder's rows"""
    from tests.test_gpu_ladder_batch import concat, ladders, make_batch, N_ROUNDS, N_SWAP, PER
    ws, seeds, sts, _, _ = ladders("simplesin", 3)
    for b, w in enumerate(ws):
        w.data[:, 0] += 7.25 * b
        w.data[:, 1] += 0.125 * b
    w = ws[0]
    n_steps = N_ROUNDS * N_SWAP
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    d = torch.zeros((n_steps, 3 * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    chains = [0, PER, 2 * PER + 1]
    batch.pointwise_begin(chains=chains)
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.pointwise_accumulate(d.data_ptr(), n_steps)
    got = batch.pointwise()
    batch.pointwise_end()
    batch.close()
    rows = d.cpu().numpy()
    assert got.n_ladders == 3 and got.n_data == w.n_data and int(got.n[0]) == n_steps
    lads = got.per_ladder()
    for b in range(3):
        assert got.x[b].tobytes() == ws[b].data[:, 0].tobytes() and got.y[b].tobytes() == ws[b].data[:, 1].tobytes()
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=1)
        mine = fold(alone, rows[:, b * PER:(b + 1) * PER], (chains[b] - b * PER,), at_mean=True)
        alone.close()
        assert_same_state(lads[b], mine, "ladder %d" % b)
        # at_mean comes from the device term over the ladder's own data (pointwise_loglike's ladder argument)
        assert np.isfinite(lads[b].at_mean).all() and lads[b].at_mean.tobytes() == mine.at_mean.tobytes()
    assert not same_floats(got.origin[0], got.origin[1])


# ---- 7. pointwise_set: a resumed run ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [5, 30])
def test_set_resumes_a_fold(cut):
    """get, end, begin, set and more samples equal the uninterrupted fold of 60 samples, bit for bit"""
    rows, n_par, _ = hand_case(wl.MODEL_SIMPLESIN)
    rows = rows[:60]
    s = HipSampler(wl.MODEL_SIMPLESIN, n_par, 5, HAND_DATA, seed=1)
    d = on_device(rows)
    whole = fold(s, rows, CHAINS)
    part = fold(s, rows[:cut], CHAINS)
    assert int(part.n[0]) == cut
    s.pointwise_begin(chains=CHAINS)
    s.pointwise_set(part)
    s.pointwise_accumulate(d[cut:].data_ptr(), 60 - cut)
    got = s.pointwise(at_mean=False)
    s.pointwise_end()
    s.close()
    assert_same_state(got, whole, "resumed at %d" % cut)
    assert got.origin.tobytes() == part.origin.tobytes() and got.par_origin.tobytes() == part.par_origin.tobytes()


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    n_chains = 96
    w = wl.simplesin(n_data=64, n_chain=n_chains)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    st, _, _ = make_pair(w, n_chains, seed=1)
    s.set_state(st)
    L = capi.lib()
    d = torch.zeros((12, n_chains, w.n_par + 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pw = Pointwise.empty((0,), w.data[:, 0], w.data[:, 1], 4, 0)
    assert L.apemost_hip_pointwise_accumulate(s._h, d.data_ptr(), 12, 0, 1) == capi.ERR_INVALID     # no begin
    assert L.apemost_hip_pointwise_get(s._h, C.byref(pw.view())) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_set(s._h, C.byref(pw.view())) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_begin(s._h, None) == capi.ERR_INVALID
    ip = C.POINTER(C.c_int32)

    def begin(chains=(0,)):
        ch = np.array(chains, dtype=np.int32)
        cfg = capi.PointwiseConfig(n_keep=len(ch), chains=ch.ctypes.data_as(ip) if len(ch) else None)
        return L.apemost_hip_pointwise_begin(s._h, C.byref(cfg))
    refused = ((), (0, 0), (2, 1), (n_chains,), (-1,), tuple(range(n_chains + 1)))
    for ch in refused:
        assert begin(ch) == capi.ERR_INVALID, ch
        assert L.apemost_hip_pointwise_get(s._h, C.byref(pw.view())) == capi.ERR_INVALID, ch       # nothing was begun
    assert begin() == capi.OK
    assert L.apemost_hip_pointwise_accumulate(s._h, d.data_ptr(), 12, 0, 0) == capi.ERR_INVALID    # thin 0
    assert L.apemost_hip_pointwise_accumulate(s._h, None, 12, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_get(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_accumulate(s._h, d.data_ptr(), 12, 12, 1) == capi.OK             # keeps nothing
    assert L.apemost_hip_pointwise_accumulate(s._h, d.data_ptr(), 12, 2, 3) == capi.OK
    assert L.apemost_hip_pointwise_get(s._h, C.byref(pw.view())) == capi.OK and int(pw.n[0]) == 4
    assert not pw.sum.any() and pw.S_up[0].tolist() == [4.0] * 64       # (rows of zeros: a constant term)
    # a begin that is refused leaves the fold begun before open, accumulating as it was
    for ch in refused:
        assert begin(ch) == capi.ERR_INVALID, ch
    assert L.apemost_hip_pointwise_begin(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_accumulate(s._h, d.data_ptr(), 12, 0, 4) == capi.OK
    assert L.apemost_hip_pointwise_get(s._h, C.byref(pw.view())) == capi.OK and int(pw.n[0]) == 7
    assert pw.S_dn[0].tolist() == [7.0] * 64
    s.pointwise_end()
    assert L.apemost_hip_pointwise_get(s._h, C.byref(pw.view())) == capi.ERR_INVALID
    out, par = np.zeros((2, 64)), np.zeros((2, 4))
    ll = L.apemost_hip_pointwise_loglike
    assert ll(s._h, 0, par.ctypes.data_as(capi._dp), out.ctypes.data_as(capi._dp)) == capi.ERR_INVALID
    assert ll(s._h, 2, None, out.ctypes.data_as(capi._dp)) == capi.ERR_INVALID
    assert ll(s._h, 2, par.ctypes.data_as(capi._dp), None) == capi.ERR_INVALID
    assert ll(s._h, 2, par.ctypes.data_as(capi._dp), out.ctypes.data_as(capi._dp)) == capi.OK      # needs no begin
    lad = L.apemost_hip_pointwise_loglike_ladder
    for b in (-1, 1):                                         # an ordinary sampler has ladder 0 only
        assert lad(s._h, b, 2, par.ctypes.data_as(capi._dp), out.ctypes.data_as(capi._dp)) == capi.ERR_INVALID
    again = np.zeros_like(out)
    assert lad(s._h, 0, 2, par.ctypes.data_as(capi._dp), again.ctypes.data_as(capi._dp)) == capi.OK
    assert again.tobytes() == out.tobytes()
    # the sampler still steps
    before = s.get_state()
    s.run_sampler(3, 5, d.data_ptr())
    s.synchronize()
    assert np.array_equal(s.get_state().n_iter, before.n_iter + 15)
    s.close()


def test_too_many_series_are_refused():
    """n_keep * n_data above 2^20 series: 3 chains of 349 526 data is 2^20 + 2; 2 chains are accepted"""
    n_data = 349526
    data = np.stack([100 + 0.5 * np.arange(n_data), np.ones(n_data)], 1)
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 3, data, seed=1)
    L = capi.lib()
    ch = np.arange(3, dtype=np.int32)
    cfg = capi.PointwiseConfig(n_keep=3, chains=ch.ctypes.data_as(C.POINTER(C.c_int32)))
    assert L.apemost_hip_pointwise_begin(s._h, C.byref(cfg)) == capi.ERR_INVALID
    assert b"2^20" in L.apemost_hip_last_error()
    cfg.n_keep = 2
    assert L.apemost_hip_pointwise_begin(s._h, C.byref(cfg)) == capi.OK
    s.pointwise_end()
    s.close()


def test_a_user_model_has_no_term():
    rs = np.random.RandomState(5)
    data = np.column_stack([(rs.uniform(size=64) < 0.5).astype(float), rs.normal(0, 1, (64, 2))])
    s = HipSampler(wl.MODEL_USER, 3, 5, data, seed=1,
                   device_model_source=os.path.join(hostlib.HOST, "examples", "device_models", "bernoulli_example.hip"))
    L = capi.lib()
    ch = np.zeros(1, dtype=np.int32)
    cfg = capi.PointwiseConfig(n_keep=1, chains=ch.ctypes.data_as(C.POINTER(C.c_int32)))
    pw = Pointwise.empty((0,), np.zeros(64), np.zeros(64), 3, wl.MODEL_USER)
    d = torch.zeros((4, 5, 5), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    out, par = np.zeros((1, 64)), np.zeros((1, 3))
    assert L.apemost_hip_pointwise_begin(s._h, C.byref(cfg)) == capi.ERR_UNSUPPORTED
    assert b"user" in L.apemost_hip_last_error()
    assert L.apemost_hip_pointwise_accumulate(s._h, d.data_ptr(), 4, 0, 1) == capi.ERR_UNSUPPORTED
    assert L.apemost_hip_pointwise_get(s._h, C.byref(pw.view())) == capi.ERR_UNSUPPORTED
    assert L.apemost_hip_pointwise_set(s._h, C.byref(pw.view())) == capi.ERR_UNSUPPORTED
    assert L.apemost_hip_pointwise_end(s._h) == capi.ERR_UNSUPPORTED
    assert L.apemost_hip_pointwise_loglike(s._h, 1, par.ctypes.data_as(capi._dp),
                                           out.ctypes.data_as(capi._dp)) == capi.ERR_UNSUPPORTED
    s.close()


# ---- 9. beside the other folds -------------------------------------------------------------------------------------------
def test_beside_the_other_folds():
    """summary, joint, evidence, autocorrelation, predict and pointwise open on the same rows: each equals what it gives
    alone"""
    from tests.test_gpu_summary import _run
    w, s, d, _ = _run("simplesin16")
    n_steps = d.shape[0]
    pieces = [(0, 100), (100, n_steps - 100)]
    nb = batches_closed(n_steps, 7)
    names = ["summary", "joint", "evidence", "autocorr", "predict", "pointwise"]

    def begin(which):
        if "summary" in which:
            s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=7, max_batches=nb)
        if "joint" in which:
            s.joint_begin(w.pmin, w.pmax, chains=(0, 2), nbins=64)
        if "evidence" in which:
            s.evidence_begin(batch_size=7, max_batches=nb)
        if "autocorr" in which:
            s.autocorr_begin(chains=(0, 2), max_lag=50)
        if "predict" in which:
            s.predict_begin(chains=(0, 2), nbins=40, lo=-1.0, hi=2.0)
        if "pointwise" in which:
            s.pointwise_begin(chains=(0, 2))
        for first, n in pieces:
            for name in which:
                getattr(s, name + "_accumulate")(d[first:].data_ptr(), n)
        out = {name: getattr(s, name)() for name in which}
        for name in which:
            if name != "summary":
                getattr(s, name + "_end")()
        return out
    every = begin(names)
    alone = {name: begin([name])[name] for name in names}
    s.close()
    assert_same_state(every["pointwise"], alone["pointwise"], "beside the others")
    assert every["pointwise"].at_mean.tobytes() == alone["pointwise"].at_mean.tobytes()
    assert int(every["pointwise"].n[0]) == n_steps and np.isfinite(every["pointwise"].lppd()).all()
    assert np.array_equal(every["summary"].hist, alone["summary"].hist)
    assert every["summary"].prob_sum.tobytes() == alone["summary"].prob_sum.tobytes()
    assert every["summary"].batch_sums.tobytes() == alone["summary"].batch_sums.tobytes()
    assert np.array_equal(every["joint"].counts, alone["joint"].counts)
    for f in ("origin", "sum", "cross"):
        assert getattr(every["joint"], f).tobytes() == getattr(alone["joint"], f).tobytes(), f
    for f in ("origin", "sum", "sq", "batch", "m", "S"):
        assert getattr(every["evidence"], f).tobytes() == getattr(alone["evidence"], f).tobytes(), f
    for f in ("origin", "sum", "lag", "head", "tail"):
        assert getattr(every["autocorr"], f).tobytes() == getattr(alone["autocorr"], f).tobytes(), f
    for f in predict_ref.FIELDS:
        assert getattr(every["predict"], f).tobytes() == getattr(alone["predict"], f).tobytes(), f


# ---- 10. a real run between launches -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["simplesin", "pulse"])
def test_a_real_run_between_launches(name):
    """8 chains, 64 data, 4 launches of 60 steps (240 kept samples), chain 0 (beta = 1).  The sum over the data of a kept sample's terms,
    from pointwise_loglike on the row's parameters, equals column n_par+1 of the row (prob - prior = beta * loglike)
    divided by beta -- for pulse after parameter 1, the offset the reference adds to its sum, has been added -- to the
    1e-12 relative that tests/test_gpu_parity.py::test_loglike_matches_oracle holds for the engine's own sum.  Every
    kept term is finite, which is asserted: the comparison cannot pass by skipping.  The fold between the launches
    equals the fold of the same rows in one call, and the sampler's trajectory equals a run without the fold.
    The launches make no swap attempt, and the chains start from the device's own prob of their parameters: like the
    reference (src/parallel_tempering_interaction.c:99-123), the engine exchanges the parameters of two chains and
    leaves each chain's prob as it was until its next accepted step, so that after a swap -- or before the first
    accepted step of a chain whose prob was never computed -- a row's prob is not that of the row's parameters, and
    the identity above is not one the engine's rows have.  Without swaps every row has it, and every row is compared.
    For pulse a second thing of the same kind: a rejected step leaves the prior of its proposal behind, as the
    reference does (apps/pulse.c:33 sets it before the decision, and a rejection restores the parameters and prob only),
    so column n_par+1 of a row whose step was rejected is prob minus another point's prior.  The engine's
    log-likelihood of such a row is column n_par (prob) minus the prior of the row's own parameters,
    -sum_j ln(h_j + HMIN) / n_modes, which is what every pulse row is compared against; where the step was accepted
    that is column n_par+1 itself, which is asserted too."""
    n_chain, n_rounds, n_swap, launches = 8, 10, 6, 4
    w = wl.simplesin(n_data=64, n_chain=n_chain) if name == "simplesin" else wl.pulse(n_data=64, n_chain=n_chain)
    st, _, _ = make_pair(w, n_chain, seed=5)
    assert st.beta[0] == 1.0
    per = n_rounds * n_swap
    out = []
    for with_fold in (True, False):
        s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=5)
        st.prob[:], st.prior[:] = s.loglike(st.params, st.beta)
        s.set_state(st)
        d = torch.zeros((launches, per, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
        if with_fold:
            s.pointwise_begin(chains=(0,))
        for k in range(launches):
            s.launch_rounds(1, per, False, d[k].data_ptr())
            if with_fold:
                s.pointwise_accumulate(d[k].data_ptr(), per)
        got = s.pointwise() if with_fold else None
        s.synchronize()
        rows = d.cpu().numpy().reshape(launches * per, n_chain, w.n_par + 2)
        if with_fold:
            s.pointwise_end()
            whole = fold(s, rows, (0,), at_mean=True)
            assert int(got.n[0]) == launches * per
            assert_same_state(got, whole, "interleaved against one call")
            assert got.at_mean.tobytes() == whole.at_mean.tobytes()
            terms = s.pointwise_loglike(rows[:, 0, :w.n_par])
            assert terms.shape == (launches * per, 64) and np.isfinite(terms).all()
            total = np.array([math.fsum(t) for t in terms.tolist()])
            if name == "simplesin":
                engine = rows[:, 0, w.n_par + 1] / s.get_state().beta[0]
            else:
                heights = rows[:, 0, 3:w.n_par:2]
                prior = -np.log(heights + 1e-6).sum(axis=1) / heights.shape[1]       # apps/pulse.c:16-22, HMIN 1e-6
                engine = (rows[:, 0, w.n_par] - prior) / s.get_state().beta[0] + rows[:, 0, 1]
                accepted = np.concatenate([[False], np.any(np.diff(rows[:, 0, :w.n_par], axis=0) != 0, axis=1)])
                assert accepted.any()                         # and where a step was accepted the column itself holds it
                assert np.allclose(rows[accepted, 0, w.n_par + 1], engine[accepted] - rows[accepted, 0, 1], rtol=1e-12, atol=0)
            worst = float(np.max(np.abs(total - engine) / np.abs(engine)))
            print("%s: sum of the terms against the engine's log-likelihood: worst relative difference %.3g" % (name, worst))
            assert worst <= 1e-12
            assert got.origin[0].tobytes() == terms[0].tobytes()
            assert got.m_up[0].tobytes() == terms.max(axis=0).tobytes() and got.m_dn[0].tobytes() == (-terms).max(axis=0).tobytes()
            assert np.allclose(got.par_mean(), rows[:, 0, :w.n_par].mean(axis=0), rtol=1e-12, atol=0)
            assert got.at_mean[0].tobytes() == s.pointwise_loglike(got.par_mean()).tobytes()
            c = got.criteria()
            assert all(np.isfinite(v) for v in c.values()) and c["p_waic2"] > 0 and c["p_loo"] > 0
            assert np.all(got.loo_ess() >= 1) and np.all(got.loo_ess() <= launches * per)
            assert np.all(got.elpd_loo() <= got.lppd())       # the harmonic mean lies below the arithmetic mean
        out.append((s.get_state(), rows))
        s.close()
    for f in ("params", "prob", "prior", "accept", "reject", "n_iter", "swapcount", "step", "beta"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()


@pytest.mark.parametrize("name", ["simplesin", "pulse"])
def test_a_run_with_swaps_against_the_engines_loglike(name):
    """the same ladders stepped with swap attempts: rows that a swap brought into chain 0 are kept samples too.  Their
    column n_par+1 belongs to other parameters (the docstring above), so the engine's log-likelihood of a row is taken
    from HipSampler.loglike on the row's own parameters at beta = 1, prob - prior: the round kernels' data sum.  The
    sum of the terms equals it -- for pulse after parameter 1 has been added -- to the same 1e-12 relative, on every
    row; that swaps were accepted into chain 0 is asserted."""
    n_chain, n_rounds, n_swap = 8, 100, 6
    w = wl.simplesin(n_data=64, n_chain=n_chain) if name == "simplesin" else wl.pulse(n_data=64, n_chain=n_chain)
    st, _, _ = make_pair(w, n_chain, seed=5)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=5)
    st.prob[:], st.prior[:] = s.loglike(st.params, st.beta)
    s.set_state(st)
    d = torch.zeros((n_rounds * n_swap, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
    s.run_sampler(n_rounds, n_swap, d.data_ptr())
    s.synchronize()
    assert int(s.get_state().swapcount[0]) > 0
    rows = d.cpu().numpy()
    p = np.ascontiguousarray(rows[:, 0, :w.n_par])
    terms = s.pointwise_loglike(p)
    prob, prior = s.loglike(p, np.ones(len(p)))
    s.close()
    assert np.isfinite(terms).all()
    total = np.array([math.fsum(t) for t in terms.tolist()])
    engine = prob - prior + (p[:, 1] if name == "pulse" else 0.0)
    worst = float(np.max(np.abs(total - engine) / np.abs(engine)))
    print("%s with swaps: sum of the terms against the engine's log-likelihood: worst relative difference %.3g" % (name, worst))
    assert worst <= 1e-12


# ---- 11. the C host: APEMOST_DUMP=binary,pointwise ----------------------------------------------------------------------------
def test_c_host_pointwise_token(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters = 8, 3000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    runs = {}
    for mode in ("binary,pointwise", "pointwise"):
        work = tmp_path / mode.replace(",", "_")
        work.mkdir()
        (work / "params").write_text(w.params_file_text())
        (work / "data").write_text(w.data_file_text())
        env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP=mode)
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
        runs[mode] = (work, env)
    work, env = runs["binary,pointwise"]
    _, params, probs = samples_bin.read(str(work / "samples.bin"))       # [iters][1][n_par], [iters][n_beta][2]
    rows = np.zeros((iters, 1, w.n_par + 2))
    rows[:, 0, :w.n_par] = params[:, 0]
    rows[:, 0, w.n_par:] = probs[:, 0]
    got = Pointwise.read(str(work / "pointwise.bin"))
    assert (got.n_keep, got.n_data, got.n_par, got.thin, got.n_ladders, got.model, got.sigma) == (1, 128, w.n_par, 1, 1, 0, 0.5)
    assert int(got.n[0]) == iters and got.chains.tolist() == [0]
    data = np.loadtxt(str(work / "data"))                     # what the host parsed
    assert got.x[0].tobytes() == data[:, 0].tobytes() and got.y[0].tobytes() == data[:, 1].tobytes()
    s = HipSampler(w.model, w.n_par, 1, data, seed=1)
    mine = fold(s, rows, (0,), at_mean=True)
    s.close()
    assert_same_state(got, mine, "the C host")
    assert got.at_mean.tobytes() == mine.at_mean.tobytes() and np.isfinite(got.at_mean).all()
    text = (work / "pointwise.txt").read_text()
    assert text == got.text()
    assert (work / "criteria.txt").read_text() == got.criteria_text()
    cols = np.array([[float(v) for v in ln.split("\t")] for ln in text.split("\n")[:-1]])
    assert cols.shape == (128, 8) and np.isfinite(cols).all()
    # alone the token writes no sample file
    only, _ = runs["pointwise"]
    assert not [f for f in os.listdir(str(only)) if f.endswith(".prob.dump") or f.startswith("prob-chain") or f == "samples.bin"]
    assert (only / "pointwise.bin").read_bytes() == (work / "pointwise.bin").read_bytes()
    assert (only / "criteria.txt").read_text() == (work / "criteria.txt").read_text()
    # --append resumes from the file; a misspelt token is refused
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = Pointwise.read(str(work / "pointwise.bin"))
    assert int(second.n[0]) == 2 * iters and second.origin.tobytes() == got.origin.tobytes()
    assert np.all(second.m_up >= got.m_up) and np.all(second.m_dn >= got.m_dn)
    bad = dict(env, APEMOST_DUMP="binary,pointwis")
    assert subprocess.call([exe, "run"], cwd=str(work), env=bad, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           timeout=300) != 0
