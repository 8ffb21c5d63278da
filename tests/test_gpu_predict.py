"""On-device posterior predictive (apemost_hip_predict_*, pt_predict.h): the curves of the four built-in models equal the
rational restatement of tests/predict_ref.py with == on the bits, and every field of the fold equals its sequential
loops: on hand-built rows over every call boundary, with x = NULL, with non-finite parameters, over several staged
pieces, at the histogram extremes, on a real run, on a ladder batch, through predict_set, with invalid arguments, beside
the other folds and through the C host's APEMOST_DUMP=predict."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.predict import PIECE, Predict
from apemost_amd.sampler import HipSampler
from apemost_amd.summary import batches_closed
from tests import hostlib
from tests import predict_ref as ref
from tests.helpers import make_pair
from tests.predict_ref import FIELDS, RefPredict, assert_equals, same_floats

pytestmark = pytest.mark.gpu


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def feed(s, d, calls, skip0=0, thin=1):
    """accumulate d in calls of the given numbers of steps; the kept steps are skip0, skip0 + thin, ... of the whole"""
    off = 0
    for n in calls:
        skip = skip0 - off if off < skip0 else (thin - (off - skip0) % thin) % thin
        s.predict_accumulate(d[off:].data_ptr(), n, skip, thin)
        off += n
    assert off == d.shape[0]


def tiny_sampler(model, n_par, n_chains=1, n_data=16):
    data = np.stack([100 + 0.5 * np.arange(n_data), np.ones(n_data)], 1)
    return HipSampler(model, n_par, n_chains, data, seed=1)


# ---- 1. the curves, bit for bit -------------------------------------------------------------------------------------
N_X = 130                                                     # two full waves of abscissae and two more


def sine_abscissae():
    x = np.concatenate([100 + 0.5 * np.arange(100), 2.45e6 + 0.01 * np.arange(20) + 0.003, -250.25 - 0.7 * np.arange(9),
                        [1e15]])                              # the last one lies past the 2^45 guard
    assert len(x) == N_X
    return x


@pytest.mark.parametrize("model,n_par", [(wl.MODEL_SIMPLESIN, 4), (wl.MODEL_SINE3, 10)])
def test_sine_curves_bit_for_bit(model, n_par):
    rng = np.random.default_rng(20 + model)
    x = sine_abscissae()
    hi = np.array([2, 0.3, 1, 2] if n_par == 4 else [2, 0.3, 1] * 3 + [2], dtype=float)
    rows = 0.02 + (hi - 0.02) * rng.uniform(size=(7, n_par))
    rows[5, 0] = -1.25                                        # a negative amplitude
    rows[6, 1] = 1e-3                                         # at x = 1e15 this one stays inside the guard: 6.3e12
    s = tiny_sampler(model, n_par)
    got = s.predict_curve(rows, x)
    one = s.predict_curve(rows[2], x)
    s.close()
    want = ref.curves(model, rows, x)
    assert got.shape == (7, N_X) and one.tobytes() == got[2].tobytes()
    assert np.isnan(want[:6, -1]).all() and np.isnan(got[:6, -1]).all() and np.isfinite(want[:, :-1]).all()
    assert (n_par == 10 or np.isfinite(want[6, -1]))
    assert same_floats(got, want), np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5].tolist()


@pytest.mark.parametrize("model,n_par", [(wl.MODEL_PULSE, 6), (wl.MODEL_PULSE_VROT, 7)])
def test_pulse_curves_bit_for_bit(model, n_par):
    rng = np.random.default_rng(30 + model)
    x = np.concatenate([np.linspace(10, 12, 126), [10.6e30, 11.3e-30, 10.6, 0.0]])
    assert len(x) == N_X
    base = np.array([5.0, 0.05, 10.6, 4.0, 11.3, 2.5] if n_par == 6 else [5.0, 0.05, 0.05, 10.6, 4.0, 11.3, 2.5])
    rows = base * (1 + 0.05 * rng.uniform(size=(7, n_par)))
    f0, f1 = n_par - 4, n_par - 2                             # the two mode frequencies; the heights follow them
    rows[2, f0 + 1] = 0.0                                     # one zero height
    rows[3, f0 + 1] = rows[3, f1 + 1] = 0.0                   # all heights zero: the curve is 0
    rows[4, [f0, f1]] *= 1e30
    rows[5, [f0, f1]] *= 1e-30
    s = tiny_sampler(model, n_par)
    got = s.predict_curve(rows, x)
    s.close()
    want = ref.curves(model, rows, x)
    assert got.shape == (7, N_X) and not got[3].any() and np.isfinite(got).all() and got[4, :126].max() < 1e-50
    assert got.tobytes() == want.tobytes()
    if model == wl.MODEL_PULSE:
        assert got.tobytes() == ref.pulse_numpy(rows, x).tobytes()


# ---- 2. hand-built rows over every call boundary ------------------------------------------------------------------------
HAND_STEPS, HAND_CHAINS = 60, [0, 3]
HAND_BINS, HAND_LO, HAND_HI = 37, 0.1, 1.2                    # the curves span about [-0.5, 1.6]: some values fall outside


def hand_x():
    return np.concatenate([100 + 0.5 * np.arange(128), [2.45e6 + 0.5, -3.25]])


def hand_rows(seed=1):
    """5 chains of simplesin parameters around the workload's start; prob has a tie at its maximum in both kept chains"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((HAND_STEPS, 5, 6))
    rows[:, :, :4] = np.array([0.9, 0.2, 0.4, 0.5]) + np.array([0.05, 1e-4, 0.02, 0.05]) * rng.standard_normal((HAND_STEPS, 5, 4))
    rows[:, :, 4] = -100 + rng.uniform(size=(HAND_STEPS, 5))
    rows[:, :, 5] = rows[:, :, 4] + 1
    rows[[7, 22, 41], 0, 4] = -50.0                           # first occurrence: kept index of step 7 (or the next kept one)
    rows[[25, 26], 3, 4] = -60.0
    return rows


VALUES = {}


def hand_values(rows, seed):
    """the restatement's curves [steps][kept chain][n_x] of hand_rows(seed): once per module"""
    if seed not in VALUES:
        x = hand_x()
        VALUES[seed] = np.array([[[ref.curve(wl.MODEL_SIMPLESIN, rows[t, c, :4], xi) for xi in x] for c in HAND_CHAINS]
                                 for t in range(rows.shape[0])])
    return VALUES[seed]


@pytest.fixture(scope="module")
def sampler5():
    s = tiny_sampler(wl.MODEL_SIMPLESIN, 4, n_chains=5)
    yield s
    s.close()


@pytest.mark.parametrize("skip0,thin", [(0, 1), (2, 1), (1, 3)])
def test_hand_built_rows_over_every_call_boundary(sampler5, skip0, thin):
    """130 abscissae: two full workgroups and one of two lanes; calls of 1, 2 and 33 steps and the rest; 37 bins over a
    range that leaves values outside; a tie in prob"""
    rows, x = hand_rows(), hand_x()
    values = hand_values(rows, 1)
    d = on_device(rows)
    s = sampler5
    s.predict_begin(chains=HAND_CHAINS, x=x, nbins=HAND_BINS, lo=HAND_LO, hi=HAND_HI, thin=thin)
    feed(s, d, [1, 2, 33, HAND_STEPS - 36], skip0, thin)
    got = s.predict()
    kept = rows[skip0::thin]
    want = RefPredict(wl.MODEL_SIMPLESIN, kept, HAND_CHAINS, x, HAND_BINS, HAND_LO, HAND_HI, values=values[skip0::thin])
    assert int(got.n[0]) == len(kept) and got.thin == thin and got.x.shape == (2, N_X)
    assert_equals(got, want, "calls %d/%d" % (skip0, thin))
    s.predict_begin(chains=HAND_CHAINS, x=x, nbins=HAND_BINS, lo=HAND_LO, hi=HAND_HI, thin=thin)
    feed(s, d, [HAND_STEPS], skip0, thin)
    assert_equals(s.predict(), got, "one call %d/%d" % (skip0, thin))
    s.predict_end()
    counted = got.hist.sum(axis=2)
    assert counted.max() > 0 and (counted < len(kept)).any()  # some values fell outside the range
    first = [t for t in (7, 22, 41) if t >= skip0 and (t - skip0) % thin == 0][0]
    assert got.best_prob.tolist() == [-50.0, -60.0] and int(got.best_n[0]) == (first - skip0) // thin + 1
    assert got.best_params[0].tobytes() == rows[first, 0, :4].tobytes()
    assert got.origin.tobytes() == values[skip0].tobytes()


# ---- 3. x = NULL ------------------------------------------------------------------------------------------------------
def test_x_null_takes_the_data_abscissae():
    w = wl.simplesin(n_data=70, n_chain=4)
    s = HipSampler(w.model, w.n_par, 4, w.data, seed=1)
    rows = hand_rows(2)[:20, :4]
    d = on_device(rows)
    s.predict_begin(chains=(1,))
    s.predict_accumulate(d.data_ptr(), 20)
    got = s.predict()
    s.predict_begin(chains=(1,), x=w.data[:, 0])
    s.predict_accumulate(d.data_ptr(), 20)
    same = s.predict()
    curves = s.predict_curve(rows[:, 1, :4])                  # x = NULL here too
    s.predict_end()
    s.close()
    assert got.n_x == 70 and got.x.tobytes() == w.data[:, 0].tobytes() and curves.shape == (20, 70)
    assert_equals(got, same, "x = NULL")
    assert got.origin[0].tobytes() == curves[0].tobytes()
    assert got.vmax[0].tobytes() == curves.max(axis=0).tobytes() and got.vmin[0].tobytes() == curves.min(axis=0).tobytes()
    assert same_floats(curves, ref.curves(w.model, rows[:, 1, :4], w.data[:, 0]))


# ---- 4. non-finite parameters -------------------------------------------------------------------------------------------
def test_non_finite_parameters_stay_in_their_chain(sampler5):
    rows, x = hand_rows(), hand_x()
    s = sampler5

    def fold(r):
        d = on_device(r)
        s.predict_begin(chains=HAND_CHAINS, x=x, nbins=HAND_BINS, lo=HAND_LO, hi=HAND_HI)
        feed(s, d, [1, 2, 33, HAND_STEPS - 36])
        return s.predict()
    clean = fold(rows)
    bad = rows.copy()
    bad[20, 3, 1] = np.nan                                    # a NaN frequency and an infinite phase: the curve is NaN
    bad[30, 3, 2] = np.inf
    bad[25, 3, 4] = np.nan                                    # the best sample of chain 3 had this prob
    got = fold(bad)
    s.predict_end()
    values = hand_values(rows, 1).copy()
    values[[20, 30], 1] = np.nan
    assert_equals(got, RefPredict(wl.MODEL_SIMPLESIN, bad, HAND_CHAINS, x, HAND_BINS, HAND_LO, HAND_HI, values=values))
    for f in ("origin", "sum", "sq", "vmin", "vmax", "hist", "best_prob", "best_params", "best_n"):
        assert getattr(got, f)[0].tobytes() == getattr(clean, f)[0].tobytes(), f
    assert np.isnan(got.sum[1]).all() and np.isnan(got.sq[1]).all()
    assert got.vmin[1].tobytes() == np.delete(values[:, 1], [20, 30], axis=0).min(axis=0).tobytes()
    assert got.vmax[1].tobytes() == np.delete(values[:, 1], [20, 30], axis=0).max(axis=0).tobytes()
    assert np.isfinite(got.vmin).all() and np.isfinite(got.vmax).all()
    assert np.all(clean.hist[1].sum(axis=1) - got.hist[1].sum(axis=1) <= 2)
    assert int(clean.best_n[1]) == 26 and int(got.best_n[1]) == 27 and got.best_prob[1] == -60.0


# ---- 5. several staged pieces -------------------------------------------------------------------------------------------
def test_several_staged_pieces():
    """a one-mode pulse at 3 abscissae over two full pieces of kept steps and a ragged one, against numpy's sequential
    np.add.accumulate, and the same steps cut elsewhere"""
    n = 2 * PIECE + 1234
    rng = np.random.default_rng(5)
    x = np.array([10.5, 10.6, 10.75])
    rows = np.zeros((n, 1, 6))
    rows[:, 0, :4] = np.array([5.0, 0.05, 10.6, 4.0]) * (1 + 0.02 * rng.standard_normal((n, 4)))
    rows[:, 0, 4] = -rng.uniform(size=n)
    rows[2 * PIECE + 5, 0, 4] = 1.0                           # the best sample lies in the third piece
    s = tiny_sampler(wl.MODEL_PULSE, 4)
    d = on_device(rows)
    s.predict_begin(chains=(0,), x=x, nbins=5, lo=0.0, hi=4.0)
    feed(s, d, [n])
    got = s.predict()
    s.predict_begin(chains=(0,), x=x, nbins=5, lo=0.0, hi=4.0)
    feed(s, d, [PIECE - 3, 5, n - PIECE - 2])
    again = s.predict()
    s.predict_end()
    s.close()
    v = ref.pulse_numpy(rows[:, 0, :4], x)                    # [n][3]
    dlt = v - v[0]
    assert int(got.n[0]) == n and got.origin[0].tobytes() == v[0].tobytes()
    assert got.sum[0].tobytes() == np.add.accumulate(dlt, axis=0)[-1].tobytes()
    assert got.sq[0].tobytes() == np.add.accumulate(dlt * dlt, axis=0)[-1].tobytes()
    assert got.vmin[0].tobytes() == v.min(axis=0).tobytes() and got.vmax[0].tobytes() == v.max(axis=0).tobytes()
    e = ref.edges(0.0, 4.0, 5)
    for i in range(3):
        counts = np.bincount([b for b in (ref.bin_of(t, e) for t in v[:, i].tolist()) if b >= 0], minlength=5)
        assert got.hist[0, i].tolist() == counts.tolist(), i
    assert int(got.best_n[0]) == 2 * PIECE + 6 and got.best_prob[0] == 1.0
    assert got.best_params[0].tobytes() == rows[2 * PIECE + 5, 0, :4].tobytes()
    assert_equals(again, got, "cut elsewhere")


# ---- 6. the histogram extremes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins,lo,hi", [(1, -1.0, 3.0), (4096, -1.0, 3.0), (200, 1e15, 1e15 + 3)],
                         ids=["1", "4096", "unsorted_edges"])
def test_histogram_extremes(nbins, lo, hi):
    """an amplitude of exactly 0 makes the curve the offset, whatever x is: the offsets are every edge of the histogram
    and its two neighbours in fp64, the widened top edge among them.  4096 bins leave one abscissa per workgroup.  Over
    [1e15, 1e15 + 3] GSL's 200 edges are not sorted -- some step back by an ulp -- and the kernel bisects as the host
    does; over [-1, 3] they are, and it walks from a guess to the same bin."""
    e = ref.edges(lo, hi, nbins)
    assert (np.diff(e) > 0).all() == (lo < 1e15)
    pts = np.array(e)
    offsets = np.concatenate([pts, np.nextafter(pts, -np.inf), np.nextafter(pts, np.inf), [lo - 1, hi + 1, (lo + hi) / 2]])
    n = len(offsets)
    rows = np.zeros((n, 1, 6))
    rows[:, 0, :4] = [0.0, 0.2, 0.4, 0.0]
    rows[:, 0, 3] = offsets
    x = np.array([100.0, 100.5, 2.45e6])
    s = tiny_sampler(wl.MODEL_SIMPLESIN, 4)
    d = on_device(rows)
    s.predict_begin(chains=(0,), x=x, nbins=nbins, lo=lo, hi=hi)
    feed(s, d, [n // 3, n - n // 3])
    got = s.predict()
    s.predict_end()
    s.close()
    counts = np.bincount([b for b in (ref.bin_of(v, e) for v in offsets.tolist()) if b >= 0], minlength=nbins)
    assert got.hist.shape == (1, 3, nbins)
    if lo < 1e15:        # of the bottom edge's three one lies below, the top edge and its upper neighbour above
        assert counts.sum() == 3 * nbins + 1
    for i in range(3):
        assert got.hist[0, i].tolist() == counts.tolist(), i
    assert got.vmin[0].tolist() == [lo - 1] * 3 and got.vmax[0].tolist() == [hi + 1] * 3
    assert got.origin[0].tolist() == [offsets[0]] * 3


# ---- 7. a real run between launches -----------------------------------------------------------------------------------------
def test_a_real_run_between_launches():
    n_chain, n_rounds, n_swap, launches = 8, 10, 6, 4
    w = wl.simplesin(n_data=64, n_chain=n_chain)
    st, _, _ = make_pair(w, n_chain, seed=5)
    per = n_rounds * n_swap
    out = []
    for with_fold in (True, False):
        s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=5)
        s.set_state(st)
        d = torch.zeros((launches, per, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
        if with_fold:
            s.predict_begin(chains=(0, 5), nbins=50, lo=-3.0, hi=5.0)
        for k in range(launches):
            s.run_sampler(n_rounds, n_swap, d[k].data_ptr())
            if with_fold:
                s.predict_accumulate(d[k].data_ptr(), per)
        got = s.predict() if with_fold else None
        s.synchronize()
        rows = d.cpu().numpy().reshape(launches * per, n_chain, w.n_par + 2)
        if with_fold:
            d2 = on_device(rows)
            s.predict_begin(chains=(0, 5), nbins=50, lo=-3.0, hi=5.0)
            s.predict_accumulate(d2.data_ptr(), launches * per)
            whole = s.predict()
            s.predict_end()
            assert int(got.n[0]) == launches * per
            assert_equals(got, whole, "interleaved against one call")
            curves = s.predict_curve(rows[:, 5, :w.n_par])
            assert got.vmax[1].tobytes() == curves.max(axis=0).tobytes() and got.origin[1].tobytes() == curves[0].tobytes()
            best = int(np.argmax(rows[:, 0, w.n_par]))
            assert int(got.best_n[0]) == best + 1 and got.best_prob[0] == rows[best, 0, w.n_par]
            assert got.best_curve(s).tobytes() == s.predict_curve(rows[best, 0, :w.n_par]).tobytes()
            assert np.all(got.sd(0) > 0) and np.array_equal(got.residuals(w.data[:, 1]), w.data[:, 1] - got.mean())
            lo68, hi68 = got.band(0.68)
            assert np.all(lo68 <= got.median()) and np.all(got.median() <= hi68)
        out.append((s.get_state(), rows))
        s.close()
    for f in ("params", "prob", "prior", "accept", "reject", "n_iter", "swapcount", "step", "beta"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()


# ---- 8. a ladder batch ----------------------------------------------------------------------------------------------------
def test_a_batch_of_three_ladders():
    """three ladders whose data have different abscissae; x = NULL: every kept chain folds over its own ladder's"""
    from tests.test_gpu_ladder_batch import concat, ladders, make_batch, N_ROUNDS, N_SWAP, PER
    ws, seeds, sts, _, _ = ladders("simplesin", 3)
    for b, w in enumerate(ws):
        w.data[:, 0] += 7.25 * b
    w = ws[0]
    n_steps = N_ROUNDS * N_SWAP
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    d = torch.zeros((n_steps, 3 * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    chains = [0, PER, 2 * PER + 1]
    batch.predict_begin(chains=chains)
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.predict_accumulate(d.data_ptr(), n_steps)
    got = batch.predict()
    rows = d.cpu().numpy()
    assert got.n_ladders == 3 and got.n_x == w.n_data
    lads = got.per_ladder()
    for b in range(3):
        assert got.x[b].tobytes() == ws[b].data[:, 0].tobytes()
        batch.predict_begin(chains=(chains[b],), x=ws[b].data[:, 0])
        batch.predict_accumulate(d.data_ptr(), n_steps)
        assert_equals(lads[b], batch.predict(), "ladder %d" % b)
        curves = batch.predict_curve(rows[:, chains[b], :w.n_par], ws[b].data[:, 0])
        assert got.origin[b].tobytes() == curves[0].tobytes() and got.vmin[b].tobytes() == curves.min(axis=0).tobytes()
    batch.close()
    assert not same_floats(got.x[0], got.x[1])


# ---- 9. predict_set: a resumed run --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [5, 30])
def test_set_resumes_a_fold(sampler5, cut):
    """get, end, begin, set and more samples equal the uninterrupted fold; chain 0's best sample is step 7: behind the
    first cut, ahead of the second"""
    rows, x = hand_rows(), hand_x()
    d = on_device(rows)
    s = sampler5
    kw = dict(chains=HAND_CHAINS, x=x, nbins=HAND_BINS, lo=HAND_LO, hi=HAND_HI)
    s.predict_begin(**kw)
    s.predict_accumulate(d.data_ptr(), HAND_STEPS)
    whole = s.predict()
    s.predict_begin(**kw)
    s.predict_accumulate(d.data_ptr(), cut)
    part = s.predict()
    s.predict_end()
    assert int(part.n[0]) == cut and (int(part.best_n[0]) == 8) == (cut > 7)
    s.predict_begin(**kw)
    s.predict_set(part)
    s.predict_accumulate(d[cut:].data_ptr(), HAND_STEPS - cut)
    got = s.predict()
    s.predict_end()
    assert_equals(got, whole, "resumed at %d" % cut)
    assert int(got.best_n[0]) == 8 and got.origin.tobytes() == part.origin.tobytes()


# ---- 10. invalid arguments ------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    n_chains = 96
    w = wl.simplesin(n_data=64, n_chain=n_chains)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    st, _, _ = make_pair(w, n_chains, seed=1)
    s.set_state(st)
    L = capi.lib()
    d = torch.zeros((12, n_chains, w.n_par + 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    pr = Predict.empty((0,), np.zeros(3), 4, 0)
    assert L.apemost_hip_predict_accumulate(s._h, d.data_ptr(), 12, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_predict_get(s._h, C.byref(pr.view())) == capi.ERR_INVALID
    assert L.apemost_hip_predict_set(s._h, C.byref(pr.view())) == capi.ERR_INVALID
    assert L.apemost_hip_predict_begin(s._h, None) == capi.ERR_INVALID
    ip = C.POINTER(C.c_int32)
    big = np.ones((1 << 20) + 1)

    def begin(chains=(0,), x=(1.0, 2.0, 3.0), n_x=None, nbins=0, lo=0.0, hi=1.0):
        ch = np.array(chains, dtype=np.int32)
        xs = None if x is None else np.ascontiguousarray(x, dtype=np.float64)
        cfg = capi.PredictConfig(n_keep=len(ch), chains=ch.ctypes.data_as(ip) if len(ch) else None,
                                 n_x=(0 if xs is None else len(xs)) if n_x is None else n_x,
                                 x=None if xs is None else xs.ctypes.data_as(capi._dp), nbins=nbins, lo=lo, hi=hi)
        return L.apemost_hip_predict_begin(s._h, C.byref(cfg))
    refused = (dict(chains=()), dict(chains=(0, 0)), dict(chains=(2, 1)), dict(chains=(n_chains,)), dict(chains=(-1,)),
               dict(chains=tuple(range(n_chains + 1))), dict(n_x=0), dict(n_x=-1), dict(x=(1.0, np.nan)),
               dict(x=(np.inf, 1.0)), dict(nbins=-1), dict(nbins=4097), dict(nbins=10, lo=1.0, hi=1.0),
               dict(nbins=10, lo=2.0, hi=1.0), dict(nbins=10, lo=np.nan, hi=1.0), dict(nbins=10, lo=0.0, hi=np.inf),
               dict(x=big),                                                      # 2^20 + 1 series
               dict(chains=(0, 1), x=big[:1 << 19], nbins=65))                   # 2^20 series x 65 bins > 2^26 counts
    for kw in refused:
        assert begin(**kw) == capi.ERR_INVALID, kw
        assert L.apemost_hip_predict_get(s._h, C.byref(pr.view())) == capi.ERR_INVALID, kw    # nothing was begun
    assert begin(chains=(0, 1), x=big[:1 << 19], nbins=64) == capi.OK           # 2^20 series, 2^26 counts: the caps
    assert begin(x=None) == capi.OK and begin(nbins=4096, lo=-1.0, hi=1.0) == capi.OK and begin(nbins=1) == capi.OK
    assert begin() == capi.OK
    assert L.apemost_hip_predict_accumulate(s._h, d.data_ptr(), 12, 0, 0) == capi.ERR_INVALID      # thin 0
    assert L.apemost_hip_predict_accumulate(s._h, None, 12, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_predict_get(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_predict_accumulate(s._h, d.data_ptr(), 12, 12, 1) == capi.OK               # keeps nothing
    assert L.apemost_hip_predict_accumulate(s._h, d.data_ptr(), 12, 2, 3) == capi.OK
    assert L.apemost_hip_predict_get(s._h, C.byref(pr.view())) == capi.OK and int(pr.n[0]) == 4
    assert not pr.sum.any() and pr.best_n[0] == 1             # (rows of zeros: a constant curve, prob 0 > -inf)
    # a begin that is refused leaves the fold begun before open, accumulating as it was
    for kw in refused:
        assert begin(**kw) == capi.ERR_INVALID, kw
    assert L.apemost_hip_predict_begin(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_predict_accumulate(s._h, d.data_ptr(), 12, 0, 4) == capi.OK
    assert L.apemost_hip_predict_get(s._h, C.byref(pr.view())) == capi.OK and int(pr.n[0]) == 7
    s.predict_end()
    assert L.apemost_hip_predict_get(s._h, C.byref(pr.view())) == capi.ERR_INVALID
    out = np.zeros((2, 3))
    par = np.zeros((2, 4))
    curve = L.apemost_hip_predict_curve
    xs = np.array([1.0, 2.0, 3.0])
    assert curve(s._h, 0, par.ctypes.data_as(capi._dp), 3, xs.ctypes.data_as(capi._dp), out.ctypes.data_as(capi._dp)) == capi.ERR_INVALID
    assert curve(s._h, 2, None, 3, xs.ctypes.data_as(capi._dp), out.ctypes.data_as(capi._dp)) == capi.ERR_INVALID
    assert curve(s._h, 2, par.ctypes.data_as(capi._dp), 3, xs.ctypes.data_as(capi._dp), None) == capi.ERR_INVALID
    assert curve(s._h, 2, par.ctypes.data_as(capi._dp), 0, xs.ctypes.data_as(capi._dp), out.ctypes.data_as(capi._dp)) == capi.ERR_INVALID
    assert curve(s._h, 2, par.ctypes.data_as(capi._dp), 3, xs.ctypes.data_as(capi._dp), out.ctypes.data_as(capi._dp)) == capi.OK
    # the sampler still steps
    before = s.get_state()
    s.run_sampler(3, 5, d.data_ptr())
    s.synchronize()
    after = s.get_state()
    assert np.array_equal(after.n_iter, before.n_iter + 15)
    s.close()


def test_a_user_model_has_no_curve():
    rs = np.random.RandomState(5)
    data = np.column_stack([(rs.uniform(size=64) < 0.5).astype(float), rs.normal(0, 1, (64, 2))])
    s = HipSampler(wl.MODEL_USER, 3, 5, data, seed=1,
                   device_model_source=os.path.join(hostlib.HOST, "examples", "device_models", "bernoulli_example.hip"))
    L = capi.lib()
    ch = np.zeros(1, dtype=np.int32)
    cfg = capi.PredictConfig(n_keep=1, chains=ch.ctypes.data_as(C.POINTER(C.c_int32)), n_x=0, x=None, nbins=0, lo=0.0, hi=0.0)
    pr = Predict.empty((0,), np.zeros(64), 3, wl.MODEL_USER)
    d = torch.zeros((4, 5, 5), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    out, par = np.zeros((1, 64)), np.zeros((1, 3))
    assert L.apemost_hip_predict_begin(s._h, C.byref(cfg)) == capi.ERR_UNSUPPORTED
    assert b"user" in L.apemost_hip_last_error()
    assert L.apemost_hip_predict_accumulate(s._h, d.data_ptr(), 4, 0, 1) == capi.ERR_UNSUPPORTED
    assert L.apemost_hip_predict_get(s._h, C.byref(pr.view())) == capi.ERR_UNSUPPORTED
    assert L.apemost_hip_predict_set(s._h, C.byref(pr.view())) == capi.ERR_UNSUPPORTED
    assert L.apemost_hip_predict_end(s._h) == capi.ERR_UNSUPPORTED
    assert L.apemost_hip_predict_curve(s._h, 1, par.ctypes.data_as(capi._dp), 0, None,
                                       out.ctypes.data_as(capi._dp)) == capi.ERR_UNSUPPORTED
    s.close()


# ---- 11. beside the other folds -------------------------------------------------------------------------------------------
def test_beside_the_other_folds():
    """summary, peaks, joint, evidence, autocorrelation and predict open on the same rows: each equals what it gives alone"""
    from tests.test_gpu_summary import _run
    w, s, d, _ = _run("simplesin16")
    n_steps = d.shape[0]
    pieces = [(0, 100), (100, n_steps - 100)]
    nb = batches_closed(n_steps, 7)
    names = ["summary", "peaks", "joint", "evidence", "autocorr", "predict"]

    def begin(which):
        if "summary" in which:
            s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=7, max_batches=nb)
        if "peaks" in which:
            s.peaks_begin(w.pmin, w.pmax, chains=(0, 2), capacity=n_steps)
        if "joint" in which:
            s.joint_begin(w.pmin, w.pmax, chains=(0, 2), nbins=64)
        if "evidence" in which:
            s.evidence_begin(batch_size=7, max_batches=nb)
        if "autocorr" in which:
            s.autocorr_begin(chains=(0, 2), max_lag=50)
        if "predict" in which:
            s.predict_begin(chains=(0, 2), nbins=40, lo=-1.0, hi=2.0)
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
    assert_equals(every["predict"], alone["predict"], "beside the others")
    assert int(every["predict"].n[0]) == n_steps and every["predict"].hist.sum() > 0
    assert np.array_equal(every["summary"].hist, alone["summary"].hist)
    assert every["summary"].prob_sum.tobytes() == alone["summary"].prob_sum.tobytes()
    assert every["summary"].batch_sums.tobytes() == alone["summary"].batch_sums.tobytes()
    for f in ("n_values", "n_peaks", "left", "right", "q", "q_set"):
        assert getattr(every["peaks"], f).tobytes() == getattr(alone["peaks"], f).tobytes(), f
    assert np.array_equal(every["joint"].counts, alone["joint"].counts)
    for f in ("origin", "sum", "cross"):
        assert getattr(every["joint"], f).tobytes() == getattr(alone["joint"], f).tobytes(), f
    for f in ("origin", "sum", "sq", "batch", "m", "S"):
        assert getattr(every["evidence"], f).tobytes() == getattr(alone["evidence"], f).tobytes(), f
    for f in ("origin", "sum", "lag", "head", "tail"):
        assert getattr(every["autocorr"], f).tobytes() == getattr(alone["autocorr"], f).tobytes(), f


# ---- 12. the C host: APEMOST_DUMP=binary,predict ----------------------------------------------------------------------------
def test_c_host_predict_token(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters = 8, 3000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    runs = {}
    for mode in ("binary,predict", "predict"):
        work = tmp_path / mode.replace(",", "_")
        work.mkdir()
        (work / "params").write_text(w.params_file_text())
        (work / "data").write_text(w.data_file_text())
        env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP=mode)
        if mode != "predict":
            env.update(APEMOST_PREDICT_BINS="60", APEMOST_PREDICT_RANGE="-1.5:2.5")
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
        runs[mode] = (work, env)
    work, env = runs["binary,predict"]
    _, params, probs = samples_bin.read(str(work / "samples.bin"))       # [iters][1][n_par], [iters][n_beta][2]
    rows = np.zeros((iters, 1, w.n_par + 2))
    rows[:, 0, :w.n_par] = params[:, 0]
    rows[:, 0, w.n_par:] = probs[:, 0]
    got = Predict.read(str(work / "predict.bin"))
    assert (got.n_keep, got.n_x, got.nbins, got.n_par, got.thin, got.n_ladders, got.model) == (1, 128, 60, w.n_par, 1, 1, 0)
    assert (got.lo, got.hi) == (-1.5, 2.5) and got.chains.tolist() == [0]
    data = np.loadtxt(str(work / "data"))                     # what the host parsed
    assert got.x[0].tobytes() == data[:, 0].tobytes()
    s = HipSampler(w.model, w.n_par, 1, data, seed=1)
    d = on_device(rows)
    s.predict_begin(chains=(0,), nbins=60, lo=-1.5, hi=2.5)
    s.predict_accumulate(d.data_ptr(), iters)
    mine = s.predict()
    s.predict_end()
    assert_equals(got, mine, "the C host")
    best = s.predict_curve(got.best_params[0])
    s.close()
    text = (work / "predict.txt").read_text()
    assert text == got.text(data[:, 1], best)
    cols = np.array([[float(v) for v in ln.split("\t")] for ln in text.split("\n")[:-1]])
    assert cols.shape == (128, 11)
    for c, want in enumerate([got.x[0], data[:, 1], got.mean(), got.sd(), data[:, 1] - got.mean(), got.vmin[0], got.vmax[0],
                              best, got.median(), got.band(0.68)[0], got.band(0.68)[1]]):
        assert cols[:, c].tolist() == [float("%.15e" % v) for v in want], c
    # alone the token writes no sample file and, without both variables, no histograms
    only, _ = runs["predict"]
    assert not [f for f in os.listdir(str(only)) if f.endswith(".prob.dump") or f.startswith("prob-chain") or f == "samples.bin"]
    plain = Predict.read(str(only / "predict.bin"))
    assert plain.nbins == 0 and len((only / "predict.txt").read_text().split("\n")[0].split("\t")) == 8
    for f in ("origin", "sum", "sq", "vmin", "vmax", "best_prob", "best_params", "best_n"):
        assert getattr(plain, f).tobytes() == getattr(got, f).tobytes(), f
    # --append resumes from the file; another range cannot
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = Predict.read(str(work / "predict.bin"))
    assert int(second.n[0]) == 2 * iters and second.origin.tobytes() == got.origin.tobytes()
    env_other = dict(env, APEMOST_PREDICT_BINS="61")
    assert subprocess.call([exe, "run", "--append"], cwd=str(work), env=env_other, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL, timeout=300) != 0
    bad = dict(env, APEMOST_DUMP="binary,predic")
    assert subprocess.call([exe, "run"], cwd=str(work), env=bad, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           timeout=300) != 0
