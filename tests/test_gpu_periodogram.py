"""On-device residual periodogram (apemost_hip_periodogram_*, apemost_amd/csrc/pt_periodogram.h) on synthetic rows
uploaded to the device.

The comparison rule.  apemost_hip_periodogram_values is the stated meaning.  Its r is held bit for bit to y - v with v from
apemost_hip_predict_curve; its c and s to mpmath's sine of the rounded argument fl(kTwoPi u) at 50 digits, u = fl(nu x)
and fl(u + 0.25), within the absolute bound tests/sine_domain.py states for the device sine (SIN_CW_ABS_ERR, 3.604e-16);
its C, S, P, peak and arg bit for bit to tests/periodogram_ref.py (exact fused multiply-adds) over the device's own r, c
and s.  The fold is held to the sequential loop of tests/periodogram_ref.py over values' C, S and P of the kept rows:
every word and count compares with == on the bits, a NaN by its position."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from apemost_amd import capi, periodogram as pg, workloads as wl
from apemost_amd.sampler import HipSampler
from tests import hostlib
from tests import periodogram_ref as ref

pytestmark = pytest.mark.gpu

SHAPES = [(wl.MODEL_SIMPLESIN, 4), (wl.MODEL_SINE3, 10)]
N_FOLD = 21          # kept samples: no multiple of the 8 a wave holds side by side, nor of a workgroup's 32
WORDS = pg.STATE + pg.PEAK_STATE + ("exceed", "peak_counts")
NAN, INF = math.nan, math.inf


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """== on the bits, a NaN by its position"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def case(model, n_par, n, n_chains, n_data, seed=0):
    """n steps of n_chains chains around the workloads' starting points and n_data data the curve comes near
    (tests/test_gpu_check.py::case for the sine models)"""
    rng = np.random.default_rng(100 + 10 * model + seed)
    rows = np.zeros((n, n_chains, n_par + 2))
    start = np.array([0.9, 0.2, 0.4, 0.5] if n_par == 4 else [0.9, 0.2, 0.4, 0.54, 0.11, 0.1, 0.27, 0.27, 0.7, 0.5])
    scale = 0.02 * np.array([1, 1e-3, 1, 1] if n_par == 4 else [1, 1e-3, 1] * 3 + [1])
    rows[:, :, :n_par] = start + scale * rng.standard_normal((n, n_chains, n_par))
    data = np.stack([100 + 0.5 * np.arange(n_data), rng.uniform(-1, 2, n_data)], 1)
    return rows, data


def grid(n_freq, seed=0):
    """n_freq frequencies in no order, 0 and a negative one among them, and weights [n_freq][3] of both signs"""
    rng = np.random.default_rng(7 + seed)
    freqs = rng.uniform(0.01, 0.95, n_freq)
    if n_freq > 2:
        freqs[1], freqs[2] = 0.0, -0.31
    return freqs, rng.standard_normal((n_freq, 3))


def feed(s, d, calls, skip0=0, thin=1):
    """accumulate d in calls of the given numbers of steps; the kept steps are skip0, skip0 + thin, ... of the whole"""
    off = 0
    for n in calls:
        skip = skip0 - off if off < skip0 else (thin - (off - skip0) % thin) % thin
        s.periodogram_accumulate(d[off:].data_ptr(), n, skip, thin)
        off += n
    assert off == d.shape[0]


def fold(s, rows, chains, freqs, w, level=INF, calls=None, skip0=0, thin=1):
    d = on_device(rows)
    s.periodogram_begin(chains=chains, freqs=freqs, weights=w, level=level, thin=thin)
    feed(s, d, calls or [len(rows)], skip0, thin)
    got = s.periodogram()
    s.periodogram_end()
    return got


class Reference:
    """the sequential loop over values' C, S, P, peak and arg of the kept rows [n][n_chains][n_par + 2]: per kept chain
    the series' words [n_freq] and the peak's words"""

    def __init__(self, s, kept, chains, mats, freqs, w, level):
        n_par = kept.shape[2] - 2
        self.n = len(kept)
        self.series, self.peak, self.P = [], [], []
        w = np.broadcast_to(w, (len(chains),) + np.shape(w)[-2:])
        level = np.broadcast_to(np.asarray(level, dtype=np.float64), (len(chains),))
        for k, (c, mat) in enumerate(zip(chains, mats)):
            par = np.ascontiguousarray(kept[:, c, :n_par])
            v = s.periodogram_values(par, mat[:, 0], mat[:, 1], freqs, w[k])
            self.series.append([ref.RefSeries(v["P"][:, j], v["C"][:, j], v["S"][:, j], level[k]) for j in range(len(freqs))])
            self.peak.append(ref.RefPeak(v["peak"], v["arg"], len(freqs)))
            self.P.append(v["P"])


def check_kept_chain(got, k, r, rk, what):
    """kept chain k of the Periodogram `got` against kept chain rk of the Reference r: == on the bits"""
    assert int(got.n[0]) == r.n, (what, int(got.n[0]), r.n)
    series, pk = r.series[rk], r.peak[rk]
    for f, name in zip(pg.STATE, ("origin", "sum", "sq", "min", "max", "sum_c", "sum_s")):
        want = np.array([getattr(q, name) for q in series], dtype=np.float64)
        assert same_bits(getattr(got, f)[k], want), (what, k, f, getattr(got, f)[k], want)
    assert got.exceed[k].tolist() == [q.exceed for q in series], (what, k, "exceed")
    for f, name in zip(pg.PEAK_STATE, ("origin", "sum", "sq", "min", "max")):
        assert same_bits(getattr(got, f)[k], getattr(pk, name)), (what, k, f, getattr(got, f)[k], getattr(pk, name))
    assert got.peak_counts[k].tolist() == pk.counts.tolist(), (what, k, "peak_counts")


def assert_same(a, b, what):
    assert int(a.n[0]) == int(b.n[0]), what
    for f in WORDS:
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (what, f)


# ---- 1. values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n_par", SHAPES)
def test_values(model, n_par):
    mpmath = pytest.importorskip("mpmath")
    from tests import sine_domain
    mp = mpmath.mp.clone()              # (a context of its own: other tests' precision stays what it was)
    mp.dps = 50
    s = HipSampler(model, n_par, 1, case(model, n_par, 1, 1, 4)[1], seed=1, sigma=0.37)
    worst = 0.0
    for n_data, n_freq in ((1, 1), (2, 65), (63, 64), (64, 63), (65, 2), (130, 130)):
        rows, data = case(model, n_par, 3, 1, n_data, seed=n_data)
        par = np.ascontiguousarray(rows[:, 0, :n_par])
        x, y = np.ascontiguousarray(data[:, 0]), np.ascontiguousarray(data[:, 1])
        freqs, w = grid(n_freq, seed=n_data)
        if n_freq > 3:
            freqs[3] = 1e12             # 2 pi nu x leaves the sine's range: NaN c and s, and NaN C, S, P at that frequency
            w[0] = w[4 % n_freq]        # (and two frequencies share their weights)
        v = s.periodogram_values(par, x, y, freqs, w)
        assert v["r"].shape == (3, n_data) and v["c"].shape == v["s"].shape == (n_freq, n_data)
        assert v["C"].shape == v["S"].shape == v["P"].shape == (3, n_freq) and v["arg"].dtype == np.int32
        assert same_bits(v["r"], y[None] - s.predict_curve(par, x))
        for j in range(n_freq):
            inside = [ref.in_range(freqs[j], xi) for xi in x]
            assert np.isnan(v["c"][j]).tolist() == np.isnan(v["s"][j]).tolist() == [not ok for ok in inside], j
            if j == 3:
                assert not any(inside)
            for i in np.flatnonzero(inside)[:: max(1, n_data // 8)]:
                u = np.float64(freqs[j]) * x[i]
                for got, uu in ((v["s"][j, i], u), (v["c"][j, i], u + np.float64(0.25))):
                    want = mp.sin(mp.mpf(float(np.float64(ref.TWO_PI) * uu)))
                    worst = max(worst, float(abs(mp.mpf(float(got)) - want)))
        assert worst <= sine_domain.SIN_CW_ABS_ERR, worst
        for t in range(3):
            Cw, Sw, Pw, m, arg = ref.row(v["r"][t], v["c"], v["s"], w)
            assert same_bits(v["C"][t], Cw) and same_bits(v["S"][t], Sw) and same_bits(v["P"][t], Pw), (n_data, n_freq, t)
            assert same_bits(v["peak"][t], m) and int(v["arg"][t]) == arg, (n_data, n_freq, t, v["peak"][t], m, v["arg"][t], arg)
    print("worst error of c and s against mpmath: %.4g (bound %.4g)" % (worst, sine_domain.SIN_CW_ABS_ERR))
    s.close()


def test_values_ties_and_rows_without_a_peak():
    """equal weights and frequencies give equal P: the first index wins; a NaN parameter row has no peak"""
    model, n_par = wl.MODEL_SIMPLESIN, 4
    rows, data = case(model, n_par, 2, 1, 70)
    s = HipSampler(model, n_par, 1, data, seed=1)
    par = np.ascontiguousarray(rows[:, 0, :n_par])
    par[1, 0] = NAN
    freqs = np.array([0.3] * 67 + [0.2] * 3)
    freqs[5] = 0.77
    w = np.tile([1.0, 0.0, 1.0], (70, 1))
    v = s.periodogram_values(par, data[:, 0], data[:, 1], freqs, w)
    P = v["P"][0]
    first = int(np.flatnonzero(P == P.max())[0])
    assert (P == P.max()).sum() > 1 and int(v["arg"][0]) == first and v["peak"][0] == P.max()
    assert np.isnan(v["P"][1]).all() and int(v["arg"][1]) == 70 and v["peak"][1] == -INF
    s.close()


# ---- 2. the fold against the sequential loop --------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n_par", SHAPES)
@pytest.mark.parametrize("L,n_freq", [(1, 1), (63, 63), (64, 64), (65, 65), (130, 130), (1, 130), (130, 1)])
def test_fold_against_the_sequential_loop(model, n_par, L, n_freq):
    rows, data = case(model, n_par, N_FOLD, 3, L, seed=L + n_freq)
    freqs, w = grid(n_freq, seed=L)
    s = HipSampler(model, n_par, 3, data, seed=1)
    probe = Reference(s, rows, [0], [data], freqs, w, INF).P[0]
    level = float(np.median(probe[np.isfinite(probe)]))             # about half of the P lie above it, and one P is it
    r = Reference(s, rows, [0, 2], [data, data], freqs, w, level)
    got = fold(s, rows, [0, 2], freqs, w, level)
    for k in range(2):
        check_kept_chain(got, k, r, k, "L %d, n_freq %d" % (L, n_freq))
    assert sum(q.exceed for q in r.series[0]) > 0 and got.lengths.tolist() == [L, L]
    # the same rows in calls of 1, 7 and the rest; a kept chain alone; skip and thin
    assert_same(fold(s, rows, [0, 2], freqs, w, level, calls=[1, 7, N_FOLD - 8]), got, "calls of 1, 7 and the rest")
    alone = fold(s, rows, [2], freqs, w, level)
    for f in WORDS:
        assert getattr(alone, f)[0].tobytes() == getattr(got, f)[1].tobytes(), f
    thinned = fold(s, rows, [0, 2], freqs, w, level, calls=[4, 9, N_FOLD - 13], skip0=2, thin=3)
    assert_same(thinned, fold(s, rows[2::3], [0, 2], freqs, w, level), "skip 2, thin 3")
    s.close()


def test_the_piece_boundary():
    """PIECE + 3 kept samples at L = 5 and n_freq = 3: the second piece goes on where the first ended"""
    model, n_par = wl.MODEL_SIMPLESIN, 4
    n = pg.PIECE + 3
    rows, data = case(model, n_par, n, 1, 5)
    freqs, w = np.array([0.3, 0.05, 0.62]), np.array([[1.0, 0.0, 1.0], [0.5, -0.2, 2.0], [1.0, 0.3, 1.0]])
    s = HipSampler(model, n_par, 1, data, seed=1)
    r = Reference(s, rows, [0], [data], freqs, w, 1.0)
    got = fold(s, rows, [0], freqs, w, 1.0)
    check_kept_chain(got, 0, r, 0, "PIECE + 3")
    assert_same(fold(s, rows, [0], freqs, w, 1.0, calls=[pg.PIECE - 1, 2, 2]), got, "calls across the piece")
    s.close()


# ---- 3. other properties ------------------------------------------------------------------------------------------------------
def test_a_nan_row_stays_in_its_kept_chain_and_get_set_resumes():
    model, n_par = wl.MODEL_SINE3, 10
    rows, data = case(model, n_par, N_FOLD, 3, 65)
    freqs, w = grid(66)
    bad = rows.copy()
    bad[4, 1, 3] = NAN
    s = HipSampler(model, n_par, 3, data, seed=1)
    level = np.array([0.5, INF, -INF])
    got = fold(s, bad, [0, 1, 2], freqs, w, level)
    clean = fold(s, rows, [0, 1, 2], freqs, w, level)
    for f in WORDS:
        assert getattr(got, f)[[0, 2]].tobytes() == getattr(clean, f)[[0, 2]].tobytes(), f
    assert np.isnan(got.sum[1]).all() and not np.isnan(got.pmax[1]).any() and got.n_no_peak(1) == 1
    assert got.peak_min[1] == -INF and got.exceed[1].sum() == 0 and got.exceed[2].tolist() == [N_FOLD] * 66
    r = Reference(s, bad, [0, 1, 2], [data] * 3, freqs, w, level)
    for k in range(3):
        check_kept_chain(got, k, r, k, "a NaN row in kept chain 1")
    # get -> end -> begin -> set -> more accumulates
    d = on_device(bad)
    s.periodogram_begin(chains=[0, 1, 2], freqs=freqs, weights=w, level=level)
    s.periodogram_accumulate(d.data_ptr(), 9)
    half = s.periodogram()
    s.periodogram_end()
    s.periodogram_begin(chains=[0, 1, 2], freqs=freqs, weights=w, level=level)
    s.periodogram_set(half)
    s.periodogram_accumulate(d[9:].data_ptr(), N_FOLD - 9)
    resumed = s.periodogram()
    s.periodogram_end()
    assert int(half.n[0]) == 9
    assert_same(resumed, got, "get, end, begin, set, accumulate")
    s.close()


# ---- 4. batches and refusals --------------------------------------------------------------------------------------------------
def test_a_ragged_batch():
    """two ladders of 2 chains over 65 and 3 data: per ladder the stand-alone sampler's bytes, with the weights of each
    ladder's own abscissae"""
    model, n_par, per, lens = wl.MODEL_SIMPLESIN, 4, 2, (65, 3)
    rows, data = case(model, n_par, N_FOLD, 2 * per, 130)
    sets = [data[10 * b:10 * b + n] for b, n in enumerate(lens)]
    freqs = np.linspace(0.05, 0.9, 9)
    chains = [1, per]
    s = HipSampler.batch(model, n_par, per, sets, [1, 2])
    d = on_device(rows)
    s.periodogram_begin(chains=chains, freqs=freqs, kind="lomb_scargle", level=2.0)
    s.periodogram_accumulate(d.data_ptr(), N_FOLD)
    got = s.periodogram()
    s.periodogram_end()
    s.close()
    assert got.lengths.tolist() == list(lens) and got.n_ladders == 2
    for b, (one, c) in enumerate(zip(got.per_ladder(), chains)):
        assert one.weights[0].tobytes() == pg.weights(sets[b][:, 0], freqs, "lomb_scargle", 0.5).tobytes()
        alone = HipSampler(model, n_par, per, sets[b], seed=1)
        da = on_device(rows[:, b * per:(b + 1) * per])
        alone.periodogram_begin(chains=[c - b * per], freqs=freqs, level=2.0)
        alone.periodogram_accumulate(da.data_ptr(), N_FOLD)
        want = alone.periodogram()
        alone.periodogram_end()
        alone.close()
        assert_same(one, want, "ladder %d" % b)
        assert one.lengths.tolist() == [lens[b]] and len(one.text().splitlines()) == 9


def test_refusals():
    model, n_par = wl.MODEL_SIMPLESIN, 4
    rows, data = case(model, n_par, 4, 3, 5)
    s = HipSampler(model, n_par, 3, data, seed=1)
    L = capi.lib()
    ip, dp = C.POINTER(C.c_int32), capi._dp
    d = on_device(rows)
    freqs, w, level = np.array([0.1, 0.2]), np.ones((1, 2, 3)), np.array([1.0])
    ch = np.array([0], dtype=np.int32)
    view = pg.Periodogram.empty([0], freqs, w, level, [5]).view()
    lens = np.zeros(1, dtype=np.int32)

    def begin(n_freq=2, f=freqs, ww=w, lv=level, chains=ch):
        return L.apemost_hip_periodogram_begin(s._h, len(chains), chains.ctypes.data_as(ip), n_freq,
                                               None if f is None else f.ctypes.data_as(dp),
                                               None if ww is None else ww.ctypes.data_as(dp),
                                               None if lv is None else lv.ctypes.data_as(dp))

    def refused(rc, text):
        assert rc == capi.ERR_INVALID and text in L.apemost_hip_last_error(), (rc, L.apemost_hip_last_error())
    # nothing was begun
    refused(L.apemost_hip_periodogram_accumulate(s._h, d.data_ptr(), 4, 0, 1), b"no periodogram_begin")
    for call in (L.apemost_hip_periodogram_get, L.apemost_hip_periodogram_set):
        refused(call(s._h, C.byref(view)), b"no periodogram_begin")
    refused(L.apemost_hip_periodogram_lengths(s._h, lens.ctypes.data_as(ip)), b"no periodogram_begin")
    # chains, the grid, and a NaN anywhere
    for bad in ([3], [-1], [1, 1], [2, 0]):
        refused(begin(chains=np.array(bad, dtype=np.int32), ww=np.ones((2, 2, 3)), lv=np.ones(2)), b"periodogram_begin")
    for n_freq in (0, -1, (1 << 20) + 1):
        refused(begin(n_freq=n_freq), b"n_freq")
    refused(begin(f=None), b"freqs is NULL")
    refused(begin(ww=None), b"weights is NULL")
    refused(begin(lv=None), b"level is NULL")
    refused(begin(f=np.array([0.1, NAN])), b"freqs[1] is NaN")
    bad = w.copy()
    bad[0, 1, 2] = NAN
    refused(begin(ww=bad), b"weights[0][1][2] is NaN")
    refused(begin(lv=np.array([NAN])), b"level[0] is NaN")
    refused(L.apemost_hip_periodogram_get(s._h, C.byref(view)), b"no periodogram_begin")     # a refused begin begins nothing
    ok = w.copy()
    ok[0, 0, 0], ok[0, 1, 1] = INF, -INF                            # a non-finite weight other than NaN is allowed
    assert begin(f=np.array([INF, -0.0]), ww=ok, lv=np.array([-INF])) == capi.OK
    refused(L.apemost_hip_periodogram_accumulate(s._h, d.data_ptr(), 4, 0, 0), b"bad arguments")      # thin 0
    refused(L.apemost_hip_periodogram_get(s._h, None), b"view is NULL")
    assert L.apemost_hip_periodogram_lengths(s._h, lens.ctypes.data_as(ip)) == capi.OK and lens.tolist() == [5]
    assert L.apemost_hip_periodogram_accumulate(s._h, d.data_ptr(), 4, 0, 1) == capi.OK
    assert L.apemost_hip_periodogram_get(s._h, C.byref(view)) == capi.OK
    assert L.apemost_hip_periodogram_end(s._h) == capi.OK
    refused(L.apemost_hip_periodogram_accumulate(s._h, d.data_ptr(), 4, 0, 1), b"no periodogram_begin")       # ended
    # values
    par = np.ascontiguousarray(rows[:2, 0, :n_par])
    x, y = np.ascontiguousarray(data[:, 0]), np.ascontiguousarray(data[:, 1])
    v = s.periodogram_values(par, x, y, freqs, w[0])                # needs no fold
    assert v["P"].shape == (2, 2)
    with pytest.raises(capi.ApemostHipError, match="NaN"):
        s.periodogram_values(par, x, y, [0.1, NAN], w[0])
    with pytest.raises(ValueError):
        s.periodogram_values(par, x, y[:3], freqs, w[0])
    with pytest.raises(ValueError):
        s.periodogram_values(par, x, y, freqs, w[0][:1])
    with pytest.raises(ValueError):
        s.periodogram_begin(freqs=freqs, weights=np.ones((2, 2)))
    with pytest.raises(ValueError):
        s.periodogram_begin()
    s.close()


def test_pulse_and_user_models_are_refused_and_the_sampler_stays_usable():
    w = wl.pulse(n_data=64, n_chain=4)
    s = HipSampler(w.model, w.n_par, 4, w.data, seed=1)
    freqs = np.array([0.1, 0.2])
    with pytest.raises(capi.ApemostHipError, match="power spectrum") as e:
        s.periodogram_begin(chains=(0,), freqs=freqs)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ApemostHipError, match="power spectrum") as e:
        s.periodogram_values(w.start, w.data[:4, 0], w.data[:4, 1], freqs, np.ones((2, 3)))
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert s.predict_curve(w.start, w.data[:4, 0]).shape == (4,)
    s.close()
    rs = np.random.RandomState(5)
    data = np.column_stack([(rs.uniform(size=64) < 0.5).astype(float), rs.normal(0, 1, (64, 2))])
    s = HipSampler(wl.MODEL_USER, 3, 5, data, seed=1,
                   device_model_source=os.path.join(hostlib.HOST, "examples", "device_models", "bernoulli_example.hip"))
    with pytest.raises(capi.ApemostHipError, match="user-supplied") as e:
        s.periodogram_begin(chains=(0,), freqs=freqs)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ApemostHipError, match="user-supplied") as e:
        s.periodogram_values(np.zeros(3), data[:4, 0], data[:4, 1], freqs, np.ones((2, 3)))
    assert e.value.code == capi.ERR_UNSUPPORTED
    s.calc_model(0, 5)
    s.synchronize()
    s.close()


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------
E2E_FREQS = 0.05 + 0.0125 * np.arange(73)
E2E_NU = 0.615       # the grid point nearest is 0.6125; outside the model's prior on its frequency, [0, 0.3]


def real_run(inject):
    """310 steps of a simplesin ladder of 64 chains over 128 data (config 2's shape cut down), chain 0 folded.  With
    `inject` the data carry a second sinusoid of amplitude 5 sigma = 2.5 at E2E_NU that the model lacks.  On the CPU
    oracle's trajectory of this seed the Lomb-Scargle power of chain 0's residuals peaks at 0.6125 in every sample with
    at least 767 against 38 anywhere else; without the injection it stays below 4.7 at every frequency."""
    from tests.helpers import make_pair
    w = wl.simplesin(n_data=128, n_chain=64)
    if inject:
        w.data[:, 1] += 2.5 * np.sin(2 * np.pi * (E2E_NU * w.data[:, 0] + 0.3))
    st, _, _ = make_pair(w, 64, seed=11, init_prob=True)
    s = HipSampler(w.model, w.n_par, 64, w.data, seed=11)
    s.set_state(st)
    d = torch.zeros((310, 64, 6), dtype=torch.float64, device="cuda")
    s.periodogram_begin(chains=(0,), freqs=E2E_FREQS, kind="lomb_scargle", level=-math.log(0.01 / len(E2E_FREQS)))
    s.run_sampler(10, 31, d.data_ptr())
    s.periodogram_accumulate(d.data_ptr(), 310)
    got = s.periodogram()
    s.periodogram_end()
    s.close()
    assert int(got.n[0]) == 310
    return got


def test_a_real_run_finds_the_frequency_the_model_lacks():
    got = real_run(True)
    nu, share = got.peak_frequency()
    assert nu == 0.05 + 0.0125 * 45 and share == 1.0, (nu, share)
    assert got.peak_mean() > 500 and got.exceed_fraction()[45] == 1.0 and int(np.argmax(got.coherent())) == 45
    assert got.coherent()[45] > 500


def test_a_real_run_without_the_signal_exceeds_nowhere():
    got = real_run(False)
    assert not got.exceed_fraction().any(), got.exceed_fraction()
    assert got.max().max() < -math.log(0.01 / len(E2E_FREQS))


# ---- 6. a sharded ladder ---------------------------------------------------------------------------------------------------------
def test_the_owning_shard_runs_the_fold():
    """a ladder of 4 chains as two shards of 2: each shard folds the kept chains it owns, under their local indices, and
    Periodogram.concat of the shards' folds is the whole ladder's fold of the same rows"""
    model, n_par = wl.MODEL_SIMPLESIN, 4
    rows, data = case(model, n_par, N_FOLD, 4, 65)
    freqs, w = grid(9)
    whole = HipSampler(model, n_par, 4, data, seed=1)
    want = fold(whole, rows, [0, 3], freqs, w, 0.5)
    whole.close()
    parts = []
    for lo, local in ((0, 0), (2, 1)):
        s = HipSampler(model, n_par, 2, data, seed=1, chain_offset=lo, n_chains_global=4)
        parts.append(fold(s, rows[:, lo:lo + 2], [local], freqs, w, 0.5))
        s.close()
    got = pg.Periodogram.concat(parts)
    assert got.chains.tolist() == [0, 1] and got.n_keep == 2
    assert_same(got, want, "two shards")
