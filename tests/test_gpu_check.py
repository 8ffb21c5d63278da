"""On-device predictive checks (apemost_hip_check_*, apemost_amd/csrc/pt_check.h) on synthetic rows uploaded to the device.

The comparison rule.  apemost_hip_check_values is the stated meaning: e, u and the three T of a parameter row.  Its e is
held bit for bit to (y - v) * (1.0 / sigma), respectively y / v, with v from apemost_hip_predict_curve; its u to mpmath's
0.5 erfc(-e / sqrt 2), respectively -expm1(-e), evaluated at the device's e at 50 digits, to 1e-12 absolute: u <= 1, so
any fp64 library error of up to 2^10 ulp stays below 1.2e-13, while an fp32 evaluation or a wrong scale is off by
>= 1e-8; its T to tests/check_ref.py over the device's e and u, bit for bit.

The fold is held to tests/check_ref.py over check_values' e and u and pointwise_loglike_at's l of the same rows:
origin, sum, sq, sum_u and m, and every word, minimum, maximum and count of the statistics, are sequences of IEEE
operations and compare with == on the bits, a NaN by its position.  S and SU carry the device's exp and are held to the
rule tests/test_gpu_pointwise.py holds S_dn to: n 2^-50 relative against math.fsum of the reference's exponentials about
the final maximum (for SU of u times them; its one extra product adds half an ulp a step and stays under the same
n 2^-50, since a step then carries at most 2.5 of the 4 half-ulps the rule allows).  m and S are also compared with a
pointwise fold's m_dn and S_dn on the same rows, byte for byte."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from apemost_amd import capi, check as ck, workloads as wl
from apemost_amd.pointwise import PIECE
from apemost_amd.sampler import HipSampler
from apemost_amd.state import ALL_FIELDS
from tests import check_ref as ref
from tests import hostlib

pytestmark = pytest.mark.gpu

SINE = (wl.MODEL_SIMPLESIN, wl.MODEL_SINE3)
SHAPES = [(wl.MODEL_SIMPLESIN, 4), (wl.MODEL_SINE3, 10), (wl.MODEL_PULSE, 6), (wl.MODEL_PULSE_VROT, 7)]
EXACT = ("origin", "sum", "sq", "sum_u", "m")
CACHE = {}


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


def feed(s, d, calls, skip0=0, thin=1, also=None):
    """accumulate d in calls of the given numbers of steps; the kept steps are skip0, skip0 + thin, ... of the whole"""
    off = 0
    for n in calls:
        skip = skip0 - off if off < skip0 else (thin - (off - skip0) % thin) % thin
        s.check_accumulate(d[off:].data_ptr(), n, skip, thin)
        if also:
            also(d[off:].data_ptr(), n, skip, thin)
        off += n
    assert off == d.shape[0]


def fold(s, rows, chains, edges=None, calls=None, skip0=0, thin=1, nbins=256):
    d = on_device(rows)
    s.check_begin(chains=chains, edges=edges, thin=thin, nbins=nbins)
    feed(s, d, calls or [len(rows)], skip0, thin)
    got = s.check()
    s.check_end()
    return got


def case(model, n_par, n, n_chains, n_data, seed=0):
    """n steps of n_chains chains around the workloads' starting points and n_data data the curve comes near"""
    rng = np.random.default_rng(100 + 10 * model + seed)
    rows = np.zeros((n, n_chains, n_par + 2))
    if model in SINE:
        start = np.array([0.9, 0.2, 0.4, 0.5] if n_par == 4 else [0.9, 0.2, 0.4, 0.54, 0.11, 0.1, 0.27, 0.27, 0.7, 0.5])
        scale = 0.02 * np.array([1, 1e-3, 1, 1] if n_par == 4 else [1, 1e-3, 1] * 3 + [1])
        rows[:, :, :n_par] = start + scale * rng.standard_normal((n, n_chains, n_par))
        data = np.stack([100 + 0.5 * np.arange(n_data), rng.uniform(-1, 2, n_data)], 1)
    else:
        base = np.array([5.0, 0.05, 10.6, 4.0, 11.3, 2.5] if n_par == 6 else [5.0, 0.05, 0.05, 10.6, 4.0, 11.3, 2.5])
        rows[:, :, :n_par] = base * (1 + 0.1 * rng.uniform(size=(n, n_chains, n_par)))
        data = np.stack([np.linspace(10, 12, n_data) if n_data > 1 else np.array([10.7]), rng.exponential(1.0, n_data)], 1)
    return rows, data


class Reference:
    """check_ref over the device's e, u and l of the kept rows [n][n_chains][n_par + 2]: per kept chain the series'
    words [L] and the statistics' words [3]"""

    def __init__(self, s, kept, chains, mats, edges):
        n_par = kept.shape[2] - 2
        self.n = len(kept)
        self.series, self.stats, self.T = [], [], []
        for c, mat in zip(chains, mats):
            par = np.ascontiguousarray(kept[:, c, :n_par])
            x, y = np.ascontiguousarray(mat[:, 0]), np.ascontiguousarray(mat[:, 1])
            e, u, T = s.check_values(par, x, y)
            l = s.pointwise_loglike_at(par, x, y)
            assert same_bits(T, ref.stats(e, u, s.cfg.model in SINE))
            self.series.append([ref.RefSeries(e[:, i], u[:, i], l[:, i]) for i in range(len(x))])
            self.stats.append([ref.RefStat(T[:, q], edges[q]) for q in range(3)])
            self.T.append(T)


def check_kept_chain(got, k, r, rk, what):
    """kept chain k of the Check `got` against kept chain rk of the Reference r, by the module's rule"""
    n = r.n
    assert int(got.n[0]) == n, (what, int(got.n[0]), n)
    series = r.series[rk]
    L = len(series)
    for f in EXACT:
        want = np.array([getattr(q, f) for q in series])
        assert same_bits(getattr(got, f)[k, :L], want), (what, k, f, getattr(got, f)[k, :L], want)
    worst = 0.0
    for f in ("S", "SU"):
        for i, q in enumerate(series):
            a = float(getattr(got, f)[k, i])
            if q.finite:
                want = getattr(q, f + "_exact")
                rel = 0.0 if a == want else abs(a - want) / abs(want)
                worst = max(worst, rel / (n * 2.0 ** -50))
            else:
                assert math.isnan(a) == math.isnan(getattr(q, f)), (what, k, f, i)
    assert worst <= 1, (what, k, "S or SU", worst)
    for q in range(3):
        st = r.stats[rk][q]
        for f, w in (("stat_origin", st.origin), ("stat_sum", st.sum), ("stat_sq", st.sq), ("stat_min", st.min),
                     ("stat_max", st.max)):
            assert same_bits(getattr(got, f)[k, q], w), (what, k, q, f, getattr(got, f)[k, q], w)
        assert got.counts[k, q].tolist() == st.counts.tolist(), (what, k, q)
    print("%s, kept chain %d: n = %d, L = %d, worst fraction of the S bound %.3g" % (what, k, n, L, worst))


def assert_same_check(a, b, what):
    assert int(a.n[0]) == int(b.n[0]), what
    for f in ck.STATE + ck.STAT_STATE + ("counts",):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (what, f)


def some_edges(T, n_edges=7):
    """edges [3][n_edges] among the T [n][3] themselves, so that a T equal to an edge occurs; spread where T repeats"""
    out = []
    for q in range(3):
        v = np.unique(T[np.isfinite(T[:, q]), q])
        pick = v[np.linspace(0, len(v) - 1, min(n_edges, len(v))).astype(int)] if len(v) else np.zeros(0)
        pick = np.unique(pick)
        while len(pick) < n_edges:
            pick = np.append(pick, (pick[-1] if len(pick) else 0.0) + 1.0)
        out.append(pick)
    return np.array(out)


# ---- 7. values ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model,n_par", SHAPES)
def test_values(model, n_par):
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    sigma = 0.37
    s = HipSampler(model, n_par, 1, case(model, n_par, 1, 1, 4)[1], seed=1, sigma=sigma)
    worst = 0.0
    for n_data in (1, 2, 63, 64, 65, 130):
        rows, data = case(model, n_par, 3, 1, n_data, seed=n_data)
        par = np.ascontiguousarray(rows[:, 0, :n_par])
        x, y = np.ascontiguousarray(data[:, 0]), np.ascontiguousarray(data[:, 1])
        e, u, T = s.check_values(par, x, y)
        one = s.check_values(par[1], x, y)
        v = s.predict_curve(par, x)
        assert e.shape == u.shape == (3, n_data) and T.shape == (3, 3)
        assert all(a.tobytes() == b[1].tobytes() for a, b in zip(one, (e, u, T)))
        with np.errstate(all="ignore"):
            want_e = (y - v) * (np.float64(1.0) / np.float64(sigma)) if model in SINE else y / v
        assert same_bits(e, want_e) and np.isfinite(e).all(), n_data
        for r in range(3):
            for i in range(n_data):
                t = mp.mpf(float(e[r, i]))
                want = mp.erfc(-t / mp.sqrt(2)) / 2 if model in SINE else -mp.expm1(-t)
                worst = max(worst, abs(float(mp.mpf(float(u[r, i])) - want)))
        assert same_bits(T, ref.stats(e, u, model in SINE)), (n_data, T, ref.stats(e, u, model in SINE))
        if n_data == 1:
            assert bits(T[:, 2]).tolist() == [0, 0, 0]        # no pair: +0.0
    s.close()
    print("model %d: worst |u - mpmath| %.3g" % (model, worst))
    assert worst <= 1e-12


# ---- 8. the fold ---------------------------------------------------------------------------------------------------------------
N_FOLD, L_FOLD, KEPT = 12, 65, [0, 2]


def fold_case(model, n_par):
    """12 steps of 3 chains, 65 data (a full wave and one: the lane-63 carry), kept chains 0 and 2; the reference of
    every count of samples the tests use, once per module"""
    key = ("fold", model)
    if key not in CACHE:
        rows, data = case(model, n_par, N_FOLD, 3, L_FOLD)
        s = HipSampler(model, n_par, 3, data, seed=1)
        T = s.check_values(np.ascontiguousarray(rows[:, 0, :n_par]), data[:, 0], data[:, 1])[2]
        edges = some_edges(T)
        refs = {n: Reference(s, rows[:n], KEPT, [data, data], edges) for n in (1, 3, 4, 5, N_FOLD)}
        refs["thin"] = Reference(s, rows[1::3], KEPT, [data, data], edges)
        s.close()
        CACHE[key] = rows, data, edges, refs
    return CACHE[key]


@pytest.mark.parametrize("model,n_par", SHAPES)
def test_fold_against_the_sequential_loop(model, n_par):
    """sample counts 1, 3, 4, 5 (the side-by-side width of the pulse models and its neighbours) and 12; the same rows
    in one call and in calls cut at [5, 7]; skip 1 and thin 3; beside a pointwise fold, whose m_dn and S_dn are m and S"""
    rows, data, edges, refs = fold_case(model, n_par)
    s = HipSampler(model, n_par, 3, data, seed=1)
    before = s.get_state()
    for n in (1, 3, 4, 5):
        got = fold(s, rows[:n], KEPT, edges)
        for k in range(2):
            check_kept_chain(got, k, refs[n], k, "model %d, %d samples" % (model, n))
    whole = fold(s, rows, KEPT, edges)
    assert whole.origin.shape == (2, L_FOLD) and whole.lengths is None and whole.counts.shape == (2, 3, 9)
    assert whole.x[1].tobytes() == data[:, 0].tobytes() and whole.y[0].tobytes() == data[:, 1].tobytes()
    for k in range(2):
        check_kept_chain(whole, k, refs[N_FOLD], k, "model %d, one call" % model)
    # a T equal to an edge lies in the slot above it
    T0 = refs[N_FOLD].T[0]
    assert any(T0[t, q] == edges[q, j] for t in range(N_FOLD) for q in range(3) for j in range(edges.shape[1]))
    # cut at [5, 7], beside a pointwise fold on the same sampler
    d = on_device(rows)
    s.check_begin(chains=KEPT, edges=edges)
    s.pointwise_begin(chains=KEPT)
    feed(s, d, [5, 7], also=s.pointwise_accumulate)
    cut, pw = s.check(), s.pointwise(at_mean=False)
    s.check_end()
    s.pointwise_end()
    assert_same_check(cut, whole, "cut at [5, 7]")
    assert cut.m.tobytes() == pw.m_dn.tobytes() and cut.S.tobytes() == pw.S_dn.tobytes()
    # skip and thin
    thinned = fold(s, rows, KEPT, edges, skip0=1, thin=3)
    again = fold(s, rows, KEPT, edges, calls=[5, 7], skip0=1, thin=3)
    assert int(thinned.n[0]) == 4 and thinned.thin == 3
    for k in range(2):
        check_kept_chain(thinned, k, refs["thin"], k, "model %d, skip 1 thin 3" % model)
    assert_same_check(again, thinned, "skip 1 thin 3, cut at [5, 7]")
    # the default edges are the null quantiles, and a fold without a histogram has the same words
    null = fold(s, rows, KEPT)
    bare = fold(s, rows, KEPT, nbins=1)
    assert null.nbins == 256 and null.edges[0].tobytes() == ck.null_edges(model, ck.FIT, L_FOLD, 255).tobytes()
    assert bare.nbins == 1 and bare.counts.shape == (2, 3, 2) and not bare.counts.any()
    for f in ck.STATE + ck.STAT_STATE:
        assert getattr(null, f).tobytes() == getattr(whole, f).tobytes() == getattr(bare, f).tobytes(), f
    assert (null.counts[:, :, :256].sum(axis=2) == N_FOLD).all() and 0 <= null.p_value("serial")[0] <= 1
    # the chains' state is untouched
    after = s.get_state()
    s.close()
    for f in ALL_FIELDS:
        assert getattr(before, f).tobytes() == getattr(after, f).tobytes(), f


def test_the_piece_boundary():
    """kPointwisePiece + 3 kept steps at n_data = 2: two launches of every kernel; cut elsewhere, the same bytes"""
    n = PIECE + 3
    model, n_par = wl.MODEL_SIMPLESIN, 4
    rows, data = case(model, n_par, n, 1, 2)
    s = HipSampler(model, n_par, 1, data, seed=1)
    T = s.check_values(np.ascontiguousarray(rows[:64, 0, :n_par]), data[:, 0], data[:, 1])[2]
    edges = some_edges(T, 5)
    got = fold(s, rows, (0,), edges)
    again = fold(s, rows, (0,), edges, calls=[PIECE - 3, 5, 1])
    r = Reference(s, rows, [0], [data], edges)
    s.close()
    check_kept_chain(got, 0, r, 0, "two pieces")
    assert_same_check(again, got, "cut elsewhere")


def test_a_nan_row_stays_in_its_kept_chain():
    model, n_par = wl.MODEL_SIMPLESIN, 4
    rows, data, edges, refs = fold_case(model, n_par)
    bad = rows.copy()
    bad[7, 2, 1] = np.nan                                     # a NaN frequency in one sample of the second kept chain
    s = HipSampler(model, n_par, 3, data, seed=1)
    clean = fold(s, rows, KEPT, edges, calls=[5, 7])
    got = fold(s, bad, KEPT, edges, calls=[5, 7])
    r = Reference(s, bad, KEPT, [data, data], edges)
    s.close()
    for f in ck.STATE + ck.STAT_STATE + ("counts",):
        assert getattr(got, f)[0].tobytes() == getattr(clean, f)[0].tobytes(), f
    assert got.counts[1, :, 8].tolist() == [1, 0, 1] and got.n_nan("fit", 1) == 1      # FIT and SERIAL are NaN, EXTREME skips
    # (every term of that sample is NaN: its EXTREME is -inf, a value like any other; min and max skip a NaN)
    assert got.counts[1, 1, :8].sum() == N_FOLD and got.stat_min[1, 1] == -math.inf
    assert np.isnan(got.stat_sum[1, 0]) and np.isnan(got.sum[1]).all() and np.isfinite(got.stat_min[1, [0, 2]]).all()
    check_kept_chain(got, 1, r, 1, "a NaN frequency")
    check_kept_chain(got, 0, refs[N_FOLD], 0, "beside a NaN frequency")


# ---- 9. placement ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lens", [(65, 65, 65), (5, 65, 64)])
def test_a_ladder_batch(lens):
    """3 ladders of 2 chains, equal and of lengths (5, 65, 64): kept chain k is the stand-alone fold of its ladder's
    data, lengths are reported, series past a length are untouched, per_ladder() trims; get -> set -> accumulate"""
    model, n_par, per = wl.MODEL_SIMPLESIN, 4, 2
    rows, data = case(model, n_par, N_FOLD, 3 * per, 130)
    sets = [data[10 * b:10 * b + n] for b, n in enumerate(lens)]
    chains = [1, per, 2 * per + 1]
    edges = np.stack([ck.null_edges(model, q, 65, 15) for q in range(3)])
    s = HipSampler.batch(model, n_par, per, sets, [1, 2, 3])
    before = s.get_state()
    if len(set(lens)) > 1:
        with pytest.raises(ValueError, match="length"):
            s.check_begin(chains=chains)                      # the null quantiles depend on the length
    got = fold(s, rows, chains, edges, calls=[5, 7])
    d = on_device(rows)
    s.check_begin(chains=chains, edges=edges)
    s.check_accumulate(d.data_ptr(), 5)
    half = s.check()
    s.check_end()
    s.check_begin(chains=chains, edges=edges)
    s.check_set(half)
    s.check_accumulate(d[5:].data_ptr(), 7)
    resumed = s.check()
    s.check_end()
    after = s.get_state()
    s.close()
    assert int(half.n[0]) == 5
    assert_same_check(resumed, got, "get, set, accumulate")
    for f in ALL_FIELDS:
        assert getattr(before, f).tobytes() == getattr(after, f).tobytes(), f
    ragged = len(set(lens)) > 1
    assert got.n_data == max(lens) and (got.lengths.tolist() == list(lens) if ragged else got.lengths is None)
    ones = got.per_ladder(3)
    for b, (one, c) in enumerate(zip(ones, chains)):
        L = lens[b]
        for f in ck.STATE + ("x", "y"):
            assert not getattr(got, f)[b, L:].any(), (b, f)
        alone = HipSampler(model, n_par, per, sets[b], seed=1)
        want = fold(alone, rows[:, b * per:(b + 1) * per], [c - b * per], edges)
        alone.close()
        assert one.n_data == L and one.x[0].tobytes() == sets[b][:, 0].tobytes() and one.lengths is None
        assert_same_check(one, want, "ladder %d" % b)
        assert len(one.text().splitlines()) == L and len(one.stats_text().splitlines()) == 3
    if ragged:
        with pytest.raises(ValueError, match="per_ladder"):
            got.text()


# ---- 10. refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals():
    model, n_par = wl.MODEL_SIMPLESIN, 4
    rows, data = case(model, n_par, 4, 3, 5)
    s = HipSampler(model, n_par, 3, data, seed=1)
    L = capi.lib()
    ip = C.POINTER(C.c_int32)
    dp = capi._dp
    d = on_device(rows)
    view = ck.Check.empty([0], data[:, 0], data[:, 1], np.zeros((3, 0)), model).view()
    lens = np.zeros(1, dtype=np.int32)
    # nothing was begun
    assert L.apemost_hip_check_accumulate(s._h, d.data_ptr(), 4, 0, 1) == capi.ERR_INVALID
    assert b"no check_begin" in L.apemost_hip_last_error()
    for call in (L.apemost_hip_check_get, L.apemost_hip_check_set):
        assert call(s._h, C.byref(view)) == capi.ERR_INVALID and b"no check_begin" in L.apemost_hip_last_error()
    assert L.apemost_hip_check_lengths(s._h, lens.ctypes.data_as(ip)) == capi.ERR_INVALID
    # chains
    for bad in ([3], [-1], [1, 1], [2, 0], []):
        ch = np.array(bad, dtype=np.int32)
        assert L.apemost_hip_check_begin(s._h, len(ch), ch.ctypes.data_as(ip), 0, None) == capi.ERR_INVALID, bad
    ch = np.array([0], dtype=np.int32)
    assert L.apemost_hip_check_begin(s._h, 1, None, 0, None) == capi.ERR_INVALID
    # edges
    good = np.array([[0.0, 1.0], [0.0, 1.0], [-1.0, 1.0]])
    for n_edges, e in ((2, None), (0, good), (-1, None), (4096, np.zeros((3, 4096)))):
        assert L.apemost_hip_check_begin(s._h, 1, ch.ctypes.data_as(ip), n_edges, None if e is None else e.ctypes.data_as(dp)) \
            == capi.ERR_INVALID, n_edges
    for q, j, v in ((0, 1, 0.0), (1, 0, math.nan), (2, 1, math.inf), (2, 0, 2.0)):
        e = good.copy()
        e[q, j] = v
        assert L.apemost_hip_check_begin(s._h, 1, ch.ctypes.data_as(ip), 2, e.ctypes.data_as(dp)) == capi.ERR_INVALID, (q, j)
        assert b"strictly ascending" in L.apemost_hip_last_error()
    assert L.apemost_hip_check_get(s._h, C.byref(view)) == capi.ERR_INVALID       # a refused begin begins nothing
    assert L.apemost_hip_check_begin(s._h, 1, ch.ctypes.data_as(ip), 2, good.ctypes.data_as(dp)) == capi.OK
    assert L.apemost_hip_check_accumulate(s._h, d.data_ptr(), 4, 0, 0) == capi.ERR_INVALID       # thin 0
    assert L.apemost_hip_check_get(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_check_lengths(s._h, lens.ctypes.data_as(ip)) == capi.OK and lens.tolist() == [5]
    assert L.apemost_hip_check_end(s._h) == capi.OK
    assert L.apemost_hip_check_accumulate(s._h, d.data_ptr(), 4, 0, 1) == capi.ERR_INVALID       # ended
    # values
    out = [np.zeros((2, 5)), np.zeros((2, 5)), np.zeros((2, 3))]
    par = np.ascontiguousarray(rows[:2, 0, :n_par])
    x, y = np.ascontiguousarray(data[:, 0]), np.ascontiguousarray(data[:, 1])
    a = [par.ctypes.data_as(dp), 5, x.ctypes.data_as(dp), y.ctypes.data_as(dp)] + [o.ctypes.data_as(dp) for o in out]
    call = L.apemost_hip_check_values
    assert call(s._h, 0, *a) == capi.ERR_INVALID and call(s._h, 2, a[0], 0, *a[2:]) == capi.ERR_INVALID
    for j in (0, 2, 3, 4, 5, 6):
        assert call(s._h, 2, *[None if i == j else v for i, v in enumerate(a)]) == capi.ERR_INVALID, j
    assert call(s._h, 2, *a) == capi.OK                       # needs no fold
    with pytest.raises(ValueError):
        s.check_values(par, x, y[:3])
    with pytest.raises(ValueError):
        s.check_begin(edges=np.zeros((2, 4)))
    s.close()


def test_a_user_model_is_refused():
    rs = np.random.RandomState(5)
    data = np.column_stack([(rs.uniform(size=64) < 0.5).astype(float), rs.normal(0, 1, (64, 2))])
    s = HipSampler(wl.MODEL_USER, 3, 5, data, seed=1,
                   device_model_source=os.path.join(hostlib.HOST, "examples", "device_models", "bernoulli_example.hip"))
    with pytest.raises(capi.ApemostHipError, match="user-supplied") as e:
        s.check_begin(chains=(0,), nbins=1)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ApemostHipError, match="user-supplied") as e:
        s.check_values(np.zeros(3), data[:4, 0], data[:4, 1])
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ApemostHipError, match="user-supplied") as e:
        s.check_begin(chains=(0,))                            # (the default edges: the null quantiles refuse it too)
    assert e.value.code == capi.ERR_UNSUPPORTED
    s.close()
