"""The tail of the pointwise fold (apemost_hip_pointwise_tail_*, pt_pointwise_tail.h) against tests/psis_ref.py's
selection: a sort of int64 keys over the dense matrix of terms.  Everything compares with == on the bits.

Where the terms come from.  Sine models: tests/pointwise_ref.py's bit-exact terms; the long series have the amplitude 0,
so the curve is the offset o and the term is ((o - y) * (o - y)) * c in plain IEEE operations, which numpy states bit
for bit (tests/test_gpu_pointwise.py::test_several_pieces_in_one_call), confirmed on samples against the rational
restatement.  Pulse models and user models: the device's own pointwise_loglike of the same rows, the same device
function.  tests/tail_linear_model.hip is a user model whose term is param0 * y_i, one multiplication: it gives the
series no built-in model can have (x = -l of both zero signs, -inf).

The end-to-end test holds tests/test_psis_cpu.py's bound for elpd."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from apemost_amd import capi, psis, workloads as wl
from apemost_amd.pointwise import PIECE, STATE
from apemost_amd.psis import PointwiseTail
from apemost_amd.sampler import HipSampler
from tests import hostlib
from tests import pointwise_ref as ref
from tests import psis_ref
from tests.helpers import make_pair
from tests.pointwise_ref import assert_same_state
from tests.test_gpu_pointwise import CHAINS, HAND_DATA, feed, hand_case, on_device, size_case
from tests.test_psis_cpu import elpd_bound

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
MODELS = os.path.join(hostlib.HOST, "examples", "device_models")
LINEAR = os.path.join(HERE, "tail_linear_model.hip")


def tail_fold(s, rows, chains, capacity, calls=None, skip0=0, thin=1, d=None):
    """(Pointwise, PointwiseTail) of the kept steps of rows, accumulated in the given calls"""
    d = on_device(rows) if d is None else d
    s.pointwise_begin(chains=chains, thin=thin, tail=capacity)
    assert s.pointwise_tail_capacity() == capacity
    feed(s, d, calls or [len(rows)], skip0, thin)
    pw, tail = s.pointwise(at_mean=False), s.pointwise_tail()
    s.pointwise_end()
    assert s.pointwise_tail_capacity() == 0
    return pw, tail


def expect(values, capacity):
    """values [n][n_keep][n_data]: the kept chains' terms -> (count, values) of the selection of -values"""
    return psis_ref.select_chains(-np.asarray(values), capacity)


def assert_tail(got, want, what=""):
    count, values = want
    assert got.count.shape == count.shape and got.values.shape == values.shape, what
    assert np.array_equal(got.count, count), (what, np.argwhere(got.count != count)[:4].tolist())
    if got.values.tobytes() != values.tobytes():
        bad = np.argwhere(got.values.view(np.uint64) != values.view(np.uint64))
        raise AssertionError("%s: %d values differ, first at %s: %r against %r" % (
            what, len(bad), tuple(bad[0]), got.values[tuple(bad[0])], values[tuple(bad[0])]))


def same_tail(a, b, what=""):
    assert np.array_equal(a.count, b.count) and a.values.tobytes() == b.values.tobytes(), what
    assert (a.n, a.capacity, a.thin) == (b.n, b.capacity, b.thin), what


# ---- 1. realistic rows at every data size -------------------------------------------------------------------------------
@pytest.mark.parametrize("n_data", [1, 63, 64, 65, 130])
def test_every_data_size(n_data):
    """12 steps of 5 chains of simplesin parameters, two kept chains, capacities 2 and 5 (both below the kept count) and
    16 (above it); calls of 1, 2 and 9 steps against one call"""
    rows, data, values = size_case()
    data, values = data[:n_data], values[:, :, :n_data]
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 5, data, seed=1)
    d = on_device(rows)
    for capacity in (2, 5, 16):
        pw, got = tail_fold(s, rows, CHAINS, capacity, [1, 2, 9], d=d)
        _, whole = tail_fold(s, rows, CHAINS, capacity, d=d)
        assert got.n == 12 == int(pw.n[0]) and got.chains.tolist() == CHAINS and got.n_data == n_data
        assert_tail(got, expect(values, capacity), "n_data %d capacity %d" % (n_data, capacity))
        same_tail(whole, got, "one call")
        assert got.values[:, :, 0].tobytes() == pw.m_dn.tobytes()       # the largest x is the fold's own maximum
    s.close()


# ---- 2. zero-amplitude rows: capacities and kept counts ------------------------------------------------------------------------------
C_SINE = ref.sine_constant(0.5)


def offset_rows(offsets):
    """offsets [n][n_chains] -> simplesin rows with the amplitude 0 and that offset"""
    n, nc = offsets.shape
    rows = np.zeros((n, nc, 6))
    rows[:, :, :4] = [0.0, 0.2, 0.4, 0.0]
    rows[:, :, 3] = offsets
    return rows


def offset_terms(offsets, y):
    """[n][n_chains][n_data]: ((o - y) * (o - y)) * c, every operation rounded once"""
    with np.errstate(all="ignore"):
        r = offsets[:, :, None] - np.asarray(y)[None, None, :]
        return (r * r) * C_SINE


def confirm(rows, data, values, chain, some):
    want = ref.terms(wl.MODEL_SIMPLESIN, rows[some, chain, :4], data, 0.5)
    assert values[some, chain].tobytes() == want.tobytes()


@pytest.mark.parametrize("capacity", [2, 5, 1024, 1025, 4096])
def test_capacities_and_kept_counts(capacity):
    """65 data (two blocks of lanes), chains 0 and 2 of 3, kept counts capacity - 1, capacity and capacity + 1 and, at the
    two small capacities, 3 * capacity.  1025 is the first capacity whose buffer doubles (P = 2048)."""
    rng = np.random.default_rng(capacity)
    n_max = max(capacity + 1, 3 * capacity if capacity <= 5 else 0)
    y = np.concatenate([rng.uniform(-1, 2, 64), [1e5]])
    data = np.stack([100 + 0.5 * np.arange(65), y], 1)
    offsets = 0.5 + 0.3 * rng.standard_normal((n_max, 3))
    rows, values = offset_rows(offsets), offset_terms(offsets, y)
    confirm(rows, data, values, 2, [0, 1, n_max - 1])
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 3, data, seed=1)
    d = on_device(rows)
    for n in sorted({capacity - 1, capacity, capacity + 1, n_max}):
        pw, got = tail_fold(s, rows[:n], [0, 2], capacity, d=d[:n])
        assert got.n == n and (got.count == min(n, capacity)).all()
        assert_tail(got, expect(values[:n][:, [0, 2]], capacity), "capacity %d, %d kept" % (capacity, n))
    s.close()


# ---- 3. the kinds of series, the pieces and the call boundaries ------------------------------------------------------------------------
SHAPE_Y = np.array([-1000.0, 1000.0, 0.25, 7.0])
SHAPE_CHAINS = [0, 1, 2, 3]
CACHE = {}


def shape_case():
    """8229 steps (the fold's piece of 8192 and 37) of 5 chains at 4 data with y = -1000, 1000, 0.25, 7.
    chain 0: the offset rises by 0.01 a step from 0.0037: at y = -1000 x = -l rises at every step (every sample is
             admitted and every piece compacts a full buffer), at y = 1000 it falls at every step (nothing is admitted
             behind the first `capacity`);
    chain 1: a constant offset: every x ties with the threshold;
    chain 2: offsets 0.25 + geometric integers: duplicates at every level, a few at the top, which straddle the threshold;
             at y = 0.25 the smallest |o - y| is 1;
    chain 3: noise, with an infinite offset (x = +inf) at six steps;
    chain 4: not kept."""
    if "shape" not in CACHE:
        rng = np.random.default_rng(8)
        n = PIECE + 37
        o = np.zeros((n, 5))
        o[:, 0] = 0.0037 + 0.01 * np.arange(n)
        o[:, 1] = 0.71
        o[:, 2] = 0.25 + rng.geometric(0.5, n)
        o[:, 3] = 0.5 + 0.3 * rng.standard_normal(n)
        o[[3, 2039, 2040, 4100, PIECE - 1, PIECE], 3] = np.inf
        o[:, 4] = 1.0
        rows, values = offset_rows(o), offset_terms(o, SHAPE_Y)
        data = np.stack([100 + 0.5 * np.arange(4), SHAPE_Y], 1)
        some = [0, 1, 2039, 2040, PIECE - 1, PIECE, n - 1]
        for c in (0, 2):
            confirm(rows, data, values, c, some)
        assert np.isneginf(values[3, 3]).all()                 # l = inf * c = -inf, x = +inf
        CACHE["shape"] = rows, data, values[:, SHAPE_CHAINS]
    return CACHE["shape"]


def shape_sampler():
    rows, data, values = shape_case()
    return HipSampler(wl.MODEL_SIMPLESIN, 4, 5, data, seed=1), rows, values


def test_the_kinds_of_series_over_the_pieces():
    """capacity 8 (tail piece 2040): 5000 kept steps cross three tail pieces, 8229 cross the fold's piece as well; one
    call, calls of 1, 7 and the rest, and cuts at the piece boundaries give the same bits"""
    s, rows, values = shape_sampler()
    d = on_device(rows)
    x = -values
    assert (np.diff(x[:, 0, 0]) > 0).all() and (np.diff(x[:, 0, 1]) < 0).all() and (np.diff(x[:, 1], axis=0) == 0).all()
    for n in (5000, PIECE + 37):
        want = expect(values[:n], 8)
        pw, got = tail_fold(s, rows[:n], SHAPE_CHAINS, 8, d=d[:n])
        assert_tail(got, want, "%d steps" % n)
        for calls in ([1, 7, n - 8], [2040, 2040, n - 4080], [2039, 2, n - 2041]):
            same_tail(tail_fold(s, rows[:n], SHAPE_CHAINS, 8, calls, d=d[:n])[1], got, str(calls))
        assert got.values[0, 0].tolist() == x[n - 8:n, 0, 0][::-1].tolist()          # rising: the last eight
        assert got.values[0, 1].tolist() == x[:8, 0, 1].tolist()                     # falling: the first eight
        assert (got.values[1] == x[0, 1][:, None]).all()                             # constant
        n_inf = int(np.isinf(x[:n, 3, 0]).sum())
        assert n_inf in (4, 6) and (got.values[3, :, :n_inf] == np.inf).all() and np.isfinite(got.values[3, :, n_inf:]).all()
        # duplicates straddle the threshold: more samples hold the eighth value than the tail has room for
        # (y = 1000 and 7, where the commonest offset gives the largest x); at the other two data the rare large offsets
        # fill the tail with runs of equal values
        for i in (1, 3):
            v8 = got.values[2, i, 7]
            assert (x[:n, 2, i] == v8).sum() > (got.values[2, i] == v8).sum() == 8, i
        for i in (0, 2):
            assert 1 < len(set(got.values[2, i].tolist())) < 8, i
        if n == 5000:                                         # 288 288 288 242 200 200 200 200, and six samples hold 200
            v8 = got.values[2, 2, 7]
            assert (x[:n, 2, 2] == v8).sum() > (got.values[2, 2] == v8).sum() < 8
    s.close()


@pytest.mark.parametrize("skip0,thin", [(2, 1), (1, 3), (5, 4)])
def test_skip_and_thin(skip0, thin):
    """the kept steps skip0, skip0 + thin, ... of the 8229, in calls of 1, 7, 33 and the rest, against the same kept rows
    accumulated in one call"""
    s, rows, values = shape_sampler()
    n = len(rows)
    pw, got = tail_fold(s, rows, SHAPE_CHAINS, 8, [1, 7, 33, n - 41], skip0, thin)
    kept = np.ascontiguousarray(rows[skip0::thin])
    assert got.n == len(kept) == int(pw.n[0]) and got.thin == thin
    assert_tail(got, expect(values[skip0::thin], 8), "skip %d thin %d" % (skip0, thin))
    _, plain = tail_fold(s, kept, SHAPE_CHAINS, 8)
    s.close()
    assert np.array_equal(plain.count, got.count) and plain.values.tobytes() == got.values.tobytes()


def test_a_nan_parameter_stays_in_its_chain():
    """a NaN frequency in two samples of chain 3 (an offset alone would not do: the amplitude is 0, but 0 * NaN is NaN):
    its count is short by two where the tail is not full, the other chains' tails are bit-identical"""
    s, rows, values = shape_sampler()
    rows, values = rows[:300], values[:300]
    bad = rows.copy()
    bad[[7, 250], 3, 1] = np.nan
    clean = tail_fold(s, rows, SHAPE_CHAINS, 512)[1]
    got = tail_fold(s, bad, SHAPE_CHAINS, 512, [1, 7, 292])[1]
    small = tail_fold(s, bad, SHAPE_CHAINS, 8)[1]
    s.close()
    v = values.copy()
    v[[7, 250], 3] = np.nan
    assert_tail(got, expect(v, 512), "a NaN frequency")
    assert_tail(small, expect(v, 8), "a NaN frequency, capacity 8")
    assert (got.count[3] == 298).all() and (got.count[:3] == 300).all() and (small.count == 8).all()
    assert got.values[:3].tobytes() == clean.values[:3].tobytes() and not np.isnan(got.values).any()


# ---- 4. interleaving, resuming, and the fold beside it -------------------------------------------------------------------------------
def test_get_between_accumulates_and_a_resumed_run():
    """get, accumulate, get: the forced sort of the first get does not disturb the state.  Then get -> a new sampler ->
    pointwise_set + tail_set -> the rest equals the uninterrupted fold."""
    s, rows, values = shape_sampler()
    rows, values = rows[:4500], values[:4500]
    d = on_device(rows)
    whole_pw, whole = tail_fold(s, rows, SHAPE_CHAINS, 8, d=d)
    for cut in (5, 2100):                                     # inside the warm-up (nothing compacted yet); behind a piece
        s.pointwise_begin(chains=SHAPE_CHAINS, tail=8)
        s.pointwise_accumulate(d.data_ptr(), cut)
        part_pw, part = s.pointwise(at_mean=False), s.pointwise_tail()
        assert_tail(part, expect(values[:cut], 8), "the first %d" % cut)
        same_tail(s.pointwise_tail(), part, "get twice")
        s.pointwise_accumulate(d[cut:].data_ptr(), len(rows) - cut)
        same_tail(s.pointwise_tail(), whole, "get, accumulate, get")
        assert_same_state(s.pointwise(at_mean=False), whole_pw, "the fold")
        s.pointwise_end()
        # a resumed run, in a sampler of its own; the loaded values need not be sorted
        s2 = HipSampler(wl.MODEL_SIMPLESIN, 4, 5, shape_case()[1], seed=1)
        s2.pointwise_begin(chains=SHAPE_CHAINS)
        s2.pointwise_set(part_pw)
        s2.pointwise_tail_begin(8)
        L = capi.lib()
        assert L.apemost_hip_pointwise_accumulate(s2._h, d[cut:].data_ptr(), 10, 0, 1) == capi.ERR_INVALID   # no tail_set yet
        assert b"pointwise_tail_set" in L.apemost_hip_last_error()
        shuffled = PointwiseTail(part.count, part.values[:, :, ::-1] if cut > 8 else part.values, 8, part.chains, part.n)
        s2.pointwise_tail_set(shuffled)
        same_tail(s2.pointwise_tail(), part, "set, get")
        s2.pointwise_accumulate(d[cut:].data_ptr(), len(rows) - cut)
        same_tail(s2.pointwise_tail(), whole, "resumed at %d" % cut)
        assert_same_state(s2.pointwise(at_mean=False), whole_pw, "the resumed fold")
        s2.close()
    s.close()


def test_the_fold_is_untouched():
    """with a tail begun, every word of the pointwise view is bitwise what it is without one"""
    for model in (wl.MODEL_SIMPLESIN, wl.MODEL_SINE3):
        rows, n_par, _ = hand_case(model)
        s = HipSampler(model, n_par, 5, HAND_DATA, seed=1)
        d = on_device(rows)
        s.pointwise_begin(chains=CHAINS)
        feed(s, d, [1, 2, 33, len(rows) - 36])
        plain = s.pointwise(at_mean=True)
        s.pointwise_end()
        with_tail, _ = tail_fold(s, rows, CHAINS, 5, [1, 2, 33, len(rows) - 36], d=d)
        s.close()
        assert_same_state(with_tail, plain, "model %d" % model)
        for f in STATE + ("par_origin", "par_sum"):
            assert getattr(with_tail, f).tobytes() == getattr(plain, f).tobytes(), f


# ---- 5. the models ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", [wl.MODEL_SIMPLESIN, wl.MODEL_SINE3], ids=["n_par4", "n_par10"])
def test_sine_models_over_tile_boundaries(model):
    """140 steps: 128 rows to an LDS tile with 4 parameters, 51 with 10; the rational restatement's terms"""
    rows, n_par, values = hand_case(model)
    s = HipSampler(model, n_par, 5, HAND_DATA, seed=1)
    for capacity in (5, 200):
        pw, got = tail_fold(s, rows, CHAINS, capacity, [1, 2, 33, len(rows) - 36])
        assert_tail(got, expect(values, capacity), "model %d capacity %d" % (model, capacity))
    s.close()


@pytest.mark.parametrize("model,n_par", [(wl.MODEL_PULSE, 6), (wl.MODEL_PULSE_VROT, 7)])
def test_pulse_models(model, n_par):
    """300 steps of 2 chains at 70 data, against the device's own pointwise_loglike; one row has a negative height
    (ln v is NaN at every datum)"""
    rng = np.random.default_rng(50 + model)
    nu = np.linspace(10, 12, 70)
    data = np.stack([nu, rng.exponential(1.0, 70)], 1)
    base = np.array([5.0, 0.05, 10.6, 4.0, 11.3, 2.5] if n_par == 6 else [5.0, 0.05, 0.05, 10.6, 4.0, 11.3, 2.5])
    rows = np.zeros((300, 2, n_par + 2))
    rows[:, :, :n_par] = base * (1 + 0.1 * rng.uniform(size=(300, 2, n_par)))
    rows[11, 1, n_par - 1] = -2.5
    rows[11, 1, n_par - 3] = -4.0
    s = HipSampler(model, n_par, 2, data, seed=1)
    values = np.stack([s.pointwise_loglike(np.ascontiguousarray(rows[:, c, :n_par])) for c in (0, 1)], axis=1)
    pw, got = tail_fold(s, rows, (0, 1), 20, [7, 293])
    s.close()
    assert np.isnan(values[11, 1]).all() and np.isfinite(values[:, 0]).all()
    assert_tail(got, expect(values, 20), "model %d" % model)
    assert got.values[:, :, 0].tobytes() == pw.m_dn.tobytes()


def test_a_batch_of_three_ladders():
    """three ladders with different data: every kept chain's tail is over its own ladder's data"""
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
    batch.pointwise_begin(chains=chains, tail=9)
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.pointwise_accumulate(d.data_ptr(), n_steps)
    got = batch.pointwise_tail()
    rows = d.cpu().numpy()
    values = np.stack([batch.pointwise_loglike(np.ascontiguousarray(rows[:, c, :w.n_par]), b) for b, c in enumerate(chains)],
                      axis=1)
    batch.pointwise_end()
    batch.close()
    assert got.n_ladders == 3 and got.n == n_steps and n_steps > 9
    assert_tail(got, expect(values, 9), "three ladders")
    lads = got.per_ladder()
    assert [t.chains.tolist() for t in lads] == [[c] for c in chains] and lads[2].values.tobytes() == got.values[2:].tobytes()
    assert got.values[0].tobytes() != got.values[1].tobytes()


def test_user_models():
    """simplesin2_hooks through the analysis module's append kernel, against its own pointwise_loglike; the linear model
    for what no built-in term can be: x of both zero signs, both infinities, NaN and exact duplicates, stated by numpy;
    a model without the hook is refused"""
    from tests.test_gpu_user_hooks import SINE2
    rng = np.random.default_rng(12)
    data = np.stack([100 + 0.5 * np.arange(70), rng.uniform(-1, 2, 70)], 1)
    rows = np.zeros((150, 3, 4))
    rows[:, :, :2] = np.array([0.9, 0.2]) + np.array([0.05, 1e-4]) * rng.standard_normal((150, 3, 2))
    s = HipSampler(wl.MODEL_USER, 2, 3, data, seed=1, device_model_source=SINE2)
    values = np.stack([s.pointwise_loglike(np.ascontiguousarray(rows[:, c, :2])) for c in (0, 2)], axis=1)
    pw, got = tail_fold(s, rows, (0, 2), 7, [1, 7, 142])
    s.close()
    assert np.isfinite(values).all()
    assert_tail(got, expect(values, 7), "simplesin2_hooks")
    # the linear model: l = param0 * y
    y = np.array([1.0, -1.0, 0.5, -0.0, 3.0])
    data = np.stack([np.arange(5.0), y], 1)
    p = rng.integers(-3, 4, (2500, 2)).astype(float)          # duplicates, and +0 among them
    p[::9, 0] = -0.0
    p[[5, 2041], 0] = np.inf
    p[[6, 2100], 0] = -np.inf
    p[[8, 77], 1] = np.nan
    rows = np.zeros((2500, 2, 4))
    rows[:, :, 0] = p
    with np.errstate(all="ignore"):
        values = p[:, :, None] * y[None, None, :]
    s = HipSampler(wl.MODEL_USER, 2, 2, data, seed=1, device_model_source=LINEAR)
    device = np.stack([s.pointwise_loglike(np.ascontiguousarray(rows[:, c, :2])) for c in (0, 1)], axis=1)
    assert np.array_equal(device.view(np.uint64)[~np.isnan(values)], values.view(np.uint64)[~np.isnan(values)])
    assert np.array_equal(np.isnan(device), np.isnan(values))
    for capacity in (8, 2500):
        pw, got = tail_fold(s, rows, (0, 1), capacity, [1, 7, 2492])
        assert_tail(got, expect(values, capacity), "the linear model, capacity %d" % capacity)
    s.close()
    x = got.values[0, 0, :int(got.count[0, 0])]
    zeros = x[x == 0]
    assert np.signbit(zeros).any() and not np.signbit(zeros).all()                   # both zeros are there ...
    assert not np.signbit(zeros[:np.argmax(np.signbit(zeros))]).any()                # ... +0 before -0
    assert x[0] == np.inf and x[-1] == -np.inf and (got.count[1] == 2498).all() and got.count[0].tolist() == [2500] * 3 + [2496, 2500]
    # a model without the hook
    rs = np.random.RandomState(5)
    data = np.column_stack([(rs.uniform(size=64) < 0.5).astype(float), rs.normal(0, 1, (64, 2))])
    s = HipSampler(wl.MODEL_USER, 3, 5, data, seed=1, device_model_source=os.path.join(MODELS, "bernoulli_example.hip"))
    L = capi.lib()
    t = PointwiseTail.empty((0,), 64, 4)
    assert L.apemost_hip_pointwise_tail_begin(s._h, 4) == capi.ERR_UNSUPPORTED and b"user" in L.apemost_hip_last_error()
    assert L.apemost_hip_pointwise_tail_get(s._h, C.byref(t.view())) == capi.ERR_INVALID
    s.close()


# ---- 6. refusals -----------------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    w = wl.simplesin(n_data=64, n_chain=4)
    s = HipSampler(w.model, w.n_par, 4, w.data, seed=1)
    L = capi.lib()
    d = torch.zeros((12, 4, w.n_par + 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    t = PointwiseTail.empty((0,), 64, 4)
    cap = C.c_int32(-1)
    assert L.apemost_hip_pointwise_tail_begin(s._h, 4) == capi.ERR_INVALID             # no pointwise_begin
    assert b"no pointwise_begin" in L.apemost_hip_last_error()
    assert L.apemost_hip_pointwise_tail_capacity(s._h, C.byref(cap)) == capi.OK and cap.value == 0
    assert L.apemost_hip_pointwise_tail_capacity(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_tail_get(s._h, C.byref(t.view())) == capi.ERR_INVALID
    s.pointwise_begin(chains=(0,))
    assert L.apemost_hip_pointwise_tail_get(s._h, C.byref(t.view())) == capi.ERR_INVALID  # a fold without a tail
    assert L.apemost_hip_pointwise_tail_set(s._h, C.byref(t.view())) == capi.ERR_INVALID
    for bad in (-1, 0, 1, 4097, 1 << 20):
        assert L.apemost_hip_pointwise_tail_begin(s._h, bad) == capi.ERR_INVALID, bad
        assert b"capacity" in L.apemost_hip_last_error()
    assert s.pointwise_tail_capacity() == 0
    assert L.apemost_hip_pointwise_tail_begin(s._h, 4) == capi.OK and s.pointwise_tail_capacity() == 4
    assert L.apemost_hip_pointwise_tail_get(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_tail_get(s._h, C.byref(capi.PointwiseTailView())) == capi.ERR_INVALID
    s.pointwise_accumulate(d.data_ptr(), 12)
    # the fold has samples of its own now: a new tail would have lost theirs; the refused begin leaves the old tail
    assert L.apemost_hip_pointwise_tail_begin(s._h, 6) == capi.ERR_INVALID and b"lost" in L.apemost_hip_last_error()
    assert L.apemost_hip_pointwise_tail_begin(s._h, 1) == capi.ERR_INVALID
    got = s.pointwise_tail()
    assert got.capacity == 4 and got.n == 12 and (got.count == 4).all()
    assert (got.values == got.values[:, :, :1]).all() and (got.values > 0).all()     # rows of zeros: a constant term
    # tail_set: a count above the capacity, a NaN among the counted values
    t.count[:] = 5
    assert L.apemost_hip_pointwise_tail_set(s._h, C.byref(t.view())) == capi.ERR_INVALID and b"capacity" in L.apemost_hip_last_error()
    t.count[:] = 2
    t.values[0, 3, 1] = np.nan
    assert L.apemost_hip_pointwise_tail_set(s._h, C.byref(t.view())) == capi.ERR_INVALID and b"NaN" in L.apemost_hip_last_error()
    t.values[0, 3, 1], t.values[0, 3, 2] = 1.0, np.nan        # behind count: ignored
    assert L.apemost_hip_pointwise_tail_set(s._h, C.byref(t.view())) == capi.OK
    back = s.pointwise_tail()
    assert (back.count == 2).all() and back.values[0, 3].tolist() == [1.0, 0.0, 0.0, 0.0]
    # pointwise_set does not touch the tail; pointwise_begin drops it
    pw = s.pointwise(at_mean=False)
    s.pointwise_set(pw)
    assert s.pointwise_tail_capacity() == 4
    assert L.apemost_hip_pointwise_tail_begin(s._h, 6) == capi.OK                      # right behind pointwise_set
    s.pointwise_begin(chains=(0, 1))
    assert s.pointwise_tail_capacity() == 0
    s.pointwise_end()
    with pytest.raises(ValueError):
        s.pointwise_begin(chains=(0,), tail="auto")
    s.pointwise_begin(chains=(0,), tail="auto:1000000")
    assert s.pointwise_tail_capacity() == 3001
    s.pointwise_end()
    s.close()


def test_too_many_slots_are_refused():
    """2^28 slots: 16 kept chains of 4096 data are 2^16 series; B = 2^13 (capacity 2049 .. 4096) is 2^29 slots and is
    refused with the capacity that fits, 2048 (B = 2^12), which is accepted"""
    n_data = 4096
    data = np.stack([100 + 0.5 * np.arange(n_data), np.ones(n_data)], 1)
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 16, data, seed=1)
    L = capi.lib()
    s.pointwise_begin(chains=tuple(range(16)))
    assert L.apemost_hip_pointwise_tail_begin(s._h, 2049) == capi.ERR_INVALID
    msg = L.apemost_hip_last_error()
    assert b"2^28" in msg and b"fits is 2048" in msg, msg
    assert s.pointwise_tail_capacity() == 0
    assert L.apemost_hip_pointwise_tail_begin(s._h, 2048) == capi.OK
    s.pointwise_end()
    s.close()


# ---- 7. end to end ---------------------------------------------------------------------------------------------------------
def test_a_real_run_end_to_end():
    """simplesin, 8 chains, 64 data, 5 launches of 600 steps without swap attempts (3000 kept samples of chain 0, M = 165):
    the tail equals the selection over pointwise_loglike of the dumped rows, psis() from the device state equals the
    dense restatement over the same terms within tests/test_psis_cpu.py's bound, and the run's rows and final state
    are bitwise those of a run without the tail"""
    n_chain, per, launches = 8, 600, 5
    w = wl.simplesin(n_data=64, n_chain=n_chain)
    st, _, _ = make_pair(w, n_chain, seed=5)
    out = []
    for with_tail in (True, False):
        s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=5)
        st.prob[:], st.prior[:] = s.loglike(st.params, st.beta)
        s.set_state(st)
        d = torch.zeros((launches, per, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
        s.pointwise_begin(chains=(0,), tail="auto:%d" % (launches * per) if with_tail else None)
        for k in range(launches):
            s.launch_rounds(1, per, False, d[k].data_ptr())
            s.pointwise_accumulate(d[k].data_ptr(), per)
        pw = s.pointwise()
        tail = s.pointwise_tail() if with_tail else None
        s.synchronize()
        rows = d.cpu().numpy().reshape(launches * per, n_chain, w.n_par + 2)
        if with_tail:
            n = launches * per
            terms = s.pointwise_loglike(np.ascontiguousarray(rows[:, 0, :w.n_par]))
            assert np.isfinite(terms).all() and tail.capacity == 166 == psis.capacity_for(n) and tail.n == n
            assert_tail(tail, expect(terms[:, None, :], 166), "the run")
            res = psis.psis(pw, tail)
            worst = 0.0
            for i in range(64):
                elpd, k_hat, M = psis_ref.psis_dense(terms[:, i], psis.gpdfit)
                assert M == 165 == res.tail_len[i] and np.float64(k_hat).tobytes() == np.float64(res.k[i]).tobytes(), i
                f = abs(res.elpd[i] - elpd) / elpd_bound(n, res.ratio[i], pw.m_dn[0, i], elpd)
                worst = max(worst, f)
                assert f <= 1, (i, res.elpd[i], elpd, res.ratio[i])
            print("psis from the device state against the dense restatement: worst %.3g of the bound; k-hat %.3f .. %.3f"
                  % (worst, res.k.min(), res.k.max()))
            # (an uncalibrated chain repeats a rejected state many times over: where the repeats fill a quarter of a
            # tail the fit has no value and k-hat is the stated +inf, in the restatement as here)
            assert np.isfinite(res.k).sum() >= 8 and not np.isnan(res.k).any() and np.isfinite(res.elpd).all()
            assert not res.tail_short.any() and len(res.text().splitlines()) == 10 + 64
        s.pointwise_end()
        out.append((s.get_state(), rows, pw))
        s.close()
    for f in ("params", "prob", "prior", "accept", "reject", "n_iter", "swapcount", "step", "beta"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()
    assert_same_state(out[0][2], out[1][2], "the fold with and without the tail")


# ---- 8. the C host: APEMOST_POINTWISE_TAIL ------------------------------------------------------------------------------------
def test_c_host_tail(tmp_path):
    """a bounded run of 3000 kept samples with APEMOST_DUMP=binary,pointwise: with APEMOST_POINTWISE_TAIL=auto the host
    writes pointwise_tail.bin, byte for byte what PointwiseTail.write gives for a Python fold of the dumped rows; every
    other file of the run is byte for byte that of the same run without the variable, which writes no tail file;
    --append resumes the tail; a malformed value and a file of another capacity are refused"""
    import subprocess
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
    import samples_bin
    from apemost_amd.pointwise import Pointwise
    n_beta, iters = 8, 3000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    runs = {}
    for tail in ("auto", None):
        work = tmp_path / ("tail_%s" % tail)
        work.mkdir()
        (work / "params").write_text(w.params_file_text())
        (work / "data").write_text(w.data_file_text())
        env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP="binary,pointwise")
        env.pop("APEMOST_POINTWISE_TAIL", None)
        if tail:
            env["APEMOST_POINTWISE_TAIL"] = tail
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
        runs[tail] = (work, env)
    work, env = runs["auto"]
    plain, _ = runs[None]
    names = sorted(os.listdir(str(work)))
    assert "pointwise_tail.bin" in names and sorted(os.listdir(str(plain))) == [f for f in names if f != "pointwise_tail.bin"]
    for f in names:
        if f != "pointwise_tail.bin" and os.path.isfile(str(work / f)):
            assert (work / f).read_bytes() == (plain / f).read_bytes(), f

    def python_tail(capacity):
        _, params, probs = samples_bin.read(str(work / "samples.bin"))
        rows = np.zeros((len(params), 1, w.n_par + 2))
        rows[:, 0, :w.n_par] = params[:, 0]
        rows[:, 0, w.n_par:] = probs[:, 0]
        s = HipSampler(w.model, w.n_par, 1, np.loadtxt(str(work / "data")), seed=1)
        _, t = tail_fold(s, rows, (0,), capacity)
        s.close()
        t.write(str(tmp_path / "python_tail.bin"))
        return t, (tmp_path / "python_tail.bin").read_bytes()
    mine, raw = python_tail(psis.capacity_for(iters))
    assert mine.capacity == 166 and mine.n == iters and (work / "pointwise_tail.bin").read_bytes() == raw
    res = psis.psis(Pointwise.read(str(work / "pointwise.bin")), PointwiseTail.read(str(work / "pointwise_tail.bin")))
    assert res.tail_len.tolist() == [165] * 128 and not np.isnan(res.k).any() and np.isfinite(res.elpd).all()
    out = subprocess.run([sys.executable, "-m", "apemost_amd.psis", str(work)], stdout=subprocess.PIPE, universal_newlines=True,
                         env=dict(os.environ, PYTHONPATH=os.path.dirname(HERE)), timeout=120)
    assert out.returncode == 0 and out.stdout == res.text()
    # refusals, before the run: the files stay as they are
    for bad, needle in (("abc", "APEMOST_POINTWISE_TAIL"), ("1", "APEMOST_POINTWISE_TAIL"), ("5000", "APEMOST_POINTWISE_TAIL")):
        r = subprocess.run([exe, "run"], cwd=str(work), env=dict(env, APEMOST_POINTWISE_TAIL=bad), stdout=subprocess.DEVNULL,
                           stderr=subprocess.PIPE, timeout=300)
        assert r.returncode != 0 and needle.encode() in r.stderr and b"expected" in r.stderr, bad
    r = subprocess.run([exe, "run", "--append"], cwd=str(work), env=dict(env, APEMOST_POINTWISE_TAIL="50"),
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
    assert r.returncode != 0 and b"another shape" in r.stderr
    assert (work / "pointwise_tail.bin").read_bytes() == raw
    # --append goes on from the file (auto keeps the file's capacity)
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = PointwiseTail.read(str(work / "pointwise_tail.bin"))
    assert second.n == 2 * iters and second.capacity == 166
    both, raw2 = python_tail(166)
    assert both.n == 2 * iters and (work / "pointwise_tail.bin").read_bytes() == raw2
    assert np.all(second.values[:, :, 0] >= mine.values[:, :, 0])
