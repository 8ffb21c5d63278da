"""The pointwise fold at the caller's data and the joint predictive of a block (apemost_hip_pointwise_begin_at,
apemost_hip_pointwise_joint_*, apemost_hip_pointwise_loglike_at; apemost_amd/csrc/pt_pointwise_joint.h) and K-fold
cross-validation on a ragged ladder batch (apemost_amd/kfold.py).

The fold's eight words are held to the rule of tests/test_gpu_pointwise.py (its `check`, its `pulse_delta`), against
tests/pointwise_ref.py over the held-out matrices: no tolerance is added here.

The joint words.  J_t is restated by tests/kfold_ref.py (joint_sum) from the reference's terms and folded by RefJoint.
Sine models: the terms are bit for bit, the two-stage sum is a fixed order of IEEE additions, so origin, sum, sq and m
compare with == on the bits; S is held to n 2^-50 relative against math.fsum of the reference's exponentials about the
final maximum, the rule of tests/test_gpu_evidence.py.  Pulse models: a term differs from the reference's by at most
delta (pulse_delta), and a sum of L terms in any fixed order carries at most (L - 1) u relative to the sum of the
magnitudes on either side (u = 2^-53), so per sample
    |J_dev - J_ref| <= Delta_t = sum_i delta_{t,i} + 2 (L - 1) u sum_i |l_{t,i}|.
Delta is carried into the five words as `check` carries delta into the series' words, with that module's factor 2:
    origin  Delta_0;   d_t = J_t - origin:  e_t = Delta_t + Delta_0 + 2 u |d_t|
    sum     sum_t e_t + 2 (n - 1) u sum_t |d_t|
    sq      sum_t (2 |d_t| e_t + e_t^2 + 2 u d_t^2) + 2 (n - 1) u sum_t d_t^2
    m       max_t Delta_t
    S       n 2^-50 + 2 (2 max_t Delta_t), relative.
The worst fraction of each bound is printed."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

from apemost_amd import capi, kfold, workloads as wl
from apemost_amd.pointwise import PIECE, STATE
from apemost_amd.sampler import HipSampler
from apemost_amd.state import ALL_FIELDS
from tests import hostlib
from tests import pointwise_ref as ref
from tests.helpers import make_pair
from tests.kfold_ref import RefJoint, joint_sum
from tests.pointwise_ref import RefPointwise, assert_same_state
from tests.test_gpu_pointwise import SINE, U, check, feed, on_device, pulse_delta, size_case

pytestmark = pytest.mark.gpu

JOINT = kfold.JOINT_STATE
CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    """== on the bits, a NaN by its position"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def assert_same_joint(got, want, what):
    assert int(got.n[0]) == int(want.n[0]), what
    for f in JOINT:
        assert same_bits(getattr(got, f), getattr(want, f)), (what, f, getattr(got, f), getattr(want, f))


def at_fold(s, rows, chains, mats, calls=None, skip0=0, thin=1, joint=True):
    """the fold of rows at the matrices `mats`: (Pointwise, Joint or None)"""
    d = on_device(rows)
    s.pointwise_begin(chains=chains, thin=thin, at=mats, joint=joint)
    feed(s, d, calls or [len(rows)], skip0, thin)
    pw = s.pointwise()
    jt = s.pointwise_joint() if joint else None
    s.pointwise_end()
    return pw, jt


def check_joint(jt, k, values, what, delta=None):
    """kept chain k's five joint words against RefJoint over the reference's terms values [n][L] by the module's rule"""
    values = np.asarray(values, dtype=np.float64)
    n, L = values.shape
    J = joint_sum(values).reshape(n)
    r = RefJoint(J)
    got = {f: float(getattr(jt, f)[k]) for f in JOINT}
    assert int(jt.n[0]) == n, (what, int(jt.n[0]), n)
    worst = {}
    if delta is None:
        for f in ("origin", "sum", "sq", "m"):
            assert same_bits(got[f], getattr(r, f)), (what, k, f, got[f], getattr(r, f))
        extra = 0.0
    else:
        assert delta.shape == values.shape and r.finite
        D = delta.sum(axis=1) + 2 * (L - 1) * U * np.abs(values).sum(axis=1)
        d = J - J[0]
        e = D + D[0] + 2 * U * np.abs(d)
        bounds = {"origin": D[0], "sum": e.sum() + 2 * (n - 1) * U * np.abs(d).sum(),
                  "sq": (2 * np.abs(d) * e + e * e + 2 * U * d * d).sum() + 2 * (n - 1) * U * (d * d).sum(), "m": D.max()}
        for f, b in bounds.items():
            diff = abs(got[f] - getattr(r, f))
            worst[f] = 0.0 if diff == 0 else diff / (2 * b)
            assert worst[f] <= 1, (what, k, f, worst[f])
        extra = 2 * (2 * D.max())
    if r.finite:
        tol = n * 2.0 ** -50 + extra
        rel = 0.0 if got["S"] == r.S_exact else abs(got["S"] - r.S_exact) / abs(r.S_exact)
        worst["S"] = rel / tol
        assert worst["S"] <= 1, (what, k, "S", worst["S"])
    else:
        assert same_bits(np.isnan(got["S"]), np.isnan(r.S)), (what, k, "S")
    print("%s, joint of kept chain %d: n = %d, L = %d, worst fractions of the bounds: %s" % (
        what, k, n, L, ", ".join("%s %.3g" % kv for kv in worst.items())))
    return r


# ---- the hand-built case of tests 2, 4 and 5: the curve is the offset ----------------------------------------------------------
N_BIG = 300
KEPT4, LENS4 = [0, 2, 3, 5], [1, 65, 130, 64]


def flat_case():
    """300 steps of 6 chains of simplesin with the amplitude exactly 0: the curve is the offset whatever the sine is, and
    the term is ((o - y) * (o - y)) * c in plain IEEE operations, which numpy states bit for bit
    (tests/test_gpu_pointwise.py::test_several_pieces_in_one_call); 130 held-out data, none of them among the sampler's
    own 7; samples spread over the run are confirmed against the rational restatement"""
    if "flat" not in CACHE:
        rng = np.random.default_rng(21)
        rows = np.zeros((N_BIG, 6, 6))
        rows[:, :, :4] = [0.0, 0.2, 0.4, 0.0]
        rows[:, :, 3] = 0.5 + 0.3 * rng.standard_normal((N_BIG, 6))
        held = np.stack([np.concatenate([200.25 + 0.5 * np.arange(128), [2.45e6 + 0.5, -3.25]]), rng.uniform(-1, 2, 130)], 1)
        own = np.stack([100 + 0.5 * np.arange(7), rng.uniform(-1, 2, 7)], 1)
        some = [0, 1, 128, N_BIG - 1]
        assert flat_values(rows[some], 3, held).tobytes() == ref.terms(wl.MODEL_SIMPLESIN, rows[some, 3, :4], held, 0.5).tobytes()
        CACHE["flat"] = rows, held, own
    return CACHE["flat"]


def flat_values(rows, chain, mat):
    """[n][len(mat)]: the terms of chain `chain` of flat_case's rows at the data mat"""
    r0 = rows[:, chain, 3, None] - mat[None, :, 1]
    v = (r0 * r0) * ref.sine_constant(0.5)
    assert not (v == 0).any()                                 # (no -0.0 among the terms: a lane partial is +0.0 + l)
    return v


def mats4(held):
    return [held[5:6], held[:65], held[:130], held[60:124]]


def check_four(pw, jt, rows, held, what):
    """the fold of four kept chains with n_at = [1, 65, 130, 64]: each kept chain against its own reference, and the
    series past each length keep their initial zeros"""
    assert pw.lengths.tolist() == LENS4 and pw.n_data == 130 and pw.origin.shape == (4, 130) and pw.heldout
    for k, (one, mat) in enumerate(zip(pw.per_ladder(4), mats4(held))):
        L = LENS4[k]
        for f in STATE + ("x", "y"):
            assert not getattr(pw, f)[k, L:].any(), (what, k, f)
        vals = flat_values(rows, KEPT4[k], mat)
        assert one.n_data == L and one.x[0].tobytes() == mat[:, 0].tobytes() and one.y[0].tobytes() == mat[:, 1].tobytes()
        check(one, RefPointwise(wl.MODEL_SIMPLESIN, rows, [KEPT4[k]], mat, values=vals[:, None, :]), wl.MODEL_SIMPLESIN,
              "%s, kept chain %d of four" % (what, k))
        check_joint(jt, k, vals, what)
    # n_at = 1: J is +0.0 + l = l, so the block's five words are the series'
    for f, g in zip(JOINT, ("origin", "sum", "sq", "m_up", "S_up")):
        assert bits(getattr(jt, f)[0]) == bits(getattr(pw, g)[0, 0]), (what, f)


# ---- 1. identity: begin_at at the kept chains' own data is begin --------------------------------------------------------------
def test_at_the_samplers_own_data_is_the_plain_fold():
    rows, data, _ = size_case()
    data = data[:65]
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 5, data, seed=1)
    d = on_device(rows)
    s.pointwise_begin(chains=[0, 3])
    feed(s, d, [1, 2, 9])
    plain = s.pointwise(at_mean=False)
    s.pointwise_end()
    mine, _ = at_fold(s, rows, [0, 3], [data, data], [1, 2, 9], joint=False)
    both, jt = at_fold(s, rows, [0, 3], data, [1, 2, 9])      # one matrix for all; the joint kernels change no word
    s.close()
    for got in (mine, both):
        assert_same_state(got, plain, "n_data 65")
        assert got.lengths is None and got.x.tobytes() == plain.x.tobytes() and got.y.tobytes() == plain.y.tobytes()
        assert got.heldout and not plain.heldout and np.isnan(got.at_mean).all()
    assert int(jt.n[0]) == 12 and jt.lengths.tolist() == [65, 65]


def test_at_a_ragged_batchs_own_data_is_the_plain_fold():
    _, data, _ = size_case()
    lens, per = [1, 65, 130], 4
    sets = [data[130 - n:] for n in lens]                     # (different data per ladder)
    rng = np.random.default_rng(3)
    rows = np.zeros((12, 3 * per, 6))
    rows[:, :, :4] = np.array([0.9, 0.2, 0.4, 0.5]) + np.array([0.05, 1e-4, 0.02, 0.05]) * rng.standard_normal((12, 3 * per, 4))
    chains = [0, per, 2 * per + 1]
    s = HipSampler.batch(wl.MODEL_SIMPLESIN, 4, per, sets, [1, 2, 3])
    d = on_device(rows)
    s.pointwise_begin(chains=chains)
    feed(s, d, [5, 7])
    plain = s.pointwise(at_mean=False)
    s.pointwise_end()
    mine, jt = at_fold(s, rows, chains, sets, [5, 7])
    s.close()
    assert_same_state(mine, plain, "lengths 1, 65, 130")
    assert mine.lengths.tolist() == lens == plain.lengths.tolist() and mine.n_data == 130
    assert mine.x.tobytes() == plain.x.tobytes() and mine.y.tobytes() == plain.y.tobytes()
    assert jt.lengths.tolist() == lens and np.isfinite(jt.lpd()).all()


# ---- 2. every length and every count of samples ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 5, 129, 300])
def test_every_length(n):
    """n_at 1, 63, 64, 65 and 130 with one kept chain, then 1, 65, 130 and 64 in one fold; n samples: the first sample
    alone, every remainder of four side by side, a tile of 128 rows and one more (n_par 4), and for the joint fold a
    chunk of 64 samples less one, one more, and several"""
    rows, held, own = flat_case()
    rows = rows[:n]
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 6, own, seed=1)
    for L in (1, 63, 64, 65, 130):
        mat = held[:L]
        pw, jt = at_fold(s, rows, [2], [mat])
        vals = flat_values(rows, 2, mat)
        assert pw.origin.shape == (1, L) and pw.lengths is None and pw.heldout and np.isnan(pw.at_mean).all()
        assert pw.x[0].tobytes() == mat[:, 0].tobytes() and pw.y[0].tobytes() == mat[:, 1].tobytes()
        check(pw, RefPointwise(wl.MODEL_SIMPLESIN, rows, [2], mat, values=vals[:, None, :]), wl.MODEL_SIMPLESIN,
              "n %d n_at %d" % (n, L))
        check_joint(jt, 0, vals, "n %d n_at %d" % (n, L))
        assert jt.lengths.tolist() == [L]
    pw, jt = at_fold(s, rows, KEPT4, mats4(held))
    s.close()
    check_four(pw, jt, rows, held, "n %d" % n)


# ---- 3. the models ---------------------------------------------------------------------------------------------------------------
def model_case(model, n_par, n):
    rng = np.random.default_rng(60 + model)
    rows = np.zeros((n, 2, n_par + 2))
    if model in SINE:
        start = np.array([0.9, 0.2, 0.4, 0.5] if n_par == 4 else [0.9, 0.2, 0.4, 0.54, 0.11, 0.1, 0.27, 0.27, 0.7, 0.5])
        scale = 0.02 * np.array([1, 1e-3, 1, 1] if n_par == 4 else [1, 1e-3, 1] * 3 + [1])
        rows[:, :, :n_par] = start + scale * rng.standard_normal((n, 2, n_par))
        held = np.stack([100.25 + 0.5 * np.arange(41), rng.uniform(-1, 2, 41)], 1)
        own = np.stack([100 + 0.5 * np.arange(16), rng.uniform(-1, 2, 16)], 1)
    else:
        base = np.array([5.0, 0.05, 10.6, 4.0, 11.3, 2.5] if n_par == 6 else [5.0, 0.05, 0.05, 10.6, 4.0, 11.3, 2.5])
        rows[:, :, :n_par] = base * (1 + 0.1 * rng.uniform(size=(n, 2, n_par)))
        held = np.stack([np.linspace(10.013, 11.987, 41), rng.exponential(1.0, 41)], 1)
        own = np.stack([np.linspace(10, 12, 16), rng.exponential(1.0, 16)], 1)
    assert not np.isin(held[:, 0], own[:, 0]).any()
    return rows, held, own


@pytest.mark.parametrize("model,n_par,n", [(wl.MODEL_SIMPLESIN, 4, 40), (wl.MODEL_SINE3, 10, 55), (wl.MODEL_PULSE, 6, 30),
                                           (wl.MODEL_PULSE_VROT, 7, 30)])
def test_every_model_at_held_out_data(model, n_par, n):
    """41 held-out data that are not in the sampler's own 16, two kept chains scored on the same matrix; sine3: 55
    samples, more than the 51 rows of a tile at n_par 10.  pointwise_loglike_at is pointwise_loglike of a sampler that
    holds those data, bit for bit"""
    rows, held, own = model_case(model, n_par, n)
    s = HipSampler(model, n_par, 2, own, seed=1)
    pw, jt = at_fold(s, rows, [0, 1], held, [7, n - 7])
    terms = s.pointwise_loglike_at(rows[:5, 1, :n_par], held[:, 0], held[:, 1])
    one = s.pointwise_loglike_at(rows[3, 1, :n_par], held[:, 0], held[:, 1])
    s.close()
    other = HipSampler(model, n_par, 1, held, seed=1)
    want = other.pointwise_loglike(rows[:5, 1, :n_par])
    other.close()
    assert terms.shape == (5, 41) and terms.tobytes() == want.tobytes() and one.tobytes() == terms[3].tobytes()
    r = RefPointwise(model, rows, [0, 1], held)
    assert r.finite.all() and pw.origin.shape == (2, 41) and pw.x[1].tobytes() == held[:, 0].tobytes()
    delta = None if model in SINE else pulse_delta(model, rows, [0, 1], held, r.values)
    check(pw, r, model, "model %d" % model, delta)
    for k in range(2):
        check_joint(jt, k, r.values[:, k, :], "model %d" % model, None if delta is None else delta[:, k, :])
    assert pw.origin[1].tobytes() == terms[0].tobytes() and np.isfinite(jt.lpd()).all()


# ---- 4. call boundaries ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip0,thin", [(2, 1), (1, 3), (5, 4)])
def test_every_cut_of_the_calls_gives_the_same_bits(skip0, thin):
    """300 steps cut at 7: two calls, a get between the calls, and get / end / begin / set / joint_set and the rest, each
    against the fold in one call, which is held to the reference"""
    rows, held, own = flat_case()
    mats = mats4(held)
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 6, own, seed=1)
    whole, whole_j = at_fold(s, rows, KEPT4, mats, None, skip0, thin)
    cut, cut_j = at_fold(s, rows, KEPT4, mats, [7, N_BIG - 7], skip0, thin)
    d = on_device(rows)
    first_kept = [t for t in range(skip0, 7, thin)]
    nxt = first_kept[-1] + thin
    s.pointwise_begin(chains=KEPT4, thin=thin, at=mats, joint=True)
    s.pointwise_accumulate(d.data_ptr(), 7, skip0, thin)
    half, half_j = s.pointwise(), s.pointwise_joint()         # a get between the calls
    s.pointwise_accumulate(d.data_ptr(), N_BIG, nxt, thin)
    between, between_j = s.pointwise(), s.pointwise_joint()
    s.pointwise_end()
    s.pointwise_begin(chains=KEPT4, thin=thin, at=mats, joint=True)
    s.pointwise_set(half)
    s.pointwise_joint_set(half_j)
    s.pointwise_accumulate(d.data_ptr(), N_BIG, nxt, thin)
    resumed, resumed_j = s.pointwise(), s.pointwise_joint()
    s.pointwise_end()
    s.close()
    kept = rows[skip0::thin]
    assert int(whole.n[0]) == len(kept) and int(half.n[0]) == len(first_kept) == int(half_j.n[0])
    check_four(whole, whole_j, kept, held, "skip %d thin %d" % (skip0, thin))
    for what, pw, jt in (("two calls", cut, cut_j), ("a get between", between, between_j), ("resumed", resumed, resumed_j)):
        assert_same_state(pw, whole, what)
        assert_same_joint(jt, whole_j, what)
        assert pw.lengths.tolist() == LENS4 and pw.thin == thin


def test_several_pieces_in_one_call():
    """kPointwisePiece + 3 kept samples at n_at = 3: the fold's piece boundary is the joint kernels' too"""
    n = PIECE + 3
    rng = np.random.default_rng(6)
    held = np.array([[100.0, 0.31], [100.5, 1.77], [2.45e6, -0.4]])
    own = np.array([[7.0, 0.1], [8.0, 0.2]])
    rows = np.zeros((n, 1, 6))
    rows[:, 0, :4] = [0.0, 0.2, 0.4, 0.0]
    rows[:, 0, 3] = 0.5 + 0.3 * rng.standard_normal(n)
    vals = flat_values(rows, 0, held)
    some = np.concatenate([np.arange(4), PIECE - 2 + np.arange(5)])
    assert vals[some].tobytes() == ref.terms(wl.MODEL_SIMPLESIN, rows[some, 0, :4], held, 0.5).tobytes()
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 1, own, seed=1)
    pw, jt = at_fold(s, rows, (0,), [held])
    again, again_j = at_fold(s, rows, (0,), [held], [PIECE - 3, 5, 1])
    s.close()
    check(pw, RefPointwise(wl.MODEL_SIMPLESIN, rows, [0], held, values=vals[:, None, :]), wl.MODEL_SIMPLESIN, "two pieces")
    check_joint(jt, 0, vals, "two pieces")
    assert_same_state(again, pw, "cut elsewhere")
    assert_same_joint(again_j, jt, "cut elsewhere")


# ---- 5. a non-finite parameter stays in its kept chain ------------------------------------------------------------------------------
def test_a_nan_parameter_stays_in_its_kept_chain():
    rows, held, own = flat_case()
    rows = rows[:70]
    bad = rows.copy()
    bad[66, KEPT4[1], 1] = np.nan                             # a NaN frequency in one sample of the second kept chain
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 6, own, seed=1)
    clean, clean_j = at_fold(s, rows, KEPT4, mats4(held), [3, 67])
    got, got_j = at_fold(s, bad, KEPT4, mats4(held), [3, 67])
    s.close()
    for k in (0, 2, 3):
        for f in STATE:
            assert getattr(got, f)[k].tobytes() == getattr(clean, f)[k].tobytes(), (k, f)
        for f in JOINT:
            assert bits(getattr(got_j, f)[k]) == bits(getattr(clean_j, f)[k]), (k, f)
    for f in ("sum", "sq", "S"):
        assert np.isnan(getattr(got_j, f)[1]), f
    assert bits(got_j.origin[1]) == bits(clean_j.origin[1]) and np.isfinite(got_j.m[1])       # a NaN never moves a maximum
    vals = flat_values(rows, KEPT4[1], held[:65])
    vals[66] = np.nan
    r = check_joint(got_j, 1, vals, "a NaN frequency")
    assert not r.finite and math.isnan(r.S) and np.isnan(got.sum[1, :65]).all()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    rows, held, own = flat_case()
    rows = rows[:12]
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 6, own, seed=1)
    L = capi.lib()
    ip = C.POINTER(C.c_int32)
    ch = np.array([0, 2], dtype=np.int32)
    cfg = capi.PointwiseConfig(n_keep=2, chains=ch.ctypes.data_as(ip))
    n_at = np.array([3, 2], dtype=np.int32)
    x, y = np.ascontiguousarray(held[:5, 0]), np.ascontiguousarray(held[:5, 1])
    dp = capi._dp

    def at(**kw):
        a = dict(n_at=n_at.ctypes.data_as(ip), x=x.ctypes.data_as(dp), y=y.ctypes.data_as(dp), joint=0)
        a.update(kw)
        return capi.PointwiseAt(**a)
    jt = kfold.Joint.empty(ch, n_at)
    assert L.apemost_hip_pointwise_begin_at(s._h, C.byref(cfg), None) == capi.ERR_INVALID
    assert b"at is NULL" in L.apemost_hip_last_error()
    assert L.apemost_hip_pointwise_begin_at(s._h, None, C.byref(at())) == capi.ERR_INVALID
    for name in ("n_at", "x", "y"):
        assert L.apemost_hip_pointwise_begin_at(s._h, C.byref(cfg), C.byref(at(**{name: None}))) == capi.ERR_INVALID
        assert ("at->%s is NULL" % name).encode() in L.apemost_hip_last_error(), name
    n_at[1] = 0
    assert L.apemost_hip_pointwise_begin_at(s._h, C.byref(cfg), C.byref(at())) == capi.ERR_INVALID
    assert b"n_at[1] = 0" in L.apemost_hip_last_error()
    n_at[1] = 2
    assert L.apemost_hip_pointwise_begin_at(s._h, C.byref(cfg), C.byref(at(joint=2))) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_joint_get(s._h, C.byref(jt.view())) == capi.ERR_INVALID       # nothing was begun
    # a fold without joint has no joint state, at the caller's data or at the sampler's
    assert L.apemost_hip_pointwise_begin_at(s._h, C.byref(cfg), C.byref(at())) == capi.OK
    for call in (L.apemost_hip_pointwise_joint_get, L.apemost_hip_pointwise_joint_set):
        assert call(s._h, C.byref(jt.view())) == capi.ERR_INVALID and b"joint = 1" in L.apemost_hip_last_error()
    # the tail on unequal n_at is refused as on a ragged batch
    assert L.apemost_hip_pointwise_tail_begin(s._h, 4) == capi.ERR_UNSUPPORTED
    s.pointwise_end()
    s.pointwise_begin(chains=ch)
    assert L.apemost_hip_pointwise_joint_get(s._h, C.byref(jt.view())) == capi.ERR_INVALID
    s.pointwise_end()
    with pytest.raises(ValueError):
        s.pointwise_begin(chains=ch, joint=True)
    with pytest.raises(ValueError):
        s.pointwise_begin(chains=ch, at=[held[:3]])
    # accumulate after a pointwise_set that loaded samples waits for pointwise_joint_set
    d = on_device(rows)
    mats = [held[:3], held[3:5]]
    part, part_j = at_fold(s, rows[:5], ch, mats)
    whole, whole_j = at_fold(s, rows, ch, mats)
    s.pointwise_begin(chains=ch, at=mats, joint=True)
    s.pointwise_set(part)
    assert L.apemost_hip_pointwise_accumulate(s._h, d[5:].data_ptr(), 7, 0, 1) == capi.ERR_INVALID
    assert b"pointwise_joint_set" in L.apemost_hip_last_error()
    stale = kfold.Joint.empty(ch, n_at)
    stale.n[0] = 4
    assert L.apemost_hip_pointwise_joint_set(s._h, C.byref(stale.view())) == capi.ERR_INVALID  # another count of samples
    s.pointwise_joint_set(part_j)
    s.pointwise_accumulate(d[5:].data_ptr(), 7)
    got, got_j = s.pointwise(), s.pointwise_joint()
    assert_same_state(got, whole, "resumed")
    assert_same_joint(got_j, whole_j, "resumed")
    # begin and end drop the joint state
    s.pointwise_begin(chains=ch)
    assert L.apemost_hip_pointwise_joint_get(s._h, C.byref(jt.view())) == capi.ERR_INVALID
    s.pointwise_end()
    assert L.apemost_hip_pointwise_joint_get(s._h, C.byref(jt.view())) == capi.ERR_INVALID
    # DIC has no held-out meaning
    with pytest.raises(ValueError, match="held-out"):
        whole.per_ladder(2)[0].dic()
    with pytest.raises(ValueError):
        whole.per_ladder(2)[1].p_dic()
    # loglike_at
    out, par = np.zeros((2, 5)), np.zeros((2, 4))
    ll = L.apemost_hip_pointwise_loglike_at
    a = [par.ctypes.data_as(dp), 5, x.ctypes.data_as(dp), y.ctypes.data_as(dp), out.ctypes.data_as(dp)]
    assert ll(s._h, 0, *a) == capi.ERR_INVALID and ll(s._h, 2, a[0], 0, *a[2:]) == capi.ERR_INVALID
    for j in (0, 2, 3, 4):
        assert ll(s._h, 2, *[None if i == j else v for i, v in enumerate(a)]) == capi.ERR_INVALID, j
    assert ll(s._h, 2, *a) == capi.OK                         # needs no fold
    s.close()


def test_a_tail_on_equal_lengths():
    """all n_at equal: the tail is allowed and holds, per series, the largest -l over pointwise_loglike_at's terms"""
    rows, held, own = flat_case()
    rows = rows[:12]
    chains, mats, cap = [1, 4], [held[:41], held[41:82]], 4
    s = HipSampler(wl.MODEL_SIMPLESIN, 4, 6, own, seed=1)
    d = on_device(rows)
    s.pointwise_begin(chains=chains, at=mats, joint=True, tail=cap)
    feed(s, d, [5, 7])
    pw, tail, jt = s.pointwise(), s.pointwise_tail(), s.pointwise_joint()
    s.pointwise_end()
    terms = [s.pointwise_loglike_at(rows[:, c, :4], m[:, 0], m[:, 1]) for c, m in zip(chains, mats)]
    s.close()
    assert pw.lengths is None and tail.count.shape == (2, 41) and (tail.count == cap).all() and int(jt.n[0]) == 12
    for k in range(2):
        want = -np.sort(terms[k], axis=0)[:cap].T             # [41][cap]: the largest x = -l, descending
        assert tail.values[k].tobytes() == np.ascontiguousarray(want).tobytes(), k
        assert pw.m_dn[k].tobytes() == want[:, 0].tobytes() and pw.origin[k].tobytes() == terms[k][0].tobytes()


def test_a_user_model_is_refused():
    rs = np.random.RandomState(5)
    data = np.column_stack([(rs.uniform(size=64) < 0.5).astype(float), rs.normal(0, 1, (64, 2))])
    s = HipSampler(wl.MODEL_USER, 3, 5, data, seed=1,
                   device_model_source=os.path.join(hostlib.HOST, "examples", "device_models", "bernoulli_example.hip"))
    with pytest.raises(capi.ApemostHipError, match="user-supplied") as e:
        s.pointwise_begin(chains=(0,), at=[data[:4, :2]])
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ApemostHipError, match="user-supplied") as e:
        s.pointwise_loglike_at(np.zeros(3), data[:4, 0], data[:4, 1])
    assert e.value.code == capi.ERR_UNSUPPORTED
    s.close()


# ---- 7. K-fold end to end -------------------------------------------------------------------------------------------------------------
PER, LAUNCHES, STEPS = 4, 5, 60


def test_kfold_end_to_end():
    """simplesin, 10 data, K = 3 interleaved: held-out sets of 4, 3, 3 rows, training sets of 6, 7, 7; 4 chains per
    ladder, 300 steps without swap attempts"""
    from tests.test_gpu_ragged_batch import concat
    w = wl.simplesin(n_data=10, n_chain=PER, seed=500)
    data = w.data
    fs = kfold.folds(10, 3)
    sets = kfold.training_sets(data, fs)
    assert [len(f) for f in fs] == [4, 3, 3] and [len(m) for m in sets] == [6, 7, 7]
    seeds = [1000 + 13 * b for b in range(3)]
    sts = []
    for b, m in enumerate(sets):
        wb = wl.simplesin(n_data=len(m), n_chain=PER, seed=500)
        wb.data = m
        st, _, _ = make_pair(wb, PER, beta_0=0.02 + 0.01 * b, seed=seeds[b])
        assert st.beta[0] == 1.0
        sts.append(st)
    n_steps = LAUNCHES * STEPS

    def run(s, n_chains, with_fold):
        d = torch.zeros((LAUNCHES, STEPS, n_chains, w.n_par + 2), dtype=torch.float64, device="cuda")
        for k in range(LAUNCHES):
            s.launch_rounds(1, STEPS, False, d[k].data_ptr())
            if with_fold:
                s.pointwise_accumulate(d[k].data_ptr(), STEPS)
        cv = kfold.result(s, fs) if with_fold else None
        s.synchronize()
        return s.get_state(), d.cpu().numpy().reshape(n_steps, n_chains, w.n_par + 2), cv

    out = []
    for with_fold in (True, False):
        s = kfold.sampler(w.model, w.n_par, PER, data, fs, seeds, waves_per_chain=1)
        assert s.n_ladders == 3 and s.n_data_per_ladder == [6, 7, 7] and s.chains_per_ladder == PER
        s.set_state(concat(sts))
        if with_fold:
            kfold.begin(s, data, fs)
        st, rows, cv = run(s, 3 * PER, with_fold)
        if with_fold:
            pw, jt = s.pointwise(), s.pointwise_joint()
            terms = [s.pointwise_loglike_at(rows[:, b * PER, :w.n_par], data[f, 0], data[f, 1]) for b, f in enumerate(fs)]
            s.pointwise_end()
        out.append((st, rows, cv))
        s.close()
    # the run with the fold is the run without, bit for bit
    for f in ALL_FIELDS:
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()
    st, rows, cv = out[0]
    # ladder b is the stand-alone sampler of training set b under seeds[b], bit for bit: the ragged batch's own guarantee
    alone_rows = []
    for b in range(3):
        alone = HipSampler(w.model, w.n_par, PER, sets[b], seed=seeds[b], waves_per_chain=1)
        alone.set_state(sts[b])
        _, r, _ = run(alone, PER, False)
        alone.close()
        alone_rows.append(r)
    assert np.concatenate(alone_rows, axis=1).tobytes() == rows.tobytes()
    # the fold against the reference over the dumped rows and the held-out matrices
    assert int(pw.n[0]) == n_steps and pw.lengths.tolist() == [4, 3, 3] and pw.chains.tolist() == [0, PER, 2 * PER]
    for b, (one, f) in enumerate(zip(pw.per_ladder(3), fs)):
        r = RefPointwise(w.model, rows, [b * PER], data[f])
        assert r.finite.all()
        check(one, r, w.model, "fold %d" % b)
        assert terms[b].tobytes() == r.values[:, 0, :].tobytes()
        rj = check_joint(jt, b, terms[b], "fold %d" % b)
        assert rj.finite
    # KFold is numpy over that state, in the original order of the data
    assert cv.n == n_steps and cv.k == 3 and cv.has_joint and cv.fold_of.tolist() == [0, 1, 2, 0, 1, 2, 0, 1, 2, 0]
    assert cv.x.tobytes() == data[:, 0].tobytes() and cv.y.tobytes() == data[:, 1].tobytes()
    want = np.zeros(10)
    for b, f in enumerate(fs):
        want[f] = [pw.m_up[b, j] + math.log(pw.S_up[b, j] / n_steps) for j in range(len(f))]
    assert cv.elpd_i.tobytes() == want.tobytes() and np.isfinite(want).all()
    assert cv.lpd_joint.tolist() == [float(jt.m[b]) + math.log(float(jt.S[b]) / n_steps) for b in range(3)]
    assert cv.joint_mean.tolist() == (jt.origin + jt.sum / n_steps).tolist() and (cv.joint_var > 0).all()
    assert cv.se > 0 and cv.compare(cv) == (0.0, 0.0)
    # the joint density of a block is not the sum of its pointwise densities
    assert all(cv.lpd_joint[b] != sum(cv.elpd_i[f]) for b, f in enumerate(fs))
