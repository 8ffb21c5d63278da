"""The optional hooks of a user-supplied device model (include/apemost_device_model.h: apemost_user_curve,
apemost_user_pointwise) on the device: apemost_hip_predict_* and apemost_hip_pointwise_* for APEMOST_MODEL_USER
(apemost_amd/csrc/pt_user_fold.h, a second run-time module).

The folds are the built-in models' and are held to the built-in models' rules: every field of a Predict equals
tests/predict_ref.py's sequential loops with == on the bits (predict_ref.assert_equals), and a Pointwise is compared by
tests/test_gpu_pointwise.py's `check` in its exact form -- origin, sum, sq, m_up, m_dn and the parameter sums with ==
on the bits, the S words to n 2^-50 and n 2^-49 -- because the restatements are handed the values (`values=`) that the
fold folds: a numpy float64 restatement where the hooks use only + - * / (bit for bit: IEEE operations, contraction
off), the device's own predict_curve / pointwise_loglike where they call the math library.

The values of the shipped examples against numpy, u = 2^-53.  Both sides perform the same IEEE operations on the same
inputs, so they differ only through the library calls: each side's sin, exp and log is within one ulp (2 u relative)
of the true value, every later arithmetic operation adds half an ulp (u relative) per side, and an error already there
is propagated through the operation.  With the factor 2 that tests/test_gpu_pointwise.py gives every such bound:
  simplesin2_hooks   w = 2 pi (f x + 0.3312) is the same double on both sides;  s = sin(w): ds = 4 u |s|;
                     v = a s: dv = |a| ds + 2 u |v|;  r = v - y: dr = dv + 2 u |r|;  q = r r: dq = 2 |r| dr + dr^2 +
                     2 u q;  l = q c (c is arithmetic only, the same double): dl = |c| dq + 2 u |l|.
  bernoulli_hooks    eta is the same double on both sides.  eta > 0: e = exp(-eta): de = 4 u e;  d = 1 + e: dd = de +
                     2 u d;  p = 1 / d: dp = dd / (d (d - dd)) + 2 u p.  Otherwise e = exp(eta), d as before, p = e / d:
                     dp = de / (d - dd) + e dd / (d (d - dd)) + 2 u p.  The term is L = log(m) with m = p or m = 1 - p
                     (dm = dp + 2 u m): dL = dm / (m - dm) + 4 u |L|  (|log(m + t) - log m| <= t / (m - t)).
                     Regressors and parameters lie in [-1, 1] with two regressors and an intercept, so |eta| <= 3 and
                     m >= 1 / (1 + e^3) = 0.047: no cancellation empties the bound.

What cannot be built: a user-supplied model does not run in ladder batches (apemost_hip_create_batch refuses it, by
design: DESIGN 5.10), so there is no batch of user ladders to fold over; that the refusal stands is asserted."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.pointwise import Pointwise
from apemost_amd.predict import PIECE, Predict
from apemost_amd.sampler import HipSampler
from apemost_amd.state import LadderState
from tests import hostlib
from tests.pointwise_ref import RefPointwise, assert_same_state
from tests.predict_ref import RefPredict, assert_equals
from tests.test_gpu_pointwise import check as check_pointwise

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
MODELS = os.path.join(hostlib.HOST, "examples", "device_models")
SINE2 = os.path.join(MODELS, "simplesin2_hooks.hip")
BERNOULLI = os.path.join(MODELS, "bernoulli_hooks.hip")
SIN, EXP, LOG = np.vectorize(math.sin), np.vectorize(math.exp), np.vectorize(math.log)   # the C library's, elementwise
EXACT_RULE = wl.MODEL_SIMPLESIN                               # check_pointwise's form for values that are bit for bit

# A Gaussian line (two parameters; with a third a parabola), + - * / only, every operation its own statement.
LINE_BASE = '''#include "apemost_device_model.h"
static __device__ double line_value(const apemost_model_ctx *ctx, int i) {
    const double x = APEMOST_DATA(ctx, i, 0);
    const double bx = ctx->params[1] * x;
    double v = ctx->params[0] + bx;
    if (ctx->n_par > 2) {
        const double xx = x * x;
        const double cxx = ctx->params[2] * xx;
        v = v + cxx;
    }
    return v;
}
static __device__ double line_term(const apemost_model_ctx *ctx, int i) {
    const double c = 1.0 / ((-2.0 * ctx->sigma) * ctx->sigma);
    const double r = line_value(ctx, i) - APEMOST_DATA(ctx, i, 1);
    const double q = r * r;
    return q * c;
}
__device__ double apemost_user_term(const apemost_model_ctx *ctx, int i) { return line_term(ctx, i); }
__device__ double apemost_user_finish(const apemost_model_ctx *ctx, double sum, double beta, double *prior) {
    (void)ctx;
    (void)prior;
    return beta * sum;
}
'''
LINE_CURVE = '''#define APEMOST_USER_CURVE 1
__device__ double apemost_user_curve(const apemost_model_ctx *ctx, int i) { return line_value(ctx, i); }
'''
LINE_POINTWISE = '''#define APEMOST_USER_POINTWISE 1
__device__ double apemost_user_pointwise(const apemost_model_ctx *ctx, int i) { return line_term(ctx, i); }
'''
SIGMA = 0.37


@pytest.fixture(scope="module")
def line_src(tmp_path_factory):
    p = tmp_path_factory.mktemp("user_hooks") / "line.hip"
    p.write_text(LINE_BASE + LINE_CURVE + LINE_POINTWISE)
    return str(p)


def line_values(params, data):
    """numpy's float64 restatement of line_value and line_term: ([...][n_data], [...][n_data]) for params [...][n_par]"""
    p = np.asarray(params, dtype=np.float64)[..., None, :]
    x, y = data[:, 0], data[:, 1]
    bx = p[..., 1] * x
    v = p[..., 0] + bx
    if p.shape[-1] > 2:
        xx = x * x
        cxx = p[..., 2] * xx
        v = v + cxx
    c = np.float64(1.0) / ((np.float64(-2.0) * np.float64(SIGMA)) * np.float64(SIGMA))
    r = v - y
    q = r * r
    return v, q * c


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def feed(s, which, d, calls, skip0=0, thin=1):
    """accumulate d in calls of the given numbers of steps; the kept steps are skip0, skip0 + thin, ... of the whole"""
    off = 0
    for n in calls:
        skip = skip0 - off if off < skip0 else (thin - (off - skip0) % thin) % thin
        getattr(s, which + "_accumulate")(d[off:].data_ptr(), n, skip, thin)
        off += n
    assert off == d.shape[0]


def both_folds(s, rows, chains, calls=None, skip0=0, thin=1, nbins=0, lo=None, hi=None, x=None):
    """(Predict, Pointwise) of the device rows, both folds open at once"""
    d = on_device(rows)
    s.predict_begin(chains=chains, x=x, nbins=nbins, lo=lo, hi=hi, thin=thin)
    s.pointwise_begin(chains=chains, thin=thin)
    for which in ("predict", "pointwise"):
        feed(s, which, d, calls or [len(rows)], skip0, thin)
    pr, pw = s.predict(), s.pointwise(at_mean=False)
    s.predict_end()
    s.pointwise_end()
    return pr, pw


def line_rows(n_steps, n_chains, n_par, seed):
    """parameter rows around a = 0.4, b = 0.01 (c = 1e-5) with noise; prob has a tie at its maximum in chain 0"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n_steps, n_chains, n_par + 2))
    rows[:, :, :n_par] = np.array([0.4, 0.01, 1e-5][:n_par]) * (1 + 0.2 * rng.standard_normal((n_steps, n_chains, n_par)))
    rows[:, :, n_par] = -100 + rng.uniform(size=(n_steps, n_chains))
    rows[:, :, n_par + 1] = rows[:, :, n_par] + 1
    if n_steps > 22:
        rows[[7, 22], 0, n_par] = -50.0
    return rows


def line_data(n_data, seed=3):
    rng = np.random.default_rng(seed)
    x = np.concatenate([100 + 0.5 * np.arange(128), [2.45e3 + 0.5, -3.25]])[:n_data]
    return np.stack([x, 1.5 + rng.uniform(-1, 2, n_data)], 1)


def kept_values(rows, chains, n_par, data):
    """the restatement's curves and terms [n][n_keep][n_data] of the kept chains"""
    v, l = line_values(rows[:, chains, :n_par], data)
    return v, l


CHAINS = [0, 3]


# ---- 1. bit for bit ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_data", [1, 63, 64, 65, 130])
def test_arithmetic_hooks_bit_for_bit_at_every_data_size(line_src, n_data):
    """one lane, a wave less one, a full wave, a wave and one, three workgroups with a ragged last one; 40 kept steps of
    5 chains, two of them kept; histograms over a range that leaves some values outside"""
    data, rows = line_data(n_data), line_rows(40, 5, 2, seed=1)
    s = HipSampler(wl.MODEL_USER, 2, 5, data, seed=1, sigma=SIGMA, device_model_source=line_src)
    assert s.user_hooks[:2] == (True, True)
    par = rows[:7, 1, :2]
    want_v, want_l = line_values(par, data)
    got_v, got_l = s.predict_curve(par), s.pointwise_loglike(par)
    assert got_v.shape == (7, n_data) and got_v.tobytes() == want_v.tobytes()
    assert got_l.tobytes() == want_l.tobytes() and (want_l < 0).all()
    assert s.predict_curve(par[2]).tobytes() == want_v[2].tobytes()
    v, l = kept_values(rows, CHAINS, 2, data)
    lo, hi = float(np.quantile(v, 0.1)), float(np.quantile(v, 0.9))
    pr, pw = both_folds(s, rows, CHAINS, nbins=37, lo=lo, hi=hi)
    s.close()
    assert pr.model == pw.model == wl.MODEL_USER and pr.x[1].tobytes() == data[:, 0].tobytes()
    assert pw.y[0].tobytes() == data[:, 1].tobytes()
    ref = RefPredict(None, rows, CHAINS, data[:, 0], 37, lo, hi, values=v)
    assert_equals(pr, ref, "n_data %d" % n_data)
    assert 0 < int(pr.hist.sum()) < 40 * 2 * n_data
    r = RefPointwise(None, rows, CHAINS, data, SIGMA, values=l)
    assert r.finite.all()
    check_pointwise(pw, r, EXACT_RULE, "n_data %d" % n_data)


# ---- 2. every call boundary ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("skip0,thin", [(0, 1), (3, 1), (0, 5), (3, 5)])
def test_call_boundaries_skip_and_thin(line_src, skip0, thin):
    """65 data, 60 steps in calls of 1, 7 and the rest: the state of one call, which is the restatement's"""
    data, rows = line_data(65), line_rows(60, 5, 2, seed=2)
    s = HipSampler(wl.MODEL_USER, 2, 5, data, seed=1, sigma=SIGMA, device_model_source=line_src)
    pr, pw = both_folds(s, rows, CHAINS, [1, 7, 52], skip0, thin, nbins=16, lo=1.0, hi=2.5)
    pr1, pw1 = both_folds(s, rows, CHAINS, None, skip0, thin, nbins=16, lo=1.0, hi=2.5)
    s.close()
    assert_equals(pr, pr1, "one call")
    assert_same_state(pw, pw1, "one call")
    kept = rows[skip0::thin]
    v, l = kept_values(kept, CHAINS, 2, data)
    assert int(pr.n[0]) == len(kept) and pr.thin == pw.thin == thin
    assert_equals(pr, RefPredict(None, kept, CHAINS, data[:, 0], 16, 1.0, 2.5, values=v), "skip %d thin %d" % (skip0, thin))
    check_pointwise(pw, RefPointwise(None, kept, CHAINS, data, SIGMA, values=l), EXACT_RULE, "skip %d thin %d" % (skip0, thin))


def test_two_pieces_in_one_call(line_src):
    """8192 + 9 kept steps of one chain at 3 data: the second piece continues the first"""
    n = PIECE + 9
    data, rows = line_data(3), line_rows(n, 1, 2, seed=3)
    s = HipSampler(wl.MODEL_USER, 2, 1, data, seed=1, sigma=SIGMA, device_model_source=line_src)
    pr, pw = both_folds(s, rows, [0])
    s.close()
    v, l = kept_values(rows, [0], 2, data)
    assert int(pr.n[0]) == int(pw.n[0]) == n
    assert_equals(pr, RefPredict(None, rows, [0], data[:, 0], values=v), "two pieces")
    check_pointwise(pw, RefPointwise(None, rows, [0], data, SIGMA, values=l), EXACT_RULE, "two pieces")


def test_three_parameters_cross_a_tile(line_src):
    """a tile holds 512 // 3 = 170 parameter rows: 345 kept steps read three tiles, the last one partly filled, and the
    tile's rows do not divide by the four samples taken side by side"""
    data, rows = line_data(65), line_rows(345, 2, 3, seed=4)
    s = HipSampler(wl.MODEL_USER, 3, 2, data, seed=1, sigma=SIGMA, device_model_source=line_src)
    pr, pw = both_folds(s, rows, [1], [100, 245])
    s.close()
    v, l = kept_values(rows, [1], 3, data)
    assert_equals(pr, RefPredict(None, rows, [1], data[:, 0], values=v), "n_par 3")
    check_pointwise(pw, RefPointwise(None, rows, [1], data, SIGMA, values=l), EXACT_RULE, "n_par 3")


# ---- 3. the shipped examples ------------------------------------------------------------------------------------------------------
def sine2_case(n_data=70, n_steps=40):
    rng = np.random.default_rng(11)
    x = 100 + 0.5 * np.arange(n_data)
    data = np.stack([x, 0.8 * np.sin(2 * np.pi * (0.21 * x + 0.3312)) + rng.normal(0, 0.5, n_data)], 1)
    rows = np.zeros((n_steps, 5, 4))
    rows[:, :, :2] = np.array([0.9, 0.2]) + np.array([0.05, 1e-4]) * rng.standard_normal((n_steps, 5, 2))
    rows[:, :, 2] = -100 + rng.uniform(size=(n_steps, 5))
    rows[:, :, 3] = rows[:, :, 2]
    return data, rows


def sine2_numpy(params, data, sigma):
    """-> curve, term, and their bounds (module docstring), [...][n_data] each"""
    p = np.asarray(params, dtype=np.float64)[..., None, :]
    x, y = data[:, 0], data[:, 1]
    w = (2.0 * 3.14159265358979323846) * (p[..., 1] * x + 0.3312)
    s = SIN(w)
    v = p[..., 0] * s
    c = np.float64(1.0) / ((np.float64(-2.0) * np.float64(sigma)) * np.float64(sigma))
    r = v - y
    q = r * r
    l = q * c
    dv = np.abs(p[..., 0]) * (4 * U * np.abs(s)) + 2 * U * np.abs(v)
    dr = dv + 2 * U * np.abs(r)
    dq = 2 * np.abs(r) * dr + dr * dr + 2 * U * q
    return v, l, dv, abs(c) * dq + 2 * U * np.abs(l)


def bernoulli_case(n_data=70, n_steps=40):
    """the outcome and two regressors in [-1, 1]; an intercept and two slopes in [-1, 1]"""
    rng = np.random.default_rng(12)
    X = rng.uniform(-1, 1, (n_data, 2))
    out = (rng.uniform(size=n_data) < 1 / (1 + np.exp(-(0.3 + 0.9 * X[:, 0] - 0.7 * X[:, 1])))).astype(float)
    data = np.column_stack([out, X])
    rows = np.zeros((n_steps, 5, 5))
    rows[:, :, :3] = rng.uniform(-1, 1, (n_steps, 5, 3))
    rows[:, :, 3] = -100 + rng.uniform(size=(n_steps, 5))
    rows[:, :, 4] = rows[:, :, 3]
    return data, rows


def bernoulli_numpy(params, data):
    """-> p, term, and their bounds (module docstring), [...][n_data] each"""
    par = np.asarray(params, dtype=np.float64)[..., None, :]
    eta = par[..., 0] + np.zeros(len(data))
    for j in (1, 2):
        eta = eta + data[:, j] * par[..., j]
    assert np.abs(eta).max() <= 3
    pos = eta > 0
    e = EXP(np.where(pos, -eta, eta))
    d = 1 + e
    p = np.where(pos, 1 / d, e / d)
    de = 4 * U * e
    dd = de + 2 * U * d
    dp = np.where(pos, dd / (d * (d - dd)), de / (d - dd) + e * dd / (d * (d - dd))) + 2 * U * p
    zero = data[:, 0] == 0
    m = np.where(zero, 1 - p, p)
    assert m.min() >= 0.047
    dm = dp + np.where(zero, 2 * U * m, 0.0)
    L = LOG(m)
    return p, L, dp, dm / (m - dm) + 4 * U * np.abs(L)


EXAMPLES = {"simplesin2_hooks": (SINE2, 2, sine2_case, lambda p, data: sine2_numpy(p, data, 0.5)),
            "bernoulli_hooks": (BERNOULLI, 3, bernoulli_case, bernoulli_numpy)}


@pytest.mark.parametrize("name", sorted(EXAMPLES))
def test_shipped_examples(name):
    """70 data (bernoulli: three columns).  The device's own curves and terms of the kept rows, handed to the
    restatements, fix the fold by the existing rules; the curves and terms themselves lie within the module's bounds of
    numpy's, with the rule's factor 2; and the sum of a row's terms is the engine's log-likelihood at beta = 1 to the
    1e-12 relative of tests/test_gpu_pointwise.py"""
    src, n_par, case, restate = EXAMPLES[name]
    data, rows = case()
    s = HipSampler(wl.MODEL_USER, n_par, 5, data, seed=1, device_model_source=src)
    assert s.user_hooks[:2] == (True, True)
    par = np.ascontiguousarray(rows[:, CHAINS, :n_par]).reshape(-1, n_par)
    v = s.predict_curve(par).reshape(len(rows), len(CHAINS), -1)
    l = s.pointwise_loglike(par).reshape(len(rows), len(CHAINS), -1)
    lo, hi = float(np.quantile(v, 0.05)), float(np.quantile(v, 0.95))
    pr, pw = both_folds(s, rows, CHAINS, [1, 7, 32], nbins=20, lo=lo, hi=hi)
    prob, prior = s.loglike(par, np.ones(len(par)))
    s.close()
    assert_equals(pr, RefPredict(None, rows, CHAINS, data[:, 0], 20, lo, hi, values=v), name)
    r = RefPointwise(None, rows, CHAINS, data, 0.5, values=l)
    assert r.finite.all()
    check_pointwise(pw, r, EXACT_RULE, name)
    want_v, want_l, dv, dl = restate(rows[:, CHAINS, :n_par], data)
    frac_v = float(np.max(np.abs(v - want_v) / (2 * dv)))
    frac_l = float(np.max(np.abs(l - want_l) / (2 * dl)))
    print("%s: curve %.3g and term %.3g of their bounds" % (name, frac_v, frac_l))
    assert np.isfinite(want_v).all() and np.isfinite(want_l).all() and frac_v <= 1 and frac_l <= 1
    # 4. the sum against the engine: prob - prior = beta * loglike at beta = 1 (simplesin2 sets no prior: prob itself)
    total = np.array([math.fsum(t) for t in l.reshape(len(par), -1).tolist()])
    engine = prob if name == "simplesin2_hooks" else prob - prior
    worst = float(np.max(np.abs(total - engine) / np.abs(engine)))
    print("%s: sum of the terms against the engine's log-likelihood: worst relative difference %.3g" % (name, worst))
    assert worst <= 1e-12


# ---- 5. a caller's grid --------------------------------------------------------------------------------------------------------------
def test_a_callers_grid_of_rows():
    """bernoulli_hooks, 70 data of 3 columns; a grid of 65 rows [n_x][n_cols] that are not the data.  The grid's curves
    are those of a sampler whose data is the grid (the upload by columns is right), and the fold over the grid equals
    the restatement fed with them"""
    data, rows = bernoulli_case()
    rng = np.random.default_rng(21)
    grid = np.column_stack([np.zeros(65), rng.uniform(-1, 1, (65, 2))])
    s = HipSampler(wl.MODEL_USER, 3, 5, data, seed=1, device_model_source=BERNOULLI)
    on_grid = HipSampler(wl.MODEL_USER, 3, 1, grid, seed=1, device_model_source=BERNOULLI)
    par = np.ascontiguousarray(rows[:, CHAINS, :3]).reshape(-1, 3)
    v = s.predict_curve(par, grid)
    assert v.shape == (len(par), 65) and v.tobytes() == on_grid.predict_curve(par).tobytes()
    want, _, dp, _ = bernoulli_numpy(par, grid)
    assert float(np.max(np.abs(v - want) / (2 * dp))) <= 1
    on_grid.close()
    d = on_device(rows)
    s.predict_begin(chains=CHAINS, x=grid, nbins=10, lo=0.2, hi=0.8)
    s.predict_accumulate(d.data_ptr(), len(rows))
    pr = s.predict()
    s.predict_end()
    assert pr.n_x == 65 and pr.x[0].tobytes() == grid[:, 0].tobytes()
    assert_equals(pr, RefPredict(None, rows, CHAINS, grid[:, 0], 10, 0.2, 0.8, values=v.reshape(len(rows), 2, 65)), "grid")
    # a non-finite entry anywhere in the rows (here in the last column, beyond the first n_x values) is refused
    L = capi.lib()
    ch = np.array(CHAINS, dtype=np.int32)
    for bad in (np.nan, np.inf):
        g = grid.copy()
        g[40, 2] = bad
        cfg = capi.PredictConfig(n_keep=2, chains=ch.ctypes.data_as(C.POINTER(C.c_int32)), n_x=65,
                                 x=g.ctypes.data_as(capi._dp), nbins=0, lo=0.0, hi=0.0)
        assert L.apemost_hip_predict_begin(s._h, C.byref(cfg)) == capi.ERR_INVALID
        assert b"not finite" in L.apemost_hip_last_error()
        out = np.zeros((1, 65))
        assert L.apemost_hip_predict_curve(s._h, 1, par.ctypes.data_as(capi._dp), 65, g.ctypes.data_as(capi._dp),
                                           out.ctypes.data_as(capi._dp)) == capi.ERR_INVALID
    s.close()


def test_a_one_dimensional_x_is_column_0():
    """through Python a 1-D x of a user model is column 0 of rows whose other columns are zero"""
    data, rows = sine2_case()
    x = 3.0 + 0.25 * np.arange(65)
    s = HipSampler(wl.MODEL_USER, 2, 5, data, seed=1, device_model_source=SINE2)
    par = rows[:6, 0, :2]
    v = s.predict_curve(par, x)
    assert v.shape == (6, 65) and v.tobytes() == s.predict_curve(par, np.stack([x, np.zeros(65)], 1)).tobytes()
    want, _, dv, _ = sine2_numpy(par, np.stack([x, np.zeros(65)], 1), 0.5)
    assert float(np.max(np.abs(v - want) / (2 * dv))) <= 1
    d = on_device(rows)
    s.predict_begin(chains=(0,), x=x)
    s.predict_accumulate(d.data_ptr(), len(rows))
    pr = s.predict()
    s.predict_end()
    vals = s.predict_curve(np.ascontiguousarray(rows[:, 0, :2]), x).reshape(len(rows), 1, 65)
    with pytest.raises(ValueError):
        s.predict_curve(par, np.zeros((65, 3)))               # rows of another width
    s.close()
    assert pr.x[0].tobytes() == x.tobytes()
    assert_equals(pr, RefPredict(None, rows, [0], x, values=vals), "1-D x")


# ---- 6. one hook only ----------------------------------------------------------------------------------------------------------------
def test_one_hook_only(tmp_path):
    """a source with the pointwise hook alone: every predict entry point is refused with words that name the missing
    hook, and the pointwise fold of the same sampler works"""
    src = tmp_path / "pointwise_only.hip"
    src.write_text("/* no APEMOST_USER_CURVE here */\n" + LINE_BASE + LINE_POINTWISE)
    data, rows = line_data(65), line_rows(40, 5, 2, seed=5)
    s = HipSampler(wl.MODEL_USER, 2, 5, data, seed=1, sigma=SIGMA, device_model_source=str(src))
    has_curve, has_pointwise, seconds = s.user_hooks
    assert (has_curve, has_pointwise) == (False, True) and seconds > 0
    L = capi.lib()
    ch = np.zeros(1, dtype=np.int32)
    cfg = capi.PredictConfig(n_keep=1, chains=ch.ctypes.data_as(C.POINTER(C.c_int32)), n_x=0, x=None, nbins=0, lo=0.0, hi=0.0)
    assert L.apemost_hip_predict_begin(s._h, C.byref(cfg)) == capi.ERR_UNSUPPORTED
    words = L.apemost_hip_last_error()
    assert b"user" in words and b"apemost_user_curve" in words and b"apemost_device_model.h" in words
    out, par = np.zeros((1, 65)), np.zeros((1, 2))
    assert L.apemost_hip_predict_curve(s._h, 1, par.ctypes.data_as(capi._dp), 0, None,
                                       out.ctypes.data_as(capi._dp)) == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ApemostHipError):
        s.predict_begin(chains=(0,))
    d = on_device(rows)
    s.pointwise_begin(chains=CHAINS)
    s.pointwise_accumulate(d.data_ptr(), len(rows))
    pw = s.pointwise(at_mean=True)
    s.pointwise_end()
    _, l = kept_values(rows, CHAINS, 2, data)
    check_pointwise(pw, RefPointwise(None, rows, CHAINS, data, SIGMA, values=l), EXACT_RULE, "pointwise only")
    assert pw.at_mean.tobytes() == line_values(pw.par_mean_all(), data)[1].tobytes()
    s.close()


# ---- 7. a resumed run; ladder batches ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [5, 30])
def test_set_resumes_both_folds_in_a_new_sampler(line_src, cut):
    """get, a new sampler of the same source, begin, set and more samples: the uninterrupted fold, bit for bit"""
    data, rows = line_data(65), line_rows(60, 5, 2, seed=6)
    s = HipSampler(wl.MODEL_USER, 2, 5, data, seed=1, sigma=SIGMA, device_model_source=line_src)
    whole = both_folds(s, rows, CHAINS, nbins=16, lo=1.0, hi=2.5)
    part = both_folds(s, rows[:cut], CHAINS, nbins=16, lo=1.0, hi=2.5)
    s.close()
    s = HipSampler(wl.MODEL_USER, 2, 5, data, seed=2, sigma=SIGMA, device_model_source=line_src)
    d = on_device(rows)
    s.predict_begin(chains=CHAINS, nbins=16, lo=1.0, hi=2.5)
    s.pointwise_begin(chains=CHAINS)
    s.predict_set(part[0])
    s.pointwise_set(part[1])
    s.predict_accumulate(d[cut:].data_ptr(), 60 - cut)
    s.pointwise_accumulate(d[cut:].data_ptr(), 60 - cut)
    pr, pw = s.predict(), s.pointwise(at_mean=False)
    s.close()
    assert_equals(pr, whole[0], "resumed at %d" % cut)
    assert_same_state(pw, whole[1], "resumed at %d" % cut)


def test_a_later_set_data_does_not_move_the_rows(line_src):
    """the folds' rows are copies taken at begin"""
    data, rows = line_data(65), line_rows(40, 5, 2, seed=7)
    s = HipSampler(wl.MODEL_USER, 2, 5, data, seed=1, sigma=SIGMA, device_model_source=line_src)
    before = both_folds(s, rows, CHAINS)
    d = on_device(rows)
    s.predict_begin(chains=CHAINS)
    s.pointwise_begin(chains=CHAINS)
    s.set_data(data + 1.0)
    s.predict_accumulate(d.data_ptr(), len(rows))
    s.pointwise_accumulate(d.data_ptr(), len(rows))
    pr, pw = s.predict(), s.pointwise(at_mean=False)
    moved = s.pointwise_loglike(rows[0, 0, :2])
    s.close()
    assert_equals(pr, before[0], "set_data after begin")
    assert_same_state(pw, before[1], "set_data after begin")
    assert moved.tobytes() == line_values(rows[0, 0, :2], data + 1.0)[1].tobytes()   # (the evaluation reads the data as it is)


def test_a_user_model_still_does_not_run_in_a_ladder_batch(line_src):
    """what the issue's batch case would need: refused at create_batch, as before this feature"""
    data = line_data(65)
    with pytest.raises(capi.ApemostHipError) as err:
        HipSampler.batch(wl.MODEL_USER, 2, 3, np.stack([data, data + 1.0]), seeds=[1, 2], sigma=SIGMA,
                         device_model_source=line_src)
    assert "ladder batches" in str(err.value)


# ---- 8. beside the round kernels ---------------------------------------------------------------------------------------------------
def test_a_real_run_with_the_folds_between_launches():
    """simplesin2_hooks, 8 chains x 64 data, 10 launches of 200 steps with swap attempts; both folds accumulate between
    the launches.  The rows and the final state are bitwise those of the same run without a fold; the folds equal one
    call over the same rows; the round module's compile time is reported as before, and a second sampler of the same
    source takes the analysis module from the process's cache"""
    n_chain, n_rounds, n_swap, launches = 8, 20, 10, 10
    data, _ = sine2_case(64)
    lo, hi, per = np.array([0.0, 0.0]), np.array([2.0, 0.3]), n_rounds * n_swap
    out = []
    for with_fold in (True, False):
        s = HipSampler(wl.MODEL_USER, 2, n_chain, data, seed=5, device_model_source=SINE2)
        assert s.user_model_compile_seconds >= 0
        st = LadderState.from_params(n_chain, np.array([0.9, 0.2]), lo, hi, (hi - lo) * 0.03)
        st.beta[:] = [1.0 if i == 0 else 0.6 ** i for i in range(n_chain)]
        st.prob[:], st.prior[:] = s.loglike(st.params, st.beta)
        s.set_state(st)
        d = torch.zeros((launches, per, n_chain, 4), dtype=torch.float64, device="cuda")
        if with_fold:
            s.predict_begin(chains=(0,), nbins=32, lo=-1.5, hi=1.5)
            s.pointwise_begin(chains=(0,))
        for k in range(launches):
            s.run_sampler(n_rounds, n_swap, d[k].data_ptr())
            if with_fold:
                s.predict_accumulate(d[k].data_ptr(), per)
                s.pointwise_accumulate(d[k].data_ptr(), per)
        got = (s.predict(), s.pointwise()) if with_fold else None
        s.synchronize()
        rows = d.cpu().numpy().reshape(launches * per, n_chain, 4)
        if with_fold:
            s.predict_end()
            s.pointwise_end()
            assert int(got[0].n[0]) == int(got[1].n[0]) == 2000
            d1 = on_device(rows)
            s.predict_begin(chains=(0,), nbins=32, lo=-1.5, hi=1.5)
            s.pointwise_begin(chains=(0,))
            s.predict_accumulate(d1.data_ptr(), len(rows))
            s.pointwise_accumulate(d1.data_ptr(), len(rows))
            whole = (s.predict(), s.pointwise())
            assert_equals(got[0], whole[0], "interleaved against one call")
            assert_same_state(got[1], whole[1], "interleaved against one call")
            assert got[1].at_mean.tobytes() == whole[1].at_mean.tobytes() and np.isfinite(got[1].at_mean).all()
            c = got[1].criteria()
            assert all(np.isfinite(v) for v in c.values()) and c["p_waic2"] > 0
            assert np.isfinite(got[0].mean(0)).all() and int(got[0].best_n[0]) >= 1
            assert s.user_hooks[:2] == (True, True)
            twin = HipSampler(wl.MODEL_USER, 2, 1, data, seed=6, device_model_source=SINE2)
            assert twin.user_hooks == (True, True, 0.0) and twin.user_model_compile_seconds >= 0
            twin.close()
        out.append((s.get_state(), rows))
        s.close()
    assert np.any(np.diff(out[0][1][:, 0, :2], axis=0) != 0)      # the chain moved
    for f in ("params", "prob", "prior", "accept", "reject", "n_iter", "swapcount", "step", "beta"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()


# ---- 9. the C host -----------------------------------------------------------------------------------------------------------------
def test_c_host_tokens_with_a_device_model(tmp_path):
    """examples/sine2_model.c with APEMOST_DEVICE_MODEL_SRC=simplesin2_hooks.hip and APEMOST_DUMP=binary,pointwise,predict
    (N_BETA 8, 64 data, 3000 iterations): the files equal a Python fold of samples.bin's chain 0.  With simplesin2.hip,
    which has no hooks, the run stops and names the hook"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters = 8, 3000
    data, _ = sine2_case(64)
    work = tmp_path / "w"
    work.mkdir()
    (work / "params").write_text("".join("%.15e\t%.15e\t%.15e\t%s\t-1\n" % row for row in
                                         ((0.9, 0.0, 2.0, "amplitude"), (0.2, 0.0, 0.3, "frequency"))))
    (work / "data").write_text("".join("%.17e\t%.17e\n" % tuple(r) for r in data))
    exe = hostlib.make(str(tmp_path / "sine2.exe"), app=os.path.join(hostlib.HOST, "examples", "sine2_model.c"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP="binary,pointwise,predict", APEMOST_DEVICE_MODEL_SRC=SINE2)
    for phase in ("calibrate_first", "calibrate_rest", "run"):
        subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    _, params, probs = samples_bin.read(str(work / "samples.bin"))       # [iters][1][n_par], [iters][n_beta][2]
    rows = np.zeros((iters, 1, 4))
    rows[:, 0, :2] = params[:, 0]
    rows[:, 0, 2:] = probs[:, 0]
    file_data = np.loadtxt(str(work / "data"))                # what the host parsed
    pw, pr = Pointwise.read(str(work / "pointwise.bin")), Predict.read(str(work / "predict.bin"))
    assert (pw.n_keep, pw.n_data, pw.n_par, pw.model, pw.sigma) == (1, 64, 2, wl.MODEL_USER, 0.5) and int(pw.n[0]) == iters
    assert (pr.n_keep, pr.n_x, pr.n_par, pr.model, pr.nbins) == (1, 64, 2, wl.MODEL_USER, 0) and int(pr.n[0]) == iters
    assert pw.x[0].tobytes() == pr.x[0].tobytes() == file_data[:, 0].tobytes() and pw.y[0].tobytes() == file_data[:, 1].tobytes()
    s = HipSampler(wl.MODEL_USER, 2, 1, file_data, seed=1, device_model_source=SINE2)
    d = on_device(rows)
    s.predict_begin(chains=(0,))
    s.pointwise_begin(chains=(0,))
    s.predict_accumulate(d.data_ptr(), iters)
    s.pointwise_accumulate(d.data_ptr(), iters)
    my_pr, my_pw = s.predict(), s.pointwise(at_mean=True)
    best = s.predict_curve(my_pr.best_params[0])
    s.close()
    assert_equals(pr, my_pr, "the C host")
    assert_same_state(pw, my_pw, "the C host")
    assert pw.at_mean.tobytes() == my_pw.at_mean.tobytes() and np.isfinite(pw.at_mean).all()
    assert (work / "pointwise.txt").read_text() == pw.text()
    assert (work / "criteria.txt").read_text() == pw.criteria_text()
    assert (work / "predict.txt").read_text() == pr.text(file_data[:, 1], best)
    # a device model without the hooks: each token stops the run with the hook's name and the header's
    bare = dict(env, APEMOST_DEVICE_MODEL_SRC=os.path.join(MODELS, "simplesin2.hip"))
    for token, hook in (("pointwise", b"apemost_user_pointwise"), ("binary,predict", b"apemost_user_curve")):
        run = subprocess.run([exe, "run"], cwd=str(work), env=dict(bare, APEMOST_DUMP=token), stdout=subprocess.DEVNULL,
                             stderr=subprocess.PIPE, timeout=300)
        assert run.returncode != 0 and hook in run.stderr and b"apemost_device_model.h" in run.stderr, run.stderr
