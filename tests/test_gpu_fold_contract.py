"""What the seven on-device folds (summary, peaks, joint, evidence, autocorr, predict, pointwise with its tail)
have in common, which their own tests only sample: the wording and the order of the shared argument checks, the
ordering of every fold's work on the one copy stream when all of them are open at once, and a second begin that
starts from nothing.  The smallest sampler there is (simplesin, 3 chains, 16 data points) over 70 synthetic rows; no
stepping launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler

pytestmark = pytest.mark.gpu

FOLDS = ("summary", "peaks", "joint", "evidence", "autocorr", "predict", "pointwise")
WITH_SET = ("summary", "joint", "evidence", "autocorr", "predict", "pointwise")
WITH_CHAINS = ("peaks", "joint", "autocorr", "predict", "pointwise")
WITH_BOX = ("summary", "peaks", "joint")
N_CHAINS, N_PAR, N_DATA, N_STEPS = 3, 4, 16, 70
LO, HI = np.array([0.0, -3.0, 10.0, -1.0]), np.array([1.0, 5.0, 11.0, 1.0])
BETAS = np.array([1.0, 0.5, 0.25])
PASSES = ((1, 3), (0, 1))          # (skip, thin): 23 + 70 kept steps
KEPT = 23 + 70
# a first configuration of every fold, and a second one of another shape
FIRST = dict(summary=dict(lo=LO, hi=HI, n_hist_chains=2, nbins=8, batch_size=4, max_batches=40),
             peaks=dict(lo=LO, hi=HI, chains=(0, 2), capacity=256),
             joint=dict(lo=LO, hi=HI, chains=(0, 2), nbins=8),
             evidence=dict(betas=BETAS, batch_size=4, max_batches=40),
             autocorr=dict(chains=(0, 2), max_lag=5),
             predict=dict(chains=(0, 2), nbins=8, lo=-3.0, hi=3.0),
             pointwise=dict(chains=(0, 2), tail=4))
SECOND = dict(summary=dict(lo=LO, hi=HI, n_hist_chains=1, nbins=5, batch_size=4, max_batches=40),
              peaks=dict(lo=LO, hi=HI, chains=(1,), capacity=256),
              joint=dict(lo=LO, hi=HI, chains=(1,), nbins=5),
              evidence=dict(betas=BETAS, batch_size=4, max_batches=7),
              autocorr=dict(chains=(1,), max_lag=3),
              predict=dict(chains=(1,), nbins=5, lo=-3.0, hi=3.0),
              pointwise=dict(chains=(1,), tail=4))
# the arrays of the second configuration's results that depend on it
SECOND_SHAPES = dict(summary=dict(hist=(1, N_PAR, 5), batch_sums=(1, N_PAR, 41)),
                     peaks=dict(n_peaks=(1, N_PAR)),
                     joint=dict(counts=(1, 6, 5, 5), sum=(1, N_PAR)),
                     evidence=dict(batch=(N_CHAINS, 8)),
                     autocorr=dict(lag=(1, N_PAR + 1, 3), head=(1, N_PAR + 1, 2)),
                     predict=dict(hist=(1, N_DATA, 5), best_params=(1, N_PAR)),
                     pointwise=dict(origin=(1, N_DATA), par_sum=(1, N_PAR)))


def tiny_sampler():
    w = wl.simplesin(n_data=N_DATA, n_chain=N_CHAINS)
    assert w.n_par == N_PAR
    return HipSampler(w.model, w.n_par, N_CHAINS, w.data, seed=1)


@pytest.fixture(scope="module")
def rows():
    """[70][3][n_par + 2] on the device: parameters around the box (a tenth outside), prob and prob - prior"""
    rng = np.random.default_rng(46)
    r = np.zeros((N_STEPS, N_CHAINS, N_PAR + 2))
    r[:, :, :N_PAR] = LO + (HI - LO) * rng.uniform(-0.05, 1.05, (N_STEPS, N_CHAINS, N_PAR))
    r[:, :, N_PAR:] = rng.normal(-20.0, 3.0, (N_STEPS, N_CHAINS, 2))
    d = torch.from_numpy(r).cuda()
    torch.cuda.synchronize()
    return d


def begin(s, fold, second=False, **over):
    k = dict(SECOND[fold] if second else FIRST[fold])
    k.update(over)
    getattr(s, fold + "_begin")(**k)


def accumulate(s, fold, rows, skip, thin):
    getattr(s, fold + "_accumulate")(rows.data_ptr(), N_STEPS, skip, thin)


def results(s, fold):
    """what the fold holds, as its result objects (pointwise: the fold and its tail)"""
    got = [getattr(s, fold)()]
    if fold == "pointwise":
        got.append(s.pointwise_tail())
    return got


def view_fields(fold):
    return [name for name, _ in getattr(capi, fold.capitalize() + "View")._fields_]


def assert_same_bits(a, b, what):
    fa, fb = vars(a), vars(b)
    assert fa.keys() == fb.keys(), what
    n_arrays = 0
    for k, va in fa.items():
        vb = fb[k]
        if isinstance(va, np.ndarray):
            n_arrays += 1
            assert va.dtype == vb.dtype and va.shape == vb.shape and va.tobytes() == vb.tobytes(), (what, k)
        elif isinstance(va, (int, float, np.integer, np.floating)):
            assert va == vb, (what, k)
    assert n_arrays >= 3, what


def fails(rc, msg):
    assert rc == capi.ERR_INVALID
    assert capi.lib().apemost_hip_last_error().decode() == msg


def raises(msg, call, *args, **kw):
    with pytest.raises(capi.ApemostHipError) as e:
        call(*args, **kw)
    assert e.value.code == capi.ERR_INVALID
    assert str(e.value) == "apemost_hip error %d: %s" % (capi.ERR_INVALID, msg)


def test_shared_errors_read_the_same_for_every_fold(rows):
    s = tiny_sampler()
    L, h = s.L, s._h
    for f in FOLDS:
        fn = lambda what: getattr(L, "apemost_hip_%s_%s" % (f, what))    # noqa: E731
        view = getattr(capi, f.capitalize() + "View")()
        fails(fn("accumulate")(h, rows.data_ptr(), N_STEPS, 0, 1), "%s_accumulate: no %s_begin" % (f, f))
        fails(fn("get")(h, C.byref(view)), "%s_get: no %s_begin" % (f, f))
        if f in WITH_SET:
            fails(fn("set")(h, C.byref(view)), "%s_set: no %s_begin" % (f, f))
        fails(fn("begin")(h, None), "%s_begin: config is NULL" % f)
        begin(s, f)
        fails(fn("accumulate")(h, rows.data_ptr(), N_STEPS, 0, 0), "%s_accumulate: bad arguments" % f)
        fails(fn("accumulate")(h, None, N_STEPS, 0, 1), "%s_accumulate: bad arguments" % f)
        fails(fn("get")(h, None), "%s view is NULL" % f)
        if f in WITH_SET:
            fails(fn("set")(h, None), "%s view is NULL" % f)
        if f in WITH_CHAINS:
            raises("%s_begin: chains[1] = 1: local chain indices in [0,3), strictly increasing" % f,
                   begin, s, f, chains=(1, 1))
            raises("%s_begin: n_keep 4 outside [1,3], or no chains" % f, begin, s, f, chains=(0, 1, 2, 3))
        if f in WITH_BOX:
            lo = LO.copy()
            lo[0] = HI[0]
            raises("%s_begin: parameter 0: range [1, 1] invalid" % f, begin, s, f, lo=lo)
        # a begin that failed left the fold that was open as it was
        accumulate(s, f, rows, 0, 1)
        assert int(np.ravel(results(s, f)[0].n)[0]) == N_STEPS
    # the order in which a call examines its arguments: joint_begin reads the chain list before the box
    lo = LO.copy()
    lo[0] = HI[0]
    raises("joint_begin: chains[1] = 1: local chain indices in [0,3), strictly increasing",
           begin, s, "joint", chains=(1, 1), lo=lo)
    s.close()


def test_all_folds_open_at_once_equal_each_fold_alone(rows):
    """every fold's kernels and copies run on the sampler's one copy stream, ordered behind its stepping stream: with
    all seven folds open and their accumulates interleaved, every array of every result equals, bit for bit, that of
    the same fold open alone on a second sampler"""
    a = tiny_sampler()
    for f in FOLDS:
        begin(a, f)
    for skip, thin in PASSES:
        for f in FOLDS:
            accumulate(a, f, rows, skip, thin)
    together = {f: results(a, f) for f in FOLDS}
    b = tiny_sampler()
    for f in FOLDS:
        begin(b, f)
        for skip, thin in PASSES:
            accumulate(b, f, rows, skip, thin)
        alone = results(b, f)
        getattr(b, f + "_end")()
        assert len(alone) == len(together[f])
        for x, y in zip(together[f], alone):
            assert int(np.ravel(x.n)[0]) == KEPT
            assert_same_bits(x, y, f)
    a.close()
    b.close()


def test_a_second_begin_starts_from_nothing(rows):
    s = tiny_sampler()
    for f in FOLDS:
        begin(s, f)
        accumulate(s, f, rows, 0, 1)
        begin(s, f, second=True)
        for r in results(s, f):
            assert int(np.ravel(r.n)[0]) == 0, f
        r = results(s, f)[0]
        for name, shape in SECOND_SHAPES[f].items():
            assert getattr(r, name).shape == shape, (f, name)
        for name in view_fields(f):
            v = np.asarray(getattr(r, name))
            if f == "predict" and name in ("vmin", "vmax", "best_prob"):
                assert np.all(v == (np.inf if name == "vmin" else -np.inf)), (f, name)
            else:
                assert not v.any(), (f, name)
        if f == "pointwise":
            assert not results(s, f)[1].count.any()
    s.close()          # with every fold still open
