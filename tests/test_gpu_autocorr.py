"""On-device autocorrelation (apemost_hip_autocorr_*, pt_autocorr.h): origin, sum, lag sums, head and tail equal
tests/autocorr_ref.py -- a restatement that shares nothing with the kernels -- with == on the bits, on hand-built rows
over every call boundary, at the lag extremes, over several staged pieces, with non-finite values, on a real run, on a
ladder batch, through autocorr_set, beside the other folds and through the C host's APEMOST_DUMP=autocorr."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.autocorr import Autocorr
from apemost_amd.sampler import HipSampler
from apemost_amd.summary import batches_closed
from tests import hostlib
from tests.autocorr_ref import FIELDS, RefAutocorr, assert_equals, same_floats
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu

PIECE = 1 << 16        # kept steps of one staged piece of a single series (apemost_hip_autocorr_begin: 2^20 / n_series,
                       # at most 65536)


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def feed(s, d, calls, skip0=0, thin=1):
    """accumulate d in calls of the given numbers of steps; the kept steps are skip0, skip0 + thin, ... of the whole"""
    off = 0
    for n in calls:
        skip = skip0 - off if off < skip0 else (thin - (off - skip0) % thin) % thin
        s.autocorr_accumulate(d[off:].data_ptr(), n, skip, thin)
        off += n
    assert off == d.shape[0]


# ---- hand-built rows against the restatement --------------------------------------------------------------------
HAND_STEPS, HAND_LAG, HAND_CHAINS = 260, 70, [0, 3]
HAND_CALLS = [1, 2, 69, 70, 71, HAND_STEPS - 213]


def hand_rows(seed=1):
    """5 chains of 3 parameters: drifting columns far from zero, each on a scale of its own"""
    rng = np.random.default_rng(seed)
    rows = np.cumsum(rng.standard_normal((HAND_STEPS, 5, 5)), axis=0) + 0.3 * rng.standard_normal((HAND_STEPS, 5, 5))
    return rows * np.array([1.0, 1e-3, 40.0, 1.0, 7.0]) + np.array([10.0, -0.5, 1e4, 0.0, -2000.0])


@pytest.fixture(scope="module")
def sampler5():
    """a ladder of 5 chains with 3 parameters: the Bernoulli example of the user models"""
    rs = np.random.RandomState(5)
    data = np.column_stack([(rs.uniform(size=64) < 0.5).astype(float), rs.normal(0, 1, (64, 2))])
    s = HipSampler(wl.MODEL_USER, 3, 5, data, seed=1,
                   device_model_source=os.path.join(hostlib.HOST, "examples", "device_models", "bernoulli_example.hip"))
    yield s
    s.close()


@pytest.mark.parametrize("skip0,thin", [(0, 1), (2, 1), (1, 3), (4, 3)])
def test_hand_built_rows_over_every_call_boundary(sampler5, skip0, thin):
    """max_lag 70 is neither a multiple of 64 nor of the four lags of a lane; calls of 1, 2, 69, 70 and 71 steps and the
    rest cover pieces shorter than the history, the ramp-up while n < L and every boundary around L - 1"""
    rows = hand_rows()
    d = on_device(rows)
    s = sampler5
    s.autocorr_begin(chains=HAND_CHAINS, max_lag=HAND_LAG, thin=thin)
    feed(s, d, HAND_CALLS, skip0, thin)
    got = s.autocorr()
    kept = rows[skip0::thin]
    assert int(got.n[0]) == len(kept) and got.cols.tolist() == [0, 1, 2, 4] and got.thin == thin
    assert_equals(got, RefAutocorr(kept, HAND_CHAINS, HAND_LAG, [0, 1, 2, 4]), "calls %d/%d" % (skip0, thin))
    s.autocorr_begin(chains=HAND_CHAINS, max_lag=HAND_LAG, thin=thin)
    feed(s, d, [HAND_STEPS], skip0, thin)
    assert_equals(s.autocorr(), got, "one call %d/%d" % (skip0, thin))
    s.autocorr_end()
    assert len(kept) > HAND_LAG and np.all(got.lag[:, :, HAND_LAG - 1] != 0) and np.all(got.tail[:, :, 0] != 0)


def test_listed_columns(sampler5):
    rows = hand_rows(2)
    d = on_device(rows)
    s = sampler5
    s.autocorr_begin(chains=[1, 2, 4], max_lag=5, cols=[1, 3, 4])
    feed(s, d, [3, HAND_STEPS - 3])
    got = s.autocorr()
    s.autocorr_end()
    assert got.lag.shape == (3, 3, 5)
    assert_equals(got, RefAutocorr(rows, [1, 2, 4], 5, [1, 3, 4]))


def test_non_finite_values_stay_in_their_series(sampler5):
    rows = hand_rows(3)
    s = sampler5

    def fold(r):
        d = on_device(r)
        s.autocorr_begin(chains=HAND_CHAINS, max_lag=HAND_LAG)
        feed(s, d, HAND_CALLS)
        return s.autocorr()
    clean = fold(rows)
    bad = rows.copy()
    bad[100, 3, 1] = np.inf
    bad[150, 3, 1] = np.nan
    bad[5, 0, 4] = -np.inf
    got = fold(bad)
    s.autocorr_end()
    assert_equals(got, RefAutocorr(bad, HAND_CHAINS, HAND_LAG, [0, 1, 2, 4]), "non-finite")
    assert not np.isfinite(got.lag[1, 1]).any() and not np.isfinite(got.lag[0, 3]).any()
    for k in range(2):
        for c in range(4):
            if (k, c) in ((1, 1), (0, 3)):
                continue
            for f in FIELDS:
                assert getattr(got, f)[k, c].tobytes() == getattr(clean, f)[k, c].tobytes(), (k, c, f)


# ---- the lag extremes and several staged pieces ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def sampler1():
    w = wl.simplesin(n_data=16, n_chain=1)
    s = HipSampler(w.model, w.n_par, 1, w.data, seed=1)
    yield s
    s.close()


def one_series(n, seed):
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, 1, 6))
    e = rng.standard_normal(n)
    x = np.zeros(n)
    for t in range(1, n):
        x[t] = 0.95 * x[t - 1] + e[t]
    rows[:, 0, 2] = x + 3.0
    return rows


def test_one_lag(sampler1):
    """max_lag 1: head and tail are empty, the carry launch is skipped"""
    rows = one_series(300, 1)
    d = on_device(rows)
    s = sampler1
    s.autocorr_begin(chains=(0,), max_lag=1, cols=(2,))
    feed(s, d, [1, 7, 292])
    got = s.autocorr()
    s.autocorr_end()
    assert got.head.shape == got.tail.shape == (1, 1, 0)
    assert_equals(got, RefAutocorr(rows, (0,), 1, [2]))


def test_the_longest_lag(sampler1):
    """max_lag 4096 over 5000 kept steps in calls of 4095, 1, 4 and 900: sixteen lag groups, a piece of one step behind
    a full history, the end of the ramp-up inside a call"""
    rows = one_series(5000, 2)
    d = on_device(rows)
    s = sampler1
    s.autocorr_begin(chains=(0,), max_lag=4096, cols=(2,))
    feed(s, d, [4095, 1, 4, 900])
    got = s.autocorr()
    s.autocorr_end()
    assert_equals(got, RefAutocorr(rows, (0,), 4096, [2]))
    assert got.lag[0, 0, 4095] != 0


def test_several_staged_pieces(sampler1):
    """three full staged pieces and a ragged one in a single call, and the same steps cut elsewhere"""
    n = 3 * PIECE + 1234
    rows = one_series(n, 3)
    d = on_device(rows)
    s = sampler1
    s.autocorr_begin(chains=(0,), max_lag=8, cols=(2,))
    feed(s, d, [n])
    got = s.autocorr()
    assert_equals(got, RefAutocorr(rows, (0,), 8, [2], long=True))
    s.autocorr_begin(chains=(0,), max_lag=8, cols=(2,))
    feed(s, d, [PIECE - 3, 5, n - PIECE - 2])
    assert_equals(s.autocorr(), got, "cut elsewhere")
    s.autocorr_end()


# ---- a real run -------------------------------------------------------------------------------------------------
def test_a_real_run_between_launches():
    n_chain, n_rounds, n_swap, launches, L = 8, 40, 10, 5, 64
    w = wl.simplesin(n_data=256, n_chain=n_chain)
    st, _, _ = make_pair(w, n_chain, seed=5)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=5)
    s.set_state(st)
    per = n_rounds * n_swap
    d = torch.zeros((launches, per, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
    s.autocorr_begin(chains=(0, 5), max_lag=L)
    for k in range(launches):
        s.run_sampler(n_rounds, n_swap, d[k].data_ptr())
        s.autocorr_accumulate(d[k].data_ptr(), per)
    got = s.autocorr()
    s.synchronize()
    s.close()
    rows = d.cpu().numpy().reshape(launches * per, n_chain, w.n_par + 2)
    n = launches * per
    assert int(got.n[0]) == n
    assert_equals(got, Autocorr.from_rows(rows, (0, 5), L), "a real run")
    assert got.origin.tobytes() == np.ascontiguousarray(rows[0][[0, 5]][:, [0, 1, 2, 3, 5]]).tobytes()
    tau, window = got.tau(0)
    for p in range(w.n_par):
        M = int(window[p]) if window[p] >= 0 else L - 1
        se = float(tau[p]) * math.sqrt(2.0 * (2 * M + 1) / n)
        print("%s: tau %.3f window %d" % (w.names[p], tau[p], window[p]))
        assert math.isfinite(tau[p]) and tau[p] >= 1 - 4 * se, (p, tau[p], se)


# ---- a ladder batch -----------------------------------------------------------------------------------------------
def test_a_batch_of_three_ladders():
    from tests.test_gpu_ladder_batch import concat, ladders, make_batch, N_ROUNDS, N_SWAP, PER
    ws, seeds, sts, _, _ = ladders("simplesin", 3)
    w = ws[0]
    n_steps = N_ROUNDS * N_SWAP
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    d = torch.zeros((n_steps, 3 * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    chains = [0, PER, 2 * PER]
    batch.autocorr_begin(chains=chains, max_lag=33)
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.autocorr_accumulate(d.data_ptr(), n_steps)
    got = batch.autocorr()
    batch.close()
    assert got.n_ladders == 3
    assert_equals(got, RefAutocorr(d.cpu().numpy(), chains, 33, [0, 1, 2, 3, 5]), "batch")
    lads = got.per_ladder()
    for b in range(3):
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=4)
        alone.set_state(sts[b])
        da = torch.zeros((n_steps, PER, w.n_par + 2), dtype=torch.float64, device="cuda")
        alone.autocorr_begin(chains=(0,), max_lag=33)
        alone.run_sampler(N_ROUNDS, N_SWAP, da.data_ptr())
        alone.autocorr_accumulate(da.data_ptr(), n_steps)
        one = alone.autocorr()
        alone.close()
        assert_equals(lads[b], one, "ladder %d" % b)
    assert not same_floats(got.lag[0], got.lag[1])


# ---- autocorr_set: a resumed run ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cut", [3, 40, 101])
def test_set_resumes_a_fold(sampler5, cut):
    """get, end, begin, set and more samples equal the uninterrupted fold, with fewer samples than lags at the cut too"""
    rows = hand_rows(4)
    d = on_device(rows)
    s = sampler5
    s.autocorr_begin(chains=HAND_CHAINS, max_lag=HAND_LAG)
    s.autocorr_accumulate(d.data_ptr(), HAND_STEPS)
    whole = s.autocorr()
    s.autocorr_begin(chains=HAND_CHAINS, max_lag=HAND_LAG)
    s.autocorr_accumulate(d.data_ptr(), cut)
    part = s.autocorr()
    s.autocorr_end()
    assert int(part.n[0]) == cut
    s.autocorr_begin(chains=HAND_CHAINS, max_lag=HAND_LAG)
    s.autocorr_set(part)
    s.autocorr_accumulate(d[cut:].data_ptr(), HAND_STEPS - cut)
    got = s.autocorr()
    s.autocorr_end()
    assert_equals(got, whole, "resumed at %d" % cut)
    assert whole.origin.tobytes() == np.ascontiguousarray(rows[0][HAND_CHAINS][:, [0, 1, 2, 4]]).tobytes()


# ---- invalid arguments ----------------------------------------------------------------------------------------------
def test_invalid_arguments():
    n_chains = 96
    w = wl.simplesin(n_data=64, n_chain=n_chains)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    st, _, _ = make_pair(w, n_chains, seed=1)
    s.set_state(st)
    L = capi.lib()
    d = torch.zeros((12, n_chains, w.n_par + 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ac = Autocorr.empty((0,), 10, 4)
    assert L.apemost_hip_autocorr_accumulate(s._h, d.data_ptr(), 12, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_autocorr_get(s._h, C.byref(ac.view())) == capi.ERR_INVALID
    assert L.apemost_hip_autocorr_set(s._h, C.byref(ac.view())) == capi.ERR_INVALID
    assert L.apemost_hip_autocorr_begin(s._h, None) == capi.ERR_INVALID
    ip = C.POINTER(C.c_int32)

    def begin(chains=(0,), max_lag=10, cols=None):
        ch = np.array(chains, dtype=np.int32)
        co = None if cols is None else np.array(cols, dtype=np.int32)
        cfg = capi.AutocorrConfig(n_keep=len(ch), chains=ch.ctypes.data_as(ip) if len(ch) else None, max_lag=max_lag,
                                  n_cols=0 if co is None else len(co),
                                  cols=None if co is None else (co if len(co) else np.zeros(1, dtype=np.int32)).ctypes.data_as(ip))
        return L.apemost_hip_autocorr_begin(s._h, C.byref(cfg))
    refused = (dict(chains=()), dict(chains=(0, 0)), dict(chains=(2, 1)), dict(chains=(n_chains,)), dict(chains=(-1,)),
               dict(chains=tuple(range(n_chains + 1))), dict(max_lag=0), dict(max_lag=-1), dict(max_lag=4097),
               dict(cols=()), dict(cols=(1, 1)), dict(cols=(3, 2)), dict(cols=(6,)), dict(cols=(-1,)),
               dict(cols=(0, 1, 2, 3, 4, 5, 5)))
    for kw in refused:
        assert begin(**kw) == capi.ERR_INVALID, kw
        assert L.apemost_hip_autocorr_get(s._h, C.byref(ac.view())) == capi.ERR_INVALID, kw    # nothing was begun
    assert begin(chains=(0, 1, 2), max_lag=4096, cols=(0, 5)) == capi.OK
    assert begin(max_lag=1) == capi.OK and begin(cols=(0, 1, 2, 3, 4, 5)) == capi.OK
    assert begin() == capi.OK
    assert L.apemost_hip_autocorr_accumulate(s._h, d.data_ptr(), 12, 0, 0) == capi.ERR_INVALID      # thin 0
    assert L.apemost_hip_autocorr_accumulate(s._h, None, 12, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_autocorr_get(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_autocorr_accumulate(s._h, d.data_ptr(), 12, 12, 1) == capi.OK               # keeps nothing
    assert L.apemost_hip_autocorr_accumulate(s._h, d.data_ptr(), 12, 2, 3) == capi.OK
    ac = Autocorr.empty((0,), 10, 4)
    assert L.apemost_hip_autocorr_get(s._h, C.byref(ac.view())) == capi.OK and int(ac.n[0]) == 4
    assert not ac.sum.any() and not ac.lag.any()             # (rows of zeros)
    # a begin that is refused leaves the fold begun before open, accumulating as it was
    for kw in refused:
        assert begin(**kw) == capi.ERR_INVALID, kw
    assert L.apemost_hip_autocorr_begin(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_autocorr_accumulate(s._h, d.data_ptr(), 12, 0, 4) == capi.OK
    assert L.apemost_hip_autocorr_get(s._h, C.byref(ac.view())) == capi.OK and int(ac.n[0]) == 7
    s.autocorr_end()
    assert L.apemost_hip_autocorr_get(s._h, C.byref(ac.view())) == capi.ERR_INVALID
    # the sampler still steps
    before = s.get_state()
    s.run_sampler(3, 5, d.data_ptr())
    s.synchronize()
    after = s.get_state()
    assert np.array_equal(after.n_iter, before.n_iter + 15)
    s.close()


def test_an_accumulator_above_the_cap_is_refused():
    """n_series * max_lag above 2^24 lag sums: 700 chains x 6 columns x 4096 lags; 3 columns fit"""
    n_chains = 700
    w = wl.simplesin(n_data=16, n_chain=n_chains)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    L = capi.lib()
    ip = C.POINTER(C.c_int32)
    ch, co = np.arange(n_chains, dtype=np.int32), np.arange(6, dtype=np.int32)
    cfg = capi.AutocorrConfig(n_keep=n_chains, chains=ch.ctypes.data_as(ip), max_lag=4096, n_cols=6, cols=co.ctypes.data_as(ip))
    assert L.apemost_hip_autocorr_begin(s._h, C.byref(cfg)) == capi.ERR_INVALID
    assert b"2^24" in L.apemost_hip_last_error()
    cfg.max_lag = 3994                                       # 4200 x 3994 = 2^24 - 2416
    assert L.apemost_hip_autocorr_begin(s._h, C.byref(cfg)) == capi.OK
    cfg.max_lag = 3995
    assert L.apemost_hip_autocorr_begin(s._h, C.byref(cfg)) == capi.ERR_INVALID
    ac = Autocorr.empty(ch, 3994, 4, co)
    assert L.apemost_hip_autocorr_get(s._h, C.byref(ac.view())) == capi.OK and int(ac.n[0]) == 0
    s.close()


# ---- beside the other folds -----------------------------------------------------------------------------------------
def test_beside_the_other_folds():
    """the summary, joint, evidence and autocorrelation folds open on the same rows: each equals the one obtained alone"""
    from tests.test_gpu_summary import _run
    w, s, d, _ = _run("simplesin16")
    n_steps = d.shape[0]
    pieces = [(0, 100), (100, n_steps - 100)]
    nb = batches_closed(n_steps, 7)

    def begin(which):
        if "summary" in which:
            s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=7, max_batches=nb)
        if "joint" in which:
            s.joint_begin(w.pmin, w.pmax, chains=(0, 2), nbins=64)
        if "evidence" in which:
            s.evidence_begin(batch_size=7, max_batches=nb)
        if "autocorr" in which:
            s.autocorr_begin(chains=(0, 2), max_lag=50)
        for first, n in pieces:
            for name in which:
                getattr(s, name + "_accumulate")(d[first:].data_ptr(), n)
        out = {name: getattr(s, name)() for name in which}
        for name in which:
            if name != "summary":
                getattr(s, name + "_end")()
        return out
    every = begin(["summary", "joint", "evidence", "autocorr"])
    alone = {name: begin([name])[name] for name in ("summary", "joint", "evidence", "autocorr")}
    s.close()
    assert_equals(every["autocorr"], alone["autocorr"], "beside the others")
    assert_equals(every["autocorr"], Autocorr.from_rows(d.cpu().numpy(), (0, 2), 50))
    assert np.array_equal(every["summary"].hist, alone["summary"].hist)
    assert every["summary"].prob_sum.tobytes() == alone["summary"].prob_sum.tobytes()
    assert every["summary"].batch_sums.tobytes() == alone["summary"].batch_sums.tobytes()
    assert np.array_equal(every["joint"].counts, alone["joint"].counts)
    for f in ("origin", "sum", "cross"):
        assert getattr(every["joint"], f).tobytes() == getattr(alone["joint"], f).tobytes(), f
    for f in ("origin", "sum", "sq", "batch", "m", "S"):
        assert getattr(every["evidence"], f).tobytes() == getattr(alone["evidence"], f).tobytes(), f


def test_the_fold_does_not_change_the_chains():
    w = wl.pulse(n_data=257, n_chain=16)
    st, _, _ = make_pair(w, 16, seed=3)
    out = []
    for with_fold in (False, True):
        s = HipSampler(w.model, w.n_par, 16, w.data, seed=3)
        s.set_state(st)
        d = torch.zeros((2, 60, 16, w.n_par + 2), dtype=torch.float64, device="cuda")
        if with_fold:
            s.autocorr_begin(chains=(0, 7), max_lag=100)
        for k in range(4):
            buf = d[k % 2]
            s.run_sampler(20, 3, buf.data_ptr())
            if with_fold:
                s.autocorr_accumulate(buf.data_ptr(), 60)
                capi.check(s.L.apemost_hip_samples_wait(s._h))    # before the buffer is written again
        s.synchronize()
        out.append((s.get_state(), d.cpu().numpy()))
        if with_fold:
            assert int(s.autocorr().n[0]) == 240
        s.close()
    for f in ("params", "prob", "prior", "accept", "reject", "n_iter", "swapcount", "step", "beta"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()


# ---- the C host: APEMOST_DUMP=binary,autocorr -----------------------------------------------------------------------
def test_c_host_autocorr_token(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters, lags = 8, 6000, 100
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    runs = {}
    for mode in ("binary,autocorr", "binary", "autocorr"):
        work = tmp_path / mode.replace(",", "_")
        work.mkdir()
        (work / "params").write_text(w.params_file_text())
        (work / "data").write_text(w.data_file_text())
        env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP=mode)
        if mode != "autocorr":
            env["APEMOST_AUTOCORR_LAGS"] = str(lags)
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
        runs[mode] = (work, env)
    work, env = runs["binary,autocorr"]
    _, params, probs = samples_bin.read(str(work / "samples.bin"))       # [iters][1][n_par], [iters][n_beta][2]
    rows = np.zeros((iters, 1, w.n_par + 2))
    rows[:, 0, :w.n_par] = params[:, 0]
    rows[:, 0, w.n_par:] = probs[:, 0]
    got = Autocorr.read(str(work / "autocorr.bin"))
    assert (got.n_keep, got.max_lag, got.n_par, got.thin, got.n_ladders) == (1, lags, w.n_par, 1, 1)
    assert got.chains.tolist() == [0] and got.cols.tolist() == [0, 1, 2, 3, 5]
    assert_equals(got, Autocorr.from_rows(rows, (0,), lags), "the C host")
    assert (work / "autocorr.txt").read_text() == got.text(w.names)
    tau, _ = got.tau(0)
    assert np.isfinite(tau).all() and np.all(tau > 0.5)
    # the token changes no other file, and alone it writes no sample file; the default is 1024 lags
    plain, _ = runs["binary"]
    assert (plain / "samples.bin").read_bytes() == (work / "samples.bin").read_bytes()
    assert not (plain / "autocorr.bin").exists()
    only, _ = runs["autocorr"]
    assert not [f for f in os.listdir(str(only)) if f.endswith(".prob.dump") or f.startswith("prob-chain") or f == "samples.bin"]
    default = Autocorr.read(str(only / "autocorr.bin"))
    assert default.max_lag == 1024
    for f in ("origin", "sum"):
        assert getattr(default, f).tobytes() == getattr(got, f).tobytes(), f
    assert default.lag[:, :, :lags].tobytes() == got.lag.tobytes()
    # --append resumes from the file
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = Autocorr.read(str(work / "autocorr.bin"))
    assert int(second.n[0]) == 2 * iters and second.origin.tobytes() == got.origin.tobytes()
    assert second.head.tobytes() == got.head.tobytes()
    _, params, probs = samples_bin.read(str(work / "samples.bin"))       # the binary sink appended its records
    rows = np.zeros((2 * iters, 1, w.n_par + 2))
    rows[:, 0, :w.n_par] = params[:, 0]
    rows[:, 0, w.n_par:] = probs[:, 0]
    assert_equals(second, Autocorr.from_rows(rows, (0,), lags), "the C host, appended")
    assert (work / "autocorr.txt").read_text() == second.text(w.names)
    env_other = dict(env, APEMOST_AUTOCORR_LAGS="64")
    assert subprocess.call([exe, "run", "--append"], cwd=str(work), env=env_other, stdout=subprocess.DEVNULL,
                           stderr=subprocess.DEVNULL, timeout=300) != 0
    bad = dict(env, APEMOST_DUMP="binary,autocor")
    assert subprocess.call([exe, "run"], cwd=str(work), env=bad, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL,
                           timeout=300) != 0
