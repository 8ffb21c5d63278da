"""On-device resampling (apemost_hip_reweight_resample, pt_resample.h) through the C ABI.

The rule for every test.  The resampler has no floating point: GIVEN the device's own q (apemost_hip_reweight_weights)
the index is compared with == against tests/resample_ref.py (Python integers, bisect), the gathered values with the
store on the bits, q_total with apemost_hip_reweight_evaluate's; a range against a fold of only its rows, a ladder of a
batch against its own sampler.  What goes through exp can move a draw only where |q - q_ref| allows, so there the
estimator is held to the caps of tests/test_resample_cpu.py on the device's draws, and every drawn sample must have
q_ref + bound > 0 with the per-sample bound of reweight_ref.errors_over_bounds."""
import ctypes as C

import numpy as np
import pytest

from apemost_amd import capi
from apemost_amd.mbar import Mbar
from apemost_amd.reweight import Reweight
from tests import mbar_ref, resample_ref, reweight_ref
from tests.test_gpu_reweight import last_error, loaded, sampler_of, wide_sampler
from tests.test_reweight_cpu import D, HI, LO, columns
from tests.test_resample_cpu import TARGETS, check_conjugate_draws

pytestmark = pytest.mark.gpu

ODD = 0x9E3779B97F4A7C15
US = (0, (1 << 64) - 1, ODD)
TILE = 4096                 # kMbarTile
SCAN_PASS = 256             # kResampleScanThreads: the tiles one pass of resample_tile_scan_kernel covers


def draws_of(N):
    return (1, 7, N, 3 * N, 4096)


def check_exact(rw, mb, g, x, K, T, targets=(1.0, 0.3), t0=0, fast=False):
    """every M and u at every target against the reference over the device's own q; x [k][T][K] is the range's store"""
    N = T * K
    flat = x.reshape(len(x), -1)
    for bt in targets:
        _, q = rw.weights(mb, bt, g=g, t0=t0, t_count=T)
        q = q.reshape(-1)
        q_total = int(rw.evaluate(mb, [bt], g=g, t0=t0, t_count=T).q_total[0, 0])
        if fast:
            c = np.cumsum(q, dtype=np.uint64)
            assert int(c[-1]) == q_total == sum(int(v) for v in q.tolist())
        else:
            c = resample_ref.cumulative(q.tolist())
        for M in draws_of(N):
            for u in US:
                r = rw.resample(mb, bt, M, u, g=g, t0=t0, t_count=T)
                if fast:
                    a, b = divmod(q_total, M)
                    m = np.arange(M, dtype=np.uint64)
                    p = m * np.uint64(a) + (m * np.uint64(b)) // np.uint64(M) + np.uint64((u * a) >> 64)
                    assert [int(p[i]) for i in (0, M - 1)] == [(u * a) >> 64, (M - 1) * a + ((M - 1) * b) // M + ((u * a) >> 64)]
                    want = np.searchsorted(c, p, side="right")
                else:
                    want = np.array(resample_ref.draws(q.tolist(), M, u)[0])
                    if M <= N:
                        resample_ref.check_rule(q.tolist(), r.index[0], M, u)
                assert r.index.dtype == np.uint32 and np.array_equal(r.index[0], want), (bt, M, u)
                assert r.x[0].tobytes() == np.ascontiguousarray(flat[:, want].T).tobytes(), (bt, M, u)
                assert int(r.q_total[0]) == q_total and r.shift == 63 - N.bit_length()
                assert r.range == (t0, T) and r.n_draws == M and r.u == u and r.beta == bt


@pytest.mark.parametrize("K,T", [(3, 50), (8, 512), (5, 1639)], ids=["N150", "N4096", "N8195"])
def test_exact_given_q(K, T):
    """below one tile; one tile exactly; two tiles and three samples"""
    betas, ell, x, g = columns(K, T, "gauss", seed=21)
    s, mb, rw = loaded(ell, x, betas, np.arange(D))
    check_exact(rw, mb, g, x, K, T)
    s.close()


def test_exact_one_tile_more_than_a_pass_of_the_tile_scan():
    """SCAN_PASS + 1 = 257 tiles: the tile-sum scan carries from its first pass into a second of one tile; one chain,
    one column, the check in numpy's uint64 (cumsum is exact below 2^63)"""
    K, T = 1, SCAN_PASS * TILE + 5
    assert (K * T + TILE - 1) // TILE == SCAN_PASS + 1
    rng = np.random.default_rng(3)
    betas = np.array([1.0])
    x = rng.standard_normal((1, T, K))
    ell = -0.5 * x[0] * x[0] * (1 + 3 * (rng.uniform(size=(T, K)) < 0.5))    # (at 1.3 the weights are e^(0.3 l): O(1))
    g = np.zeros(1)
    s, mb, rw = loaded(ell, x, betas, [0])
    check_exact(rw, mb, g, x, K, T, targets=(1.3,), fast=True)
    s.close()


def test_spread_weights():
    """10^4 between neighbouring chains: only the coldest chain's samples carry weight at beta = 1, and M exceeds them"""
    K, T = 5, 1639
    betas, ell, x, g = columns(K, T, "spread", seed=9)
    s, mb, rw = loaded(ell, x, betas, np.arange(D))
    N = K * T
    for bt in (1.0, 1.5):
        _, q = rw.weights(mb, bt, g=g, t0=0, t_count=T)
        q = q.reshape(-1).tolist()
        live = sum(v > 0 for v in q)
        assert 0 < live <= T
        for M in (live + 1, N, 3 * N):
            r = rw.resample(mb, bt, M, ODD, g=g, t0=0, t_count=T)
            want, _ = resample_ref.draws(q, M, ODD)
            assert r.counts().tolist() == resample_ref.counts(want, N) and r.index[0].tolist() == want
            resample_ref.check_rule(q, r.index[0], M, ODD)
            assert all(q[n] > 0 for n in set(r.index[0].tolist()))
    s.close()


def test_sixteen_columns():
    K, T, k = 5, 1639, 16
    betas, ell, x4, g = columns(K, T, "gauss", seed=21)
    x = np.stack([x4[a % D] * (1 + a // D) + a for a in range(k)])
    s, mb, rw = loaded(ell, x, betas, list(range(k)), sampler=wide_sampler(K))
    _, q = rw.weights(mb, 0.3, g=g, t0=0, t_count=T)
    for M in (7, 4096, 3 * K * T):
        r = rw.resample(mb, 0.3, M, ODD, g=g, t0=0, t_count=T)
        want, _ = resample_ref.draws(q.reshape(-1).tolist(), M, ODD)
        assert r.index[0].tolist() == want and r.x.shape == (1, M, k)
        assert r.x[0].tobytes() == np.ascontiguousarray(x.reshape(k, -1)[:, want].T).tobytes()
    s.close()


def test_a_range_equals_a_fold_of_its_rows():
    """900 steps = 4500 samples, a tile and a ragged one, starting inside a tile of the whole store"""
    K, T = 5, 1639
    betas, ell, x, g = columns(K, T, "gauss", seed=5)
    s, mb, rw = loaded(ell, x, betas, np.arange(D))
    t0, n = 333, 900
    part = [rw.resample(mb, 0.4, M, u, g=g, t0=t0, t_count=n) for M in (7, 4096, 13500) for u in US]
    check_exact(rw, mb, g, x[:, t0:t0 + n], K, n, targets=(0.4,), t0=t0)
    s.close()
    fs, fmb, fresh = loaded(ell[t0:t0 + n], x[:, t0:t0 + n], betas, np.arange(D))
    whole = [fresh.resample(fmb, 0.4, M, u, g=g, t0=0, t_count=n) for M in (7, 4096, 13500) for u in US]
    fs.close()
    for a, b in zip(part, whole):
        assert a.index.tobytes() == b.index.tobytes() and a.x.tobytes() == b.x.tobytes() and a.q_total == b.q_total
        assert a.step[0].tolist() == (b.step[0] + t0).tolist() and a.chain.tobytes() == b.chain.tobytes()


def test_a_ladder_of_a_batch_equals_its_own_sampler():
    K, T = 5, 1000
    parts = [columns(K, T, "gauss", seed=40 + b) for b in range(2)]
    betas = np.concatenate([p[0] * (1 - 0.1 * b) for b, p in enumerate(parts)])
    ell = np.concatenate([p[1] for p in parts], axis=1)
    x = np.concatenate([p[2] for p in parts], axis=2)
    g = np.concatenate([p[3] for p in parts])
    cols = [0, 2, 3]
    s, mb, rw = loaded(ell, x[cols], betas, cols, n_ladders=2)
    got = {(M, u): rw.resample(mb, 0.3, M, u, g=g, t0=0, t_count=T) for M in (7, 4096, 3 * K * T) for u in US}
    direct = s.reweight_resample(g, 0.3, 4096, ODD)
    s.close()
    assert direct.index.tobytes() == got[4096, ODD].index.tobytes() and direct.x.tobytes() == got[4096, ODD].x.tobytes()
    assert direct.range == (0, T) and direct.n == T
    for b in range(2):
        k = slice(b * K, (b + 1) * K)
        one_s, one_mb, one_rw = loaded(ell[:, k], x[cols][:, :, k], betas[k], cols)
        for (M, u), r in got.items():
            alone = one_rw.resample(one_mb, 0.3, M, u, g=g[k], t0=0, t_count=T)
            one = r.per_ladder()[b]
            for w in ("index", "x", "q_total"):
                assert getattr(one, w).tobytes() == getattr(alone, w).tobytes(), (b, M, u, w)
            assert r.index.shape == (2, M) and one.n_ladders == 1 and one.n_chains == K
            assert r.chain[b].tolist() == (alone.chain[0] + b * K).tolist()
        one_s.close()


def test_through_exp_on_the_conjugate_problem():
    K, T = 8, 2000
    betas, ell, x = reweight_ref.conjugate(K, T, D)
    s, mb, rw = loaded(ell, x, betas, np.arange(D), LO, HI, 20)
    used, change = mb.solve(tol=1e-10)
    assert change <= 1e-10
    ess = rw.evaluate(mb, TARGETS).ess()
    drawn = {}

    def resample(bt, M, u):
        r = rw.resample(mb, bt, M, u)
        drawn.setdefault(bt, set()).update(r.index[0].tolist())
        return r
    check_conjugate_draws(resample, ess, "device")
    s.close()
    N, tiles = K * T, (K * T + TILE - 1) // TILE
    lnD = mbar_ref.ln_d(ell, betas, mb.g)
    shift = reweight_ref.shift_of(N)
    for bt in TARGETS:
        m, e, x_abs_max = reweight_ref.weights(ell, lnD, bt)
        E_x, _ = mbar_ref.bounds(K, tiles, lnD, x_abs_max)
        q_ref = np.rint(np.ldexp(e, shift))
        bound = 2.0 ** shift * (2 * E_x + 4 * 2.0 ** -53) * e + 1
        at = np.array(sorted(drawn[bt]))
        print("beta %.3g: %d distinct samples drawn, the smallest q_ref + bound among them %.3g" % (bt, len(at), (q_ref + bound)[at].min()))
        assert np.all(q_ref[at] + bound[at] > 0)


def test_refusals():
    betas, ell, x, g = columns(4, 20, "gauss")
    s = sampler_of(4)
    L = capi.lib()
    gp = g.ctypes.data_as(capi._dp)
    index = np.zeros(64, dtype=np.uint32)
    out = capi.ReweightDraws(index=index.ctypes.data_as(C.POINTER(C.c_uint32)))

    def resample(M, t0=0, n=20, beta=1.0, g_=gp, out_=C.byref(out)):
        return L.apemost_hip_reweight_resample(s._h, t0, n, g_, beta, M, 0, out_)
    # before begin
    assert resample(8) == capi.ERR_INVALID and last_error() == "reweight_resample: no reweight_begin"
    s.mbar_begin(20, betas)
    assert resample(8) == capi.ERR_INVALID and last_error() == "reweight_resample: no reweight_begin"
    s.reweight_begin([0, 1, 2, 3, 4], nbins=0)
    # the arguments, before any device work
    assert resample(0) == capi.ERR_INVALID and "n_draws 0 outside [1,2^24]" in last_error()
    assert resample((1 << 24) + 1) == capi.ERR_INVALID and "n_draws 16777217 outside [1,2^24]" in last_error()
    assert resample(1 << 24) == capi.ERR_INVALID
    assert "1 ladders x 16777216 draws x 5 columns are more than 2^26 values" in last_error()
    assert resample(8, out_=None) == capi.ERR_INVALID and last_error() == "reweight_resample: out is NULL"
    assert resample(8, g_=None) == capi.ERR_INVALID and last_error() == "reweight_resample: g is NULL"
    for bad in (-0.5, np.inf, np.nan):
        assert resample(8, beta=bad) == capi.ERR_INVALID and "the target is" in last_error()
    # only one of the two stores advanced
    s.mbar_set(Mbar(ell, betas))
    assert resample(8) == capi.ERR_INVALID
    assert "reweight_resample: stores out of step: mbar holds 20 kept steps, reweight 0" in last_error()
    # a column that is not finite
    x5 = np.concatenate([x, x[:1]])
    x5[1, 3, 2] = np.nan
    s.reweight_set(Reweight(x5, np.arange(5), n_bad=[[0, 1, 0, 0, 0]]))
    assert resample(8) == capi.ERR_INVALID
    assert "reweight_resample: ladder 0 stores 1 values of column 1 that are not finite" in last_error()
    x5[1, 3, 2] = 0.0
    s.reweight_set(Reweight(x5, np.arange(5)))
    # the refusals of mbar_iterate
    for t0, n in ((0, 0), (20, 1), (5, 16)):
        assert resample(8, t0, n) == capi.ERR_INVALID and "go past the 20 stored" in last_error()
    bad_g = g.copy()
    bad_g[2] = np.nan
    assert resample(8, g_=bad_g.ctypes.data_as(capi._dp)) == capi.ERR_INVALID and "g[2]" in last_error()
    # and a call that goes through: any pointer of out may be NULL
    assert resample(64) == capi.OK and np.all(np.diff(index.astype(np.int64)) >= 0) and index.max() < 80
    assert L.apemost_hip_reweight_resample(s._h, 0, 20, gp, 1.0, 8, 0, C.byref(capi.ReweightDraws())) == capi.OK
    s.reweight_end()
    assert resample(8) == capi.ERR_INVALID and last_error() == "reweight_resample: no reweight_begin"
    s.close()
