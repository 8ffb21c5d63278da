"""On-device reweighted posteriors (apemost_hip_reweight_*, pt_reweight.h) through the C ABI.

The rule for every test.  What the header states as exact is compared with == on the bits: the store, and, GIVEN the
device's own e_n (apemost_hip_reweight_weights), every word of an evaluation: q = rint(ldexp(e, s)), the histograms as
the integer bincount of q under the bins of tests/summary_rows.py, q_total, S1 and cross as numpy's products through
mbar.tile_sum, and m, S0, SS against apemost_hip_mbar_evaluate; 64 targets against one at a time, a range against a
fold of only its rows, a ladder of a batch against its own sampler.  What goes through exp is compared with
tests/reweight_ref.py (exact sums over numpy's exp) under the bounds of tests/test_gpu_mbar.py (E_x, R0) carried to
these words in reweight_ref.errors_over_bounds:  |q - q_ref| <= 2^s (2 E_x + 4 u) e + 1 per sample, the sum of that per
bin and for q_total, (R0 + 2 u) sum e |d_a| for S1 and (R0 + 4 u) sum e |d_a d_b| for cross.  The estimator is held to
5 analytic standard errors on the conjugate problem, where the reference alone stays under 2 (tests/test_reweight_cpu.py
prints them).  The tests print the worst error they saw beside the bound."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.joint import bins_of, tri_index
from apemost_amd.mbar import Mbar, tile_sum
from apemost_amd.reweight import Reweight, Reweighted, weighted_bincount
from apemost_amd.sampler import HipSampler
from apemost_amd.summary import batches_closed
from tests import hostlib, mbar_ref, reweight_ref
from tests.evidence_ref import same_floats
from tests.helpers import make_pair
from tests.summary_rows import gsl_edges
from tests.test_reweight_cpu import D, HI, LO, check_conjugate, columns

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
WORDS = Reweighted._WORDS


def sampler_of(n_chains, n_ladders=1):
    w = wl.simplesin(n_data=16, n_chain=n_chains // n_ladders)
    if n_ladders == 1:
        return HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    return HipSampler.batch(w.model, w.n_par, n_chains // n_ladders, np.stack([w.data] * n_ladders), list(range(1, n_ladders + 1)))


def wide_sampler(n_chains):
    """a user model of 14 parameters: 16 columns in a row"""
    rs = np.random.RandomState(5)
    data = np.column_stack([(rs.uniform(size=32) < 0.5).astype(float), rs.normal(0, 1, (32, 13))])
    return HipSampler(wl.MODEL_USER, 14, n_chains, data, seed=1,
                      device_model_source=os.path.join(hostlib.HOST, "examples", "device_models", "bernoulli_example.hip"))


def loaded(ell, x, betas, cols, lo=None, hi=None, nbins=0, n_ladders=1, capacity=None, sampler=None):
    """(sampler, its Mbar, its Reweight) with the stores ell [n][n_chains] and x [k][n][n_chains] loaded through set"""
    ell, x = np.ascontiguousarray(ell), np.ascontiguousarray(x)
    s = sampler or sampler_of(ell.shape[1], n_ladders)
    s.mbar_begin(capacity or len(ell), betas)
    s.reweight_begin(cols, lo, hi, nbins)
    s.mbar_set(Mbar(ell, betas, n_ladders))
    s.reweight_set(Reweight(x, cols, lo, hi, nbins, n_ladders))
    mb, rw = s.mbar(), s.reweight()
    assert rw.x.tobytes() == x.tobytes() and rw.n == len(ell) == mb.n
    return s, mb, rw


def last_error():
    return capi.lib().apemost_hip_last_error().decode()


def same_words(a, b, what=""):
    for w in WORDS:
        assert getattr(a, w).tobytes() == getattr(b, w).tobytes(), (what, w)


# ---- the store ------------------------------------------------------------------------------------------------------
def test_the_store():
    """the rows of the evidence fold's hand-built test: 300 chains, three calls with skip 2 and thin 3"""
    from tests.test_gpu_evidence import calls_of, hand_built, on_device
    rows, _, _ = hand_built()
    calls, kept = calls_of([81, 92, 87], 3, 2)
    betas = 0.01 ** (np.arange(300) / 299.0)
    cols = [1, 4, 5]
    want = np.ascontiguousarray(np.moveaxis(rows[kept][:, :, cols], 2, 0))
    n_bad = int((~np.isfinite(want[2])).sum())
    assert n_bad >= 2 * 111 and np.isnan(want[2]).any() and np.isinf(want[2]).any() and np.isfinite(want[:2]).all()
    s = sampler_of(300)
    d = on_device(rows)
    L = capi.lib()
    lo, hi = [-1.0, -1.0, -2000.0], [1.0, 1.0, 0.0]
    s.mbar_begin(len(kept), betas)
    s.reweight_begin(cols, lo, hi, 10)
    for first, n, skip in calls:
        s.reweight_accumulate(d[first:].data_ptr(), n, skip, 3)
    three = s.reweight()
    assert three.n == len(kept) == 86 and same_floats(three.x, want) and three.n_bad.tolist() == [[0, 0, n_bad]]
    # one step too many
    assert L.apemost_hip_reweight_accumulate(s._h, d.data_ptr(), 1, 0, 1) == capi.ERR_INVALID
    assert "reweight_accumulate" in last_error() and "beyond capacity = 86" in last_error()
    assert L.apemost_hip_reweight_accumulate(s._h, d.data_ptr(), 260, 260, 1) == capi.OK      # keeps nothing
    # only one of the two stores advanced
    g = np.zeros(300)
    bt = np.array([1.0])
    out = np.zeros(1)
    sums = capi.ReweightSums(S0=out.ctypes.data_as(capi._dp))
    args = (g.ctypes.data_as(capi._dp), bt.ctypes.data_as(capi._dp), 1, C.byref(sums))
    assert L.apemost_hip_reweight_evaluate(s._h, 0, 86, *args) == capi.ERR_INVALID
    assert "stores out of step: mbar holds 0 kept steps, reweight 86" in last_error()
    assert L.apemost_hip_reweight_weights(s._h, 0, 86, g.ctypes.data_as(capi._dp), 1.0, None, None) == capi.ERR_INVALID
    assert "stores out of step" in last_error()
    # in step, the counts refuse the sums, and say why: first mbar's own, then the column's
    s.mbar_accumulate(d.data_ptr(), 260, 2, 3)
    assert L.apemost_hip_reweight_evaluate(s._h, 0, 86, *args) == capi.ERR_INVALID
    assert "stores %d values that are not finite" % n_bad in last_error()
    finite = np.where(np.isfinite(rows[kept][:, :, 5]), rows[kept][:, :, 5], -1000.0) / betas
    s.mbar_set(Mbar(finite, betas))
    assert L.apemost_hip_reweight_evaluate(s._h, 0, 86, *args) == capi.ERR_INVALID
    assert "ladder 0 stores %d values of column 5 that are not finite" % n_bad in last_error()
    with pytest.raises(ValueError, match="%d values of column 5 that are not finite" % n_bad):
        Reweight.from_rows(rows[kept], betas, cols).evaluate(Mbar(finite, betas), [1.0], g=g)
    # three calls equal one
    s.mbar_begin(len(kept), betas)
    s.reweight_begin(cols, lo, hi, 10)
    s.reweight_accumulate(d.data_ptr(), 260, 2, 3)
    one = s.reweight()
    assert same_floats(one.x, three.x) and one.n_bad.tobytes() == three.n_bad.tobytes()
    assert same_floats(Reweight.from_rows(rows[kept], betas, cols).x, one.x)
    # get -> begin -> set -> get, into a larger capacity, and on from there
    s.mbar_begin(100, betas)
    s.reweight_begin(cols, lo, hi, 10)
    assert s.reweight().n == 0
    s.reweight_set(one)
    back = s.reweight()
    assert back.n == 86 and same_floats(back.x, one.x) and back.n_bad.tobytes() == one.n_bad.tobytes()
    s.reweight_accumulate(d.data_ptr(), 14, 0, 1)
    more = s.reweight()
    assert more.n == 100 and same_floats(more.x[:, 86:], np.moveaxis(rows[:14][:, :, cols], 2, 0))
    assert same_floats(more.x[:, :86], one.x)
    s.reweight_end()
    s.mbar_end()
    s.close()


# ---- on the bits, given the device's own e --------------------------------------------------------------------------
def edge_values(lo, hi, nbins, rng, count):
    """values exactly on edges, on the widened top edge and beside it, on and beside the corners, outside, inside"""
    e = gsl_edges(lo, hi, nbins)
    near = np.concatenate([e[:: max(1, nbins // 40)], [lo, hi, e[nbins]]])
    pool = np.concatenate([near, np.nextafter(near, -np.inf), np.nextafter(near, np.inf),
                           [lo - (hi - lo), hi + (hi - lo), 0.0, -0.0], lo + (hi - lo) * rng.uniform(0, 1, 50)])
    return pool[rng.integers(0, len(pool), count)]


@pytest.mark.parametrize("K,T,k,nbins", [(5, 1, 1, 1), (1, 8195, 4, 2), (5, 1639, 16, 4096)],
                         ids=["N5-1col-1bin", "N8195-K1-4cols-2bins", "16cols-4096bins"])
def test_on_the_bits_given_e(K, T, k, nbins):
    """one ragged tile; two tiles and one of 3 samples with one chain; 16 columns, all 136 cross sums, 4096 bins"""
    betas, ell, x4, g = columns(K, T, "gauss", seed=21)
    rng = np.random.default_rng(77)
    lo = [-4.0, 0.1, 1e15, -7.3][:k] if k <= 4 else [-4.0 + 0.1 * a for a in range(k)]
    hi = [4.0, 50.0, 1e15 + 3, -0.2][:k] if k <= 4 else [4.0 + 0.2 * a for a in range(k)]
    x = np.zeros((k, T, K))
    for a in range(k):
        about_zero = lo[a] < 0 < hi[a]
        x[a] = x4[a % D] * (1 + a // D) if about_zero else lo[a] + (hi[a] - lo[a]) * rng.uniform(-0.1, 1.1, (T, K))
        on = rng.uniform(size=(T, K)) < (0.6 if a % 2 else 0.1)
        x[a][on] = edge_values(lo[a], hi[a], nbins, rng, int(on.sum()))
    cols = list(range(k)) if k == 16 else list(range(6))[-k:]
    s, mb, rw = loaded(ell, x, betas, cols, lo, hi, nbins, sampler=wide_sampler(K) if k == 16 else None)
    targets = [1.0, 0.3, 0.0]
    got = rw.evaluate(mb, targets, g=g, t0=0, t_count=T)
    sums = mb.evaluate(targets, g=g, t0=0, t_count=T)
    N = T * K
    assert got.shift == 63 - N.bit_length()
    for t, bt in enumerate(targets):
        e, q = rw.weights(mb, bt, g=g, t0=0, t_count=T)
        e, q = e.reshape(-1), q.reshape(-1)
        assert e.max() == 1.0 and e.min() >= 0
        assert q.tobytes() == np.rint(np.ldexp(e, got.shift)).astype(np.uint64).tobytes()
        assert int(got.q_total[0, t]) == sum(int(v) for v in q)
        for w in ("m", "S0", "SS"):
            assert getattr(got, w)[0, t] == sums[w][0, t], w
        assert got.S0[0, t] == tile_sum(e) and got.SS[0, t] == tile_sum(e * e)
        d = [x[a].reshape(-1) - x[a, 0, 0] for a in range(k)]
        for a in range(k):
            assert got.origin[0, a] == x[a, 0, 0]
            ed = e * d[a]
            assert got.S1[0, t, a] == tile_sum(ed), (a, t)
            for b in range(a, k):
                assert got.cross[0, t, tri_index(k, a, b)] == tile_sum(ed * d[b]), (a, b, t)
            edges = gsl_edges(lo[a], hi[a], nbins)
            bins = np.array([reweight_ref.bin_of(v, edges) for v in x[a].reshape(-1).tolist()])
            want = [0] * nbins
            for b_, w_ in zip(bins.tolist(), q.tolist()):
                if b_ >= 0:
                    want[b_] += w_
            assert [int(v) for v in got.hist[0, t, a]] == want, (a, t)
            if N > 1000:
                assert (bins < 0).any() and sum(want) < int(got.q_total[0, t])      # (some weight lies outside)
    host = Reweight(x, cols, lo, hi, nbins).evaluate_numpy(Mbar(ell, betas), targets, g=g, t0=0, t_count=T)
    assert host.origin.tobytes() == got.origin.tobytes() and host.shift == got.shift
    s.close()


# ---- independence, on the bits ----------------------------------------------------------------------------------------
def test_targets_ranges_and_ladders_do_not_meet():
    K, T = 5, 1639
    betas, ell, x, g = columns(K, T, "gauss", seed=5)
    cols = [0, 1, 2, 3]
    s, mb, rw = loaded(ell, x, betas, cols, LO, HI, 20)
    targets = np.concatenate([[0.0, 1.5], betas, np.linspace(0.02, 1.2, 57)])
    assert len(targets) == 64
    all_ = rw.evaluate(mb, targets, g=g, t0=0, t_count=T)
    for t in (0, 1, 5, 17, 63):
        one = rw.evaluate(mb, [targets[t]], g=g, t0=0, t_count=T)
        for w in ("m", "S0", "SS", "S1", "cross", "hist", "q_total"):
            assert getattr(one, w)[:, 0].tobytes() == np.ascontiguousarray(getattr(all_, w)[:, t]).tobytes(), (t, w)
    # a range against a fold that holds only its rows: 900 steps = 4500 samples, a tile and a ragged one, starting
    # inside a tile of the whole store
    t0, n = 333, 900
    few = [0.0, 0.4, 1.0]
    part = rw.evaluate(mb, few, g=g, t0=t0, t_count=n)
    part_e, part_q = rw.weights(mb, 0.4, g=g, t0=t0, t_count=n)
    s.close()
    fs, fmb, fresh = loaded(ell[t0:t0 + n], x[:, t0:t0 + n], betas, cols, LO, HI, 20)
    whole = fresh.evaluate(fmb, few, g=g, t0=0, t_count=n)
    whole_e, whole_q = fresh.weights(fmb, 0.4, g=g, t0=0, t_count=n)
    fs.close()
    same_words(part, whole, "range")
    assert part_e.tobytes() == whole_e.tobytes() and part_q.tobytes() == whole_q.tobytes()


def test_a_ladder_of_a_batch_equals_its_own_sampler():
    K, T = 5, 300
    parts = [columns(K, T, "gauss", seed=40 + b) for b in range(3)]
    betas = np.concatenate([p[0] * (1 - 0.1 * b) for b, p in enumerate(parts)])
    ell = np.concatenate([p[1] for p in parts], axis=1)
    x = np.concatenate([p[2] for p in parts], axis=2)
    g = np.concatenate([p[3] for p in parts])
    cols, few = [0, 2, 3], [0.0, 0.3, 1.5]
    s, mb, rw = loaded(ell, x[[0, 2, 3]], betas, cols, LO[:3], HI[:3], 33, n_ladders=3)
    got = rw.evaluate(mb, few, g=g, t0=0, t_count=T)
    e, q = rw.weights(mb, 0.3, g=g, t0=0, t_count=T)
    s.close()
    for b, one in enumerate(got.per_ladder()):
        k = slice(b * K, (b + 1) * K)
        one_s, one_mb, one_rw = loaded(ell[:, k], x[[0, 2, 3]][:, :, k], betas[k], cols, LO[:3], HI[:3], 33)
        alone = one_rw.evaluate(one_mb, few, g=g[k], t0=0, t_count=T)
        alone_e, alone_q = one_rw.weights(one_mb, 0.3, g=g[k], t0=0, t_count=T)
        one_s.close()
        same_words(one, alone, "ladder %d" % b)
        assert alone_e.tobytes() == np.ascontiguousarray(e[:, k]).tobytes()
        assert alone_q.tobytes() == np.ascontiguousarray(q[:, k]).tobytes()


# ---- e against the reference ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "spread"])
def test_against_the_reference(kind):
    K, T, nbins = 5, 1639, 20
    betas, ell, x, g = columns(K, T, kind, seed=9)
    targets = [1.0, 0.3, 0.0, 1.5]
    s, mb, rw = loaded(ell, x, betas, np.arange(D), LO, HI, nbins)
    got = rw.evaluate(mb, targets, g=g, t0=0, t_count=T)
    dev = [rw.weights(mb, bt, g=g, t0=0, t_count=T) for bt in targets]
    s.close()
    N, tiles = ell.size, (ell.size + 4095) // 4096
    lnD = mbar_ref.ln_d(ell, betas, g)
    for t, bt in enumerate(targets):
        ref = reweight_ref.sums(x, ell, lnD, bt, LO, HI, nbins)
        E_x, R0 = mbar_ref.bounds(K, tiles, lnD, ref["x_abs_max"])
        err = reweight_ref.errors_over_bounds(got, 0, t, ref, E_x, R0, nbins)
        q = np.array([int(v) for v in dev[t][1].reshape(-1)], dtype=object)
        dq = np.abs(q - np.array(ref["q"], dtype=object)).astype(np.float64)
        err["q"] = float((dq / (2.0 ** ref["shift"] * (2 * E_x + 4 * U) * ref["e"] + 1)).max())
        print("%s, beta_t = %.4g: error over bound %s (E_x %.3g, R0 %.3g, worst |q - q_ref| %.0f of 2^%d)"
              % (kind, bt, " ".join("%s %.3f" % kv for kv in err.items()), E_x, R0, dq.max(), ref["shift"]))
        assert all(v <= 1 for v in err.values()), (bt, err)


# ---- the estimator ------------------------------------------------------------------------------------------------------
def test_the_conjugate_problem_solved_on_the_device():
    K, T = 8, 2000
    betas, ell, x = reweight_ref.conjugate(K, T, D)
    s, mb, rw = loaded(ell, x, betas, np.arange(D), LO, HI, 20)
    used, change = mb.solve(tol=1e-10)
    assert change <= 1e-10
    targets = np.array([1.0, 0.3, 0.0, 1.5])
    r = rw.evaluate(mb, targets)
    s.close()
    assert r.range == (0, T) and r.ess()[0] > T
    check_conjugate(r, targets)


# ---- a real run -------------------------------------------------------------------------------------------------------
def test_a_real_run_beside_the_summary_fold():
    """no statistical claim (quirk Q1): finite, normalised, and on the bits the host's integer histogram of the
    device's e; the summary beside it is the summary alone"""
    n_chain, n_rounds, n_swap, nbins = 8, 30, 10, 50
    w = wl.simplesin(n_data=16, n_chain=n_chain)
    st, _, _ = make_pair(w, n_chain, seed=5)
    n = n_rounds * n_swap
    hists = []
    for with_fold in (True, False):
        s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=5)
        s.set_state(st)
        d = torch.zeros((n, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
        s.summary_begin(w.pmin, w.pmax, nbins=nbins, batch_size=17, max_batches=batches_closed(n, 17))
        if with_fold:
            s.mbar_begin(n)
            s.reweight_begin(None, w.pmin, w.pmax, nbins)
        s.run_sampler(n_rounds, n_swap, d.data_ptr())
        s.summary_accumulate(d.data_ptr(), n)
        if with_fold:
            s.mbar_accumulate(d.data_ptr(), n)
            s.reweight_accumulate(d.data_ptr(), n)
            mb, rw = s.mbar(), s.reweight()
            rows = d.cpu().numpy()
            host = Reweight.from_rows(rows, st.beta, None, w.pmin, w.pmax, nbins)
            assert rw.n == n and rw.x.tobytes() == host.x.tobytes() and not rw.n_bad.any() and rw.cols.tolist() == [0, 1, 2, 3]
            g, _ = mb.iterate(mb.start(), 5)
            r = rw.evaluate(mb, [1.0, 0.5], g=g, t0=0, t_count=n)
            for t, bt in enumerate((1.0, 0.5)):
                e, q = rw.weights(mb, bt, g=g, t0=0, t_count=n)
                for a in range(4):
                    want = weighted_bincount(bins_of(host.x[a].reshape(-1), r.edges(a)), q.reshape(-1), nbins)
                    assert want.tobytes() == r.hist[0, t, a].tobytes()
                    assert int(r.hist[0, t, a].sum()) <= int(r.q_total[0, t]) == int(q.sum(dtype=np.uint64))
            assert all(np.isfinite(v).all() for v in (r.mean(), r.sd(), r.ess(), r.mass())) and np.all(r.ess() >= 1)
            assert np.all(r.mean() >= np.array(w.pmin)) and np.all(r.mean() <= np.array(w.pmax))
        hists.append(s.summary())
        s.close()
    assert hists[0].hist.tobytes() == hists[1].hist.tobytes() and hists[0].prob_sum.tobytes() == hists[1].prob_sum.tobytes()
    # a shard of a sharded ladder
    shard = HipSampler(w.model, w.n_par, 4, w.data, seed=5, chain_offset=0, n_chains_global=8)
    cols = np.arange(4, dtype=np.int32)
    cfg = capi.ReweightConfig(n_cols=4, cols=cols.ctypes.data_as(C.POINTER(C.c_int32)), nbins=0)
    assert capi.lib().apemost_hip_reweight_begin(shard._h, C.byref(cfg)) == capi.ERR_UNSUPPORTED
    shard.close()


# ---- protocol and refusals --------------------------------------------------------------------------------------------
def test_protocol_wording_and_refusals():
    betas, ell, x, g = columns(4, 20, "gauss")
    s = sampler_of(4)
    L = capi.lib()
    d = torch.zeros((12, 4, 6), dtype=torch.float64, device="cuda")
    view = capi.ReweightView()
    gp = g.ctypes.data_as(capi._dp)
    out = np.zeros(64)                                         # (S0 of up to 64 targets)
    sums = capi.ReweightSums(S0=out.ctypes.data_as(capi._dp))
    bt = np.array([0.0])

    def begin(cols, nbins=5, lo=(0.0,) * 16, hi=(1.0,) * 16):
        c = np.ascontiguousarray(cols, dtype=np.int32)
        lo_, hi_ = np.array(lo[:len(c)], dtype=np.float64), np.array(hi[:len(c)], dtype=np.float64)
        cfg = capi.ReweightConfig(n_cols=len(c), cols=c.ctypes.data_as(C.POINTER(C.c_int32)), nbins=nbins,
                                  lo=lo_.ctypes.data_as(capi._dp), hi=hi_.ctypes.data_as(capi._dp))
        return L.apemost_hip_reweight_begin(s._h, C.byref(cfg))

    def evaluate(t0, n, targets=bt):
        targets = np.ascontiguousarray(targets, dtype=np.float64)
        return L.apemost_hip_reweight_evaluate(s._h, t0, n, gp, targets.ctypes.data_as(capi._dp), len(targets), C.byref(sums))
    # before begin: the protocol's words
    assert L.apemost_hip_reweight_accumulate(s._h, d.data_ptr(), 12, 0, 1) == capi.ERR_INVALID
    assert last_error() == "reweight_accumulate: no reweight_begin"
    assert L.apemost_hip_reweight_get(s._h, C.byref(view)) == capi.ERR_INVALID and last_error() == "reweight_get: no reweight_begin"
    assert evaluate(0, 1) == capi.ERR_INVALID and "no reweight_begin" in last_error()
    assert begin([0, 1]) == capi.ERR_INVALID and "no mbar_begin" in last_error()
    s.mbar_begin(20, betas)
    assert L.apemost_hip_reweight_begin(s._h, None) == capi.ERR_INVALID and last_error() == "reweight_begin: config is NULL"
    for bad in ([0, 6], [-1, 2], [2, 2], [3, 1]):
        assert begin(bad) == capi.ERR_INVALID and "strictly increasing" in last_error() and "cols[" in last_error(), bad
    assert begin(list(range(6)) + [6] * 11) == capi.ERR_INVALID and "n_cols 17 outside [1,16]" in last_error()
    assert begin([]) == capi.ERR_INVALID and "n_cols 0" in last_error()
    assert begin([0, 1], 4097) == capi.ERR_INVALID and "nbins 4097" in last_error()
    assert begin([0, 1], 5, (0.0, 1.0), (1.0, 1.0)) == capi.ERR_INVALID and "parameter 1: range [1, 1] invalid" in last_error()
    assert begin([0, 1], 5, (0.0, np.nan), (1.0, 2.0)) == capi.ERR_INVALID and "parameter 1" in last_error()
    assert L.apemost_hip_reweight_get(s._h, C.byref(view)) == capi.ERR_INVALID                 # refused begins opened nothing
    # a store above 2^30 values: the message gives the columns that fit
    s.mbar_begin(1 << 26, betas)
    assert begin([0, 1, 2, 3, 4]) == capi.ERR_INVALID and "at most 4 columns fit" in last_error()
    # the mbar fold already stores rows
    s.mbar_begin(20, betas)
    s.mbar_set(Mbar(ell, betas))
    assert begin([0, 1]) == capi.ERR_INVALID and "already stores 20 kept steps" in last_error()
    s.mbar_begin(20, betas)
    assert begin([0, 1, 2, 3], 5, LO, HI) == capi.OK
    assert L.apemost_hip_reweight_get(s._h, None) == capi.ERR_INVALID and last_error() == "reweight view is NULL"
    assert L.apemost_hip_reweight_set(s._h, None) == capi.ERR_INVALID and last_error() == "reweight view is NULL"
    assert L.apemost_hip_reweight_accumulate(s._h, d.data_ptr(), 12, 0, 0) == capi.ERR_INVALID
    assert last_error() == "reweight_accumulate: bad arguments"
    s._rw_cols, s._rw_lo, s._rw_hi, s._rw_nbins = np.arange(4, dtype=np.int32), np.array(LO), np.array(HI), 5
    s.mbar_set(Mbar(ell, betas))
    s.reweight_set(Reweight(x, np.arange(4), LO, HI, 5))
    n21 = np.array([21], dtype=np.uint64)
    assert L.apemost_hip_reweight_set(s._h, C.byref(capi.ReweightView(n=n21.ctypes.data_as(capi._up)))) == capi.ERR_INVALID
    assert "beyond capacity = 20" in last_error()
    # the refusals of mbar_iterate, and the targets
    for t0, n in ((0, 0), (20, 1), (5, 16)):
        assert evaluate(t0, n) == capi.ERR_INVALID and "go past the 20 stored" in last_error()
    for bad in (-0.5, np.inf, np.nan):
        assert evaluate(0, 20, [1.0, bad]) == capi.ERR_INVALID and "target 1 is" in last_error()
        assert L.apemost_hip_reweight_weights(s._h, 0, 20, gp, bad, None, None) == capi.ERR_INVALID
    assert evaluate(0, 20, []) == capi.ERR_INVALID and "n_t 0 outside [1,64]" in last_error()
    assert evaluate(0, 20, [1.0] * 65) == capi.ERR_INVALID and "n_t 65 outside [1,64]" in last_error()
    assert L.apemost_hip_reweight_evaluate(s._h, 0, 20, None, bt.ctypes.data_as(capi._dp), 1, C.byref(sums)) == capi.ERR_INVALID
    bad_g = g.copy()
    bad_g[2] = np.nan
    assert L.apemost_hip_reweight_evaluate(s._h, 0, 20, bad_g.ctypes.data_as(capi._dp), bt.ctypes.data_as(capi._dp), 1,
                                           C.byref(sums)) == capi.ERR_INVALID and "g[2]" in last_error()
    assert evaluate(0, 20) == capi.OK and out[0] >= 1
    assert L.apemost_hip_reweight_weights(s._h, 0, 20, gp, 0.0, None, None) == capi.OK         # any pointer may be NULL
    # more than 2^24 counts
    s.mbar_begin(20, betas)
    assert begin([0, 1, 2, 3], 4096, LO, HI) == capi.OK
    s.mbar_set(Mbar(ell, betas))
    s._rw_nbins = 4096
    s.reweight_set(Reweight(x, np.arange(4), LO, HI, 4096))
    assert evaluate(0, 20, [1.0] * 64) == capi.OK                                            # 4 x 64 x 4096 = 2^20
    s.mbar_begin(20, betas)
    assert L.apemost_hip_reweight_get(s._h, C.byref(view)) == capi.ERR_INVALID                 # mbar_begin dropped it
    assert last_error() == "reweight_get: no reweight_begin"
    assert begin([0, 1]) == capi.OK
    s.mbar_end()
    assert L.apemost_hip_reweight_get(s._h, C.byref(view)) == capi.ERR_INVALID                 # and so did mbar_end
    s.close()


def test_more_than_2_24_counts_are_refused():
    """ladders x 64 targets x 4 columns x 4096 bins: 8 ladders are 2^23 counts, 32 are 2^25"""
    L = capi.lib()
    w = wl.simplesin(n_data=16, n_chain=2)
    bt = np.ones(64)
    for n_lad, code in ((8, capi.OK), (32, capi.ERR_INVALID)):
        s = HipSampler.batch(w.model, w.n_par, 2, np.stack([w.data] * n_lad), list(range(1, n_lad + 1)))
        betas = np.tile([1.0, 0.5], n_lad)
        s.mbar_begin(4, betas)
        s.reweight_begin(None, LO, HI, 4096)
        ell = -np.arange(8.0 * n_lad).reshape(4, 2 * n_lad)
        s.mbar_set(Mbar(ell, betas, n_lad))
        s.reweight_set(Reweight(np.zeros((4, 4, 2 * n_lad)), np.arange(4), LO, HI, 4096, n_lad))
        g, out = np.zeros(2 * n_lad), np.zeros(n_lad * 64)
        sums = capi.ReweightSums(S0=out.ctypes.data_as(capi._dp))
        assert L.apemost_hip_reweight_evaluate(s._h, 0, 4, g.ctypes.data_as(capi._dp), bt.ctypes.data_as(capi._dp), 64,
                                               C.byref(sums)) == code
        if code == capi.OK:
            assert np.all(out >= 1)
        else:
            assert "32 ladders x 64 targets x 4 columns x 4096 bins are more than 2^24 counts" in last_error()
        s.close()
