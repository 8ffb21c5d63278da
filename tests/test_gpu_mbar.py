"""On-device MBAR (apemost_hip_mbar_*, pt_mbar.h) against tests/mbar_ref.py, a restatement that shares nothing with the
kernels or with apemost_amd/mbar.py and sums exactly (math.fsum over numpy's exp).

The rule for every test.  What the header states as exact is compared with == on the bits: the store (one IEEE
division), the order of the sums (n_iter updates against n_iter calls, a range against a fold of only its rows, a
ladder of a batch against its own sampler, G of an evaluation against the next iteration's g).  What goes through exp
and log is compared with the reference under a bound derived here, with u = 2^-53 and exp, log good to one ulp = 2 u on
either side (the device library's bound and numpy's):

  lnD.  x_j = beta_j l + c_j is the same two IEEE operations on the same inputs on both sides, and so is x_j - m: no
  difference.  S = sum_j exp(x_j - m) >= 1: 2 u per exp on either side, (K - 1) u for the device's sequential sum, u for
  the reference's one rounding: relative 4 u + (K + 1) u.  log(S) <= ln K: 2 u ln K on either side; the last add rounds to
  u |lnD| on either side.  So  E_D = 4 u (1 + ln K) + (K + 1) u + 2 u max|lnD|  bounds |lnD_device - lnD_ref|.
  x_tn = beta_t l_n - lnD_n: the absolute error of lnD enters directly, and the difference rounds to u |x| on either
  side:  E_x = E_D + 2 u max|x_tn|.  It bounds the maxima m_t too.
  S0.  The argument x_tn - m_t differs by at most 2 E_x and rounds to u |x_tn - m_t| on either side; no term with
  |x_tn - m_t| > 745 is other than 0, so that is at most 745 * 2 u relative to the term; 2 u per exp on either side; a
  term passes at most 63 lane additions, 6 of the tree and tiles - 1 of the tiles on the device, one rounding in the
  reference:  R0 = 2 E_x + 745 * 2 u + 4 u + (70 + tiles) u  bounds the relative error of S0 (its terms are positive).
  G_t = m_t + log(S0):  tol_G = E_x + R0 + 2^-51 ln N + 2^-52 max|G|  (log(S0) <= ln N, one ulp per log on either side,
  the last add).  A free energy relative to g_0 is a difference of two of them: 2 tol_G.
  S2 and SS have positive terms like S0: S2 carries two more products on either side (R0 + 4 u), SS the square of e
  and one product on either side (2 R0 + 2 u).  S1's terms change sign and carry one product on either side: (R0 + 2 u)
  times A1 = sum e |d|, which the reference computes.  d = l_n - l_first is the same operation on both sides.
The tests print the worst error they saw beside the bound."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.mbar import Mbar
from apemost_amd.sampler import HipSampler
from tests import mbar_ref
from tests.evidence_ref import same_floats
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
D = 4


def sampler_of(n_chains, n_ladders=1):
    w = wl.simplesin(n_data=16, n_chain=n_chains // n_ladders)
    if n_ladders == 1:
        return HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    return HipSampler.batch(w.model, w.n_par, n_chains // n_ladders, np.stack([w.data] * n_ladders), list(range(1, n_ladders + 1)))


def loaded(ell, betas, n_ladders=1, capacity=None):
    """(sampler, its Mbar) with the store ell [n][n_chains] loaded through mbar_set"""
    ell = np.ascontiguousarray(ell)
    s = sampler_of(ell.shape[1], n_ladders)
    s.mbar_begin(capacity or len(ell), betas)
    s.mbar_set(Mbar(ell, betas, n_ladders))
    mb = s.mbar()
    assert mb.ell.tobytes() == ell.tobytes() and mb.n == len(ell)
    return s, mb


def last_error():
    return capi.lib().apemost_hip_last_error().decode()


def columns(K, T, kind, seed=11):
    """(betas, ell [T][K], g): the Gaussian columns of the conjugate problem, or the same with 10^4 between
    neighbouring chains, so that most exps underflow and the maxima carry the result; g is a rough guess"""
    betas, ell = mbar_ref.conjugate(K, T, D, seed=seed)
    g = mbar_ref.ln_z_exact(betas, D) + 0.05 * np.cos(np.arange(K))
    if kind == "spread":
        ell = ell - 1.0e4 * np.arange(K)
    return betas, ell, g


# ---- the store ------------------------------------------------------------------------------------------------------
def test_the_store():
    """the rows of the evidence fold's hand-built test: 300 chains, three calls with skip 2 and thin 3"""
    from tests.test_gpu_evidence import calls_of, hand_built, on_device
    rows, _, _ = hand_built()
    calls, kept = calls_of([81, 92, 87], 3, 2)
    betas = 0.01 ** (np.arange(300) / 299.0)
    want = rows[kept][:, :, 5] / betas
    n_bad = int((~np.isfinite(want)).sum())
    assert n_bad >= 2 * 111                                   # (steps 41 and 131 of the 111 chains of kinds 5, 6, 7)
    s = sampler_of(300)
    d = on_device(rows)
    L = capi.lib()
    s.mbar_begin(len(kept), betas)
    for first, n, skip in calls:
        s.mbar_accumulate(d[first:].data_ptr(), n, skip, 3)
    three = s.mbar()
    assert three.n == len(kept) == 86 and same_floats(three.ell, want) and int(three.n_bad[0]) == n_bad
    # one step too many
    assert L.apemost_hip_mbar_accumulate(s._h, d.data_ptr(), 1, 0, 1) == capi.ERR_INVALID
    assert "beyond capacity = 86" in last_error()
    assert L.apemost_hip_mbar_accumulate(s._h, d.data_ptr(), 260, 260, 1) == capi.OK      # keeps nothing
    # the count refuses the passes, and says why
    g = np.zeros(300)
    assert L.apemost_hip_mbar_iterate(s._h, 0, 86, 1, g.ctypes.data_as(capi._dp), None) == capi.ERR_INVALID
    assert "stores %d values that are not finite" % n_bad in last_error()
    with pytest.raises(ValueError, match="%d values that are not finite" % n_bad):
        Mbar.from_rows(rows[kept], betas).solve_numpy()
    # three calls equal one
    s.mbar_begin(len(kept), betas)
    s.mbar_accumulate(d.data_ptr(), 260, 2, 3)
    one = s.mbar()
    assert same_floats(one.ell, three.ell) and one.n_bad.tobytes() == three.n_bad.tobytes()
    assert same_floats(Mbar.from_rows(rows[kept], betas).ell, one.ell)
    # get -> begin -> set -> get
    s.mbar_begin(100, betas)
    assert s.mbar().n == 0
    s.mbar_set(one)
    back = s.mbar()
    assert back.n == 86 and same_floats(back.ell, one.ell) and back.n_bad.tobytes() == one.n_bad.tobytes()
    s.mbar_accumulate(d.data_ptr(), 14, 0, 1)
    assert s.mbar().n == 100 and same_floats(s.mbar().ell[86:], rows[:14, :, 5] / betas)
    s.mbar_end()
    s.close()


# ---- one iteration against the reference ----------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "spread"])
@pytest.mark.parametrize("K,T", [(1, 50), (5, 1), (5, 1639), (70, 60)])
def test_one_iteration_from_a_given_g(K, T, kind):
    """one sample tile and a ragged one; two full tiles and one of 3 samples; more targets than a wave and than a
    group of 16"""
    betas, ell, g = columns(K, T, kind)
    s, mb = loaded(ell, betas)
    got, prev = mb.iterate(g, 1)
    s.close()
    want, lnD = mbar_ref.one_iteration(ell, betas, g)
    assert prev.tobytes() == g.tobytes()
    worst, bound = float(np.abs(got - want).max()), mbar_ref.tol_G(K, ell, lnD, betas, want)
    print("K = %d, T = %d, %s: worst |g - ref| %.3g, bound %.3g" % (K, T, kind, worst, bound))
    assert worst <= bound
    host, _ = Mbar(ell, betas).iterate(g, 1)                   # the same order with numpy's exp: the same bound
    assert float(np.abs(host - want).max()) <= bound


@pytest.mark.parametrize("kind", ["gauss", "spread"])
def test_one_iteration_of_a_batch_and_its_ladders_alone(kind):
    K, T = 5, 300
    parts = [columns(K, T, kind, seed=40 + b) for b in range(3)]
    betas = np.concatenate([p[0] * (1 - 0.1 * b) for b, p in enumerate(parts)])
    ell = np.concatenate([p[1] for p in parts], axis=1)
    g = np.concatenate([p[2] for p in parts])
    s, mb = loaded(ell, betas, 3)
    got, _ = mb.iterate(g, 1)
    sums = mb.evaluate([0.0, 0.3, 1.5], g=got)
    w = mb.log_weights(0.3, g=got)
    s.close()
    for b in range(3):
        k = slice(b * K, (b + 1) * K)
        want, lnD = mbar_ref.one_iteration(ell[:, k], betas[k], g[k])
        worst, bound = float(np.abs(got[k] - want).max()), mbar_ref.tol_G(K, ell[:, k], lnD, betas[k], want)
        print("ladder %d, %s: worst %.3g, bound %.3g" % (b, kind, worst, bound))
        assert worst <= bound
        one_s, one = loaded(ell[:, k], betas[k])
        alone, _ = one.iterate(g[k], 1)
        alone_sums = one.evaluate([0.0, 0.3, 1.5], g=alone)
        alone_w = one.log_weights(0.3, g=alone)
        one_s.close()
        assert alone.tobytes() == got[k].tobytes()
        for word in ("m", "S0", "S1", "S2", "SS", "G"):
            assert alone_sums[word][0].tobytes() == sums[word][b].tobytes(), word
        assert alone_sums["ell_first"][0] == sums["ell_first"][b] == ell[0, b * K]
        assert alone_w.tobytes() == np.ascontiguousarray(w[:, k]).tobytes()


# ---- order, on the bits -----------------------------------------------------------------------------------------------
def test_the_order_is_fixed():
    K, T = 5, 1639
    betas, ell, g = columns(K, T, "gauss", seed=5)
    s, mb = loaded(ell, betas)
    one, p1 = mb.iterate(g, 1)
    two, p2 = mb.iterate(g, 2)
    again, _ = mb.iterate(one, 1)
    assert p2.tobytes() == one.tobytes() and two.tobytes() == again.tobytes() and one.tobytes() != two.tobytes()
    three, p3 = mb.iterate(g, 3)
    assert p3.tobytes() == two.tobytes() and three.tobytes() == mb.iterate(two, 1)[0].tobytes()
    # a range against a fold that holds only its rows: 900 steps = 4500 samples, a tile and a ragged one, starting
    # inside a tile of the whole store
    t0, n = 333, 900
    targets = [0.0, 0.4, 1.0]
    part_g, _ = mb.iterate(g, 2, t0, n)
    part = mb.evaluate(targets, g=part_g, t0=t0, t_count=n)
    part_w = mb.log_weights(0.4, g=part_g, t0=t0, t_count=n)
    s.close()
    fs, fresh = loaded(ell[t0:t0 + n], betas)
    fresh_g, _ = fresh.iterate(g, 2)
    whole = fresh.evaluate(targets, g=fresh_g)
    whole_w = fresh.log_weights(0.4, g=fresh_g)
    fs.close()
    assert part_g.tobytes() == fresh_g.tobytes() and part_w.tobytes() == whole_w.tobytes()
    for word in ("m", "S0", "S1", "S2", "SS", "G", "ell_first"):
        assert part[word].tobytes() == whole[word].tobytes(), word


# ---- evaluate -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["gauss", "spread"])
def test_evaluate_against_the_reference(kind):
    K, T = 5, 1639
    betas, ell, g = columns(K, T, kind, seed=9)
    targets = np.concatenate([[0.0], betas, (betas[:-1] + betas[1:]) / 2, [1.5]])     # 11: two pieces of at most K
    s, mb = loaded(ell, betas)
    got = mb.evaluate(targets, g=g)
    nxt, _ = mb.iterate(g, 1)
    w = mb.log_weights(0.5, g=g)
    s.close()
    assert got["G"][0, 1:1 + K].tobytes() == nxt.tobytes()         # the same kernel order
    assert got["ell_first"][0] == ell[0, 0]
    N, tiles = ell.size, (ell.size + 4095) // 4096
    lnD = mbar_ref.ln_d(ell, betas, g)
    for t, bt in enumerate(targets.tolist()):
        ref = mbar_ref.sums(ell, lnD, bt)
        E_x, R0 = mbar_ref.bounds(K, tiles, lnD, ref["x_abs_max"])
        err = {"m": abs(got["m"][0, t] - ref["m"]) / E_x,
               "S0": abs(got["S0"][0, t] / ref["S0"] - 1) / R0,
               "S1": abs(got["S1"][0, t] - ref["S1"]) / ((R0 + 2 * U) * ref["A1"]) if ref["A1"] > 0 else 0.0,
               "S2": abs(got["S2"][0, t] / ref["S2"] - 1) / (R0 + 4 * U) if ref["S2"] > 0 else float(got["S2"][0, t] != 0),
               "SS": abs(got["SS"][0, t] / ref["SS"] - 1) / (2 * R0 + 2 * U),
               "G": abs(got["G"][0, t] - ref["G"]) / mbar_ref.tol_G(K, ell, lnD, [bt], np.array([ref["G"]]))}
        print("%s, beta_t = %.4g: error over bound %s (E_x %.3g, R0 %.3g)"
              % (kind, bt, " ".join("%s %.3f" % kv for kv in err.items()), E_x, R0))
        assert all(v <= 1 for v in err.values()), (bt, err)
        assert got["S0"][0, t] >= 1 and got["SS"][0, t] >= 1       # the maximum's own term is exp(0)
    total = np.exp(w).sum()
    print("%s: sum of the weights - 1 = %.3g, bound %.3g" % (kind, total - 1, N * 2.0 ** -50))
    assert w.shape == (T, K) and abs(total - 1) <= N * 2.0 ** -50


# ---- the solve --------------------------------------------------------------------------------------------------------
def test_solve_the_conjugate_problem_on_the_device():
    K, T = 8, 2000
    betas, ell = mbar_ref.conjugate(K, T, D)
    s, mb = loaded(ell, betas)
    used, change = mb.solve(tol=1e-10)
    assert change <= 1e-10 and used <= 10000
    g = mb.free_energy()
    G, lnD = mbar_ref.one_iteration(ell, betas, g)
    moved, bound = float(np.abs((G - G[0]) - g).max()), 1e-10 + 2 * mbar_ref.tol_G(K, ell, lnD, betas, G)
    print("%d iterations; the reference's map moves the result by %.3g, bound %.3g" % (used, moved, bound))
    assert moved <= bound
    targets = np.append(betas, 0.0)
    want = mbar_ref.ln_z_exact(targets, D) - mbar_ref.ln_z_exact(betas[0], D)
    got, err = mb.ln_z(targets), mb.error(blocks=10, what="ln_z", betas=targets)
    print("ln_z - exact:", got - want, "block error:", err)
    assert np.all(np.abs(got - want) <= 5 * err)
    mean, merr = mb.mean_loglike(targets), mb.error(blocks=10, what="mean_loglike", betas=targets)
    assert np.all(np.abs(mean - mbar_ref.mean_exact(targets, D)) <= 5 * merr)
    assert abs(mb.ln_evidence() - mbar_ref.ln_z_exact(1.0, D)) <= 5 * float(mb.error(blocks=10))
    assert np.all(mb.ess(betas) >= T)
    host = Mbar(ell, betas)
    host.solve_numpy(tol=1e-10)
    assert np.all(np.abs(host.free_energy() - g) <= 1e-9)
    s.close()


# ---- a real run -------------------------------------------------------------------------------------------------------
def test_a_real_run_beside_the_evidence_fold():
    n_chain, n_rounds, n_swap, bs = 8, 150, 10, 17
    from apemost_amd.summary import batches_closed
    w = wl.simplesin(n_data=16, n_chain=n_chain)
    st, _, _ = make_pair(w, n_chain, seed=5)
    half = n_rounds * n_swap
    nb = batches_closed(2 * half, bs)
    words = []
    for with_mbar in (True, False):
        s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=5)
        s.set_state(st)
        d = torch.zeros((2 * half, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
        s.evidence_begin(batch_size=bs, max_batches=nb)
        if with_mbar:
            s.mbar_begin(2 * half)
        for first in (0, half):
            s.run_sampler(n_rounds, n_swap, d[first:].data_ptr())
            s.evidence_accumulate(d[first:].data_ptr(), half)
            if with_mbar:
                s.mbar_accumulate(d[first:].data_ptr(), half)
        if with_mbar:
            mb = s.mbar()
            rows = d.cpu().numpy()
            host = Mbar.from_rows(rows, st.beta)
            assert mb.n == 2 * half and mb.ell.tobytes() == host.ell.tobytes() and int(mb.n_bad[0]) == 0
            assert mb.betas.tobytes() == st.beta.tobytes()
            g, _ = mb.iterate(mb.start(), 5)
            host_g, _ = host.iterate(host.start(), 5)
            assert np.isfinite(g).all() and np.all(np.abs(g - host_g) <= 1e-9 * np.abs(host_g).max())
        words.append(s.evidence())
        s.close()
    for f in ("origin", "sum", "sq", "batch", "m", "S"):
        assert getattr(words[0], f).tobytes() == getattr(words[1], f).tobytes(), f
    assert int(words[0].n[0]) == 2 * half
    # a shard of a sharded ladder
    shard = HipSampler(w.model, w.n_par, 4, w.data, seed=5, chain_offset=0, n_chains_global=8)
    with pytest.raises(capi.ApemostHipError) as e:
        shard.mbar_begin(10, st.beta[:4])
    assert e.value.code == capi.ERR_UNSUPPORTED
    shard.close()


# ---- protocol and refusals --------------------------------------------------------------------------------------------
def test_protocol_wording_and_refusals():
    betas, ell, g = columns(4, 20, "gauss")
    s = sampler_of(4)
    L = capi.lib()
    d = torch.zeros((12, 4, 6), dtype=torch.float64, device="cuda")
    view, eview = capi.MbarView(), capi.EvidenceView()
    said = []
    for fold in ("mbar", "evidence"):                         # before begin: as the evidence fold words it
        acc, get = getattr(L, "apemost_hip_%s_accumulate" % fold), getattr(L, "apemost_hip_%s_get" % fold)
        msgs = []
        assert acc(s._h, d.data_ptr(), 12, 0, 1) == capi.ERR_INVALID
        msgs.append(last_error())
        assert get(s._h, C.byref(view if fold == "mbar" else eview)) == capi.ERR_INVALID
        msgs.append(last_error())
        said.append([m.replace(fold, "FOLD") for m in msgs])
    assert said[0] == said[1] and said[0][0] == "FOLD_accumulate: no FOLD_begin"
    gp = g.ctypes.data_as(capi._dp)
    assert L.apemost_hip_mbar_iterate(s._h, 0, 1, 1, gp, None) == capi.ERR_INVALID and "no mbar_begin" in last_error()
    s.mbar_begin(20, betas)
    assert L.apemost_hip_mbar_get(s._h, None) == capi.ERR_INVALID and last_error() == "mbar view is NULL"
    assert L.apemost_hip_mbar_set(s._h, None) == capi.ERR_INVALID and last_error() == "mbar view is NULL"
    assert L.apemost_hip_mbar_accumulate(s._h, d.data_ptr(), 12, 0, 0) == capi.ERR_INVALID
    assert last_error() == "mbar_accumulate: bad arguments"
    s.mbar_set(Mbar(ell, betas))

    def begin(capacity, b):
        b = np.ascontiguousarray(b, dtype=np.float64)
        cfg = capi.MbarConfig(capacity=capacity, betas=b.ctypes.data_as(capi._dp))
        return L.apemost_hip_mbar_begin(s._h, C.byref(cfg))
    # refused begins leave the fold as it was
    assert L.apemost_hip_mbar_begin(s._h, None) == capi.ERR_INVALID
    for bad in ([1.0, 0.5, 0.25, 0.0], [1.0, 0.5, 0.5, 0.1], [1.0, np.nan, 0.2, 0.1], [0.5, 1.0, 0.2, 0.1]):
        assert begin(20, bad) == capi.ERR_INVALID and "strictly decreasing" in last_error(), bad
    assert begin(0, betas) == capi.ERR_INVALID
    assert begin((1 << 26) + 1, betas) == capi.ERR_INVALID and "[1, %d]" % (1 << 26) in last_error()
    assert s.mbar().n == 20
    for t0, n in ((0, 0), (20, 1), (5, 16)):
        assert L.apemost_hip_mbar_iterate(s._h, t0, n, 1, gp, None) == capi.ERR_INVALID and "go past the 20 stored" in last_error()
    assert L.apemost_hip_mbar_iterate(s._h, 0, 20, 0, gp, None) == capi.ERR_INVALID
    out = np.zeros(1)
    sums = capi.MbarSums(G=out.ctypes.data_as(capi._dp))
    for bad in (-0.5, np.inf, np.nan):
        bt = np.array([bad])
        assert L.apemost_hip_mbar_evaluate(s._h, 0, 20, gp, bt.ctypes.data_as(capi._dp), 1, C.byref(sums)) == capi.ERR_INVALID
    bt = np.array([0.0])
    assert L.apemost_hip_mbar_evaluate(s._h, 0, 20, gp, bt.ctypes.data_as(capi._dp), 1, C.byref(sums)) == capi.OK
    assert np.isfinite(out[0])
    # a second begin drops the fold begun before
    s.mbar_begin(5, betas)
    assert s.mbar().n == 0
    assert L.apemost_hip_mbar_accumulate(s._h, d.data_ptr(), 12, 0, 2) == capi.ERR_INVALID     # 6 > 5
    s.mbar_end()
    assert L.apemost_hip_mbar_get(s._h, C.byref(view)) == capi.ERR_INVALID and last_error() == "mbar_get: no mbar_begin"
    s.close()
