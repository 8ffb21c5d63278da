"""apemost_amd/reweight.py on the host (evaluate_numpy, the estimators, reweight.bin) against tests/reweight_ref.py, a
restatement that sums exactly.  The bounds are those of tests/test_gpu_reweight.py, derived in
reweight_ref.errors_over_bounds and tests/test_gpu_mbar.py: evaluate_numpy follows the kernels' order with numpy's exp."""
import math

import numpy as np
import pytest

from apemost_amd.mbar import Mbar, tile_sum
from apemost_amd.reweight import Reweight, Reweighted, fixed_point, shift_of
from tests import mbar_ref, reweight_ref

D = 4
LO, HI = [-4.0] * D, [4.0] * D


def columns(K, T, kind, seed=11):
    """(betas, ell [T][K], x [D][T][K], g): the conjugate problem, or its ell with 10^4 between neighbouring chains"""
    betas, ell, x = reweight_ref.conjugate(K, T, D, seed=seed)
    g = mbar_ref.ln_z_exact(betas, D) + 0.05 * np.cos(np.arange(K))
    if kind == "spread":
        ell = ell - 1.0e4 * np.arange(K)
    return betas, ell, x, g


def test_the_draws_are_mbar_refs():
    for K, T in ((8, 2000), (1, 50), (5, 1639)):
        betas, ell = mbar_ref.conjugate(K, T, D)
        b2, e2, x = reweight_ref.conjugate(K, T, D)
        assert betas.tobytes() == b2.tobytes() and ell.tobytes() == e2.tobytes() and x.shape == (D, T, K)
        assert np.array_equal(-0.5 * (np.moveaxis(x, 0, 2) ** 2).sum(axis=2), ell)


def test_shift_and_fixed_point():
    assert [shift_of(n) for n in (1, 2, 3, 4, 4095, 4096, 1 << 28)] == [62, 61, 61, 60, 51, 50, 34]
    for N in (1, 5, 8195, 1 << 28):
        assert N << shift_of(N) < 1 << 63
    e = np.array([1.0, 0.5, 2.0 ** -62, 2.0 ** -63, 3 * 2.0 ** -63, 0.0, 5e-324])
    assert fixed_point(e, 62).tolist() == [1 << 62, 1 << 61, 1, 0, 2, 0, 0]      # (ties to even)


@pytest.mark.parametrize("kind", ["gauss", "spread"])
@pytest.mark.parametrize("K,T,nbins", [(1, 50, 1), (5, 1, 2), (5, 1639, 20)])
def test_evaluate_numpy_against_the_reference(K, T, nbins, kind):
    betas, ell, x, g = columns(K, T, kind)
    targets = [1.0, 0.3, 0.0, 1.5]
    rw = Reweight(x, np.arange(D), LO, HI, nbins)
    got = rw.evaluate_numpy(Mbar(ell, betas), targets, g=g, t0=0, t_count=T)
    lnD = mbar_ref.ln_d(ell, betas, g)
    N, tiles = ell.size, (ell.size + 4095) // 4096
    assert got.shift == reweight_ref.shift_of(N)
    for t, bt in enumerate(targets):
        ref = reweight_ref.sums(x, ell, lnD, bt, LO, HI, nbins)
        E_x, R0 = mbar_ref.bounds(K, tiles, lnD, ref["x_abs_max"])
        err = reweight_ref.errors_over_bounds(got, 0, t, ref, E_x, R0, nbins)
        print("%s, K = %d, T = %d, beta_t = %.4g: error over bound %s" % (kind, K, T, bt, " ".join("%s %.3f" % kv for kv in err.items())))
        assert all(v <= 1 for v in err.values()), (bt, err)
        assert got.origin[0].tolist() == ref["origin"]
        assert int(got.hist[0, t].sum(axis=1).max()) <= int(got.q_total[0, t]) < 1 << 63


def test_the_sums_are_the_stated_operations():
    """given e, every word is one expression: the products, tile_sum, rint(ldexp), the integer bincount"""
    K, T = 5, 1639
    betas, ell, x, g = columns(K, T, "gauss", seed=3)
    rw = Reweight(x[:2], [0, 1], LO[:2], HI[:2], 7)
    mb = Mbar(ell, betas)
    got = rw.evaluate_numpy(mb, [0.3], g=g, t0=0, t_count=T)
    e, q = rw.weights(mb, 0.3, g=g, t0=0, t_count=T)
    e, q = e.reshape(-1), q.reshape(-1)
    d0, d1 = x[0].reshape(-1) - x[0, 0, 0], x[1].reshape(-1) - x[1, 0, 0]
    assert got.S0[0, 0] == tile_sum(e) and got.SS[0, 0] == tile_sum(e * e)
    assert got.S1[0, 0].tolist() == [tile_sum(e * d0), tile_sum(e * d1)]
    assert got.cross[0, 0].tolist() == [tile_sum((e * d0) * d0), tile_sum((e * d0) * d1), tile_sum((e * d1) * d1)]
    assert q.tolist() == np.rint(np.ldexp(e, got.shift)).astype(np.uint64).tolist()
    assert int(got.q_total[0, 0]) == sum(int(v) for v in q)
    sums = mb.evaluate([0.3], g=g, t0=0, t_count=T)
    assert (got.m[0, 0], got.S0[0, 0], got.SS[0, 0]) == (sums["m"][0, 0], sums["S0"][0, 0], sums["SS"][0, 0])
    # a range equals a store of only its rows; a batch its ladders
    part = rw.evaluate_numpy(mb, [0.3], g=g, t0=333, t_count=900)
    alone = Reweight(x[:2, 333:1233], [0, 1], LO[:2], HI[:2], 7).evaluate_numpy(Mbar(ell[333:1233], betas), [0.3], g=g, t0=0, t_count=900)
    for w in Reweighted._WORDS:
        assert getattr(part, w).tobytes() == getattr(alone, w).tobytes(), w


def test_the_conjugate_problem_on_the_host():
    """the estimator: means 0 and variances 1 / (1 + beta) in every coordinate within 5 analytic standard errors, the
    20-bin marginal within 5 binomial ones; the Kish size at beta = 1 exceeds one chain's draws"""
    K, T = 8, 2000
    betas, ell, x = reweight_ref.conjugate(K, T, D)
    mb = Mbar(ell, betas, threads=4)
    mb.solve_numpy(tol=1e-10)
    targets = np.array([1.0, 0.3, 0.0, 1.5])
    r = Reweight(x, np.arange(D), LO, HI, 20, mbar=mb).evaluate(None, targets)
    ess = r.ess()
    print("ESS:", ess)
    assert ess[0] > T
    check_conjugate(r, targets)


def check_conjugate(r, targets):
    ess, mean, sd = r.ess(), r.mean(), r.sd()
    mass = r.mass()
    for t, bt in enumerate(targets.tolist()):
        v = 1.0 / (1.0 + bt)
        z_mean = np.abs(mean[t]) / math.sqrt(v / ess[t])
        z_var = np.abs(sd[t] ** 2 - v) / (v * math.sqrt(2.0 / ess[t]))
        edges = r.edges(0)
        cdf = np.array([0.5 * (1 + math.erf(e / math.sqrt(2 * v))) for e in edges])
        p = np.diff(cdf)
        big = p > 20.0 / ess[t]
        z_bin = np.abs(mass[t][:, big] - p[big]) / np.sqrt(p[big] * (1 - p[big]) / ess[t])
        print("beta %.3g: ESS %.0f, worst z of the means %.2f, of the variances %.2f, of %d bins %.2f"
              % (bt, ess[t], z_mean.max(), z_var.max(), int(big.sum()), z_bin.max()))
        assert z_mean.max() <= 5 and z_var.max() <= 5 and z_bin.max() <= 5
        med = [float(r.quantile(0.5, a, t)) for a in range(r.n_cols)]
        assert np.all(np.abs(med) <= 0.4 + 5 * math.sqrt(v / ess[t]))             # (a bin is 0.4 wide)


def test_the_file_round_trip_and_the_text(tmp_path):
    K, T = 5, 300
    parts = [columns(K, T, "gauss", seed=40 + b) for b in range(2)]
    betas = np.concatenate([p[0] * (1 - 0.1 * b) for b, p in enumerate(parts)])
    ell = np.concatenate([p[1] for p in parts], axis=1)
    x = np.concatenate([p[2] for p in parts], axis=2)
    g = np.concatenate([p[3] for p in parts])
    rw = Reweight(x[1:4], [1, 2, 5], LO[:3], HI[:3], 9, n_ladders=2, thin=3)
    r = rw.evaluate_numpy(Mbar(ell, betas, 2), [1.0, 0.25], g=g, t0=10, t_count=280)
    path = str(tmp_path / "reweight.bin")
    r.write(path)
    back = Reweighted.read(path)
    for w in Reweighted._WORDS + ("cols", "betas_t", "lo", "hi"):
        assert getattr(back, w).tobytes() == getattr(r, w).tobytes() and getattr(back, w).dtype == getattr(r, w).dtype, w
    assert (back.shift, back.nbins, back.n_ladders, back.n_chains, back.n, back.thin, back.range) == \
        (r.shift, 9, 2, 2 * K, T, 3, (10, 280))
    with open(path, "rb") as f:
        raw = f.read()
    back.write(path)
    with open(path, "rb") as f:
        assert f.read() == raw
    with open(path, "wb") as f:
        f.write(raw[:-8])
    with pytest.raises(ValueError, match="bytes, expected"):
        Reweighted.read(path)
    # per ladder, and the text of one
    ones = r.per_ladder()
    for b, one in enumerate(ones):
        alone = Reweight(x[1:4, :, b * K:(b + 1) * K], [1, 2, 5], LO[:3], HI[:3], 9, thin=3).evaluate_numpy(
            Mbar(ell[:, b * K:(b + 1) * K], betas[b * K:(b + 1) * K]), [1.0, 0.25], g=g[b * K:(b + 1) * K], t0=10, t_count=280)
        for w in Reweighted._WORDS:
            assert getattr(one, w).tobytes() == getattr(alone, w).tobytes(), (b, w)
    with pytest.raises(ValueError, match="per_ladder"):
        r.text()
    lines = ones[0].text(["a", "b", "c"]).splitlines()
    assert len(lines) == 6
    f = lines[4].split("\t")
    assert f[1] == "b" and f[0] == "%.15e" % 0.25 and f[2] == "%.15e" % ones[0].mean()[1, 1] and f[4] == "%.15e" % ones[0].ess()[1]
    assert np.allclose(ones[0].corr()[0].diagonal(), 1.0) and ones[0].cov().shape == (2, 3, 3)
    w = r.weights(1)
    assert w.shape == (280, 2 * K) and abs(w[:, :K].sum() - 1) <= 1e-12 and abs(w[:, K:].sum() - 1) <= 1e-12


def test_refusals_on_the_host():
    K, T = 4, 20
    betas, ell, x, g = columns(K, T, "gauss")
    mb = Mbar(ell, betas)
    rw = Reweight(x, np.arange(D), LO, HI, 5)
    with pytest.raises(ValueError, match="stores out of step"):
        Reweight(x[:, :19], np.arange(D)).evaluate_numpy(mb, [1.0], g=g)
    for bad in ([-0.5], [np.inf], [np.nan], [], [1.0] * 65):
        with pytest.raises(ValueError, match="targets"):
            rw.evaluate_numpy(mb, bad, g=g)
    with pytest.raises(ValueError, match="strictly increasing"):
        Reweight(x[:2], [1, 1])
    with pytest.raises(ValueError, match="n_cols 17"):
        Reweight(np.zeros((17, 2, K)), np.arange(17))
    rows = np.zeros((T, K, D + 2))
    rows[:, :, :D] = np.moveaxis(x, 0, 2)
    rows[:, :, D + 1] = ell * betas
    rows[3, 1, 2] = np.nan
    rows[4, 1, 2] = np.inf
    bad = Reweight.from_rows(rows, betas, lo=LO, hi=HI, nbins=5)
    assert bad.n_bad.tolist() == [[0, 0, 2, 0]] and bad.cols.tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError, match="stores 2 values of column 2 that are not finite"):
        bad.evaluate(None, [1.0], g=g)
    with pytest.raises(ValueError, match="no free energies"):
        rw.evaluate_numpy(mb, [1.0])
