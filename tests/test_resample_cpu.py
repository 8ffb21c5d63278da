"""Resampling on the host (apemost_amd/reweight.py: systematic_positions, Reweight.resample_numpy, Resampled and
resample.bin) against tests/resample_ref.py, a restatement in Python integers with bisect.  The rule has no floating
point, so everything given q is compared with ==.  The estimator is held to the project's 5 standard errors on the
conjugate problem (tests/test_reweight_cpu.py, check_conjugate): the draws of M from a weighted sample of Kish size ESS
carry the variance of both, v / ESS + v / M for a mean and v^2 (2 / ESS + 2 / M) for a variance, v = 1 / (1 + beta)."""
import math

import numpy as np
import pytest

from apemost_amd.mbar import Mbar
from apemost_amd.reweight import Resampled, Reweight, systematic_positions
from tests import resample_ref, reweight_ref
from tests.test_reweight_cpu import D, HI, LO, columns

US = (0, 1, 1 << 63, (1 << 64) - 1)
TARGETS = (1.0, 0.3, 0.0, 1.5)


def draws_of(N):
    return (1, 7, N, 3 * N)


@pytest.mark.parametrize("Q,M", [(1 << 34, 1), (1 << 34, 1 << 20), ((1 << 63) - 1, 1 << 24), (12345678901234567, 4096),
                                 (7, 7), (22, 7)])
def test_positions_are_the_references(Q, M):
    for u in US + (0x9E3779B97F4A7C15,) if M < 1 << 24 else US[-1:]:
        p = systematic_positions(Q, M, u)
        assert p.dtype == np.uint64 and len(p) == M
        some = sorted(set([0, 1, M // 2, M - 2, M - 1]) & set(range(M)))
        a, b = divmod(Q, M)
        assert [int(p[m]) for m in some] == [m * a + (m * b) // M + ((u * a) >> 64) for m in some]
        if M <= 4096:
            assert [int(v) for v in p] == resample_ref.positions(Q, M, u)
        assert np.all(p[1:] >= p[:-1])
        assert int(p[-1]) < Q
    for bad in ((Q, 0, 0), (Q, (1 << 24) + 1, 0), (Q, M, 1 << 64), (Q, M, -1), (1 << 63, M, 0), (M - 1, M, 0)):
        with pytest.raises(ValueError):
            systematic_positions(*bad)


@pytest.mark.parametrize("kind", ["gauss", "spread"])
@pytest.mark.parametrize("K,T", [(3, 50), (5, 1639)], ids=["N150", "N8195"])
def test_resample_numpy_is_the_reference(K, T, kind):
    """below one tile, and two tiles and three samples; with `spread` nearly every q is zero"""
    betas, ell, x, g = columns(K, T, kind)
    mb = Mbar(ell, betas)
    rw = Reweight(x, np.arange(D), LO, HI, 0)
    N = K * T
    for bt in (1.0, 0.3):
        _, q = rw.weights(mb, bt, g=g, t0=0, t_count=T)
        q = [int(v) for v in q.reshape(-1)]
        if kind == "spread":
            assert sum(v > 0 for v in q) <= T                    # (one chain's samples at the most: M = N exceeds them)
        for M in draws_of(N):
            for u in US:
                r = rw.resample_numpy(mb, bt, M, u, g=g, t0=0, t_count=T)
                want, Q = resample_ref.draws(q, M, u)
                assert r.index.dtype == np.uint32 and r.index[0].tolist() == want, (bt, M, u)
                assert int(r.q_total[0]) == Q and r.shift == reweight_ref.shift_of(N)
                resample_ref.check_rule(q, r.index[0], M, u)
                assert r.counts().tolist() == resample_ref.counts(want, N)
                flat = x.reshape(D, -1)
                assert r.x[0].tobytes() == np.ascontiguousarray(flat[:, want].T).tobytes()
                assert r.step[0].tolist() == [n // K for n in want] and r.chain[0].tolist() == [n % K for n in want]
    # a range equals a store of only its rows; resample() without a device is resample_numpy
    part = rw.resample(mb, 0.3, 500, 12345, g=g, t0=T // 5, t_count=T // 2)
    alone = Reweight(x[:, T // 5:T // 5 + T // 2], np.arange(D)).resample_numpy(
        Mbar(ell[T // 5:T // 5 + T // 2], betas), 0.3, 500, 12345, g=g, t0=0, t_count=T // 2)
    assert part.index.tobytes() == alone.index.tobytes() and part.x.tobytes() == alone.x.tobytes()
    assert part.step[0].tolist() == (alone.step[0] + T // 5).tolist()


def test_a_batch_its_ladders_and_the_files(tmp_path):
    K, T = 5, 300
    parts = [columns(K, T, "gauss", seed=40 + b) for b in range(2)]
    betas = np.concatenate([p[0] * (1 - 0.1 * b) for b, p in enumerate(parts)])
    ell = np.concatenate([p[1] for p in parts], axis=1)
    x = np.concatenate([p[2] for p in parts], axis=2)
    g = np.concatenate([p[3] for p in parts])
    rw = Reweight(x[1:4], [1, 2, 5], n_ladders=2, thin=3)
    mb = Mbar(ell, betas, 2)
    u = (1 << 64) - 3
    both = [rw.resample_numpy(mb, bt, 257, u, g=g, t0=10, t_count=280) for bt in (1.0, 0.25)]
    r = both[0]
    assert r.index.shape == (2, 257) and r.x.shape == (2, 257, 3) and r.mean().shape == (2, 3) and r.cov().shape == (2, 3, 3)
    ones = r.per_ladder()
    for b, one in enumerate(ones):
        k = slice(b * K, (b + 1) * K)
        alone = Reweight(x[1:4, :, k], [1, 2, 5], thin=3).resample_numpy(Mbar(ell[:, k], betas[k]), 1.0, 257, u, g=g[k],
                                                                         t0=10, t_count=280)
        for w in ("index", "x", "q_total"):
            assert getattr(one, w).tobytes() == getattr(alone, w).tobytes(), (b, w)
        assert r.chain[b].tolist() == (alone.chain[0] + b * K).tolist() and r.step[b].tolist() == alone.step[0].tolist()
        assert one.mean().tobytes() == np.ascontiguousarray(r.mean()[b]).tobytes()
    # resample.bin
    path = str(tmp_path / "resample.bin")
    Resampled.write_all(path, both)
    back = Resampled.read_all(path)
    assert len(back) == 2 and Resampled.read(path, 1).index.tobytes() == both[1].index.tobytes()
    for got, want in zip(back, both):
        for w in ("index", "x", "q_total", "cols"):
            assert getattr(got, w).tobytes() == getattr(want, w).tobytes() and getattr(got, w).dtype == getattr(want, w).dtype, w
        assert (got.beta, got.u, got.n_draws, got.shift, got.n_ladders, got.n_chains, got.n, got.thin, got.range) == \
            (want.beta, u, 257, want.shift, 2, 2 * K, T, 3, (10, 280))
    with open(path, "rb") as f:
        raw = f.read()
    Resampled.write_all(path, back)
    with open(path, "rb") as f:
        assert f.read() == raw
    both[1].write(path)
    assert Resampled.read(path).beta == 0.25 and len(Resampled.read_all(path)) == 1
    with open(path, "wb") as f:
        f.write(raw[:-8])
    with pytest.raises(ValueError, match="bytes, expected"):
        Resampled.read(path)
    with open(path, "wb") as f:
        f.write(b"APEMOSTW" + raw[8:])
    with pytest.raises(ValueError, match="not a resample file"):
        Resampled.read(path)
    with pytest.raises(ValueError, match="share the store"):
        Resampled.write_all(path, [both[0], rw.resample_numpy(mb, 0.25, 256, u, g=g, t0=10, t_count=280)])
    # the text dumps and the text of one ladder
    with pytest.raises(ValueError, match="per_ladder"):
        r.write_dumps(tmp_path)
    with pytest.raises(ValueError, match="per_ladder"):
        r.text()
    one = ones[1]
    paths = one.write_dumps(tmp_path, ["a", "b", "c"], t=3)
    assert [p.split("/")[-1] for p in paths] == ["a-reweighted-3.dump", "b-reweighted-3.dump", "c-reweighted-3.dump"]
    for a, p in enumerate(paths):
        with open(p) as f:
            lines = f.read().splitlines()
        assert lines == ["%.15e" % v for v in one.x[0, :, a].tolist()]
        assert np.array([float(v) for v in lines]).tobytes() == np.array([float("%.15e" % v) for v in one.x[0, :, a]]).tobytes()
    lines = one.text(["a", "b", "c"]).splitlines()
    f = lines[1].split("\t")
    assert len(lines) == 3 and f[:2] == ["%.15e" % 1.0, "b"] and f[2] == "%.15e" % one.mean()[1] and f[3] == "%.15e" % one.sd()[1]
    assert f[4] == "%.15e" % np.sort(one.x[0, :, 1])[128]                               # (257 draws: the 129th)
    # exact quantiles from the sorted draws
    v = np.sort(one.x[0, :, 0])
    assert one.quantile([0.0, 1.0 / 257, 0.5, 1.0], 0).tolist() == [v[0], v[0], v[128], v[256]]
    assert np.allclose(np.diagonal(one.cov()), one.sd() ** 2)


def test_refusals_on_the_host():
    betas, ell, x, g = columns(4, 20, "gauss")
    mb = Mbar(ell, betas)
    rw = Reweight(x, np.arange(D), LO, HI, 5)
    for bad in (0, (1 << 24) + 1):
        with pytest.raises(ValueError, match="n_draws %d outside" % bad):
            rw.resample_numpy(mb, 1.0, bad, 0, g=g)
    with pytest.raises(ValueError, match="1 ladders x 16777216 draws x 5 columns are more than 2\\^26 values"):
        Reweight(np.concatenate([x, x[:1]]), np.arange(5)).resample_numpy(mb, 1.0, 1 << 24, 0, g=g)
    with pytest.raises(ValueError, match="u is a uint64"):
        rw.resample_numpy(mb, 1.0, 16, 1 << 64, g=g)
    with pytest.raises(ValueError, match="targets"):
        rw.resample_numpy(mb, -1.0, 16, 0, g=g)
    with pytest.raises(ValueError, match="stores out of step"):
        Reweight(x[:, :19], np.arange(D)).resample_numpy(mb, 1.0, 16, 0, g=g)
    with pytest.raises(ValueError, match="no free energies"):
        rw.resample_numpy(mb, 1.0, 16, 0)


def z_of_draws(xs, beta, ess, M):
    """(worst z of the means, of the variances) of draws xs [M][D] of the conjugate problem at beta"""
    v = 1.0 / (1.0 + beta)
    z_mean = np.abs(xs.mean(axis=0)) / math.sqrt(v / ess + v / M)
    z_var = np.abs(xs.var(axis=0) - v) / (v * math.sqrt(2.0 / ess + 2.0 / M))
    return float(z_mean.max()), float(z_var.max())


def check_conjugate_draws(resample, ess, what):
    """resample(beta, M, u) -> Resampled of one ladder; ess [n_t] of the weighted sample at TARGETS"""
    worst = [0.0, 0.0]
    for t, bt in enumerate(TARGETS):
        for M in (4096, 16000):
            for u in US:
                r = resample(bt, M, u)
                zm, zv = z_of_draws(r.x[0], bt, float(ess[t]), M)
                worst = [max(worst[0], zm), max(worst[1], zv)]
                assert zm <= 5 and zv <= 5, (bt, M, u, zm, zv)
    print("%s: worst z of the means %.2f, of the variances %.2f" % (what, worst[0], worst[1]))


def test_the_conjugate_problem_on_the_host():
    K, T = 8, 2000
    betas, ell, x = reweight_ref.conjugate(K, T, D)
    mb = Mbar(ell, betas, threads=4)
    mb.solve_numpy(tol=1e-10)
    rw = Reweight(x, np.arange(D), LO, HI, 0, mbar=mb)
    ess = rw.evaluate(None, TARGETS).ess()
    check_conjugate_draws(lambda bt, M, u: rw.resample(None, bt, M, u), ess, "resample_numpy")
    # the reference on the same q gives the same draws
    _, q = rw.weights(None, 0.3)
    want, _ = resample_ref.draws([int(v) for v in q.reshape(-1)], 4096, 1 << 63)
    assert rw.resample(None, 0.3, 4096, 1 << 63).index[0].tolist() == want
