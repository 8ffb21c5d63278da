"""apemost_amd/mbar.py on the host (Mbar.from_rows, solve_numpy) against the analytic conjugate problem and against
tests/mbar_ref.py.  No GPU.

The one-iteration bound used below and in tests/test_gpu_mbar.py, where it is derived: two evaluations of G_t that
follow the stated operations, with exp and log good to one ulp each, differ by at most
    tol_G = E_x + R0 + 2^-51 ln N + 2^-52 max|G|
with E_x and R0 of mbar_ref.bounds."""
import math

import numpy as np
import pytest

from apemost_amd.mbar import Mbar, check_betas
from tests import mbar_ref

K, T, D = 8, 2000, 4


@pytest.fixture(scope="module")
def solved():
    betas, ell = mbar_ref.conjugate(K, T, D)
    mb = Mbar(ell, betas)
    rows = np.zeros((T, K, 5))
    rows[:, :, 4] = ell * betas
    assert Mbar.from_rows(rows, betas).ell.tobytes() == (rows[:, :, 4] / betas).tobytes() and mb.n == T
    used, change = mb.solve_numpy(tol=1e-10)
    assert change <= 1e-10 and used == mb.iterations
    return betas, ell, mb


tol_G = mbar_ref.tol_G


def test_ln_z_and_mean_meet_the_analytic_values(solved):
    betas, ell, mb = solved
    targets = np.append(betas, 0.0)
    want = mbar_ref.ln_z_exact(targets, D) - mbar_ref.ln_z_exact(betas[0], D)
    got, err = mb.ln_z(targets), mb.error(blocks=10, what="ln_z", betas=targets)
    print("ln_z - exact:", got - want, "block error:", err)
    assert got[0] == 0 and err[0] == 0
    assert np.all(np.abs(got - want) <= 5 * err)
    assert abs(mb.ln_evidence() - mbar_ref.ln_z_exact(1.0, D)) <= 5 * float(mb.error(blocks=10))
    mean, merr = mb.mean_loglike(targets), mb.error(blocks=10, what="mean_loglike", betas=targets)
    print("mean - exact:", mean - mbar_ref.mean_exact(targets, D), "block error:", merr)
    assert np.all(np.abs(mean - mbar_ref.mean_exact(targets, D)) <= 5 * merr)
    # Var_beta[l] = d / (2 (1 + beta)^2): a looser look, the block error of a variance is itself noisy
    var = mb.var_loglike(betas)
    assert np.all(np.abs(var / (D / (2 * (1 + betas) ** 2)) - 1) < 0.2)


def test_the_reference_alone_meets_the_condition(solved):
    """the seed was fixed after this: mbar_ref's own solve lies within 5 block errors of the analytic values"""
    betas, ell, mb = solved
    g, _ = mbar_ref.solve(ell, betas, tol=1e-10)
    targets = np.append(betas, 0.0)
    want = mbar_ref.ln_z_exact(targets, D) - mbar_ref.ln_z_exact(betas[0], D)
    got = mbar_ref.ln_z(ell, betas, g, targets)
    blocks = []
    for i in range(10):
        part = ell[i * T // 10:(i + 1) * T // 10]
        gb, _ = mbar_ref.solve(part, betas, tol=1e-10)
        blocks.append(mbar_ref.ln_z(part, betas, gb, targets))
    err = np.std(np.array(blocks), axis=0, ddof=1) / math.sqrt(10)
    assert np.all(np.abs(got - want) <= 5 * err), (got - want, err)
    assert np.all(np.abs(mb.free_energy() - g) <= 1e-9)


def test_ess_counts_at_least_a_chain(solved):
    betas, ell, mb = solved
    ess = mb.ess(betas)
    assert np.all(ess >= T) and np.all(ess <= K * T)


def test_the_fixed_point_holds_under_the_reference_map(solved):
    betas, ell, mb = solved
    g = mb.free_energy()
    G, lnD = mbar_ref.one_iteration(ell, betas, g)
    moved = np.abs((G - G[0]) - g)
    bound = 1e-10 + 2 * tol_G(K, ell, lnD, betas, G)
    print("moved by", moved.max(), "bound", bound)
    assert np.all(moved <= bound)


def test_one_numpy_iteration_against_the_reference():
    betas, ell = mbar_ref.conjugate(5, 1639, D, seed=3)
    mb = Mbar(ell, betas)
    g = np.array([0.0, 0.3, 0.7, 1.0, 1.1])
    got, prev = mb.iterate(g, 1)
    want, lnD = mbar_ref.one_iteration(ell, betas, g)
    assert prev.tobytes() == g.tobytes()
    worst, bound = np.abs(got - want).max(), tol_G(5, ell, lnD, betas, want)
    print("worst", worst, "bound", bound)
    assert worst <= bound
    two, before = mb.iterate(g, 2)
    assert before.tobytes() == got.tobytes() and two.tobytes() == mb.iterate(got, 1)[0].tobytes()
    # a sub-range is a store that holds only its rows
    sub = Mbar(ell[100:900], betas)
    assert mb.iterate(g, 1, 100, 800)[0].tobytes() == sub.iterate(g, 1)[0].tobytes()
    # log weights sum to one
    w = mb.log_weights(0.5, g=got)
    assert abs(np.exp(w).sum() - 1) <= ell.size * 2.0 ** -50


def test_write_read_round_trip(tmp_path, solved):
    betas, ell, mb = solved
    path = str(tmp_path / "mbar.bin")
    mb.write(path)
    back = Mbar.read(path)
    assert back.ell.tobytes() == mb.ell.tobytes() and back.betas.tobytes() == betas.tobytes()
    assert back.g.tobytes() == mb.g.tobytes() and back.range == mb.range == (0, T) and back.n_ladders == 1
    assert back.ln_evidence() == mb.ln_evidence()
    fresh = Mbar(ell[:7], betas)
    fresh.write(path)
    back = Mbar.read(path)
    assert back.g is None and back.n == 7
    with open(path, "ab") as f:
        f.write(b"x")
    with pytest.raises(ValueError):
        Mbar.read(path)


def test_text_and_ladders(solved):
    betas, ell, mb = solved
    lines = mb.text().split("\n")
    assert lines[-1] == "" and len(lines) == K + 2 and lines[K].startswith("ln_evidence\t")
    table = np.array([[float(x) for x in l.split("\t")] for l in lines[:K]])
    assert np.allclose(table[:, 0], betas, rtol=1e-15, atol=0) and np.allclose(table[:, 1], mb.free_energy(), atol=1e-9)
    two = Mbar(np.concatenate([ell, ell[::-1]], axis=1), np.concatenate([betas, betas]), n_ladders=2)
    two.solve_numpy(tol=1e-8, t_count=400)
    a, b = two.per_ladder()
    assert a.g.tobytes() == two.g[:K].tobytes() and b.ell.tobytes() == ell[::-1].tobytes()
    alone = Mbar(ell[:400], betas)
    alone.solve_numpy(tol=1e-8)
    assert alone.g.tobytes() == a.g.tobytes() and two.ln_evidence()[0] == alone.ln_evidence()


def test_refusals():
    for bad in ([1.0, 0.5, 0.0], [1.0, 1.0], [0.5, 1.0], [1.0, np.nan], [1.0, -0.5], [np.inf, 1.0], []):
        with pytest.raises(ValueError):
            check_betas(bad)
    with pytest.raises(ValueError):
        check_betas([1.0, 0.5, 1.0], n_ladders=2)
    check_betas([1.0, 0.5, 1.0, 0.25], n_ladders=2)
    col = np.full((6, 2), -3.0)
    col[4, 1] = np.nan
    col[2, 0] = -np.inf
    mb = Mbar.from_rows(col, [1.0, 0.5])
    assert int(mb.n_bad[0]) == 2
    with pytest.raises(ValueError, match="2 values that are not finite"):
        mb.solve_numpy()
    ok = Mbar.from_rows(np.full((6, 2), -3.0), [1.0, 0.5])
    for t0, t_count in ((0, 0), (3, 4), (7, 1)):
        with pytest.raises(ValueError):
            ok.iterate(np.zeros(2), 1, t0, t_count)
    with pytest.raises(ValueError):
        ok.ln_z([0.5])                                       # not solved
    ok.solve_numpy()
    with pytest.raises(ValueError):
        ok.ln_z([-0.1])
    with pytest.raises(RuntimeError):
        betas, ell = mbar_ref.conjugate(4, 50, D, seed=1)
        Mbar(ell, betas).solve_numpy(tol=0.0, max_iter=3, check_every=2)
