"""MBAR restated for the tests: it shares nothing with apemost_amd/mbar.py or the kernels.  lnD and every sum are
math.fsum over numpy's exp, which is exact summation and one ulp per exp, so that the error of what is returned here is
a few ulp whatever the number of samples.  One ladder at a time: ell [T][K] (kept step, chain), betas [K]."""
import math

import numpy as np


def conjugate(K=8, T=2000, d=4, seed=20080614, beta_max=1.0, beta_min=0.01):
    """the conjugate problem: l = -|x|^2 / 2 in d dimensions under the prior N(0, I), so that the chain at beta draws
    x ~ N(0, I / (1 + beta)) and ln Z(beta) = -(d / 2) ln(1 + beta).  K geometric betas from beta_max down to beta_min,
    T independent draws per chain.  Returns (betas [K], ell [T][K])."""
    rng = np.random.default_rng(seed)
    betas = beta_max * (beta_min / beta_max) ** (np.arange(K) / max(K - 1, 1)) if K > 1 else np.array([beta_max])
    x = rng.standard_normal((T, K, d)) / np.sqrt(1.0 + betas)[None, :, None]
    return betas, -0.5 * (x * x).sum(axis=2)


def ln_z_exact(beta, d=4):
    return -(d / 2.0) * np.log1p(np.asarray(beta, dtype=np.float64))


def mean_exact(beta, d=4):
    return -d / (2.0 * (1.0 + np.asarray(beta, dtype=np.float64)))


def ln_d(ell, betas, g):
    """lnD_n of every sample, [T * K] in stored order"""
    T, K = ell.shape
    c = math.log(float(T)) - np.asarray(g, dtype=np.float64)
    out = np.empty(T * K)
    for n, l in enumerate(ell.reshape(-1).tolist()):
        x = betas * l + c
        m = x.max()
        out[n] = m + math.log(math.fsum(np.exp(x - m).tolist()))
    return out


def sums(ell, lnD, beta_t):
    """dict m, S0, S1, S2, SS, G of one target, and A1 = sum e |d| (the scale of S1's error)"""
    l = ell.reshape(-1)
    x = beta_t * l - lnD
    m = float(x.max())
    e = np.exp(x - m)
    d = l - l[0]
    S0 = math.fsum(e.tolist())
    return dict(m=m, S0=S0, S1=math.fsum((e * d).tolist()), S2=math.fsum((e * d * d).tolist()),
                SS=math.fsum((e * e).tolist()), G=m + math.log(S0), A1=math.fsum((e * np.abs(d)).tolist()),
                x_abs_max=float(np.abs(x).max()))


def one_iteration(ell, betas, g):
    """G(g) at the sampled betas, [K]; also returns lnD"""
    lnD = ln_d(ell, betas, g)
    return np.array([sums(ell, lnD, bt)["G"] for bt in betas.tolist()]), lnD


def solve(ell, betas, tol=1e-10, max_iter=10000):
    g = np.zeros(len(betas))
    for it in range(max_iter):
        new, _ = one_iteration(ell, betas, g)
        new = new - new[0]
        change = float(np.abs(new - g).max())
        g = new
        if change <= tol:
            return g, it + 1
    raise RuntimeError("mbar_ref.solve: no convergence")


def ln_z(ell, betas, g, targets):
    """ln Z(beta_t) - ln Z(beta_0) for the free energies g, both from the same weights"""
    lnD = ln_d(ell, betas, g)
    G = [sums(ell, lnD, bt)["G"] for bt in np.asarray(targets, dtype=np.float64).tolist()]
    return np.array(G) - sums(ell, lnD, float(betas[0]))["G"]


# ---- the bounds of the comparisons with the device (derived in tests/test_gpu_mbar.py) --------------------------------
def bounds(K, tiles, lnD, x_abs_max):
    """(E_x, R0): the absolute bound on x_tn and m_t, and the relative bound on S0, between two evaluations that follow
    the stated operations with exp and log good to one ulp each"""
    u = 2.0 ** -53
    E_D = 4 * u * (1 + math.log(max(K, 2))) + (K + 1) * u + 2 * u * float(np.abs(lnD).max())
    E_x = E_D + 2 * u * x_abs_max
    R0 = 2 * E_x + 745 * 2 * u + 4 * u + (70 + tiles) * u
    return E_x, R0


def tol_G(K, ell, lnD, targets, G):
    """the bound on |G_t| between two such evaluations: E_x + R0 + 2^-51 ln N + 2^-52 max|G|"""
    N = ell.size
    l = ell.reshape(-1)
    x_abs = max(float(np.abs(bt * l - lnD).max()) for bt in np.asarray(targets, dtype=np.float64).tolist())
    E_x, R0 = bounds(K, (N + 4095) // 4096, lnD, x_abs)
    return E_x + R0 + 2.0 ** -51 * math.log(max(N, 2)) + 2.0 ** -52 * float(np.abs(G).max())
