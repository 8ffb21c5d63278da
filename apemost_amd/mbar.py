"""MBAR (multistate Bennett acceptance ratio, Shirts & Chodera 2008) over a tempered ladder: the free energies
ln Z(beta_k) from the loglike of every kept step of every chain, and from the same weights ln Z, E[loglike],
Var[loglike] and the effective sample size at any beta, sampled or not, and the evidence ln Z(1) - ln Z(0).

An Mbar holds what apemost_hip_mbar_get hands out (include/apemost_hip.h, apemost_hip_mbar_view): ell[n][n_chains], the
loglike l = v / beta_c of column n_par+1 of the kept rows (chains ladder-major), and per ladder the count of stored
values that are not finite.  With g_k the running estimate of ln Z(beta_k), K chains per ladder and T kept steps in the
range [t0, t0 + t_count), sample n = (kept step, chain) in stored order:

    lnD_n = ln sum_j exp(beta_j l_n + c_j),   c_j = ln T - g_j          (row pass)
    G_t   = ln sum_n exp(beta_t l_n - lnD_n)                            (column pass, any target beta_t)
    g <- G(g) at the sampled betas                                      (one self-consistent iteration)

G(g + a) = G(g) + a, so the passes never normalise: solve() subtracts g_0 of every ladder and stops when no g_k - g_0
moves by more than tol.  Begun by HipSampler.mbar_begin the passes run on the device (csrc/pt_mbar.h); from_rows and
solve_numpy are the same estimator on the host in the kernels' stated order, operation for operation (numpy's exp and
log in place of the device library's): x_j = beta_j * l + c_j as one rounded multiply and one rounded add, the maximum
over j ascending, S = sum_j exp(x_j - m) sequentially, lnD = m + log(S); per target x_n = beta_t * l_n - lnD_n, the exact
maximum m_t, e = exp(x_n - m_t), d = l_n - l_first, and the sums S0 = sum e, S1 = sum e d, S2 = sum (e d) d, SS = sum e e
in tiles of 4096 samples counted from the range's first: lane i of 64 adds the terms of samples i, i + 64, ... in that
order, the 64 partials go through the adjacent-pairs tree, the tile partials are added in tile order.

Rows written after an accepted swap carry the pre-swap value of the column until the chain's next accept, as they do
for the evidence fold: ell is v / beta of the chain the row is stored under.

mbar.bin (little-endian), version 1; the C host's APEMOST_DUMP token `mbar` writes the same bytes:
    char[8]  "APEMOSTM"
    uint32   version, n_chains, n_ladders, solved (0 or 1)
    uint64   n, thin, t0, t_count                                 (the range of the solve; 0, 0 where not solved)
    double   betas[n_chains]
    uint64   n_bad[n_ladders]
    double   g[n_chains]                                          (g_k - g_0 of every ladder; 0 where not solved)
    double   ell[n][n_chains]
"""
import ctypes as C
import math
import struct
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import capi

MAGIC = b"APEMOSTM"
VERSION = 1
_HEAD = struct.Struct("<8s4I4Q")
TILE, LANES = 4096, 64
WORDS = ("m", "S0", "S1", "S2", "SS", "G")


def check_betas(betas, n_ladders=1):
    """ladder-major betas as Evidence.coefficients wants them: finite, positive, strictly decreasing in every ladder"""
    betas = np.ascontiguousarray(betas, dtype=np.float64)
    if betas.ndim != 1 or n_ladders < 1 or len(betas) == 0 or len(betas) % n_ladders:
        raise ValueError("betas must hold n_ladders equal ladders")
    per = len(betas) // n_ladders
    for b in range(n_ladders):
        lad = betas[b * per:(b + 1) * per]
        if not (np.isfinite(lad).all() and (lad > 0).all() and (np.diff(lad) < 0).all()):
            raise ValueError("ladder %d: betas must be finite, positive and strictly decreasing" % b)
    return betas


# ---- the passes on the host, one ladder, in the kernels' order ------------------------------------------------------
def row_pass(ell, betas, c):
    """lnD of the samples ell [N] (stored order) for the ladder's betas and c = ln T - g"""
    m = betas[0] * ell + c[0]
    for j in range(1, len(betas)):
        m = np.maximum(m, betas[j] * ell + c[j])
    S = np.zeros_like(ell)
    for j in range(len(betas)):
        S = S + np.exp((betas[j] * ell + c[j]) - m)
    return m + np.log(S)


def tile_sum(terms):
    """the sum of terms [N] in the fixed order: lane partials, the adjacent-pairs tree, tiles in order"""
    n = len(terms)
    tiles = (n + TILE - 1) // TILE
    a = np.zeros(tiles * TILE)
    a[:n] = terms
    a = a.reshape(tiles, TILE // LANES, LANES)               # [tile][r][lane]: sample r * 64 + lane of the tile
    p = np.zeros((tiles, LANES))
    for r in range(TILE // LANES):
        p = p + a[:, r, :]
    while p.shape[1] > 1:
        p = p[:, 0::2] + p[:, 1::2]
    total = 0.0
    for x in p[:, 0].tolist():
        total += x
    return total


def col_pass(ell, lnD, beta_t, full):
    """(m, S0[, S1, S2, SS, G]) of one target over the samples ell [N] with their lnD"""
    x = beta_t * ell - lnD
    m = float(x.max())
    e = np.exp(x - m)
    if not full:
        return m, tile_sum(e)
    d = ell - ell[0]
    ed = e * d
    S0 = tile_sum(e)
    return m, S0, tile_sum(ed), tile_sum(ed * d), tile_sum(e * e), m + math.log(S0)


class Mbar:
    def __init__(self, ell, betas, n_ladders=1, n_bad=None, thin=1, sampler=None, threads=1):
        self.n_ladders, self.thin, self.threads = int(n_ladders), int(thin), int(threads)
        self.betas = check_betas(betas, self.n_ladders)
        nc = len(self.betas)
        self.ell = np.ascontiguousarray(ell, dtype=np.float64).reshape(-1, nc)
        self.n_bad = (np.zeros(self.n_ladders, dtype=np.uint64) if n_bad is None
                      else np.ascontiguousarray(n_bad, dtype=np.uint64).reshape(self.n_ladders))
        self._sampler = sampler      # the HipSampler whose open fold holds this store, or None: the passes run in numpy
        self.g = None                # [n_chains]: g_k - g_0 of every ladder once solved
        self.range = (0, 0)          # (t0, t_count) of the solve
        self.iterations, self.change = 0, math.inf

    @property
    def n(self):
        return len(self.ell)

    @property
    def n_chains(self):
        return len(self.betas)

    @property
    def per(self):
        return self.n_chains // self.n_ladders

    @classmethod
    def from_rows(cls, rows, betas, n_ladders=1, thin=1, threads=1):
        """the store of host sample rows [n][n_chains][n_par+2] (already thinned) or of the column itself
        [n][n_chains]: what the device stores, for tests and for existing dumps"""
        rows = np.asarray(rows, dtype=np.float64)
        col = rows[:, :, -1] if rows.ndim == 3 else rows
        betas = check_betas(betas, n_ladders)
        with np.errstate(all="ignore"):
            ell = col / betas
        bad = (~np.isfinite(ell)).reshape(len(ell), n_ladders, -1).sum(axis=(0, 2))
        return cls(ell, betas, n_ladders, bad, thin, None, threads)

    def view(self):
        """the apemost_hip_mbar_view over this object's arrays"""
        self._n = np.array([self.n], dtype=np.uint64)
        return capi.MbarView(n=self._n.ctypes.data_as(capi._up), n_bad=self.n_bad.ctypes.data_as(capi._up),
                             ell=self.ell.ctypes.data_as(capi._dp))

    # -- the passes: on the device where the store is there, else in numpy ---------------------------------------------
    def _check_range(self, t0, t_count):
        t_count = self.n - t0 if t_count is None else t_count
        if t_count < 1 or t0 < 0 or t0 + t_count > self.n:
            raise ValueError("kept steps [%d, %d + %d) are empty or go past the %d stored" % (t0, t0, t_count, self.n))
        for b in range(self.n_ladders):
            if self.n_bad[b]:
                raise ValueError("ladder %d stores %d values that are not finite" % (b, int(self.n_bad[b])))
        return int(t0), int(t_count)

    def _ladder(self, b, t0, t_count):
        """(samples [N] in stored order, betas [K]) of ladder b over the range"""
        k = slice(b * self.per, (b + 1) * self.per)
        return np.ascontiguousarray(self.ell[t0:t0 + t_count, k]).reshape(-1), self.betas[k]

    def _map(self, f, items):
        if self.threads > 1 and len(items) > 1:
            with ThreadPoolExecutor(self.threads) as pool:
                return list(pool.map(f, items))
        return [f(x) for x in items]

    def _row_pass(self, ell, betas, c):
        cuts = np.linspace(0, len(ell), max(1, min(self.threads, len(ell) // 16384)) + 1).astype(int)
        return np.concatenate(self._map(lambda i: row_pass(ell[cuts[i]:cuts[i + 1]], betas, c), list(range(len(cuts) - 1))))

    def iterate(self, g, n_iter=1, t0=0, t_count=None):
        """(g after n_iter updates, g before the last of them) over the kept steps [t0, t0 + t_count); g [n_chains]"""
        t0, t_count = self._check_range(t0, t_count)
        g = np.ascontiguousarray(g, dtype=np.float64).copy()
        assert g.shape == (self.n_chains,) and n_iter >= 1
        prev = np.zeros_like(g)
        if self._sampler is not None:
            s = self._sampler
            capi.check(s.L.apemost_hip_mbar_iterate(s._h, t0, t_count, n_iter, g.ctypes.data_as(capi._dp),
                                                    prev.ctypes.data_as(capi._dp)))
            return g, prev
        lnT = math.log(float(t_count))
        for b in range(self.n_ladders):
            k = slice(b * self.per, (b + 1) * self.per)
            ell, betas = self._ladder(b, t0, t_count)
            gb = g[k].copy()
            for _ in range(n_iter):
                prev[k] = gb
                lnD = self._row_pass(ell, betas, lnT - gb)
                gb = np.array([m + math.log(S0) for m, S0 in self._map(lambda bt: col_pass(ell, lnD, bt, False), betas.tolist())])
            g[k] = gb
        return g, prev

    def evaluate(self, betas_t, g=None, t0=None, t_count=None):
        """{m, S0, S1, S2, SS, G = m + log(S0): [n_ladders][n_t], ell_first: [n_ladders]} of the targets betas_t (finite, >= 0) for the
        free energies g (default: the solve's, over its range)"""
        g, t0, t_count = self._solved(g, t0, t_count)
        bt = np.ascontiguousarray(betas_t, dtype=np.float64).reshape(-1)
        if len(bt) < 1 or not (np.isfinite(bt).all() and (bt >= 0).all()):
            raise ValueError("a target is finite and >= 0")
        L, nt = self.n_ladders, len(bt)
        out = {w: np.zeros((L, nt)) for w in WORDS}
        out["ell_first"] = np.zeros(L)
        if self._sampler is not None:
            s, dp = self._sampler, capi._dp
            sums = capi.MbarSums(ell_first=out["ell_first"].ctypes.data_as(dp), **{w: out[w].ctypes.data_as(dp) for w in WORDS})
            capi.check(s.L.apemost_hip_mbar_evaluate(s._h, t0, t_count, g.ctypes.data_as(dp), bt.ctypes.data_as(dp), nt,
                                                     C.byref(sums)))
            return out
        lnT = math.log(float(t_count))
        for b in range(L):
            ell, betas = self._ladder(b, t0, t_count)
            lnD = self._row_pass(ell, betas, lnT - g[b * self.per:(b + 1) * self.per])
            for t, words in enumerate(self._map(lambda x: col_pass(ell, lnD, x, True), bt.tolist())):
                for w, v in zip(WORDS, words):
                    out[w][b, t] = v
            out["ell_first"][b] = ell[0]
        return out

    def log_weights(self, beta, g=None, t0=None, t_count=None):
        """[t_count][n_chains]: beta l_n - lnD_n - G(beta), the log of the weight, normalised per ladder, with which
        sample (kept step, chain) of the range enters an expectation at `beta`: reweight with them whatever was kept of
        those rows"""
        g, t0, t_count = self._solved(g, t0, t_count)
        beta = float(beta)
        if not (math.isfinite(beta) and beta >= 0):
            raise ValueError("a target is finite and >= 0")
        out = np.zeros((t_count, self.n_chains))
        if self._sampler is not None:
            s, dp = self._sampler, capi._dp
            capi.check(s.L.apemost_hip_mbar_log_weights(s._h, t0, t_count, g.ctypes.data_as(dp), beta, out.ctypes.data_as(dp)))
            return out
        lnT = math.log(float(t_count))
        for b in range(self.n_ladders):
            k = slice(b * self.per, (b + 1) * self.per)
            ell, betas = self._ladder(b, t0, t_count)
            lnD = self._row_pass(ell, betas, lnT - g[k])
            m, S0 = col_pass(ell, lnD, beta, False)
            out[:, k] = ((beta * ell - lnD) - (m + math.log(S0))).reshape(t_count, self.per)
        return out

    # -- the solve -----------------------------------------------------------------------------------------------------
    def _relative(self, g):
        return (g.reshape(self.n_ladders, self.per) - g.reshape(self.n_ladders, self.per)[:, :1]).reshape(-1)

    def start(self, t0=0, t_count=None):
        """where solve() starts: the trapezoid rule over the per-chain means of l, from the hottest chain up, less g_0"""
        t0, t_count = self._check_range(t0, t_count)
        mean = self.ell[t0:t0 + t_count].mean(axis=0).reshape(self.n_ladders, self.per)
        b = self.betas.reshape(self.n_ladders, self.per)
        g = np.zeros_like(mean)
        for k in range(self.per - 2, -1, -1):
            g[:, k] = g[:, k + 1] + (b[:, k] - b[:, k + 1]) * (mean[:, k] + mean[:, k + 1]) / 2
        return self._relative(g.reshape(-1))

    def solve(self, tol=1e-10, max_iter=10000, check_every=10, t0=0, t_count=None, g=None):
        """iterates g <- G(g) over the kept steps [t0, t0 + t_count) (default: all), check_every updates between two
        looks, until max_k |change of (g_k - g_0)| <= tol.  Returns (iterations used, the last change) and raises
        RuntimeError if max_iter updates did not get there."""
        t0, t_count = self._check_range(t0, t_count)
        g = self.start(t0, t_count) if g is None else self._relative(np.asarray(g, dtype=np.float64))
        used, change = 0, math.inf
        while used < max_iter:
            k = min(int(check_every), max_iter - used)
            g, prev = self.iterate(g, k, t0, t_count)
            used += k
            g, prev = self._relative(g), self._relative(prev)
            change = float(np.abs(g - prev).max())
            if change <= tol:
                break
        self.g, self.range, self.iterations, self.change = g, (t0, t_count), used, change
        if not change <= tol:
            raise RuntimeError("mbar: %d iterations left a change of %g, above tol = %g" % (used, change, tol))
        return used, change

    def solve_numpy(self, **kw):
        """solve() with the passes in numpy, whatever holds the store; the estimators then evaluate in numpy too"""
        self._sampler = None
        return self.solve(**kw)

    def _solved(self, g, t0, t_count):
        if g is None:
            if self.g is None:
                raise ValueError("no free energies: solve() first, or give g")
            g = self.g
        if t0 is None:
            t0, t_count = self.range if self.g is not None else (0, None)
        t0, t_count = self._check_range(t0, t_count)
        return np.ascontiguousarray(g, dtype=np.float64), t0, t_count

    # -- estimators ------------------------------------------------------------------------------------------------------
    def _shape(self, a):
        return a[0] if self.n_ladders == 1 else a

    def free_energy(self):
        """ln Z(beta_k) - ln Z(beta_0) of every chain: the solve's fixed point"""
        if self.g is None:
            raise ValueError("no free energies: solve() first")
        return self.g.copy()

    def ln_z(self, betas):
        """ln Z(beta) - ln Z(beta_0) at the given betas: [n_t], or [n_ladders][n_t] for a batch"""
        bt = np.asarray(betas, dtype=np.float64).reshape(-1)
        cold = self.betas[::self.per]                        # beta_0 of every ladder: a target like any other, so that
        first = np.unique(cold)                              # ln_z(beta_0) is 0 however far the solve went
        G = self.evaluate(np.concatenate([bt, first]))["G"]
        at = len(bt) + np.searchsorted(first, cold)
        return self._shape(G[:, :len(bt)] - G[np.arange(self.n_ladders), at][:, None])

    def ln_evidence(self):
        """ln p(D|M,I) = ln_z(1) - ln_z(0).  beta = 0 is not sampled: ln Z(0) is an extrapolation from the hottest rung,
        as good as that rung's samples cover the prior (ess(0) says how many of them count)."""
        z = self.ln_z([1.0, 0.0])
        return float(z[0] - z[1]) if self.n_ladders == 1 else z[:, 0] - z[:, 1]

    def mean_loglike(self, betas):
        """E_beta[loglike] = l_first + S1 / S0"""
        e = self.evaluate(betas)
        return self._shape(e["ell_first"][:, None] + e["S1"] / e["S0"])

    def var_loglike(self, betas):
        """Var_beta[loglike] = S2 / S0 - (S1 / S0)^2, the moments about the range's first sample"""
        e = self.evaluate(betas)
        r = e["S1"] / e["S0"]
        return self._shape(e["S2"] / e["S0"] - r * r)

    def ess(self, betas):
        """Kish's effective sample size S0^2 / SS of the whole ladder's samples at beta"""
        e = self.evaluate(betas)
        return self._shape(e["S0"] * e["S0"] / e["SS"])

    def error(self, blocks=10, what="ln_evidence", betas=None):
        """the standard error of the mean of `what` ("ln_evidence", or "ln_z", "mean_loglike", "var_loglike" at
        `betas`) over `blocks` contiguous time blocks of the solve's range, each solved on its own from this solve's
        free energies: the spread of the block estimates over sqrt(blocks)"""
        if self.g is None:
            raise ValueError("no free energies: solve() first")
        t0, t_count = self.range
        if blocks < 2 or blocks > t_count:
            raise ValueError("blocks: 2 .. %d" % t_count)
        est = []
        for i in range(blocks):
            lo, hi = t0 + i * t_count // blocks, t0 + (i + 1) * t_count // blocks
            part = Mbar(self.ell, self.betas, self.n_ladders, self.n_bad, self.thin, self._sampler, self.threads)
            part.solve(t0=lo, t_count=hi - lo, g=self.g)
            est.append(part.ln_evidence() if what == "ln_evidence" else getattr(part, what)(betas))
        return np.std(np.array(est), axis=0, ddof=1) / math.sqrt(blocks)

    # -- ladders, text, mbar.bin -----------------------------------------------------------------------------------------
    def per_ladder(self):
        """one Mbar per ladder of a batch (chains ladder-major), on the host"""
        out = []
        for b in range(self.n_ladders):
            k = slice(b * self.per, (b + 1) * self.per)
            one = Mbar(self.ell[:, k], self.betas[k], 1, self.n_bad[b:b + 1], self.thin, None, self.threads)
            if self.g is not None:
                one.g, one.range, one.iterations, one.change = self.g[k].copy(), self.range, self.iterations, self.change
            out.append(one)
        return out

    def text(self, blocks=10):
        """mbar.txt of one ladder: per rung `beta ln_z mean_loglike var_loglike ess`, "%.15e", tab separated, then
        `ln_evidence value error` with the block error"""
        if self.n_ladders != 1:
            raise ValueError("a batch of %d ladders: take per_ladder() first" % self.n_ladders)
        cols = (self.betas, self.ln_z(self.betas), self.mean_loglike(self.betas), self.var_loglike(self.betas),
                self.ess(self.betas))
        out = ["\t".join(_fmt(float(col[c])) for col in cols) + "\n" for c in range(self.n_chains)]
        out.append("ln_evidence\t%s\t%s\n" % (_fmt(self.ln_evidence()), _fmt(float(self.error(blocks)))))
        return "".join(out)

    def write(self, path):
        solved = self.g is not None
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_chains, self.n_ladders, int(solved), self.n, self.thin,
                               *(self.range if solved else (0, 0))))
            f.write(np.ascontiguousarray(self.betas, dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(self.n_bad, dtype="<u8").tobytes())
            f.write(np.ascontiguousarray(self.g if solved else np.zeros(self.n_chains), dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(self.ell, dtype="<f8").tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not an mbar file" % path)
        magic, version, nc, n_ladders, solved, n, thin, t0, t_count = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not an mbar file of version %d" % (path, VERSION))
        want = _HEAD.size + 8 * (2 * nc + n_ladders + n * nc)
        if want != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), want))
        off = _HEAD.size
        betas = np.frombuffer(raw, dtype="<f8", count=nc, offset=off).copy()
        bad = np.frombuffer(raw, dtype="<u8", count=n_ladders, offset=off + 8 * nc).copy()
        g = np.frombuffer(raw, dtype="<f8", count=nc, offset=off + 8 * (nc + n_ladders)).copy()
        ell = np.frombuffer(raw, dtype="<f8", count=n * nc, offset=off + 8 * (2 * nc + n_ladders)).copy()
        mb = cls(ell.reshape(n, nc), betas, n_ladders, bad, thin)
        if solved:
            mb.g, mb.range = g, (t0, t_count)
        return mb


def _fmt(v):
    return "nan" if v != v else "%.15e" % v
