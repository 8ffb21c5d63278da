"""Reweighted posteriors: the moments and the marginal histograms of chosen columns of the sample row at any
beta_t >= 0, sampled or not, estimated from every kept step of every chain of a tempered ladder with the MBAR weights
(apemost_amd/mbar.py), not from chain 0 alone.

A Reweight holds what apemost_hip_reweight_get hands out (include/apemost_hip.h, apemost_hip_reweight_view):
x[n_cols][n][n_chains], the columns `cols` of the kept rows, and per (ladder, column) the count of stored values that
are not finite.  It belongs to an Mbar over the same rows, which has the loglike and, once solved, the free energies g.
Per ladder over the kept steps [t0, t0 + t_count), N = t_count * K samples in stored order (step-major, the chain
fastest), for a target beta_t:

    lnD_n, x_tn = beta_t l_n - lnD_n, the exact maximum m_t, e_n = exp(x_tn - m_t)        (mbar.py, unchanged)
    origin_a = x_a of the range's first sample of the ladder,  d_a = x_a,n - origin_a
    S0 = sum e,  SS = sum e e,  S1[a] = sum e d_a,  cross[a][b] = sum (e d_a) d_b,  a <= b
    q_n = (uint64) rint(ldexp(e_n, s)),  s = 63 - bit_length(N)
    hist[a][bin] = sum of q_n over the samples whose x_a falls in the bin,  q_total = sum q_n

Every product is rounded once, every floating-point sum is mbar.tile_sum (tiles of 4096 samples from the range's first,
64 lane partials, the adjacent-pairs tree, tiles in order); the bins are the run summary's (summary.edges, the
bisection of gsl_histogram_increment; values outside [lo, hi + (hi - lo) / 10000), NaN included, are not counted).  The
scaling by 2^s is exact and rint is the one rounding of q; e <= 1 gives sum q < 2^63; the integer sums do not depend on
the order.  A bin differs from 2^s sum e by at most N_bin / 2; relative to the normalisation S0 >= ESS the error is at
most N 2^-(s+1) / ESS.

    E[x_a] = origin_a + S1[a] / S0,   Cov[x_a, x_b] = cross[a][b] / S0 - (S1[a] / S0)(S1[b] / S0),   ESS = S0^2 / SS

Begun by HipSampler.reweight_begin the sums run on the device (csrc/pt_reweight.h); from_rows and evaluate_numpy are
the same estimator on the host in the same order, operation for operation (numpy's exp in place of the device
library's).

Rows written after an accepted swap carry the pre-swap prob - prior until the chain's next accept (DESIGN.md, quirk
Q1): in those rows l is not the loglike of the row's parameters, so the weight and the value it weights do not belong
together.  The estimate inherits that from the reference's schedule; DESIGN.md section 11 names the share of such rows.

reweight.bin (little-endian), version 1; it holds the sums, not the store:
    char[8]  "APEMOSTW"
    uint32   version, n_chains, n_ladders, n_cols, n_t, nbins
    int32    shift
    uint32   0
    uint64   n, thin, t0, t_count                                 (n: kept steps stored; the range of the evaluation)
    int32    cols[16]                                             (the first n_cols; the rest 0)
    double   lo[n_cols], hi[n_cols]                               (0 where nbins = 0)
    double   betas_t[n_t]
    double   m[n_ladders][n_t], S0[n_ladders][n_t], SS[n_ladders][n_t]
    double   origin[n_ladders][n_cols]
    double   S1[n_ladders][n_t][n_cols]
    double   cross[n_ladders][n_t][n_cols (n_cols + 1) / 2]       (the upper triangle, row-major)
    uint64   hist[n_ladders][n_t][n_cols][nbins]
    uint64   q_total[n_ladders][n_t]

Resampling (Reweight.resample, csrc/pt_resample.h): M equally weighted draws per ladder from the weighted sample of one
target, for whatever the sums do not answer.  In integers alone, with sample n in stored order and the caller's uint64 u:

    C_n = q_0 + ... + q_n,  Q = C_{N-1} = q_total;   a = Q div M,  b = Q mod M,  o = (u a) >> 64
    p_m = m a + (m b) div M + o,  m = 0 .. M-1;   draw m is the smallest n with C_n > p_m

systematic resampling with an integer offset: p is non-decreasing and below Q, a sample with q_n = 0 is never drawn and
sample n is drawn floor(M q_n / Q) or ceil(M q_n / Q) times.  The draws come out in stored order (time-major): equally
weighted, not exchangeable in order.  resample_numpy is the same rule on the host (np.cumsum in uint64, exact below
2^63, and np.searchsorted): the same indices whenever the q agree.

resample.bin (little-endian), version 1; one record per target:
    char[8]  "APEMOSTS"
    uint32   version, n_chains, n_ladders, n_cols, n_t, n_draws
    int32    shift
    uint32   0
    uint64   n, thin, t0, t_count, u
    int32    cols[16]                                             (the first n_cols; the rest 0)
    n_t times:
        double   beta_t
        uint64   q_total[n_ladders]
        uint32   index[n_ladders][n_draws]
        double   x[n_ladders][n_draws][n_cols]
"""
import ctypes as C
import math
import struct

import numpy as np

from . import capi
from .joint import bins_of, tri_index
from .mbar import tile_sum
from .summary import edges as summary_edges

MAGIC = b"APEMOSTW"
VERSION = 1
_HEAD = struct.Struct("<8s6IiI4Q16i")
MAX_COLS, MAX_BINS, MAX_TARGETS = 16, 4096, 64
RESAMPLE_MAGIC = b"APEMOSTS"
RESAMPLE_VERSION = 1
_RESAMPLE_HEAD = struct.Struct("<8s6IiI5Q16i")
MAX_DRAWS, MAX_DRAW_VALUES = 1 << 24, 1 << 26


def shift_of(N):
    """s = 63 - bit_length(N): the fixed point of the weights of N samples"""
    return 63 - int(N).bit_length()


def fixed_point(e, s):
    """q = (uint64) rint(ldexp(e, s))"""
    return np.rint(np.ldexp(e, s)).astype(np.uint64)


def systematic_positions(Q, M, u):
    """p_m = m a + (m b) div M + o, m = 0 .. M-1, with a = Q div M, b = Q mod M, o = (u a) >> 64: uint64 [M],
    non-decreasing and below Q.  a, b and o are Python integers (u a has 128 bits); every term of p_m is below 2^63, so
    the uint64 arithmetic over m is exact."""
    Q, M, u = int(Q), int(M), int(u)
    if not 1 <= M <= MAX_DRAWS:
        raise ValueError("n_draws %d outside [1,2^24]" % M)
    if not 0 <= u < 1 << 64:
        raise ValueError("u is a uint64")
    if not M <= Q < 1 << 63:
        raise ValueError("Q = %d outside [n_draws, 2^63)" % Q)
    a, b = divmod(Q, M)
    o = (u * a) >> 64
    m = np.arange(M, dtype=np.uint64)
    return m * np.uint64(a) + (m * np.uint64(b)) // np.uint64(M) + np.uint64(o)


def check_cols(cols, n_par):
    cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
    if not 1 <= len(cols) <= MAX_COLS:
        raise ValueError("n_cols %d outside [1,%d]" % (len(cols), MAX_COLS))
    if cols[0] < 0 or (n_par is not None and cols[-1] > n_par + 1) or np.any(np.diff(cols) <= 0):
        raise ValueError("columns in [0, n_par + 1], strictly increasing")
    return cols


class Reweight:
    def __init__(self, x, cols, lo=None, hi=None, nbins=0, n_ladders=1, n_bad=None, thin=1, sampler=None, mbar=None):
        self.cols = check_cols(cols, None)
        k = len(self.cols)
        x = np.ascontiguousarray(x, dtype=np.float64)
        self.x = x.reshape(k, -1, x.shape[-1])
        self.n_ladders, self.thin, self.nbins = int(n_ladders), int(thin), int(nbins)
        if not 0 <= self.nbins <= MAX_BINS:
            raise ValueError("nbins %d outside [0,%d]" % (self.nbins, MAX_BINS))
        self.lo = np.zeros(k) if lo is None else np.ascontiguousarray(lo, dtype=np.float64).reshape(k)
        self.hi = np.zeros(k) if hi is None else np.ascontiguousarray(hi, dtype=np.float64).reshape(k)
        if self.nbins and not (np.isfinite(self.lo).all() and np.isfinite(self.hi).all() and (self.lo < self.hi).all()):
            raise ValueError("the histogram ranges must be finite with lo < hi")
        self.n_bad = (np.zeros((self.n_ladders, k), dtype=np.uint64) if n_bad is None
                      else np.ascontiguousarray(n_bad, dtype=np.uint64).reshape(self.n_ladders, k))
        self._sampler = sampler      # the HipSampler whose open fold holds this store, or None: the sums run in numpy
        self.mbar = mbar             # the Mbar over the same rows, where the maker knew it

    @property
    def n(self):
        return self.x.shape[1]

    @property
    def n_chains(self):
        return self.x.shape[2]

    @property
    def n_cols(self):
        return len(self.cols)

    @classmethod
    def from_rows(cls, rows, betas, cols=None, lo=None, hi=None, nbins=0, n_ladders=1, thin=1, threads=1):
        """the store, and the Mbar beside it (.mbar), of host sample rows [n][n_chains][n_par+2] (already thinned):
        what the device stores.  cols None: the parameters."""
        from .mbar import Mbar
        rows = np.asarray(rows, dtype=np.float64)
        n_par = rows.shape[2] - 2
        cols = check_cols(np.arange(n_par) if cols is None else cols, n_par)
        x = np.ascontiguousarray(np.moveaxis(rows[:, :, cols], 2, 0))
        bad = (~np.isfinite(x)).reshape(len(cols), len(rows), n_ladders, -1).sum(axis=(1, 3)).T
        return cls(x, cols, lo, hi, nbins, n_ladders, bad, thin, None, Mbar.from_rows(rows, betas, n_ladders, thin, threads))

    def view(self):
        """the apemost_hip_reweight_view over this object's arrays"""
        self._n = np.array([self.n], dtype=np.uint64)
        return capi.ReweightView(n=self._n.ctypes.data_as(capi._up), n_bad=self.n_bad.ctypes.data_as(capi._up),
                                 x=self.x.ctypes.data_as(capi._dp))

    def _args(self, mbar, g, t0, t_count):
        mbar = self.mbar if mbar is None else mbar
        if mbar is None:
            raise ValueError("no Mbar: give the one over the same rows")
        if mbar.n != self.n or mbar.n_chains != self.n_chains or mbar.n_ladders != self.n_ladders:
            raise ValueError("stores out of step: mbar holds %d kept steps of %d chains, reweight %d of %d"
                             % (mbar.n, mbar.n_chains, self.n, self.n_chains))
        g, t0, t_count = mbar._solved(g, t0, t_count)
        for b in range(self.n_ladders):
            for k in range(self.n_cols):
                if self.n_bad[b, k]:
                    raise ValueError("ladder %d stores %d values of column %d that are not finite"
                                     % (b, int(self.n_bad[b, k]), int(self.cols[k])))
        return mbar, g, t0, t_count

    @staticmethod
    def _targets(betas_t):
        bt = np.ascontiguousarray(betas_t, dtype=np.float64).reshape(-1)
        if not 1 <= len(bt) <= MAX_TARGETS or not (np.isfinite(bt).all() and (bt >= 0).all()):
            raise ValueError("1 .. %d targets, each finite and >= 0" % MAX_TARGETS)
        return bt

    def _result(self, mbar, g, bt, t0, t_count):
        L, nt, k = self.n_ladders, len(bt), self.n_cols
        r = Reweighted(self.cols, bt, self.lo, self.hi, self.nbins, L, self.n_chains, self.n, self.thin, (t0, t_count))
        r.shift = shift_of(t_count * (self.n_chains // L))
        r._source = (self, mbar, g)
        return r, L, nt, k

    def evaluate(self, mbar=None, betas_t=(1.0,), g=None, t0=None, t_count=None):
        """the Reweighted of the targets betas_t (1 .. 64, finite, >= 0) under the Mbar's free energies (default: its
        solve's, over its range): on the device where the store is there, else in numpy"""
        if self._sampler is None:
            return self.evaluate_numpy(mbar, betas_t, g, t0, t_count)
        mbar, g, t0, t_count = self._args(mbar, g, t0, t_count)
        bt = self._targets(betas_t)
        r, L, nt, k = self._result(mbar, g, bt, t0, t_count)
        s, dp, up = self._sampler, capi._dp, capi._up
        shift = np.zeros(1, dtype=np.int32)
        sums = capi.ReweightSums(m=r.m.ctypes.data_as(dp), S0=r.S0.ctypes.data_as(dp), SS=r.SS.ctypes.data_as(dp),
                                 origin=r.origin.ctypes.data_as(dp), S1=r.S1.ctypes.data_as(dp),
                                 cross=r.cross.ctypes.data_as(dp), shift=shift.ctypes.data_as(C.POINTER(C.c_int32)),
                                 hist=r.hist.ctypes.data_as(up), q_total=r.q_total.ctypes.data_as(up))
        capi.check(s.L.apemost_hip_reweight_evaluate(s._h, t0, t_count, g.ctypes.data_as(dp), bt.ctypes.data_as(dp), nt,
                                                     C.byref(sums)))
        assert int(shift[0]) == r.shift
        return r

    def _ladder_e(self, mbar, g, b, t0, t_count, bt):
        """(m, e [N]) of ladder b's range for every target of bt, lazily: lnD is formed once"""
        per = mbar.per
        ell, betas = mbar._ladder(b, t0, t_count)
        lnD = mbar._row_pass(ell, betas, math.log(float(t_count)) - g[b * per:(b + 1) * per])
        for beta in bt.tolist():
            x = beta * ell - lnD
            m = float(x.max())
            yield m, np.exp(x - m)

    def evaluate_numpy(self, mbar=None, betas_t=(1.0,), g=None, t0=None, t_count=None):
        """evaluate() on the host, in the kernels' order"""
        mbar, g, t0, t_count = self._args(mbar, g, t0, t_count)
        bt = self._targets(betas_t)
        r, L, nt, k = self._result(mbar, g, bt, t0, t_count)
        per = self.n_chains // L
        for b in range(L):
            cols = [np.ascontiguousarray(self.x[a, t0:t0 + t_count, b * per:(b + 1) * per]).reshape(-1) for a in range(k)]
            r.origin[b] = [c[0] for c in cols]
            d = [c - c[0] for c in cols]
            bins = [bins_of(c, summary_edges(float(self.lo[a]), float(self.hi[a]), self.nbins)) for a, c in enumerate(cols)] \
                if self.nbins else []
            for t, (m, e) in enumerate(self._ladder_e(mbar, g, b, t0, t_count, bt)):
                r.m[b, t], r.S0[b, t], r.SS[b, t] = m, tile_sum(e), tile_sum(e * e)
                for a in range(k):
                    ed = e * d[a]
                    r.S1[b, t, a] = tile_sum(ed)
                    for c in range(a, k):
                        r.cross[b, t, tri_index(k, a, c)] = tile_sum(ed * d[c])
                q = fixed_point(e, r.shift)
                r.q_total[b, t] = q.sum(dtype=np.uint64)
                for a in range(k if self.nbins else 0):
                    r.hist[b, t, a] = weighted_bincount(bins[a], q, self.nbins)
        return r

    def weights(self, mbar=None, beta=1.0, g=None, t0=None, t_count=None):
        """(e, q), [t_count][n_chains] each: the weights an evaluation at `beta` uses, unnormalised within every ladder
        (divide e by its ladder's sum): reweight with them whatever was kept of those rows"""
        mbar, g, t0, t_count = self._args(mbar, g, t0, t_count)
        bt = self._targets([beta])
        if self._sampler is None:
            return self._weights_numpy(mbar, g, t0, t_count, bt)
        e = np.zeros((t_count, self.n_chains))
        q = np.zeros((t_count, self.n_chains), dtype=np.uint64)
        s = self._sampler
        capi.check(s.L.apemost_hip_reweight_weights(s._h, t0, t_count, g.ctypes.data_as(capi._dp), float(bt[0]),
                                                    e.ctypes.data_as(capi._dp), q.ctypes.data_as(capi._up)))
        return e, q

    def _weights_numpy(self, mbar, g, t0, t_count, bt):
        e = np.zeros((t_count, self.n_chains))
        q = np.zeros((t_count, self.n_chains), dtype=np.uint64)
        per = self.n_chains // self.n_ladders
        s = shift_of(t_count * per)
        for b in range(self.n_ladders):
            for _, eb in self._ladder_e(mbar, g, b, t0, t_count, bt):
                e[:, b * per:(b + 1) * per] = eb.reshape(t_count, per)
                q[:, b * per:(b + 1) * per] = fixed_point(eb, s).reshape(t_count, per)
        return e, q

    # -- resampling ------------------------------------------------------------------------------------------------------
    def _draws(self, beta, n_draws, u, t0, t_count):
        n_draws, u = int(n_draws), int(u)
        if not 1 <= n_draws <= MAX_DRAWS:
            raise ValueError("n_draws %d outside [1,2^24]" % n_draws)
        if self.n_ladders * n_draws * self.n_cols > MAX_DRAW_VALUES:
            raise ValueError("%d ladders x %d draws x %d columns are more than 2^26 values"
                             % (self.n_ladders, n_draws, self.n_cols))
        if not 0 <= u < 1 << 64:
            raise ValueError("u is a uint64")
        r = Resampled(self.cols, beta, u, n_draws, self.n_ladders, self.n_chains, self.n, self.thin, (t0, t_count))
        r.shift = shift_of(t_count * (self.n_chains // self.n_ladders))
        return r

    def resample(self, mbar=None, beta=1.0, n_draws=4096, u=0, g=None, t0=None, t_count=None):
        """the Resampled of n_draws equally weighted draws per ladder at the target `beta` (finite, >= 0) with the
        offset word u (a uint64; a seed) under the Mbar's free energies: on the device where the store is there, else
        in numpy"""
        if self._sampler is None:
            return self.resample_numpy(mbar, beta, n_draws, u, g, t0, t_count)
        mbar, g, t0, t_count = self._args(mbar, g, t0, t_count)
        bt = self._targets([beta])
        r = self._draws(float(bt[0]), n_draws, u, t0, t_count)
        s = self._sampler
        shift = np.zeros(1, dtype=np.int32)
        out = capi.ReweightDraws(index=r.index.ctypes.data_as(C.POINTER(C.c_uint32)), x=r.x.ctypes.data_as(capi._dp),
                                 q_total=r.q_total.ctypes.data_as(capi._up),
                                 shift=shift.ctypes.data_as(C.POINTER(C.c_int32)))
        capi.check(s.L.apemost_hip_reweight_resample(s._h, t0, t_count, g.ctypes.data_as(capi._dp), float(bt[0]),
                                                     r.n_draws, r.u, C.byref(out)))
        assert int(shift[0]) == r.shift
        return r

    def resample_numpy(self, mbar=None, beta=1.0, n_draws=4096, u=0, g=None, t0=None, t_count=None):
        """resample() on the host: q of evaluate_numpy's path, a uint64 cumsum and searchsorted"""
        mbar, g, t0, t_count = self._args(mbar, g, t0, t_count)
        bt = self._targets([beta])
        r = self._draws(float(bt[0]), n_draws, u, t0, t_count)
        _, q = self._weights_numpy(mbar, g, t0, t_count, bt)
        per = self.n_chains // self.n_ladders
        for b in range(self.n_ladders):
            ladder = slice(b * per, (b + 1) * per)
            c = np.cumsum(np.ascontiguousarray(q[:, ladder]).reshape(-1), dtype=np.uint64)
            r.q_total[b] = c[-1]
            r.index[b] = np.searchsorted(c, systematic_positions(int(c[-1]), r.n_draws, r.u), side="right")
            for a in range(self.n_cols):
                r.x[b, :, a] = np.ascontiguousarray(self.x[a, t0:t0 + t_count, ladder]).reshape(-1)[r.index[b]]
        return r


def weighted_bincount(bins, q, nbins):
    """hist[b] = the sum of the integers q over the samples of bin b (bins < 0: not counted), exact in uint64"""
    out = np.zeros(nbins, dtype=np.uint64)
    keep = bins >= 0
    np.add.at(out, bins[keep], q[keep])
    return out


class Reweighted:
    """the sums of an evaluation; every estimator is [n_t]... for one ladder and [n_ladders][n_t]... for a batch"""

    def __init__(self, cols, betas_t, lo, hi, nbins, n_ladders, n_chains, n, thin, range_):
        self.cols = np.ascontiguousarray(cols, dtype=np.int32)
        self.betas_t = np.ascontiguousarray(betas_t, dtype=np.float64)
        self.lo, self.hi = np.ascontiguousarray(lo, dtype=np.float64), np.ascontiguousarray(hi, dtype=np.float64)
        self.nbins, self.n_ladders, self.n_chains, self.n, self.thin = int(nbins), int(n_ladders), int(n_chains), int(n), int(thin)
        self.range = (int(range_[0]), int(range_[1]))
        L, nt, k = self.n_ladders, len(self.betas_t), len(self.cols)
        self.shift = 0
        self.m, self.S0, self.SS = np.zeros((L, nt)), np.zeros((L, nt)), np.zeros((L, nt))
        self.origin = np.zeros((L, k))
        self.S1 = np.zeros((L, nt, k))
        self.cross = np.zeros((L, nt, k * (k + 1) // 2))
        self.hist = np.zeros((L, nt, k, self.nbins), dtype=np.uint64)
        self.q_total = np.zeros((L, nt), dtype=np.uint64)
        self._source = None

    @property
    def n_cols(self):
        return len(self.cols)

    def _shape(self, a):
        return a[0] if self.n_ladders == 1 else a

    # -- estimators ------------------------------------------------------------------------------------------------------
    def _ratio(self):
        return self.S1 / self.S0[:, :, None]

    def mean(self):
        """E[x_a] = origin_a + S1[a] / S0: [n_t][n_cols]"""
        return self._shape(self.origin[:, None, :] + self._ratio())

    def _cov(self):
        k, r = self.n_cols, self._ratio()
        out = np.zeros(self.S0.shape + (k, k))
        for a in range(k):
            for b in range(a, k):
                v = self.cross[:, :, tri_index(k, a, b)] / self.S0 - r[:, :, a] * r[:, :, b]
                out[:, :, a, b] = out[:, :, b, a] = v
        return out

    def cov(self):
        """Cov[x_a, x_b] = cross[a][b] / S0 - (S1[a] / S0)(S1[b] / S0), the moments about the range's first sample:
        [n_t][n_cols][n_cols]"""
        return self._shape(self._cov())

    def sd(self):
        c = self._cov()
        with np.errstate(invalid="ignore"):
            return self._shape(np.sqrt(np.diagonal(c, axis1=2, axis2=3)))

    def corr(self):
        c = self._cov()
        with np.errstate(invalid="ignore", divide="ignore"):
            s = np.sqrt(np.diagonal(c, axis1=2, axis2=3))
            return self._shape(c / (s[:, :, :, None] * s[:, :, None, :]))

    def ess(self):
        """Kish's effective sample size S0^2 / SS of the whole ladder's samples: [n_t]"""
        return self._shape(self.S0 * self.S0 / self.SS)

    def edges(self, a):
        return summary_edges(float(self.lo[a]), float(self.hi[a]), self.nbins)

    def mass(self):
        """hist / q_total: the weight of every bin as a share of all samples' (what fell outside the ranges is
        missing from a column's sum): [n_t][n_cols][nbins]"""
        return self._shape(self.hist.astype(np.float64) / self.q_total.astype(np.float64)[:, :, None, None])

    def density(self):
        """mass() over the bin widths"""
        width = np.array([np.diff(self.edges(a)) for a in range(self.n_cols)]).reshape(self.n_cols, self.nbins)
        return self._shape(self.hist.astype(np.float64) / self.q_total.astype(np.float64)[:, :, None, None] / width)

    def marginal(self, a, t=0, ladder=0):
        """(edges [nbins + 1], density [nbins]) of column slot a at target t"""
        e = self.edges(a)
        return e, self.hist[ladder, t, a].astype(np.float64) / float(self.q_total[ladder, t]) / np.diff(e)

    def quantile(self, p, a, t=0, ladder=0):
        """the p-quantile(s) of column slot a at target t from the weighted histogram: the weight inside the range is
        the whole, and a bin's weight is spread evenly over it"""
        e = self.edges(a)
        h = [int(v) for v in self.hist[ladder, t, a]]
        total = sum(h)
        if total == 0:
            raise ValueError("no weight inside the range of column slot %d" % a)
        cum = np.concatenate([[0.0], np.cumsum([v / total for v in h])])
        cum[-1] = 1.0
        return np.interp(np.asarray(p, dtype=np.float64), cum, e)

    def weights(self, t=0):
        """[t_count][n_chains]: the weights of target t, normalised to 1 within every ladder"""
        if self._source is None:
            raise ValueError("read from a file: the store is not here")
        rw, mbar, g = self._source
        e, _ = rw.weights(mbar, float(self.betas_t[t]), g, self.range[0], self.range[1])
        per = self.n_chains // self.n_ladders
        return e / np.repeat(self.S0[:, t], per)[None, :]

    # -- ladders, text, reweight.bin -------------------------------------------------------------------------------------
    _WORDS = ("m", "S0", "SS", "origin", "S1", "cross", "hist", "q_total")

    def per_ladder(self):
        """one Reweighted per ladder of a batch"""
        per, out = self.n_chains // self.n_ladders, []
        for b in range(self.n_ladders):
            one = Reweighted(self.cols, self.betas_t, self.lo, self.hi, self.nbins, 1, per, self.n, self.thin, self.range)
            one.shift = self.shift
            for w in self._WORDS:
                setattr(one, w, getattr(self, w)[b:b + 1].copy())
            out.append(one)
        return out

    def text(self, names=None):
        """reweight.txt of one ladder: per target and column `beta name mean sd ess`, "%.15e", tab separated"""
        if self.n_ladders != 1:
            raise ValueError("a batch of %d ladders: take per_ladder() first" % self.n_ladders)
        names = ["col%d" % c for c in self.cols] if names is None else list(names)
        mean, sd, ess = self.mean(), self.sd(), self.ess()
        return "".join("%s\t%s\t%s\t%s\t%s\n" % (_fmt(float(bt)), names[a], _fmt(float(mean[t, a])), _fmt(float(sd[t, a])),
                                                 _fmt(float(ess[t])))
                       for t, bt in enumerate(self.betas_t) for a in range(self.n_cols))

    def write(self, path):
        cols = np.zeros(MAX_COLS, dtype=np.int32)
        cols[:self.n_cols] = self.cols
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_chains, self.n_ladders, self.n_cols, len(self.betas_t), self.nbins,
                               self.shift, 0, self.n, self.thin, self.range[0], self.range[1], *cols.tolist()))
            for a in (self.lo, self.hi, self.betas_t, self.m, self.S0, self.SS, self.origin, self.S1, self.cross):
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())
            f.write(np.ascontiguousarray(self.hist, dtype="<u8").tobytes())
            f.write(np.ascontiguousarray(self.q_total, dtype="<u8").tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not a reweight file" % path)
        head = _HEAD.unpack_from(raw, 0)
        magic, version, nc, L, k, nt, nbins, shift, _, n, thin, t0, t_count = head[:13]
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a reweight file of version %d" % (path, VERSION))
        if not (1 <= k <= MAX_COLS and 1 <= nt <= MAX_TARGETS and 0 <= nbins <= MAX_BINS and L >= 1):
            raise ValueError("%s: a header out of range" % path)
        ntri = k * (k + 1) // 2
        sizes = [k, k, nt, L * nt, L * nt, L * nt, L * k, L * nt * k, L * nt * ntri, L * nt * k * nbins, L * nt]
        if _HEAD.size + 8 * sum(sizes) != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), _HEAD.size + 8 * sum(sizes)))
        parts, off = [], _HEAD.size
        for i, count in enumerate(sizes):
            parts.append(np.frombuffer(raw, dtype="<u8" if i >= 9 else "<f8", count=count, offset=off).copy())
            off += 8 * count
        r = cls(np.array(head[13:13 + k]), parts[2], parts[0], parts[1], nbins, L, nc, n, thin, (t0, t_count))
        r.shift = shift
        for w, a in zip(cls._WORDS, parts[3:]):
            setattr(r, w, a.reshape(getattr(r, w).shape).astype(getattr(r, w).dtype))
        return r


class Resampled:
    """n_draws equally weighted draws per ladder at one target, in stored order (time-major).  index, x and q_total
    carry the ladder first; every estimator is [...] for one ladder and [n_ladders][...] for a batch."""

    def __init__(self, cols, beta, u, n_draws, n_ladders, n_chains, n, thin, range_):
        self.cols = np.ascontiguousarray(cols, dtype=np.int32)
        self.beta, self.u, self.n_draws = float(beta), int(u), int(n_draws)
        self.n_ladders, self.n_chains, self.n, self.thin = int(n_ladders), int(n_chains), int(n), int(thin)
        self.range = (int(range_[0]), int(range_[1]))
        self.shift = 0
        self.index = np.zeros((self.n_ladders, self.n_draws), dtype=np.uint32)
        self.x = np.zeros((self.n_ladders, self.n_draws, len(self.cols)))
        self.q_total = np.zeros(self.n_ladders, dtype=np.uint64)

    @property
    def n_cols(self):
        return len(self.cols)

    @property
    def per(self):
        return self.n_chains // self.n_ladders

    @property
    def step(self):
        """[n_ladders][n_draws]: the kept step a draw was stored at, t0 + index div K"""
        return self.range[0] + self.index.astype(np.int64) // self.per

    @property
    def chain(self):
        """[n_ladders][n_draws]: the sampler's chain a draw came from, ladder b's first chain being b K"""
        return np.arange(self.n_ladders)[:, None] * self.per + self.index.astype(np.int64) % self.per

    def _shape(self, a):
        return a[0] if self.n_ladders == 1 else a

    def counts(self):
        """how often every sample of the range was drawn: [N], N = t_count K"""
        N = self.range[1] * self.per
        return self._shape(np.stack([np.bincount(i, minlength=N) for i in self.index]))

    def mean(self):
        """[n_cols]: the mean of the draws"""
        return self._shape(self.x.mean(axis=1))

    def cov(self):
        """[n_cols][n_cols]: the covariance of the draws about their mean, over n_draws"""
        d = self.x - self.x.mean(axis=1, keepdims=True)
        return self._shape(np.einsum("bma,bmc->bac", d, d) / self.n_draws)

    def sd(self):
        return self._shape(self.x.std(axis=1))

    def quantile(self, p, a, ladder=0):
        """the p-quantile(s) of column slot a, exact from the sorted draws: the smallest draw v with at least a share p
        of the draws <= v"""
        v = np.sort(self.x[ladder, :, a])
        p = np.asarray(p, dtype=np.float64)
        if np.any(p < 0) or np.any(p > 1):
            raise ValueError("a quantile is in [0, 1]")
        return v[np.clip(np.ceil(p * self.n_draws).astype(np.int64) - 1, 0, self.n_draws - 1)]

    def per_ladder(self):
        """one Resampled per ladder of a batch"""
        out = []
        for b in range(self.n_ladders):
            one = Resampled(self.cols, self.beta, self.u, self.n_draws, 1, self.per, self.n, self.thin, self.range)
            one.shift = self.shift
            one.index, one.x, one.q_total = self.index[b:b + 1].copy(), self.x[b:b + 1].copy(), self.q_total[b:b + 1].copy()
            out.append(one)
        return out

    def _one(self):
        if self.n_ladders != 1:
            raise ValueError("a batch of %d ladders: take per_ladder() first" % self.n_ladders)

    def text(self, names=None):
        """per column one line `beta name mean sd median` of one ladder's draws, "%.15e", tab separated"""
        self._one()
        names = ["col%d" % c for c in self.cols] if names is None else list(names)
        mean, sd = self.mean(), self.sd()
        return "".join("%s\t%s\t%s\t%s\t%s\n" % (_fmt(self.beta), names[a], _fmt(float(mean[a])), _fmt(float(sd[a])),
                                                 _fmt(float(self.quantile(0.5, a))))
                       for a in range(self.n_cols))

    def write_dumps(self, directory, names=None, t=0):
        """one ladder's draws as the reference's text sample dumps: per column <name>-reweighted-<t>.dump, one "%.15e"
        line per draw, the format of <name>-chain-0.prob.dump; returns the paths"""
        import os
        self._one()
        names = ["col%d" % c for c in self.cols] if names is None else list(names)
        paths = []
        for a in range(self.n_cols):
            paths.append(os.path.join(str(directory), "%s-reweighted-%d.dump" % (names[a], t)))
            with open(paths[-1], "w") as f:
                f.write("".join("%.15e\n" % v for v in self.x[0, :, a].tolist()))
        return paths

    def write(self, path):
        Resampled.write_all(path, [self])

    @staticmethod
    def write_all(path, targets):
        """resample.bin of the targets' draws: the same store, range, n_draws and u, one record per target"""
        r = targets[0]
        same = ("n_chains", "n_ladders", "n_draws", "shift", "n", "thin", "range", "u")
        if any(getattr(o, w) != getattr(r, w) for o in targets for w in same) \
                or any(o.cols.tobytes() != r.cols.tobytes() for o in targets):
            raise ValueError("the targets of one file share the store, the range, n_draws and u")
        cols = np.zeros(MAX_COLS, dtype=np.int32)
        cols[:r.n_cols] = r.cols
        with open(path, "wb") as f:
            f.write(_RESAMPLE_HEAD.pack(RESAMPLE_MAGIC, RESAMPLE_VERSION, r.n_chains, r.n_ladders, r.n_cols, len(targets),
                                        r.n_draws, r.shift, 0, r.n, r.thin, r.range[0], r.range[1], r.u, *cols.tolist()))
            for o in targets:
                f.write(struct.pack("<d", o.beta))
                f.write(np.ascontiguousarray(o.q_total, dtype="<u8").tobytes())
                f.write(np.ascontiguousarray(o.index, dtype="<u4").tobytes())
                f.write(np.ascontiguousarray(o.x, dtype="<f8").tobytes())

    @classmethod
    def read_all(cls, path):
        """the Resampled of every target of a resample.bin"""
        with open(path, "rb") as f:
            raw = f.read()
        head = _RESAMPLE_HEAD.unpack_from(raw, 0) if len(raw) >= _RESAMPLE_HEAD.size else (b"",) * 2
        if head[0] != RESAMPLE_MAGIC or head[1] != RESAMPLE_VERSION:
            raise ValueError("%s: not a resample file of version %d" % (path, RESAMPLE_VERSION))
        nc, L, k, nt, M, shift, _, n, thin, t0, t_count, u = head[2:14]
        if not (1 <= k <= MAX_COLS and 1 <= nt <= MAX_TARGETS and 1 <= M <= MAX_DRAWS and L >= 1):
            raise ValueError("%s: a header out of range" % path)
        record = 8 + 8 * L + 4 * L * M + 8 * L * M * k
        if _RESAMPLE_HEAD.size + nt * record != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), _RESAMPLE_HEAD.size + nt * record))
        out, off = [], _RESAMPLE_HEAD.size
        for _ in range(nt):
            r = cls(np.array(head[14:14 + k]), struct.unpack_from("<d", raw, off)[0], u, M, L, nc, n, thin, (t0, t_count))
            r.shift = shift
            off += 8
            r.q_total = np.frombuffer(raw, dtype="<u8", count=L, offset=off).astype(np.uint64)
            off += 8 * L
            r.index = np.frombuffer(raw, dtype="<u4", count=L * M, offset=off).astype(np.uint32).reshape(L, M)
            off += 4 * L * M
            r.x = np.frombuffer(raw, dtype="<f8", count=L * M * k, offset=off).astype(np.float64).reshape(L, M, k)
            off += 8 * L * M * k
            out.append(r)
        return out

    @classmethod
    def read(cls, path, t=0):
        """target t of a resample.bin"""
        return cls.read_all(path)[t]


def _fmt(v):
    return "nan" if v != v else "%.15e" % v
