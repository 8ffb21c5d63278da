"""Posterior predictive checks from what apemost_hip_check_get hands out: is the model adequate for these data, or is
there still a signal in the residuals?

A Check holds one view (include/apemost_hip.h, apemost_hip_check_view), the data it was folded over and the edges of its
histograms.  With v the model curve at x_i under a kept sample (the operation order is in apemost_amd/csrc/pt_check.h):

    simplesin, sine3    e = (y_i - v) / sigma, the standardised residual;   u = Phi(e)
    pulse, pulse_vrot   e = y_i / v, the ratio, Exp(1) under the model;      u = 1 - exp(-e)

u is the predictive CDF at the observed value.  Per datum i (all of these return [n_data] arrays):

    pit        = sum_u / n            the posterior mean of u: uniform on (0, 1) over the data if the model is adequate
    loo_pit    = SU / S               the same under the leave-one-out weights 1 / p(y_i | theta): the datum does not
                                      vouch for itself
    resid_mean = origin + sum / n     resid_sd = sqrt((sq - sum * sum / n) / (n - 1)), never below 0

Per kept sample the device takes three discrepancy statistics T over the kept chain's L data and folds them per kept chain:

    FIT      sine: sum e^2, null chi^2 with L degrees of freedom; pulse: sum e, null Gamma(L, 1)
    EXTREME  sine: max |e_i|; pulse: max e_i
    SERIAL   sum_{i >= 1} (u_i - 1/2) (u_{i-1} - 1/2): null mean 0, variance (L - 1) / 144; the one that sees an
             unmodelled periodic signal

stat_mean, stat_sd, stat_min and stat_max describe T over the samples.  With the histogram's edges at the null quantiles
j / nbins (null_edges; HipSampler.check_begin's default), slot b of p_hist holds the samples whose null CDF lies in
[b, b + 1) / nbins, and

    p_value(stat, "upper") = sum_b counts[b] (1 - (b + 1/2) / nbins) / n

is the posterior predictive p-value of T, the posterior mean of the null's upper tail at T, to a half-width of
1 / (2 nbins): small where T is larger than the model allows.  "lower" is its complement, "two" twice the smaller of the
two (half-width 1 / nbins).  Samples whose T is NaN are counted in the last slot and left out of n here.  The null law of
SERIAL is a normal approximation, poor for small L; a histogram over other edges than the null quantiles is a
histogram and its p_value means nothing.

The checks mean what they say for a chain at beta = 1, which is chain 0 and the default.  A fold over a batch whose
ladders differ in data length stays rectangular and carries `lengths`; per_ladder() trims, and text and write refuse
the untrimmed object.  The package does not use scipy: null_edges is the library's own host function.

check.bin (little-endian), version 1:
    char[8]  "APEMOSTK"
    uint32   version, n_keep, n_data, n_edges, n_ladders, model, 0, 0
    uint64   n, thin
    double   sigma
    int32    chains[n_keep]
    double   x, y: [n_keep][n_data] each
    double   origin, sum, sq, sum_u, m, S, SU: [n_keep][n_data] each
    double   edges[3][n_edges]
    double   stat_origin, stat_sum, stat_sq, stat_min, stat_max: [n_keep][3] each
    uint64   counts[n_keep][3][n_edges + 2]
"""
import struct

import numpy as np

from . import capi

MAGIC = b"APEMOSTK"
VERSION = 1
FIT, EXTREME, SERIAL = 0, 1, 2
N_STATS = 3
STAT_NAMES = ("fit", "extreme", "serial")
MAX_EDGES = 4095
STATE = ("origin", "sum", "sq", "sum_u", "m", "S", "SU")
STAT_STATE = ("stat_origin", "stat_sum", "stat_sq", "stat_min", "stat_max")
_HEAD = struct.Struct("<8s8I2Qd")


def null_edges(model, stat, n_data, n_edges):
    """[n_edges]: the null quantiles (j + 1) / (n_edges + 1) of statistic `stat` of a built-in model over n_data data
    (apemost_hip_check_null_edges: host arithmetic, no device); FIT and EXTREME exact, SERIAL a normal approximation"""
    out = np.zeros(max(int(n_edges), 0))
    capi.check(capi.lib().apemost_hip_check_null_edges(int(model), int(stat), int(n_data), int(n_edges),
                                                       out.ctypes.data_as(capi._dp)))
    return out


def slots(T, edges):
    """the slot of every T among the ascending edges, as the device counts: #{j : edges[j] <= T}, len(edges) + 1 for NaN"""
    T = np.asarray(T, dtype=np.float64)
    b = np.searchsorted(np.asarray(edges, dtype=np.float64), T, side="right")
    return np.where(np.isnan(T), len(edges) + 1, b)


def _stat(stat):
    if isinstance(stat, str):
        if stat not in STAT_NAMES:
            raise ValueError("statistic %r: one of %s" % (stat, ", ".join(STAT_NAMES)))
        return STAT_NAMES.index(stat)
    if stat not in (FIT, EXTREME, SERIAL):
        raise ValueError("statistic %r: 0, 1 or 2" % (stat,))
    return int(stat)


class Check:
    """The state of one fold of the predictive checks and what it says (the formulas are in the module's docstring)."""

    lengths = None   # [n_keep] data per kept chain of a ragged batch's fold

    def __init__(self, n, origin, sum, sq, sum_u, m, S, SU, stat_origin, stat_sum, stat_sq, stat_min, stat_max, counts, chains,
                 x, y, edges, model, sigma=0.5, thin=1, n_ladders=1):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.chains = np.ascontiguousarray(chains, dtype=np.int32).reshape(-1)
        self.n_keep = len(self.chains)
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.n_keep, -1)
        self.n_data = self.x.shape[1]
        shape = (self.n_keep, self.n_data)
        self.y = np.ascontiguousarray(y, dtype=np.float64).reshape(shape)
        for name, a in zip(STATE, (origin, sum, sq, sum_u, m, S, SU)):
            setattr(self, name, np.ascontiguousarray(a, dtype=np.float64).reshape(shape))
        for name, a in zip(STAT_STATE, (stat_origin, stat_sum, stat_sq, stat_min, stat_max)):
            setattr(self, name, np.ascontiguousarray(a, dtype=np.float64).reshape(self.n_keep, N_STATS))
        self.edges = np.ascontiguousarray(edges, dtype=np.float64).reshape(N_STATS, -1)
        self.n_edges = self.edges.shape[1]
        self.nbins = self.n_edges + 1
        self.counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(self.n_keep, N_STATS, self.n_edges + 2)
        self.model, self.sigma, self.thin, self.n_ladders = int(model), float(sigma), int(thin), int(n_ladders)

    @classmethod
    def empty(cls, chains, x, y, edges, model, sigma=0.5, thin=1, n_ladders=1):
        k = len(chains)
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        x = np.tile(x, (k, 1)) if x.ndim == 1 else x
        y = np.tile(y, (k, 1)) if y.ndim == 1 else y
        edges = np.asarray(edges, dtype=np.float64).reshape(N_STATS, -1)
        z = [np.zeros(x.shape) for _ in STATE] + [np.zeros((k, N_STATS)) for _ in STAT_STATE]
        return cls(np.zeros(1, dtype=np.uint64), *z, np.zeros((k, N_STATS, edges.shape[1] + 2), dtype=np.uint64), chains, x, y,
                   edges, model, sigma, thin, n_ladders)

    def view(self):
        """the apemost_hip_check_view over this object's arrays"""
        dp = capi._dp
        return capi.CheckView(n=self.n.ctypes.data_as(capi._up), counts=self.counts.ctypes.data_as(capi._up),
                              **{f: getattr(self, f).ctypes.data_as(dp) for f in STATE + STAT_STATE})

    def is_ragged(self):
        return self.lengths is not None and bool(np.any(np.asarray(self.lengths) != self.n_data))

    def _no_padding(self, what):
        if self.is_ragged():
            raise ValueError("%s over a ragged batch's fold would take padding for data (lengths %s of n_data %d): "
                             "use per_ladder(), which trims every ladder to its length"
                             % (what, np.asarray(self.lengths).tolist(), self.n_data))

    def per_ladder(self, n_ladders=None):
        """one Check per ladder of a batch: the kept chains, ladder-major, in equal shares; of a ragged batch's fold
        each trimmed to its ladder's length"""
        n_ladders = self.n_ladders if n_ladders is None else n_ladders
        if n_ladders < 1 or self.n_keep % n_ladders:
            raise ValueError("%d kept chains are not %d equal ladders" % (self.n_keep, n_ladders))
        per = self.n_keep // n_ladders
        out = []
        for b in range(n_ladders):
            k = slice(b * per, (b + 1) * per)
            m = self.n_data
            if self.lengths is not None:
                mine = np.asarray(self.lengths)[k]
                if np.any(mine != mine[0]):
                    raise ValueError("ladder %d: its kept chains have lengths %s" % (b, mine.tolist()))
                m = int(mine[0])
            out.append(Check(self.n.copy(), *[getattr(self, f)[k, :m] for f in STATE], *[getattr(self, f)[k] for f in STAT_STATE],
                             self.counts[k], self.chains[k], self.x[k, :m], self.y[k, :m], self.edges, self.model, self.sigma,
                             self.thin, 1))
        return out

    # -- per datum ----------------------------------------------------------------------------
    def _n(self):
        return np.float64(self.n[0])

    def pit(self, k=0):
        """[n_data]: sum_u / n, the posterior predictive PIT of every datum"""
        with np.errstate(all="ignore"):
            return self.sum_u[k] / self._n()

    def loo_pit(self, k=0):
        """[n_data]: SU / S, the leave-one-out PIT of every datum"""
        with np.errstate(all="ignore"):
            return self.SU[k] / self.S[k]

    def resid_mean(self, k=0):
        """[n_data]: origin + sum / n, the posterior mean of e"""
        with np.errstate(all="ignore"):
            return self.origin[k] + self.sum[k] / self._n()

    def resid_sd(self, k=0):
        """[n_data]: sqrt((sq - sum * sum / n) / (n - 1)), the variance never below 0"""
        return _sd(self.sum[k], self.sq[k], self._n())

    def outliers(self, level=0.01, k=0):
        """indices of the data whose leave-one-out PIT lies in a tail of mass level / 2 (or is NaN): the observations
        the rest of the data and the model do not expect"""
        p = self.loo_pit(k)
        if self.lengths is not None:
            p = p[:int(np.asarray(self.lengths)[k])]
        with np.errstate(all="ignore"):
            return np.flatnonzero(~((p >= level / 2) & (p <= 1 - level / 2)))

    # -- per statistic ------------------------------------------------------------------------
    def stat_mean(self, k=0):
        """[3]: the mean of every statistic over the kept samples"""
        with np.errstate(all="ignore"):
            return self.stat_origin[k] + self.stat_sum[k] / self._n()

    def stat_sd(self, k=0):
        return _sd(self.stat_sum[k], self.stat_sq[k], self._n())

    def p_hist(self, stat, k=0):
        """[nbins]: the counts of the statistic's slots, the NaN slot left out"""
        return self.counts[k, _stat(stat), :self.nbins].copy()

    def n_nan(self, stat, k=0):
        return int(self.counts[k, _stat(stat), self.nbins])

    def p_value(self, stat, tail="upper", k=0):
        """(p, half_width): the posterior predictive p-value of the statistic from its histogram over the null
        quantiles; tail "upper", "lower" or "two".  NaN without a histogram or without a sample that is not NaN"""
        if tail not in ("upper", "lower", "two"):
            raise ValueError("tail %r: upper, lower or two" % (tail,))
        n = upper = 0.0
        for b, c in enumerate(self.p_hist(stat, k).tolist()):     # (in slot order, as the C host adds)
            n += float(c)
            upper += float(c) * (1.0 - (b + 0.5) / float(self.nbins))
        if self.nbins < 2 or n == 0:
            return float("nan"), float("nan")
        upper = upper / n
        half = 1.0 / (2 * self.nbins)
        if tail == "upper":
            return upper, half
        if tail == "lower":
            return 1.0 - upper, half
        return min(1.0, 2.0 * min(upper, 1.0 - upper)), 2 * half

    # -- text ---------------------------------------------------------------------------------
    def text(self, k=0):
        """check.txt: one line per datum, `x y mean sd pit loo_pit`, tab separated, %.15e"""
        self._no_padding("text")
        cols = [self.x[k], self.y[k], self.resid_mean(k), self.resid_sd(k), self.pit(k), self.loo_pit(k)]
        return "".join("\t".join(_fmt(float(c[i])) for c in cols) + "\n" for i in range(self.n_data))

    def stats_text(self, k=0):
        """check_stats.txt: one line per statistic, `name mean sd min max p_upper p_lower p_two`, tab separated"""
        mean, sd = self.stat_mean(k), self.stat_sd(k)
        return "".join("\t".join([STAT_NAMES[q]] + [_fmt(float(v)) for v in (
            mean[q], sd[q], self.stat_min[k, q], self.stat_max[k, q], self.p_value(q, "upper", k)[0],
            self.p_value(q, "lower", k)[0], self.p_value(q, "two", k)[0])]) + "\n" for q in range(N_STATS))

    # -- check.bin ----------------------------------------------------------------------------
    def _arrays(self):
        return ([(self.chains, "<i4"), (self.x, "<f8"), (self.y, "<f8")] + [(getattr(self, f), "<f8") for f in STATE] +
                [(self.edges, "<f8")] + [(getattr(self, f), "<f8") for f in STAT_STATE] + [(self.counts, "<u8")])

    def write(self, path):
        self._no_padding("write")
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_keep, self.n_data, self.n_edges, self.n_ladders, self.model, 0, 0,
                               int(self.n[0]), self.thin, self.sigma))
            for a, t in self._arrays():
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not a check file" % path)
        magic, version, n_keep, n_data, n_edges, n_ladders, model, _, _, n, thin, sigma = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a check file of version %d" % (path, VERSION))
        ns, nq = n_keep * n_data, n_keep * N_STATS
        want = _HEAD.size + 4 * n_keep + 8 * (9 * ns + N_STATS * n_edges + 5 * nq + nq * (n_edges + 2))
        if want != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), want))
        off = _HEAD.size

        def take(count, dtype):
            nonlocal off
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=off)
            off += a.itemsize * count
            return a.copy()
        chains, x, y = take(n_keep, "<i4"), take(ns, "<f8"), take(ns, "<f8")
        state = [take(ns, "<f8") for _ in STATE]
        edges = take(N_STATS * n_edges, "<f8")
        stat = [take(nq, "<f8") for _ in STAT_STATE]
        counts = take(nq * (n_edges + 2), "<u8")
        return cls([n], *state, *stat, counts, chains, x, y, edges, model, sigma, thin, n_ladders)


def _sd(total, sq, n):
    with np.errstate(all="ignore"):
        v = (sq - total * total / n) / (n - np.float64(1.0))
        return np.sqrt(np.where(v < 0, 0.0, v))


def _fmt(v):
    return "nan" if v != v else "%.15e" % v
