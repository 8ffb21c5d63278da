"""Autocorrelation of sample columns: lag sums of kept chains, from what apemost_hip_autocorr_get hands out, and the
integrated autocorrelation time, the effective sample size and the Monte Carlo standard error they give.

An Autocorr holds one view (include/apemost_hip.h, apemost_hip_autocorr_view).  A series is one (kept chain k, listed
column c) pair with the samples x_0, x_1, ... in kept order and d_t = x_t - origin; with L = max_lag it keeps n, origin,
sum = sum d_t, lag[l] = sum_{t >= l} d_t d_{t-l} for l < L, head[j] = d_j and tail[j] = d_{n-(L-1)+j} for j < L - 1
(0 where there is no such sample).  With m = sum / n the autocovariance about the mean follows exactly:

    acov_l = (lag_l - m (sum - sum_{j<l} head_j) - m (sum - sum of the last l tail entries) + (n - l) m^2) / n

The estimators are written as scalar loops over Python floats, so that the C host (apemost_amd/host/src/run_autocorr.c)
can repeat them operation for operation.  It reads and writes `autocorr.bin`, the file the C host's run phase leaves
with the APEMOST_DUMP token `autocorr`.

autocorr.bin (little-endian), version 1:
    char[8]  "APEMOSTA"
    uint32   version, n_keep, n_cols, max_lag, n_par, n_ladders
    uint64   n, thin
    int32    chains[n_keep], cols[n_cols]
    double   origin[n_keep][n_cols], sum[n_keep][n_cols]
    double   lag[n_keep][n_cols][max_lag]
    double   head[n_keep][n_cols][max_lag - 1], tail[n_keep][n_cols][max_lag - 1]
"""
import math
import struct

import numpy as np

from . import capi

MAGIC = b"APEMOSTA"
VERSION = 1
MAX_LAG = 4096
_HEAD = struct.Struct("<8s6I2Q")


def default_cols(n_par):
    """the n_par parameters and column n_par + 1 (prob - prior)"""
    return list(range(n_par)) + [n_par + 1]


class Autocorr:
    def __init__(self, n, origin, sum, lag, head, tail, chains, cols, n_par, thin=1, n_ladders=1):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.chains = np.ascontiguousarray(chains, dtype=np.int32).reshape(-1)
        self.cols = np.ascontiguousarray(cols, dtype=np.int32).reshape(-1)
        self.n_keep, self.n_cols = len(self.chains), len(self.cols)
        shape = (self.n_keep, self.n_cols)
        self.origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(shape)
        self.sum = np.ascontiguousarray(sum, dtype=np.float64).reshape(shape)
        self.lag = np.ascontiguousarray(lag, dtype=np.float64).reshape(shape + (-1,))
        self.max_lag = self.lag.shape[2]
        self.head = np.ascontiguousarray(head, dtype=np.float64).reshape(shape + (self.max_lag - 1,))
        self.tail = np.ascontiguousarray(tail, dtype=np.float64).reshape(shape + (self.max_lag - 1,))
        self.n_par, self.thin, self.n_ladders = int(n_par), int(thin), int(n_ladders)

    @classmethod
    def empty(cls, chains, max_lag, n_par, cols=None, thin=1, n_ladders=1):
        cols = default_cols(n_par) if cols is None else cols
        k, c, L = len(chains), len(cols), int(max_lag)
        return cls(np.zeros(1, dtype=np.uint64), np.zeros((k, c)), np.zeros((k, c)), np.zeros((k, c, L)),
                   np.zeros((k, c, L - 1)), np.zeros((k, c, L - 1)), chains, cols, n_par, thin, n_ladders)

    def view(self):
        """the apemost_hip_autocorr_view over this object's arrays"""
        dp = capi._dp
        return capi.AutocorrView(n=self.n.ctypes.data_as(capi._up), origin=self.origin.ctypes.data_as(dp),
                                 sum=self.sum.ctypes.data_as(dp), lag=self.lag.ctypes.data_as(dp),
                                 head=self.head.ctypes.data_as(dp), tail=self.tail.ctypes.data_as(dp))

    @classmethod
    def from_rows(cls, rows, chains, max_lag, cols=None, thin=1):
        """the fold of host sample rows [n][n_chains][n_par+2] (already thinned; thin is recorded): what the device
        computes, for tests and for existing dumps.  Lag by lag with numpy's cumulative sums, which add in sample order."""
        rows = np.asarray(rows, dtype=np.float64)
        n, _, w = rows.shape
        ac = cls.empty(chains, max_lag, w - 2, cols, thin)
        ac.n[0] = n
        L, H = ac.max_lag, ac.max_lag - 1
        if n == 0:
            return ac
        with np.errstate(all="ignore"):
            for k, chain in enumerate(ac.chains.tolist()):
                for c, col in enumerate(ac.cols.tolist()):
                    x = np.ascontiguousarray(rows[:, chain, col])
                    d = x - x[0]
                    ac.origin[k, c] = x[0]
                    ac.sum[k, c] = _total(d)
                    for l in range(min(L, n)):
                        ac.lag[k, c, l] = _total(d[l:] * d[:n - l])
                    ac.head[k, c, :min(H, n)] = d[:min(H, n)]
                    if H > 0:
                        ac.tail[k, c, max(H - n, 0):] = d[max(n - H, 0):]
        return ac

    def per_ladder(self, n_ladders=None):
        """one Autocorr per ladder of a batch: the kept chains, ladder-major, in equal shares"""
        n_ladders = self.n_ladders if n_ladders is None else n_ladders
        if n_ladders < 1 or self.n_keep % n_ladders:
            raise ValueError("%d kept chains are not %d equal ladders" % (self.n_keep, n_ladders))
        per = self.n_keep // n_ladders
        out = []
        for b in range(n_ladders):
            k = slice(b * per, (b + 1) * per)
            out.append(Autocorr(self.n.copy(), self.origin[k], self.sum[k], self.lag[k], self.head[k], self.tail[k],
                                self.chains[k], self.cols, self.n_par, self.thin, 1))
        return out

    # -- what it gives ------------------------------------------------------------------------
    def lags(self):
        """lags that have at least one pair: min(max_lag, n)"""
        return min(self.max_lag, int(self.n[0]))

    def mean(self, k=0):
        with np.errstate(all="ignore"):
            return self.origin[k] + self.sum[k] / np.float64(self.n[0])

    def _acov(self, k, c):
        """the autocovariance about the mean of series (k, c) as a list of max_lag floats, 0 from lag n on"""
        L, H = self.max_lag, self.max_lag - 1
        n = float(int(self.n[0]))
        out = [0.0] * L
        if n == 0:
            return out
        total = float(self.sum[k, c])
        lag, head, tail = self.lag[k, c].tolist(), self.head[k, c].tolist(), self.tail[k, c].tolist()
        m = total / n
        first = 0.0                                          # sum of the first l values of d
        last = 0.0                                           # sum of the last l values of d
        for l in range(self.lags()):
            if l > 0:
                first += head[l - 1]
                last += tail[H - l]
            a = lag[l] - m * (total - first)
            a = a - m * (total - last)
            a = a + (n - l) * m * m
            out[l] = a / n
        return out

    def acov(self, k=0):
        """[n_cols][max_lag]: the autocovariance (divided by n) of every column of kept chain k"""
        return np.array([self._acov(k, c) for c in range(self.n_cols)])

    def variance(self, k=0):
        return self.acov(k)[:, 0]

    @staticmethod
    def _rho(acov):
        a0 = acov[0]
        return [_div(a, a0) for a in acov]

    def acf(self, k=0):
        """[n_cols][max_lag]: acov / acov[0]"""
        return np.array([self._rho(self._acov(k, c)) for c in range(self.n_cols)])

    def _tau(self, acov, method, c):
        rho, lags = self._rho(acov), self.lags()
        if method == "sokal":
            # the smallest window M >= c tau(M), tau(M) = 1 + 2 sum_{l <= M} rho_l (Sokal 1989)
            s = 0.0
            for M in range(1, lags):
                s += rho[M]
                t = 1.0 + 2.0 * s
                if M >= c * t:
                    return t, M
            return 1.0 + 2.0 * s, -1
        if method == "geyer":
            # the initial positive sequence: Gamma_j = rho_2j + rho_2j+1 summed while positive (Geyer 1992)
            g, j = 0.0, 0
            while 2 * j + 1 < lags:
                G = rho[2 * j] + rho[2 * j + 1]
                if not G > 0:
                    return 2.0 * g - 1.0, 2 * j - 1
                g += G
                j += 1
            return 2.0 * g - 1.0, -1
        raise ValueError("method %r: sokal or geyer" % (method,))

    def tau(self, k=0, method="sokal", c=5.0):
        """(tau [n_cols], window [n_cols]) of kept chain k, in kept samples.  window is the last lag summed; -1 where
        no window closed below max_lag: tau is then the sum over all lags, a lower bound."""
        got = [self._tau(self._acov(k, col), method, float(c)) for col in range(self.n_cols)]
        return np.array([t for t, _ in got]), np.array([w for _, w in got], dtype=np.int64)

    def converged(self, k=0, method="sokal", c=5.0):
        return self.tau(k, method, c)[1] >= 0

    def ess(self, k=0, method="sokal", c=5.0):
        """n / tau"""
        return np.array([_div(float(int(self.n[0])), t) for t in self.tau(k, method, c)[0].tolist()])

    def mcse(self, k=0, method="sokal", c=5.0):
        """sqrt(acov_0 tau / n): the standard error of the mean"""
        n = float(int(self.n[0]))
        return np.array([_sqrt(_div(a0 * t, n))
                         for a0, t in zip(self.variance(k).tolist(), self.tau(k, method, c)[0].tolist())])

    def text(self, names=None, k=0):
        """autocorr.txt: one line per column, `name mean variance tau_sokal window ess mcse tau_geyer`, tab separated,
        "%.15e".  names: of the parameters; column n_par is `prob`, column n_par + 1 `prob-prior`."""
        names = ["p%d" % p for p in range(self.n_par)] if names is None else list(names)
        names = names[:self.n_par] + ["prob", "prob-prior"]
        n = float(int(self.n[0]))
        out = []
        for c, col in enumerate(self.cols.tolist()):
            acov = self._acov(k, c)
            mean = float(self.origin[k, c]) + _div(float(self.sum[k, c]), n)
            ts, w = self._tau(acov, "sokal", 5.0)
            tg, _ = self._tau(acov, "geyer", 5.0)
            out.append("%s\t%s\t%s\t%s\t%d\t%s\t%s\t%s\n" % (names[col], _fmt(mean), _fmt(acov[0]), _fmt(ts), w,
                                                             _fmt(_div(n, ts)), _fmt(_sqrt(_div(acov[0] * ts, n))),
                                                             _fmt(tg)))
        return "".join(out)

    # -- autocorr.bin ---------------------------------------------------------------------------
    def write(self, path):
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_keep, self.n_cols, self.max_lag, self.n_par, self.n_ladders,
                               int(self.n[0]), self.thin))
            for a, t in ((self.chains, "<i4"), (self.cols, "<i4"), (self.origin, "<f8"), (self.sum, "<f8"),
                         (self.lag, "<f8"), (self.head, "<f8"), (self.tail, "<f8")):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not an autocorr file" % path)
        magic, version, n_keep, n_cols, L, n_par, n_ladders, n, thin = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not an autocorr file of version %d" % (path, VERSION))
        ns = n_keep * n_cols
        want = _HEAD.size + 4 * (n_keep + n_cols) + 8 * ns * (2 + L + 2 * (L - 1))
        if L < 1 or want != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), want))
        off = _HEAD.size

        def take(count, dtype):
            nonlocal off
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=off)
            off += a.itemsize * count
            return a.copy()
        chains, cols = take(n_keep, "<i4"), take(n_cols, "<i4")
        origin, total = take(ns, "<f8"), take(ns, "<f8")
        lag, head, tail = take(ns * L, "<f8"), take(ns * (L - 1), "<f8"), take(ns * (L - 1), "<f8")
        return cls([n], origin, total, lag.reshape(n_keep, n_cols, L), head, tail, chains, cols, n_par, thin, n_ladders)


def _total(v):
    """the sequential sum 0.0 + v_0 + v_1 + ...: numpy's cumulative sum adds in index order"""
    return np.cumsum(np.concatenate(([0.0], v)))[-1]


def _div(a, b):
    """a / b as C divides: by zero gives inf or NaN"""
    if b == 0:
        if a != a or a == 0:
            return math.nan
        return math.copysign(math.inf, a) * math.copysign(1.0, b)
    return a / b


def _sqrt(v):
    return math.sqrt(v) if v >= 0 else math.nan


def _fmt(v):
    return "nan" if v != v else "%.15e" % v
