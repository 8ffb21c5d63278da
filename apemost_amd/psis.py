"""Pareto-smoothed importance-sampling leave-one-out (PSIS-LOO; Vehtari, Gelman & Gabry 2017; Vehtari, Simpson, Gelman,
Yao & Gabry 2024) from the state of a pointwise fold and its tail, without the per-sample terms.

A series is one (kept chain k, datum i) pair; its leave-one-out log weights are x_t = -l_t over the n kept samples.  The
pointwise fold (pointwise.py) keeps m = m_dn = max x and S_dn = sum exp(x - m).  The tail (apemost_hip_pointwise_tail_*,
apemost_amd/csrc/pt_pointwise_tail.h) keeps count = min(capacity, samples whose term is not NaN) and values[0 .. count),
the largest x, descending, exactly.  PSIS replaces the M largest weights by order statistics of a generalised Pareto
distribution fitted to them, M = tail_length(n) = ceil(min(0.2 n, 3 sqrt(n / r_eff))); it needs the M + 1 largest
values (the last is the cutoff) and nothing else of the samples, so capacity_for(n) = min(4096, tail_length(n) + 1).

psis(), per series:
    M     = min(tail_length(n, r_eff), count - 1); tail_short says where the capacity (or NaN terms) cut it short
    t_j   = values[M-1-j] - m, j = 0 .. M-1, ascending, all <= 0;  cutoff c = values[M] - m
    fit   (k, sigma) = gpdfit(exp(t) - exp(c)), unless M < 5, m is not finite, or t_{M-1} - t_0 < 2^-52 / 100 (all tail
          values equal): then there is no fit, pareto_k = +inf and the weights stay raw.  A NaN k becomes +inf; a
          non-finite k leaves the tail raw as well.
    s_j   = min(0, ln(sigma * expm1(-k * log1p(-p_j)) / k + exp(c))), p_j = (j + 1/2) / M; for k = 0 the limit
          -sigma * log1p(-p_j) in place of the quotient.  (smooth=False: s = t.)
    elpd  = ln((n - M) + sum_j exp(s_j - t_j)) - m - ln(S_dn - sum_j exp(t_j) + sum_j exp(s_j)),
          the three sums by math.fsum.  With s = t this is ln n - m - ln S_dn = Pointwise.elpd_loo.
The last subtraction carries S_dn's own error: the device's sequential sum is good to n 2^-50 relative to S_dn
(tests/test_gpu_pointwise.py), which is n 2^-50 * ratio relative to the difference, ratio = S_dn / (S_dn - sum exp(t) +
sum exp(s)).  psis() returns that ratio per datum (Psis.ratio): where it is large the smoothed denominator has been
cancelled and elpd carries an error of about n 2^-50 * ratio.  Where the fold's S_dn is NaN or infinite (a NaN or
infinite term) elpd is what IEEE arithmetic gives, as Pointwise.elpd_loo is; pareto_k comes from the tail alone.

pareto_k is the diagnostic: below k_threshold(n) = min(1 - 1 / log10 n, 0.7) the estimate is reliable, between that and 1
it is biased, above 1 the weights have no mean (k_table).  r_eff is not estimated here: the default 1 is the rule for
independent samples.  Tails beyond 4095 values are not kept: runs above 1.86e6 kept samples get tail_short.

pointwise_tail.bin (little-endian), version 1:
    char[8]  "APEMOSTT"
    uint32   version, n_keep, n_data, capacity, n_ladders, 0, 0, 0
    uint64   n, thin
    int32    chains[n_keep]
    uint64   count[n_keep][n_data]
    double   values[n_keep][n_data][capacity]      descending; the slots at and behind count are 0

`python -m apemost_amd.psis DIR` reads pointwise.bin and pointwise_tail.bin of a run directory and prints Psis.text().
"""
import math
import os
import struct
import sys

import numpy as np

from . import capi
from .pointwise import Pointwise, _fmt, _ln, _spread, _total

MAGIC = b"APEMOSTT"
VERSION = 1
MAX_CAPACITY = 4096
MIN_TAIL = 5
_HEAD = struct.Struct("<8s8I2Q")


def tail_length(n, r_eff=1.0):
    """M of the rule: ceil(min(0.2 n, 3 sqrt(n / r_eff)))"""
    n = float(n)
    return int(math.ceil(min(0.2 * n, 3.0 * math.sqrt(n / r_eff))))


def capacity_for(n):
    """the tail capacity a run of n kept samples needs: the M largest weights and the cutoff, at most 4096"""
    return max(2, min(MAX_CAPACITY, tail_length(n) + 1))


def k_threshold(n):
    """min(1 - 1 / log10 n, 0.7): the Pareto k up to which n samples give a reliable estimate"""
    n = float(n)
    if n <= 1:
        return -math.inf
    return min(1.0 - 1.0 / math.log10(n), 0.7)


def gpdfit(x):
    """(k, sigma) of a generalised Pareto distribution fitted to the ascending positive exceedances x: the Zhang-Stephens
    (2009) estimator with the weakly informative adjustment of k, as the `loo` package configures it.  A NaN k becomes
    +inf."""
    x = np.asarray(x, dtype=np.float64)
    N = len(x)
    with np.errstate(all="ignore"):
        G = 30 + int(math.floor(math.sqrt(N)))
        xstar = x[int(math.floor(N / 4 + 0.5)) - 1]
        j = np.arange(1, G + 1, dtype=np.float64)
        theta = 1.0 / x[N - 1] + (1.0 - np.sqrt(G / (j - 0.5))) / 3.0 / xstar
        kj = np.array([np.mean(np.log1p(-th * x)) for th in theta])
        lj = N * (np.log(-theta / kj) - kj - 1.0)
        w = np.array([1.0 / np.sum(np.exp(lj - v)) for v in lj])
        theta_hat = np.sum(theta * w)
        k = np.mean(np.log1p(-theta_hat * x))
        sigma = -k / theta_hat
        k = (k * N + 5.0) / (N + 10.0)
    k, sigma = float(k), float(sigma)
    if k != k:
        k = math.inf
    return k, sigma


class PointwiseTail:
    """The tail of a pointwise fold: count [n_keep][n_data] and values [n_keep][n_data][capacity], the count largest
    x = -l of every series, descending (the module's docstring has the file's layout)."""

    def __init__(self, count, values, capacity, chains, n, thin=1, n_ladders=1):
        self.chains = np.ascontiguousarray(chains, dtype=np.int32).reshape(-1)
        self.n_keep = len(self.chains)
        self.capacity = int(capacity)
        self.count = np.ascontiguousarray(count, dtype=np.uint64).reshape(self.n_keep, -1).copy()
        self.n_data = self.count.shape[1]
        self.values = np.ascontiguousarray(values, dtype=np.float64).reshape(self.n_keep, self.n_data, self.capacity).copy()
        self.n, self.thin, self.n_ladders = int(n), int(thin), int(n_ladders)
        if self.count.size and int(self.count.max()) > self.capacity:
            raise ValueError("a count of %d is above the capacity %d" % (int(self.count.max()), self.capacity))

    @classmethod
    def empty(cls, chains, n_data, capacity, n=0, thin=1, n_ladders=1):
        k = len(chains)
        return cls(np.zeros((k, n_data), dtype=np.uint64), np.zeros((k, n_data, capacity)), capacity, chains, n, thin,
                   n_ladders)

    def view(self):
        """the apemost_hip_pointwise_tail_view over this object's arrays"""
        return capi.PointwiseTailView(count=self.count.ctypes.data_as(capi._up), values=self.values.ctypes.data_as(capi._dp))

    def clear_unused(self):
        """0 in the slots at and behind count, which pointwise_tail_get leaves unspecified"""
        self.values[np.arange(self.capacity)[None, None, :] >= self.count[:, :, None].astype(np.int64)] = 0.0

    def per_ladder(self, n_ladders=None):
        """one PointwiseTail per ladder of a batch: the kept chains, ladder-major, in equal shares"""
        n_ladders = self.n_ladders if n_ladders is None else n_ladders
        if n_ladders < 1 or self.n_keep % n_ladders:
            raise ValueError("%d kept chains are not %d equal ladders" % (self.n_keep, n_ladders))
        per = self.n_keep // n_ladders
        return [PointwiseTail(self.count[b * per:(b + 1) * per], self.values[b * per:(b + 1) * per], self.capacity,
                              self.chains[b * per:(b + 1) * per], self.n, self.thin, 1) for b in range(n_ladders)]

    def write(self, path):
        t = PointwiseTail(self.count, self.values, self.capacity, self.chains, self.n, self.thin, self.n_ladders)
        t.clear_unused()
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, t.n_keep, t.n_data, t.capacity, t.n_ladders, 0, 0, 0, t.n, t.thin))
            f.write(t.chains.astype("<i4").tobytes())
            f.write(t.count.astype("<u8").tobytes())
            f.write(t.values.astype("<f8").tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not a pointwise tail file" % path)
        magic, version, n_keep, n_data, capacity, n_ladders, _, _, _, n, thin = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a pointwise tail file of version %d" % (path, VERSION))
        ns = n_keep * n_data
        want = _HEAD.size + 4 * n_keep + 8 * ns + 8 * ns * capacity
        if want != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), want))
        off = _HEAD.size
        chains = np.frombuffer(raw, "<i4", n_keep, off)
        off += 4 * n_keep
        count = np.frombuffer(raw, "<u8", ns, off)
        off += 8 * ns
        values = np.frombuffer(raw, "<f8", ns * capacity, off)
        return cls(count, values, capacity, chains, n, thin, n_ladders)


def _series(n, count, values, m, S, r_eff, smooth):
    """(elpd, pareto_k, M, ratio) of one series: the module's docstring, line by line"""
    M = max(0, min(tail_length(n, r_eff), int(count) - 1))
    k_hat = math.inf
    with np.errstate(all="ignore"):
        if M == 0 or not math.isfinite(m):
            lnS = _ln([S])[0]
            return float(math.log(n) - m - lnS) if n > 0 else math.nan, k_hat, M, 1.0
        t = values[M - 1::-1][:M] - m
        c = float(values[M] - m)
        s = t
        if not (np.all(np.isfinite(t)) and math.isfinite(c)):  # an infinite term in the tail: raw, s - t has no value
            return float(math.log(n) - m - _ln([S])[0]), k_hat, M, 1.0
        if M >= MIN_TAIL and float(t[M - 1] - t[0]) >= 2.0 ** -52 / 100:
            ec = float(np.exp(np.float64(c)))
            k_hat, sigma = gpdfit(np.exp(t) - ec)
            if smooth and math.isfinite(k_hat):
                p = (np.arange(M, dtype=np.float64) + 0.5) / M
                if k_hat == 0:
                    q = -sigma * np.log1p(-p)
                else:
                    q = sigma * np.expm1(-k_hat * np.log1p(-p)) / k_hat
                s = np.minimum(0.0, np.log(q + ec))
        et, es = math.fsum(np.exp(t).tolist()), math.fsum(np.exp(s).tolist())
        num = float(n - M) + math.fsum(np.exp(s - t).tolist())
        den = S - et + es
        elpd = float(_ln([num])[0] - m - _ln([den])[0])
        ratio = float(S / den) if den != 0 else math.inf
    return elpd, k_hat, M, ratio


def psis(pointwise, tail, k=0, r_eff=1.0, smooth=True):
    """PSIS-LOO of kept chain k from a Pointwise and the PointwiseTail of the same fold: a Psis with, per datum, elpd_loo,
    pareto_k, tail_len and the cancellation ratio of the smoothed denominator (the module's docstring).  ValueError unless
    both hold the same n, kept chains and data size."""
    if int(pointwise.n[0]) != tail.n:
        raise ValueError("the fold holds %d samples, the tail %d" % (int(pointwise.n[0]), tail.n))
    if not np.array_equal(pointwise.chains, tail.chains):
        raise ValueError("the fold keeps the chains %s, the tail %s" % (pointwise.chains.tolist(), tail.chains.tolist()))
    if pointwise.n_data != tail.n_data:
        raise ValueError("the fold holds %d data, the tail %d" % (pointwise.n_data, tail.n_data))
    n, nd = tail.n, tail.n_data
    elpd, k_hat, M, ratio = np.zeros(nd), np.zeros(nd), np.zeros(nd, dtype=np.int64), np.zeros(nd)
    for i in range(nd):
        elpd[i], k_hat[i], M[i], ratio[i] = _series(n, tail.count[k, i], tail.values[k, i], float(pointwise.m_dn[k, i]),
                                                    float(pointwise.S_dn[k, i]), r_eff, smooth)
    rule = min(tail_length(n, r_eff), max(n - 1, 0))
    return Psis(n, elpd, k_hat, M, ratio, M < rule, pointwise.lppd(k), pointwise.x[k], pointwise.y[k], r_eff)


class Psis:
    """The result of psis(): per datum elpd (elpd_loo()), k (pareto_k()), tail_len, ratio and tail_short."""

    def __init__(self, n, elpd, k, tail_len, ratio, tail_short, lppd, x, y, r_eff=1.0):
        self.n = int(n)
        self.elpd, self.k, self.ratio = (np.asarray(a, dtype=np.float64) for a in (elpd, k, ratio))
        self.tail_len = np.asarray(tail_len, dtype=np.int64)
        self.tail_short = np.asarray(tail_short, dtype=bool)
        self.lppd = np.asarray(lppd, dtype=np.float64)
        self.x, self.y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        self.r_eff = float(r_eff)

    def elpd_loo(self):
        """[n_data]"""
        return self.elpd

    def pareto_k(self):
        """[n_data]"""
        return self.k

    def looic(self):
        return -2.0 * _total(self.elpd)

    def p_loo(self):
        """sum lppd - sum elpd_loo"""
        return _total(self.lppd) - _total(self.elpd)

    def se(self):
        """the standard error of sum elpd_loo: sqrt(n_data * variance of the pointwise elpd_loo)"""
        return _spread(self.elpd)

    def k_threshold(self, n=None):
        return k_threshold(self.n if n is None else n)

    def k_table(self):
        """{"good" | "bad" | "very bad": indices}: k at most the threshold; above it and at most 1; above 1 (or NaN)"""
        thr = self.k_threshold()
        with np.errstate(all="ignore"):
            good = self.k <= thr
            bad = ~good & (self.k <= 1.0)
        return {"good": np.flatnonzero(good), "bad": np.flatnonzero(bad), "very bad": np.flatnonzero(~good & ~bad)}

    def compare(self, other):
        """(difference, standard error) of the summed elpd_loo against another Psis over the same data; positive favours
        this model"""
        if self.x.tobytes() != other.x.tobytes() or self.y.tobytes() != other.y.tobytes():
            raise ValueError("the two results do not hold the same data")
        with np.errstate(all="ignore"):
            d = self.elpd - other.elpd
        return _total(d), _spread(d)

    def text(self):
        """the summary, the k table and one line per datum: `x y elpd_loo pareto_k tail_len ratio`"""
        tab = self.k_table()
        out = ["n\t%d\n" % self.n, "elpd_loo\t%s\n" % _fmt(_total(self.elpd)), "se\t%s\n" % _fmt(self.se()),
               "looic\t%s\n" % _fmt(self.looic()), "p_loo\t%s\n" % _fmt(self.p_loo()),
               "k_threshold\t%s\n" % _fmt(self.k_threshold()), "tail_short\t%d\n" % int(self.tail_short.sum())]
        for name in ("good", "bad", "very bad"):
            out.append("k %s\t%d\t%s\n" % (name, len(tab[name]), " ".join(str(i) for i in tab[name].tolist())))
        for i in range(len(self.elpd)):
            out.append("\t".join([_fmt(float(self.x[i])), _fmt(float(self.y[i])), _fmt(float(self.elpd[i])),
                                  "inf" if self.k[i] == math.inf else _fmt(float(self.k[i])), str(int(self.tail_len[i])),
                                  _fmt(float(self.ratio[i]))]) + "\n")
        return "".join(out)


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if len(argv) != 1:
        sys.stderr.write("usage: python -m apemost_amd.psis DIR   (DIR holds pointwise.bin and pointwise_tail.bin)\n")
        return 2
    try:
        pw = Pointwise.read(os.path.join(argv[0], "pointwise.bin"))
        tail = PointwiseTail.read(os.path.join(argv[0], "pointwise_tail.bin"))
        sys.stdout.write(psis(pw, tail).text())
    except (OSError, ValueError) as e:
        sys.stderr.write("psis: %s\n" % e)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
