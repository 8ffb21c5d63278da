"""The residual periodogram under the posterior, from what apemost_hip_periodogram_get hands out: what is left in the
residuals of a sine model, at which frequency, how strong, and with what posterior probability?

For every kept sample theta_t of a kept chain and every frequency nu_j of a grid the device takes, with r_i = y_i -
m(x_i; theta_t) (the operation order is in apemost_amd/csrc/pt_periodogram.h):

    C_j = sum_i r_i cos(2 pi nu_j x_i)      S_j = sum_i r_i sin(2 pi nu_j x_i)
    P_j = wcc C^2 + wcs C S + wss S^2

The weights are host policy and are fixed at begin (weights() below).  With G = [[sum c^2, sum c s], [sum c s, sum s^2]]
the Gram matrix of the two columns at one frequency and b = (C, S):

    "lomb_scargle"   b' G^-1 b / (2 sigma^2): half the reduction in chi^2 of the least-squares sinusoid at nu_j, the
                     generalised Lomb-Scargle power.  Exp(1) under Gaussian white noise of known sigma.
    "schuster"       (C^2 + S^2) / (L sigma^2): the classical periodogram.
    "amplitude2"     b' G^-2 b: the squared amplitude of the least-squares sinusoid.

A singular G (nu = 0, or a grid on which the two columns are proportional) has no inverse: its weights are zero, and so
is P there, for "lomb_scargle" and "amplitude2".

A Periodogram holds one view (include/apemost_hip.h, apemost_hip_periodogram_view).  Per kept chain k, [n_freq] arrays:

    mean = origin + sum / n     var = (sq - sum^2 / n) / (n - 1), never below 0     sd, min, max
    coherent         the power of the posterior MEAN residual, from sum_c / n and sum_s / n through the same weights
                     (C and S are linear in r): what all samples agree on.  mean - coherent is what the posterior's
                     spread adds.
    exceed_fraction  the share of samples with P above the kept chain's level
    peak_hist        how often each frequency held the highest peak of a sample (the first of equal ones)
    peak_frequency   the mode of peak_hist and its share;  peak_mean, peak_sd: the moments of the highest peak

The arrays are rectangular in the frequencies, which every kept chain shares; `lengths` are the data each kept chain's
ladder really has (they differ in a ragged batch), which nothing here pads.  per_ladder() splits a batch's fold.

periodogram.bin (little-endian), version 1:
    char[8]  "APEMOSTG"
    uint32   version, n_keep, n_freq, n_ladders, model, 0, 0, 0
    uint64   n, thin
    double   sigma
    int32    chains[n_keep], lengths[n_keep]
    double   freqs[n_freq], weights[n_keep][n_freq][3], level[n_keep]
    double   origin, sum, sq, pmin, pmax, sum_c, sum_s: [n_keep][n_freq] each
    uint64   exceed[n_keep][n_freq]
    double   peak_origin, peak_sum, peak_sq, peak_min, peak_max: [n_keep] each
    uint64   peak_counts[n_keep][n_freq + 1]
"""
import struct

import numpy as np

from . import capi

MAGIC = b"APEMOSTG"
VERSION = 1
PIECE = 512          # kept steps of one launch at most (APEMOST_PERIODOGRAM_PIECE)
SIDE = 8             # kept samples a wave of the hot kernel holds side by side
MAX_FREQ = 1 << 20
KINDS = ("lomb_scargle", "schuster", "amplitude2")
STATE = ("origin", "sum", "sq", "pmin", "pmax", "sum_c", "sum_s")
PEAK_STATE = ("peak_origin", "peak_sum", "peak_sq", "peak_min", "peak_max")
_HEAD = struct.Struct("<8s8I2Qd")
SINGULAR = 1e-10     # G counts as singular where det G <= SINGULAR * (trace G / 2)^2 (trace G = L: a vanishing column too)


def weights(x, freqs, kind="lomb_scargle", sigma=1.0):
    """[n_freq][3] = (wcc, wcs, wss) of the quadratic form P = wcc C^2 + wcs C S + wss S^2 over the abscissae x [L] (host
    arithmetic, numpy's own cos and sin); kind and sigma as in the module's docstring.  Where the Gram matrix of a
    frequency is singular (nu = 0, for one) "lomb_scargle" and "amplitude2" give weights of zero."""
    if kind not in KINDS:
        raise ValueError("kind %r: one of %s" % (kind, ", ".join(KINDS)))
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    freqs = np.asarray(freqs, dtype=np.float64).reshape(-1)
    sigma = float(sigma)
    if not sigma > 0:
        raise ValueError("sigma %r: positive" % (sigma,))
    out = np.zeros((len(freqs), 3))
    if kind == "schuster":
        out[:, 0] = out[:, 2] = 1.0 / (len(x) * sigma * sigma)
        return out
    step = max(1, (1 << 22) // max(len(x), 1))
    for j0 in range(0, len(freqs), step):
        arg = 2.0 * np.pi * np.outer(freqs[j0:j0 + step], x)
        c, s = np.cos(arg), np.sin(arg)
        cc, cs, ss = (c * c).sum(1), (c * s).sum(1), (s * s).sum(1)
        det = cc * ss - cs * cs
        ok = det > SINGULAR * (0.5 * (cc + ss)) ** 2
        with np.errstate(all="ignore"):
            a, b, d = ss / det, -cs / det, cc / det          # G^-1 = [[a, b], [b, d]]
        if kind == "lomb_scargle":
            w = np.stack([a, 2.0 * b, d], 1) / (2.0 * sigma * sigma)
        else:
            w = np.stack([a * a + b * b, 2.0 * b * (a + d), b * b + d * d], 1)
        out[j0:j0 + step] = np.where(ok[:, None], w, 0.0)
    return out


def power(w, C, S):
    """the quadratic form in the device's association, elementwise: ((wcc C) C + (wcs C) S) + (wss S) S"""
    w = np.asarray(w, dtype=np.float64)
    with np.errstate(all="ignore"):
        return ((w[..., 0] * C) * C + (w[..., 1] * C) * S) + (w[..., 2] * S) * S


class Periodogram:
    """The state of one fold of the residual periodogram and what it says (the formulas are in the module's docstring)."""

    def __init__(self, n, origin, sum, sq, pmin, pmax, sum_c, sum_s, exceed, peak_origin, peak_sum, peak_sq, peak_min,
                 peak_max, peak_counts, chains, freqs, weights, level, lengths, model=0, sigma=0.5, thin=1, n_ladders=1):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.chains = np.ascontiguousarray(chains, dtype=np.int32).reshape(-1)
        self.n_keep = len(self.chains)
        self.freqs = np.ascontiguousarray(freqs, dtype=np.float64).reshape(-1)
        self.n_freq = len(self.freqs)
        shape = (self.n_keep, self.n_freq)
        for name, a in zip(STATE, (origin, sum, sq, pmin, pmax, sum_c, sum_s)):
            setattr(self, name, np.ascontiguousarray(a, dtype=np.float64).reshape(shape))
        self.exceed = np.ascontiguousarray(exceed, dtype=np.uint64).reshape(shape)
        for name, a in zip(PEAK_STATE, (peak_origin, peak_sum, peak_sq, peak_min, peak_max)):
            setattr(self, name, np.ascontiguousarray(a, dtype=np.float64).reshape(self.n_keep))
        self.peak_counts = np.ascontiguousarray(peak_counts, dtype=np.uint64).reshape(self.n_keep, self.n_freq + 1)
        self.weights = np.ascontiguousarray(weights, dtype=np.float64).reshape(self.n_keep, self.n_freq, 3)
        self.level = np.ascontiguousarray(level, dtype=np.float64).reshape(self.n_keep)
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(self.n_keep)
        self.model, self.sigma, self.thin, self.n_ladders = int(model), float(sigma), int(thin), int(n_ladders)

    @classmethod
    def empty(cls, chains, freqs, weights, level, lengths, model=0, sigma=0.5, thin=1, n_ladders=1):
        k, f = len(chains), len(freqs)
        z = [np.zeros((k, f)) for _ in STATE]
        return cls(np.zeros(1, dtype=np.uint64), *z, np.zeros((k, f), dtype=np.uint64), *[np.zeros(k) for _ in PEAK_STATE],
                   np.zeros((k, f + 1), dtype=np.uint64), chains, freqs, weights, level, lengths, model, sigma, thin, n_ladders)

    def view(self):
        """the apemost_hip_periodogram_view over this object's arrays"""
        dp = capi._dp
        return capi.PeriodogramView(n=self.n.ctypes.data_as(capi._up), exceed=self.exceed.ctypes.data_as(capi._up),
                                    peak_counts=self.peak_counts.ctypes.data_as(capi._up),
                                    **{f: getattr(self, f).ctypes.data_as(dp) for f in STATE + PEAK_STATE})

    def _pick(self, k):
        return Periodogram(self.n.copy(), *[getattr(self, f)[k] for f in STATE], self.exceed[k],
                           *[getattr(self, f)[k] for f in PEAK_STATE], self.peak_counts[k], self.chains[k], self.freqs,
                           self.weights[k], self.level[k], self.lengths[k], self.model, self.sigma, self.thin, 1)

    def per_ladder(self, n_ladders=None):
        """one Periodogram per ladder of a batch: the kept chains, ladder-major, in equal shares"""
        n_ladders = self.n_ladders if n_ladders is None else n_ladders
        if n_ladders < 1 or self.n_keep % n_ladders:
            raise ValueError("%d kept chains are not %d equal ladders" % (self.n_keep, n_ladders))
        per = self.n_keep // n_ladders
        return [self._pick(slice(b * per, (b + 1) * per)) for b in range(n_ladders)]

    @staticmethod
    def concat(shards):
        """the Periodogram of a sharded ladder's folds: the kept chains of every shard one after the other, in shard order
        (the chain indices stay the shards' local ones); the shards share the grid and the count of samples"""
        s0 = shards[0]
        assert all(int(s.n[0]) == int(s0.n[0]) and s.freqs.tobytes() == s0.freqs.tobytes() and s.thin == s0.thin
                   for s in shards)
        cat = np.concatenate
        return Periodogram(s0.n.copy(), *[cat([getattr(s, f) for s in shards]) for f in STATE], cat([s.exceed for s in shards]),
                           *[cat([getattr(s, f) for s in shards]) for f in PEAK_STATE], cat([s.peak_counts for s in shards]),
                           cat([s.chains for s in shards]), s0.freqs, cat([s.weights for s in shards]),
                           cat([s.level for s in shards]), cat([s.lengths for s in shards]), s0.model, s0.sigma, s0.thin,
                           s0.n_ladders)

    # -- per frequency ------------------------------------------------------------------------
    def _n(self):
        return np.float64(self.n[0])

    def mean(self, k=0):
        """[n_freq]: origin + sum / n, the posterior mean of P"""
        with np.errstate(all="ignore"):
            return self.origin[k] + self.sum[k] / self._n()

    def var(self, k=0):
        """[n_freq]: (sq - sum * sum / n) / (n - 1), never below 0"""
        n = self._n()
        with np.errstate(all="ignore"):
            v = (self.sq[k] - self.sum[k] * self.sum[k] / n) / (n - np.float64(1.0))
            return np.where(v < 0, 0.0, v)

    def sd(self, k=0):
        with np.errstate(all="ignore"):
            return np.sqrt(self.var(k))

    def min(self, k=0):
        return self.pmin[k].copy()

    def max(self, k=0):
        return self.pmax[k].copy()

    def coherent(self, k=0):
        """[n_freq]: the power of the mean residual, from sum_c / n and sum_s / n through the kept chain's weights"""
        with np.errstate(all="ignore"):
            return power(self.weights[k], self.sum_c[k] / self._n(), self.sum_s[k] / self._n())

    def exceed_fraction(self, k=0):
        """[n_freq]: the share of kept samples whose P lies above level[k]"""
        with np.errstate(all="ignore"):
            return self.exceed[k].astype(np.float64) / self._n()

    # -- the highest peak ---------------------------------------------------------------------
    def peak_hist(self, k=0):
        """[n_freq]: how many kept samples had their highest peak at each frequency"""
        return self.peak_counts[k, :self.n_freq].copy()

    def n_no_peak(self, k=0):
        """kept samples without a P above -inf"""
        return int(self.peak_counts[k, self.n_freq])

    def peak_frequency(self, k=0):
        """(frequency, share): the frequency that most often held a sample's highest peak (the first of equal counts) and
        the share of the kept samples it held it for; (NaN, 0) before there is a peak"""
        h = self.peak_hist(k)
        if int(h.sum()) == 0:
            return float("nan"), 0.0
        j = int(np.argmax(h))
        return float(self.freqs[j]), float(h[j]) / float(self._n())

    def peak_mean(self, k=0):
        with np.errstate(all="ignore"):
            return float(self.peak_origin[k] + self.peak_sum[k] / self._n())

    def peak_sd(self, k=0):
        n = self._n()
        with np.errstate(all="ignore"):
            v = (self.peak_sq[k] - self.peak_sum[k] * self.peak_sum[k] / n) / (n - np.float64(1.0))
            return float(np.sqrt(v if v > 0 else 0.0)) if v == v else float("nan")

    # -- text ---------------------------------------------------------------------------------
    def text(self, k=0):
        """periodogram.txt: one line per frequency, `nu mean sd min max coherent peak_share`, tab separated, %.15e"""
        with np.errstate(all="ignore"):
            share = self.peak_hist(k).astype(np.float64) / self._n()
        cols = [self.freqs, self.mean(k), self.sd(k), self.pmin[k], self.pmax[k], self.coherent(k), share]
        return "".join("\t".join(_fmt(float(c[j])) for c in cols) + "\n" for j in range(self.n_freq))

    # -- periodogram.bin ----------------------------------------------------------------------
    def _arrays(self):
        return ([(self.chains, "<i4"), (self.lengths, "<i4"), (self.freqs, "<f8"), (self.weights, "<f8"), (self.level, "<f8")] +
                [(getattr(self, f), "<f8") for f in STATE] + [(self.exceed, "<u8")] +
                [(getattr(self, f), "<f8") for f in PEAK_STATE] + [(self.peak_counts, "<u8")])

    def write(self, path):
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_keep, self.n_freq, self.n_ladders, self.model, 0, 0, 0, int(self.n[0]),
                               self.thin, self.sigma))
            for a, t in self._arrays():
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not a periodogram file" % path)
        magic, version, n_keep, n_freq, n_ladders, model, _, _, _, n, thin, sigma = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a periodogram file of version %d" % (path, VERSION))
        ns = n_keep * n_freq
        want = _HEAD.size + 8 * n_keep + 8 * (n_freq + 3 * ns + n_keep + 7 * ns + ns + 5 * n_keep + n_keep * (n_freq + 1))
        if want != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), want))
        off = _HEAD.size

        def take(count, dtype):
            nonlocal off
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=off)
            off += a.itemsize * count
            return a.copy()
        chains, lengths = take(n_keep, "<i4"), take(n_keep, "<i4")
        freqs, w, level = take(n_freq, "<f8"), take(3 * ns, "<f8"), take(n_keep, "<f8")
        state = [take(ns, "<f8") for _ in STATE]
        exceed = take(ns, "<u8")
        peak = [take(n_keep, "<f8") for _ in PEAK_STATE]
        counts = take(n_keep * (n_freq + 1), "<u8")
        return cls([n], *state, exceed, *peak, counts, chains, freqs, w, level, lengths, model, sigma, thin, n_ladders)


def _fmt(v):
    return "nan" if v != v else "%.15e" % v
