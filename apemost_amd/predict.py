"""Posterior predictive of the built-in models: the model curve over the abscissae with its mean, spread, credible bands
and best fit, from what apemost_hip_predict_get hands out.

A Predict holds one view (include/apemost_hip.h, apemost_hip_predict_view) and the abscissae it was folded over.  A
series is one (kept chain k, abscissa i) pair with the samples v_t = curve(parameters of kept sample t of chain k, x_i);
it keeps n, origin = v_0, sum and sq (the sums of d = v - origin and of d * d), vmin, vmax and, with nbins > 0, the
counts of v over the run summary's edges of [lo, hi].  Per kept chain it keeps the best sample: best_prob, best_params
and its 1-based kept index best_n.

    mean = origin + sum / n          var = (sq - sum * sum / n) / n

A fold at the data's abscissae of a batch whose ladders differ in data length (HipSampler.batch with a list of
matrices) stays rectangular, n_x being the longest kept ladder's length, and carries `lengths` [n_keep]: kept chain k
has lengths[k] abscissae, and the entries behind them hold their initial values (sums 0, vmin +inf, vmax -inf, counts
0, x 0).  per_ladder() trims every ladder's object to its length; what it returns are ordinary Predict objects.  A
reduction over the abscissae (chi2, text, write) of the untrimmed object would take padding for data and raises
ValueError instead.

Medians and credible bands come from the counts: mean +- sd is not a credible band when the frequency posterior is
multimodal.  `curve_numpy` states the four curves in plain numpy (the operation order of apemost_amd/csrc/pt_predict.h
with numpy's sine in place of the device's).

predict.bin (little-endian), version 1:
    char[8]  "APEMOSTP"
    uint32   version, n_keep, n_x, nbins, n_par, n_ladders, model, 0
    uint64   n, thin
    double   lo, hi
    int32    chains[n_keep]
    double   x[n_keep][n_x]
    double   origin, sum, sq, vmin, vmax: [n_keep][n_x] each
    uint64   hist[n_keep][n_x][nbins]
    double   best_prob[n_keep], best_params[n_keep][n_par]
    uint64   best_n[n_keep]
"""
import math
import struct

import numpy as np

from . import capi
from .summary import edges as summary_edges
from .workloads import MODEL_PULSE, MODEL_PULSE_VROT, MODEL_SIMPLESIN, MODEL_SINE3

MAGIC = b"APEMOSTP"
VERSION = 1
MAX_BINS = 4096
PIECE = 8192            # kept steps of one launch of the device fold (pt_predict.h, kPredictPiece)
_HEAD = struct.Struct("<8s8I2Q2d")
TWO_PI = 2.0 * math.pi
SINE_RANGE = 35184372088832.0   # 2^45


def curve_numpy(model, params, x):
    """the model curve [n][n_x] of the parameter rows params [n][n_par] (or one row: [n_x]) at x, every operation in
    the order of pt_predict.h; the sine is numpy's"""
    params = np.asarray(params, dtype=np.float64)
    one = params.ndim == 1
    p = params.reshape(len(params) if not one else 1, -1)[:, :, None]
    x = np.asarray(x, dtype=np.float64).reshape(1, -1)
    with np.errstate(all="ignore"):
        if model in (MODEL_SIMPLESIN, MODEL_SINE3):
            m = np.zeros((p.shape[0], x.shape[1]))
            ok = np.ones(m.shape, dtype=bool)
            for c in range(1 if model == MODEL_SIMPLESIN else 3):
                a, f, ph = p[:, 3 * c], p[:, 3 * c + 1], p[:, 3 * c + 2]
                u = f * x + ph
                term = a * np.sin(TWO_PI * u)
                m = term if model == MODEL_SIMPLESIN else m + term
                ok &= TWO_PI * (np.abs(f) * np.abs(x) + np.abs(ph)) < SINE_RANGE
            m = m + p[:, 3 if model == MODEL_SIMPLESIN else 9]
            out = np.where(ok, m, np.nan)
        elif model == MODEL_PULSE:
            out = np.zeros((p.shape[0], x.shape[1]))
            for j in range(2, p.shape[1] - 1, 2):
                out = out + _lorentz(p[:, j + 1], p[:, j] - x, p[:, 0])
        elif model == MODEL_PULSE_VROT:
            out = np.zeros((p.shape[0], x.shape[1]))
            d = p[:, 5] - x
            out = out + _lorentz(p[:, 4], p[:, 3] - x, p[:, 0])
            out = out + _lorentz(p[:, 6], d + -p[:, 2], p[:, 0])
            out = out + _lorentz(p[:, 6], d, p[:, 0])
            out = out + _lorentz(p[:, 6], d + p[:, 2], p[:, 0])
        else:
            raise ValueError("model %r has no curve" % (model,))
    return out[0] if one else out


def _lorentz(h, d, lifetime):
    t = (TWO_PI * d) * lifetime
    return h / (1 + t * t)


class Predict:
    lengths = None   # [n_keep] abscissae per kept chain of a ragged batch's fold (see the module's docstring)

    def __init__(self, n, origin, sum, sq, vmin, vmax, hist, best_prob, best_params, best_n, chains, x, n_par, model,
                 lo=0.0, hi=0.0, thin=1, n_ladders=1):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.chains = np.ascontiguousarray(chains, dtype=np.int32).reshape(-1)
        self.n_keep = len(self.chains)
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.n_keep, -1)
        self.n_x = self.x.shape[1]
        shape = (self.n_keep, self.n_x)
        for name, a in (("origin", origin), ("sum", sum), ("sq", sq), ("vmin", vmin), ("vmax", vmax)):
            setattr(self, name, np.ascontiguousarray(a, dtype=np.float64).reshape(shape))
        self.hist = np.ascontiguousarray(hist, dtype=np.uint64).reshape(shape + (-1,))
        self.nbins = self.hist.shape[2]
        self.n_par, self.model = int(n_par), int(model)
        self.best_prob = np.ascontiguousarray(best_prob, dtype=np.float64).reshape(self.n_keep)
        self.best_params = np.ascontiguousarray(best_params, dtype=np.float64).reshape(self.n_keep, self.n_par)
        self.best_n = np.ascontiguousarray(best_n, dtype=np.uint64).reshape(self.n_keep)
        self.lo, self.hi, self.thin, self.n_ladders = float(lo), float(hi), int(thin), int(n_ladders)

    @classmethod
    def empty(cls, chains, x, n_par, model, nbins=0, lo=0.0, hi=0.0, thin=1, n_ladders=1):
        k = len(chains)
        x = np.asarray(x, dtype=np.float64)
        x = np.tile(x, (k, 1)) if x.ndim == 1 else x
        z = np.zeros(x.shape)
        return cls(np.zeros(1, dtype=np.uint64), z, z.copy(), z.copy(), np.full(x.shape, np.inf),
                   np.full(x.shape, -np.inf), np.zeros(x.shape + (int(nbins),), dtype=np.uint64), np.full(k, -np.inf),
                   np.zeros((k, n_par)), np.zeros(k, dtype=np.uint64), chains, x, n_par, model, lo, hi, thin, n_ladders)

    def view(self):
        """the apemost_hip_predict_view over this object's arrays"""
        dp, up = capi._dp, capi._up
        return capi.PredictView(n=self.n.ctypes.data_as(up), origin=self.origin.ctypes.data_as(dp),
                                sum=self.sum.ctypes.data_as(dp), sq=self.sq.ctypes.data_as(dp),
                                vmin=self.vmin.ctypes.data_as(dp), vmax=self.vmax.ctypes.data_as(dp),
                                hist=self.hist.ctypes.data_as(up) if self.nbins else None,
                                best_prob=self.best_prob.ctypes.data_as(dp),
                                best_params=self.best_params.ctypes.data_as(dp), best_n=self.best_n.ctypes.data_as(up))

    def is_ragged(self):
        """the kept chains differ in length: entries behind lengths[k] are padding"""
        return self.lengths is not None and bool(np.any(np.asarray(self.lengths) != self.n_x))

    def _no_padding(self, what):
        if self.is_ragged():
            raise ValueError("%s over a ragged batch's fold would take padding for data (lengths %s of n_x %d): "
                             "use per_ladder(), which trims every ladder to its length"
                             % (what, np.asarray(self.lengths).tolist(), self.n_x))

    def per_ladder(self, n_ladders=None):
        """one Predict per ladder of a batch: the kept chains, ladder-major, in equal shares; of a ragged batch's fold
        each trimmed to its ladder's length (the kept chains of one ladder share it)"""
        n_ladders = self.n_ladders if n_ladders is None else n_ladders
        if n_ladders < 1 or self.n_keep % n_ladders:
            raise ValueError("%d kept chains are not %d equal ladders" % (self.n_keep, n_ladders))
        per = self.n_keep // n_ladders
        out = []
        for b in range(n_ladders):
            k = slice(b * per, (b + 1) * per)
            m = self.n_x
            if self.lengths is not None:
                mine = np.asarray(self.lengths)[k]
                if np.any(mine != mine[0]):
                    raise ValueError("ladder %d: its kept chains have lengths %s" % (b, mine.tolist()))
                m = int(mine[0])
            out.append(Predict(self.n.copy(), self.origin[k, :m], self.sum[k, :m], self.sq[k, :m], self.vmin[k, :m],
                               self.vmax[k, :m], self.hist[k, :m], self.best_prob[k], self.best_params[k], self.best_n[k],
                               self.chains[k], self.x[k, :m], self.n_par, self.model, self.lo, self.hi, self.thin, 1))
        return out

    # -- what it gives ------------------------------------------------------------------------
    def mean(self, k=0):
        """[n_x]: origin + sum / n"""
        with np.errstate(all="ignore"):
            return self.origin[k] + self.sum[k] / np.float64(self.n[0])

    def var(self, k=0):
        """[n_x]: the variance about the mean (divided by n), (sq - sum * sum / n) / n, never below 0"""
        n = np.float64(self.n[0])
        with np.errstate(all="ignore"):
            v = (self.sq[k] - self.sum[k] * self.sum[k] / n) / n
            return np.where(v < 0, 0.0, v)

    def sd(self, k=0):
        with np.errstate(all="ignore"):
            return np.sqrt(self.var(k))

    def edges(self):
        return summary_edges(self.lo, self.hi, self.nbins)

    def quantile(self, q, k=0):
        """[n_x]: the q-quantile (0 <= q <= 1) of the counted values of every abscissa, linear inside its bin: with
        N counted values and C_b of them below bin b, the value at rank q N is e[b] + (q N - C_b) / count_b *
        (e[b+1] - e[b]) for the first bin whose cumulative count reaches q N.  NaN where nothing was counted."""
        if self.nbins < 1:
            raise ValueError("no histograms: predict_begin(nbins=...)")
        if not 0 <= q <= 1:
            raise ValueError("quantile %r outside [0, 1]" % (q,))
        e = self.edges()
        out = np.full(self.n_x, np.nan)
        for i in range(self.n_x):
            c = self.hist[k, i].astype(np.float64)
            cum = np.cumsum(c)
            total = cum[-1]
            if total == 0:
                continue
            want = q * total
            b = int(np.searchsorted(cum, want, side="left"))
            while c[b] == 0:        # (want == 0 with empty leading bins)
                b += 1
            below = cum[b] - c[b]
            out[i] = e[b] + (want - below) / c[b] * (e[b + 1] - e[b])
        return out

    def median(self, k=0):
        return self.quantile(0.5, k)

    def band(self, level=0.68, k=0):
        """(lower, upper): the central credible band of the given level, the quantiles (1 -+ level) / 2"""
        if not 0 < level < 1:
            raise ValueError("level %r outside (0, 1)" % (level,))
        return self.quantile((1 - level) / 2, k), self.quantile((1 + level) / 2, k)

    def counted(self, k=0):
        """[n_x]: values inside the histogram range (the rest of n fell outside or were NaN)"""
        return self.hist[k].sum(axis=1)

    def best_curve(self, sampler=None, k=0):
        """[n_x]: the curve of the best sample of kept chain k over this fold's abscissae: on the device through
        sampler.predict_curve, or by curve_numpy without a sampler"""
        if sampler is None:
            return curve_numpy(self.model, self.best_params[k], self.x[k])
        return sampler.predict_curve(self.best_params[k], self.x[k])

    def default_kind(self):
        return "ratio" if self.model in (MODEL_PULSE, MODEL_PULSE_VROT) else "difference"

    def residuals(self, y, kind=None, k=0):
        """[n_x]: y - mean ("difference": the sine models, what prewhitening works on) or y / mean ("ratio": a power
        spectrum over its limit spectrum); the default follows the model"""
        kind = self.default_kind() if kind is None else kind
        y = np.asarray(y, dtype=np.float64)
        with np.errstate(all="ignore"):
            if kind == "difference":
                return y - self.mean(k)
            if kind == "ratio":
                return y / self.mean(k)
        raise ValueError("kind %r: difference or ratio" % (kind,))

    def chi2(self, y, sigma, k=0):
        """sum ((y - mean) / sigma)^2 over the abscissae"""
        self._no_padding("chi2")
        r = (np.asarray(y, dtype=np.float64) - self.mean(k)) / sigma
        return float(np.sum(r * r))

    def text(self, y, best=None, k=0):
        """predict.txt: one line per abscissa, `x y mean sd residual min max best` (and `median lower68 upper68` with
        histograms), tab separated, "%.15e".  y: data column 1; best: the best-fit curve (default: curve_numpy)."""
        self._no_padding("text")
        best = self.best_curve(None, k) if best is None else best
        cols = [self.x[k], np.asarray(y, dtype=np.float64), self.mean(k), self.sd(k), self.residuals(y, None, k),
                self.vmin[k], self.vmax[k], np.asarray(best, dtype=np.float64)]
        if self.nbins:
            cols += [self.median(k)] + list(self.band(0.68, k))
        return "".join("\t".join(_fmt(float(c[i])) for c in cols) + "\n" for i in range(self.n_x))

    # -- predict.bin ----------------------------------------------------------------------------
    def _arrays(self):
        return ((self.chains, "<i4"), (self.x, "<f8"), (self.origin, "<f8"), (self.sum, "<f8"), (self.sq, "<f8"),
                (self.vmin, "<f8"), (self.vmax, "<f8"), (self.hist, "<u8"), (self.best_prob, "<f8"),
                (self.best_params, "<f8"), (self.best_n, "<u8"))

    def write(self, path):
        self._no_padding("write")
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_keep, self.n_x, self.nbins, self.n_par, self.n_ladders, self.model,
                               0, int(self.n[0]), self.thin, self.lo, self.hi))
            for a, t in self._arrays():
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not a predict file" % path)
        magic, version, n_keep, n_x, nbins, n_par, n_ladders, model, _, n, thin, lo, hi = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a predict file of version %d" % (path, VERSION))
        ns = n_keep * n_x
        want = _HEAD.size + 4 * n_keep + 8 * (6 * ns + ns * nbins + n_keep * (2 + n_par))
        if want != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), want))
        off = _HEAD.size

        def take(count, dtype):
            nonlocal off
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=off)
            off += a.itemsize * count
            return a.copy()
        chains, x = take(n_keep, "<i4"), take(ns, "<f8")
        origin, total, sq, vmin, vmax = (take(ns, "<f8") for _ in range(5))
        hist = take(ns * nbins, "<u8").reshape(n_keep, n_x, nbins)
        best_prob, best_params, best_n = take(n_keep, "<f8"), take(n_keep * n_par, "<f8"), take(n_keep, "<u8")
        return cls([n], origin, total, sq, vmin, vmax, hist, best_prob, best_params, best_n, chains, x, n_par, model,
                   lo, hi, thin, n_ladders)


def _fmt(v):
    return "nan" if v != v else "%.15e" % v
