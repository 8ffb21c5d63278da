"""Information criteria from the pointwise log-likelihood: WAIC, importance-sampling leave-one-out and DIC, from what
apemost_hip_pointwise_get hands out.

A Pointwise holds one view (include/apemost_hip.h, apemost_hip_pointwise_view), the data it was folded over, the
sampler's sigma and `at_mean`.  A series is one (kept chain k, datum i) pair with the samples l_t = the log-likelihood
term of datum i under kept sample t of chain k; it keeps n, origin = l_0, sum and sq (the sums of d = l - origin and of
d * d), the running log-sum-exp of l (m_up, S_up) and of -l (m_dn, S_dn) with the sum of the squared exponentials of the
latter (S2_dn).  Per kept chain it keeps par_origin and par_sum, which give the posterior mean parameters.  at_mean is
l_i at those mean parameters: HipSampler.pointwise() fills it with one pointwise_loglike call; it is not part of the
device state, and NaN where nobody filled it.

Per datum i (all of these return [n_data] arrays; the criteria are their sums):

    mean_loglike = origin + sum / n              var_loglike = (sq - sum * sum / n) / (n - 1), never below 0
    lppd         = m_up + ln(S_up / n)           the log of the mean likelihood of the datum
    p_waic 1     = 2 (lppd - mean_loglike)       p_waic 2 = var_loglike
    elpd_waic    = lppd - p_waic                 waic = -2 sum elpd_waic
    elpd_loo     = -(m_dn + ln(S_dn / n))        the log of the harmonic mean: plain importance-sampling leave-one-out
    looic        = -2 sum elpd_loo               p_loo = sum lppd - sum elpd_loo
    loo_ess      = S_dn^2 / S2_dn                the effective sample size of the leave-one-out weights, between 1 and n
    p_dic        = 2 (sum at_mean - sum mean_loglike)      dic = -2 sum at_mean + 2 p_dic

The standard errors (waic_se, compare) are sqrt(n_data * variance over the data of the pointwise values), the variance
divided by n_data - 1: the standard error of the summed elpd; that of waic = -2 elpd is twice it.  elpd_loo here is
plain importance sampling; loo_ess says where it collapses -- towards 1, one sample carries the leave-one-out estimate
of that datum and elpd_loo is not to be trusted there (loo_unreliable).  Pareto smoothing of the weights, with the
Pareto k of every datum as the diagnostic, is apemost_amd/psis.py: it takes this object and the fold's tail
(HipSampler.pointwise_begin(tail=...), pointwise_tail()), the sorted largest weights per datum kept on the device.

Keep in mind:
  * The criteria mean what they say for a chain at beta = 1, which is chain 0 and the default: a tempered chain samples
    another distribution than the posterior.
  * The mean of a circular parameter (a phase) is the user's responsibility: par_mean is the plain arithmetic mean of the
    samples as they are stored, and DIC evaluates the model there.
  * For the sine models the constant -ln(sigma sqrt(2 pi)) of a normal density is left out of every term, as the
    reference's likelihood leaves it out: every criterion's elpd is shifted by that amount per datum, differences
    between models fitted with the same sigma are not.  For the pulse models the term is -(ln v + y / v); the
    parameter-1 offset that the reference adds to the sum is not a datum's term and is left out.

A fold over a batch whose ladders differ in data length (HipSampler.batch with a list of matrices) stays rectangular,
n_data being the longest kept ladder's length, and carries `lengths` [n_keep]: kept chain k has lengths[k] data, and
the entries behind them hold their initial values, 0 (at_mean: NaN).  per_ladder() trims every ladder's object to its
length; what it returns are ordinary Pointwise objects.  A reduction over the data of the untrimmed object (lppd,
elpd_*, waic*, looic, p_*, dic, compare, criteria, text, write) would take padding for data and raises ValueError
instead.

A fold begun at the caller's data (HipSampler.pointwise_begin(at=...), apemost_hip_pointwise_begin_at) scores the kept
chains on data the sampler was not fitted to: the object is the same, with `heldout` set, x and y the caller's, and
`lengths` where the kept chains' blocks differ in length.  lppd is then the held-out log predictive density of every
datum (apemost_amd/kfold.py turns it into K-fold cross-validation); the _dn words (elpd_loo, loo_ess) are still folded
and mean nothing there, at_mean stays NaN, and dic and p_dic raise ValueError.

`loglike_numpy` states the term in plain numpy (the operation order of apemost_amd/csrc/pt_pointwise.h on
predict.curve_numpy's curve, with numpy's sine and logarithm in place of the device's).

pointwise.bin (little-endian), version 1:
    char[8]  "APEMOSTW"
    uint32   version, n_keep, n_data, n_par, n_ladders, model, 0, 0
    uint64   n, thin
    double   sigma
    int32    chains[n_keep]
    double   x, y: [n_keep][n_data] each
    double   origin, sum, sq, m_up, S_up, m_dn, S_dn, S2_dn: [n_keep][n_data] each
    double   par_origin, par_sum: [n_keep][n_par] each
    double   at_mean[n_keep][n_data]
"""
import math
import struct

import numpy as np

from . import capi
from .predict import curve_numpy
from .workloads import MODEL_PULSE, MODEL_PULSE_VROT, MODEL_SIMPLESIN, MODEL_SINE3

MAGIC = b"APEMOSTW"
VERSION = 1
PIECE = 8192            # kept steps of one launch of the device fold (pt_pointwise.h, kPointwisePiece)
_HEAD = struct.Struct("<8s8I2Qd")
STATE = ("origin", "sum", "sq", "m_up", "S_up", "m_dn", "S_dn", "S2_dn")
CRITERIA = ("n", "lppd", "p_waic1", "p_waic2", "elpd_waic", "waic", "waic_se", "elpd_loo", "looic", "p_loo", "dic",
            "p_dic")


def sine_constant(sigma):
    """c of the sine models' term l = (v - y)^2 * c: 1.0 / ((-2.0 * sigma) * sigma), every operation rounded once"""
    sigma = np.float64(sigma)
    with np.errstate(all="ignore"):
        return np.float64(1.0) / ((np.float64(-2.0) * sigma) * sigma)


def loglike_numpy(model, rows, data, sigma=0.5, hmin=1e-6):
    """the pointwise log-likelihood [n][n_data] of the parameter rows [n][n_par] (or one row: [n_data]) over the data
    [n_data][>= 2] (columns 0 and 1), every operation in the order of pt_pointwise.h; sine and logarithm are numpy's.
    hmin belongs to the pulse models' prior and does not enter a datum's term: it is accepted so that a workload's
    settings can be passed as they are."""
    del hmin
    data = np.asarray(data, dtype=np.float64)
    v = curve_numpy(model, rows, data[:, 0])
    y = data[:, 1]
    with np.errstate(all="ignore"):
        if model in (MODEL_SIMPLESIN, MODEL_SINE3):
            r = v - y
            q = r * r
            return q * sine_constant(sigma)
        if model in (MODEL_PULSE, MODEL_PULSE_VROT):
            return -(np.log(v) + y / v)
    raise ValueError("model %r has no datum's term" % (model,))


def _ln(a):
    """elementwise natural logarithm by the C library's log (what the C host calls): NaN below 0 and for NaN"""
    out = np.empty(len(a))
    for i, v in enumerate(np.asarray(a, dtype=np.float64).tolist()):
        if v != v or v < 0:
            out[i] = math.nan
        elif v == 0:
            out[i] = -math.inf
        elif v == math.inf:
            out[i] = math.inf
        else:
            out[i] = math.log(v)
    return out


def _total(a):
    """the sum in index order from 0.0, as a C loop adds"""
    t = 0.0
    for v in np.asarray(a, dtype=np.float64).tolist():
        t = t + v
    return t


def _spread(a):
    """sqrt(n * variance) of the values a, the variance about their mean divided by n - 1 (NaN for one value)"""
    a = np.asarray(a, dtype=np.float64)
    n = np.float64(len(a))
    with np.errstate(all="ignore"):
        mean = np.float64(_total(a)) / n
        d = a - mean
        var = np.float64(_total(d * d)) / (n - np.float64(1.0))
        return float(np.sqrt(n * var))


class Pointwise:
    """The state of one pointwise fold and the information criteria it gives (the formulas are in the module's
    docstring).

    * The criteria mean what they say for a chain at beta = 1, which is chain 0 and the default: a tempered chain
      samples another distribution than the posterior.
    * The mean of a circular parameter (a phase) is the user's responsibility: par_mean is the plain arithmetic mean of
      the samples as they are stored, and DIC (at_mean, dic, p_dic) evaluates the model there.
    * For the sine models the constant -ln(sigma sqrt(2 pi)) of a normal density is left out of every term, as the
      reference's likelihood leaves it out: every elpd is shifted by that amount per datum, the same for every model
      fitted with the same sigma.  For the pulse models the term is -(ln v + y / v); the parameter-1 offset that the
      reference adds to the sum is not a datum's term and is left out.
    * at_mean is filled by HipSampler.pointwise() on the device (pointwise_loglike, in a batch over the kept chain's
      own ladder's data); it is NaN where nobody filled it, and dic and p_dic with it."""

    lengths = None   # [n_keep] data per kept chain of a ragged batch's fold (see the module's docstring)
    heldout = False  # the fold was begun at the caller's data (HipSampler.pointwise_begin(at=...)): x and y are those,
    #                  lppd is the held-out log predictive density (apemost_amd/kfold.py), the _dn words (elpd_loo,
    #                  loo_ess) mean nothing, and DIC has no held-out meaning: at_mean stays NaN, dic and p_dic raise

    def __init__(self, n, origin, sum, sq, m_up, S_up, m_dn, S_dn, S2_dn, par_origin, par_sum, chains, x, y, n_par, model,
                 sigma=0.5, thin=1, n_ladders=1, at_mean=None):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.chains = np.ascontiguousarray(chains, dtype=np.int32).reshape(-1)
        self.n_keep = len(self.chains)
        self.x = np.ascontiguousarray(x, dtype=np.float64).reshape(self.n_keep, -1)
        self.n_data = self.x.shape[1]
        shape = (self.n_keep, self.n_data)
        self.y = np.ascontiguousarray(y, dtype=np.float64).reshape(shape)
        for name, a in zip(STATE, (origin, sum, sq, m_up, S_up, m_dn, S_dn, S2_dn)):
            setattr(self, name, np.ascontiguousarray(a, dtype=np.float64).reshape(shape))
        self.n_par, self.model = int(n_par), int(model)
        self.par_origin = np.ascontiguousarray(par_origin, dtype=np.float64).reshape(self.n_keep, self.n_par)
        self.par_sum = np.ascontiguousarray(par_sum, dtype=np.float64).reshape(self.n_keep, self.n_par)
        self.sigma, self.thin, self.n_ladders = float(sigma), int(thin), int(n_ladders)
        self.at_mean = (np.full(shape, np.nan) if at_mean is None
                        else np.ascontiguousarray(at_mean, dtype=np.float64).reshape(shape).copy())

    @classmethod
    def empty(cls, chains, x, y, n_par, model, sigma=0.5, thin=1, n_ladders=1):
        k = len(chains)
        x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
        x = np.tile(x, (k, 1)) if x.ndim == 1 else x
        y = np.tile(y, (k, 1)) if y.ndim == 1 else y
        z = [np.zeros(x.shape) for _ in STATE]
        return cls(np.zeros(1, dtype=np.uint64), *z, np.zeros((k, n_par)), np.zeros((k, n_par)), chains, x, y, n_par,
                   model, sigma, thin, n_ladders)

    def view(self):
        """the apemost_hip_pointwise_view over this object's arrays"""
        dp = capi._dp
        return capi.PointwiseView(n=self.n.ctypes.data_as(capi._up), par_origin=self.par_origin.ctypes.data_as(dp),
                                  par_sum=self.par_sum.ctypes.data_as(dp),
                                  **{f: getattr(self, f).ctypes.data_as(dp) for f in STATE})

    def is_ragged(self):
        """the kept chains differ in length: entries behind lengths[k] are padding"""
        return self.lengths is not None and bool(np.any(np.asarray(self.lengths) != self.n_data))

    def _no_padding(self, what):
        if self.is_ragged():
            raise ValueError("%s over a ragged batch's fold would take padding for data (lengths %s of n_data %d): "
                             "use per_ladder(), which trims every ladder to its length"
                             % (what, np.asarray(self.lengths).tolist(), self.n_data))

    def _not_heldout(self, what):
        if self.heldout:
            raise ValueError("%s of a fold begun at held-out data: DIC evaluates the data the posterior was fitted to "
                             "and has no held-out meaning" % what)

    def per_ladder(self, n_ladders=None):
        """one Pointwise per ladder of a batch: the kept chains, ladder-major, in equal shares; of a ragged batch's
        fold each trimmed to its ladder's length (the kept chains of one ladder share it)"""
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
            out.append(Pointwise(self.n.copy(), *[getattr(self, f)[k, :m] for f in STATE], self.par_origin[k],
                                 self.par_sum[k], self.chains[k], self.x[k, :m], self.y[k, :m], self.n_par, self.model,
                                 self.sigma, self.thin, 1, self.at_mean[k, :m]))
            out[-1].heldout = self.heldout
        return out

    # -- per datum ----------------------------------------------------------------------------
    def _n(self):
        return np.float64(self.n[0])

    def mean_loglike(self, k=0):
        """[n_data]: origin + sum / n"""
        with np.errstate(all="ignore"):
            return self.origin[k] + self.sum[k] / self._n()

    def var_loglike(self, k=0):
        """[n_data]: the sample variance of l over the kept samples, (sq - sum * sum / n) / (n - 1), never below 0"""
        n = self._n()
        with np.errstate(all="ignore"):
            v = (self.sq[k] - self.sum[k] * self.sum[k] / n) / (n - np.float64(1.0))
            return np.where(v < 0, 0.0, v)

    def lppd(self, k=0):
        """[n_data]: m_up + ln(S_up / n), the log pointwise predictive density"""
        self._no_padding("lppd")
        with np.errstate(all="ignore"):
            return self.m_up[k] + _ln(self.S_up[k] / self._n())

    def p_waic(self, kind=2, k=0):
        """[n_data]: the effective number of parameters per datum: kind 1 is 2 (lppd - mean_loglike), kind 2 the
        variance of l"""
        self._no_padding("p_waic")
        if kind == 2:
            return self.var_loglike(k)
        if kind == 1:
            with np.errstate(all="ignore"):
                return np.float64(2.0) * (self.lppd(k) - self.mean_loglike(k))
        raise ValueError("kind %r: 1 or 2" % (kind,))

    def elpd_waic(self, kind=2, k=0):
        self._no_padding("elpd_waic")
        with np.errstate(all="ignore"):
            return self.lppd(k) - self.p_waic(kind, k)

    def waic(self, kind=2, k=0):
        self._no_padding("waic")
        return -2.0 * _total(self.elpd_waic(kind, k))

    def waic_se(self, kind=2, k=0):
        """the standard error of sum elpd_waic: sqrt(n_data * variance of the pointwise elpd_waic)"""
        self._no_padding("waic_se")
        return _spread(self.elpd_waic(kind, k))

    def elpd_loo(self, k=0):
        """[n_data]: -(m_dn + ln(S_dn / n)): the log of the harmonic mean of the datum's likelihood"""
        self._no_padding("elpd_loo")
        with np.errstate(all="ignore"):
            return -(self.m_dn[k] + _ln(self.S_dn[k] / self._n()))

    def looic(self, k=0):
        self._no_padding("looic")
        return -2.0 * _total(self.elpd_loo(k))

    def p_loo(self, k=0):
        self._no_padding("p_loo")
        return _total(self.lppd(k)) - _total(self.elpd_loo(k))

    def loo_ess(self, k=0):
        """[n_data]: S_dn^2 / S2_dn, the effective sample size of the leave-one-out weights: n where every sample
        weighs the same, 1 where one sample carries the datum"""
        with np.errstate(all="ignore"):
            return self.S_dn[k] * self.S_dn[k] / self.S2_dn[k]

    def loo_unreliable(self, min_ess=10.0, k=0):
        """indices of the data whose leave-one-out weights have an effective sample size below min_ess (or NaN)"""
        with np.errstate(all="ignore"):
            return np.flatnonzero(~(self.loo_ess(k) >= min_ess))

    # -- DIC ----------------------------------------------------------------------------------
    def par_mean(self, k=0):
        """[n_par]: the plain arithmetic mean of the kept samples' parameters, par_origin + par_sum / n"""
        with np.errstate(all="ignore"):
            return self.par_origin[k] + self.par_sum[k] / self._n()

    def par_mean_all(self):
        return np.array([self.par_mean(k) for k in range(self.n_keep)]).reshape(self.n_keep, self.n_par)

    def p_dic(self, k=0):
        """2 (sum l_i(mean parameters) - sum mean_loglike); needs at_mean"""
        self._no_padding("p_dic")
        self._not_heldout("p_dic")
        return 2.0 * (_total(self.at_mean[k]) - _total(self.mean_loglike(k)))

    def dic(self, k=0):
        self._no_padding("dic")
        self._not_heldout("dic")
        return -2.0 * _total(self.at_mean[k]) + 2.0 * self.p_dic(k)

    # -- comparing two models on the same data ------------------------------------------------
    def compare(self, other, kind="loo", k=0, k_other=0):
        """(difference, standard error): sum over the data of this model's pointwise elpd minus the other's, and
        sqrt(n_data * variance of the pointwise differences).  kind: "loo" or "waic".  Positive favours this model.
        ValueError unless both were folded over the same data."""
        self._no_padding("compare")
        other._no_padding("compare")
        if self.x[k].tobytes() != other.x[k_other].tobytes() or self.y[k].tobytes() != other.y[k_other].tobytes():
            raise ValueError("the two folds do not hold the same data")
        if kind == "loo":
            a, b = self.elpd_loo(k), other.elpd_loo(k_other)
        elif kind == "waic":
            a, b = self.elpd_waic(2, k), other.elpd_waic(2, k_other)
        else:
            raise ValueError("kind %r: loo or waic" % (kind,))
        with np.errstate(all="ignore"):
            d = a - b
        return _total(d), _spread(d)

    # -- text ---------------------------------------------------------------------------------
    def criteria(self, k=0):
        """the criteria of kept chain k in the order of criteria.txt"""
        lppd, loo = _total(self.lppd(k)), _total(self.elpd_loo(k))
        return dict(zip(CRITERIA, (float(self.n[0]), lppd, _total(self.p_waic(1, k)), _total(self.p_waic(2, k)),
                                   _total(self.elpd_waic(2, k)), self.waic(2, k), self.waic_se(2, k), loo,
                                   -2.0 * loo, lppd - loo, self.dic(k), self.p_dic(k))))

    def criteria_text(self, k=0):
        """criteria.txt: `name<TAB>value` lines, %.15e"""
        return "".join("%s\t%s\n" % (name, _fmt(v)) for name, v in self.criteria(k).items())

    def text(self, k=0):
        """pointwise.txt: one line per datum, `x y mean sd lppd p_waic2 elpd_loo ess`, tab separated, %.15e"""
        self._no_padding("text")
        with np.errstate(all="ignore"):
            cols = [self.x[k], self.y[k], self.mean_loglike(k), np.sqrt(self.var_loglike(k)), self.lppd(k),
                    self.p_waic(2, k), self.elpd_loo(k), self.loo_ess(k)]
        return "".join("\t".join(_fmt(float(c[i])) for c in cols) + "\n" for i in range(self.n_data))

    # -- pointwise.bin --------------------------------------------------------------------------
    def _arrays(self):
        return ([(self.chains, "<i4"), (self.x, "<f8"), (self.y, "<f8")] + [(getattr(self, f), "<f8") for f in STATE] +
                [(self.par_origin, "<f8"), (self.par_sum, "<f8"), (self.at_mean, "<f8")])

    def write(self, path):
        self._no_padding("write")
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_keep, self.n_data, self.n_par, self.n_ladders, self.model, 0, 0,
                               int(self.n[0]), self.thin, self.sigma))
            for a, t in self._arrays():
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not a pointwise file" % path)
        magic, version, n_keep, n_data, n_par, n_ladders, model, _, _, n, thin, sigma = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a pointwise file of version %d" % (path, VERSION))
        ns = n_keep * n_data
        want = _HEAD.size + 4 * n_keep + 8 * (11 * ns + 2 * n_keep * n_par)
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
        par_origin, par_sum = take(n_keep * n_par, "<f8"), take(n_keep * n_par, "<f8")
        at_mean = take(ns, "<f8")
        return cls([n], *state, par_origin, par_sum, chains, x, y, n_par, model, sigma, thin, n_ladders, at_mean)


def _fmt(v):
    return "nan" if v != v else "%.15e" % v
