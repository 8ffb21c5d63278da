"""K-fold and leave-block-out cross-validation on ladder batches: the held-out log predictive density of every datum
and the joint predictive density of every block, from a pointwise fold begun at the caller's data
(apemost_hip_pointwise_begin_at, include/apemost_hip.h; the joint rule is the head of
apemost_amd/csrc/pt_pointwise_joint.h).

PSIS (apemost_amd/psis.py) flags the data whose leave-one-out estimate cannot be trusted; the answer to a flagged datum,
or to a series where leaving one point out means little, is to refit without a block and score the block that was left
out.  The K training sets differ in length by at most one row and each needs a ladder of its own: a ragged ladder batch
(HipSampler.batch with a list of matrices) runs them in one launch, bit for bit as K stand-alone samplers would.  This
module is the front end; everything in it except the two sampler calls (sampler(), begin()) is numpy.

    folds = kfold.folds(len(data), 5)                        # K sorted index arrays that partition range(n_data)
    s = kfold.sampler(model, n_par, n_chains, data, folds, seeds)    # ladder b is fitted to data without folds[b]
    ...                                                      # set_state / calibrate as for any batch
    kfold.begin(s, data, folds)                              # chain 0 of ladder b (beta = 1) is scored on data[folds[b]]
    s.run_sampler(n_rounds, n_swap, d.data_ptr()); s.pointwise_accumulate(d.data_ptr(), n_rounds * n_swap)
    cv = kfold.result(s, folds)                              # a KFold
    cv.elpd, cv.se, cv.lpd_joint, cv.compare(other)

Per datum i of fold b, with the series (kept chain b, position of i in folds[b]) of the pointwise fold:
    elpd_i      = m_up + ln(S_up / n)          the log of the mean over the kept samples of the datum's likelihood under a
                                               posterior that has not seen it
    elpd        = sum elpd_i                   se = sqrt(n_data * variance of elpd_i), the variance divided by n_data - 1
Per fold b, from the joint state (kfold.Joint: origin, sum, sq, m, S of J_t = the sum of the block's terms under sample t):
    lpd_joint   = m + ln(S / n)                the log predictive density of the block as a whole; not sum elpd_i of it
    joint_mean  = origin + sum / n             joint_var = (sq - sum * sum / n) / (n - 1), never below 0
The _dn words of the fold (the leave-one-out side) are still folded, because the kernel is the pointwise fold's, and
mean nothing here: a datum that was never in cannot be left out.  Nothing in this module reads them.

As everywhere in the pointwise fold, the sine models' terms leave out the constant -ln(sigma sqrt(2 pi)) per datum:
elpd is shifted by n_data times that, differences between models fitted with the same sigma are not.

kfold.bin (little-endian), version 1:
    char[8]  "APEMOSTK"
    uint32   version, n_data, K, has_joint
    uint64   n, thin
    int32    fold_of[n_data]
    double   x, y, elpd_i: [n_data] each
    double   lpd_joint, joint_mean, joint_var: [K] each (NaN without joint)
"""
import struct

import numpy as np

from . import capi
from .pointwise import _fmt, _ln, _spread, _total

MAGIC = b"APEMOSTK"
VERSION = 1
_HEAD = struct.Struct("<8s4I2Q")
SCHEMES = ("interleaved", "blocks", "random")
JOINT_STATE = ("origin", "sum", "sq", "m", "S")


def folds(n_data, k, scheme="interleaved", seed=None):
    """K sorted index arrays that partition range(n_data).  interleaved: fold b holds the i with i % k == b.  blocks:
    contiguous blocks whose sizes differ by at most one, the longer ones first (leave-block-out of a series).  random:
    a permutation by numpy.random.default_rng(seed) dealt out as `blocks` deals the identity, each fold sorted."""
    n_data, k = int(n_data), int(k)
    if n_data < 1 or k < 1 or k > n_data:
        raise ValueError("%d folds of %d data: 1 <= k <= n_data" % (k, n_data))
    if scheme not in SCHEMES:
        raise ValueError("scheme %r: one of %s" % (scheme, ", ".join(SCHEMES)))
    idx = np.arange(n_data, dtype=np.int64)
    if scheme == "interleaved":
        return [idx[b::k].copy() for b in range(k)]
    if scheme == "random":
        idx = np.random.default_rng(seed).permutation(n_data).astype(np.int64)
    short, longer = divmod(n_data, k)
    sizes = [short + 1] * longer + [short] * (k - longer)
    ends = np.cumsum(sizes)
    return [np.sort(idx[e - m:e]) for e, m in zip(ends.tolist(), sizes)]


def _check(n_data, fs):
    fs = [np.asarray(f, dtype=np.int64).reshape(-1) for f in fs]
    seen = np.concatenate(fs) if fs else np.zeros(0, dtype=np.int64)
    if len(seen) != n_data or not np.array_equal(np.sort(seen), np.arange(n_data)):
        raise ValueError("the folds do not partition range(%d)" % n_data)
    return fs


def training_sets(data, fs):
    """one matrix per fold: the rows of data that the fold does not hold, in their original order"""
    data = np.asarray(data, dtype=np.float64)
    out = []
    for f in _check(len(data), fs):
        keep = np.ones(len(data), dtype=bool)
        keep[f] = False
        out.append(np.ascontiguousarray(data[keep]))
    return out


def sampler(model, n_par, n_chains, data, fs, seeds, **kw):
    """a ragged ladder batch of len(fs) ladders of n_chains chains each: ladder b holds the training set of fold b and
    runs under seeds[b], bit for bit the stand-alone sampler of that training set and seed"""
    from .sampler import HipSampler
    if len(seeds) != len(fs):
        raise ValueError("%d seeds for %d folds" % (len(seeds), len(fs)))
    sets = training_sets(data, fs)
    if any(len(m) < 1 for m in sets):
        raise ValueError("a training set is empty: one fold holds every datum")
    return HipSampler.batch(model, n_par, n_chains, sets, list(seeds), **kw)


def begin(s, data, fs, thin=1, joint=True, tail=None):
    """open the pointwise fold of the batch `s` at the held-out data: chain 0 of ladder b, which has beta = 1, is scored
    on data[fs[b]]"""
    data = np.asarray(data, dtype=np.float64)
    fs = _check(len(data), fs)
    if len(fs) != s.n_ladders:
        raise ValueError("%d folds for a batch of %d ladders" % (len(fs), s.n_ladders))
    s.pointwise_begin(chains=[b * s.chains_per_ladder for b in range(len(fs))], thin=thin, tail=tail,
                      at=[data[f][:, :2] for f in fs], joint=joint)


def result(s, fs):
    """the open fold of begin() as a KFold (synchronises with the accumulates issued so far)"""
    pw = s.pointwise(at_mean=False)
    jt = s.pointwise_joint() if getattr(s, "_pw_joint", False) else None
    return KFold.from_state(pw, jt, fs)


class Joint:
    """The joint predictive state of a fold's blocks (apemost_hip_pointwise_joint_view): per kept chain the moments
    about the first sample and the running log-sum-exp of J_t, the sum over its block of the terms under sample t."""

    def __init__(self, n, origin, sum, sq, m, S, chains, lengths, thin=1):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.chains = np.ascontiguousarray(chains, dtype=np.int32).reshape(-1)
        self.n_keep = len(self.chains)
        for name, a in zip(JOINT_STATE, (origin, sum, sq, m, S)):
            setattr(self, name, np.ascontiguousarray(a, dtype=np.float64).reshape(self.n_keep).copy())
        self.lengths = np.ascontiguousarray(lengths, dtype=np.int32).reshape(self.n_keep)
        self.thin = int(thin)

    @classmethod
    def empty(cls, chains, lengths, thin=1):
        z = [np.zeros(len(chains)) for _ in JOINT_STATE]
        return cls(np.zeros(1, dtype=np.uint64), *z, chains, lengths, thin)

    def view(self):
        """the apemost_hip_pointwise_joint_view over this object's arrays"""
        return capi.PointwiseJointView(n=self.n.ctypes.data_as(capi._up),
                                       **{f: getattr(self, f).ctypes.data_as(capi._dp) for f in JOINT_STATE})

    def _n(self):
        return np.float64(self.n[0])

    def lpd(self):
        """[n_keep]: m + ln(S / n), the log predictive density of every kept chain's block as a whole"""
        with np.errstate(all="ignore"):
            return self.m + _ln(self.S / self._n())

    def mean(self):
        """[n_keep]: origin + sum / n, the mean over the kept samples of the block's log-likelihood"""
        with np.errstate(all="ignore"):
            return self.origin + self.sum / self._n()

    def var(self):
        """[n_keep]: (sq - sum * sum / n) / (n - 1), never below 0"""
        n = self._n()
        with np.errstate(all="ignore"):
            v = (self.sq - self.sum * self.sum / n) / (n - np.float64(1.0))
            return np.where(v < 0, 0.0, v)


class KFold:
    """The result of a K-fold run: elpd_i [n_data] in the original order of the data, elpd and se, and per fold
    lpd_joint, joint_mean and joint_var [K] (NaN where the fold kept no joint state).  fold_of[i] is the fold datum i
    was held out in; n the kept samples."""

    def __init__(self, n, x, y, elpd_i, fold_of, lpd_joint=None, joint_mean=None, joint_var=None, thin=1):
        self.n, self.thin = int(n), int(thin)
        self.x, self.y, self.elpd_i = (np.ascontiguousarray(a, dtype=np.float64).reshape(-1) for a in (x, y, elpd_i))
        self.n_data = len(self.x)
        self.fold_of = np.ascontiguousarray(fold_of, dtype=np.int32).reshape(self.n_data)
        self.k = int(self.fold_of.max()) + 1 if self.n_data else 0
        self.has_joint = lpd_joint is not None
        nan = np.full(self.k, np.nan)
        self.lpd_joint, self.joint_mean, self.joint_var = (
            nan.copy() if a is None else np.ascontiguousarray(a, dtype=np.float64).reshape(self.k)
            for a in (lpd_joint, joint_mean, joint_var))

    @classmethod
    def from_state(cls, pw, jt, fs):
        """from the Pointwise of a fold begun at the held-out data (kept chain b scored on fold b, in the fold's order)
        and its Joint, or None"""
        fs = [np.asarray(f, dtype=np.int64).reshape(-1) for f in fs]
        if len(fs) != pw.n_keep:
            raise ValueError("%d folds, %d kept chains" % (len(fs), pw.n_keep))
        n_data = sum(len(f) for f in fs)
        fs = _check(n_data, fs)
        lens = np.full(pw.n_keep, pw.n_data) if pw.lengths is None else np.asarray(pw.lengths)
        if [len(f) for f in fs] != lens.tolist():
            raise ValueError("the folds hold %s data, the kept chains %s" % ([len(f) for f in fs], lens.tolist()))
        x, y, elpd, fold_of = np.zeros(n_data), np.zeros(n_data), np.zeros(n_data), np.zeros(n_data, dtype=np.int32)
        n = np.float64(pw.n[0])
        for b, f in enumerate(fs):
            m = len(f)
            with np.errstate(all="ignore"):
                elpd[f] = pw.m_up[b, :m] + _ln(pw.S_up[b, :m] / n)
            x[f], y[f], fold_of[f] = pw.x[b, :m], pw.y[b, :m], b
        if jt is None:
            return cls(int(pw.n[0]), x, y, elpd, fold_of, thin=pw.thin)
        if int(jt.n[0]) != int(pw.n[0]):
            raise ValueError("the fold holds %d samples, its joint state %d" % (int(pw.n[0]), int(jt.n[0])))
        return cls(int(pw.n[0]), x, y, elpd, fold_of, jt.lpd(), jt.mean(), jt.var(), pw.thin)

    def folds(self):
        """the K sorted index arrays"""
        return [np.flatnonzero(self.fold_of == b) for b in range(self.k)]

    @property
    def elpd(self):
        """sum elpd_i, in the data's order"""
        return _total(self.elpd_i)

    @property
    def se(self):
        """sqrt(n_data * variance of elpd_i): the standard error of elpd (NaN for one datum)"""
        return _spread(self.elpd_i)

    def compare(self, other, k_other=0):
        """(difference, standard error) of the summed elpd against another KFold, a psis.Psis or a pointwise.Pointwise
        (its plain importance-sampling elpd_loo of kept chain k_other) over the same data, paired datum by datum:
        sum of the differences and sqrt(n_data * their variance).  Positive favours this one.  ValueError unless both
        hold the same data in the same order."""
        if isinstance(other, KFold):
            ox, oy, oe = other.x, other.y, other.elpd_i
        elif hasattr(other, "pareto_k"):
            ox, oy, oe = other.x, other.y, other.elpd_loo()
        else:
            ox, oy, oe = other.x[k_other], other.y[k_other], other.elpd_loo(k_other)
        if self.x.tobytes() != np.ascontiguousarray(ox, dtype=np.float64).tobytes() or \
                self.y.tobytes() != np.ascontiguousarray(oy, dtype=np.float64).tobytes():
            raise ValueError("the two results do not hold the same data")
        with np.errstate(all="ignore"):
            d = self.elpd_i - np.asarray(oe, dtype=np.float64)
        return _total(d), _spread(d)

    def text(self):
        """the summary, one line per fold (`fold size elpd lpd_joint joint_mean joint_var`) and one per datum
        (`x y fold elpd_i`)"""
        out = ["n\t%d\n" % self.n, "k\t%d\n" % self.k, "elpd\t%s\n" % _fmt(self.elpd), "se\t%s\n" % _fmt(self.se)]
        for b, f in enumerate(self.folds()):
            out.append("fold %d\t%d\t%s\t%s\t%s\t%s\n" % (b, len(f), _fmt(_total(self.elpd_i[f])),
                                                          _fmt(float(self.lpd_joint[b])), _fmt(float(self.joint_mean[b])),
                                                          _fmt(float(self.joint_var[b]))))
        for i in range(self.n_data):
            out.append("%s\t%s\t%d\t%s\n" % (_fmt(float(self.x[i])), _fmt(float(self.y[i])), int(self.fold_of[i]),
                                             _fmt(float(self.elpd_i[i]))))
        return "".join(out)

    def write(self, path):
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_data, self.k, 1 if self.has_joint else 0, self.n, self.thin))
            f.write(self.fold_of.astype("<i4").tobytes())
            for a in (self.x, self.y, self.elpd_i, self.lpd_joint, self.joint_mean, self.joint_var):
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not a kfold file" % path)
        magic, version, n_data, k, has_joint, n, thin = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a kfold file of version %d" % (path, VERSION))
        want = _HEAD.size + 4 * n_data + 8 * (3 * n_data + 3 * k)
        if want != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), want))
        off = _HEAD.size
        fold_of = np.frombuffer(raw, dtype="<i4", count=n_data, offset=off).copy()
        off += 4 * n_data

        def take(count):
            nonlocal off
            a = np.frombuffer(raw, dtype="<f8", count=count, offset=off).copy()
            off += 8 * count
            return a
        x, y, elpd = take(n_data), take(n_data), take(n_data)
        joint = [take(k) for _ in range(3)]
        if not has_joint:
            joint = [None] * 3
        return cls(n, x, y, elpd, fold_of, *joint, thin=thin)
