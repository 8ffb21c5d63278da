"""Joint marginals: pair histograms and moments of kept chains, from what apemost_hip_joint_get hands out.

A Joint holds one view (include/apemost_hip.h, apemost_hip_joint_view): per kept chain k the number of kept
samples, for every pair q = (i, j) the nbins x nbins counts over the run summary's bins, and the moments about the
first sample: origin, sum of d = v - origin, and the sums of d_i * d_j.  From them come the mean, the covariance and
the correlation matrix, the 2-D posterior density of a pair and its two 1-D projections, which are the summary's
histograms.  It reads and writes `joint.bin`, the file the C host's run phase leaves with the APEMOST_DUMP token
`joint`, and the text files for gnuplot.

joint.bin (little-endian), version 1:
    char[8]  "APEMOSTJ"
    uint32   version, n_keep, n_par, nbins, n_pairs, 0
    uint64   n, thin
    int32    chains[n_keep]
    int32    pairs[n_pairs][2]
    double   lo[n_par], hi[n_par]
    double   origin[n_keep][n_par], sum[n_keep][n_par]
    double   cross[n_keep][n_par (n_par + 1) / 2]          (upper triangle, row by row)
    uint64   counts[n_keep][n_pairs][nbins][nbins]
"""
import ctypes as C
import os
import struct

import numpy as np

from . import capi
from .summary import edges as summary_edges

MAGIC = b"APEMOSTJ"
VERSION = 1
_HEAD = struct.Struct("<8s6I2Q")


def all_pairs(n_par):
    """every (i, j), i < j, in lexicographic order: the default pair list"""
    return [(i, j) for i in range(n_par) for j in range(i + 1, n_par)]


def tri_index(n_par, i, j):
    """slot of (i, j), i <= j, in the row-major upper triangle"""
    return i * n_par - i * (i - 1) // 2 + (j - i)


def bins_of(values, e):
    """the bin of every value over the edges e (e[b] <= v < e[b+1]), -1 outside [e[0], e[n]) and for NaN:
    gsl_histogram_increment's bisection, all values at once"""
    v = np.asarray(values, dtype=np.float64)
    n = len(e) - 1
    with np.errstate(invalid="ignore"):
        inside = (v >= e[0]) & (v < e[n])
        left = np.zeros(v.shape, dtype=np.int64)
        right = np.full(v.shape, n, dtype=np.int64)
        while np.any(right - left > 1):
            mid = (left + right) >> 1
            go = right - left > 1
            up = go & (v >= e[mid])
            left = np.where(up, mid, left)
            right = np.where(go & ~up, mid, right)
    return np.where(inside, left, -1)


class Joint:
    def __init__(self, n, counts, origin, sum, cross, pairs, lo, hi, nbins, chains=None, thin=1):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.origin = np.ascontiguousarray(origin, dtype=np.float64)         # [k][p]
        self.sum = np.ascontiguousarray(sum, dtype=np.float64)               # [k][p]
        self.cross = np.ascontiguousarray(cross, dtype=np.float64)           # [k][n_par (n_par + 1) / 2]
        self.pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        self.lo = np.ascontiguousarray(lo, dtype=np.float64)
        self.hi = np.ascontiguousarray(hi, dtype=np.float64)
        self.nbins = int(nbins)
        self.n_keep, self.n_par = self.sum.shape
        self.counts = np.ascontiguousarray(counts, dtype=np.uint64).reshape(self.n_keep, len(self.pairs), self.nbins,
                                                                             self.nbins)
        assert self.origin.shape == self.sum.shape and self.lo.shape == self.hi.shape == (self.n_par,)
        assert self.cross.shape == (self.n_keep, self.n_par * (self.n_par + 1) // 2)
        self.chains = np.arange(self.n_keep, dtype=np.int32) if chains is None else np.ascontiguousarray(chains, dtype=np.int32)
        self.thin = int(thin)

    @classmethod
    def empty(cls, n_keep, n_par, nbins, pairs, lo, hi, chains=None, thin=1):
        pairs = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
        return cls(np.zeros(1, dtype=np.uint64), np.zeros((n_keep, len(pairs), nbins, nbins), dtype=np.uint64),
                   np.zeros((n_keep, n_par)), np.zeros((n_keep, n_par)), np.zeros((n_keep, n_par * (n_par + 1) // 2)),
                   pairs, lo, hi, nbins, chains, thin)

    def view(self):
        """the apemost_hip_joint_view over this object's arrays"""
        return capi.JointView(n=self.n.ctypes.data_as(capi._up), counts=self.counts.ctypes.data_as(capi._up),
                              origin=self.origin.ctypes.data_as(capi._dp), sum=self.sum.ctypes.data_as(capi._dp),
                              cross=self.cross.ctypes.data_as(capi._dp))

    @classmethod
    def from_rows(cls, rows, lo, hi, chains=(0,), nbins=200, pairs=None, thin=1):
        """the joint marginals of host sample rows [n][n_chains][n_par+2] (already thinned): what the device
        computes, for tests and for existing dumps.  Counts by numpy, the moments as sequential Python sums."""
        rows = np.asarray(rows, dtype=np.float64)
        n, _, w = rows.shape
        n_par = w - 2
        pairs = all_pairs(n_par) if pairs is None else pairs
        jt = cls.empty(len(chains), n_par, nbins, pairs, lo, hi, chains, thin)
        jt.n[0] = n
        e = [summary_edges(float(jt.lo[p]), float(jt.hi[p]), nbins) for p in range(n_par)]
        for k, c in enumerate(chains):
            b = [bins_of(rows[:, c, p], e[p]) for p in range(n_par)]
            for q, (i, j) in enumerate(jt.pairs.tolist()):
                ok = (b[i] >= 0) & (b[j] >= 0)
                jt.counts[k, q] = np.bincount(b[i][ok] * nbins + b[j][ok], minlength=nbins * nbins).reshape(nbins, nbins)
            if n == 0:
                continue
            cols = [rows[:, c, p].tolist() for p in range(n_par)]
            origin = [col[0] for col in cols]
            d = [[v - o for v in col] for col, o in zip(cols, origin)]
            jt.origin[k] = origin
            for p in range(n_par):
                s = 0.0
                for x in d[p]:
                    s += x
                jt.sum[k, p] = s
            for i in range(n_par):
                for j in range(i, n_par):
                    s = 0.0
                    for x, y in zip(d[i], d[j]):
                        s += x * y
                    jt.cross[k, tri_index(n_par, i, j)] = s
        return jt

    # -- what it gives ------------------------------------------------------------------------
    def edges(self, p):
        """the nbins + 1 bin edges of parameter p: the run summary's"""
        return summary_edges(float(self.lo[p]), float(self.hi[p]), self.nbins)

    def pair_index(self, i, j):
        return self.pairs.tolist().index([i, j])

    def marginal(self, k, q, axis):
        """the 1-D projection of pair q of kept chain k onto its first (axis 0) or second (axis 1) parameter"""
        return self.counts[k, q].sum(axis=1 - axis, dtype=np.uint64)

    def mean(self, k=0):
        with np.errstate(all="ignore"):
            return self.origin[k] + self.sum[k] / np.float64(self.n[0])

    def cross_matrix(self, k=0):
        m = np.zeros((self.n_par, self.n_par))
        for i in range(self.n_par):
            for j in range(i, self.n_par):
                m[i, j] = m[j, i] = self.cross[k, tri_index(self.n_par, i, j)]
        return m

    def cov(self, k=0):
        """the sample covariance (cross_ij - sum_i sum_j / n) / (n - 1)"""
        n = np.float64(self.n[0])
        s = self.sum[k]
        with np.errstate(all="ignore"):
            return (self.cross_matrix(k) - np.outer(s, s) / n) / (n - np.float64(1))

    def corr(self, k=0):
        """cov_ij / (sqrt(cov_ii) sqrt(cov_jj)); the diagonal is 1 where the variance is finite and positive, NaN
        elsewhere"""
        c = self.cov(k)
        with np.errstate(all="ignore"):
            sd = np.sqrt(np.diag(c))
            r = c / np.outer(sd, sd)
        v = np.diag(c)
        r[np.diag_indices(self.n_par)] = np.where(np.isfinite(v) & (v > 0), 1.0, np.nan)
        return r

    def density(self, k, q):
        """(x edges, y edges, density [nbins][nbins]) of pair q: counts / (total * bin area), which sums to one over
        the box's nominal bins"""
        i, j = self.pairs[q]
        c = self.counts[k, q].astype(np.float64)
        area = (self.hi[i] - self.lo[i]) / self.nbins * ((self.hi[j] - self.lo[j]) / self.nbins)
        with np.errstate(all="ignore"):
            return self.edges(i), self.edges(j), c / (c.sum() * area)

    # -- joint.bin ------------------------------------------------------------------------------
    def write(self, path):
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_keep, self.n_par, self.nbins, len(self.pairs), 0, int(self.n[0]),
                               self.thin))
            for a, t in ((self.chains, "<i4"), (self.pairs, "<i4"), (self.lo, "<f8"), (self.hi, "<f8"), (self.origin, "<f8"),
                         (self.sum, "<f8"), (self.cross, "<f8"), (self.counts, "<u8")):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        magic, version, n_keep, n_par, nbins, n_pairs, _, n, thin = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a joint file of version %d" % (path, VERSION))
        off = _HEAD.size

        def take(count, dtype):
            nonlocal off
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=off)
            off += a.itemsize * count
            return a.copy()
        tri = n_par * (n_par + 1) // 2
        chains, pairs = take(n_keep, "<i4"), take(2 * n_pairs, "<i4").reshape(n_pairs, 2)
        lo, hi = take(n_par, "<f8"), take(n_par, "<f8")
        origin, total = take(n_keep * n_par, "<f8").reshape(n_keep, n_par), take(n_keep * n_par, "<f8").reshape(n_keep, n_par)
        cross = take(n_keep * tri, "<f8").reshape(n_keep, tri)
        counts = take(n_keep * n_pairs * nbins * nbins, "<u8")
        if off != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), off))
        return cls([n], counts, origin, total, cross, pairs, lo, hi, nbins, chains, thin)

    # -- text for gnuplot ---------------------------------------------------------------------------
    def pair_text(self, k, q):
        """`x_lower x_upper y_lower y_upper count` per cell, x-major, a blank line after each x row (gnuplot's
        `splot ... with pm3d` reads that)"""
        i, j = self.pairs[q]
        ex = ["%.15e" % v for v in self.edges(i).tolist()]
        ey = ["%.15e" % v for v in self.edges(j).tolist()]
        c = self.counts[k, q].tolist()
        out = []
        for a in range(self.nbins):
            head = ex[a] + " " + ex[a + 1] + " "
            row = c[a]
            out.append("".join("%s%s %s %d\n" % (head, ey[b], ey[b + 1], row[b]) for b in range(self.nbins)))
            out.append("\n")
        return "".join(out)

    def correlation_text(self, k=0):
        """n_par lines of n_par values, "%.15e", tab separated; a NaN prints as nan"""
        return "".join("\t".join("nan" if v != v else "%.15e" % v for v in row) + "\n" for row in self.corr(k).tolist())

    def write_text(self, directory, names, k=0):
        """<name_i>-<name_j>.joint for every pair of kept chain k, and correlation.matrix"""
        assert len(names) == self.n_par
        for q, (i, j) in enumerate(self.pairs.tolist()):
            with open(os.path.join(str(directory), "%s-%s.joint" % (names[i], names[j])), "w") as f:
                f.write(self.pair_text(k, q))
        with open(os.path.join(str(directory), "correlation.matrix"), "w") as f:
            f.write(self.correlation_text(k))
