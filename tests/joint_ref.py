"""A plain restatement of what the joint marginals (pt_joint.h) must compute from sample rows, which shares nothing
with the kernel or with apemost_amd.joint.Joint.from_rows: the bin of every value by the bisection of
tests/summary_rows.bins_of over GSL's uniform edges, a Python loop that fills the grid, sequential Python float
additions for origin, sum and cross.  Test infrastructure only."""
import numpy as np

from tests.summary_rows import gsl_edges


def bin_indices(values, e):
    """tests/summary_rows.bins_of in its index form: the bin of every value (e[b] <= v < e[b+1]), -1 outside
    [e[0], e[n]) and for NaN.  np.searchsorted where the edges are sorted, gsl_histogram_increment's bisection where
    they are not."""
    n = len(e) - 1
    v = np.asarray(values, dtype=np.float64)
    out = np.full(len(v), -1, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        inside = np.flatnonzero((v >= e[0]) & (v < e[n]))
    if np.all(np.diff(e) >= 0):
        idx = np.searchsorted(e, v[inside], side="right") - 1
        out[inside] = np.minimum(idx, n - 1)
    else:
        for k in inside.tolist():
            x = float(v[k])
            left, right = 0, n
            while right - left > 1:
                mid = (left + right) // 2
                if x >= e[mid]:
                    left = mid
                else:
                    right = mid
            out[k] = left
    return out


def pairs_of(n_par):
    out = []
    for i in range(n_par):
        for j in range(i + 1, n_par):
            out.append((i, j))
    return out


class RefJoint:
    """rows [n][n_chains][n_par+2], already thinned; chains: the kept chains; boxes: (lo, hi) per parameter"""

    def __init__(self, rows, boxes, chains, nbins, pairs=None):
        rows = np.asarray(rows, dtype=np.float64)
        n, _, w = rows.shape
        n_par = w - 2
        self.pairs = pairs_of(n_par) if pairs is None else [tuple(p) for p in pairs]
        self.n = n
        self.counts = np.zeros((len(chains), len(self.pairs), nbins, nbins), dtype=np.uint64)
        self.origin = np.zeros((len(chains), n_par))
        self.sum = np.zeros((len(chains), n_par))
        self.cross = np.zeros((len(chains), n_par * (n_par + 1) // 2))
        edges = [gsl_edges(lo, hi, nbins) for lo, hi in boxes]
        for k, c in enumerate(chains):
            idx = [bin_indices(rows[:, c, p], edges[p]).tolist() for p in range(n_par)]
            for q, (i, j) in enumerate(self.pairs):
                grid = [[0] * nbins for _ in range(nbins)]
                for a, b in zip(idx[i], idx[j]):
                    if a >= 0 and b >= 0:
                        grid[a][b] += 1
                self.counts[k, q] = grid
            if n == 0:
                continue
            cols = [rows[:, c, p].tolist() for p in range(n_par)]
            for p in range(n_par):
                self.origin[k, p] = cols[p][0]
                s = 0.0
                for v in cols[p]:
                    s += v - cols[p][0]
                self.sum[k, p] = s
            t = 0
            for i in range(n_par):
                for j in range(i, n_par):
                    oi, oj = cols[i][0], cols[j][0]
                    s = 0.0
                    for x, y in zip(cols[i], cols[j]):
                        prod = (x - oi) * (y - oj)
                        s += prod
                    self.cross[k, t] = s
                    t += 1


def same_floats(a, b):
    """bit for bit wherever the value is not a NaN, and NaN exactly where the other is NaN (a NaN's sign differs
    between machines, its presence does not)"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()


def assert_equals(jt, ref, finite_chains=(), what=""):
    """a Joint against a RefJoint: n and counts with ==, the moments bit for bit.  Only a NaN is compared by its
    position; for the kept-chain slots in finite_chains origin and sum must hold none (their rows are finite; a cross
    sum of such rows can still overflow to inf - inf), so those compare bit for bit throughout."""
    assert int(jt.n[0]) == ref.n, what
    assert [tuple(p) for p in jt.pairs.tolist()] == ref.pairs, what
    bad = np.argwhere(jt.counts != ref.counts)
    assert len(bad) == 0, "%s: first of %d differing counts at (k, q, a, b) = %s: %d, expected %d" % (
        what, len(bad), tuple(bad[0]), jt.counts[tuple(bad[0])], ref.counts[tuple(bad[0])])
    for k in range(len(ref.origin)):
        if k in finite_chains:
            assert not np.isnan(ref.origin[k]).any() and not np.isnan(ref.sum[k]).any(), (what, k)
        for f in ("origin", "sum", "cross"):
            assert same_floats(getattr(jt, f)[k], getattr(ref, f)[k]), (what, k, f, getattr(jt, f)[k], getattr(ref, f)[k])
