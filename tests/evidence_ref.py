"""A plain restatement of what the evidence fold (pt_evidence.h) must compute from column n_par+1 of sample rows,
which shares nothing with the kernels or with apemost_amd.evidence: sequential Python float operations for origin, sum,
sq, the batch sums and m (the running maximum of coef * v), and `decimal` at 60 digits for the exact
sum_t exp(x_t - m_final), against which S is judged.  Test infrastructure only."""
import decimal
import math

import numpy as np

DIGITS = 60


def closes(n, bs):
    """sample n, counted from 1, closes a batch when n % bs == bs - 1"""
    return n % bs == bs - 1


def exact_sum_exp(xs, m):
    """sum exp(x - m) over finite x <= m, exact to DIGITS digits, as a float; terms below exp(-800) add nothing to a sum
    that holds the term exp(0) = 1 and are left out"""
    ctx = decimal.Context(prec=DIGITS, Emin=-10 ** 9, Emax=10 ** 9)
    total = decimal.Decimal(0)
    dm = decimal.Decimal(m)
    for x in xs:
        d = ctx.subtract(decimal.Decimal(x), dm)
        if d > -800:
            total = ctx.add(total, ctx.exp(d))
    return float(total)


class RefEvidence:
    """col: [n][n_chains], the kept values of column n_par+1; coef: [2][n_chains] (up, down).  S holds the exact value
    for chains whose column is finite, NaN elsewhere (finite[c] says which)."""

    def __init__(self, col, coef, batch_size, max_batches):
        col = np.asarray(col, dtype=np.float64)
        n, nc = col.shape
        self.n = n
        self.origin, self.sum, self.sq = np.zeros(nc), np.zeros(nc), np.zeros(nc)
        self.batch = np.zeros((nc, max_batches + 1))
        self.m, self.S = np.zeros((2, nc)), np.full((2, nc), np.nan)
        self.finite = np.isfinite(col).all(axis=0)
        if n == 0:
            return
        for c in range(nc):
            v = col[:, c].tolist()
            self.origin[c] = v[0]
            s = 0.0
            for x in v:
                s += x - v[0]
            self.sum[c] = s
            s = 0.0
            for x in v:
                d = x - v[0]
                prod = d * d
                s += prod
            self.sq[c] = s
            part, k = 0.0, 0
            for i, x in enumerate(v):
                part += x
                if closes(i + 1, batch_size):
                    self.batch[c, k] = part
                    part = 0.0
                    k += 1
            self.batch[c, k] = part
            for r in range(2):
                a = float(coef[r][c])
                xs = [a * x for x in v]
                m = xs[0]
                for x in xs[1:]:
                    if x > m:
                        m = x
                self.m[r, c] = m
                if self.finite[c]:
                    self.S[r, c] = exact_sum_exp(xs, m)


def same_floats(a, b):
    """bit for bit wherever the value is not a NaN, and NaN exactly where the other is NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return False
    ok = ~np.isnan(a)
    return a[ok].tobytes() == b[ok].tobytes()


def assert_equals(ev, ref, what=""):
    """an Evidence against a RefEvidence: origin, sum, sq, batch with == on the bits everywhere (a NaN by its
    position); m on the bits and S to n 2^-50 relative on the chains whose column is finite.  Returns the largest
    relative error of S in units of 2^-53."""
    assert int(ev.n[0]) == ref.n, what
    for f in ("origin", "sum", "sq", "batch"):
        got, want = getattr(ev, f), getattr(ref, f)
        assert same_floats(got, want), (what, f, np.argwhere(~((got == want) | (np.isnan(got) & np.isnan(want))))[:5])
    fin = ref.finite
    assert same_floats(ev.m[:, fin], ref.m[:, fin]), (what, "m")
    if ref.n == 0 or not fin.any():
        return 0.0
    got, want = ev.S[:, fin], ref.S[:, fin]
    assert np.isfinite(got).all() and (want >= 1).all(), what
    rel = np.abs(got - want) / want
    worst = float(rel.max())
    print("%s: S of %d finite chains, n = %d: largest relative error %.3g = %.2f x 2^-53 (bound n 2^-50 = %.3g)" % (
        what, int(fin.sum()), ref.n, worst, worst * 2.0 ** 53, ref.n * 2.0 ** -50))
    assert worst <= ref.n * 2.0 ** -50, (what, worst, np.argwhere(rel > ref.n * 2.0 ** -50)[:5])
    return worst * 2.0 ** 53
