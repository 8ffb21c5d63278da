"""A restatement of the autocorrelation fold (include/apemost_hip.h, apemost_hip_autocorr_*) that shares nothing with
the kernels or with apemost_amd/autocorr.py: time is the outer loop, one sample after the other, and every lag sum
receives its rounded product in that order; Autocorr.from_rows goes lag by lag instead.  For series too long for a
Python loop over time, ref_series_long takes numpy's cumulative sums, which add in the same order.  Test infrastructure
only."""
import numpy as np


def ref_series(x, L):
    """(origin, sum, lag [L], head [L-1], tail [L-1]) of one series x_0, x_1, ... by a sequential loop over time"""
    x = np.asarray(x, dtype=np.float64)
    n, H = len(x), L - 1
    lag, head, tail = np.zeros(L), np.zeros(H), np.zeros(H)
    if n == 0:
        return 0.0, 0.0, lag, head, tail
    origin = x[0]
    total = np.float64(0.0)
    with np.errstate(all="ignore"):
        d = np.zeros(n)
        for t in range(n):
            d[t] = x[t] - origin
            total = total + d[t]
            m = min(t, L - 1) + 1                            # lags 0 .. m-1 have a partner at time t
            past = d[t::-1][:m] if t >= 1 else d[:1]         # d_t, d_{t-1}, ..., d_{t-m+1}
            prod = d[t] * past
            lag[:m] = lag[:m] + prod
    for j in range(H):
        if j < n:
            head[j] = d[j]
        if n - H + j >= 0:
            tail[j] = d[n - H + j]
    return origin, total, lag, head, tail


def ref_series_long(x, L):
    """the same by cumulative sums (np.cumsum adds in index order), for long series and few lags"""
    x = np.asarray(x, dtype=np.float64)
    n, H = len(x), L - 1
    lag, head, tail = np.zeros(L), np.zeros(H), np.zeros(H)
    with np.errstate(all="ignore"):
        d = x - x[0]
        for l in range(min(L, n)):
            lag[l] = _total(d[l:] * d[:n - l])
        total = _total(d)
    for j in range(H):
        if j < n:
            head[j] = d[j]
        if n - H + j >= 0:
            tail[j] = d[n - H + j]
    return x[0], total, lag, head, tail


def _total(v):
    """0.0 + v_0 + v_1 + ... in index order (the leading zero decides the sign of a zero sum)"""
    return np.cumsum(np.concatenate(([0.0], v)))[-1]


class RefAutocorr:
    """the fold of kept rows [n][n_chains][w] for the kept chains and columns"""

    def __init__(self, rows, chains, L, cols, long=False):
        rows = np.asarray(rows, dtype=np.float64)
        k, c = len(chains), len(cols)
        self.n = rows.shape[0]
        self.origin, self.sum = np.zeros((k, c)), np.zeros((k, c))
        self.lag, self.head, self.tail = np.zeros((k, c, L)), np.zeros((k, c, L - 1)), np.zeros((k, c, L - 1))
        f = ref_series_long if long else ref_series
        for a, chain in enumerate(chains):
            for b, col in enumerate(cols):
                o, s, lag, head, tail = f(rows[:, chain, col], L)
                self.origin[a, b], self.sum[a, b] = o, s
                self.lag[a, b], self.head[a, b], self.tail[a, b] = lag, head, tail


def same_floats(a, b):
    """bit for bit, except that a NaN equals a NaN of any sign and payload"""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a[~na].view(np.uint64), b[~nb].view(np.uint64)))


FIELDS = ("origin", "sum", "lag", "head", "tail")


def assert_equals(got, ref, what=""):
    """an Autocorr (or RefAutocorr) against another, every field with == on the bits"""
    n = int(got.n[0]) if hasattr(got.n, "__len__") else int(got.n)
    m = int(ref.n[0]) if hasattr(ref.n, "__len__") else int(ref.n)
    assert n == m, (what, n, m)
    for f in FIELDS:
        a, b = getattr(got, f), getattr(ref, f)
        if not same_floats(a, b):
            a, b = np.asarray(a), np.asarray(b)
            with np.errstate(all="ignore"):
                bad = np.argwhere(~((a == b) | (np.isnan(a) & np.isnan(b))))
            at = tuple(bad[0]) if len(bad) else ()
            raise AssertionError("%s %s: %d entries differ (signs of zero included), first at %s: %r against %r" % (
                what, f, len(bad), at, a[at] if len(bad) else None, b[at] if len(bad) else None))
