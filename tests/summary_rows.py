"""Hand-built sample rows for the run summary (pt_summary.h) and a plain restatement of what it must compute
from them, which shares nothing with the kernel: bins by np.searchsorted over GSL's uniform edges, sums as
sequential Python float additions.  Test infrastructure only; used by tests/test_gpu_summary.py (the kernel) and
tests/test_summary_host.py (the restatement itself against the host's `analyse`).

Four parameters per row (the samplers of the tests are simplesin's), hence two sets of boxes.  They are the
boxes where a guess (v-lo)/(hi-lo)*nbins is off by one, a negative one and one of width 1e-300.
"""
import numpy as np

BOX_SETS = {
    "A": [(0.1, 50.0), (10.0, 12.0), (1e15, 1e15 + 3), (-7.3, -0.2)],
    "B": [(-5e-301, 5e-301), (0.0, 0.3), (-1e15 - 3, -1e15), (0.1, 50.0)],
}
N_STEPS = 3000
# (first step, steps, skip, thin) of every summary_accumulate call: the first keeps 2300 steps in one launch
# (passes of 1024, 1024 and 252 values), the others thin
CALLS = [(0, 2300, 0, 1), (2300, 400, 3, 7), (2700, 300, 1, 2)]


def gsl_edges(lo, hi, n):
    """gsl_histogram_set_ranges_uniform and the reference's create_hist()"""
    e = [((n - i) / n) * lo + (i / n) * hi for i in range(n + 1)]
    e[n] += (hi - lo) / 10000
    return np.array(e)


def kept_steps():
    return np.concatenate([np.arange(first + skip, first + n, thin) for first, n, skip, thin in CALLS])


def pool(lo, hi, nbins, finite_only, rng):
    """the values of one parameter: every edge and its two neighbours, the box's corners and the widened top with
    their neighbours, zeros, subnormals, values far outside, a few hundred inside; and the non-finite ones"""
    e = gsl_edges(lo, hi, nbins)
    top = hi + (hi - lo) / 10000
    near = np.concatenate([e, [lo, hi, top]])
    v = [near, np.nextafter(near, -np.inf), np.nextafter(near, np.inf),
         [0.0, -0.0, 5e-324, -5e-324, 1.1e-308, -1.1e-308, 2.2250738585072014e-308, 1e300, -1e300, 1e17, -1e17,
          lo - (hi - lo), hi + (hi - lo)],
         lo + (hi - lo) * rng.uniform(0, 1, 300)]
    if not finite_only:
        v.append([np.inf, -np.inf, np.nan, np.copysign(np.nan, -1.0)])
    return np.concatenate([np.asarray(x, dtype=np.float64) for x in v])


def build_rows(box_set, nbins, n_chains=300, seed=1):
    """rows [N_STEPS][n_chains][6].  Column p walks parameter p's pool across the chains of a group, so that every
    pool value is kept in some chain; chains with h % 3 == 0 also see the non-finite values (their batch sums
    turn NaN), the others stay finite so that their sums compare bit for bit.  prob - prior spans 1e-300 to
    1e300 with mixed signs: its sum depends on the order of the additions."""
    rng = np.random.default_rng(seed)
    boxes = BOX_SETS[box_set]
    rows = np.zeros((N_STEPS, n_chains, 6))
    for p, (lo, hi) in enumerate(boxes):
        fin, full = pool(lo, hi, nbins, True, rng), pool(lo, hi, nbins, False, rng)
        assert len(full) <= 2300 * n_chains // 3
        for h0, pl in ((0, full), (1, fin), (2, fin)):
            m = len(range(h0, n_chains, 3))                  # slot i of the group's j-th chain: value i * m + j
            rows[:, h0::3, p] = pl[(np.arange(N_STEPS)[:, None] * m + np.arange(m)[None, :]) % len(pl)]
    rows[:, :, 4] = rng.normal(-50, 5, (N_STEPS, n_chains))
    sign = np.where(rng.uniform(size=(N_STEPS, n_chains)) < 0.5, -1.0, 1.0)
    rows[:, :, 5] = sign * 10.0 ** rng.uniform(-300, 300, (N_STEPS, n_chains))
    return rows, boxes


def bins_of(values, e):
    """gsl_histogram_increment: counts of e[b] <= v < e[b+1]; outside [e[0], e[n]) and NaN are dropped.  By
    np.searchsorted where the edges are sorted.  GSL's formula does not always sort them ([1e15, 1e15+3] at 200
    bins has six that step back by an ulp); there "the bin" is whatever gsl_histogram_increment's bisection
    settles on, and that bisection is restated here."""
    n = len(e) - 1
    v = np.asarray(values, dtype=np.float64)
    v = v[(v >= e[0]) & (v < e[n])]
    if np.all(np.diff(e) >= 0):
        idx = np.searchsorted(e, v, side="right") - 1
        idx = np.minimum(idx, n - 1)      # (duplicates of e[n] below it: the last bin)
    else:
        idx = np.zeros(len(v), dtype=np.int64)
        for k, x in enumerate(v.tolist()):
            left, right = 0, n
            while right - left > 1:
                mid = (left + right) // 2
                if x >= e[mid]:
                    left = mid
                else:
                    right = mid
            idx[k] = left
    return np.bincount(idx, minlength=n).astype(np.uint64)


def batches_of(values, bs):
    """batch_means_error(): sample n (from 1) closes a batch when n % bs == bs - 1; sequential sums; the open
    batch's sum last"""
    out, part = [], 0.0
    for n, v in enumerate(values, 1):
        part += v
        if n % bs == bs - 1:
            out.append(part)
            part = 0.0
    return out, part


def expected(rows, boxes, nbins, bs, n_hist):
    """(n, prob_sum[c], hist[h][p][b], batch[h][p] = (closed sums, open sum)) of the kept steps of CALLS"""
    kept = rows[kept_steps()]
    n, n_chains, w = kept.shape
    prob_sum = np.zeros(n_chains)
    for c in range(n_chains):
        s = 0.0
        for v in kept[:, c, w - 1].tolist():
            s += v
        prob_sum[c] = s
    hist = np.zeros((n_hist, w - 2, nbins), dtype=np.uint64)
    batch = {}
    for p, (lo, hi) in enumerate(boxes):
        e = gsl_edges(lo, hi, nbins)
        for h in range(n_hist):
            hist[h, p] = bins_of(kept[:, h, p], e)
            batch[h, p] = batches_of(kept[:, h, p].tolist(), bs)
    return n, prob_sum, hist, batch
