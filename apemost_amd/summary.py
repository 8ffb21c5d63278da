"""Run summaries: what the `analyse` phase prints, from running sums instead of sample dumps.

A RunSummary holds what apemost_hip_summary_get hands out (include/apemost_hip.h): the number of kept
samples, per chain the sum of prob - prior, and per histogram chain and parameter the bin counts of
marginal_distribution() and the batch sums of batch_means_error() (apemost_amd/host/src/analyse.c).
From them it computes the model evidence, the marginal densities and the batch-means error exactly as
`analyse` does from the text dumps, and it reads and writes `summary.bin`, the file the C host's run
phase leaves with APEMOST_DUMP=summary.

summary.bin (little-endian), version 1:
    char[8]  "APEMOSTS"
    uint32   version, n_beta, n_par, nbins
    uint64   thin, batch_size
    uint32   n_hist_chains, 0
    uint64   n, n_batches, max_batches
    double   lo[n_par], hi[n_par]
    double   prob_sum[n_beta]
    uint64   hist[n_hist_chains][n_par][nbins]
    double   batch_sums[n_hist_chains][n_par][max_batches + 1]   (slot n_batches: the open batch)
"""
import math
import struct

import numpy as np

MAGIC = b"APEMOSTS"
VERSION = 1
_HEAD = struct.Struct("<8s4I2Q2I3Q")


def batch_closes(n, bs):
    """batch_means_error(): sample n (counted from 1) closes a batch when n % bs == bs - 1"""
    return n % bs == bs - 1


def batches_closed(n_samples, bs):
    """batches batch_means_error() counts after n_samples samples (the incomplete tail is not one)"""
    return n_samples if bs == 1 else (n_samples + 1) // bs


def batch_index(i, bs):
    """batch of the sample with 0-based index i: batch 0 holds bs - 1 samples, every later one bs
    (for bs = 1 every sample is a batch of its own)"""
    return batches_closed(i, bs)


def batch_size_for(n_samples):
    """the batch size analyse uses for n_samples histogrammed values: (unsigned long)sqrt(total)"""
    return int(math.sqrt(float(n_samples)))


def edges(lo, hi, nbins):
    """marginal_distribution()'s bin edges, which are the reference's create_hist(): GSL's
    gsl_histogram_set_ranges_uniform, ((n-b)/n)*lo + (b/n)*hi, the top one widened by (hi-lo)/10000"""
    e = [((nbins - b) / nbins) * lo + (b / nbins) * hi for b in range(nbins + 1)]
    e[nbins] += (hi - lo) / 10000
    return np.array(e)


def bin_of(v, lo, hi, e):
    """gsl_histogram_increment's bin of v over the edges e (bin b holds e[b] <= v < e[b+1]), or -1 outside
    [e[0], e[nbins]) (NaN included): a bisection, as in the host's gslcompat.c"""
    left, right = 0, len(e) - 1
    if not (v >= e[0] and v < e[right]):
        return -1
    while right - left > 1:
        mid = (left + right) // 2
        if v >= e[mid]:
            left = mid
        else:
            right = mid
    return left


def gelman_rubin(rows, n_ladders, chain=0):
    """R-hat per parameter (Gelman & Rubin 1992, the classic between/within form) of chain `chain` (0: beta = 1)
    of every ladder of a replica batch.  rows: sample rows [n][n_ladders * n_chains][n_par + 2], ladder-major, already
    cut to the part to judge (burn-in dropped).  With m = n_ladders sequences of n draws: W = the mean of the
    sequences' sample variances, B / n = the sample variance of their means, var+ = (n - 1) / n * W + B / n,
    R-hat = sqrt(var+ / W)."""
    rows = np.asarray(rows, dtype=np.float64)
    n, total, w = rows.shape
    if n_ladders < 2 or total % n_ladders or n < 2:
        raise ValueError("gelman_rubin needs at least two ladders of equal size and two samples")
    per = total // n_ladders
    if not 0 <= chain < per:
        raise ValueError("chain %d outside a ladder of %d chains" % (chain, per))
    x = rows[:, chain::per, :w - 2]                   # [n][m][n_par]
    within = x.var(axis=0, ddof=1).mean(axis=0)       # W
    b_over_n = x.mean(axis=0).var(axis=0, ddof=1)     # B / n
    return np.sqrt(((n - 1) / n * within + b_over_n) / within)


def ladder_evidences(prob_sum, n, betas, n_ladders):
    """ln p(D|M,I) of every ladder of a batch from a summary's ladder-major prob_sum and betas (RunSummary.evidence,
    the integrator of analyse_data_probability, ladder by ladder): the spread over replicas is its error bar"""
    prob_sum, betas = np.asarray(prob_sum, dtype=np.float64), np.asarray(betas, dtype=np.float64)
    if n_ladders < 1 or len(prob_sum) % n_ladders or len(betas) != len(prob_sum):
        raise ValueError("prob_sum and betas must hold n_ladders equal ladders")
    per = len(prob_sum) // n_ladders
    empty = np.zeros((0, 0, 0))
    return np.array([RunSummary(n, prob_sum[b * per:(b + 1) * per], empty, empty, 0, [], [], 1).evidence(
        betas[b * per:(b + 1) * per]) for b in range(n_ladders)])


class RunSummary:
    def __init__(self, n, prob_sum, hist, batch_sums, n_batches, lo, hi, batch_size, thin=1):
        self.n = int(n)
        self.prob_sum = np.asarray(prob_sum, dtype=np.float64)
        self.hist = np.asarray(hist, dtype=np.uint64)                # [h][p][nbins]
        self.batch_sums = np.asarray(batch_sums, dtype=np.float64)   # [h][p][max_batches + 1]
        self.n_batches = int(n_batches)
        self.lo = np.asarray(lo, dtype=np.float64)
        self.hi = np.asarray(hi, dtype=np.float64)
        self.batch_size = int(batch_size)
        self.thin = int(thin)

    @property
    def n_hist_chains(self):
        return self.hist.shape[0]

    @property
    def n_par(self):
        return len(self.lo)

    @property
    def nbins(self):
        return self.hist.shape[2]

    @property
    def max_batches(self):
        return self.batch_sums.shape[2] - 1

    @classmethod
    def from_rows(cls, rows, n_hist_chains, nbins, batch_size, max_batches, lo, hi, thin=1):
        """the summary of host sample rows [n][n_chains][n_par+2] (already thinned), with the host loops of
        analyse.c: what the device computes, for tests and for summaries of existing dumps"""
        rows = np.asarray(rows, dtype=np.float64)
        n, n_chains, w = rows.shape
        n_par = w - 2
        prob_sum = np.zeros(n_chains)
        for c in range(n_chains):
            s = 0.0
            for v in rows[:, c, n_par + 1].tolist():
                s += v
            prob_sum[c] = s
        hist = np.zeros((n_hist_chains, n_par, nbins), dtype=np.uint64)
        batch = np.zeros((n_hist_chains, n_par, max_batches + 1))
        for h in range(n_hist_chains):
            for p in range(n_par):
                e = edges(float(lo[p]), float(hi[p]), nbins).tolist()
                part, nb = 0.0, 0
                for i, v in enumerate(rows[:, h, p].tolist()):
                    b = bin_of(v, float(lo[p]), float(hi[p]), e)
                    if b >= 0:
                        hist[h, p, b] += 1
                    part += v
                    if batch_closes(i + 1, batch_size):
                        batch[h, p, nb] = part
                        part, nb = 0.0, nb + 1
                batch[h, p, nb] = part
        return cls(n, prob_sum, hist, batch, batches_closed(n, batch_size), lo, hi, batch_size, thin)

    @staticmethod
    def concat(shards):
        """the summary of a sharded ladder: prob_sum concatenated, the rest from shard 0 (chain 0's)"""
        s0 = shards[0]
        assert all(s.n == s0.n for s in shards)
        return RunSummary(s0.n, np.concatenate([s.prob_sum for s in shards]), s0.hist, s0.batch_sums, s0.n_batches,
                          s0.lo, s0.hi, s0.batch_size, s0.thin)

    # -- what analyse prints -----------------------------------------------------------
    def evidence(self, betas):
        """ln p(D|M,I): per chain mean(prob - prior) / beta, rectangle rule from the hottest chain to beta = 1
        (analyse_data_probability)"""
        betas = [float(b) for b in betas]
        mean = [float(s) / b / self.n for s, b in zip(self.prob_sum.tolist(), betas)]
        logprob, previous = 0.0, 0.0
        for j in range(len(betas) - 1, -1, -1):
            logprob += mean[j] * (betas[j] - previous)
            previous = betas[j]
        return logprob

    def evidence_per_ladder(self, betas, n_ladders):
        """evidence() of every ladder of a batch (prob_sum and betas ladder-major)"""
        return ladder_evidences(self.prob_sum, self.n, betas, n_ladders)

    def histogram_density(self, p, h=0):
        """(edges, density, mean, sigma) of parameter p of chain h: counts * width / total (gsl_histogram_scale), and
        the mean and standard deviation of the bin centres by the running recurrences of gsl_histogram_mean and
        gsl_histogram_sigma, operation for operation"""
        lo, hi = float(self.lo[p]), float(self.hi[p])
        e = edges(lo, hi, self.nbins)
        counts = self.hist[h, p].astype(np.float64).tolist()
        total = 0.0
        for c in counts:
            total += c
        width = (hi - lo) / self.nbins
        dens = [c * (width / total) for c in counts]
        el = e.tolist()
        wsum = mean = 0.0
        for b in range(self.nbins):
            if dens[b] > 0:
                wsum += dens[b]
                mean += ((el[b + 1] + el[b]) / 2 - mean) * (dens[b] / wsum)
        wsum = var = 0.0
        for b in range(self.nbins):
            if dens[b] > 0:
                d = (el[b + 1] + el[b]) / 2 - mean
                wsum += dens[b]
                var += (d * d - var) * (dens[b] / wsum)
        return e, np.array(dens), mean, math.sqrt(var)

    def batch_means_error(self, p, h=0, mean=None):
        """batch_means_error() over the closed batches with this summary's batch size; mean defaults to the
        histogram's"""
        if mean is None:
            mean = self.histogram_density(p, h)[2]
        errorsum = 0.0
        for s in self.batch_sums[h, p, :self.n_batches].tolist():
            d = s / self.batch_size - mean
            errorsum += d * d
        return math.sqrt(errorsum / self.n_batches) if self.n_batches else float("nan")

    # -- summary.bin ---------------------------------------------------------------------
    def write(self, path, n_beta=None):
        n_beta = len(self.prob_sum) if n_beta is None else n_beta
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, n_beta, self.n_par, self.nbins, self.thin, self.batch_size,
                               self.n_hist_chains, 0, self.n, self.n_batches, self.max_batches))
            for a, t in ((self.lo, "<f8"), (self.hi, "<f8"), (self.prob_sum, "<f8"), (self.hist, "<u8"),
                         (self.batch_sums, "<f8")):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        (magic, version, n_beta, n_par, nbins, thin, bs, n_hist, _, n, n_batches,
         max_batches) = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a summary file of version %d" % (path, VERSION))
        off = _HEAD.size

        def take(count, dtype):
            nonlocal off
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=off)
            off += 8 * count
            return a.copy()
        lo, hi = take(n_par, "<f8"), take(n_par, "<f8")
        prob_sum = take(n_beta, "<f8")
        hist = take(n_hist * n_par * nbins, "<u8").reshape(n_hist, n_par, nbins)
        batch = take(n_hist * n_par * (max_batches + 1), "<f8").reshape(n_hist, n_par, max_batches + 1)
        if off != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), off))
        return cls(n, prob_sum, hist, batch, n_batches, lo, hi, bs, thin)
