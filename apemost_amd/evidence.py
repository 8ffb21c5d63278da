"""Evidence estimators from what apemost_hip_evidence_get hands out: thermodynamic integration with the rectangle,
trapezoid and variance-corrected trapezoid rules, the stepping-stone estimator in both directions, and error bars.

An Evidence holds one view (include/apemost_hip.h, apemost_hip_evidence_view) of column n_par+1 of the sample rows,
v = prob - prior = beta * loglike, for every chain c: the number of kept samples n, the moments about the first sample
(origin, sum of d = v - origin, sq = sum of d * d), the batch sums of v under batch_means_error()'s closing rule, and
for s = up, down the running log-sum-exp (m, S) of coef_s[c] * v, so that ln mean exp(coef_s v) = m + ln(S / n).  With

    coef_up[c]   =  (beta_{c-1} - beta_c) / beta_c      (0 for the coldest chain of a ladder)
    coef_down[c] = -(beta_c - beta_{c+1}) / beta_c      (-1 for the hottest: the step from beta_min to 0)

these are ln Z(beta_{c-1}) / Z(beta_c) and ln Z(beta_{c+1}) / Z(beta_c), the ratios of the stepping-stone estimator
(Xie et al. 2011) taken from the hotter and from the colder chain's samples.  The thermodynamic rules integrate
E_beta[loglike] over beta from the per-chain means; "corrected" subtracts dbeta^2 / 12 (V_colder - V_hotter) from every
trapezoid, because dE/dbeta = Var_beta[loglike] (Friel et al. 2014).

evidence.bin (little-endian), version 1; the C host's APEMOST_DUMP token `evidence` writes the same bytes:
    char[8]  "APEMOSTE"
    uint32   version, n_chains, n_ladders, 0
    uint64   n, thin, batch_size, max_batches
    double   betas[n_chains], coef_up[n_chains], coef_down[n_chains]
    double   origin[n_chains], sum[n_chains], sq[n_chains]
    double   m[2][n_chains], S[2][n_chains]                       (up, down)
    double   batch[n_chains][max_batches + 1]                     (slot n_batches: the open batch)
"""
import math
import struct

import numpy as np

from . import capi
from .summary import batch_closes, batches_closed

MAGIC = b"APEMOSTE"
VERSION = 1
_HEAD = struct.Struct("<8s4I4Q")
UP, DOWN = 0, 1


class Evidence:
    def __init__(self, n, origin, sum, sq, batch, m, S, betas, batch_size, coef_up, coef_down, n_ladders=1, thin=1):
        self.n = np.ascontiguousarray(n, dtype=np.uint64).reshape(1)
        self.betas = np.ascontiguousarray(betas, dtype=np.float64)
        nc = len(self.betas)
        self.origin = np.ascontiguousarray(origin, dtype=np.float64).reshape(nc)
        self.sum = np.ascontiguousarray(sum, dtype=np.float64).reshape(nc)
        self.sq = np.ascontiguousarray(sq, dtype=np.float64).reshape(nc)
        self.batch = np.ascontiguousarray(batch, dtype=np.float64).reshape(nc, -1)     # [c][max_batches + 1]
        self.m = np.ascontiguousarray(m, dtype=np.float64).reshape(2, nc)
        self.S = np.ascontiguousarray(S, dtype=np.float64).reshape(2, nc)
        self.coef = np.ascontiguousarray([coef_up, coef_down], dtype=np.float64).reshape(2, nc)
        self.batch_size, self.n_ladders, self.thin = int(batch_size), int(n_ladders), int(thin)
        if self.n_ladders < 1 or nc % self.n_ladders:
            raise ValueError("%d chains are not %d equal ladders" % (nc, self.n_ladders))

    @property
    def n_chains(self):
        return len(self.betas)

    @property
    def max_batches(self):
        return self.batch.shape[1] - 1

    @property
    def n_batches(self):
        return batches_closed(int(self.n[0]), self.batch_size)

    @staticmethod
    def coefficients(betas, n_ladders=1):
        """(coef_up, coef_down) of ladder-major betas, which must be positive and strictly decreasing within every
        ladder: with beta = 0 the column is identically 0 and loglike cannot be recovered from it"""
        betas = np.asarray(betas, dtype=np.float64)
        if betas.ndim != 1 or n_ladders < 1 or len(betas) == 0 or len(betas) % n_ladders:
            raise ValueError("betas must hold n_ladders equal ladders")
        per = len(betas) // n_ladders
        up, down = np.zeros(len(betas)), np.zeros(len(betas))
        for b in range(n_ladders):
            lad = betas[b * per:(b + 1) * per]
            if not (np.isfinite(lad).all() and (lad > 0).all() and (np.diff(lad) < 0).all()):
                raise ValueError("ladder %d: betas must be finite, positive and strictly decreasing" % b)
            for c in range(per):
                up[b * per + c] = (lad[c - 1] - lad[c]) / lad[c] if c > 0 else 0.0
                down[b * per + c] = -(lad[c] - lad[c + 1]) / lad[c] if c + 1 < per else -1.0
        return up, down

    @classmethod
    def empty(cls, betas, batch_size, max_batches, coef_up=None, coef_down=None, n_ladders=1, thin=1):
        betas = np.asarray(betas, dtype=np.float64)
        if coef_up is None or coef_down is None:
            coef_up, coef_down = cls.coefficients(betas, n_ladders)
        nc = len(betas)
        return cls(np.zeros(1, dtype=np.uint64), np.zeros(nc), np.zeros(nc), np.zeros(nc), np.zeros((nc, max_batches + 1)),
                   np.zeros((2, nc)), np.zeros((2, nc)), betas, batch_size, coef_up, coef_down, n_ladders, thin)

    def view(self):
        """the apemost_hip_evidence_view over this object's arrays"""
        dp = capi._dp
        return capi.EvidenceView(n=self.n.ctypes.data_as(capi._up), origin=self.origin.ctypes.data_as(dp),
                                 sum=self.sum.ctypes.data_as(dp), sq=self.sq.ctypes.data_as(dp),
                                 batch=self.batch.ctypes.data_as(dp), m=self.m.ctypes.data_as(dp),
                                 S=self.S.ctypes.data_as(dp))

    @classmethod
    def from_rows(cls, rows, betas, batch_size=1, max_batches=None, n_ladders=1, thin=1, coef_up=None, coef_down=None):
        """the fold of host sample rows [n][n_chains][n_par+2] (already thinned) or of the column itself [n][n_chains],
        with sequential host loops: what the device computes, for tests and for summaries of existing dumps"""
        rows = np.asarray(rows, dtype=np.float64)
        col = rows[:, :, -1] if rows.ndim == 3 else rows
        n, nc = col.shape
        if max_batches is None:
            max_batches = batches_closed(n, batch_size)
        ev = cls.empty(betas, batch_size, max_batches, coef_up, coef_down, n_ladders, thin)
        assert ev.n_chains == nc and batches_closed(n, batch_size) <= max_batches
        ev.n[0] = n
        if n == 0:
            return ev
        for c in range(nc):
            v = col[:, c].tolist()
            o = v[0]
            s = q = part = 0.0
            nb = 0
            for i, x in enumerate(v):
                d = x - o
                s += d
                q += d * d
                part += x
                if batch_closes(i + 1, batch_size):
                    ev.batch[c, nb] = part
                    part, nb = 0.0, nb + 1
            ev.batch[c, nb] = part
            ev.origin[c], ev.sum[c], ev.sq[c] = o, s, q
            for k in (UP, DOWN):
                a = float(ev.coef[k, c])
                m, S = a * v[0], 1.0
                for x in v[1:]:
                    x = a * x
                    if x > m:
                        S = S * _exp(m - x) + 1.0
                        m = x
                    else:
                        S += _exp(x - m)
                ev.m[k, c], ev.S[k, c] = m, S
        return ev

    # -- ladders and shards -----------------------------------------------------------------------
    def per_ladder(self, n_ladders=None):
        """one Evidence per ladder of a batch (chains ladder-major)"""
        n_ladders = self.n_ladders if n_ladders is None else n_ladders
        if n_ladders < 1 or self.n_chains % n_ladders:
            raise ValueError("%d chains are not %d equal ladders" % (self.n_chains, n_ladders))
        per = self.n_chains // n_ladders
        out = []
        for b in range(n_ladders):
            k = slice(b * per, (b + 1) * per)
            out.append(Evidence(self.n.copy(), self.origin[k], self.sum[k], self.sq[k], self.batch[k], self.m[:, k],
                                self.S[:, k], self.betas[k], self.batch_size, self.coef[UP, k], self.coef[DOWN, k], 1,
                                self.thin))
        return out

    @staticmethod
    def concat(shards):
        """the Evidence of a sharded ladder: every per-chain array concatenated in shard order (the shards were begun
        with their slices of the whole ladder's coefficients)"""
        s0 = shards[0]
        assert all(int(s.n[0]) == int(s0.n[0]) and s.batch_size == s0.batch_size and s.max_batches == s0.max_batches
                   for s in shards)
        cat = np.concatenate
        return Evidence(s0.n.copy(), cat([s.origin for s in shards]), cat([s.sum for s in shards]),
                        cat([s.sq for s in shards]), cat([s.batch for s in shards]), cat([s.m for s in shards], axis=1),
                        cat([s.S for s in shards], axis=1), cat([s.betas for s in shards]), s0.batch_size,
                        cat([s.coef[UP] for s in shards]), cat([s.coef[DOWN] for s in shards]), 1, s0.thin)

    # -- per chain --------------------------------------------------------------------------------
    def mean_loglike(self):
        """(origin + sum / n) / beta per chain"""
        with np.errstate(all="ignore"):
            return (self.origin + self.sum / np.float64(self.n[0])) / self.betas

    def var_loglike(self):
        """(sq - sum^2 / n) / (n - 1) / beta^2 per chain"""
        n = np.float64(self.n[0])
        with np.errstate(all="ignore"):
            return (self.sq - self.sum * self.sum / n) / (n - np.float64(1)) / (self.betas * self.betas)

    def mcse(self):
        """per-chain batch-means standard error of the mean of loglike: the spread of the closed batches' means about
        the chain's mean, batch_means_error()'s sqrt(sum d^2 / n_batches), divided by sqrt(n_batches).  A batch mean is
        its sum over the samples it holds (batch 0 holds batch_size - 1 of them, or 1 for batch_size 1): dividing
        batch 0 by batch_size as analyse does would shift it by mean / batch_size, which for v of the order of -10^3 is
        more than the spread being measured.  NaN with fewer than two closed batches."""
        nb, bs = self.n_batches, self.batch_size
        out = np.full(self.n_chains, np.nan)
        if nb < 2:
            return out
        counts = np.full(nb, float(bs))
        counts[0] = bs - 1 if bs > 1 else 1
        with np.errstate(all="ignore"):
            mean_v = self.origin + self.sum / np.float64(self.n[0])
            d = self.batch[:, :nb] / counts - mean_v[:, None]
            return np.sqrt((d * d).sum(axis=1) / nb) / math.sqrt(nb) / self.betas

    def ln_mean_exp(self, direction):
        """ln mean exp(coef v) = m + ln(S / n) per chain: direction "up" gives ln Z(beta_{c-1}) / Z(beta_c), "down"
        gives ln Z(beta_{c+1}) / Z(beta_c) (for the hottest chain ln Z(0) / Z(beta_min))"""
        k = {"up": UP, "down": DOWN}[direction]
        with np.errstate(all="ignore"):
            return self.m[k] + np.log(self.S[k] / np.float64(self.n[0]))

    # -- ln p(D|M,I) of one ladder ----------------------------------------------------------------
    def _one_ladder(self):
        if self.n_ladders != 1:
            raise ValueError("a batch of %d ladders: take per_ladder() first" % self.n_ladders)

    def base_term(self, base="rectangle"):
        """the piece of ln Z below beta_min: "rectangle" is E_last * beta_last, the reference's (E taken constant down
        to beta = 0); "down" is -ln mean exp(-v) on the hottest chain, the stepping stone from beta_min to 0"""
        self._one_ladder()
        if base == "rectangle":
            return float(self.mean_loglike()[-1] * self.betas[-1])
        if base == "down":
            return -float(self.ln_mean_exp("down")[-1])
        raise ValueError("base: 'rectangle' or 'down'")

    def _weights(self, rule):
        """the weight of every chain's mean loglike in the thermodynamic rule over beta_min .. beta_0"""
        b = self.betas
        w = np.zeros(self.n_chains)
        if rule == "rectangle":
            w[:-1] = b[:-1] - b[1:]
        elif rule in ("trapezoid", "corrected"):
            w[:-1] += (b[:-1] - b[1:]) / 2
            w[1:] += (b[:-1] - b[1:]) / 2
        else:
            raise ValueError("rule: 'rectangle', 'trapezoid' or 'corrected'")
        return w

    def thermodynamic(self, rule="rectangle", base="rectangle"):
        """ln p(D|M,I) by thermodynamic integration.  "rectangle": mean_j (beta_j - beta_{j+1}) from the hottest chain
        up, RunSummary.evidence restated; "trapezoid": the mean of both ends of every interval; "corrected": the
        trapezoid minus dbeta^2 / 12 (V_colder - V_hotter) per interval.  base: see base_term."""
        self._one_ladder()
        mean = self.mean_loglike().tolist()
        b = self.betas.tolist()
        var = self.var_loglike().tolist() if rule == "corrected" else None
        self._weights(rule)                                  # (refuses an unknown rule)
        total = self.base_term(base)
        for j in range(len(b) - 2, -1, -1):                  # from the hottest interval up
            db = b[j] - b[j + 1]
            if rule == "rectangle":
                total += mean[j] * db
            else:
                total += (mean[j] + mean[j + 1]) / 2 * db
                if rule == "corrected":
                    total -= db * db / 12 * (var[j] - var[j + 1])
        return total

    def stepping_stone(self, direction="up", base="down"):
        """ln p(D|M,I) as the sum of ln Z(beta_c) / Z(beta_{c+1}) over the ladder: "up" takes every ratio from the
        hotter chain's samples, ln mean exp((beta_c - beta_{c+1}) loglike) at beta_{c+1}; "down" from the colder
        chain's, -ln mean exp(-(beta_c - beta_{c+1}) loglike) at beta_c.  base: see base_term."""
        self._one_ladder()
        if direction == "up":
            steps = self.ln_mean_exp("up")[1:]
        elif direction == "down":
            steps = -self.ln_mean_exp("down")[:-1]
        else:
            raise ValueError("direction: 'up' or 'down'")
        total = self.base_term(base)
        for x in steps[::-1].tolist():
            total += x
        return total

    def error(self, rule="trapezoid", base="rectangle"):
        """the standard error of thermodynamic(rule, base) by the delta method from mcse(): sqrt(sum_c (w_c mcse_c)^2)
        with w_c the weight of chain c's mean in the rule.  The chains are treated as independent, which replica
        exchange does not make them; the variance term of "corrected" and the base "down" are taken as exact.  The
        error of the stepping-stone estimators comes from replicas (a ladder batch), not from here."""
        self._one_ladder()
        w = self._weights(rule)
        if base == "rectangle":
            w[-1] += self.betas[-1]
        elif base != "down":
            raise ValueError("base: 'rectangle' or 'down'")
        e = self.mcse()
        return float(np.sqrt(((w * e) ** 2).sum()))

    def totals(self):
        """the named totals evidence.txt ends with, in its order"""
        return [("thermodynamic_rectangle", self.thermodynamic("rectangle", "rectangle")),
                ("thermodynamic_trapezoid", self.thermodynamic("trapezoid", "rectangle")),
                ("thermodynamic_corrected", self.thermodynamic("corrected", "rectangle")),
                ("thermodynamic_corrected_base_down", self.thermodynamic("corrected", "down")),
                ("stepping_stone_up", self.stepping_stone("up", "down")),
                ("stepping_stone_down", self.stepping_stone("down", "down")),
                ("base_rectangle", self.base_term("rectangle")),
                ("base_down", self.base_term("down")),
                ("error_rectangle", self.error("rectangle")),
                ("error_trapezoid", self.error("trapezoid")),
                ("error_corrected", self.error("corrected"))]

    def text(self):
        """evidence.txt: per chain `beta mean_loglike var_loglike mcse ln_r_up ln_r_down`, "%.15e", then the totals"""
        cols = (self.betas, self.mean_loglike(), self.var_loglike(), self.mcse(), self.ln_mean_exp("up"),
                self.ln_mean_exp("down"))
        out = ["\t".join(_fmt(float(col[c])) for col in cols) + "\n" for c in range(self.n_chains)]
        out += ["%s\t%s\n" % (name, _fmt(v)) for name, v in self.totals()]
        return "".join(out)

    # -- evidence.bin -----------------------------------------------------------------------------
    def write(self, path):
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_chains, self.n_ladders, 0, int(self.n[0]), self.thin,
                               self.batch_size, self.max_batches))
            for a in (self.betas, self.coef[UP], self.coef[DOWN], self.origin, self.sum, self.sq, self.m, self.S,
                      self.batch):
                f.write(np.ascontiguousarray(a, dtype="<f8").tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        if len(raw) < _HEAD.size:
            raise ValueError("%s: not an evidence file" % path)
        magic, version, nc, n_ladders, _, n, thin, bs, max_batches = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not an evidence file of version %d" % (path, VERSION))
        want = _HEAD.size + 8 * (nc * 6 + 4 * nc + nc * (max_batches + 1))
        if want != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), want))
        off = _HEAD.size

        def take(count):
            nonlocal off
            a = np.frombuffer(raw, dtype="<f8", count=count, offset=off)
            off += 8 * count
            return a.copy()
        betas, up, down = take(nc), take(nc), take(nc)
        origin, total, sq = take(nc), take(nc), take(nc)
        m, S = take(2 * nc), take(2 * nc)
        batch = take(nc * (max_batches + 1))
        return cls([n], origin, total, sq, batch, m, S, betas, bs, up, down, n_ladders, thin)


def _exp(x):
    try:
        return math.exp(x)
    except OverflowError:                                    # (never for x <= 0; a non-finite column)
        return math.inf


def _fmt(v):
    return "nan" if v != v else "%.15e" % v
