"""Replica flow of one ladder: what APEMOST_HIP_FLAG_TRACK_REPLICAS counts on the device (the specification is at
the flag in include/apemost_hip.h), with the figures a tempering ladder is judged and re-spaced by.  numpy only.

Rung a is chain a of the ladder (0 = the beta = 1 end).  Pair a is (a, a + 1); its figures sit at index a and the
entry of the last rung is not a pair (swap_rate and rejection are NaN there)."""
import numpy as np

# the arrays that cross the C ABI (apemost_hip_replica_flow_view), in its order
FIELDS = (("replica", np.uint32), ("heading", np.uint32), ("n_up", np.uint64), ("n_down", np.uint64),
          ("attempts", np.uint64), ("round_trips", np.uint64))
HEADING_NONE, HEADING_FROM_BOTTOM, HEADING_FROM_TOP = 0, 1, 2


def initial(n):
    """(replica, heading) of a ladder of n rungs before its first swap attempt"""
    replica = np.arange(n, dtype=np.uint32)
    heading = np.zeros(n, dtype=np.uint32)
    if n > 1:
        heading[0], heading[n - 1] = HEADING_FROM_BOTTOM, HEADING_FROM_TOP
    return replica, heading


class ReplicaFlow:
    def __init__(self, replica, heading, n_up, n_down, attempts, round_trips, swapcount=None, beta=None):
        n = len(replica)
        for (k, t), v in zip(FIELDS, (replica, heading, n_up, n_down, attempts, round_trips)):
            a = np.array(v, dtype=t)
            if a.shape != (n,):
                raise ValueError("%s: %d entries for a ladder of %d rungs" % (k, a.size, n))
            setattr(self, k, a)
        self.swapcount = None if swapcount is None else np.array(swapcount, dtype=np.uint64)
        self.beta = None if beta is None else np.array(beta, dtype=np.float64)

    def __len__(self):
        return len(self.replica)

    # -- per pair ----------------------------------------------------------------------------
    @property
    def swap_rate(self):
        """swapcount[a] / attempts[a] of pair a; NaN for a pair without attempts and at the last rung"""
        if self.swapcount is None:
            raise ValueError("swap_rate needs the chains' swapcount")
        att = self.attempts.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            rate = np.where(att > 0, self.swapcount.astype(np.float64) / att, np.nan)
        if len(rate):
            rate[-1] = np.nan
        return rate

    @property
    def rejection(self):
        return 1.0 - self.swap_rate

    @property
    def barrier(self):
        """the sum of the pairs' rejections (the communication barrier of Syed et al. 2019); pairs without attempts
        are left out"""
        return float(np.nansum(self.rejection[:-1]))

    # -- per rung ----------------------------------------------------------------------------
    @property
    def up_fraction(self):
        """n_up / (n_up + n_down): of the replicas met at this rung, the share that last visited the bottom end
        (Katzgraber et al. 2006: a straight line from 1 at rung 0 to 0 at the top is the ladder to aim for); NaN
        where both are 0"""
        up, down = self.n_up.astype(np.float64), self.n_down.astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return np.where(up + down > 0, up / (up + down), np.nan)

    def round_trip_rate(self, n_rounds):
        """round trips of all replicas per round"""
        return float(self.round_trips.sum()) / n_rounds

    # -- re-spacing --------------------------------------------------------------------------
    def suggest_betas(self, betas=None, n=None):
        """a ladder of n betas (default: as many as now) with equal rejection between neighbours, from the
        rejections measured on the ladder `betas` (default: self.beta).  The cumulative rejection Lambda at rung a
        is the sum of the rejections of the pairs below it; Lambda is interpolated piecewise linearly as a function
        of beta along the ladder, and the new beta_k sit at Lambda = k * Lambda_total / (n - 1).  The two end betas
        are kept exactly.  Pairs without attempts take the mean rejection of the others (1 if there are none).  A
        rejection below 1e-9 counts as 1e-9, so that Lambda rises strictly and the result is strictly monotone."""
        betas = np.array(self.beta if betas is None else betas, dtype=np.float64)
        m = len(betas)
        if m != len(self) or m < 2:
            raise ValueError("suggest_betas: %d betas for a ladder of %d rungs (at least 2)" % (m, len(self)))
        n = m if n is None else int(n)
        if n < 2:
            raise ValueError("suggest_betas: a ladder needs two ends")
        rej = self.rejection[:-1].copy()
        known = ~np.isnan(rej)
        rej[~known] = rej[known].mean() if known.any() else 1.0
        rej = np.maximum(rej, 1e-9)
        lam = np.concatenate([[0.0], np.cumsum(rej)])
        out = np.interp(np.arange(n) * (lam[-1] / (n - 1)), lam, betas)
        out[0], out[-1] = betas[0], betas[-1]
        return out

    # -- the dump file: one line per rung, then one per replica ------------------------------
    def write(self, path):
        """replica_flow.dump: per rung "beta replica heading attempts swapcount n_up n_down" (tabs; beta as %.17g),
        then per replica its round trips"""
        beta = np.zeros(len(self)) if self.beta is None else self.beta
        swapcount = np.zeros(len(self), dtype=np.uint64) if self.swapcount is None else self.swapcount
        with open(path, "w") as f:
            for a in range(len(self)):
                f.write("%.17g\t%d\t%d\t%d\t%d\t%d\t%d\n" % (beta[a], self.replica[a], self.heading[a], self.attempts[a],
                                                            swapcount[a], self.n_up[a], self.n_down[a]))
            for label in range(len(self)):
                f.write("%d\n" % self.round_trips[label])

    @classmethod
    def read(cls, path):
        rows = [line.split() for line in open(path) if line.strip()]
        if len(rows) % 2 or any(len(r) != 7 for r in rows[:len(rows) // 2]) or any(len(r) != 1 for r in rows[len(rows) // 2:]):
            raise ValueError("%s is not a replica flow dump" % path)
        n = len(rows) // 2
        rung = rows[:n]
        col = lambda j: [int(r[j]) for r in rung]
        return cls(replica=col(1), heading=col(2), attempts=col(3), swapcount=col(4), n_up=col(5), n_down=col(6),
                   round_trips=[int(r[0]) for r in rows[n:]], beta=[float(r[0]) for r in rung])

    def __eq__(self, other):
        if not isinstance(other, ReplicaFlow):
            return NotImplemented
        same = all(np.array_equal(getattr(self, k), getattr(other, k)) for k, _ in FIELDS)
        for k in ("swapcount", "beta"):
            a, b = getattr(self, k), getattr(other, k)
            same = same and ((a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b)))
        return same

    __hash__ = None
