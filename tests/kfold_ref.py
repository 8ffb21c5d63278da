"""A restatement of the joint predictive of a block (apemost_amd/csrc/pt_pointwise_joint.h; include/apemost_hip.h,
apemost_hip_pointwise_begin_at with joint = 1) that shares nothing with the kernels or with apemost_amd/kfold.py.

joint_sum is the two-stage sum of the rule: 64 lane partials, each from +0.0 over the terms i = j, j + 64, ... in
ascending order, then the adjacent-pairs tree taken six times.  numpy adds two float64 arrays element by element with
one IEEE rounding each, so both stages are stated with whole-array additions.  RefJoint folds J_t one sample after the
other in Python, with math.exp, and keeps beside its sequential S the sum of the exponentials about the final maximum
taken without summation error (math.fsum), which the comparison rule of tests/test_gpu_evidence.py needs.  Test
infrastructure only."""
import math

import numpy as np

LANES = 64


def joint_sum(terms):
    """J of the terms [..., L]: an array of the leading shape (a float for one block)"""
    terms = np.asarray(terms, dtype=np.float64)
    L = terms.shape[-1]
    p = np.zeros(terms.shape[:-1] + (LANES,))
    with np.errstate(all="ignore"):
        for i0 in range(0, L, LANES):
            chunk = terms[..., i0:i0 + LANES]
            m = chunk.shape[-1]
            p[..., :m] = p[..., :m] + chunk
        for _ in range(6):
            p = p[..., 0::2] + p[..., 1::2]
    out = p[..., 0]
    return float(out) if out.ndim == 0 else out


def exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


class RefJoint:
    """origin, sum, sq, m, S of the samples J [n] of one kept chain, folded sequentially; S_exact: math.fsum of the
    exponentials about the final maximum (0.0 where a sample is not finite)"""

    def __init__(self, J):
        J = [float(v) for v in np.asarray(J, dtype=np.float64).reshape(-1).tolist()]
        self.n = len(J)
        self.origin = self.sum = self.sq = self.m = self.S = self.S_exact = 0.0
        self.finite = True
        if not J:
            return
        origin = J[0]
        total = sq = 0.0
        m, S = origin, 1.0
        for t, v in enumerate(J):
            d = v - origin
            total = total + d
            dd = d * d
            sq = sq + dd
            if t == 0:
                continue
            if v > m:
                S = S * exp(m - v) + 1.0
                m = v
            else:
                S = S + exp(v - m)
        self.origin, self.sum, self.sq, self.m, self.S = origin, total, sq, m, S
        self.finite = all(math.isfinite(v) for v in J)
        if self.finite:
            self.S_exact = math.fsum(exp(v - m) for v in J)

    def lpd(self):
        return self.m + math.log(self.S / self.n)
