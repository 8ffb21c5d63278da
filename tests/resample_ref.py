"""Systematic resampling with an integer offset, restated in Python integers: the reference of
apemost_amd.reweight.systematic_positions, Reweight.resample_numpy and apemost_hip_reweight_resample.  Shares nothing
with apemost_amd/reweight.py.  With the integer weights q_0 .. q_{N-1}, M draws and the uint64 u:

    C_n = q_0 + ... + q_n,  Q = C_{N-1};   a = Q div M,  b = Q mod M,  o = (u a) div 2^64
    p_m = m a + (m b) div M + o;   draw m is the smallest n with C_n > p_m  (bisect_right over the list of C)"""
import bisect


def positions(Q, M, u):
    """[p_0 .. p_{M-1}], Python integers"""
    assert 1 <= M <= Q and 0 <= u < 1 << 64
    a, b = divmod(Q, M)
    o = (u * a) >> 64
    return [m * a + (m * b) // M + o for m in range(M)]


def cumulative(q):
    out, run = [], 0
    for v in q:
        run += int(v)
        out.append(run)
    return out


def draws(q, M, u):
    """(index [M], Q) of the integer weights q (any sequence of integers, in stored order)"""
    C = cumulative(q)
    return [bisect.bisect_right(C, p) for p in positions(C[-1], M, u)], C[-1]


def counts(index, N):
    out = [0] * N
    for n in index:
        out[n] += 1
    return out


def check_rule(q, index, M, u):
    """what the rule promises of any correct index: p non-decreasing and below Q, the draws in stored order, no sample
    of weight zero drawn, and every sample drawn floor(M q / Q) or ceil(M q / Q) times: |count Q - M q| < Q"""
    q = [int(v) for v in q]
    Q = sum(q)
    p = positions(Q, M, u)
    assert all(lo <= hi for lo, hi in zip(p, p[1:])) and 0 <= p[0] and p[-1] < Q
    index = [int(n) for n in index]
    assert len(index) == M and all(lo <= hi for lo, hi in zip(index, index[1:]))
    for n, c in enumerate(counts(index, len(q))):
        assert abs(c * Q - M * q[n]) < Q, (n, c, q[n])
        assert q[n] > 0 or c == 0, n
