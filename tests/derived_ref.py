"""A plain restatement of what the derived-quantity fold (pt_derived.h) must compute, which shares nothing with the
kernels or with apemost_amd/derived.py: an interpreter of the column programs on Python floats, one row at a time, and
sequential Python loops for the fold.  Bins come from tests/summary_rows.gsl_edges through tests/joint_ref, the joint
part is tests/joint_ref.RefJoint over the computed columns.  Also: a seeded generator of valid random programs from
the exact group, and the fixed argument lists and error bounds of the library group.  Test infrastructure only."""
import math

import numpy as np

from tests.joint_ref import RefJoint, assert_equals, bin_indices, same_floats
from tests.summary_rows import BOX_SETS, batches_of, gsl_edges, pool

# include/apemost_hip.h, restated
(COL, CONST, DUP, SWAP, ADD, SUB, MUL, DIV, NEG, ABS, INV, SQRT, FLOOR, MIN, MAX, LOG, EXP, SIN, COS,
 ATAN2) = range(20)
MAX_DEPTH, MAX_CODE = 16, 256
POPS_PUSHES = {COL: (0, 1), CONST: (0, 1), DUP: (1, 2), SWAP: (2, 2), ADD: (2, 1), SUB: (2, 1), MUL: (2, 1), DIV: (2, 1),
               NEG: (1, 1), ABS: (1, 1), INV: (1, 1), SQRT: (1, 1), FLOOR: (1, 1), MIN: (2, 1), MAX: (2, 1), LOG: (1, 1),
               EXP: (1, 1), SIN: (1, 1), COS: (1, 1), ATAN2: (2, 1)}


def word(op, operand=0):
    return op | (operand << 8)


# ---- IEEE fp64 on Python floats, where Python raises or returns an int instead ------------------------------------------
def _div(a, b):
    if b != 0:
        return a / b
    if a != a or a == 0:
        return math.nan
    return math.copysign(math.inf, a) * math.copysign(1.0, b)


def _sqrt(a):
    return math.sqrt(a) if a >= 0 else (math.nan if a == a else a)      # (sqrt(-0.0) is -0.0, which math.sqrt gives)


def _floor(a):
    if a != a or math.isinf(a) or a == 0:
        return a
    r = float(math.floor(a))
    return r if r != 0 else math.copysign(0.0, a)


def run(code, consts, x):
    """the value of one program for the row x (a list of Python floats); exact group only"""
    st = []
    for w in code:
        op, arg = w & 255, w >> 8
        if op == COL:
            st.append(x[arg])
        elif op == CONST:
            st.append(consts[arg])
        elif op == DUP:
            st.append(st[-1])
        elif op == SWAP:
            st[-1], st[-2] = st[-2], st[-1]
        elif op in (NEG, ABS, INV, SQRT, FLOOR):
            t = st.pop()
            st.append(-t if op == NEG else math.fabs(t) if op == ABS else _div(1.0, t) if op == INV else
                      _sqrt(t) if op == SQRT else _floor(t))
        elif op in (ADD, SUB, MUL, DIV, MIN, MAX):
            t = st.pop()
            b = st.pop()
            st.append(b + t if op == ADD else b - t if op == SUB else b * t if op == MUL else _div(b, t) if op == DIV else
                      (b if b < t else t) if op == MIN else (b if b > t else t))
        else:
            raise ValueError("opcode %d is not of the exact group" % op)
    assert len(st) == 1
    return st[0]


def values(programs, rows):
    """[n][n_col] of rows [n][w]; programs: (code, consts) pairs"""
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros((len(rows), len(programs)))
    for i, x in enumerate(rows.tolist()):
        for c, (code, consts) in enumerate(programs):
            out[i, c] = run(code, consts, x)
    return out


# ---- random programs of the exact group -----------------------------------------------------------------------------
_WEIGHTS = {ADD: 6, SUB: 6, MUL: 4, DIV: 2, MIN: 3, MAX: 3, NEG: 2, ABS: 3, INV: 1, SQRT: 1, FLOOR: 2, SWAP: 2, DUP: 2,
            COL: 5, CONST: 3}
CONST_POOL = [0.0, -0.0, 1.0, -1.0, 0.5, 2.0, 3.0, 1e-3, 7.25, -13.5, 1e10, 1e-10, 0.1, 1.0 / 3.0, 1e300, 5e-324]


def random_program(rng, n_par, length, want_depth):
    """(code, consts): `length` instructions of the exact group that reach stack depth `want_depth` and leave one
    value.  Needs length >= 2 want_depth - 1."""
    assert 1 <= want_depth <= MAX_DEPTH and 2 * want_depth - 1 <= length <= MAX_CODE
    consts = [CONST_POOL[i] for i in rng.permutation(len(CONST_POOL))[:8].tolist()]
    code, depth, reached = [], 0, False
    for i in range(length):
        rem = length - i - 1
        ok = []
        for op, wgt in _WEIGHTS.items():
            pops, pushes = POPS_PUSHES[op]
            after = depth + pushes - pops
            if pops <= depth and 1 <= after <= MAX_DEPTH and after - 1 <= rem:
                ok.append((op, wgt))
        if not reached and depth < want_depth:
            up = [(op, wgt) for op, wgt in ok if op in (COL, CONST, DUP)]
            if up:                     # (always possible: the pushes come first and length >= 2 want_depth - 1)
                ok = up
        ops = [op for op, _ in ok]
        p = np.array([wgt for _, wgt in ok], dtype=np.float64)
        op = ops[int(rng.choice(len(ops), p=p / p.sum()))]
        arg = int(rng.integers(0, n_par + 2)) if op == COL else int(rng.integers(0, len(consts))) if op == CONST else 0
        code.append(word(op, arg))
        depth += POPS_PUSHES[op][1] - POPS_PUSHES[op][0]
        reached = reached or depth >= want_depth
    assert depth == 1 and reached, (depth, reached)
    return code, consts


def depth_of(code):
    depth = deepest = 0
    for w in code:
        pops, pushes = POPS_PUSHES[w & 255]
        assert depth >= pops
        depth += pushes - pops
        deepest = max(deepest, depth)
    return deepest


def random_programs(seed, count, n_par):
    """`count` programs: the first of depth 16, the second of 256 instructions (and depth 16), the rest of mixed
    lengths and depths; every opcode of the exact group occurs among them"""
    rng = np.random.default_rng(seed)
    out = [random_program(rng, n_par, 40, 16), random_program(rng, n_par, 256, 16)]
    while len(out) < count:
        depth = int(rng.integers(1, MAX_DEPTH + 1))
        out.append(random_program(rng, n_par, int(rng.integers(2 * depth - 1, 97)), depth))
    seen = {w & 255 for code, _ in out for w in code}
    assert seen == set(_WEIGHTS), sorted(set(_WEIGHTS) - seen)
    return out


# ---- the library group: fixed arguments, and the error bounds measured on the card ----------------------------------
def library_arguments():
    """{name: (a,) or (y, x)}: the argument lists of the five library functions"""
    rng = np.random.default_rng(2024)
    big = 10.0 ** rng.uniform(0.5, 6.0, 1500) * np.where(rng.uniform(size=1500) < 0.5, -1.0, 1.0)
    circle = np.concatenate([np.linspace(-math.pi, math.pi, 2001), rng.uniform(-math.pi, math.pi, 1000), big,
                             [1e6, -1e6, 0.0, -0.0, 5e-324, 1e-300]])
    zeros_and_signs = [0.0, -0.0, 1.0, -1.0, 5e-324, -5e-324, 1e300, -1e300, 2.5, -2.5]
    yy, xx = np.meshgrid(zeros_and_signs, zeros_and_signs, indexing="ij")
    gy = 10.0 ** rng.uniform(-300, 300, 2000) * np.where(rng.uniform(size=2000) < 0.5, -1.0, 1.0)
    gx = 10.0 ** rng.uniform(-300, 300, 2000) * np.where(rng.uniform(size=2000) < 0.5, -1.0, 1.0)
    near = 10.0 ** rng.uniform(-3, 3, 2000)
    return {
        "log": (np.concatenate([10.0 ** np.linspace(-300, 300, 2401), rng.uniform(0.5, 2.0, 1000), [1.0, 5e-324]]),),
        "exp": (np.concatenate([np.linspace(-700, 700, 2801), rng.uniform(-1, 1, 1000), [0.0, -0.0, 1e-300]]),),
        "sin": (circle,),
        "cos": (circle,),
        "atan2": (np.concatenate([yy.ravel(), gy, near * rng.uniform(0.5, 2.0, 2000)]),
                  np.concatenate([xx.ravel(), gx, near * np.where(rng.uniform(size=2000) < 0.5, -1.0, 1.0)])),
    }


def ulp_errors(name, args, got):
    """the error of every result in ulps of the true value, by mpmath at 300 bits.  Where the true value is zero the
    result must be that zero, sign included (an error of 0, else inf)."""
    import mpmath
    mpmath.mp.prec = 300
    f = {"log": mpmath.log, "exp": mpmath.exp, "sin": mpmath.sin, "cos": mpmath.cos, "atan2": mpmath.atan2}[name]
    out = np.zeros(len(got))
    cols = [a.tolist() for a in args]
    for i, g in enumerate(np.asarray(got, dtype=np.float64).tolist()):
        a = [c[i] for c in cols]
        if name == "atan2" and a[0] == 0:
            # (mpmath knows no signed zero) atan2(+-0, x): +-0 for x > 0 or +0, +-pi for x < 0 or -0
            positive = math.copysign(1.0, a[1]) > 0
            true = mpmath.mpf(0) if positive else mpmath.pi
            sign = math.copysign(1.0, a[0])
            if positive:
                out[i] = 0.0 if (g == 0 and math.copysign(1.0, g) == sign) else math.inf
                continue
            true = true * sign
        else:
            true = f(*[mpmath.mpf(v) for v in a])
        if true == 0:
            out[i] = 0.0 if (g == 0 and math.copysign(1.0, g) == math.copysign(1.0, a[0])) else math.inf
            continue
        nearest = float(true)
        if math.isinf(nearest) or g != g or math.isinf(g):
            out[i] = 0.0 if g == nearest else math.inf
            continue
        ulp = math.ulp(nearest) if nearest != 0 else 5e-324
        out[i] = float(abs(mpmath.mpf(g) - true) / mpmath.mpf(ulp))
    return out


# Largest error measured on an MI355X (the device library of ROCm) over library_arguments(), in ulps of the true value.
# The bound is the next integer above the measured value plus one, so that a device-library update that moves one
# rounding does not fail the suite: 2 ulp for log, exp, sin and cos, 3 ulp for atan2.
LIBRARY_MEASURED_ULP = {"log": 0.613050, "exp": 0.783615, "sin": 0.730244, "cos": 0.695383, "atan2": 1.406762}
LIBRARY_BOUND_ULP = {k: math.floor(v) + 2 for k, v in LIBRARY_MEASURED_ULP.items()}


# ---- the fold -----------------------------------------------------------------------------------------------------------
def _lesser(a, b):
    return b if (b < a or (b == a and math.copysign(1.0, b) < 0)) else a


def _greater(a, b):
    return b if (b > a or (b == a and math.copysign(1.0, b) > 0)) else a


class RefDerived:
    """vals [n][n_chains][n_col], the computed columns of the kept rows, already thinned; boxes: (lo, hi) per column"""

    def __init__(self, vals, boxes, chains, nbins, bs, pairs):
        vals = np.asarray(vals, dtype=np.float64)
        n, n_chains, n_col = vals.shape
        as_rows = np.zeros((n, n_chains, n_col + 2))
        as_rows[:, :, :n_col] = vals
        self.joint = RefJoint(as_rows, boxes, chains, nbins, pairs)
        self.n = n
        self.hist = np.zeros((len(chains), n_col, nbins), dtype=np.uint64)
        self.batch = {}
        self.nonfinite = np.zeros((len(chains), n_col), dtype=np.uint64)
        self.vmin = np.full((len(chains), n_col), np.inf)
        self.vmax = np.full((len(chains), n_col), -np.inf)
        for k, ch in enumerate(chains):
            for c in range(n_col):
                col = vals[:, ch, c]
                idx = bin_indices(col, gsl_edges(boxes[c][0], boxes[c][1], nbins))
                for b in idx.tolist():
                    if b >= 0:
                        self.hist[k, c, b] += 1
                self.batch[k, c] = batches_of(col.tolist(), bs)
                mn, mx, bad = math.inf, -math.inf, 0
                for v in col.tolist():
                    if v == v:
                        mn, mx = _lesser(mn, v), _greater(mx, v)
                    if v != v or math.isinf(v):
                        bad += 1
                self.vmin[k, c], self.vmax[k, c], self.nonfinite[k, c] = mn, mx, bad


# ---- what the CPU and the GPU tests share ---------------------------------------------------------------------------------
def special_rows(n=512, seed=3):
    """[n][6]: the pool values of tests/summary_rows.py (every edge's neighbours, subnormals, both zeros, infinities
    and NaNs by position) shuffled over the columns, and ordinary values between them"""
    rng = np.random.default_rng(seed)
    drawn = np.concatenate([pool(lo, hi, 37, False, rng) for lo, hi in BOX_SETS["A"] + BOX_SETS["B"]])
    rows = rng.normal(0.0, 3.0, (n, 6))
    mask = rng.uniform(size=(n, 6)) < 0.5
    rows[mask] = drawn[rng.integers(0, len(drawn), int(mask.sum()))]
    special = (np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308)
    for j, v in enumerate(special * 6):                      # each of them in every column
        rows[(5 * j + 1) % n, j % 6 if j < 8 else (j // 8 + j) % 6] = v
    for v in (np.inf, -np.inf, np.nan, 0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308):
        assert (np.isnan(rows).any() if v != v else ((rows == v) & (np.signbit(rows) == np.signbit(v))).any()), v
    return rows


COLUMNS = ["p0", "p1", "p2", "p3", "p1 - p0", "p3 / p1", "sqrt(abs(p0 * p3))", "min(p0, p1)"]
EXTRA_BOXES = {"A": [(-40.0, 12.0), (-0.75, 0.0), (0.0, 20.0), (0.1, 12.0)],
               "B": [(0.0, 0.3), (0.0, 1000.0), (0.0, 1e-149), (-5e-301, 5e-301)]}
PAIRS = [(0, 1), (2, 3), (0, 4), (4, 5), (6, 7), (1, 7)]
CHAINS = [0, 1, 2, 299]


def assert_equals_ref(got, want, finite_chains=(), what=""):
    """a Derived against a RefDerived: counts with ==, sums bit for bit, a NaN by its position"""
    assert_equals(got.joint, want.joint, finite_chains, what)
    assert np.array_equal(got.hist, want.hist), what
    assert np.array_equal(got.nonfinite, want.nonfinite), what
    assert got.vmin.tobytes() == want.vmin.tobytes() and got.vmax.tobytes() == want.vmax.tobytes(), what
    assert got.n_batches == len(want.batch[0, 0][0]), what
    for (k, c), (closed, part) in want.batch.items():
        assert same_floats(got.batch[k, c, :len(closed)], np.array(closed)), (what, k, c)
        assert same_floats(got.batch[k, c, len(closed)], part), (what, k, c)
        assert not got.batch[k, c, len(closed) + 1:].any(), (what, k, c)
