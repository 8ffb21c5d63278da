"""The device sine (apemost_amd/csrc/pt_device.h, sin_cw / sin_cw_n) over its whole argument range: the arguments at
which a Cody-Waite reduction and an odd polynomial go wrong, a true sine to hold them against, and a probe that reads
the sine a likelihood kernel computed back out of HipSampler.loglike.  CPU only; shared by
tests/test_sine_domain_cpu.py and tests/test_gpu_sine_domain.py.

The sine's argument is x = fl(kTwoPi * u) of a phase in turns u; the shipped form (sin_multiple) takes the
multiple of pi from the phase, n = rint(2 u), so r = x - n pi leaves [-pi/2, pi/2], the interval the polynomial was
fitted on, wherever 2 u is within an ulp of a half integer.  phases() is the fixed list, in named classes:

  small         |u| < 2
  medium        |u| < 2e3
  log_uniform   |u| log-uniform from 1 to the guard
  half_integer  2 u at 0, +-1, +-2 ulps from k + 1/2, k in every binary decade 2^0 .. 2^44 (the guard, x < 2^45, ends
                them at 2 u < 2^45 / pi = 2^43.35), both signs
  integer       2 u at 0, +-1 ulp from k, the same decades: the sine's zeros, where only the reduction is left
  top_octave    x uniform in [2^44, 2^45)
  guard_edge    the largest u for which the range guard still holds, and its neighbours below
  inexact       u = fl(fl(f x0) + ph) at x0 = 12345.678, f in [0.1, 0.3], ph in [0, 1]: the phase's two roundings,
                which a fused f x0 + ph does not reproduce (phases_inexact() gives the (f, ph, u) triples)

The probe (probe_inputs / probe_sine_error).  Data: n identical points (x0, 0); sigma = 0.5, beta = 1; one parameter
point (a, f, ph, o) = (1, f, ph, o_h) per hard phase with o_h = fl(2^-7 - S_h), S_h the true sine.  The model value is
m = fl(sine + o_h) = d, the residual, and prob = -2 n d^2 up to the roundings of the sum: d = 2^-7 + (sine - S_h) + rho
with rho = o_h - (2^-7 - S_h) known exactly.  d is recovered from prob in mpmath; every rounding of the sum is relative to
d^2 ~ 6e-5, so the sine's error follows to a few 1e-17 (resolution())."""
import functools
import math
from fractions import Fraction

import mpmath
import numpy as np

from tests import predict_ref as ref

MP = mpmath.mp.clone()      # a context of its own: the precision of other tests' mpmath stays what it was
MP.prec = 300

# The one measured number: the largest |sin_cw - sin| that tests/test_sine_domain_cpu.py finds over phases() against
# mpmath, plus 2^-53 (a sample does not find the supremum, and one final rounding of a value below 1 is 2^-53).  The
# list's worst argument is WORST_PHASE, of the class half_integer (2 u = 14648149.499999998, one ulp below a half
# integer: n = 14648149, r = pi/2 + 5.9e-9); random arguments stay below 1.8e-16.  4 ulp of 1 are 4.4e-16.
WORST_PHASE = 7324074.749999999
WORST_ERR = 2.4937e-16                             # measured 2.49363705e-16
SIN_CW_ABS_ERR = WORST_ERR + 2.0 ** -53            # 3.604e-16

X0_INEXACT = 12345.678
U_GUARD_CEIL = ref.RANGE / ref.TWO_PI              # about 5.6e12; the guard's edge is within a few ulps of it
R_EXCESS_BOUND = 2.0 ** -8                         # see reduced()
HALF_PI = math.pi / 2
PROBE_OFFSET = 2.0 ** -7
MAX_PROBE_POINTS = 256


def in_range(u):
    """the range guard of a phase u at x = 1, ph = 0 (Model::load, pt_device.h)"""
    return ref.sine_in_range(u, 0.0, 1.0)


@functools.lru_cache(maxsize=None)
def largest_phase():
    """the largest u for which the guard holds"""
    u = U_GUARD_CEIL
    while in_range(u):
        u = math.nextafter(u, math.inf)
    while not in_range(u):
        u = math.nextafter(u, 0.0)
    return u


def step_ulps(v, k):
    """v moved by k doubles (k < 0: towards -inf)"""
    for _ in range(abs(k)):
        v = math.nextafter(v, math.inf if k > 0 else -math.inf)
    return v


@functools.lru_cache(maxsize=None)
def phases_inexact():
    """(f, ph, u) with u = fl(fl(f X0_INEXACT) + ph), the phase as the kernels round it; only triples whose fused
    phase fma(f, X0_INEXACT, ph) is another double"""
    rs = np.random.RandomState(8128)
    out = []
    for f, ph in zip(rs.uniform(0.1, 0.3, 3000).tolist(), rs.uniform(0, 1, 3000).tolist()):
        u = ref.add(ref.mul(f, X0_INEXACT), ph)
        if u != ref.fma(f, X0_INEXACT, ph):
            out.append((f, ph, u))
    return tuple(out[:1500])


@functools.lru_cache(maxsize=None)
def phases():
    """{class: tuple of phases u}, deterministic; every u passes the guard"""
    rs = np.random.RandomState(20240521)
    top = largest_phase()
    out = {}
    out["small"] = tuple(rs.uniform(-2, 2, 1500).tolist())
    out["medium"] = tuple(rs.uniform(-2e3, 2e3, 1500).tolist())
    out["log_uniform"] = tuple((rs.choice([-1.0, 1.0], 3000) * 10.0 ** rs.uniform(0, math.log10(top), 3000)).tolist())
    half, whole = [WORST_PHASE], []
    k_end = int(2 * top) - 1                       # 2 u < 2^45 / pi = 2^43.35: the guard ends the last decade
    for e in range(45):                            # k in [2^e, 2^(e+1)), e = 0 .. 44
        lo, hi = 2 ** e, min(2 ** (e + 1), k_end)
        if lo >= hi:
            continue
        ks = sorted({lo, hi - 1} | {int(k) for k in rs.randint(lo, hi, 13, dtype=np.int64)})
        for k in ks:
            for sign in (1.0, -1.0):
                for j in (0, 1, -1, 2, -2):
                    half.append(sign * step_ulps(k + 0.5, j) / 2)
                for j in (0, 1, -1):
                    whole.append(sign * step_ulps(float(k), j) / 2)
    out["half_integer"] = tuple(u for u in half if in_range(u))
    out["integer"] = tuple(u for u in whole if in_range(u))
    u_lo = 2.0 ** 44 / ref.TWO_PI
    out["top_octave"] = tuple((rs.choice([-1.0, 1.0], 2000) * rs.uniform(u_lo, top, 2000)).tolist())
    out["guard_edge"] = tuple(s * step_ulps(top, -j) for j in range(5) for s in (1.0, -1.0))
    out["inexact"] = tuple(u for _, _, u in phases_inexact())
    for name, us in out.items():
        assert all(in_range(u) for u in us), name
    return out


def argument(u):
    return ref.mul(ref.TWO_PI, u)


def true_sine(x):
    """sin of the double x, as an mpf at 300 bits"""
    return MP.sin(MP.mpf(x))


def reduced(x, u):
    """r of the shipped reduction: n = rint(2 u), r = fma(n, -pi_mid, fma(n, -pi_hi, x)).

    |r| <= pi/2 + 2^-8 inside the guard:  |2 u - n| <= 1/2 exactly (2 u is exact), and
    x = kTwoPi u + rho with |rho| <= ulp(x) / 2 <= 2^-9 for |x| < 2^45, kTwoPi = 2 pi - 2.45e-16, so
    x - n pi = pi (2 u - n) + rho - 2.45e-16 u, and 2.45e-16 * 5.6e12 = 1.37e-3; the two FMAs of the reduction add
    their roundings, below 1e-15, and pi_hi + pi_mid is pi to 1e-32.  pi/2 + 2^-9 + 1.37e-3 + 1e-15 < pi/2 + 2^-8."""
    fm = ref.fma(u, 2.0, ref.MAGIC)
    fn = ref.sub(fm, ref.MAGIC)
    return ref.fma(fn, ref.NPI_MID, ref.fma(fn, ref.NPI_HI, x))


def sine_error(u, x=None):
    """predict_ref.sin_cw (the shipped form) minus the true sine of the same rounded argument, as a float"""
    x = argument(u) if x is None else x
    return float(MP.mpf(ref.sin_cw(x, u)) - true_sine(x))


def exact_in_range(f, ph, x):
    """the guard's predicate, each of its three operations rounded once from exact rational arithmetic, written out on
    its own (finite arguments)"""
    def rn(q):
        return q.numerator / q.denominator
    s = rn(Fraction(rn(Fraction(abs(f)) * Fraction(abs(x)))) + Fraction(abs(ph)))
    return Fraction(rn(Fraction(ref.TWO_PI) * Fraction(s))) < Fraction(2) ** 45


# ---- the probe through HipSampler.loglike ---------------------------------------------------------------------------
def resolution(n_data, waves):
    """what the probe can resolve of d, absolute.  The data sum adds ceil(n / T) equal squares per lane (one rounding
    each, the square's own included in the first), then 6 levels across the lanes of a wave, up to `waves` partial sums,
    and at most 4 more roundings behind them (beta * sum and the division by -2 sigma^2, both exact here):
    (ceil(n / T) + 6 + waves + 4) 2^-53 relative on d^2, half of that relative on d = 2^-7 (1 + 1e-13); d itself is
    fl(sine + o_h), one rounding of half an ulp of 2^-7 (2^-61) where that addition is not exact."""
    t = 64 * waves
    rel = (-(-n_data // t) + 6 + waves + 4) * 2.0 ** -53
    return PROBE_OFFSET * (1 + 2.0 ** -30) * rel / 2 + 2.0 ** -61


def _offset(s_true):
    """o_h = fl(2^-7 - S_h) and rho = o_h - (2^-7 - S_h)"""
    want = MP.mpf(PROBE_OFFSET) - s_true
    o = float(want)                                 # mpmath rounds to nearest
    return o, MP.mpf(o) - want


@functools.lru_cache(maxsize=None)
def probe_points(group):
    """the hard phases a probe evaluates, at most MAX_PROBE_POINTS of (f, ph, u): x0 = 1, ph = 0, u = f ('exact') or
    x0 = X0_INEXACT ('inexact').  'exact': the list's worst argument, the guard's edge, the first entries of the random
    classes, three half integers of every binary decade and the integers at a stride, through every sign and ulp offset."""
    if group == "inexact":
        return tuple(phases_inexact()[:MAX_PROBE_POINTS])
    p = phases()
    pick = [WORST_PHASE] + list(p["guard_edge"])
    pick += p["small"][:12] + p["medium"][:12] + p["log_uniform"][:20] + p["top_octave"][:20]
    half, whole = p["half_integer"], p["integer"]
    by_decade = {}
    for u in half:
        by_decade.setdefault(int(math.log2(abs(2 * u))), []).append(u)
    for e, us in sorted(by_decade.items()):         # three per binary decade; 7 is prime to the 10 entries (sign, offset)
        pick += [us[(e + 7 * j) % len(us)] for j in range(3)]       # of one k: every sign and offset in turn
    pick += whole[::71][:45]                        # and 71 to the 6 entries per k of the integers
    pick = list(dict.fromkeys(pick))
    assert len(pick) <= MAX_PROBE_POINTS
    return tuple((u, 0.0, u) for u in pick)


@functools.lru_cache(maxsize=None)
def _probe_params(points, x0, model, component):
    n_par = 4 if model == "simplesin" else 10
    base = 0 if model == "simplesin" else 3 * component
    params = np.zeros((len(points), n_par))
    info = []
    for i, (f, ph, u) in enumerate(points):
        assert ref.add(ref.mul(f, x0), ph) == u
        x = argument(u)
        o, rho = _offset(true_sine(x))
        params[i, base:base + 3] = (1.0, f, ph)
        params[i, n_par - 1] = o
        info.append(dict(u=u, x=x, rho=rho, o=o, d_model=ref.add(ref.sin_cw(x, u), o)))
    params.setflags(write=False)
    return params, tuple(info)


def probe_inputs(group, n_data, model="simplesin", component=0, x0=None, points=None):
    """(data [n_data][2], params [n_points][n_par], info) of one probe: n identical points (x0, 0) and one parameter
    point per hard phase (in sine3: in `component`, the other two with a = f = ph = 0); info holds, per point, the
    phase u, the argument x, rho and the modelled residual d_model = fl(sin_cw + o_h).  points: (f, ph, u) triples of
    the caller's instead of probe_points(group), u = fl(fl(f x0) + ph).  params and info are shared and read-only."""
    x0 = (1.0 if group == "exact" else X0_INEXACT) if x0 is None else x0
    pts = probe_points(group) if points is None else tuple(points)
    params, info = _probe_params(pts, x0, model, component)
    return np.tile([x0, 0.0], (n_data, 1)), params, info


def probe_sine_error(prob, info, n_data):
    """from the probs of one probe: (the kernel's sine minus the true sine, the kernel's residual minus the modelled
    one), two float arrays; d = sqrt(prob / (-2 n))"""
    err, off = np.zeros(len(info)), np.zeros(len(info))
    for i, (p, h) in enumerate(zip(prob, info)):
        d = MP.sqrt(MP.mpf(float(p)) / (-2 * n_data))
        err[i] = float(d - PROBE_OFFSET - h["rho"])
        off[i] = float(d - MP.mpf(h["d_model"]))
    return err, off
