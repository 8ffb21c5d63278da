"""The pulse and pulse_vrot likelihoods (apemost_amd/csrc/pt_device.h) over their whole range: the table logarithm as
it ships, the exact value of the reference's expression, a restatement of every fast form with its range guards, the
error budget each form is held to, and the inputs that walk the guards' edges.  CPU only; shared by
tests/test_pulse_domain_cpu.py and tests/test_gpu_pulse_domain.py.  The analogue of tests/sine_domain.py.

THE TABLE LOGARITHM.  table() parses apemost_amd/csrc/log_table.h (hex floats) -- not the generator's table: the model
is of what ships.  dev_log(x, e) restates log_begin / log_end with single-rounded FMAs; `e` is what LogProdT::finish adds
to the exponent (ln(x 2^e)).  Domain: NORMAL positive doubles.  The bit trick takes the exponent from the bit pattern,
so a subnormal (exponent field 0) would be read as 2^-1023 times a mantissa that lacks its leading one; no caller
reaches one: the prior takes ln(h + hmin) with hmin > 0 normal (or h itself normal), the serial term's y and finish()'s
v = m / md with m, md in [1/2, 1) lie in (1/2, 2), and a lane whose products came near the subnormals is taken again in
the reference's order with ocml's log (LogProdT::bad).  log_arguments() is the fixed list, in named classes.

THE ONE MEASURED NUMBER.  LOG_WORST_ULP: the model's worst error over log_arguments() against 200-bit mpmath, in ulp of
the result, plus one final rounding (0.5 ulp) -- measured by tests/test_pulse_domain_cpu.py, written down here with
its argument, as sine_domain.WORST_ERR was.  tools/make_logtab.py's "<= 0.7 ulp" holds on that tool's domain, |k| <= 1075
(measured: 0.51); finish() raises k beyond it, where the head of the sum is no longer exact and the worst grows to 1.0.

THE EXACT VALUE.  exact() evaluates the reference's expression in mpmath (a context of its own, 240 bits) from the
double inputs: y_i = sum_j h_j / (1 + (2 pi (f_j - nu_i) tau)^2) (apps/pulse.c; pulse_vrot: four Lorentzians, at fa and
at fb - vrot, fb, fb + vrot with the height hb), 2 pi the reference's double 2 * M_PI;
S = sum_i (ln y_i + d_i / y_i), prior = -sum_j ln(h_j + hmin) / n_modes, prob = prior - beta (p1 + S), and
T = sum_i (|ln y_i| + |d_i / y_i|), the scale rounding is relative to (the logarithms change sign: |S| is not it).
A change of units by powers of two -- frequencies x 2^a, lifetime / 2^a, heights and data x 2^b -- is exact on the
inputs, leaves (f - nu) tau and d / y what they were and multiplies y by 2^b: the per-point values are computed once
in the base units and ln y_i(b) = ln y_i(0) + b ln 2 (scaled() asserts that the scaling of the inputs is exact).

THE FAST FORMS.  device_eval() restates Engine::lane_sum lane by lane: rows in registers, the pipelined four-wide loop
(pulse_vrot, one and two waves; with one wave its FAST form, one reciprocal for four points), the plain four-wide loop,
the two-wide loop, the one-wide tail, renorm() where the loops place it, finish() by table or by libm's log (the LEAN
one-wave pulse kernel), the wave sums, the tree and Model::finish.  Every operation is rounded once (FMAs through
libm's fma); the reciprocal is the correctly rounded 1 / b (the hardware's seed cannot be modelled bit for bit; rcp_nr
is within 1 ulp for any seed good to 2^-24, tests/test_device_math_models.py).  The predicates suspect() and bad() are
restated on the restated exponents and an evaluation is classified per wave:
  quad   the four-point form stood (pulse_vrot, one wave, at least one pipelined pass)
  pair   the two-point form stood
  ref    the wave took its share again in the reference's order (Model::term_ref)
  edge   the deciding exponent is within 1 of its threshold (kQuadExponent, kPairExponent, or a finite product with
         exponent 1023 / 1024 next to overflow): c_tau's last bit is not modelled, so either neighbour may run
An evaluation is `edge` if any of its waves is, `mixed` if its waves differ (far_point), else its waves' class.

THE ERROR BUDGET, derived by counting roundings in pt_device.h; u = 2^-53, every product, sum or FMA is one rounding
(relative u), rcp_nr is 1 ulp (2 u), first order throughout (prob_budget() multiplies by 1 + 2^-20 for the second order).
Per point, t_i = |d_i / y_i| and l_i = |ln y_i| exact; per lane, A_l = sum t_i, L_l = |ln prod y_i|, G_l = the number of
groups the lane adds (one FMA into acc each).

  y_i (relative).  c_tau = rcp_nr(t t), t = fl(2 pi tau): 1 + 2 + 2 = 5 u, common to all points, sensitivity
  d ln y / d ln c in [0, 1): 5.  q_j = fma(dist, dist, c): dist carries E_j u absolute (E_j = |dist| for one
  subtraction; pulse_vrot's fb - nu -+ vrot rounds twice, E_j = |fb - nu| + |dist|, which cancellation can make large
  against |dist|), so q_j carries kappa_j = 1 + 2 |dist| E_j / q_j; the q_j enter N and D as the same values and
  sum_j |d ln y / d ln q_j| = 1: kappa_i = max_j kappa_j (pulse: <= 3; pulse_vrot: computed from the inputs, never from
  a device's output).  The form's own products, F = roundings in N plus roundings in D:
    pulse 1 mode   N = h c (1), D = q (0)                                                       F = 1
    pulse 2 modes  D = q0 q1 (1); N = fma(hc0, q1, hc1 q0): hc (1), product (1), fma (1)        F = 4
    pulse 3 modes  q12 (1), D (1); N: hc (1), hc2 q1 (1), fma (1), q0 (..) (1), q12 (1), fma (1)  F = 8
    pulse > 3      y = sum_j (h_j c) rcp(q_j): 1 + 2 + 1 per term, M - 1 additions; D = 1       F = M + 3
    pulse_vrot     D = A (B1 (B2 B3)) (3); S = fma(B1, B2 + B3, P) (3); N = fma(ha_c, B1P, hb_c (A S)):
                   max(1 + 2, 1 + 1 + 3 + 1) + 1 = 7                                             F = 10
  eps_i = 5 + kappa_i + F.
  The quotient t_i (relative), on top of eps_i:  one point  rcp (2) + d D (1) = 3;  a pair  pN (1) + rcp (2) +
  num = fma(d0 D0, N1, (d1 D1) N0) (2 + 1) = 6;  four points  P = pN01 pN23 (3) + rcp (2) + num (3 + 1 + 1 + 1) = 11.
  ln of the lane's product (absolute):  per point eps_i, and per point 2 for the group's products and the two
  mantissa products (pair: pN, pD, m, md = 4 for two points; four points: 3 + 3 + 1 + 1 = 8 for four; one point: 2);
  renorm() is exact;  finish: div_fast(m, md) 1.5 ulp = 3, and the logarithm:  table  2 LOG_WORST_ULP L_l;
  LEAN  libm's / ocml's log to 3 ulp (the OpenCL bound) of |ln v| <= 0.7: 5, then fma(e, ln2_hi, .) + e ln2_lo: 3 L_l.
  The sums: acc = fma(num, r, acc) G_l times, each relative to at most A_l; acc += ln prod: 1; the wave butterfly: 6
  levels; the tree over W waves: ceil(log2 W) levels -- each relative to at most sum_l (A_l + L_l).
  So  |S_dev - S| <= u ( sum_i (eps_i + Q) t_i + sum_i (eps_i + 2) + sum_l (G_l A_l + 3 + c_log(L_l))
                         + (7 + ceil(log2 W)) sum_l (A_l + L_l) ),   Q = 6 (pair) or 11 (quad):
  the shape u (a sum |d_i / y_i| + b n + c |ln of the lane products|) with a = eps + Q + G + 7 + log2 W, b = eps + 2 and
  c = 2 LOG_WORST_ULP + 7 + log2 W.
  ref (Model::term_ref and the oracle).  a = 2 pi dist tau: 2 roundings, squared: 4 + 1, 1 + a a (1), h / . (1), M - 1
  additions, no c_tau: eps_ref_i = (kappa_i - 1) + M + 6.  log(y) to 3 ulp: 6 l_i; d / y: 1; their sum: 1, relative to
  l_i + t_i; acc += term R_l times (the lane's rows), each relative to at most sum over the lane of l_i + t_i -- the scale
  is T, not the lane products:
      |S_dev - S| <= u ( sum_i (eps_ref_i (1 + t_i) + 7 l_i + 2 t_i) + (R + 7 + ceil(log2 W)) sum_i (l_i + t_i) ).
  The oracle adds its n terms serially: its budget is this one with R = n and W = 1.
  prob = prior - beta (p1 + S):  beta times the above, plus u (2 beta (|p1| + |S|) + |prob|) for the three roundings
  of Model::finish, plus the prior's: u ((2 P_log sum_j |ln(h_j + hmin)| + M) / M + (M + 1) |prior|) with
  P_log = LOG_WORST_ULP (table) or 3 (ocml): the logarithms, the additions h + hmin, the sum and the division."""
import ctypes
import ctypes.util
import functools
import math
import os
import re
import types

import mpmath
import numpy as np

from apemost_amd import workloads as wl
from tests import data_lengths as dl

MP = mpmath.mp.clone()      # a context of its own: the precision of other tests' mpmath stays what it was
MP.prec = 240
U = 2.0 ** -53
TWO_PI = 2.0 * 3.14159265358979323846264338328
K_QUAD, K_PAIR = 900, 1000                         # kQuadExponent, kPairExponent (pt_device.h)
HMIN = 1e-6
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "apemost_amd", "csrc", "log_table.h")
OFF_HI = 0x3FE60000                                # the high word of 0.6875

# measured by tests/test_pulse_domain_cpu.py::test_modelled_logarithm_against_mpmath over log_arguments(): the worst
# error in ulp of the result, at (LOG_WORST_X, LOG_WORST_E) of the class finish_long -- beyond |k| = 1075 the head
# k ln2_hi + logc_hi rounds, which costs up to half an ulp more; plus one final rounding.  Every class with |k| <= 1075
# (tools/make_logtab.py's domain) stays at LOG_TABLE_DOMAIN_ULP, worst 0.5101 at x = 1.05078125, the first double of
# its bin: the generator's "<= 0.7 ulp" holds there.
LOG_WORST_X, LOG_WORST_E = 0.6610424313060136, 3013
LOG_WORST_MEASURED = 0.9944                        # measured 0.99429
LOG_WORST_ULP = LOG_WORST_MEASURED + 0.5
LOG_TABLE_DOMAIN_ULP = 0.7

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma_obj = np.frompyfunc(_libm.fma, 3, 1)


_LD = np.longdouble
_LD_OK = np.finfo(_LD).nmant >= 63 and np.finfo(_LD).maxexp > 8000


def fma(a, b, c):
    """fl(a b + c), rounded once, elementwise.  Where the extended type has 64 bits the value is first taken there
    (two roundings of 2^-64, no overflow), and only the elements whose extended value lies too close to a midpoint of
    two doubles for that to decide the rounding -- or which are subnormal, or not finite -- go through libm's fma."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64),
                                  np.asarray(c, dtype=np.float64))
    if not _LD_OK or a.size < 8:
        return np.asarray(_fma_obj(a, b, c), dtype=np.float64)
    with np.errstate(all="ignore"):
        out = a * b + c                                   # (an operand that is not finite: IEEE's rules, as they are)
        fin = np.flatnonzero((np.isfinite(a) & np.isfinite(b) & np.isfinite(c)).ravel())
        if len(fin) == 0:
            return out
        a, b, c = a.ravel()[fin], b.ravel()[fin], c.ravel()[fin]
        p = a.astype(_LD) * b.astype(_LD)
        r = p + c.astype(_LD)
        d = r.astype(np.float64)
        ad, ar = np.abs(d), np.abs(r)
        gap = np.where(ar < ad, np.spacing(np.nextafter(ad, 0.0)), np.spacing(ad)) / 2      # to the midpoint on r's side
        slack = gap.astype(_LD) - np.abs(ar - ad.astype(_LD))
        unsure = ~(slack > (np.abs(p) + ar) * _LD(2.0 ** -61)) | ~(ad >= 2.0 ** -1000) | ~np.isfinite(d)
    if unsure.any():
        d[unsure] = np.asarray(_fma_obj(a[unsure], b[unsure], c[unsure]), dtype=np.float64)
    out = out.copy()
    out.ravel()[fin] = d
    return out


# ---- the table logarithm as shipped ------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(path=HEADER):
    """(tab [256][3] = invc, logc_hi, logc_lo; kLn2Hi; kLn2Lo) parsed from the committed header"""
    text = open(path).read()
    hx = r"(-?0x[0-9a-fA-F.]+p[-+]?\d+)"
    ln2hi = float.fromhex(re.search(r"kLn2Hi\s*=\s*" + hx, text).group(1))
    ln2lo = float.fromhex(re.search(r"kLn2Lo\s*=\s*" + hx, text).group(1))
    body = text[text.index("g_logtab"):]
    body = body[body.index("{") + 1:body.index("}")]
    vals = [float.fromhex(v) for v in re.findall(hx, body)]
    assert len(vals) == 768, len(vals)
    tab = np.array(vals).reshape(256, 3)
    tab.setflags(write=False)
    return tab, ln2hi, ln2lo


def log_index(x):
    """(bin i, exponent k, z) of log_begin's bit trick"""
    bits = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    xhi = (bits >> np.uint64(32)).astype(np.int64)
    thi = (xhi - OFF_HI) & 0xFFFFFFFF
    i = (thi >> 12) & 0xFF
    k = np.where(thi >= 2 ** 31, thi - 2 ** 32, thi) >> 20
    zhi = (xhi - (thi & 0xFFF00000)) & 0xFFFFFFFF
    z = ((zhi.astype(np.uint64) << np.uint64(32)) | (bits & np.uint64(0xFFFFFFFF))).view(np.float64)
    return i, k, z


def dev_log(x, e=0, tab=None):
    """log_begin / log_end of normal positive doubles x (elementwise), the exponent raised by e as finish() does"""
    t, ln2hi, ln2lo = table() if tab is None else tab
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    i, k, z = log_index(x)
    kd = (k + np.asarray(e, dtype=np.int64)).astype(np.float64)
    r = fma(z, t[i, 0], -1.0)
    r2 = r * r
    r4 = r2 * r2
    p01 = fma(1.0 / 3.0, r, -0.5)
    p23 = fma(0.2, r, -0.25)
    p45 = fma(1.0 / 7.0, r, -1.0 / 6.0)
    q0 = fma(p23, r2, p01)
    p = fma(p45, r4, q0)
    t1 = fma(kd, ln2hi, t[i, 1])
    lo = fma(kd, ln2lo, t[i, 2])
    return t1 + (r + fma(r2, p, lo))


def _from_bits(b):
    return np.array(b, dtype=np.uint64).view(np.float64)


@functools.lru_cache(maxsize=None)
def log_arguments():
    """{class: (x [n], e [n])}: the logarithm's arguments, deterministic; e = 0 but in the class `finish`"""
    rs = np.random.RandomState(20241021)
    off = OFF_HI << 32
    out = {}
    edges = []
    for kexp in (-1021, -511, -1, 0, 1, 512, 1023):     # z in [0.6875, 1) has the exponent field of 2^(k - 1)
        for i in range(256):
            lo, hi = off + (i << 44), off + ((i + 1) << 44) - 1
            for b in (lo, lo + 1, (lo + hi) // 2, hi):
                edges.append(b + (kexp << 52))
    x = _from_bits([b for b in edges if 0 < (b >> 52) < 2047])
    out["bin_edges"] = x
    one = np.array([1.0])
    out["near_one"] = np.array([np.nextafter(1.0, 0), np.nextafter(np.nextafter(1.0, 0), 0), 1.0, np.nextafter(1.0, 2),
                                np.nextafter(np.nextafter(1.0, 2), 2)])
    lo159, lo161 = off + (159 << 44), off + (161 << 44)
    out["bins_159_160"] = _from_bits(rs.randint(lo159, lo161, 400, dtype=np.int64).astype(np.uint64))
    out["extremes"] = np.array([2.0 ** -1022, np.nextafter(2.0 ** -1022, 1), np.finfo(np.float64).max,
                                np.nextafter(np.finfo(np.float64).max, 0)])
    out["powers_of_two"] = np.ldexp(one, np.arange(-1022, 1024)).ravel()
    out["random"] = np.ldexp(rs.uniform(0.5, 1.0, 1500), rs.randint(-1021, 1025, 1500))
    res = {k: (v, np.zeros(len(v), dtype=np.int64)) for k, v in out.items()}
    # LogProdT::finish: v = fl(m fl(1 / md)), m and md in [1/2, 1), the exponent e of the lane's product added
    m, md = rs.uniform(0.5, 1.0, 1200), rs.uniform(0.5, 1.0, 1200)
    m[:8], md[:8] = [0.5, 0.5, 1 - 2.0 ** -53, 1 - 2.0 ** -53, 0.75, 0.5, 0.5 + 2.0 ** -53, 0.6],\
                    [0.5, 1 - 2.0 ** -53, 0.5, 1 - 2.0 ** -53, 0.75, 0.75, 0.5, 0.6]
    e = np.concatenate([np.zeros(8, dtype=np.int64), rs.randint(-1070, 1071, 592)])
    res["finish"] = (m[:600] * (1.0 / md[:600]), e)
    # the same beyond |k| = 1075, where k ln2_hi + logc_hi is no longer exact: the product of a long lane in ordinary
    # units (1024 points of config 5 per lane) or of a few points in extreme ones
    res["finish_long"] = (m[600:] * (1.0 / md[600:]), np.concatenate([rs.randint(-4000, 4001, 300), rs.randint(-40000, 40001, 300)]))
    for k, (v, ee) in res.items():
        assert np.all((v >= 2.0 ** -1022) & np.isfinite(v)), k
        v.setflags(write=False)
        ee.setflags(write=False)
    return res


def true_log(x, e=0):
    """ln(x 2^e) as an mpf"""
    return MP.log(MP.mpf(float(x))) + int(e) * MP.log(2)


def ulp_of(v):
    return float(np.spacing(abs(float(v))))


def log_error_ulp(x, e=0, tab=None):
    """|dev_log - ln| in ulp of the (rounded) true value, per argument; 0 where both are 0"""
    got = dev_log(x, e, tab)
    out = np.zeros(len(got))
    for j, (xv, ev, g) in enumerate(zip(np.atleast_1d(x), np.broadcast_to(e, got.shape), got)):
        want = true_log(xv, ev)
        if want == 0:
            out[j] = 0.0 if g == 0 else math.inf
        else:
            out[j] = float(abs(MP.mpf(float(g)) - want) / ulp_of(want))
    return out


# ---- models, inputs ----------------------------------------------------------------------------------------------------
NAMES = ("pulse1", "pulse2", "pulse3", "pulse4", "pulse5", "pulse_vrot")


def modes_of(name):
    return 4 if name == "pulse_vrot" else int(name[5:])


def kernel_name(name):
    """the name tests/data_lengths.py knows the model by"""
    return "pulse_vrot" if name == "pulse_vrot" else "pulse"


def model_id(name):
    return wl.MODEL_PULSE_VROT if name == "pulse_vrot" else wl.MODEL_PULSE


def n_par(name):
    return 7 if name == "pulse_vrot" else 2 + 2 * modes_of(name)


def height_columns(name):
    return [4, 6] if name == "pulse_vrot" else [3 + 2 * j for j in range(modes_of(name))]


def freq_columns(name):
    return [2, 3, 5] if name == "pulse_vrot" else [2 + 2 * j for j in range(modes_of(name))]


@functools.lru_cache(maxsize=None)
def base_data(name, n):
    """the workload's data vector in its own units (nu in [10, 12], d = y Exp(1) > 0), read-only"""
    w = wl.pulse_vrot(n_data=n, n_chain=2) if name == "pulse_vrot" else wl.pulse(n_data=n, n_chain=2)
    w.data.setflags(write=False)
    return w.data


@functools.lru_cache(maxsize=None)
def base_params(name, rows=3):
    """parameter rows in ordinary units: the inner part of the workload's prior box"""
    rs = np.random.RandomState([17, modes_of(name), name == "pulse_vrot"])
    p = np.zeros((rows, n_par(name)))
    p[:, 0] = rs.uniform(2.0, 20.0, rows)
    p[:, 1] = rs.uniform(0.1, 0.9, rows)
    if name == "pulse_vrot":
        p[:, 2] = rs.uniform(0.02, 0.4, rows)
    for c in freq_columns(name)[1 if name == "pulse_vrot" else 0:]:
        p[:, c] = rs.uniform(10.2, 11.8, rows)
    for c in height_columns(name):
        p[:, c] = rs.uniform(0.5, 16.0, rows)
    p.setflags(write=False)
    return p


def scaled(name, params, data, a, b):
    """(params, data) in other units: frequencies x 2^a, lifetime / 2^a, heights and data x 2^b -- exact, or None where
    an input would leave the normal range"""
    p, d = np.array(params, dtype=np.float64), np.array(data, dtype=np.float64)
    p[..., 0] = np.ldexp(p[..., 0], -a)
    p[..., freq_columns(name)] = np.ldexp(p[..., freq_columns(name)], a)
    p[..., height_columns(name)] = np.ldexp(p[..., height_columns(name)], b)
    d[:, 0] = np.ldexp(d[:, 0], a)
    d[:, 1] = np.ldexp(d[:, 1], b)
    moved = np.concatenate([p[..., [0] + freq_columns(name) + height_columns(name)].ravel(), d.ravel()])
    if not np.all(np.isfinite(moved) & (np.abs(moved) >= 2.0 ** -1022)):
        return None
    return p, d


@functools.lru_cache(maxsize=None)
def _kernel_lengths(waves, kern):
    return tuple(n for n in dl.sampling_lengths(waves, kern) if n != 4100)


def sweep_lengths(waves, name):
    """tests/data_lengths.py's sampling lengths without the one that only stages more than 64 KiB: every loop form"""
    return _kernel_lengths(waves, kernel_name(name))


def unit_length(waves):
    """the data length of the sweep of units: one four-wide group (with one wave: one pipelined pass of pulse_vrot,
    the FAST form), or one two-wide group (four waves), and a one-wide tail of three lanes"""
    return {1: 4 * 64 + 3, 2: 4 * 128 + 3, 4: 2 * 256 + 3}[waves]


TOP_BAND = "top_band"


@functools.lru_cache(maxsize=None)
def units(name):
    """the sweep of unit scales: a tuple of (a, b, tag).  Coarse: every 64 binades of a (at b = 0) and of b (at a = 0)
    over the range in which the inputs stay normal, and the corners a, b = +-448.  Fine: every binade from 12 below to
    12 above each threshold as the products of this model reach it.  With M Lorentzian denominators per point
    (pulse_vrot: 4) a point's D grows like 2^(2 M a) and its N like 2^(b + 2 M a); pair products twice and four-point
    products four times as fast (the serial form above three modes: N = y ~ 2^b, D = 1, while q ~ 2^(2 a) inside the
    reciprocal).  Thresholds: +-kQuadExponent, -kPairExponent, the top (2^1000 .. overflow at 2^1024) and the bottom
    (2^-1000 .. underflow at 2^-1074).  tag TOP_BAND: the pair product pN = N0 N1 in about [2^1022, 2^1024) -- finite,
    its reciprocal a subnormal -- the band the pair form's smallest-exponent tracking does not see."""
    m = modes_of(name)
    out = {}

    def put(a, b, tag):
        out.setdefault((a, b), tag)
    for v in range(-960, 961, 64):
        put(v, 0, "coarse_a")
        put(0, v, "coarse_b")
    for a in (-448, 448):
        for b in (-448, 448):
            put(a, b, "corner")
    serial = name != "pulse_vrot" and m > 3
    rates_a = [2] if serial else [2 * m, 4 * m] + ([8 * m] if name == "pulse_vrot" else [])
    rates_b = [1, 2] + ([4] if name == "pulse_vrot" else [])
    thresholds = [K_QUAD, -K_QUAD] if name == "pulse_vrot" else []
    thresholds += [K_PAIR, -K_PAIR, 1024, -1074]
    for th in thresholds:
        for rate in rates_a:
            c = int(round(th / rate))
            for a in range(c - 12, c + 13):
                put(a, 0, "fine_a")
        for rate in rates_b:
            c = int(round(th / rate))
            for b in range(c - 12, c + 13):
                if abs(b) <= 1000:
                    put(0, b, "fine_b")
    # the denominators alone next to the subnormals: at b = 16 the pair product of the numerators is 2^16 .. 2^32 above
    # that of the denominators, so pD = D0 D1 walks through [2^-1074, 2^-1000] while 1 / pN is still finite -- the only
    # place where a product that underflowed into a subnormal is used at all (below 2^-1024 the reciprocal of pN
    # overflows, the sum is NaN and bad() holds whatever kPairExponent is)
    if not serial:
        for th in (-K_PAIR, -1074):
            c = int(round(th / (4 * m)))
            for a in range(c - 12, c + 13):
                put(a, 16, "fine_a_den")
    # the top band: a one-point numerator h c ~ 2^511 (h ~ 1e154), its pair product next to overflow; c_tau ~ 2^-10 and
    # h ~ 2^2: these b cover it for every row of base_params (pulse_vrot's N = hc q^3 reaches it later)
    for b in range(500, 548 if name == "pulse_vrot" else 532):
        out[(0, b)] = TOP_BAND
    return tuple((a, b, t) for (a, b), t in sorted(out.items()))


def far_point(name, waves, last):
    """one data vector in ordinary units, 2 T + 1 points, with a single datum moved far from every mode: nu = 4e151,
    d = 7e-306.  There every q_j = dist^2 ~ 2^1007 while the reference's a a ~ 1e307 is still finite, y ~ 2^-1013 is a
    normal number and d / y ~ 1.  A point's denominator D of two q and more overflows, and the serial form's N = y
    makes a pair product below 2^-1000: bad() holds either way, and only the wave that holds the datum takes its share
    again.  (The one-mode pulse stays in range there, D = q and N = h c: it has no such point.)  last: the datum sits
    in the last wave instead of wave 0.  Returns (data, index)."""
    assert modes_of(name) >= 2
    t = 64 * waves
    d = np.array(base_data(name, 2 * t + 1))
    idx = (t - 64 + 5) if last else 5               # row 0: lane 5 of wave 0, or of the last wave
    d[idx] = (4e151, 7e-306)
    return d, idx


# ---- the exact value ---------------------------------------------------------------------------------------------------
def _lines(name, p):
    """[(f, h, k)] of the Lorentzians of one parameter row; k: the multiple of vrot added to the distance, or None"""
    if name == "pulse_vrot":
        return [(p[3], p[4], None), (p[5], p[6], -1), (p[5], p[6], 0), (p[5], p[6], 1)]
    return [(p[2 + 2 * j], p[3 + 2 * j], None) for j in range(modes_of(name))]


def exact_points(name, p, data):
    """per point (ln y_i, d_i / y_i) as mpf lists, the reference's expression from the double inputs"""
    f = MP.mpf
    scale = f(TWO_PI) * f(float(p[0]))               # 2 pi tau, exact: the product of the three factors has no order
    lines = [(f(float(fj)), f(float(hj)), k) for fj, hj, k in _lines(name, p)]
    vrot = f(float(p[2])) if name == "pulse_vrot" else None
    lny, q = [], []
    for nu, d in data:
        nu = f(float(nu))
        y = f(0)
        for fj, hj, k in lines:
            dist = fj - nu + (k * vrot if k else 0)
            a = scale * dist
            y += hj / (1 + a * a)
        lny.append(MP.log(y))
        q.append(f(float(d)) / y)
    return lny, q


@functools.lru_cache(maxsize=256)
def _exact_base(name, row_key, n, data_key):
    p = np.array(row_key)
    data = base_data(name, n) if data_key is None else np.array(data_key).reshape(-1, 2)
    lny, q = exact_points(name, p, data)
    return MP.fsum(lny) + MP.fsum(q), np.array([float(v) for v in lny]), np.array([float(v) for v in q])


def exact(name, p, n, beta, a=0, b=0, hmin=HMIN, data=None):
    """the exact value of one evaluation: base-unit parameter row p on base_data(name, n) (or `data`, base units), seen
    in the units (a, b).  Returns a namespace: prob, prior, S (mpf), T, lny, t (floats per point, in these units)."""
    key = None if data is None else tuple(np.asarray(data).ravel().tolist())
    s0, lny_f, q_f = _exact_base(name, tuple(float(v) for v in p), n, key)
    s = s0 + n * b * MP.log(2)
    hs = [MP.mpf(float(np.ldexp(p[c], b))) + MP.mpf(hmin) for c in height_columns(name)]
    # (h + hmin is rounded by the kernels and by the reference alike before the logarithm: the exact value takes the
    # exact sum, and the budget counts that rounding)
    logs = [MP.log(h) for h in hs]
    prior = -MP.fsum(logs) / len(hs)
    prob = prior - MP.mpf(float(beta)) * (MP.mpf(float(p[1])) + s)
    lny = lny_f + b * math.log(2.0)
    return types.SimpleNamespace(prob=prob, prior=prior, S=s, T=float(np.abs(lny).sum() + np.abs(q_f).sum()), lny=lny, t=q_f,
                                 sum_abs_log_h=float(sum(abs(v) for v in logs)), p1=float(p[1]), beta=float(beta))


# ---- the restated device forms -----------------------------------------------------------------------------------------
def rcp_nr(b):
    """the correctly rounded 1 / b; NaN where rcp_nr's Newton step gives NaN (b zero or not finite, or 1 / b infinite)"""
    b = np.asarray(b, dtype=np.float64)
    with np.errstate(all="ignore"):
        r = 1.0 / b
    return np.where(np.isfinite(b) & (b != 0) & np.isfinite(r), r, np.nan)


class _Model:
    """the per-step constants of Model::load and the per-point N, D of few_modes_nd / terms_lp"""

    def __init__(self, name, p):
        self.name, self.p, self.m = name, p, modes_of(name)
        with np.errstate(all="ignore"):
            t = TWO_PI * p[0]
            self.c = float(rcp_nr(t * t))
            self.lines = _lines(name, p)
            self.hc = [float(h) * self.c for _, h, _ in self.lines]

    def dist(self, j, x):
        f, _, k = self.lines[j]
        d = f - x
        return d if not k else d + k * self.p[2]

    def nd(self, x):
        dist = [self.dist(j, x) for j in range(self.m)]
        q = [fma(d, d, self.c) for d in dist]
        hc = self.hc
        if self.name == "pulse_vrot":
            a_, b1, b2, b3 = q
            pp = b2 * b3
            b1p = b1 * pp
            s = fma(b1, b2 + b3, pp)
            return fma(hc[0], b1p, hc[1] * (a_ * s)), a_ * b1p
        if self.m == 1:
            return np.full_like(x, hc[0]), q[0]
        if self.m == 2:
            return fma(hc[0], q[1], hc[1] * q[0]), q[0] * q[1]
        if self.m == 3:
            q12 = q[1] * q[2]
            return fma(hc[0], q12, q[0] * fma(hc[1], q[2], hc[2] * q[1])), q[0] * q12
        y = np.zeros_like(x)
        for j in range(self.m):
            y = y + hc[j] * rcp_nr(q[j])
        return y, np.ones_like(x)

    def term_ref(self, x, d):
        y = np.zeros_like(x)
        for j in range(self.m):
            a = TWO_PI * self.dist(j, x) * self.p[0]
            y = y + self.lines[j][1] / (1 + a * a)
        return np.log(y) + d / y


def _exp(v):
    """v_frexp_exp_i32_f64: 0 for zero, inf and NaN"""
    return np.where(np.isfinite(v), np.frexp(v)[1], 0).astype(np.int64)


def _mant(v):
    return np.where(np.isfinite(v), np.frexp(v)[0], v)


class _LogProd:
    def __init__(self, t):
        self.m, self.md = np.ones(t), np.ones(t)
        self.e, self.e_lo, self.e_hi = (np.zeros(t, dtype=np.int64) for _ in range(3))
        self.top = np.zeros(t, dtype=np.int64)      # not the kernel's: the largest exponent a product reached at all

    def mul_ratio(self, n, d, sel, tracked):
        en, ed = _exp(n), _exp(d)
        self.e[sel] += en - ed
        self.e_lo[sel] = np.minimum(self.e_lo[sel], np.minimum(en, ed))
        if tracked:
            self.e_hi[sel] = np.maximum(self.e_hi[sel], np.maximum(en, ed))
        self.top[sel] = np.maximum(self.top[sel], np.maximum(en, ed))
        self.m[sel] *= _mant(n)
        self.md[sel] *= _mant(d)

    def renorm(self, sel):
        m, e = np.frexp(self.m[sel])
        self.m[sel] = np.where(np.isfinite(self.m[sel]), m, self.m[sel])
        self.e[sel] += np.where(np.isfinite(self.m[sel]), e, 0)
        m, e = np.frexp(self.md[sel])
        self.md[sel] = np.where(np.isfinite(self.md[sel]), m, self.md[sel])
        self.e[sel] -= np.where(np.isfinite(self.md[sel]), e, 0)

    def finish(self, lean):
        v = self.m * rcp_nr(self.md)
        ok = (v > 0) & np.isfinite(v)
        vs = np.where(ok, v, 1.0)
        if lean:
            _, ln2hi, ln2lo = table()
            e = self.e.astype(np.float64)
            return fma(e, ln2hi, np.log(np.where(ok, v, np.nan))) + e * ln2lo
        return np.where(ok, dev_log(vs, self.e), np.nan)


def walk(nrows, n_data, waves, name, fast):
    """the groups a lane with `nrows` rows adds, Engine::lane_sum: [(first row, width, FAST, renorm after)]"""
    t, kern = 64 * waves, kernel_name(name)
    kw = dl.k_wide(waves)
    if n_data == kw * t:
        return [(0, kw, False, False)]
    out, r = [], 0
    if dl.pipelined(waves, kern):
        passes = n_data // (4 * t)
        for k in range(passes):
            out.append((4 * k, 4, fast, k % 2 == 1))
        r = 4 * passes
    elif waves < 8:
        while nrows - r >= 4:
            out.append((r, 4, False, True))
            r += 4
    while nrows - r >= 2:
        out.append((r, 2, False, True))
        r += 2
    while nrows - r >= 1:
        out.append((r, 1, False, True))
        r += 1
    return out


def _grid(mod, data, waves):
    """N, D and d of every point, [rows][T] (NaN past the end): they do not depend on how the points are grouped"""
    n, t = len(data), 64 * waves
    rows_max = -(-n // t)
    pad = np.full((rows_max * t, 2), np.nan)
    pad[:n] = data
    with np.errstate(all="ignore"):
        nn, dd = mod.nd(pad[:, 0])
    return nn.reshape(rows_max, t), dd.reshape(rows_max, t), pad[:, 1].reshape(rows_max, t)


def _lane_sum(mod, data, waves, fast, grid):
    """(acc [T], lp) of the fast forms, every lane of the workgroup"""
    name, n, t = mod.name, len(data), 64 * waves
    acc, lp = np.zeros(t), _LogProd(t)
    gn, gd, ys = grid
    lanes = np.arange(t)
    nrows_of = (n - lanes + t - 1) // t
    with np.errstate(all="ignore"):
        for nrows in sorted(set(nrows_of.tolist())):
            sel = np.flatnonzero(nrows_of == nrows)
            if nrows == 0 or len(sel) == 0:
                continue
            for r0, width, is_fast, renorm in walk(nrows, n, waves, name, fast):
                nn = [gn[r0 + j, sel] for j in range(width)]
                dd = [gd[r0 + j, sel] for j in range(width)]
                yy = [ys[r0 + j, sel] for j in range(width)]
                if is_fast and width == 4:
                    pn01, pd01, pn23, pd23 = nn[0] * nn[1], dd[0] * dd[1], nn[2] * nn[3], dd[2] * dd[3]
                    num01 = fma(yy[0] * dd[0], nn[1], (yy[1] * dd[1]) * nn[0])
                    num23 = fma(yy[2] * dd[2], nn[3], (yy[3] * dd[3]) * nn[2])
                    pq, pdq = pn01 * pn23, pd01 * pd23
                    num = fma(num01, pn23, num23 * pn01)
                    acc[sel] = fma(num, rcp_nr(pq), acc[sel])
                    lp.mul_ratio(pq, pdq, sel, True)
                else:
                    for j in range(0, width - 1, 2):
                        pn, pd = nn[j] * nn[j + 1], dd[j] * dd[j + 1]
                        num = fma(yy[j] * dd[j], nn[j + 1], (yy[j + 1] * dd[j + 1]) * nn[j])
                        acc[sel] = fma(num, rcp_nr(pn), acc[sel])
                        lp.mul_ratio(pn, pd, sel, False)
                    if width & 1:
                        acc[sel] = fma(yy[-1] * dd[-1], rcp_nr(nn[-1]), acc[sel])
                        lp.mul_ratio(nn[-1], dd[-1], sel, False)
                if renorm:
                    lp.renorm(sel)
        lean = waves == 1 and name != "pulse_vrot"      # finish<kLean && Model::kLeanLog>
        acc = acc + lp.finish(lean)
    return acc, lp


def _near(v, th):
    return abs(int(v) - th) <= 1


def device_eval(name, p, data, beta, waves, hmin=HMIN):
    """the restated evaluation of one parameter row p (in the units of data): a namespace with prob, prior, S, the
    per-wave classes and the evaluation's class"""
    p = np.asarray(p, dtype=np.float64)
    mod = _Model(name, p)
    n, t = len(data), 64 * waves
    kern = kernel_name(name)
    quads = name == "pulse_vrot" and waves == 1 and dl.pipe_passes(n, waves, kern) > 0
    classes, edge_of = [None] * waves, [() for _ in range(waves)]
    acc = None
    with np.errstate(all="ignore"):
        grid = _grid(mod, data, waves)
        if quads:
            acc, lp = _lane_sum(mod, data, waves, True, grid)
            suspect = (lp.e_lo < -K_QUAD) | (lp.e_hi > K_QUAD) | ~np.isfinite(acc)
            if _near(lp.e_lo.min(), -K_QUAD) or _near(lp.e_hi.max(), K_QUAD):
                edge_of[0] = ("quad", "pair")
            if suspect.any():
                acc = None
            else:
                classes[0] = "quad"
        if acc is None:
            acc, lp = _lane_sum(mod, data, waves, False, grid)
        bad = (lp.e_lo < -K_PAIR) | ~np.isfinite(acc)
        ref_acc = None
        for w in range(waves):
            s = slice(64 * w, 64 * w + 64)
            if classes[w] == "quad":
                continue
            # (a product that did overflow decides by itself: the edge at the top is a finite product next to overflow)
            if _near(lp.e_lo[s].min(), -K_PAIR) or (lp.top[s].max() >= 1023 and np.isfinite(acc[s]).all()):
                edge_of[w] = edge_of[w] + ("pair", "ref")
            if bad[s].any():
                classes[w] = "ref"
                if ref_acc is None:
                    ref_acc = np.zeros(t)
                    for i0 in range(0, n, t):
                        blk = data[i0:i0 + t]
                        ref_acc[:len(blk)] = ref_acc[:len(blk)] + mod.term_ref(blk[:, 0], blk[:, 1])
                acc[s] = ref_acc[s]
            else:
                classes[w] = "pair"
        parts = []
        for w in range(waves):
            v = acc[64 * w:64 * w + 64].copy()
            while len(v) > 1:
                v = v[:len(v) // 2] + v[len(v) // 2:]
            parts.append(v[0])
        span = 1
        while span < waves:
            for w in range(0, waves - span, 2 * span):
                parts[w] = parts[w] + parts[w + span]
            span *= 2
        s_dev = parts[0]
        hs = np.array([p[c] for c in height_columns(name)]) + hmin
        logs = np.log(hs) if waves == 1 else dev_log(hs)
        pr = 0.0
        for v in logs:
            pr = pr + v
        prior = -pr / len(hs)
        prob = prior + -beta * (p[1] + s_dev)
    if any(edge_of):
        cls = "edge"
    elif len(set(classes)) > 1:
        cls = "mixed"
    else:
        cls = classes[0]
    return types.SimpleNamespace(prob=float(prob), prior=float(prior), S=float(s_dev), classes=classes, edge_of=edge_of, cls=cls)


# ---- the budget --------------------------------------------------------------------------------------------------------
F_FORM = {"pulse1": 1, "pulse2": 4, "pulse3": 8, "pulse4": 7, "pulse5": 8, "pulse_vrot": 10}
Q_FORM = {"pair": 6, "quad": 11}


def kappa(name, p, data):
    """kappa_i per point, from the inputs in any units (it has none)"""
    mod = _Model(name, np.asarray(p, dtype=np.float64))
    x = np.asarray(data)[:, 0]
    out = np.ones(len(x))
    with np.errstate(all="ignore"):
        for j, (f, _, k) in enumerate(mod.lines):
            d = np.abs(mod.dist(j, x))
            e = d + (np.abs(f - x) if k else 0.0)
            kj = 1 + 2 * d * e / (mod.c + d * d)
            out = np.maximum(out, np.where(np.isfinite(kj), kj, 3.0 if not k else np.inf))
    return out


def _log_levels(w):
    return int(math.ceil(math.log2(w))) if w > 1 else 0


def sum_budget(name, ex, kap, waves, form, wave=None, oracle=False):
    """the bound on |S_dev - S| / u of the lanes of one wave (wave=None: of all) computed in the form `form`"""
    n = len(ex.t)
    t = 64 * waves
    idx = np.arange(n)
    if wave is not None:
        idx = idx[(idx % t) // 64 == wave]
    if len(idx) == 0:
        return 0.0
    m = modes_of(name)
    ti, li, ki = np.abs(ex.t[idx]), np.abs(ex.lny[idx]), kap[idx]
    lane = idx % t
    levels = 7 + _log_levels(waves)
    if form == "ref":
        eps = (ki - 1) + m + 6
        rows = n if oracle else -(-n // t)
        levels = 0 if oracle else levels
        return float(np.sum(eps * (1 + ti) + 7 * li + 2 * ti) + (rows + levels) * np.sum(li + ti))
    eps = 5 + ki + F_FORM[name]
    a_l = np.bincount(lane, weights=ti, minlength=t)
    l_l = np.abs(np.bincount(lane, weights=ex.lny[idx], minlength=t))
    g_l = np.zeros(t)
    for ln in np.unique(lane):
        g_l[ln] = sum(1 if fst and w == 4 else (w + 1) // 2 for _, w, fst, _ in
                      walk((n - ln + t - 1) // t, n, waves, name, form == "quad"))
    lean = waves == 1 and name != "pulse_vrot"
    used = np.bincount(lane, minlength=t) > 0
    c_log = np.where(used, 3 + (5 + 3 * l_l if lean else 2 * LOG_WORST_ULP * l_l), 0.0)
    return float(np.sum((eps + Q_FORM[form]) * ti) + np.sum(eps + 2) + np.sum(g_l * a_l + c_log) + levels * np.sum(a_l + l_l))


def prob_budget(name, ex, kap, waves, dev):
    """the bound on |prob_dev - prob_exact| for the restated classification dev (device_eval), absolute"""
    total = 0.0
    for w in range(waves):
        forms = dev.edge_of[w] or (dev.classes[w],)
        total += max(sum_budget(name, ex, kap, waves, f, wave=w) for f in forms)
    return _finish_budget(name, ex, total, waves == 1)


def oracle_budget(name, ex, kap):
    return _finish_budget(name, ex, sum_budget(name, ex, kap, 1, "ref", oracle=True), True)


def _finish_budget(name, ex, total, libm_prior):
    m = len(height_columns(name))
    p_log = 3.0 if libm_prior else LOG_WORST_ULP
    prior_err = (2 * p_log * ex.sum_abs_log_h + m) / m + (m + 1) * abs(float(ex.prior))
    fin = 2 * ex.beta * (abs(ex.p1) + abs(float(ex.S))) + abs(float(ex.prob))
    return U * (1 + 2.0 ** -20) * (ex.beta * total + fin + prior_err)
