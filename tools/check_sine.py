#!/usr/bin/env python3
"""Accuracy of the device sine (pt_device.h: sin_cw, two-term Cody-Waite reduction modulo pi + one
odd polynomial on [-pi/2, pi/2]) against 200-bit arithmetic, operation by operation as the kernel
rounds them (every FMA rounds once).  Reports the absolute error (what a likelihood sees: it adds
a sin() to numbers of order one) and the relative error in ulp, for the kernel's two-term
reduction and for a three-term one (which keeps the relative error near the zeros of the sine at
the price of one more FMA per sine); the polynomial by Horner's scheme, as the kernel has it.  Both forms of the
multiple of pi are reported: n = rint(x / pi), and the one that ships, n = rint(2 u) from the phase in turns (fm = fma(u, 2, magic)).

    python tools/check_sine.py [samples]"""
import math
import random
import sys

import mpmath as mp

mp.mp.prec = 200

INV_PI = 3.18309886183790691216e-01
NPI_HI, NPI_MID, NPI_LO = -3.14159265358979311600e+00, -1.22464679914735320717e-16, 2.99476980971833966589e-33
MAGIC = 6755399441055744.0
S = [-1.66666666666666657415e-01, 8.33333333333331587045e-03, -1.98412698412549659988e-04, 2.75573192191608328544e-06,
     -2.50521076166904495328e-08, 1.60589772926427431318e-10, -7.64396966398807388923e-13, 2.73143687693798929796e-15]


def fma(a, b, c):
    return float(mp.mpf(a) * mp.mpf(b) + mp.mpf(c))


def reduce_(x, terms=2, u=None):
    """u: the phase in turns, x = fl(2 pi u): the form that ships (sin_multiple), n = rint(2 u)"""
    fm = fma(x, INV_PI, MAGIC) if u is None else fma(u, 2.0, MAGIC)
    fn = fm - MAGIC
    r = fma(fn, NPI_HI, x)
    r = fma(fn, NPI_MID, r)
    if terms == 3:
        r = fma(fn, NPI_LO, r)
    return r, int(fn) & 1


def horner(x, terms=2, u=None):
    r, odd = reduce_(x, terms, u)
    z = r * r
    q = fma(z, S[7], S[6])
    for k in (5, 4, 3, 2, 1, 0):
        q = fma(z, q, S[k])
    v = fma(r * z, q, r)
    return -v if odd else v


def ulp_err(got, x):
    ref = mp.sin(mp.mpf(x))
    if ref == 0:
        return 0.0
    e = mp.frexp(ref)[1]
    return float(abs(mp.mpf(got) - ref) / mp.ldexp(1, e - 53))


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 20000
    rnd = random.Random(1)
    worst = {"abs2": 0.0, "ulp2": 0.0, "ulp2_away": 0.0, "ulp3": 0.0}
    for i in range(n):
        kind = i % 5
        if kind == 0:
            x = rnd.uniform(-10, 10)
        elif kind == 1:
            x = rnd.uniform(-1e4, 1e4)
        elif kind == 2:
            x = rnd.choice((-1, 1)) * 10 ** rnd.uniform(0, 13.5)
        elif kind == 3:  # neighbourhoods of k pi / 2
            x = float(mp.mpf(rnd.randrange(-100000, 100000)) * mp.pi / 2) + rnd.uniform(-1e-6, 1e-6)
        else:  # the doubles nearest to k pi: the worst cancellation the reduction can meet
            x = float(mp.mpf(rnd.randrange(1, 10 ** rnd.randrange(1, 13))) * mp.pi)
        ref = mp.sin(mp.mpf(x))
        h2, h3 = horner(x, 2), horner(x, 3)
        worst["abs2"] = max(worst["abs2"], float(abs(mp.mpf(h2) - ref)))
        worst["ulp2"] = max(worst["ulp2"], ulp_err(h2, x))
        if abs(ref) > 1e-6:
            worst["ulp2_away"] = max(worst["ulp2_away"], ulp_err(h2, x))
        worst["ulp3"] = max(worst["ulp3"], ulp_err(h3, x))
    # the form that ships: n = rint(2 u) from the phase in turns, x = fl(2 pi u).  The two forms differ where 2 u is
    # within an ulp of a half integer: there r leaves [-pi/2, pi/2] (tests/sine_domain.py holds the list and the bound)
    two_pi = 2.0 * 3.14159265358979323846264338328
    shipped = {"abs": 0.0, "abs_half": 0.0, "r_over": 0.0}
    for i in range(n):
        if i % 2:
            u = rnd.choice((-1, 1)) * 10 ** rnd.uniform(0, 12.7)
            key = "abs"
        else:
            k = rnd.randrange(1, 2 ** rnd.randrange(1, 44))
            u = rnd.choice((-1, 1)) * (k + 0.5) / 2
            for _ in range(rnd.randrange(3)):
                u = math.nextafter(u, rnd.choice((-math.inf, math.inf)))
            key = "abs_half"
        x = float(mp.mpf(two_pi) * mp.mpf(u))
        if abs(x) >= 2.0 ** 45:
            continue
        shipped[key] = max(shipped[key], float(abs(mp.mpf(horner(x, 2, u)) - mp.sin(mp.mpf(x)))))
        shipped["r_over"] = max(shipped["r_over"], abs(reduce_(x, 2, u)[0]) - math.pi / 2)
    print("max error over %d samples, |x| < 3e13" % n)
    print("  as shipped (n = rint(2 u) from the phase, |x| < 2^45): absolute %.3g at random phases, %.3g with 2 u within"
          " two ulps of a half integer (|r| - pi/2 up to %.3g)" % (shipped["abs"], shipped["abs_half"], shipped["r_over"]))
    print("  kernel (two-term reduction, Horner): absolute %.3g; relative %.3g ulp where |sin| > 1e-6, %.3g ulp anywhere"
          % (worst["abs2"], worst["ulp2_away"], worst["ulp2"]))
    print("  three-term reduction, Horner: %.3g ulp anywhere" % worst["ulp3"])


if __name__ == "__main__":
    main()
