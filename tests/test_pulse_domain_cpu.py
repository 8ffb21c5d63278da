"""tests/pulse_domain.py held against itself and against 200-bit arithmetic, on the CPU: the committed table of the device
logarithm against its generator, the modelled logarithm against mpmath, every restated form of the pulse likelihoods
and the double-precision oracle against the derived budget, and the sweep of units against the conditions the GPU
tests rely on (every class met, few edge points)."""
import importlib.util
import math
import os
from fractions import Fraction

import numpy as np
import pytest

from oracle import oracle as orc
from tests import data_lengths as dl
from tests import pulse_domain as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def generator():
    spec = importlib.util.spec_from_file_location("make_logtab", os.path.join(ROOT, "tools", "make_logtab.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- header against generator ------------------------------------------------------------------------------------------
def test_committed_table_equals_the_generator(generator):
    tab, ln2hi, ln2lo = pd.table()
    gen = np.array(generator.TAB, dtype=np.float64)
    assert tab.shape == gen.shape == (256, 3)
    diff = np.argwhere(_bits(tab) != _bits(gen))
    assert len(diff) == 0, "log_table.h differs from tools/make_logtab.py at (bin, column) %s" % diff[:5].tolist()
    assert (ln2hi.hex(), ln2lo.hex()) == (generator.LN2_HI.hex(), generator.LN2_LO.hex())


def test_table_structure():
    tab, ln2hi, ln2lo = pd.table()
    for i in (159, 160):                                  # the two bins next to 1: r = z - 1
        assert tab[i].tolist() == [1.0, 0.0, 0.0]
    assert np.all(tab[:, 0] > 0)
    # k ln2_hi + logc_hi is exact for |k| <= 1075: the FMA's one rounding changes nothing
    hi = [Fraction(v) for v in tab[:, 1].tolist()]
    l2 = Fraction(ln2hi)
    for k in (-1075, -1074, -1023, -512, -1, 0, 1, 2, 3, 511, 1023, 1024, 1075):
        for h in hi:
            q = k * l2 + h
            assert Fraction(q.numerator / q.denominator) == q, (k, float(h))
    i, k, z = pd.log_index(np.array([0.6875, 1.0, np.nextafter(1.375, 0), 2.0 ** -1022, np.finfo(float).max]))
    assert i.tolist() == [0, 160, 255, 160, 159] and k.tolist() == [0, 0, 0, -1022, 1024]
    assert z.tolist() == [0.6875, 1.0, float(np.nextafter(1.375, 0)), 1.0, float(np.nextafter(1.0, 0))]


# ---- the modelled logarithm against mpmath -----------------------------------------------------------------------------
def test_modelled_logarithm_against_mpmath():
    worst, at = 0.0, None
    for cls, (x, e) in pd.log_arguments().items():
        err = pd.log_error_ulp(x, e)
        j = int(np.argmax(err))
        print("%-14s %5d arguments, worst %.4f ulp at x = %r e = %d" % (cls, len(x), err[j], float(x[j]), int(e[j])))
        if cls != "finish_long":                          # tools/make_logtab.py's domain: its "<= 0.7 ulp" holds
            assert err[j] <= pd.LOG_TABLE_DOMAIN_ULP, (cls, float(x[j]), int(e[j]), err[j])
        if err[j] > worst:
            worst, at = float(err[j]), (cls, float(x[j]), int(e[j]))
    print("worst %.4f ulp at %s" % (worst, at))
    assert worst <= pd.LOG_WORST_MEASURED, (worst, at)
    assert worst >= pd.LOG_WORST_MEASURED - 0.01, "LOG_WORST_MEASURED is stale: measured %.4f at %s" % (worst, at)
    assert at[1:] == (pd.LOG_WORST_X, pd.LOG_WORST_E)


def test_modelled_logarithm_exact_at_one_and_monotone_across_bins():
    assert pd.dev_log(np.array([1.0]))[0] == 0.0 and not np.signbit(pd.dev_log(np.array([1.0]))[0])
    off = pd.OFF_HI << 32
    for kexp in (-1000, -1, 0, 1, 1000):
        b = np.array([off + (i << 44) + (kexp << 52) for i in range(257)], dtype=np.uint64)   # 256: the next binade's bin 0
        lo = pd.dev_log((b - np.uint64(1)).view(np.float64))
        at = pd.dev_log(b.view(np.float64))
        up = pd.dev_log((b + np.uint64(1)).view(np.float64))
        assert np.all(lo <= at) and np.all(at <= up), (kexp, np.flatnonzero((lo > at) | (at > up))[:5])
        assert np.all(np.diff(at) > 0)


# ---- the restated forms and the oracle against the budget --------------------------------------------------------------
def _check(name, waves, n, row, beta, a=0, b=0, data=None, want_oracle=False):
    """one evaluation: the restatement (and the oracle) within the budget; returns the class"""
    p0 = pd.base_params(name)[row]
    base = pd.base_data(name, n) if data is None else data
    sc = pd.scaled(name, p0, base, a, b)
    assert sc is not None, (name, a, b)
    p, d = sc
    ex = pd.exact(name, p0, len(base), beta, a, b, data=data)
    kap = pd.kappa(name, p0, base)
    dev = pd.device_eval(name, p, d, beta, waves)
    what = "%s waves=%d n=%d row=%d a=%d b=%d %s %s" % (name, waves, len(base), row, a, b, dev.cls, dev.classes)
    assert math.isfinite(dev.prob), what
    bud = pd.prob_budget(name, ex, kap, waves, dev)
    err = abs(float(pd.MP.mpf(dev.prob) - ex.prob))
    assert err <= bud, "%s: the restated form is %.3g from the exact value, budget %.3g" % (what, err, bud)
    assert bud <= 1e-13 * ex.T * max(beta, 1e-3) + 1e-13 * abs(float(ex.prob)), (what, bud)    # far below the suite's 1e-12
    if want_oracle:
        got = orc.loglike(pd.model_id(name), p, d, beta=beta)[0]
        ob = pd.oracle_budget(name, ex, kap)
        oerr = abs(float(pd.MP.mpf(float(got)) - ex.prob))
        assert oerr <= ob, "%s: the oracle is %.3g from the exact value, budget %.3g" % (what, oerr, ob)
    return dev


@pytest.mark.parametrize("name", pd.NAMES)
def test_every_loop_form_within_budget_at_ordinary_units(name):
    classes = set()
    for waves in dl.WAVES:
        for n in pd.sweep_lengths(waves, name):        # (the row by the length: a length met at several wave counts is one exact value)
            dev = _check(name, waves, n, n % 3, (1.0, 0.37, 0.05)[n % 3], want_oracle=waves == 1)
            classes.add(dev.cls)
    assert classes <= {"quad", "pair"}, classes


@pytest.mark.parametrize("name", pd.NAMES)
def test_sweep_of_units_classes_and_budget(name):
    """every unit of the sweep: the restatement is finite and within the budget of its class (edge: of the larger
    neighbour), the oracle within its own; every class this model can reach is met; at most 5 % are edge points"""
    seen, n_units, n_edge = {}, 0, 0
    for waves in (1, 4):
        n = pd.unit_length(waves)
        for a, b, tag in pd.units(name):
            if pd.scaled(name, pd.base_params(name)[0], pd.base_data(name, n), a, b) is None:
                continue
            dev = _check(name, waves, n, 0, 0.7, a, b, want_oracle=waves == 1 and tag.startswith("coarse"))
            seen.setdefault(dev.cls, []).append((waves, a, b))
            n_units += 1
            n_edge += dev.cls == "edge"
    print(name, {k: len(v) for k, v in seen.items()}, "of", n_units)
    want = {"pair", "ref", "edge"} | ({"quad"} if name == "pulse_vrot" else set())
    assert want <= set(seen), (name, sorted(seen))
    assert n_edge <= 0.05 * n_units, (n_edge, n_units)
    band = [(w, b) for w, a, b in seen.get("pair", []) + seen.get("edge", []) if a == 0 and 500 <= b < 532]
    assert band, "the top band holds no evaluation the fast forms keep"


@pytest.mark.parametrize("name", [n for n in pd.NAMES if n != "pulse1"])
@pytest.mark.parametrize("waves", [2, 4, 8])
def test_far_point_sends_one_wave_back(name, waves):
    for last in (False, True):
        data, idx = pd.far_point(name, waves, last)
        dev = _check(name, waves, len(data), 1, 0.7, data=data)
        w = (idx % (64 * waves)) // 64
        assert dev.classes[w] == "ref" and all(c == "pair" for i, c in enumerate(dev.classes) if i != w), dev.classes
        assert dev.cls == "mixed"
