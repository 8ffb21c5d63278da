"""The device sine and its range guard on the card, through the existing ABI alone (HipSampler.loglike, predict_curve,
run_sampler, burn_in_only): no probe kernel, no hook.

  * the near-fit probe (tests/sine_domain.py): the sine every loop form of the likelihood kernels computes, read back
    out of prob to a few 1e-17, against a true sine (SIN_CW_ABS_ERR) and against the modelled sine (predict_ref.sin_cw)
    at the hard phases -- next to half integers and integers in every binary decade, the top octave, the guard's edge,
    phases whose two roundings a fused multiply-add would not reproduce -- at every wave count and loop regime;
  * the folds' sine at the same phases, bit for bit;
  * the guard's edge in loglike: NaN exactly where the predicate fails, the sine within its bound where it holds;
  * sampling with the per-step check running (a prior box that is not in range) and across the guard (the box is cut by
    it), on every kernel path, against the oracle with its opt-in guard, and in a ladder batch."""
import math
import types

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler
from apemost_amd.state import ALL_FIELDS, LadderState
from oracle import oracle as orc
from tests import data_lengths as dl
from tests import predict_ref as ref
from tests import sine_domain as sd
from tests.helpers import assert_match, make_pair, to_oracle
from tests.test_gpu_ladder_edges import FIELDS, PATHS, _policy

pytestmark = pytest.mark.gpu

MODELS = {"simplesin": (wl.MODEL_SIMPLESIN, 4, (0,)), "sine3": (wl.MODEL_SINE3, 10, (0, 1, 2))}
F_INDEX = {"simplesin": (1,), "sine3": (1, 4, 7)}
SEED, N_CHAIN, N_SWAP, PIECES = 5, 4, 5, (2, 4)      # 6 rounds of 5 steps in two launches
PIECES_CUT = (4, 8)                                  # across the guard: 12 rounds, for 20 out-of-range proposals and more


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the near-fit probe -----------------------------------------------------------------------------------------------
def _probe(s, group, n, name, waves, x0=None, points=None):
    """one loglike call per component: (worst |error|, worst |offset from the model|) over the finite probs, and the
    probs; asserts both bounds per argument"""
    res = sd.resolution(n, waves)
    assert res < 4e-17, (n, waves, res)
    worst, probs = [0.0, 0.0], []
    for comp in MODELS[name][2]:
        _, params, info = sd.probe_inputs(group, n, name, comp, x0=x0, points=points)
        prob, _ = s.loglike(params, 1.0)
        probs.append(prob)
        ok = np.isfinite(prob)
        if points is None:
            assert ok.all() and (prob < 0).all(), (name, waves, n, group, comp)
        err, off = sd.probe_sine_error(np.where(ok, prob, -1.0), info, n)
        for i in np.flatnonzero(ok):
            what = "%s waves=%d n_data=%d %s component %d u=%r" % (name, waves, n, group, comp, info[i]["u"])
            assert abs(err[i]) <= sd.SIN_CW_ABS_ERR + res, "%s: the sine is %.3g from the true sine" % (what, err[i])
            assert abs(off[i]) <= res, "%s: the sine is %.3g from the modelled sine (resolution %.3g)" % (what, off[i], res)
        if ok.any():
            worst = [max(worst[0], float(np.abs(err[ok]).max())), max(worst[1], float(np.abs(off[ok]).max()))]
    return worst, probs


@pytest.mark.parametrize("name,waves", [(m, w) for m in MODELS for w in dl.WAVES])
def test_sine_of_every_loop_form_at_the_hard_phases(name, waves):
    """per argument, length and wave count: (i) |inferred error| <= SIN_CW_ABS_ERR + resolution, (ii) the inferred sine
    is the modelled one within the resolution -- so the 1-wide tail, the 2-wide and 4-wide loops, the rows in registers
    and every pass parity of the pipelined loop compute one sine"""
    model, n_par, _ = MODELS[name]
    worst = [0.0, 0.0]
    for group in ("exact", "inexact"):
        for n in dl.sampling_lengths(waves, name):
            data, _, _ = sd.probe_inputs(group, n, name)
            s = HipSampler(model, n_par, 2, data, waves_per_chain=waves, sigma=0.5)
            assert s.geometry[0] == waves
            w, _ = _probe(s, group, n, name, waves)
            s.close()
            worst = [max(a, b) for a, b in zip(worst, w)]
    print("%s waves=%d: worst inferred error of the sine %.4g (bound %.4g), worst distance from the modelled sine %.3g"
          % (name, waves, worst[0], sd.SIN_CW_ABS_ERR, worst[1]))


@pytest.mark.parametrize("name", list(MODELS))
def test_the_folds_sine_at_the_hard_phases_bit_for_bit(name):
    """predict_curve (the curve function of the predictive and pointwise folds) against predict_ref.curve"""
    model, n_par, comps = MODELS[name]
    for group in ("exact", "inexact"):
        data, _, _ = sd.probe_inputs(group, 3, name)
        s = HipSampler(model, n_par, 2, data)
        for comp in comps:
            _, params, info = sd.probe_inputs(group, 3, name, comp)
            got = s.predict_curve(params, x=[data[0, 0]])
            want = np.array([[ref.curve(model, p, data[0, 0])] for p in params])
            assert np.array_equal(want[:, 0], [h["d_model"] for h in info])
            assert ref.same_floats(got, want), (name, group, comp, np.flatnonzero(_bits(got) != _bits(want))[:5])
        s.close()


# ---- the guard's edge in loglike ----------------------------------------------------------------------------------------
def _edge(pred, start):
    """the largest double v >= 0 with pred(v), found from a start within a few thousand doubles of it"""
    v = start
    for _ in range(10000):
        if not pred(v):
            break
        v = math.nextafter(v, math.inf)
    for _ in range(10000):
        if pred(v):
            return v
        v = math.nextafter(v, 0.0)
    raise AssertionError("no edge near %r" % start)


def _edge_points(x0):
    """(f, ph, u) at the three doubles either side of the predicate's edge in f (at ph = 0.25 and 0) and in ph (at
    f = 0.2 / |x0|), with both signs of f and ph"""
    top, ax = sd.largest_phase(), abs(x0)
    pts = []
    for ph in (0.25, 0.0):
        f_edge = _edge(lambda f: ref.sine_in_range(f, ph, x0), (top - ph) / ax * (1 - 2.0 ** -50))
        pts += [(sd.step_ulps(f_edge, k), ph) for k in (-2, -1, 0, 1, 2, 3)]
    f = 0.2 / ax
    ph_edge = _edge(lambda ph: ref.sine_in_range(f, ph, x0), (top - 0.2) * (1 - 2.0 ** -50))
    pts += [(f, sd.step_ulps(ph_edge, k)) for k in (-2, -1, 0, 1, 2, 3)]
    out = []
    for f, ph in pts:
        for sf in (1.0, -1.0):
            for sp in (1.0, -1.0):
                out.append((sf * f, sp * ph, ref.add(ref.mul(sf * f, x0), sp * ph)))
    return tuple(dict.fromkeys(out))


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("x0", [1.0, -2.45e6, 1e13])
def test_loglike_at_the_guards_edge(name, x0):
    """data with max |x| = |x0|: prob is NaN exactly where the predicate 2 pi (|f| max|x| + |ph|) < 2^45 fails, for the
    sine in any component, and where it holds the sine is within its bound (the probe at these arguments)"""
    model, n_par, comps = MODELS[name]
    n, waves = 65, 1
    pts = _edge_points(x0)
    expect = np.array([ref.sine_in_range(f, ph, x0) for f, ph, _ in pts])
    assert 0.3 * len(pts) < expect.sum() < 0.7 * len(pts)
    assert all(sd.exact_in_range(f, ph, x0) == e for (f, ph, _), e in zip(pts, expect))
    data, _, _ = sd.probe_inputs("exact", n, name, x0=x0, points=pts)
    s = HipSampler(model, n_par, 2, data, waves_per_chain=waves)
    _, probs = _probe(s, "exact", n, name, waves, x0=x0, points=pts)        # asserts the bounds where prob is finite
    for comp, prob in zip(comps, probs):
        assert np.array_equal(np.isnan(prob), ~expect) and np.isfinite(prob[expect]).all(), (
            name, x0, comp, [pts[i] for i in np.flatnonzero(np.isnan(prob) != ~expect)][:4])
    # a parameter that is not a number
    for comp in comps:
        base = 3 * comp if name == "sine3" else 0
        rows = []
        for bad in (math.nan, math.inf, -math.inf):
            for j in (1, 2):
                p = np.zeros(n_par)
                p[base:base + 3] = (1.0, 0.2 / abs(x0), 0.25)
                p[base + j] = bad
                rows.append(p)
        prob, _ = s.loglike(rows, 1.0)
        assert np.isnan(prob).all(), (name, x0, comp, prob)
    s.close()


@pytest.mark.parametrize("name", list(MODELS))
def test_loglike_is_nan_for_any_frequency_once_an_abscissa_is_not_finite(name):
    model, n_par, comps = MODELS[name]
    w = wl.by_name(name, n_data=65, n_chain=2)
    good = HipSampler(model, n_par, 2, w.data, waves_per_chain=1)
    rows = []
    for f in (0.0, 0.2, -0.1, 1e-300):
        p = w.start.copy()
        p[list(F_INDEX[name])] = f
        rows.append(p)
    prob, _ = good.loglike(rows, 1.0)
    good.close()
    assert np.isfinite(prob).all()
    for bad in (math.nan, math.inf, -math.inf):
        data = w.data.copy()
        data[7, 0] = bad
        s = HipSampler(model, n_par, 2, data, waves_per_chain=1)
        prob, _ = s.loglike(rows, 1.0)
        s.close()
        assert np.isnan(prob).all(), (name, bad, prob)


# ---- sampling: the per-step check, and across the guard ------------------------------------------------------------------
X_FAR_INSIDE, X_FAR_CUT = 1e12, 2e13
SAMPLING_PATHS = ("two_phase_w1", "two_phase_w4", "two_phase_w8", "one_barrier_w4", "one_barrier_w8")
BURN_PATHS = ("two_phase_w1", "one_barrier_w4")      # pt_calibrate_kernel and pt_calibrate_ob_kernel
BURN = 201                                           # both halves of burn_in(), one block of 200 steps each


def _problem(name, waves, x_far, cut, n_chain=N_CHAIN, seed=SEED, data_seed=None, init_prob=False):
    """T + 1 points of the workload with one datum moved to x_far; every step width set here, the same for every chain.
    cut: the chains start at f = 0.27 (simplesin; component 2 of sine3) with step 0.02, next to the guard's cut at
    f = 0.28 inside the box.  (workload, device state, oracle ladder, oracle rng)"""
    n = 64 * waves + 1
    src = wl.by_name(name, n_data=n, n_chain=n_chain, **({"seed": data_seed} if data_seed else {}))
    data = src.data.copy()
    if cut and name == "simplesin":     # the workload's signal at the frequency next to the cut: the chains stay there
        rs = np.random.RandomState(data_seed or 1)
        data[:, 1] = np.sin(2 * np.pi * (0.27 * data[:, 0] + 0.4)) + 0.5 + rs.normal(0, 0.5, n)
    if x_far is not None:
        data[n // 3, 0] = x_far
    start, step = src.start.copy(), src.step * 0.3
    step[list(F_INDEX[name])] = 0.002
    if cut:
        start[F_INDEX[name][-1]], step[F_INDEX[name][-1]] = 0.27, 0.02
    w = types.SimpleNamespace(model=src.model, n_par=src.n_par, data=data, start=start, pmin=src.pmin, pmax=src.pmax,
                              step=step, n_data=n)
    st, lad, rng = make_pair(w, n_chain, seed=seed)
    st.step[:] = step
    to_oracle(st, lad)
    if init_prob:
        for c in range(n_chain):
            orc.calc_model(lad, c)
        st.prob[:], st.prior[:] = lad.prob, lad.prior
    return w, st, lad, rng


def _sampler(w, n_chain, path, monkeypatch, seed=SEED):
    waves, flags, helper = PATHS[path]
    assert helper is None
    monkeypatch.delenv("APEMOST_OB_HELPER", raising=False)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=seed, waves_per_chain=waves, flags=flags)
    assert s.geometry[0] == waves
    return s


def _run(w, st, path, monkeypatch, n_chain=N_CHAIN, seed=SEED, pieces=PIECES):
    import torch
    s = _sampler(w, n_chain, path, monkeypatch, seed)
    s.set_state(st)
    launch = _policy(s)
    assert launch == (1 if path.startswith("one_barrier") else 0), (path, launch)
    d = torch.zeros((sum(pieces) * N_SWAP, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
    done = 0
    for k in pieces:
        s.run_sampler(k, N_SWAP, d[done * N_SWAP:].data_ptr())
        done += k
    s.synchronize()
    out = s.get_state(), d.cpu().numpy()
    s.close()
    return out


def _same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a[0], f), getattr(b[0], f)), "%s: %s differs" % (what, f)
    assert np.array_equal(_bits(a[1]), _bits(b[1])), what + ": rows differ"


def _in_range_everywhere(name, w, x_far, rows, dev, what):
    for params in list(rows[:, :, :w.n_par].reshape(-1, w.n_par)) + list(dev.params):
        assert all(ref.sine_in_range(params[j], params[j + 1], x_far) for j in F_INDEX[name]), (what, params)
    assert np.isfinite(rows[:, :, w.n_par:]).all() and np.isfinite(dev.prob).all(), what
    assert np.array_equal(dev.accept + dev.reject, np.full(len(dev.accept), len(rows), dtype=np.uint64)), what


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("waves", [1, 4, 8])
def test_sampling_with_the_check_running_every_step(name, waves, monkeypatch):
    """one datum at x = 1e12.  Run B: the ordinary prior box, in range as a whole (Model::set_box: no check per step).
    Run A: pmax of every frequency at 100, so that the box is not in range and Model::load checks every proposal.  No
    visited frequency comes within 10 step widths of B's box -- the polar method with 32-bit uniforms cannot jump that
    far -- so no proposal is redrawn in either run and the two are one chain, bit for bit, on every kernel of this wave
    count; and that chain is the oracle's."""
    w, st_b, lad, rng = _problem(name, waves, X_FAR_INSIDE, cut=False)
    st_a = st_b.copy()
    st_a.pmax[:, list(F_INDEX[name])] = 100.0
    for j in F_INDEX[name]:
        assert ref.sine_in_range(w.pmax[j], w.pmax[j + 1], X_FAR_INSIDE) and not ref.sine_in_range(100.0, 0.0, X_FAR_INSIDE)
    with orc.sine_guard() as g:
        ref_rows = orc.run_sampler(lad, rng, sum(PIECES), N_SWAP, record=True)
    assert g.final == 0
    runs = {}
    for path in [p for p in SAMPLING_PATHS if PATHS[p][0] == waves]:
        for box, st in (("A", st_a), ("B", st_b)):
            what = "%s %s box %s" % (name, path, box)
            dev, rows = runs[path, box] = _run(w, st, path, monkeypatch)
            assert_match(dev, lad, rng, what=what)
            np.testing.assert_allclose(rows, ref_rows, rtol=1e-9, atol=1e-300, err_msg=what + " rows")
            _in_range_everywhere(name, w, X_FAR_INSIDE, rows, dev, what)
            for j in F_INDEX[name]:
                visited = np.concatenate([st.params[None, :, j], rows[:, :, j], dev.params[None, :, j]])
                assert (visited - 10 * st.step[:, j] > w.pmin[j]).all() and (visited + 10 * st.step[:, j] < w.pmax[j]).all(), what
    first = runs["two_phase_w%d" % waves, "B"]
    for key, run in runs.items():
        _same(run, first, "%s %s against the two-phase kernel with the box in range" % ((name,) + key[:1]))
    assert len({rows[:, :, F_INDEX[name][0]].tobytes() for _, rows in runs.values()}) == 1


@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("waves", [1, 4, 8])
def test_sampling_across_the_guard(name, waves, monkeypatch):
    """one datum at x = 2e13: the guard cuts the frequency at 0.28 inside its prior box, the chains start at 0.27 with
    step 0.02.  An out-of-range proposal has prob = NaN and is rejected -- by the two-phase accept test and by the
    one-barrier owner's threshold of -inf -- so the chain is the guarded oracle's, stays in range, and keeps moving."""
    w, st, lad, rng = _problem(name, waves, X_FAR_CUT, cut=True)
    j = F_INDEX[name][-1]
    assert ref.sine_in_range(0.2799, 1.0, X_FAR_CUT) and not ref.sine_in_range(0.2801, 0.0, X_FAR_CUT) and w.pmax[j] >= 0.3
    with orc.sine_guard() as g:
        ref_rows = orc.run_sampler(lad, rng, sum(PIECES_CUT), N_SWAP, record=True)
    assert g.final >= 20, g.final
    assert lad.accept.min() > 0
    runs = {}
    for path in [p for p in SAMPLING_PATHS if PATHS[p][0] == waves]:
        what = "%s %s" % (name, path)
        dev, rows = runs[path] = _run(w, st, path, monkeypatch, pieces=PIECES_CUT)
        assert_match(dev, lad, rng, what=what)
        np.testing.assert_allclose(rows, ref_rows, rtol=1e-9, atol=1e-300, err_msg=what + " rows")
        _in_range_everywhere(name, w, X_FAR_CUT, rows, dev, what)
    for path, run in runs.items():
        _same(run, runs["two_phase_w%d" % waves], "%s %s against the two-phase kernel" % (name, path))


@pytest.mark.parametrize("path", BURN_PATHS)
@pytest.mark.parametrize("name", list(MODELS))
@pytest.mark.parametrize("case", ["box_not_in_range", "across_the_guard"])
def test_burn_in_through_the_guard(case, name, path, monkeypatch):
    """burn_in_only through both calibration kernels (steps of 10 % and 5 % of the prior range): with pmax of the
    frequencies at 100 and a datum at 1e12 the guard cuts the box at f = 5.6, with the ordinary box and a datum at 2e13
    at 0.28; the guarded oracle's chain either way"""
    n_chain, waves = 3, PATHS[path][0]
    x_far = X_FAR_INSIDE if case == "box_not_in_range" else X_FAR_CUT
    w, st, lad, rng = _problem(name, waves, x_far, cut=case == "across_the_guard", n_chain=n_chain, init_prob=True)
    if case == "box_not_in_range":
        st.pmax[:, list(F_INDEX[name])] = 100.0
        to_oracle(st, lad)
    s = _sampler(w, n_chain, path, monkeypatch)
    s.set_state(st)
    status, iters = s.markov_chain_calibrate(0, n_chain, capi.calib_defaults(burn_in_iterations=BURN), burn_in_only=True)
    dev = s.get_state()
    s.close()
    assert not status.any() and not iters.any()
    with orc.sine_guard() as g:
        for c in range(n_chain):
            orc.burn_in(lad, rng, c, BURN)
    what = "burn_in %s %s %s" % (case, name, path)
    assert g.final >= 20, (what, g.final)
    assert np.array_equal(dev.step, st.step), what
    for f in ("accept", "reject", "n_iter", "swapcount", "params_accepts", "params_rejects"):
        assert np.array_equal(getattr(dev, f), getattr(lad, f)), "%s %s" % (what, f)
    assert np.array_equal(dev.ticks, rng.ticks), what + " ticks"
    for f in ("params", "params_best", "beta", "prior"):
        np.testing.assert_allclose(getattr(dev, f), getattr(lad, f), rtol=1e-9, atol=1e-300, err_msg="%s %s" % (what, f))
    # prob at the device's own parameters: with steps of 10 % of the range the kernel's Gaussian and libm's differ in
    # the last bits now and then, and with a datum at 2e13 two ulps of a frequency are 3e-5 of prob (sine3, one wave:
    # f of component 0 two ulps apart, prob -2.990813 against -2.990845, both sides bit-equal at the same parameters)
    with orc.sine_guard():
        for f, at in (("prob", dev.params), ("prob_best", dev.params_best)):
            want = [orc.loglike(w.model, p, w.data, beta=b)[0] for p, b in zip(at, dev.beta)]
            np.testing.assert_allclose(getattr(dev, f), want, rtol=1e-9, atol=1e-300, err_msg="%s %s" % (what, f))
    assert np.isfinite(dev.prob).all(), what
    for params in dev.params:
        assert all(ref.sine_in_range(params[j], params[j + 1], x_far) for j in F_INDEX[name]), (what, params)
    assert np.array_equal(dev.accept + dev.reject, np.full(n_chain, 400, dtype=np.uint64)), what


@pytest.mark.parametrize("name,path", [("simplesin", "two_phase_w1"), ("simplesin", "one_barrier_w4"),
                                       ("sine3", "one_barrier_w8"), ("sine3", "two_phase_w4")])
def test_a_batch_of_a_cut_ladder_and_an_ordinary_one(name, path, monkeypatch):
    """a ladder batch keeps max |x| per ladder: ladder 0 holds the datum at 2e13 and is cut by the guard, ladder 1 is the
    plain workload with its box in range; each is its stand-alone sampler bit for bit"""
    import torch
    waves, flags, _ = PATHS[path]
    monkeypatch.delenv("APEMOST_OB_HELPER", raising=False)
    probs = [_problem(name, waves, X_FAR_CUT, cut=True, seed=41), _problem(name, waves, None, cut=False, seed=42, data_seed=77)]
    w = probs[0][0]
    with orc.sine_guard() as g:
        orc.run_sampler(probs[0][2], probs[0][3], sum(PIECES_CUT), N_SWAP)
        cut = g.count()
        orc.run_sampler(probs[1][2], probs[1][3], sum(PIECES_CUT), N_SWAP)
        assert cut >= 20 and g.count() == cut
    batch = HipSampler.batch(w.model, w.n_par, N_CHAIN, np.stack([p[0].data for p in probs]), [41, 42],
                             waves_per_chain=waves, flags=flags)
    both = LadderState(2 * N_CHAIN, w.n_par)
    for f in ALL_FIELDS:
        getattr(both, f)[...] = np.concatenate([getattr(p[1], f) for p in probs])
    batch.set_state(both)
    d = torch.zeros((sum(PIECES_CUT) * N_SWAP, 2 * N_CHAIN, w.n_par + 2), dtype=torch.float64, device="cuda")
    batch.run_sampler(sum(PIECES_CUT), N_SWAP, d.data_ptr())
    batch.synchronize()
    got, rows = batch.get_state(), d.cpu().numpy()
    batch.close()
    for b, (wb, st, lad, rng) in enumerate(probs):
        alone = _run(wb, st, path, monkeypatch, seed=(41, 42)[b], pieces=PIECES_CUT)
        what = "%s %s ladder %d" % (name, path, b)
        for f in FIELDS:
            assert np.array_equal(batch.ladder_view(getattr(got, f), b), getattr(alone[0], f)), "%s: %s differs" % (what, f)
        assert np.array_equal(_bits(batch.ladder_view(rows, b)), _bits(alone[1])), what + ": rows differ"
        assert_match(alone[0], lad, rng, what=what)
    _in_range_everywhere(name, w, X_FAR_CUT, batch.ladder_view(rows, 0), types.SimpleNamespace(
        params=got.params[:N_CHAIN], prob=got.prob[:N_CHAIN], accept=got.accept[:N_CHAIN], reject=got.reject[:N_CHAIN]),
        name + " " + path + " ladder 0")
