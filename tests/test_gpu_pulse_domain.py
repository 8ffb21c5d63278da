"""The pulse and pulse_vrot likelihoods on the card, held to the error budget derived in tests/pulse_domain.py, through the
existing ABI alone (HipSampler.loglike, set_data, run_sampler, burn_in_only, HipSampler.batch): no probe kernel, no hook.

  1. the table logarithm read back bit for bit out of the returned prior, at every argument of log_arguments();
  2. LogProdT::finish read back: one point with d = 0, the heights swept so that m / md crosses every table bin;
  3. every loop form at ordinary units, every model and wave count, |prob - exact| within the budget;
  4. the sweep of units: accuracy on both sides of every range guard, the band at the top of the range included;
  5. one wave of a workgroup falls back, its neighbours do not (far_point);
  6. sampling across a guard on every kernel path, through burn_in_only and in a ladder batch.

The exact value is 240-bit mpmath from the double inputs; the budget's constants are counted roundings, not outputs."""
import math
import types

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler
from apemost_amd.state import ALL_FIELDS, LadderState
from oracle import oracle as orc
from tests import data_lengths as dl
from tests import pulse_domain as pd
from tests.helpers import assert_match, make_pair, to_oracle
from tests.test_gpu_ladder_edges import FIELDS, PATHS, _policy

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _err(got, want_mpf):
    return abs(float(pd.MP.mpf(float(got)) - want_mpf))


# ---- 1. the table logarithm, bit for bit -------------------------------------------------------------------------------
def _height_arguments():
    """every argument of log_arguments() a height can carry: with hmin = 0 the kernel's h + hmin is h itself, any normal
    double (the class finish_long and the exponents of finish belong to test 2: a height has no exponent to add)"""
    xs = [x for cls, (x, e) in pd.log_arguments().items() if cls != "finish_long"]
    return np.unique(np.concatenate(xs))


@pytest.mark.parametrize("name", ["pulse1", "pulse_vrot"])
@pytest.mark.parametrize("waves", dl.WAVES)
def test_table_logarithm_read_back_from_the_prior(name, waves):
    """The returned prior of a one-mode pulse is ldexp(-log(h + hmin), 0), of pulse_vrot -(log(ha + hmin) +
    log(hb + hmin)) / 2 with hb = 1 and hmin = 0: that logarithm is exactly 0 and the halving is exact.  Which
    logarithm: Engine::setup_lanes is set_lean's only caller in the loglike kernel, with kLean = (WAVES == 1) -- so two
    waves and more read the table (the one-barrier engines call set_lean(false) always) and must equal
    pulse_domain.dev_log bit for bit, which tests/test_pulse_domain_cpu.py holds to LOG_WORST_MEASURED against mpmath;
    the one-wave kernels take ocml's log, which is not this project's code: 1e-13 as before."""
    x = _height_arguments()
    params = np.zeros((len(x), pd.n_par(name)))
    params[:, 0], params[:, 1] = 5.0, 0.05
    if name == "pulse1":
        params[:, 2], params[:, 3] = 10.9, x
    else:
        params[:, 2:] = (0.05, 10.6, 0.0, 11.3, 1.0)
        params[:, 4] = x
    data = np.array(pd.base_data(name, 3))
    s = HipSampler(pd.model_id(name), pd.n_par(name), 2, data, waves_per_chain=waves, hmin=0.0)
    assert s.geometry[0] == waves
    _, prior = s.loglike(params, 1.0)
    s.close()
    model = pd.dev_log(x)
    want = -model if name == "pulse1" else -(0.0 + model + 0.0) / 2.0
    if waves == 1:
        true = np.array([float(-pd.true_log(v)) for v in x]) / (1.0 if name == "pulse1" else 2.0)
        np.testing.assert_allclose(prior, true, rtol=1e-13, atol=1e-300)
        return
    bad = np.flatnonzero(_bits(prior) != _bits(want))
    assert len(bad) == 0, "%s waves=%d: %d of %d priors differ from the modelled table logarithm, first at x = %r (bin %d): %r != %r" % (
        name, waves, len(bad), len(x), x[bad[0]], pd.log_index(x[bad[:1]])[0][0], prior[bad[0]], want[bad[0]])


# ---- 2. LogProdT::finish -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4])
def test_finish_read_back_across_every_table_bin(waves):
    """one data point (nu, 0), one-mode pulse, p1 = 0, beta = 1, hmin = 0: every lane but one holds the empty product
    (ln 1 = 0, added exactly), so prob - prior = -ln(N / D) as finish() takes it from the mantissas of N = h c and
    D = q.  Budget: the point's own eps (c_tau 5, q 3, N 1) and div_fast's 1.5 ulp on the argument, the logarithm's
    bound on the result, one rounding of prior - S.  One wave: finish<true>, ocml's log; four: finish<false>, the table."""
    name = "pulse1"
    hs = np.concatenate([2.0 ** (np.arange(1024) / 1024.0) * 1.37, 2.0 ** (np.arange(0, 1024, 7) / 1024.0) * 3.1e40,
                         2.0 ** (np.arange(0, 1024, 7) / 1024.0) * 4.7e-35])
    tau, f, nu = 5.0, 10.9, 10.83
    params = np.zeros((len(hs), 4))
    params[:, 0], params[:, 2], params[:, 3] = tau, f, hs
    data = np.array([[nu, 0.0]])
    # the restated argument of the logarithm crosses every bin
    mod = [pd._Model(name, p) for p in params[:1]][0]
    n_, d_ = mod.nd(np.array([nu] * 8))
    v = np.frexp(hs * mod.c)[0] * pd.rcp_nr(np.frexp(d_[0])[0])
    assert len(set(pd.log_index(v)[0].tolist())) == 256
    s = HipSampler(wl.MODEL_PULSE, 4, 2, data, waves_per_chain=waves, hmin=0.0)
    prob, prior = s.loglike(params, 1.0)
    s.close()
    f_ = pd.MP.mpf
    a = f_(pd.TWO_PI) * (f_(f) - f_(nu)) * f_(tau)
    worst = 0.0
    for h, pb, pr in zip(hs, prob, prior):
        ln_y = pd.MP.log(f_(float(h)) / (1 + a * a))
        c_log = (5 + 3 * abs(float(ln_y))) if waves == 1 else 2 * pd.LOG_WORST_ULP * abs(float(ln_y))
        bud = pd.U * (1 + 2.0 ** -20) * (9 + 3 + c_log + abs(float(pb)))
        err = _err(pb, f_(float(pr)) - ln_y)
        worst = max(worst, err / bud)
        assert err <= bud, "waves=%d h=%r: finish is %.3g from ln y, budget %.3g" % (waves, h, err, bud)
    print("finish waves=%d: worst error / budget %.3f over %d heights" % (waves, worst, len(hs)))


# ---- 3. every loop form at ordinary units ------------------------------------------------------------------------------
BETAS = (1.0, 0.37, 0.05)


def _evaluate(s, name, waves, n, rows, a=0, b=0, data=None):
    """loglike of base rows `rows` in the units (a, b) on the sampler s (its data set here); per row (error, budget,
    restated evaluation), finite-ness and the budget asserted"""
    base = pd.base_data(name, n) if data is None else data
    p0 = pd.base_params(name)
    sc = pd.scaled(name, p0[list(rows)], base, a, b)
    assert sc is not None
    params, d = sc
    beta = np.array([BETAS[r] for r in rows])
    s.set_data(d)
    prob, _ = s.loglike(params, beta)
    out = []
    for j, r in enumerate(rows):
        ex = pd.exact(name, p0[r], len(base), beta[j], a, b, data=data)
        dev = pd.device_eval(name, params[j], d, beta[j], waves)
        bud = pd.prob_budget(name, ex, pd.kappa(name, p0[r], base), waves, dev)
        what = "%s waves=%d n=%d row=%d a=%d b=%d class %s %s" % (name, waves, len(base), r, a, b, dev.cls, dev.classes)
        assert math.isfinite(prob[j]), what + ": prob is %r where the exact value is %.17g" % (prob[j], float(ex.prob))
        err = _err(prob[j], ex.prob)
        print("%s: error %.3g budget %.3g" % (what, err, bud))
        assert err <= bud, "%s: prob %.17g is %.3g from the exact value, budget %.3g" % (what, prob[j], err, bud)
        out.append((err, bud, dev))
    return out


@pytest.mark.parametrize("name", pd.NAMES)
@pytest.mark.parametrize("waves", dl.WAVES)
def test_every_loop_form_at_ordinary_units(name, waves):
    worst = 0.0
    for n in pd.sweep_lengths(waves, name):
        s = HipSampler(pd.model_id(name), pd.n_par(name), 2, np.array(pd.base_data(name, n)), waves_per_chain=waves)
        assert s.geometry[0] == waves
        res = _evaluate(s, name, waves, n, (n % 3, (n + 1) % 3))
        s.close()
        assert all(dev.cls in ("quad", "pair") for _, _, dev in res)
        worst = max([worst] + [e / b for e, b, _ in res])
    print("%s waves=%d: worst error / budget %.3f" % (name, waves, worst))


# ---- 4. the sweep of units ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", pd.NAMES)
@pytest.mark.parametrize("waves", [1, 4])
def test_sweep_of_units(name, waves):
    """every scale of units(name): prob finite and within the budget of the form the restatement names (edge: the
    larger of the two neighbours'), on both sides of every threshold -- a guard one binade too late or too early is an
    error here, not a classification.  TOP_BAND (pulse_domain.units): the pair product N0 N1 in [2^1022, 2^1024), whose
    reciprocal is a subnormal that a flushing v_rcp_f64 would turn into a vanished d / y under a finite sum (it does not
    flush: the band is right).  What kPairExponent guards: a pair product of the numerators below 2^-1024 already makes
    its reciprocal overflow and the sum NaN, so bad() holds there whatever the threshold; what the threshold adds is the
    denominators' product, whose mantissa goes into ln of the lane's product after it lost -1022 - e bits as a subnormal
    (2^-35 on one pair at e = -1040).  The units tagged fine_a_den (b = 16) are where that shows: with the guard moved
    to 1040 on a scratch build the worst error of the sweep rises from 0.11 to 0.785 of the budget (one-mode pulse,
    four waves; the restatement predicts 0.794) and the sweep still passes: 2^-35 on a few pairs of a 515-point sum is
    what a worst-case budget allows, and the guard has that much room.  At 1050 seven of these twelve cases fail, at the
    fine_a_den units, by 1e-8 .. 1e-7 against budgets of 1e-11."""
    n = pd.unit_length(waves)
    s = HipSampler(pd.model_id(name), pd.n_par(name), 2, np.array(pd.base_data(name, n)), waves_per_chain=waves)
    worst, band = {}, 0
    for a, b, tag in pd.units(name):
        if pd.scaled(name, pd.base_params(name)[:2], pd.base_data(name, n), a, b) is None:
            continue
        rows = (0, 1) if tag == pd.TOP_BAND else (0,)
        for err, bud, dev in _evaluate(s, name, waves, n, rows, a, b):
            worst[dev.cls] = max(worst.get(dev.cls, 0.0), err / bud)
            band += tag == pd.TOP_BAND and dev.cls in ("pair", "edge")
    s.close()
    assert band > 0
    print("%s waves=%d: worst error / budget per class %s" % (name, waves, {k: round(v, 3) for k, v in sorted(worst.items())}))


# ---- 5. one wave falls back ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in pd.NAMES if n != "pulse1"])
@pytest.mark.parametrize("waves", [2, 4, 8])
def test_one_wave_falls_back_its_neighbours_do_not(name, waves):
    for last in (False, True):
        data, idx = pd.far_point(name, waves, last)
        s = HipSampler(pd.model_id(name), pd.n_par(name), 2, data, waves_per_chain=waves)
        res = _evaluate(s, name, waves, len(data), (0, 1, 2), data=data)
        s.close()
        w = (idx % (64 * waves)) // 64
        for _, _, dev in res:
            assert dev.classes[w] == "ref" and dev.classes.count("pair") == waves - 1, dev.classes


# ---- 6. sampling across a guard ----------------------------------------------------------------------------------------
N_CHAIN, N_SWAP, PIECES, SEED = 4, 5, (4, 8), 5
SAMPLING = {"pulse2": -492, "pulse_vrot": -486}     # b: heights and data x 2^b; see _problem


def _problem(name, waves, far=False, b=None, n_chain=N_CHAIN, seed=SEED, init_prob=False):
    """the workload in units in which the lifetime's prior box straddles the pair guard: heights and data x 2^b, so that
    the smallest pair product N0 N1 ~ (h c q)^2 sits at 2^-1000 for a lifetime near the start (c = 1 / (2 pi tau)^2:
    a longer lifetime falls back, a shorter one does not).  far: ordinary units and far_point's datum instead."""
    kern = pd.kernel_name(name)
    n = 2 * 64 * waves + 1
    src = wl.by_name(kern, n_data=n, n_chain=n_chain)
    b = (0 if far else SAMPLING[name]) if b is None else b
    data = pd.far_point(name, waves, True)[0] if far else np.array(src.data)
    data[:, 1] = np.ldexp(data[:, 1], b)
    hc = pd.height_columns(name)
    start, pmin, pmax, step = (np.array(v, dtype=np.float64) for v in (src.start, src.pmin, src.pmax, src.step * 0.3))
    for v in (start, pmin, pmax, step):
        v[hc] = np.ldexp(v[hc], b)
    pmin[hc] = np.ldexp(0.5, b)                      # (heights of 0: y = 0 and NaN on both sides, not what this is about)
    w = types.SimpleNamespace(model=src.model, n_par=src.n_par, data=data, start=start, pmin=pmin, pmax=pmax, step=step,
                              n_data=n)
    st, lad, rng = make_pair(w, n_chain, seed=seed)
    if not far and b != 0:                           # the chains start either side of the guard and wander from there
        for c in range(n_chain):
            st.params[c, 0] = st.params_best[c, 0] = start[0] * (0.6, 1.7, 0.85, 1.25)[c % 4]
        to_oracle(st, lad)
    if init_prob:
        for c in range(n_chain):
            orc.calc_model(lad, c)
        st.prob[:], st.prior[:] = lad.prob, lad.prior
    return w, st, lad, rng


def _run(w, st, path, monkeypatch, n_chain=N_CHAIN, seed=SEED, pieces=PIECES):
    import torch
    waves, flags, helper = PATHS[path]
    if helper is None:
        monkeypatch.delenv("APEMOST_OB_HELPER", raising=False)
    else:
        monkeypatch.setenv("APEMOST_OB_HELPER", helper)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=seed, waves_per_chain=waves, flags=flags)
    assert s.geometry[0] == waves
    s.set_state(st)
    assert (_policy(s) != 0) == path.startswith("one_barrier"), path
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


def _classes(name, w, waves, rows):
    """how many visited states the restatement evaluates with a wave in a fast form (`fast`), with a wave that fell back
    (`ref`), and at an edge (counted in neither)"""
    out = {"fast": 0, "ref": 0, "edge": 0}
    for p in np.unique(rows[:, :, :w.n_par].reshape(-1, w.n_par), axis=0):
        dev = pd.device_eval(name, p, w.data, 1.0, waves)
        if dev.cls == "edge":
            out["edge"] += 1
            continue
        out["fast"] += any(c in ("pair", "quad") for c in dev.classes)
        out["ref"] += "ref" in dev.classes
    return out


@pytest.mark.parametrize("name", list(SAMPLING))
@pytest.mark.parametrize("waves,far", [(1, False), (2, False), (4, False), (8, False), (2, True), (4, True), (8, True)])
def test_sampling_across_the_pair_guard(name, waves, far, monkeypatch):
    """a ladder whose chains' lifetimes wander across the pair guard (far: whose last wave alone falls back at every
    step): counters and ticks are the oracle's, rows to 1e-9, and every kernel path of this wave count is the
    two-phase kernel bit for bit -- Engine::reduce_data_xy and ObEngine::lik_partial both decide per wave"""
    w, st, lad, rng = _problem(name, waves, far=far)
    ref_rows = orc.run_sampler(lad, rng, sum(PIECES), N_SWAP, record=True)
    seen = _classes(name, w, waves, ref_rows)
    print(name, waves, far, seen)
    assert seen["fast"] >= 5 and seen["ref"] >= 5, seen
    assert lad.accept.min() > 0
    runs = {}
    for path in [p for p in PATHS if PATHS[p][0] == waves]:
        what = "%s %s far=%s" % (name, path, far)
        dev, rows = runs[path] = _run(w, st, path, monkeypatch)
        assert_match(dev, lad, rng, what=what)
        np.testing.assert_allclose(rows, ref_rows, rtol=1e-9, atol=1e-300, err_msg=what + " rows")
        assert np.isfinite(rows).all(), what
    for path, run in runs.items():
        _same(run, runs["two_phase_w%d" % waves], "%s %s against the two-phase kernel" % (name, path))


@pytest.mark.parametrize("path", ["two_phase_w1", "one_barrier_w4"])      # pt_calibrate_kernel and pt_calibrate_ob_kernel
def test_burn_in_across_the_pair_guard(path, monkeypatch):
    name, n_chain, waves, burn = "pulse2", 3, PATHS[path][0], 201
    w, st, lad, rng = _problem(name, waves, n_chain=n_chain, init_prob=True)
    monkeypatch.delenv("APEMOST_OB_HELPER", raising=False)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=SEED, waves_per_chain=waves, flags=PATHS[path][1])
    s.set_state(st)
    status, iters = s.markov_chain_calibrate(0, n_chain, capi.calib_defaults(burn_in_iterations=burn), burn_in_only=True)
    dev = s.get_state()
    s.close()
    assert not status.any() and not iters.any()
    for c in range(n_chain):
        orc.burn_in(lad, rng, c, burn)
    what = "burn_in %s %s" % (name, path)
    for f in ("accept", "reject", "n_iter", "swapcount", "params_accepts", "params_rejects"):
        assert np.array_equal(getattr(dev, f), getattr(lad, f)), "%s %s" % (what, f)
    assert np.array_equal(dev.ticks, rng.ticks), what + " ticks"
    for f in ("params", "params_best", "beta", "prior", "prob", "prob_best"):
        np.testing.assert_allclose(getattr(dev, f), getattr(lad, f), rtol=1e-9, atol=1e-300, err_msg="%s %s" % (what, f))
    cls = {pd.device_eval(name, p, w.data, 1.0, waves).cls for p in np.concatenate([dev.params, dev.params_best])}
    assert np.isfinite(dev.prob).all() and cls <= {"pair", "ref", "edge"}, (what, cls)


@pytest.mark.parametrize("path", ["two_phase_w1", "one_barrier_w4"])
def test_a_batch_of_a_straddling_ladder_and_an_ordinary_one(path, monkeypatch):
    """ladder 0 in the straddling units, ladder 1 in ordinary ones: each is its stand-alone sampler bit for bit"""
    import torch
    name = "pulse2"
    waves, flags, _ = PATHS[path]
    monkeypatch.delenv("APEMOST_OB_HELPER", raising=False)
    probs = [_problem(name, waves, seed=41), _problem(name, waves, b=0, seed=42)]
    w = probs[0][0]
    batch = HipSampler.batch(w.model, w.n_par, N_CHAIN, np.stack([p[0].data for p in probs]), [41, 42],
                             waves_per_chain=waves, flags=flags)
    both = LadderState(2 * N_CHAIN, w.n_par)
    for f in ALL_FIELDS:
        getattr(both, f)[...] = np.concatenate([getattr(p[1], f) for p in probs])
    batch.set_state(both)
    d = torch.zeros((sum(PIECES) * N_SWAP, 2 * N_CHAIN, w.n_par + 2), dtype=torch.float64, device="cuda")
    batch.run_sampler(sum(PIECES), N_SWAP, d.data_ptr())
    batch.synchronize()
    got, rows = batch.get_state(), d.cpu().numpy()
    batch.close()
    for b, (wb, st, lad, rng) in enumerate(probs):
        alone = _run(wb, st, path, monkeypatch, seed=(41, 42)[b], pieces=(sum(PIECES),))
        what = "%s %s ladder %d" % (name, path, b)
        for f in FIELDS:
            assert np.array_equal(batch.ladder_view(getattr(got, f), b), getattr(alone[0], f)), "%s: %s differs" % (what, f)
        assert np.array_equal(_bits(batch.ladder_view(rows, b)), _bits(alone[1])), what + ": rows differ"
        orc.run_sampler(lad, rng, sum(PIECES), N_SWAP)
        assert_match(alone[0], lad, rng, what=what)
