"""A user-supplied device likelihood in the one-barrier kernels (APEMOST_HIP_FLAG_USER_ONE_BARRIER,
pt_onebarrier.h lik_step_user): every likelihood wave and the owner call the user's finish() on the data sum
and apply the reference's check_accept, so the chain is bit-identical to the two-phase kernels' -- round
shapes, the redraw path, the calibration, ties of the accept comparison included -- and to the oracle's
restatement of the reference's apps to 1e-9."""
import os
import subprocess
import time

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler
from apemost_amd.state import LadderState
from oracle import oracle as orc
from tests import hostlib
from tests.helpers import assert_match, to_oracle

pytestmark = pytest.mark.gpu

MODELS = os.path.join(hostlib.HOST, "examples", "device_models")
OB = capi.FLAG_USER_ONE_BARRIER
FIELDS = ("params", "params_best", "prob", "prob_best", "prior", "accept", "reject", "swapcount", "ticks", "n_iter",
          "params_accepts", "params_rejects", "step")


def _sine2(n_data=300):
    rs = np.random.RandomState(4)
    x = 100 + 0.5 * np.arange(n_data)
    y = 0.8 * np.sin(2 * np.pi * (0.21 * x + 0.3312)) + rs.normal(0, 0.5, n_data)
    box = dict(start=np.array([0.9, 0.2]), pmin=np.array([0.0, 0.0]), pmax=np.array([2.0, 0.3]))
    return np.stack([x, y], 1), box


def _bernoulli(n_data=257):
    rs = np.random.RandomState(5)
    X = rs.normal(0, 1, (n_data, 2))
    eta = 0.3 + 1.1 * X[:, 0] - 0.7 * X[:, 1]
    out = (rs.uniform(size=n_data) < 1 / (1 + np.exp(-eta))).astype(float)
    box = dict(start=np.array([0.0, 0.0, 0.0]), pmin=np.array([-5.0] * 3), pmax=np.array([5.0] * 3))
    return np.column_stack([out, X]), box


def _normal(n_data=4):
    box = dict(start=np.array([3.0]), pmin=np.array([0.0]), pmax=np.array([9000.0]))
    return np.zeros((n_data, 2)), box


CASES = {"simplesin2": (_sine2, orc.MODEL_SINE2), "bernoulli_example": (_bernoulli, orc.MODEL_BERNOULLI),
         "normal": (_normal, orc.MODEL_NORMAL)}


def _ladder(name, n_chain, step_scale=0.03, **make_kw):
    """(data, box, start state, oracle ladder at the same state)"""
    make, omodel = CASES[name]
    data, box = make(**make_kw)
    n_par = len(box["start"])
    st = LadderState.from_params(n_chain, box["start"], box["pmin"], box["pmax"], (box["pmax"] - box["pmin"]) * step_scale)
    for i in range(n_chain):
        st.beta[i] = orc.get_chain_beta(orc.LADDER_CHEBYSHEV_BETA, i, n_chain, 0.05) if n_chain > 1 else 1.0
        st.step[i] = np.minimum(st.step[i] * st.beta[i] ** -0.5, box["pmax"] - box["pmin"])
    lad = orc.Ladder(omodel, n_chain, n_par, data)
    to_oracle(st, lad)
    for c in range(n_chain):
        orc.calc_model(lad, c)
    st.prob[:], st.prior[:] = lad.prob, lad.prior
    return data, box, st, lad


def _sampler(name, data, n_par, n_chain, st, waves, flags, seed, src=None):
    s = HipSampler(wl.MODEL_USER, n_par, n_chain, data, seed=seed, waves_per_chain=waves, flags=flags,
                   device_model_source=src or os.path.join(MODELS, name + ".hip"))
    s.set_state(st)
    return s


def _run(name, data, n_par, st, waves, flags, seed, n_rounds, n_swap, pieces=None):
    import torch
    n_chain = len(st.prob)
    s = _sampler(name, data, n_par, n_chain, st, waves, flags, seed)
    policy = s.launch_policy[0]
    d = torch.zeros((n_rounds * n_swap, n_chain, n_par + 2), dtype=torch.float64, device="cuda")
    done = 0
    for k in (pieces or (n_rounds,)):
        s.run_sampler(k, n_swap, d[done * n_swap:].data_ptr())
        done += k
    s.synchronize()
    out = s.get_state(), d.cpu().numpy(), policy
    s.close()
    return out


def _same(a, b, what):
    for f in FIELDS:
        assert np.array_equal(getattr(a, f), getattr(b, f)), (what, f)


@pytest.mark.parametrize("name", sorted(CASES))
@pytest.mark.parametrize("waves", [4, 8])
def test_user_one_barrier_equals_two_phase_kernel_and_oracle(name, waves):
    """8 chains, 60 rounds x 11 steps with swaps: the one-barrier kernel (launch policy 1) gives the two-phase
    kernel's state and sample rows bit for bit and the oracle's to 1e-9; then the calibration: status and
    sweep counts exact against the oracle, the state bit-identical to the two-phase calibration's"""
    import torch
    n_chain, seed, n_rounds, n_swap = 8, 71, 60, 11
    data, box, st, lad = _ladder(name, n_chain)
    n_par = len(box["start"])
    dcfg = capi.calib_defaults(burn_in_iterations=400, iter_limit=20000)
    out = {}
    for flags in (OB, 0):
        s = _sampler(name, data, n_par, n_chain, st, waves, flags, seed)
        assert bool(s.launch_policy[0]) == (flags == OB)
        d = torch.zeros((n_rounds * n_swap, n_chain, n_par + 2), dtype=torch.float64, device="cuda")
        s.run_sampler(n_rounds, n_swap, d.data_ptr())
        s.synchronize()
        run = s.get_state()
        status, iters = s.markov_chain_calibrate(0, n_chain, dcfg)
        out[flags] = (run, d.cpu().numpy(), np.array(status), np.array(iters), s.get_state())
        s.close()
    a, sa = out[OB][0], out[OB][1]
    _same(a, out[0][0], "run " + name)
    assert np.array_equal(sa, out[0][1])
    rng = orc.Rng(orc.RNG_STREAMS, seed, lad)
    rows = orc.run_sampler(lad, rng, n_rounds, n_swap, record=True)
    assert_match(a, lad, rng, what="user one-barrier run " + name)
    np.testing.assert_allclose(sa, rows, rtol=1e-9, atol=1e-300)
    assert np.array_equal(out[OB][2], out[0][2]) and np.array_equal(out[OB][3], out[0][3])
    _same(out[OB][4], out[0][4], "calibration " + name)
    ocfg = orc.calib_defaults(burn_in_iterations=400, iter_limit=20000)
    for c in range(n_chain):
        assert (int(out[OB][2][c]), int(out[OB][3][c])) == orc.markov_chain_calibrate(lad, rng, c, ocfg), c
    assert_match(out[OB][4], lad, rng, what="user one-barrier calibration " + name)


@pytest.mark.parametrize("waves", [4, 8])
@pytest.mark.parametrize("n_swap", [1, 2, 15])
def test_user_one_barrier_round_shapes(n_swap, waves):
    """rounds of one step, of two, of many; launches cut at arbitrary rounds; single-round launches: all
    bit-identical to one another and to the two-phase kernel"""
    n_chain, seed, n_rounds = 16, 5, 90
    data, box, st, lad = _ladder("simplesin2", n_chain, n_data=1024)
    a, sa, pa = _run("simplesin2", data, 2, st, waves, OB, seed, n_rounds, n_swap)
    assert pa
    for flags, pieces in ((OB, (1, 7, 40, 42)), (OB | capi.FLAG_SINGLE_ROUND_LAUNCHES, None), (0, None)):
        o, so, _ = _run("simplesin2", data, 2, st, waves, flags, seed, n_rounds, n_swap, pieces=pieces)
        _same(a, o, (flags, pieces))
        assert np.array_equal(sa, so), (flags, pieces)
    rng = orc.Rng(orc.RNG_STREAMS, seed, lad)
    ref = orc.run_sampler(lad, rng, n_rounds, n_swap, record=True)
    assert_match(a, lad, rng, what="user one-barrier round shape %d waves %d" % (n_swap, waves))
    np.testing.assert_allclose(sa, ref, rtol=1e-9, atol=1e-300)


def test_user_one_barrier_redraw_path():
    """step widths of six times the prior box: the prepared attempts fail and the workgroup takes the redraw
    path (an extra barrier) all the time; the re-drawn row is the one the next step decides on"""
    n_chain, seed = 4, 3
    data, box, st, lad = _ladder("simplesin2", n_chain)
    st.step[:] = (box["pmax"] - box["pmin"]) * 6.0
    lad.step[:] = st.step
    for waves in (4, 8):
        dev, samples, policy = _run("simplesin2", data, 2, st, waves, OB, seed, 12, 5)
        two, samples2, _ = _run("simplesin2", data, 2, st, waves, 0, seed, 12, 5)
        assert policy
        _same(dev, two, "redraw waves %d" % waves)
        assert np.array_equal(samples, samples2)
        lad2 = orc.Ladder(orc.MODEL_SINE2, n_chain, 2, data)
        to_oracle(st, lad2)
        rng2 = orc.Rng(orc.RNG_STREAMS, seed, lad2)
        ref = orc.run_sampler(lad2, rng2, 12, 5, record=True)
        assert_match(dev, lad2, rng2, what="user one-barrier wide steps waves=%d" % waves)
        np.testing.assert_allclose(samples, ref, rtol=1e-9, atol=1e-300)


def test_user_one_barrier_injected_ties_follow_the_reference_rule(capsys):
    """The tie of check_accept injected as in test_gpu_one_barrier.test_injected_ties_of_the_accept_comparison:
    `prob` set to prob_new - ln U of the coming step, moved by k = -12..12 units u, one step through
    apemost_hip_launch_round.  The user form decides with the reference's comparison itself: the decisions
    equal the reference rule for every k -- there is no window."""
    import torch
    kRange, n_chain, seed, n_par = 12, 8, 61, 2
    data, box, st, lad = _ladder("simplesin2", n_chain)
    st.prob[:] = -1e10                           # quirk Q2: the first proposal is accepted whatever it is

    def one_step(state):
        s = _sampler("simplesin2", data, n_par, n_chain, state, 4, OB, seed)
        assert s.launch_policy[0]
        d = torch.zeros((1, n_chain, n_par + 2), dtype=torch.float64, device="cuda")
        s.launch_round(1, False, d.data_ptr())
        s.synchronize()
        out = s.get_state(), d.cpu().numpy()[0]
        s.close()
        return out

    first, rows = one_step(st)
    assert np.all(first.accept == 1)
    prob_new = rows[:, n_par].copy()
    prior = prob_new - rows[:, n_par + 1]
    ln_u = np.array([orc.accept_log_uniform(seed, c, n_par, 0) for c in range(n_chain)])
    assert np.all(ln_u < 0)
    tie = prob_new - ln_u
    unit = 2.0 ** -52 * np.maximum.reduce([np.abs(prob_new), np.abs(prior), np.abs(ln_u), np.abs(tie)])
    n_acc = np.zeros(n_chain, int)
    for k in range(-kRange, kRange + 1):
        inj = st.copy()
        p = tie + k * unit
        inj.prob[:] = p
        ref = (prob_new == p) | (prob_new > p) | (ln_u < prob_new - p)
        got, rows_k = one_step(inj)
        assert np.array_equal(got.accept == 1, ref), k
        acc = got.accept == 1
        assert np.array_equal(rows_k[acc, :n_par], rows[acc, :n_par]), k
        n_acc += acc
    with capsys.disabled():
        print("\n[simplesin2, user one-barrier] accepts of the 25 injected ties per chain: %s" % n_acc.tolist())
    assert np.all(n_acc > 0) and np.all(n_acc < 2 * kRange + 1)   # the tie lies inside the injected range


def test_user_one_barrier_variant_and_errors():
    """a logistic-proposal sampler under the flag runs the one-barrier round kernel and matches the oracle; its
    calibration stays on the two-phase kernel (bit-identical to the flag-off sampler's); the flag on a built-in
    model is refused"""
    n_chain, seed = 4, 62
    data, box, st, lad = _ladder("simplesin2", n_chain)
    flags = capi.FLAG_PROPOSAL_LOGISTIC
    states = {}
    for extra in (OB, 0):
        s = _sampler("simplesin2", data, 2, n_chain, st, 4, flags | extra, seed)
        assert bool(s.launch_policy[0]) == bool(extra)
        s.run_sampler(20, 5)
        s.synchronize()
        run = s.get_state()
        status, iters = s.markov_chain_calibrate(0, n_chain, capi.calib_defaults(burn_in_iterations=400, iter_limit=4000))
        states[extra] = (run, s.get_state(), np.array(status), np.array(iters))
        s.close()
    _same(states[OB][0], states[0][0], "logistic run")
    _same(states[OB][1], states[0][1], "logistic calibration")
    assert np.array_equal(states[OB][2], states[0][2]) and np.array_equal(states[OB][3], states[0][3])
    lad.proposal = orc.PROPOSAL_LOGISTIC
    rng = orc.Rng(orc.RNG_STREAMS, seed, lad)
    orc.run_sampler(lad, rng, 20, 5)
    assert_match(states[OB][0], lad, rng, what="user one-barrier, logistic proposals")
    w = wl.simplesin(n_data=256, n_chain=4)
    with pytest.raises(capi.ApemostHipError) as err:
        HipSampler(w.model, w.n_par, 4, w.data, seed=1, flags=OB)
    assert "USER_ONE_BARRIER" in str(err.value)


def test_c_application_output_is_the_same_with_the_flag(tmp_path):
    """examples/sine2_model.c with APEMOST_DEVICE_MODEL_SRC=simplesin2.hip: its three phases with and without
    APEMOST_FLAGS=1024 write byte-identical files"""
    n_beta, burn, iters = 5, 400, 2000
    data, box = _sine2(1024)
    exe = hostlib.make(str(tmp_path / "sine2.exe"), app=os.path.join(hostlib.HOST, "examples", "sine2_model.c"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=%d -DMAX_ITERATIONS=%d" % (n_beta, burn, iters))
    outs = {}
    for flags in ("1024", None):
        work = tmp_path / ("w%s" % flags)
        work.mkdir()
        (work / "params").write_text("".join("%.15e\t%.15e\t%.15e\t%s\t-1\n" % (s0, lo, hi, nm) for s0, lo, hi, nm in
                                             zip(box["start"], box["pmin"], box["pmax"], ("amplitude", "frequency"))))
        (work / "data").write_text("".join("%.17e\t%.17e\n" % tuple(r) for r in data))
        env = dict(os.environ, APEMOST_SEED="13", APEMOST_DEVICE_MODEL_SRC=os.path.join(MODELS, "simplesin2.hip"))
        env.pop("APEMOST_FLAGS", None)
        if flags:
            env["APEMOST_FLAGS"] = flags
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=600)
        outs[flags] = {p: (work / p).read_bytes() for p in sorted(os.listdir(str(work)))}
    assert sorted(outs["1024"]) == sorted(outs[None]) and len(outs[None]) > 3
    for p in outs[None]:
        assert outs["1024"][p] == outs[None][p], p


def test_user_one_barrier_rate(tmp_path, capsys):
    """simplesin2, 16 chains, flag on and off alternated in one process, each timed on run_sampler(200, 50) after
    a warm-up: at 1024 points and 4 waves the one-barrier kernel takes the serial phase off the step (>= 1.15x);
    at 8192 points and 8 waves the likelihood dominates (>= 0.97x).  Prints both rates and hiprtc's compile times."""
    src = tmp_path / "simplesin2_rate.hip"       # (a source of its own: compiled here, not taken from the process's cache)
    src.write_text(open(os.path.join(MODELS, "simplesin2.hip")).read() + "\n/* rate test */\n")
    n_chain, reps = 16, 3
    lines, ratios = [], {}
    for n_data, waves in ((1024, 4), (8192, 8)):
        data, box = _sine2(n_data)
        st = LadderState.from_params(n_chain, box["start"], box["pmin"], box["pmax"], (box["pmax"] - box["pmin"]) * 0.03)
        samplers, compile_s, best = {}, {}, {OB: 0.0, 0: 0.0}
        for flags in (OB, 0):
            s = _sampler("simplesin2", data, 2, n_chain, st, waves, flags, 3, src=str(src))
            assert s.geometry[0] == waves and bool(s.launch_policy[0]) == bool(flags)
            compile_s[flags] = s.user_model_compile_seconds
            s.calc_model(0, n_chain)
            s.run_sampler(4, 50)
            s.synchronize()
            samplers[flags] = s
        for _ in range(reps):
            for flags in (OB, 0):
                s = samplers[flags]
                t0 = time.perf_counter()
                s.run_sampler(200, 50)
                s.synchronize()
                best[flags] = max(best[flags], 200 * 50 * n_chain / (time.perf_counter() - t0))
        _same(samplers[OB].get_state(), samplers[0].get_state(), "rate run %d" % n_data)
        for s in samplers.values():
            s.close()
        ratios[n_data] = best[OB] / best[0]
        lines.append("%d points, %d waves: %.3g (one-barrier) vs %.3g (two-phase) steps/s = %.2fx; hiprtc %.2f s (flag) / %.2f s"
                     % (n_data, waves, best[OB], best[0], ratios[n_data], compile_s[OB], compile_s[0]))
    with capsys.disabled():
        print("\n[simplesin2, 16 chains] " + "\n[simplesin2, 16 chains] ".join(lines))
    assert ratios[1024] >= 1.15
    assert ratios[8192] >= 0.97
