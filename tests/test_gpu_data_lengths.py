"""The data sum at the lengths where its loops change regime (tests/data_lengths.py): rows in registers, every pass
count and parity of the software-pipelined loop, the 4-wide and 2-wide loops, the 1-wide tail, ragged and idle
wavefronts, a staged vector of more than 64 KiB -- for every model at 1, 2, 4, 6 and 8 waves per chain, staged in LDS
(lds_policy 1) and read through L2 (lds_policy 2), in the loglike, round, one-barrier and calibration kernels and in
the indexed loops of a user-supplied model.  A tail that drops or repeats a point is an error of order 1 / n_data in
the log-likelihood: the 1e-12 gate sees it at once, at a length where that tail runs.

References: the extended-precision restatement (tests/loglike_ref.py) and the CPU oracle; every input is shown
well-conditioned on the CPU first (tests/test_data_lengths_cpu.py).  Bit-identity: staged against unstaged (the same
arithmetic on the same numbers in the same order), one-barrier against two-phase, helper on against helper off."""
import numpy as np
import pytest

from apemost_amd import capi
from apemost_amd.sampler import HipSampler
from oracle import oracle as orc
from tests import data_lengths as dl
from tests.helpers import assert_match, make_pair
from tests.test_gpu_ladder_edges import FIELDS, PATHS as EDGE_PATHS, _policy, _split_ok

pytestmark = pytest.mark.gpu

SHAPES = [(m, w) for m in dl.MODELS for w in dl.WAVES]
PATHS = dict(EDGE_PATHS, two_phase_w6=(6, 0, None))     # name: (waves, flags, APEMOST_OB_HELPER or None)
SEED, N_CHAIN, N_SWAP, PIECES = 5, 4, 5, (2, 4)         # 6 rounds of 5 steps in two launches
BURN = 201      # burn_in() steps in blocks of 200 while iter < burn / 2, then while iter < burn: one block each, the shortest
                # burn-in that runs both halves (src/markov_chain.c:34-79)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _expected_policy(path, name, beta):
    """0 two-phase, 1 one-barrier, 2 one-barrier with a helper wavefront (tests/test_gpu_ladder_edges.py)"""
    waves, flags, helper = PATHS[path]
    if waves not in dl.ONE_BARRIER_WAVES or flags & capi.FLAG_TWO_BARRIER_STEP:
        return 0
    return 2 if helper is None and name in ("pulse", "pulse_vrot") and _split_ok(beta) else 1


def _sampler(w, n_chain, path, policy, monkeypatch):
    waves, flags, helper = PATHS[path]
    if helper is None:
        monkeypatch.delenv("APEMOST_OB_HELPER", raising=False)
    else:
        monkeypatch.setenv("APEMOST_OB_HELPER", helper)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=SEED, waves_per_chain=waves, flags=flags, lds_policy=policy)
    assert s.geometry == (waves, policy == 1), (path, policy, s.geometry)
    return s


def _same_state(a, b, what, fields=FIELDS):
    for f in fields:
        assert np.array_equal(getattr(a, f), getattr(b, f)), "%s: %s differs" % (what, f)


# ---- (a) loglike at every length ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,waves", SHAPES)
def test_loglike_at_every_length(name, waves):
    """pt_loglike_kernel at every length of the matrix: prob within 1e-12 (BASELINE 3.6) of the extended
    reference and of the oracle, prior within 1e-13, a sampler that stages and one that does not equal bit for bit.
    (geometry reports the staging mode of the sampler's stepping kernels; apemost_hip_loglike itself reads through L2
    under either policy, so here the bit-identity holds the two samplers to one kernel -- the staging copy is compared
    by the sampling and calibration tests below.)"""
    worst = 0.0
    for n in dl.lengths(waves, name):
        c = dl.case(name, n)
        got = {}
        for policy in (1, 2):
            s = HipSampler(c.w.model, c.w.n_par, 2, c.w.data, waves_per_chain=waves, lds_policy=policy)
            assert s.geometry == (waves, policy == 1), (n, policy, s.geometry)
            got[policy] = s.loglike(c.params, c.beta)
            s.close()
        prob, prior = got[1]
        what = "%s waves=%d n_data=%d" % (name, waves, n)
        assert np.all(np.isfinite(prob)), what
        e_ext, e_orc = dl.rel_err(prob, c.ext_prob), dl.rel_err(prob, c.orc_prob)
        worst = max(worst, float(e_ext.max()))
        assert e_ext.max() <= 1e-12, "%s: prob %s from the extended reference" % (what, e_ext)
        assert e_orc.max() <= 1e-12, "%s: prob %s from the oracle" % (what, e_orc)
        assert dl.rel_err(prior, c.ext_prior).max() <= 1e-13 and dl.rel_err(prior, c.orc_prior).max() <= 1e-13, what + ": prior"
        assert np.array_equal(_bits(prob), _bits(got[2][0])), what + ": prob differs staged / unstaged"
        assert np.array_equal(_bits(prior), _bits(got[2][1])), what + ": prior differs staged / unstaged"
    print("%s waves=%d: largest error of prob against the extended reference %.3g" % (name, waves, worst))


# ---- (b) sampling at the shortest length of every regime ----------------------------------------------------------------
def _run(w, st, path, policy, monkeypatch):
    """run_sampler with swap attempts in two launches; (state, sample rows, launch policy)"""
    import torch
    s = _sampler(w, N_CHAIN, path, policy, monkeypatch)
    s.set_state(st)
    launch = _policy(s)
    d = torch.zeros((sum(PIECES) * N_SWAP, N_CHAIN, w.n_par + 2), dtype=torch.float64, device="cuda")
    done = 0
    for k in PIECES:
        s.run_sampler(k, N_SWAP, d[done * N_SWAP:].data_ptr())
        done += k
    s.synchronize()
    out = s.get_state(), d.cpu().numpy(), launch
    s.close()
    return out


@pytest.mark.parametrize("name,waves", SHAPES)
def test_sampling_at_every_regime(name, waves, monkeypatch):
    """4 chains, 6 rounds of 5 steps with swap attempts, cut into launches of 2 and 4 rounds, on every kernel of this
    wave count (two-phase; at 4 and 8 waves also one-barrier with and without the helper wavefront), staged and
    unstaged: the oracle's chain (counters and ticks exact, fp64 and every sample row to 1e-9), and ONE
    chain bit for bit whatever the kernel and the staging mode.  (SEED: a comparison of a step can land inside the
    1e-9 noise of the data sum, about 1e-10 per step; this seed does not.)"""
    paths = [p for p in PATHS if PATHS[p][0] == waves]
    base = "two_phase_w%d" % waves
    assert base in paths
    for n in dl.sampling_lengths(waves, name):
        w = dl.case(name, n).w
        st, lad, rng = make_pair(w, N_CHAIN, seed=SEED)
        ref = orc.run_sampler(lad, rng, sum(PIECES), N_SWAP, record=True)
        runs = {}
        for path in paths:
            for policy in (1, 2):
                what = "%s n_data=%d %s lds_policy=%d" % (name, n, path, policy)
                dev, rows, launch = runs[path, policy] = _run(w, st, path, policy, monkeypatch)
                assert launch == _expected_policy(path, name, st.beta), (what, launch)
                assert_match(dev, lad, rng, what=what)
                assert np.isfinite(rows)[np.isfinite(ref)].all(), what
                np.testing.assert_allclose(rows, ref, rtol=1e-9, atol=1e-300, err_msg=what + " rows")
        twin, twin_rows, _ = runs[base, 1]
        for (path, policy), (dev, rows, _) in runs.items():
            what = "%s n_data=%d: %s lds_policy=%d against %s staged" % (name, n, path, policy, base)
            _same_state(dev, twin, what)
            assert np.array_equal(_bits(rows), _bits(twin_rows)), what + ": rows differ"


# ---- (c) the calibration kernels ---------------------------------------------------------------------------------------------
CALIBRATION_SHAPES = [(m, w) for m in dl.MODELS for w in (1, 4, 6, 8)] + [("simplesin", 2), ("pulse_vrot", 2)]


@pytest.mark.parametrize("name,waves", CALIBRATION_SHAPES)
def test_calibration_kernels_at_the_edge_lengths(name, waves, monkeypatch):
    """pt_calibrate_kernel / pt_calibrate_ob_kernel (the same loops compiled under another register pressure): the
    shortest burn_in() that runs both of its halves, then markov_chain_step_for on every parameter, at T + 1,
    kWide * T and the longest length of the matrix; against orc.burn_in / orc.step_for (tests/test_gpu_calibration.py),
    staged and unstaged bit for bit -- and at 4 and 8 waves the one-barrier calibration kernel and the two-phase one
    bit for bit"""
    import torch
    n_chain, n_for = 3, 3
    paths = [p for p in PATHS if PATHS[p][0] == waves and not p.endswith("no_helper")]
    for n in dl.calibration_lengths(waves, name):
        w = dl.case(name, n).w
        st, lad, rng = make_pair(w, n_chain, seed=SEED, init_prob=True)
        for c in range(n_chain):
            orc.burn_in(lad, rng, c, BURN)
        burned = {f: getattr(lad, f).copy() for f in ("params", "prob", "prior", "accept", "reject")}
        ref = np.zeros((w.n_par, n_for, n_chain, w.n_par + 2))
        for p in range(w.n_par):
            for k in range(n_for):
                for c in range(n_chain):
                    orc.step_for(lad, rng, c, p)
                    orc.check_best(lad, c)
                    lad.n_iter[c] += 1
                    ref[p, k, c, :w.n_par] = lad.params[c]
                    ref[p, k, c, w.n_par] = lad.prob[c]
                    ref[p, k, c, w.n_par + 1] = lad.prob[c] - lad.prior[c]
        out = {}
        for path in paths:
            for policy in (1, 2):
                what = "%s n_data=%d %s lds_policy=%d" % (name, n, path, policy)
                s = _sampler(w, n_chain, path, policy, monkeypatch)
                s.set_state(st)
                status, iters = s.markov_chain_calibrate(0, n_chain, capi.calib_defaults(burn_in_iterations=BURN),
                                                         burn_in_only=True)
                assert not status.any() and not iters.any(), what
                mid = s.get_state()
                assert np.array_equal(mid.step, st.step), what                 # restored bit for bit
                assert np.array_equal(mid.accept, burned["accept"]) and np.array_equal(mid.reject, burned["reject"]), what
                for f in ("params", "prob", "prior"):
                    np.testing.assert_allclose(getattr(mid, f), burned[f], rtol=1e-9, atol=1e-300, err_msg="%s burn_in %s" % (what, f))
                d = torch.zeros(ref.shape, dtype=torch.float64, device="cuda")
                for p in range(w.n_par):
                    s.markov_chain_step_for(p, n_for, d[p].data_ptr())
                s.synchronize()
                dev, rows = s.get_state(), d.cpu().numpy()
                s.close()
                assert_match(dev, lad, rng, what=what)
                np.testing.assert_allclose(rows, ref, rtol=1e-9, atol=1e-300, err_msg=what + " step_for rows")
                out[path, policy] = mid, dev, rows
        first = out[paths[0], 1]
        for (path, policy), (mid, dev, rows) in out.items():
            what = "%s n_data=%d: %s lds_policy=%d against %s staged" % (name, n, path, policy, paths[0])
            _same_state(mid, first[0], what + " after burn_in", FIELDS + ("step",))
            _same_state(dev, first[1], what + " after step_for", FIELDS + ("step",))
            assert np.array_equal(_bits(rows), _bits(first[2])), what + ": step_for rows differ"


# ---- (d) a user-supplied model: the indexed loops ----------------------------------------------------------------------------
@pytest.mark.parametrize("waves", [1, 4, 8])
def test_user_model_at_ragged_lengths(waves):
    """Engine::reduce_data_indexed and ObEngine::lik_partial_user with the shipped simplesin2.hip at 1, T - 1, T + 1 and
    3 T + 1 points: loglike against the oracle's restatement of the app to 1e-12 and a run with swaps to 1e-9
    (the checks of tests/test_gpu_user_model.py), the one-barrier run equal to the two-phase run bit for bit"""
    from tests.test_gpu_user_model import CASES
    from tests.test_gpu_user_one_barrier import OB, _ladder, _run as run_user, _sampler as user_sampler
    n_chain, seed, n_rounds, n_swap = 4, 61, 6, 5
    t = dl.threads(waves)
    for n in (1, t - 1, t + 1, 3 * t + 1):
        data, box, st, lad = _ladder("simplesin2", n_chain, n_data=n)
        n_par = len(box["start"])
        what = "simplesin2 waves=%d n_data=%d" % (waves, n)
        rs = np.random.RandomState([waves, n])
        pts = box["pmin"] + (box["pmax"] - box["pmin"]) * rs.uniform(0.05, 0.95, (6, n_par))
        betas = rs.uniform(0.05, 1, len(pts))
        want = [orc.loglike(CASES["simplesin2"][1], p, data, beta=b) for p, b in zip(pts, betas)]
        rng = orc.Rng(orc.RNG_STREAMS, seed, lad)
        ref = orc.run_sampler(lad, rng, n_rounds, n_swap, record=True)
        runs = {}
        for flags in ((0, OB) if waves in dl.ONE_BARRIER_WAVES else (0,)):
            s = user_sampler("simplesin2", data, n_par, n_chain, st, waves, flags, seed)
            assert s.geometry == (waves, False) and bool(s.launch_policy[0]) == (flags == OB), what
            prob, prior = s.loglike(pts, betas)
            s.close()
            np.testing.assert_allclose(prob, [r[0] for r in want], rtol=1e-12, atol=1e-300, err_msg=what)
            np.testing.assert_allclose(prior, [r[1] for r in want], rtol=1e-12, atol=1e-300, err_msg=what)
            dev, rows, launch = runs[flags] = run_user("simplesin2", data, n_par, st, waves, flags, seed, n_rounds, n_swap,
                                                       pieces=(2, 4))
            assert bool(launch) == (flags == OB), what
            assert_match(dev, lad, rng, what=what)
            np.testing.assert_allclose(rows, ref, rtol=1e-9, atol=1e-300, err_msg=what + " rows")
        if OB in runs:
            _same_state(runs[OB][0], runs[0][0], what + ": one-barrier against two-phase", FIELDS + ("step",))
            assert np.array_equal(_bits(runs[OB][1]), _bits(runs[0][1])), what + ": rows differ"
