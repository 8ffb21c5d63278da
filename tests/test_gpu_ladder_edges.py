"""Ladders at the edges of the beta arithmetic, against the CPU oracle: the hottest chain at beta = 0
(-DBETA_0=0, src/parallel_tempering_beta.c:53-90), a chain whose beta is > 0 but whose 1/beta overflows, a
ladder of equal betas (hot_chains: every swap ratio a rounding residue) and a ladder of one chain.  There the
one-barrier threshold multiplies by 1/beta (pt_onebarrier.h, ObThreshold) and the swap ratio divides by beta
(pt_kernels.h; parallel_tempering_interaction.c:35): NaN and infinities are where a kernel can be wrong
without any calibrated-looking ladder noticing.  Every entry is compared with the oracle (counters and
ticks exact, fp64 to 1e-9), the one-barrier kernels bit for bit with the two-phase one, and the launch
policy with the kernel each case is named after."""
import numpy as np
import pytest

from apemost_amd import capi
from apemost_amd.sampler import HipSampler
from oracle import oracle as orc
from tests.helpers import assert_match, make_pair, small_workloads

pytestmark = pytest.mark.gpu

N_CHAIN, N_ROUNDS, N_SWAP, SEED = 8, 40, 11, 5
TINY = 1e-310   # > 0, and 1 / TINY overflows
MODELS = ["simplesin", "sine3", "pulse", "pulse_vrot"]
FIELDS = ("params", "params_best", "prob", "prob_best", "prior", "accept", "reject", "swapcount", "ticks", "n_iter",
          "params_accepts", "params_rejects")

# make_pair arguments of each ladder; chain 0 is the coldest (beta 1), chain N_CHAIN - 1 the hottest
LADDERS = {
    "beta0": dict(beta_0=0.0),                                    # (a) chebyshev, hottest chain at beta 0
    "beta0_tiny": dict(beta_0=0.0, betas={N_CHAIN - 2: TINY}),    # (b) ... and the next one at 1e-310
    "hot_chains": dict(beta_0=0.5, ladder_kind=orc.LADDER_HOT_CHAINS),   # (c) every beta 0.5
}

# name: (waves per chain, flags, APEMOST_OB_HELPER or None for the engine's choice)
PATHS = {
    "two_phase_w1": (1, 0, None),
    "two_phase_w2": (2, 0, None),
    "two_phase_w4": (4, capi.FLAG_TWO_BARRIER_STEP, None),
    "two_phase_w8": (8, capi.FLAG_TWO_BARRIER_STEP, None),
    "one_barrier_w4": (4, 0, None),
    "one_barrier_w8": (8, 0, None),
    "one_barrier_w4_no_helper": (4, 0, "0"),
    "one_barrier_w8_no_helper": (8, 0, "0"),
}
ONE_BARRIER = [p for p in PATHS if p.startswith("one_barrier")]


def _split_ok(beta):
    """the helper wavefront's threshold holds both halves scaled by 1/beta: it may only run where that is finite"""
    beta = np.asarray(beta, dtype=np.float64)
    with np.errstate(divide="ignore", over="ignore"):
        return bool(np.all((beta > 0) & np.isfinite(1.0 / beta)))


def _expected_policy(path, name, beta):
    """launch_policy[0] the sampler must report: 0 two-phase, 1 one-barrier, 2 one-barrier with a helper wavefront"""
    waves, flags, helper = PATHS[path]
    if waves < 4 or flags & capi.FLAG_TWO_BARRIER_STEP:
        return 0
    return 2 if helper is None and name in ("pulse", "pulse_vrot") and _split_ok(beta) else 1


def _policy(s):
    return (2 if s.ob_helper else 1) if s.launch_policy[0] else 0


def _sampler(w, n_chain, path, monkeypatch, **kw):
    waves, flags, helper = PATHS[path]
    if helper is None:
        monkeypatch.delenv("APEMOST_OB_HELPER", raising=False)
    else:
        monkeypatch.setenv("APEMOST_OB_HELPER", helper)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=SEED, waves_per_chain=waves, flags=flags, **kw)
    assert s.geometry[0] == waves
    return s


def _run(w, st, n_chain, path, monkeypatch, pieces):
    """run_sampler with swaps, cut into launches of `pieces` rounds; (state, sample rows, launch policy)"""
    import torch
    s = _sampler(w, n_chain, path, monkeypatch)
    s.set_state(st)
    policy = _policy(s)
    d = torch.zeros((sum(pieces) * N_SWAP, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
    done = 0
    for k in pieces:
        s.run_sampler(k, N_SWAP, d[done * N_SWAP:].data_ptr())
        done += k
    s.synchronize()
    out = s.get_state(), d.cpu().numpy(), policy
    s.close()
    return out


def _assert_rows(rows, ref, what):
    assert np.isfinite(rows)[np.isfinite(ref)].all(), what + ": rows not finite where the oracle's are"
    np.testing.assert_allclose(rows, ref, rtol=1e-9, atol=1e-300, err_msg=what + " rows")


def _check_run_sampler(w, name, path, n_chain, monkeypatch, what, **ladder):
    st, lad, rng = make_pair(w, n_chain, seed=SEED, **ladder)
    dev, rows, policy = _run(w, st, n_chain, path, monkeypatch, pieces=(13, N_ROUNDS - 13))
    ref = orc.run_sampler(lad, rng, N_ROUNDS, N_SWAP, record=True)
    if st.beta[-1] == 0:
        # independent of the oracle: the beta = 0 chain moves (accepts whenever prior_new - prior_old > ln U)
        assert dev.accept[-1] > 0, "%s: the beta = 0 chain is frozen (accept %s)" % (what, dev.accept)
    assert_match(dev, lad, rng, what=what)
    _assert_rows(rows, ref, what)
    if path in ONE_BARRIER:
        twin, twin_rows, _ = _run(w, st, n_chain, "two_phase_w%d" % PATHS[path][0], monkeypatch, pieces=(N_ROUNDS,))
        for f in FIELDS:
            assert np.array_equal(getattr(dev, f), getattr(twin, f)), "%s: %s differs from the two-phase kernel" % (what, f)
        assert np.array_equal(rows, twin_rows), what + ": rows differ from the two-phase kernel"
    assert policy == _expected_policy(path, name, st.beta), (what, policy)


@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("ladder", list(LADDERS))
def test_run_sampler_on_edge_ladder(ladder, name, path, monkeypatch):
    w = small_workloads()[name]
    _check_run_sampler(w, name, path, N_CHAIN, monkeypatch, "%s %s %s" % (ladder, name, path), **LADDERS[ladder])


@pytest.mark.parametrize("path", ONE_BARRIER)
@pytest.mark.parametrize("name", MODELS)
def test_single_chain_ladder_on_one_barrier_kernels(name, path, monkeypatch):
    """(d) one chain (beta 1, no swap partner) on the one-barrier kernels, helper on and off"""
    w = small_workloads()[name]
    _check_run_sampler(w, name, path, 1, monkeypatch, "one chain %s %s" % (name, path))


@pytest.mark.parametrize("waves", [1, 2, 4, 8])
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("ladder", ["beta0", "beta0_tiny"])
def test_launch_round_for_on_edge_ladder(ladder, name, waves):
    """markov_chain_step_for on every parameter in turn: the accept test of a single-parameter update at
    beta 0 and 1e-310"""
    import torch
    w = small_workloads()[name]
    st, lad, rng = make_pair(w, N_CHAIN, seed=SEED, init_prob=True, **LADDERS[ladder])
    s = HipSampler(w.model, w.n_par, N_CHAIN, w.data, seed=SEED, waves_per_chain=waves)
    s.set_state(st)
    what = "step_for %s %s waves=%d" % (ladder, name, waves)
    for p, n in [(p, 5 + p) for p in range(w.n_par)] + [(0, 20)]:
        d = torch.zeros((n, N_CHAIN, w.n_par + 2), dtype=torch.float64, device="cuda")
        s.markov_chain_step_for(p, n, d.data_ptr())
        s.synchronize()
        ref = np.zeros((n, N_CHAIN, w.n_par + 2))
        for k in range(n):
            for c in range(N_CHAIN):
                orc.step_for(lad, rng, c, p)
                orc.check_best(lad, c)
                lad.n_iter[c] += 1
                ref[k, c, :w.n_par] = lad.params[c]
                ref[k, c, w.n_par] = lad.prob[c]
                ref[k, c, w.n_par + 1] = lad.prob[c] - lad.prior[c]
        _assert_rows(d.cpu().numpy(), ref, "%s p=%d" % (what, p))
    dev = s.get_state()
    s.close()
    assert_match(dev, lad, rng, what=what)
    assert dev.params_accepts[-1].sum() > 0, what + ": the beta = 0 chain is frozen"


@pytest.mark.parametrize("path", ["one_barrier_w4", "one_barrier_w8", "one_barrier_w4_no_helper",
                                  "one_barrier_w8_no_helper"])
@pytest.mark.parametrize("name", ["pulse", "pulse_vrot"])
def test_calibration_with_a_beta_zero_chain(name, path, monkeypatch):
    """markov_chain_calibrate on ladder (a) in the one-barrier calibration kernel, helper on and off: the
    reference's calibration of a beta = 0 chain is well defined but need not converge -- its status is
    compared exactly either way"""
    w = small_workloads()[name]
    st, lad, rng = make_pair(w, N_CHAIN, seed=SEED, init_prob=True, **LADDERS["beta0"])
    s = _sampler(w, N_CHAIN, path, monkeypatch)
    s.set_state(st)
    policy = _policy(s)
    dcfg = capi.calib_defaults(burn_in_iterations=200, iter_limit=3000)
    ocfg = orc.calib_defaults(burn_in_iterations=200, iter_limit=3000)
    status, iters = s.markov_chain_calibrate(0, N_CHAIN, dcfg)
    dev = s.get_state()
    s.close()
    for c in range(N_CHAIN):
        st_o, it_o = orc.markov_chain_calibrate(lad, rng, c, ocfg)
        assert status[c] == st_o and iters[c] == it_o, (c, status[c], st_o, iters[c], it_o)
    assert_match(dev, lad, rng, what="calibrate beta0 %s %s" % (name, path))
    assert policy == _expected_policy(path, name, st.beta), policy


@pytest.mark.parametrize("path", ["two_phase_w1", "two_phase_w2", "one_barrier_w4", "one_barrier_w8",
                                  "one_barrier_w8_no_helper"])
@pytest.mark.parametrize("name", MODELS)
@pytest.mark.parametrize("ladder", ["beta0", "beta0_tiny"])
def test_burn_in_only_on_edge_ladder(ladder, name, path, monkeypatch):
    """burn_in_only (the -DSKIP_CALIBRATE_ALLCHAINS path of calibrate_rest) through the calibration kernels"""
    w = small_workloads()[name]
    n_iter = 300
    st, lad, rng = make_pair(w, N_CHAIN, seed=SEED, init_prob=True, **LADDERS[ladder])
    s = _sampler(w, N_CHAIN, path, monkeypatch)
    s.set_state(st)
    status, iters = s.markov_chain_calibrate(0, N_CHAIN, capi.calib_defaults(burn_in_iterations=n_iter),
                                             burn_in_only=True)
    dev = s.get_state()
    s.close()
    assert not status.any() and not iters.any()
    for c in range(N_CHAIN):
        orc.burn_in(lad, rng, c, n_iter)
    assert np.array_equal(dev.step, st.step)
    assert dev.accept[-1] > 0, "burn_in %s %s %s: the beta = 0 chain is frozen" % (ladder, name, path)
    assert_match(dev, lad, rng, what="burn_in %s %s %s" % (ladder, name, path))


class _Concat:
    """shard states side by side, field by field, as assert_match reads a whole ladder's"""

    def __init__(self, parts):
        self._parts = parts

    def __getattr__(self, f):
        return np.concatenate([getattr(p, f) for p in self._parts])


@pytest.mark.parametrize("name", MODELS)
def test_two_shards_with_the_beta_zero_chain_alone(name):
    """the two-shard edge exchange on ladder (a), cut at n - 1: the beta = 0 chain is a shard of its own and
    every swap it takes part in crosses the halo.  Against the oracle (the whole-ladder device run shares the
    kernels with the shards, so agreeing with it proves less)."""
    import torch
    from apemost_amd.distributed import HipShardEngine
    w = small_workloads()[name]
    n_rounds, n_swap, split = 80, 3, N_CHAIN - 1
    st, lad, rng = make_pair(w, N_CHAIN, seed=SEED, **LADDERS["beta0"])
    shards = []
    for lo, hi in ((0, split), (split, N_CHAIN)):
        s = HipSampler(w.model, w.n_par, hi - lo, w.data, seed=SEED, chain_offset=lo, n_chains_global=N_CHAIN)
        s.set_state(st.slice(lo, hi))
        if s.launch_policy[0]:
            assert s.ob_helper == (name in ("pulse", "pulse_vrot") and _split_ok(st.beta[lo:hi])), (lo, hi)
        shards.append(HipShardEngine(s, torch))
    exchanges, pending, rnd = 0, False, 0
    for r in range(n_rounds + 1):
        n_steps = n_swap if r < n_rounds else 0
        if pending:
            a = shards[0].swap_pair(rnd)
            assert a == shards[1].swap_pair(rnd)
            if a == split - 1:
                up, down = shards[0].edge_export(1), shards[1].edge_export(0)
                for e in shards:
                    e.s.synchronize()
                shards[0].edge_import(1, down)
                shards[1].edge_import(0, up)
                exchanges += 1
            rnd += 1
        for e in shards:
            e.launch_rounds(1, n_steps, pending, None)
        pending = n_steps > 0
    got = [e.s.get_state() for e in shards]
    for e in shards:
        e.s.close()
    assert exchanges > 0
    orc.run_sampler(lad, rng, n_rounds, n_swap)
    assert got[1].accept[0] > 0, "the beta = 0 chain is frozen"
    assert_match(_Concat(got), lad, rng, what="two shards beta0 %s" % name)
