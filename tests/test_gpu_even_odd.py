"""Even-odd swap sweeps (APEMOST_HIP_FLAG_SWAP_EVEN_ODD, include/apemost_hip.h): every neighbour pair of the round's
parity attempts a swap each round.  Everything through the C ABI, against the CPU restatement of the schedule built
from the oracle's primitives (tests/even_odd_ref.py): integer state bit-exact, rows and final state to rel 1e-9
(DESIGN 7).  None of these tests runs anything into the hand-off timeout on purpose."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler
from apemost_amd.state import LadderState
from oracle import oracle as orc
from tests import even_odd_ref as eo
from tests import hostlib
from tests.helpers import assert_match, make_pair, small_workloads, to_oracle
from tests.test_even_odd_cpu import N_ROUNDS, N_SWAP, SEED, TWO_CHAINS, check_schedule_really_swaps

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EO = capi.FLAG_SWAP_EVEN_ODD


def _run(w, st, n_chain, n_rounds, n_swap, waves, seed, flags=EO, parts=None, **kw):
    """run_sampler on a whole ladder (in `parts` calls); (state, rows, launch_policy, ob_helper)"""
    import torch
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=seed, waves_per_chain=waves, flags=flags, **kw)
    s.set_state(st)
    d = torch.zeros((n_rounds * n_swap, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
    done = 0
    for k in parts or [n_rounds]:
        s.run_sampler(k, n_swap, d[done * n_swap:].data_ptr())
        done += k
    assert done == n_rounds
    s.synchronize()
    assert s.round == (n_rounds, False)
    out = s.get_state(), d.cpu().numpy(), s.launch_policy, s.ob_helper
    for a in range(n_chain - 1):       # swapcount / swap_attempts is the per-pair swap rate
        if flags & EO:
            assert s.swap_attempts(a, 0, n_rounds) == sum(1 for r in range(n_rounds) if r % 2 == a % 2)
        assert out[0].swapcount[a] <= s.swap_attempts(a, 0, n_rounds)
    assert s.swap_attempts(n_chain - 1, 0, n_rounds) == 0 and s.swap_attempts(0, 0, 0) == 0
    s.close()
    return out


def _default_total(w, n_chain, n_rounds, n_swap, seed):
    st0, lad0, rng0 = make_pair(w, n_chain, seed=seed)
    orc.run_sampler(lad0, rng0, n_rounds, n_swap, n_threads=8)
    return int(lad0.swapcount.sum())


def check_against_restatement(name, waves, flags=0, n_chain=8, n_rounds=N_ROUNDS, seed=SEED, expect_helper=None):
    w = small_workloads()[name]
    st, lad, rng = make_pair(w, n_chain, seed=seed)
    dev, rows, policy, helper = _run(w, st, n_chain, n_rounds, N_SWAP, waves, seed, flags=flags | EO)
    ref = eo.run_sampler(lad, rng, n_rounds, N_SWAP, record=True, n_threads=8)
    what = "even-odd %s waves=%d flags=%d chains=%d" % (name, waves, flags, n_chain)
    print(what, "swapcount", dev.swapcount, "policy", policy, "helper", helper)
    assert_match(dev, lad, rng, what=what)
    np.testing.assert_allclose(rows, ref, rtol=1e-9, atol=1e-300)
    if expect_helper is not None:
        assert helper == expect_helper
    # whole ladders keep their multi-round launches
    assert policy[2] == (1 if flags & capi.FLAG_SINGLE_ROUND_LAUNCHES else 1024)
    assert policy[0] == (waves in (4, 8) and not flags & capi.FLAG_TWO_BARRIER_STEP)
    return dev, rows


@pytest.mark.parametrize("name,waves,flags", [
    ("simplesin", 1, 0), ("simplesin", 2, 0), ("simplesin", 4, 0), ("simplesin", 8, 0),
    ("simplesin", 4, capi.FLAG_SINGLE_ROUND_LAUNCHES), ("simplesin", 8, capi.FLAG_TWO_BARRIER_STEP),
    ("simplesin", 1, capi.FLAG_SINGLE_ROUND_LAUNCHES), ("pulse", 4, 0), ("pulse_vrot", 1, 0), ("sine3", 2, 0)])
def test_run_sampler_matches_the_restatement(name, waves, flags):
    """8 chains x 120 rounds x 3 steps: the two-phase kernels (1, 2 waves; 8 forced back to them), the one-barrier
    kernels (4, 8; pulse with its helper wavefront), in-launch sweeps and sweeps fused into the next launch's start.
    And the schedule is really different and really swaps: at least 1.5 times the default schedule's swaps on the
    same ladder, no pair above its attempts, at most one pair that never swapped."""
    dev, _ = check_against_restatement(name, waves, flags, expect_helper=True if (name, waves) == ("pulse", 4) else None)
    w = small_workloads()[name]
    check_schedule_really_swaps(dev.swapcount[:7].astype(np.int64), _default_total(w, 8, N_ROUNDS, N_SWAP, SEED), N_ROUNDS)
    assert dev.swapcount[7] == 0


def test_pulse_without_the_helper_wavefront_in_a_fresh_process():
    """APEMOST_OB_HELPER=0 is read when the sampler is created: a child process with it set runs the same check on
    the one-barrier kernel without the helper wavefront"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_even_odd import check_against_restatement\n"
            "check_against_restatement('pulse', 4, expect_helper=False)\nprint('CHILD OK')\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, APEMOST_OB_HELPER="0"), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b"CHILD OK" in out.stdout, out.stdout.decode(errors="replace")[-3000:]


@pytest.mark.parametrize("n_chain,waves,seed", [(7, 4, SEED), (7, 1, SEED), (2, 1, TWO_CHAINS["seed"]), (2, 8, TWO_CHAINS["seed"])])
def test_chains_that_sit_a_sweep_out(n_chain, waves, seed):
    """an odd ladder (the top chain sits the even sweeps out, chain 0 the odd ones) and two chains (one pair, even
    sweeps only; seed 11, for which the CPU restatement swaps 30 times in 120 rounds)"""
    n_rounds = TWO_CHAINS["n_rounds"] if n_chain == 2 else N_ROUNDS
    dev, _ = check_against_restatement("simplesin", waves, n_chain=n_chain, n_rounds=n_rounds, seed=seed)
    if n_chain == 2:
        assert 1 <= dev.swapcount[0] <= n_rounds // 2
    else:
        w = small_workloads()["simplesin"]
        check_schedule_really_swaps(dev.swapcount[:n_chain - 1].astype(np.int64),
                                    _default_total(w, n_chain, n_rounds, N_SWAP, seed), n_rounds)


@pytest.mark.parametrize("name,waves", [("simplesin", 4), ("simplesin", 8), ("pulse", 4), ("pulse_vrot", 8)])
def test_kernels_and_launch_forms_agree_bit_for_bit(name, waves):
    """one-barrier against two-phase, multi-round launches against single-round ones, and launch boundaries:
    120 rounds in one call and as 7 + 113"""
    w = small_workloads()[name]
    st, _, _ = make_pair(w, 8, seed=SEED)
    ob, rows, policy, _ = _run(w, st, 8, N_ROUNDS, N_SWAP, waves, SEED)
    assert policy[0] and policy[2] > 1
    for flags, parts in ((capi.FLAG_TWO_BARRIER_STEP, None), (capi.FLAG_SINGLE_ROUND_LAUNCHES, None), (0, [7, 113]),
                         (capi.FLAG_TWO_BARRIER_STEP | capi.FLAG_SINGLE_ROUND_LAUNCHES, [7, 113])):
        other, rows2, policy2, _ = _run(w, st, 8, N_ROUNDS, N_SWAP, waves, SEED, flags=EO | flags, parts=parts)
        assert policy2[0] == (not flags & capi.FLAG_TWO_BARRIER_STEP)
        assert policy2[2] == (1 if flags & capi.FLAG_SINGLE_ROUND_LAUNCHES else 1024)
        for f in ("params", "params_best", "prob", "prior", "prob_best", "accept", "reject", "swapcount", "ticks", "n_iter",
                  "params_accepts", "params_rejects"):
            assert np.array_equal(getattr(other, f), getattr(ob, f)), (flags, parts, f)
        assert np.array_equal(rows2, rows), (flags, parts)


def test_set_round_and_get_round_carry_the_schedule_over():
    """7 rounds on one sampler, its state and swap position loaded into a fresh one, 113 more: the same chain as
    120 rounds in one call; an odd starting sweep attempts the odd pairs first"""
    import torch
    w = small_workloads()["simplesin"]
    st, lad, rng = make_pair(w, 8, seed=SEED)
    whole, rows, _, _ = _run(w, st, 8, N_ROUNDS, N_SWAP, 4, SEED)
    a = HipSampler(w.model, w.n_par, 8, w.data, seed=SEED, waves_per_chain=4, flags=EO)
    a.set_state(st)
    d = torch.zeros((N_ROUNDS * N_SWAP, 8, w.n_par + 2), dtype=torch.float64, device="cuda")
    a.run_sampler(7, N_SWAP, d.data_ptr())
    a.synchronize()
    assert a.round == (7, False)
    mid = a.get_state()
    a.close()
    b = HipSampler(w.model, w.n_par, 8, w.data, seed=SEED, waves_per_chain=4, flags=EO)
    b.set_state(mid)
    b.set_round(7, False)
    assert b.round == (7, False) and b.swap_pair(7) == 1 and b.swap_pair(8) == 0
    assert b.swap_attempts(0, 7, 113) == 56 and b.swap_attempts(1, 7, 113) == 57
    b.run_sampler(113, N_SWAP, d[7 * N_SWAP:].data_ptr())
    b.synchronize()
    assert b.round == (120, False)
    end = b.get_state()
    b.close()
    for f in ("params", "params_best", "prob", "prob_best", "accept", "reject", "swapcount", "ticks", "n_iter"):
        assert np.array_equal(getattr(end, f), getattr(whole, f)), f
    assert np.array_equal(d.cpu().numpy(), rows)
    ref = eo.run_sampler(lad, rng, N_ROUNDS, N_SWAP, record=True)
    assert_match(end, lad, rng, what="set_round")
    np.testing.assert_allclose(rows, ref, rtol=1e-9, atol=1e-300)


def test_a_proposal_law_together_with_the_flag():
    w = small_workloads()["simplesin"]
    st, lad, rng = make_pair(w, 8, seed=SEED)
    lad.proposal = orc.PROPOSAL_LOGISTIC
    dev, rows, _, _ = _run(w, st, 8, N_ROUNDS, N_SWAP, 4, SEED, flags=EO | capi.FLAG_PROPOSAL_LOGISTIC)
    ref = eo.run_sampler(lad, rng, N_ROUNDS, N_SWAP, record=True)
    assert_match(dev, lad, rng, what="even-odd + logistic")
    np.testing.assert_allclose(rows, ref, rtol=1e-9, atol=1e-300)
    assert dev.swapcount.sum() > 0


def test_adapt_together_with_the_flag():
    """-DADAPT makes every round a launch of its own: the launch-start sweep only.  The restatement follows
    orc_run_sampler's order: the round's steps, adapt(), then the sweep; past ADAPT's 20000 counted updates"""
    w = small_workloads()["simplesin"]
    n_rounds, n_swap, seed = 420, 70, 41
    st, lad, rng = make_pair(w, 8, seed=seed)
    lad.adapt, lad.adapt_target = 1, 0.5
    step0 = st.step.copy()
    import torch
    s = HipSampler(w.model, w.n_par, 8, w.data, seed=seed, waves_per_chain=4, flags=EO | capi.FLAG_ADAPT, adapt_target=0.5)
    assert s.launch_policy[2] == 1
    s.set_state(st)
    d = torch.zeros((n_rounds * n_swap, 8, w.n_par + 2), dtype=torch.float64, device="cuda")
    s.run_sampler(n_rounds, n_swap, d.data_ptr())
    s.synchronize()
    dev = s.get_state()
    s.close()
    ref = eo.run_sampler(lad, rng, n_rounds, n_swap, record=True, n_threads=8)
    assert_match(dev, lad, rng, what="even-odd + adapt")
    np.testing.assert_allclose(d.cpu().numpy(), ref, rtol=1e-9, atol=1e-300)
    assert not np.allclose(dev.step, step0) and dev.swapcount.sum() > 0


def test_config4_shape_one_step_per_round_matches_the_restatement():
    """the flagship shard as the engine launches it (pulse, 256 chains x 1024 points, n_swap 1, the helper form): every
    step is a round, every chain hands off at every step, alternately with its upper and its lower neighbour, 96
    rounds in one launch"""
    n_chain, n_rounds, seed = 256, 96, 404
    w = wl.pulse(n_data=1024, n_chain=n_chain)
    st, lad, rng = make_pair(w, n_chain, seed=seed, init_prob=True)
    dev, rows, policy, helper = _run(w, st, n_chain, n_rounds, 1, 0, seed)
    assert policy[0] and policy[2] >= n_rounds and helper
    ref = eo.run_sampler(lad, rng, n_rounds, 1, record=True, n_threads=8)
    assert_match(dev, lad, rng, what="config 4 shape")
    np.testing.assert_allclose(rows, ref, rtol=1e-9, atol=1e-300)
    assert dev.swapcount.sum() > n_rounds


@pytest.mark.parametrize("bounds", [[(0, 2), (2, 9)], [(0, 5), (5, 9)], [(0, 2), (2, 6), (6, 9)], [(0, 3), (3, 5), (5, 9)]])
@pytest.mark.parametrize("waves", [1, 4])
def test_run_shards_equals_the_whole_ladder(bounds, waves):
    """apemost_hip_run_shards with 2 and 3 shards on device 0 of a 9-chain ladder -- edges of both parities; the
    interior shards (2, 6) and (3, 5) get both of their edges in one sweep (pairs 1 and 5, pairs 2 and 4) --
    bit-identical to the whole ladder at the same waves_per_chain, which matches the restatement;
    rounds_within_shard and swap_pair as specified.  (The edges are put where the restatement swaps: pair 3 of this
    ladder never does.)"""
    import torch
    w = small_workloads()["simplesin"]
    n_global = 9
    st, lad, rng = make_pair(w, n_global, seed=SEED)
    ref, d_whole, _, _ = _run(w, st, n_global, N_ROUNDS, N_SWAP, waves, SEED)
    shards = []
    for lo, hi in bounds:
        s = HipSampler(w.model, w.n_par, hi - lo, w.data, seed=SEED, chain_offset=lo, n_chains_global=n_global,
                       waves_per_chain=waves, flags=EO)
        s.set_state(st.slice(lo, hi))
        shards.append(s)
        for first in range(4):
            # the edge between chains o-1 and o is straddled by the sweeps of the parity of o-1
            want = 0
            while want < 5 and not ((lo > 0 and (lo - 1) % 2 == (first + want) % 2) or
                                    (hi < n_global and (hi - 1) % 2 == (first + want) % 2)):
                want += 1
            assert s.rounds_within_shard(first, 5) == want <= 2, (lo, hi, first)
        assert [s.swap_pair(r) for r in range(4)] == [0, 1, 0, 1]
    n = len(bounds)
    bufs = [torch.zeros((N_ROUNDS * N_SWAP, hi - lo, w.n_par + 2), dtype=torch.float64, device="cuda") for lo, hi in bounds]
    torch.cuda.synchronize()
    handles = (C.c_void_p * n)(*[s._h for s in shards])
    L = capi.lib()
    for off, part in ((0, 7), (7, 113)):                  # two calls: the swap position carries over
        ptrs = (C.c_void_p * n)(*[b[off * N_SWAP:].data_ptr() for b in bufs])
        capi.check(L.apemost_hip_run_shards(handles, n, part, N_SWAP, ptrs))
    for s in shards:
        s.synchronize()
    got = [s.get_state() for s in shards]
    for f in ("params", "params_best", "prob", "prob_best", "prior", "accept", "reject", "swapcount", "ticks", "n_iter"):
        assert np.array_equal(np.concatenate([getattr(g, f) for g in got]), getattr(ref, f)), f
    assert np.array_equal(torch.cat(bufs, dim=1).cpu().numpy(), d_whole)
    for lo, hi in bounds[:-1]:
        assert ref.swapcount[hi - 1] > 0                   # every shard edge was crossed
    orc_rows = eo.run_sampler(lad, rng, N_ROUNDS, N_SWAP, record=True)
    assert_match(ref, lad, rng, what="run_shards")
    np.testing.assert_allclose(d_whole, orc_rows, rtol=1e-9, atol=1e-300)
    check_schedule_really_swaps(ref.swapcount[:8].astype(np.int64), _default_total(w, 9, N_ROUNDS, N_SWAP, SEED), N_ROUNDS)
    # a shard of the other schedule does not continue this ladder
    lo, hi = bounds[-1]
    odd = HipSampler(w.model, w.n_par, hi - lo, w.data, seed=SEED, chain_offset=lo, n_chains_global=n_global, waves_per_chain=waves)
    odd.set_round(*shards[0].round)
    mixed = (C.c_void_p * n)(*([s._h for s in shards[:-1]] + [odd._h]))
    assert L.apemost_hip_run_shards(mixed, n, 1, 1, None) == capi.ERR_INVALID
    odd.close()
    for s in shards:
        s.close()


def test_a_user_supplied_model_runs_the_schedule():
    """hiprtc compiles the variant instantiations of a user's likelihood: the schedule comes with them"""
    import torch
    rs = np.random.RandomState(4)
    x = 100 + 0.5 * np.arange(300)
    data = np.stack([x, 0.8 * np.sin(2 * np.pi * (0.21 * x + 0.3312)) + rs.normal(0, 0.5, 300)], 1)
    start, pmin, pmax = np.array([0.9, 0.2]), np.array([0.0, 0.0]), np.array([2.0, 0.3])
    n_chain, seed = 6, 31
    st = LadderState.from_params(n_chain, start, pmin, pmax, (pmax - pmin) * 0.03)
    for i in range(n_chain):
        st.beta[i] = orc.get_chain_beta(orc.LADDER_CHEBYSHEV_BETA, i, n_chain, 0.05)
        st.step[i] = np.minimum(st.step[i] * st.beta[i] ** -0.5, pmax - pmin)
    lad = orc.Ladder(orc.MODEL_SINE2, n_chain, 2, data)
    to_oracle(st, lad)
    for c in range(n_chain):
        orc.calc_model(lad, c)
    st.prob[:], st.prior[:] = lad.prob, lad.prior
    rng = orc.Rng(orc.RNG_STREAMS, seed, lad)
    src = os.path.join(hostlib.HOST, "examples", "device_models", "simplesin2.hip")
    for waves in (2, 4):
        s = HipSampler(wl.MODEL_USER, 2, n_chain, data, seed=seed, waves_per_chain=waves, flags=EO, device_model_source=src)
        s.set_state(st)
        d = torch.zeros((60 * 3, n_chain, 4), dtype=torch.float64, device="cuda")
        s.run_sampler(60, 3, d.data_ptr())
        s.synchronize()
        dev = s.get_state()
        s.close()
        if waves == 2:
            ref = eo.run_sampler(lad, rng, 60, 3, record=True)
            first = dev, d.cpu().numpy()
            assert_match(dev, lad, rng, what="user model even-odd")
            np.testing.assert_allclose(first[1], ref, rtol=1e-9, atol=1e-300)
            assert dev.swapcount.sum() > 0
        else:
            assert np.array_equal(dev.swapcount, first[0].swapcount) and np.array_equal(dev.accept, first[0].accept)
            np.testing.assert_allclose(d.cpu().numpy(), first[1], rtol=1e-9, atol=1e-300)


def test_create_time_refusals_and_the_distributed_driver():
    w = small_workloads()["simplesin"]
    for other in (capi.FLAG_RANDOMSWAP, capi.FLAG_TEST_WITHHOLD_PUBLISH):
        with pytest.raises(capi.ApemostHipError, match="SWAP_EVEN_ODD excludes") as e:
            HipSampler(w.model, w.n_par, 4, w.data, flags=EO | other)
        assert e.value.code == capi.ERR_INVALID
    with pytest.raises(capi.ApemostHipError, match="1, 2, 4 or 8 waves"):
        HipSampler(w.model, w.n_par, 4, w.data, flags=EO, waves_per_chain=6)
    import torch
    from apemost_amd.distributed import HipShardEngine, ShardedLadder
    s = HipSampler(w.model, w.n_par, 4, w.data, flags=EO)
    with pytest.raises(ValueError, match="even-odd"):
        ShardedLadder(HipShardEngine(s, torch), 4, 0, 4, 0, 1)
    s.close()
    s = HipSampler(w.model, w.n_par, 4, w.data)
    ShardedLadder(HipShardEngine(s, torch), 4, 0, 4, 0, 1)          # the default schedule is driven as before
    assert s.swap_pair(0) == capi.swap_pair(0, 0, 4)
    s.close()


@pytest.mark.parametrize("name,waves", [("simplesin", 4), ("pulse", 8), ("simplesin", 1)])
def test_calibration_is_the_same_with_and_without_the_flag(name, waves):
    """the calibration has no swaps: status, sweep counts and state bit-identical"""
    w = small_workloads()[name]
    n_chain, seed = 4, 17
    cfg = capi.calib_defaults(burn_in_iterations=300, iter_limit=100000)
    out = []
    for flags in (0, EO):
        st, _, _ = make_pair(w, n_chain, seed=seed, init_prob=True)
        s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=seed, waves_per_chain=waves, flags=flags)
        s.set_state(st)
        status, iters = s.markov_chain_calibrate(0, n_chain, cfg)
        out.append((status, iters, s.get_state()))
        s.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][1].min() >= 200
    for f in ("params", "params_best", "step", "prob", "prior", "prob_best", "accept", "reject", "n_iter", "ticks",
              "params_accepts", "params_rejects", "swapcount"):
        assert np.array_equal(getattr(out[0][2], f), getattr(out[1][2], f)), f


def _rt(a):
    return np.array([float("%.15e" % v) for v in np.ravel(a)]).reshape(np.shape(a))


def test_c_application_built_with_the_macro_equals_python_mirror_also_in_two_shards(tmp_path):
    """-DSWAP_EVEN_ODD on the application's compile line: the run phase writes byte-identical dumps for APEMOST_DEVICES
    unset and 0,0 (apemost_hip_run_shards), and its prob-chain<i>.dump files are the Python mirror's rows in the
    reference's format"""
    import torch
    n_beta, burn, iters, n_swap = 9, 600, 2000, 5     # (acceptance_rate.dump gets a line every 1000 iterations)
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"), ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=%d -DMAX_ITERATIONS=%d -DN_SWAP=%d "
                                                           "-DSWAP_EVEN_ODD" % (n_beta, burn, iters, n_swap))
    outs = {}
    for name, devices in (("one", None), ("two", "0,0")):
        work = tmp_path / name
        work.mkdir()
        (work / "params").write_text(w.params_file_text())
        (work / "data").write_text(w.data_file_text())
        env = dict(os.environ, APEMOST_SEED="12")
        if devices:
            env["APEMOST_DEVICES"] = devices
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL)
        outs[name] = work
    files = ["calibration_results", "acceptance_rate.dump", "amplitude-chain-0.prob.dump", "phase-chain-0.prob.dump"] + \
            ["prob-chain%d.dump" % i for i in range(n_beta)]
    for f in files:
        assert (outs["two"] / f).read_bytes() == (outs["one"] / f).read_bytes(), f
    data = np.loadtxt(str(outs["one"] / "data"))
    st = LadderState.from_params(n_beta, _rt(w.start), _rt(w.pmin), _rt(w.pmax), _rt(w.step))
    st.read_calibration_results((outs["one"] / "calibration_results").read_text())
    s = HipSampler(w.model, 4, n_beta, data, seed=12, flags=EO)
    s.set_state(st)
    d = torch.zeros((iters, n_beta, 6), dtype=torch.float64, device="cuda")
    s.run_sampler(iters // n_swap, n_swap, d.data_ptr())
    s.synchronize()
    run = s.get_state()
    s.close()
    rows = d.cpu().numpy()
    for i in range(n_beta):
        want = "".join("%6e\t%6e\n" % (r[4], r[5]) for r in rows[:, i])
        assert (outs["one"] / ("prob-chain%d.dump" % i)).read_text() == want, i
    assert np.array_equal(np.loadtxt(str(outs["one"] / "amplitude-chain-0.prob.dump")), _rt(rows[:, 0, 0]))
    accept = (outs["one"] / "acceptance_rate.dump").read_text().strip().splitlines()[-1].split()
    assert [int(t) for t in accept] == [iters] + [int(a) for a in run.accept]
    assert run.swapcount[:8].sum() > 0 and all(run.swapcount[a] <= (iters // n_swap + 1 - a % 2) // 2 for a in range(8))
    # and the default build of the same application samples something else
    exe0 = hostlib.make(str(tmp_path / "sine0.exe"), ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=%d -DMAX_ITERATIONS=%d -DN_SWAP=%d"
                                                             % (n_beta, burn, iters, n_swap))
    work = tmp_path / "default"
    work.mkdir()
    for f in ("params", "data", "calibration_results"):
        (work / f).write_bytes((outs["one"] / f).read_bytes())
    subprocess.check_call([exe0, "run"], cwd=str(work), env=dict(os.environ, APEMOST_SEED="12"), stdout=subprocess.DEVNULL)
    assert (work / "prob-chain1.dump").read_bytes() != (outs["one"] / "prob-chain1.dump").read_bytes()
