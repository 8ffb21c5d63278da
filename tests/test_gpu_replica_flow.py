"""Replica-flow tracking (APEMOST_HIP_FLAG_TRACK_REPLICAS, include/apemost_hip.h) on the device, through the C ABI,
against the replay of the oracle's own swap attempts (tests/replica_flow_ref.py).  Flow arrays are compared with ==.
The ladder is the one tests/test_replica_flow_cpu.py shows to make round trips and to swap on every pair.  None of
these tests runs anything into the hand-off timeout."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from apemost_amd.replica_flow import FIELDS, ReplicaFlow
from apemost_amd.sampler import HipSampler
from apemost_amd.state import LadderState
from oracle import oracle as orc
from tests import hostlib
from tests import replica_flow_ref as rfr
from tests.helpers import assert_match, make_pair, small_workloads, to_oracle
from tests.test_replica_flow_cpu import (BETA_0, N_CHAIN, N_ROUNDS, N_SWAP, SCHEDULE_SEED, SEED, check_flow_is_not_trivial,
                                         oracle_run)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TR = capi.FLAG_TRACK_REPLICAS
SCHEDULE_FLAG = {"default": 0, "randomswap": capi.FLAG_RANDOMSWAP, "even_odd": capi.FLAG_SWAP_EVEN_ODD}
STATE_FIELDS = ("params", "params_best", "step", "prob", "prior", "prob_best", "accept", "reject", "swapcount", "ticks",
                "n_iter", "params_accepts", "params_rejects")


def same_flow(a, b):
    return all(np.array_equal(getattr(a, k), getattr(b, k)) for k, _ in FIELDS)


def assert_flow(dev, ref, what=""):
    for k, _ in FIELDS:
        assert np.array_equal(getattr(dev, k), getattr(ref, k)), "%s %s: device %s, replay %s" % (what, k, getattr(dev, k), getattr(ref, k))


def _run(w, st, n_chain, n_rounds, n_swap, waves, seed, flags, parts=None, rows=True, **kw):
    """run_sampler on a whole ladder (in `parts` calls): (state, rows, flow or None, launch_policy, ob_helper)"""
    import torch
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=seed, waves_per_chain=waves, flags=flags, **kw)
    s.set_state(st)
    d = torch.zeros((n_rounds * n_swap, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda") if rows else None
    done = 0
    for k in parts or [n_rounds]:
        s.run_sampler(k, n_swap, d[done * n_swap:].data_ptr() if rows else 0)
        done += k
    s.synchronize()
    assert s.round == (n_rounds, False)
    flow = s.replica_flow() if flags & TR else None
    out = s.get_state(), (d.cpu().numpy() if rows else None), flow, s.launch_policy, s.ob_helper
    if flow is not None:                 # the device's attempts are the schedule's own count
        for a in range(n_chain):
            assert int(flow.attempts[a]) == s.swap_attempts(a, 0, n_rounds), a
    s.close()
    return out


def check_against_replay(name, schedule, waves, flags=0, expect_helper=None, setup=None, parts=None, **kw):
    w = small_workloads()[name]
    st, lad, rng, ref, attempts, ref_rows = oracle_run(name, schedule, record=True, setup=setup)
    check_flow_is_not_trivial(ref, attempts)
    dev, rows, flow, policy, helper = _run(w, st, N_CHAIN, N_ROUNDS, N_SWAP, waves, SCHEDULE_SEED[schedule],
                                           TR | SCHEDULE_FLAG[schedule] | flags, parts=parts, **kw)
    what = "%s %s waves=%d flags=%d" % (name, schedule, waves, flags)
    print(what, "round trips", flow.round_trips, "replica", flow.replica, "policy", policy, "helper", helper)
    assert_match(dev, lad, rng, what=what)
    np.testing.assert_allclose(rows, ref_rows, rtol=1e-9, atol=1e-300)
    assert_flow(flow, ref, what)
    assert np.array_equal(flow.swapcount, ref.swapcount) and np.array_equal(flow.beta, ref.beta)
    if expect_helper is not None:
        assert helper == expect_helper
    if not flags & (capi.FLAG_ADAPT | capi.FLAG_RWM):
        assert policy[2] == (1 if flags & capi.FLAG_SINGLE_ROUND_LAUNCHES else 1024)
        assert policy[0] == (waves in (4, 8) and not flags & capi.FLAG_TWO_BARRIER_STEP)
    return dev, rows, flow


@pytest.mark.parametrize("schedule", ["default", "randomswap", "even_odd"])
@pytest.mark.parametrize("name,waves,flags", [
    ("simplesin", 1, 0), ("simplesin", 2, 0), ("simplesin", 4, 0), ("simplesin", 4, capi.FLAG_TWO_BARRIER_STEP),
    ("simplesin", 8, 0), ("pulse", 1, 0), ("pulse", 2, 0), ("pulse", 4, 0), ("pulse", 4, capi.FLAG_TWO_BARRIER_STEP)])
def test_device_flow_equals_the_replay_of_the_oracles_attempts(name, schedule, waves, flags):
    """5 chains x 400 rounds x 2 steps: the two-phase kernels (1, 2 waves; 4 forced back to them), the one-barrier
    kernels (4, 8; pulse with its helper wavefront), all swaps inside the launches"""
    check_against_replay(name, schedule, waves, flags, expect_helper=True if (name, waves, flags) == ("pulse", 4, 0) else None)


def test_pulse_without_the_helper_wavefront_in_a_fresh_process():
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_replica_flow import check_against_replay\n"
            "for schedule in ('default', 'even_odd'):\n"
            "    check_against_replay('pulse', schedule, 4, expect_helper=False)\nprint('CHILD OK')\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, APEMOST_OB_HELPER="0"), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b"CHILD OK" in out.stdout, out.stdout.decode(errors="replace")[-3000:]


@pytest.mark.parametrize("schedule", ["default", "even_odd"])
def test_adapt_together_with_the_flag(schedule):
    """-DADAPT makes every round a launch of its own: the launch-start attempt only"""
    def setup(lad):
        lad.adapt, lad.adapt_target = 1, 0.5
    check_against_replay("simplesin", schedule, 4, capi.FLAG_ADAPT, setup=setup, adapt_target=0.5)


@pytest.mark.parametrize("schedule", ["default", "randomswap", "even_odd"])
@pytest.mark.parametrize("name,waves", [("simplesin", 4), ("pulse", 4), ("simplesin", 1)])
def test_launch_forms_and_boundaries_give_identical_flow_and_the_flag_leaves_the_chain_alone(name, schedule, waves):
    """multi-round launches, SINGLE_ROUND_LAUNCHES, the two-phase kernels and shifted launch boundaries: the same flow;
    and with the flag every sample row and every state field is bit for bit what the sampler gives without it"""
    w = small_workloads()[name]
    SEED = SCHEDULE_SEED[schedule]
    st, _, _ = make_pair(w, N_CHAIN, beta_0=BETA_0, seed=SEED)
    base = SCHEDULE_FLAG[schedule]
    ref, rows, flow, policy, _ = _run(w, st, N_CHAIN, N_ROUNDS, N_SWAP, waves, SEED, TR | base)
    assert policy[2] == 1024 and flow.round_trips.sum() >= 1
    for flags, parts in ((capi.FLAG_SINGLE_ROUND_LAUNCHES, None), (0, [7, 393]), (0, [1, 2, 397]),
                         (capi.FLAG_TWO_BARRIER_STEP, [150, 250]),
                         (capi.FLAG_TWO_BARRIER_STEP | capi.FLAG_SINGLE_ROUND_LAUNCHES, [7, 393])):
        other, rows2, flow2, policy2, _ = _run(w, st, N_CHAIN, N_ROUNDS, N_SWAP, waves, SEED, TR | base | flags, parts=parts)
        assert policy2[2] == (1 if flags & capi.FLAG_SINGLE_ROUND_LAUNCHES else 1024)
        assert_flow(flow2, flow, "%s flags=%d parts=%s" % (schedule, flags, parts))
        for f in STATE_FIELDS:
            assert np.array_equal(getattr(other, f), getattr(ref, f)), (flags, parts, f)
        assert np.array_equal(rows2, rows), (flags, parts)
    for flags in (0, capi.FLAG_SINGLE_ROUND_LAUNCHES):
        plain, rows0, none, _, _ = _run(w, st, N_CHAIN, N_ROUNDS, N_SWAP, waves, SEED, base | flags)
        assert none is None
        for f in STATE_FIELDS:
            assert getattr(plain, f).tobytes() == getattr(ref, f).tobytes(), f
        assert rows0.tobytes() == rows.tobytes()


@pytest.mark.parametrize("schedule", ["default", "even_odd"])
@pytest.mark.parametrize("waves", [1, 4])
def test_a_batch_of_three_ladders_equals_three_tracked_samplers(schedule, waves):
    import torch
    w = small_workloads()["simplesin"]
    seeds = [SEED, 11, 5]
    base = TR | SCHEDULE_FLAG[schedule]
    alone = []
    for seed in seeds:
        st, _, _ = make_pair(w, N_CHAIN, beta_0=BETA_0, seed=seed)
        alone.append(_run(w, st, N_CHAIN, N_ROUNDS, N_SWAP, waves, seed, base, rows=False))
    st, _, _ = make_pair(w, N_CHAIN, beta_0=BETA_0, seed=SEED)
    big = LadderState(3 * N_CHAIN, w.n_par)
    for f in STATE_FIELDS + ("beta", "pmin", "pmax"):
        getattr(big, f)[...] = np.concatenate([getattr(st, f)] * 3)
    s = HipSampler.batch(w.model, w.n_par, N_CHAIN, w.data, seeds, waves_per_chain=waves, flags=base)
    s.set_state(big)
    s.run_sampler(N_ROUNDS, N_SWAP, 0)
    s.synchronize()
    flows, state = s.replica_flow(), s.get_state()
    assert len(flows) == 3 and s.replica_flow(ladder=1) == flows[1]
    for b in range(3):
        assert_flow(flows[b], alone[b][2], "ladder %d" % b)
        assert np.array_equal(flows[b].swapcount, alone[b][0].swapcount)
        assert np.array_equal(s.ladder_view(state.params, b), alone[b][0].params)
        for a in range(N_CHAIN):
            assert int(flows[b].attempts[a]) == s.swap_attempts(a, 0, N_ROUNDS, ladder=b)
    assert sum(int(f.round_trips.sum()) for f in flows) >= 1
    assert not same_flow(flows[0], flows[1])
    # set and reset go per ladder too
    s.replica_flow_reset()
    assert all(f.attempts.sum() == 0 and list(f.replica) == list(range(N_CHAIN)) for f in s.replica_flow())
    s.replica_flow_set(flows)
    assert all(same_flow(x, y) for x, y in zip(s.replica_flow(), flows))
    s.close()


def test_a_user_supplied_model_equals_the_replay():
    """hiprtc compiles the variant instantiations of a user's likelihood: the tracking comes with them"""
    rs = np.random.RandomState(4)
    x = 100 + 0.5 * np.arange(300)
    data = np.stack([x, 0.8 * np.sin(2 * np.pi * (0.21 * x + 0.3312)) + rs.normal(0, 0.5, 300)], 1)
    start, pmin, pmax = np.array([0.9, 0.2]), np.array([0.0, 0.0]), np.array([2.0, 0.3])
    n_chain, seed, n_rounds = 4, 31, 300
    src = os.path.join(hostlib.HOST, "examples", "device_models", "simplesin2.hip")
    for schedule in ("default", "even_odd"):
        st = LadderState.from_params(n_chain, start, pmin, pmax, (pmax - pmin) * 0.03)
        for i in range(n_chain):
            st.beta[i] = orc.get_chain_beta(orc.LADDER_CHEBYSHEV_BETA, i, n_chain, 0.3)
            st.step[i] = np.minimum(st.step[i] * st.beta[i] ** -0.5, pmax - pmin)
        lad = orc.Ladder(orc.MODEL_SINE2, n_chain, 2, data)
        to_oracle(st, lad)
        for c in range(n_chain):
            orc.calc_model(lad, c)
        st.prob[:], st.prior[:] = lad.prob, lad.prior
        rng = orc.Rng(orc.RNG_STREAMS, seed, lad)
        ref, attempts, _ = rfr.oracle_flow(lad, rng, n_rounds, 3, even_odd=schedule == "even_odd")
        assert ref.attempts.sum() == len(attempts) and any(sw for _, _, sw in attempts)
        for waves in (2, 4):
            s = HipSampler(wl.MODEL_USER, 2, n_chain, data, seed=seed, waves_per_chain=waves, flags=TR | SCHEDULE_FLAG[schedule],
                           device_model_source=src)
            s.set_state(st)
            s.run_sampler(n_rounds, 3, 0)
            s.synchronize()
            dev, flow = s.get_state(), s.replica_flow()
            s.close()
            assert np.array_equal(dev.swapcount, lad.swapcount) and np.array_equal(dev.accept, lad.accept)
            assert_flow(flow, ref, "user model %s waves=%d" % (schedule, waves))


@pytest.mark.parametrize("schedule", ["default", "even_odd"])
def test_a_resumed_run_and_a_reset(schedule):
    """get -> new sampler -> set_state + replica_flow_set + set_round -> continue equals the uninterrupted run; a reset
    after some rounds equals a run started there"""
    w = small_workloads()["simplesin"]
    flags = TR | SCHEDULE_FLAG[schedule]
    st, _, _ = make_pair(w, N_CHAIN, beta_0=BETA_0, seed=SEED)
    whole, _, flow, _, _ = _run(w, st, N_CHAIN, N_ROUNDS, N_SWAP, 4, SEED, flags, rows=False)
    a = HipSampler(w.model, w.n_par, N_CHAIN, w.data, seed=SEED, waves_per_chain=4, flags=flags)
    a.set_state(st)
    a.run_sampler(151, N_SWAP, 0)
    a.synchronize()
    mid, mid_flow = a.get_state(), a.replica_flow()
    assert mid_flow.attempts.sum() > 0 and not same_flow(mid_flow, flow)
    a.close()
    b = HipSampler(w.model, w.n_par, N_CHAIN, w.data, seed=SEED, waves_per_chain=4, flags=flags)
    b.set_state(mid)
    b.replica_flow_set(mid_flow)
    b.set_round(151, False)
    assert same_flow(b.replica_flow(), mid_flow)
    b.run_sampler(N_ROUNDS - 151, N_SWAP, 0)
    b.synchronize()
    end, end_flow = b.get_state(), b.replica_flow()
    for f in STATE_FIELDS:
        assert np.array_equal(getattr(end, f), getattr(whole, f)), f
    assert_flow(end_flow, flow, "resumed")
    # reset: the rest of the run counted from the initial flow, which is what the replay of those attempts gives
    c = HipSampler(w.model, w.n_par, N_CHAIN, w.data, seed=SEED, waves_per_chain=4, flags=flags)
    c.set_state(mid)
    c.replica_flow_set(mid_flow)
    c.set_round(151, False)
    c.replica_flow_reset()
    fresh = c.replica_flow()
    assert list(fresh.replica) == list(range(N_CHAIN)) and list(fresh.heading) == [1, 0, 0, 0, 2]
    assert fresh.attempts.sum() == fresh.n_up.sum() == fresh.n_down.sum() == fresh.round_trips.sum() == 0
    c.run_sampler(N_ROUNDS - 151, N_SWAP, 0)
    c.synchronize()
    after_reset = c.replica_flow()
    _, _, _, _, attempts, _ = oracle_run("simplesin", schedule)
    first_late = 151
    late = [t for t in attempts if t[0] >= first_late]
    assert_flow(after_reset, rfr.replay(N_CHAIN, late), "reset")
    for x in (b, c):
        x.close()


def _view(n, **arrays):
    keep = {k: np.ascontiguousarray(v, dtype=t) for k, t in FIELDS for kk, v in arrays.items() if kk == k}
    v = capi.ReplicaFlowView(**{k: a.ctypes.data_as(C.POINTER(C.c_uint32 if a.dtype == np.uint32 else C.c_uint64))
                                for k, a in keep.items()})
    return v, keep


def test_every_refusal():
    import torch
    w = small_workloads()["simplesin"]
    L = capi.lib()
    plain = HipSampler(w.model, w.n_par, 4, w.data)
    v, keep = _view(4, replica=[0, 1, 2, 3])
    for call in (lambda: L.apemost_hip_replica_flow_get(plain._h, C.byref(v)),
                 lambda: L.apemost_hip_replica_flow_set(plain._h, C.byref(v)),
                 lambda: L.apemost_hip_replica_flow_reset(plain._h)):
        assert call() == capi.ERR_UNSUPPORTED and b"TRACK_REPLICAS" in L.apemost_hip_last_error()
    with pytest.raises(capi.ApemostHipError) as e:
        plain.replica_flow()
    assert e.value.code == capi.ERR_UNSUPPORTED
    plain.close()
    with pytest.raises(capi.ApemostHipError, match="sharded") as e:
        HipSampler(w.model, w.n_par, 4, w.data, flags=TR, chain_offset=2, n_chains_global=8)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(capi.ApemostHipError, match="1, 2, 4 or 8 waves"):
        HipSampler(w.model, w.n_par, 4, w.data, flags=TR, waves_per_chain=6)
    s = HipSampler(w.model, w.n_par, 4, w.data, flags=TR)
    for bad in ([0, 1, 1, 3], [0, 1, 2, 4]):
        v, keep = _view(4, replica=bad)
        assert L.apemost_hip_replica_flow_set(s._h, C.byref(v)) == capi.ERR_INVALID
        assert b"permutation" in L.apemost_hip_last_error()
    v, keep = _view(4, heading=[1, 0, 3, 2])
    assert L.apemost_hip_replica_flow_set(s._h, C.byref(v)) == capi.ERR_INVALID
    assert L.apemost_hip_replica_flow_get(s._h, None) == capi.ERR_INVALID
    assert list(s.replica_flow().replica) == [0, 1, 2, 3]                   # a refused set changed nothing
    buf = torch.zeros(capi.lib().apemost_hip_edge_doubles(w.n_par), dtype=torch.float64, device="cuda")
    handles = (C.c_void_p * 1)(s._h)
    for rc in (L.apemost_hip_run_shards(handles, 1, 1, 1, None), L.apemost_hip_edge_export(s._h, 1, buf.data_ptr()),
               L.apemost_hip_edge_import(s._h, 0, buf.data_ptr()), L.apemost_hip_set_chain_offset(s._h, 0)):
        assert rc == capi.ERR_UNSUPPORTED
    other = HipSampler(w.model, w.n_par, 4, w.data, flags=TR)
    assert L.apemost_hip_edge_exchange(s._h, other._h) == capi.ERR_UNSUPPORTED
    other.close()
    from apemost_amd.distributed import HipShardEngine, ShardedLadder
    with pytest.raises(ValueError, match="replica flow"):
        ShardedLadder(HipShardEngine(s, torch), 4, 0, 4, 0, 1)
    s.close()


def _rt(a):
    return np.array([float("%.15e" % v) for v in np.ravel(a)]).reshape(np.shape(a))


@pytest.mark.parametrize("extra,flag", [("", 0), (" -DSWAP_EVEN_ODD", capi.FLAG_SWAP_EVEN_ODD)])
def test_c_application_built_with_the_macro_writes_the_python_mirrors_dump(tmp_path, extra, flag):
    """-DTRACK_REPLICAS on the application's compile line: the run phase leaves replica_flow.dump, equal to what the
    Python mirror of the same run writes; with APEMOST_DEVICES (a sharded ladder) the engine refuses"""
    n_beta, burn, iters, n_swap = 5, 600, 2000, 2
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"), ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=%d -DMAX_ITERATIONS=%d -DN_SWAP=%d "
                                                           "-DBETA_0=0.2 -DTRACK_REPLICAS%s" % (n_beta, burn, iters, n_swap, extra))
    work = tmp_path / "run"
    work.mkdir()
    (work / "params").write_text(w.params_file_text())
    (work / "data").write_text(w.data_file_text())
    env = dict(os.environ, APEMOST_SEED="12")
    for phase in ("calibrate_first", "calibrate_rest", "run"):
        subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=600)
    got = ReplicaFlow.read(str(work / "replica_flow.dump"))
    data = np.loadtxt(str(work / "data"))
    st = LadderState.from_params(n_beta, _rt(w.start), _rt(w.pmin), _rt(w.pmax), _rt(w.step))
    st.read_calibration_results((work / "calibration_results").read_text())
    s = HipSampler(w.model, 4, n_beta, data, seed=12, flags=TR | flag)
    s.set_state(st)
    s.run_sampler(iters // n_swap, n_swap, 0)
    s.synchronize()
    mine = s.replica_flow()
    s.close()
    mine.write(str(tmp_path / "mirror.dump"))
    assert (work / "replica_flow.dump").read_text() == (tmp_path / "mirror.dump").read_text()
    assert got == ReplicaFlow.read(str(tmp_path / "mirror.dump")) and got.attempts.sum() >= iters // n_swap
    assert got.swapcount.sum() > 0 and np.array_equal(got.beta, st.beta)
    out = subprocess.run([exe, "run"], cwd=str(work), env=dict(env, APEMOST_DEVICES="0,0"), stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode != 0 and b"TRACK_REPLICAS" in out.stdout and b"sharded" in out.stdout, out.stdout[-2000:]
