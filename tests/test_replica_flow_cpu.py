"""Replica-flow tracking (APEMOST_HIP_FLAG_TRACK_REPLICAS), the parts that need no GPU: the flag, the struct and the
three entry points; the create-time refusal of a sharded ladder; the five rules through tests/replica_flow_ref.replay;
ReplicaFlow's figures, its dump file and suggest_betas; and the oracle run whose replay the GPU tests compare with."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi, workloads as wl
from apemost_amd.replica_flow import ReplicaFlow, initial
from tests import hostlib
from tests import replica_flow_ref as rfr
from tests.helpers import make_pair, small_workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("apemost_hip_replica_flow_get", "apemost_hip_replica_flow_set", "apemost_hip_replica_flow_reset")
# the ladder of the GPU tests: 5 chains down to beta 0.2, 400 rounds x 2 steps, seed 23
N_CHAIN, BETA_0, SEED, N_ROUNDS, N_SWAP = 5, 0.2, 23, 400, 2
SCHEDULES = ("default", "randomswap", "even_odd")
# (-DRANDOMSWAP reads other uniforms: under seed 23 its pulse ladder makes no round trip in 400 rounds, under 5 it does)
SCHEDULE_SEED = {"default": SEED, "even_odd": SEED, "randomswap": 5}


def oracle_run(name, schedule, n_chain=N_CHAIN, n_rounds=N_ROUNDS, n_swap=N_SWAP, seed=None, record=False, setup=None,
               init_prob=False):
    """(device state to start from, oracle ladder after the run, rng, ReplicaFlow of the replay, attempts, rows)"""
    w = small_workloads()[name]
    seed = SCHEDULE_SEED[schedule] if seed is None else seed
    st, lad, rng = make_pair(w, n_chain, beta_0=BETA_0, seed=seed, init_prob=init_prob)
    lad.randomswap = int(schedule == "randomswap")
    if setup:
        setup(lad)
    rf, attempts, rows = rfr.oracle_flow(lad, rng, n_rounds, n_swap, even_odd=schedule == "even_odd", record=record,
                                         n_threads=8)
    return st, lad, rng, rf, attempts, rows


def check_flow_is_not_trivial(rf, attempts, schedule=None):
    """what the issue asks of the oracle's own replay, so that no comparison passes on an all-zero flow"""
    n = len(rf)
    assert rf.round_trips.sum() >= 1, rf.round_trips
    assert all(any(sw for _, a, sw in attempts if a == pair) for pair in range(n - 1)), "a pair never swapped"
    assert rf.attempts.sum() == len(attempts) and rf.attempts[n - 1] == 0


def test_header_declares_library_exports_and_capi_binds():
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    build.build_hip()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", build.HIP_LIB]).decode()
    L = capi.lib()
    m = re.search(r"APEMOST_HIP_FLAG_TRACK_REPLICAS\s*=\s*(\d+)", header)
    assert m and int(m.group(1)) == capi.FLAG_TRACK_REPLICAS == 4096
    assert "#define APEMOST_HIP_ABI_VERSION 3" in header and capi.ABI_VERSION == 3 and L.apemost_hip_abi_version() == 3
    assert re.search(r"uint32_t \*replica, \*heading;\s*uint64_t \*n_up, \*n_down, \*attempts, \*round_trips;\s*"
                     r"\} apemost_hip_replica_flow_view;", header)
    assert [f for f, _ in capi.ReplicaFlowView._fields_] == ["replica", "heading", "n_up", "n_down", "attempts", "round_trips"]
    assert C.sizeof(capi.ReplicaFlowView) == 6 * C.sizeof(C.c_void_p)
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert re.search(r" T %s$" % name, nm, re.M), name
        assert name in capi.EXPORTS and getattr(L, name).argtypes, name
    declared = set(re.findall(r"^(?:int|int32_t|int64_t|void|const char \*) ?\*?(apemost_hip_\w+)\(", header, re.M))
    assert declared and all(re.search(r" T %s$" % d, nm, re.M) for d in declared), declared
    doc = header[header.index("Replica-flow tracking"):header.index("APEMOST_HIP_FLAG_TRACK_REPLICAS = 4096")]
    for phrase in ("round_trips[its label] += 1", "the label follows params", "attempts[a] += 1", "heading[0] = 1",
                   "before any device is touched"):
        assert phrase in doc, phrase
    for name in ("DESIGN.md", "README.md"):
        assert "TRACK_REPLICAS" in open(os.path.join(ROOT, name)).read(), name


def _create(**kw):
    build.build_hip()
    base = dict(abi_version=capi.ABI_VERSION, device=0, model=wl.MODEL_SIMPLESIN, n_par=4, n_chains=4, n_data=16, n_cols=2,
                flags=capi.FLAG_TRACK_REPLICAS, chain_offset=0, n_chains_global=4, seed=1, sigma=0.5, hmin=1e-6)
    base.update(kw)
    L, h = capi.lib(), C.c_void_p()
    rc = L.apemost_hip_create(C.byref(capi.Config(**base)), C.byref(h))
    msg = L.apemost_hip_last_error().decode()
    if rc == capi.OK:
        L.apemost_hip_destroy(h)
    else:
        assert not h.value
    return rc, msg


@pytest.mark.parametrize("kw", [dict(chain_offset=1, n_chains_global=5), dict(n_chains_global=8),
                                dict(chain_offset=4, n_chains_global=8, flags=capi.FLAG_TRACK_REPLICAS | capi.FLAG_SWAP_EVEN_ODD)])
def test_a_sharded_ladder_is_refused_before_any_device_is_touched(kw):
    """ERR_UNSUPPORTED and the engine's message, on a machine with or without a GPU"""
    rc, msg = _create(**kw)
    assert rc == capi.ERR_UNSUPPORTED and "TRACK_REPLICAS" in msg and "sharded" in msg, (rc, msg)
    rc, msg = _create(flags=0, **{k: v for k, v in kw.items() if k != "flags"})
    assert rc != capi.ERR_UNSUPPORTED, msg               # without the flag the same shard is no such refusal


def test_the_entry_points_refuse_a_null_sampler():
    build.build_hip()
    L = capi.lib()
    v = capi.ReplicaFlowView()
    assert L.apemost_hip_replica_flow_get(None, C.byref(v)) == capi.ERR_INVALID
    assert L.apemost_hip_replica_flow_set(None, C.byref(v)) == capi.ERR_INVALID
    assert L.apemost_hip_replica_flow_reset(None) == capi.ERR_INVALID


def _walk_up_and_back(n):
    """replica 0 carried from rung 0 to rung n-1 and back by accepted swaps"""
    up = [(r, a, True) for r, a in enumerate(range(n - 1))]
    down = [(n - 1 + r, a, True) for r, a in enumerate(range(n - 2, -1, -1))]
    return up + down


@pytest.mark.parametrize("n", [2, 3, 5])
def test_a_replica_walked_up_and_back_makes_exactly_one_round_trip(n):
    rf = rfr.replay(n, _walk_up_and_back(n))
    assert rf.replica[0] == 0 and rf.heading[0] == 1
    # replica 0 went up with heading 1, took heading 2 at the top and closed its trip when it came back to rung 0.
    # Nobody else did: the replica that started at the top only stepped down one rung and back -- except with two
    # rungs, where that one rung is rung 0 and the two replicas trade places twice
    assert rf.round_trips[0] == 1, rf.round_trips
    assert rf.round_trips.sum() == (2 if n == 2 else 1), rf.round_trips
    assert rf.attempts.sum() == 2 * (n - 1) and sorted(rf.replica) == list(range(n))


@pytest.mark.parametrize("n", [3, 5])
def test_a_replica_that_turns_round_below_the_top_makes_none(n):
    # replica 0 up to rung n-2 and back; rejected attempts at the top pair keep the ends' headings alive
    up = [(r, a, True) for r, a in enumerate(range(n - 2))]
    down = [(100 + r, a, True) for r, a in enumerate(range(n - 3, -1, -1))]
    rf = rfr.replay(n, up + [(50, n - 2, False)] + down)
    assert rf.replica[0] == 0 and rf.round_trips[0] == 0 and rf.heading[0] == 1
    assert rf.round_trips.sum() == 0, rf.round_trips


def test_hand_written_lists_rule_by_rule():
    # n = 2: a rejected attempt moves the counters only
    rf = rfr.replay(2, [(0, 0, False)])
    assert list(rf.replica) == [0, 1] and list(rf.heading) == [1, 2]
    assert list(rf.n_up) == [1, 0] and list(rf.n_down) == [0, 1] and list(rf.attempts) == [1, 0] and rf.round_trips.sum() == 0
    # an accepted one brings replica 1 (heading 2) to rung 0: one round trip of replica 1
    rf = rfr.replay(2, [(0, 0, True)])
    assert list(rf.replica) == [1, 0] and list(rf.heading) == [1, 2] and list(rf.round_trips) == [0, 1]
    # n = 3, the middle rung has no heading until a replica with one arrives
    rf = rfr.replay(3, [(0, 1, False)])
    assert list(rf.heading) == [1, 0, 2] and list(rf.n_up) == [0, 0, 0] and list(rf.n_down) == [0, 0, 1]
    rf = rfr.replay(3, [(0, 0, True), (1, 0, False)])
    assert list(rf.replica) == [1, 0, 2] and list(rf.heading) == [1, 1, 2] and list(rf.n_up) == [2, 2, 0]
    assert list(rf.attempts) == [2, 0, 0] and rf.round_trips.sum() == 0
    # n = 1: nothing to attempt
    rf = rfr.replay(1, [])
    assert list(rf.replica) == [0] and list(rf.heading) == [0]
    # replay goes on from a flow it is given
    both = rfr.replay(3, [(0, 0, True), (1, 0, False)])
    assert rfr.replay(3, [(1, 0, False)], start=rfr.replay(3, [(0, 0, True)])) == both


@pytest.mark.parametrize("n", [2, 3, 5, 8])
def test_random_attempt_lists(n):
    rs = np.random.RandomState(n)
    attempts = [(r, int(rs.randint(n - 1)), bool(rs.rand() < 0.6)) for r in range(3000)]
    rf = rfr.replay(n, attempts)
    assert sorted(rf.replica) == list(range(n))
    up = rf.up_fraction
    assert up[0] == 1 and up[n - 1] == 0
    assert rf.attempts.sum() == len(attempts) and rf.attempts[n - 1] == 0
    assert np.all(rf.n_up + rf.n_down <= rf.attempts + np.concatenate([[0], rf.attempts[:-1]]))
    assert rf.round_trips.sum() > 0 and set(rf.heading) <= {0, 1, 2}


def _flow(rejections, attempts=1000):
    n = len(rejections) + 1
    replica, heading = initial(n)
    att = np.array([attempts] * (n - 1) + [0], dtype=np.uint64)
    swaps = np.array([round(attempts * (1 - r)) for r in rejections] + [0], dtype=np.uint64)
    z = np.zeros(n, dtype=np.uint64)
    return ReplicaFlow(replica, heading, z, z, att, z, swapcount=swaps)


def test_suggest_betas():
    betas = np.array([1.0, 0.7, 0.45, 0.3, 0.2, 0.05])
    out = _flow([0.4] * 5).suggest_betas(betas)
    np.testing.assert_allclose(out, betas, rtol=1e-12)        # equal rejections: the ladder stays
    assert out[0].tobytes() == betas[0].tobytes() and out[-1].tobytes() == betas[-1].tobytes()
    rej = [0.1, 0.1, 0.9, 0.1, 0.1]
    f = _flow(rej)
    out = f.suggest_betas(betas)
    assert out[0].tobytes() == betas[0].tobytes() and out[-1].tobytes() == betas[-1].tobytes()
    assert np.all(np.diff(out) < 0)
    # the betas move towards the pair (2, 3) that rejects: more of them lie inside [0.3, 0.45]
    assert out[2] < betas[2] and out[3] > betas[3]
    assert ((out <= betas[2]) & (out >= betas[3])).sum() > 2
    assert abs(f.barrier - sum(rej)) < 1e-12 and np.isnan(f.swap_rate[-1])
    np.testing.assert_allclose(f.rejection[:-1], rej, atol=1e-12)
    # another size, the ends still kept; pairs without attempts take the others' mean; zero rejections stay monotone
    out9 = f.suggest_betas(betas, n=9)
    assert len(out9) == 9 and out9[0] == betas[0] and out9[-1] == betas[-1] and np.all(np.diff(out9) < 0)
    g = _flow([0.4, 0.4, 0.4, 0.4, 0.4])
    g.attempts[2] = 0
    g.swapcount[2] = 0
    np.testing.assert_allclose(g.suggest_betas(betas), betas, rtol=1e-12)
    assert np.all(np.diff(_flow([0.0, 0.0, 0.5, 0.0, 0.0]).suggest_betas(betas)) < 0)
    # a pure function: the flow and the betas are left alone
    before = betas.copy()
    f.suggest_betas(betas)
    assert np.array_equal(betas, before) and f == _flow(rej)
    assert f.round_trip_rate(100) == 0.0 and np.all(np.isnan(f.up_fraction))


def test_write_and_read_round_trip(tmp_path):
    rs = np.random.RandomState(3)
    rf = rfr.replay(6, [(r, int(rs.randint(5)), bool(rs.rand() < 0.5)) for r in range(500)])
    rf.beta = np.array([1.0, 0.73, 1 / 3.0, 0.2, 0.1 + 0.2, 1e-3])
    rf.swapcount = np.array([50, 40, 30, 20, 10, 0], dtype=np.uint64)
    path = str(tmp_path / "replica_flow.dump")
    rf.write(path)
    back = ReplicaFlow.read(path)
    assert back == rf and back.beta.tobytes() == rf.beta.tobytes()
    lines = open(path).read().splitlines()
    assert len(lines) == 12 and len(lines[0].split("\t")) == 7 and len(lines[6].split()) == 1


def test_c_host_builds_with_the_macro_under_the_strict_flags(tmp_path):
    build.build_hip()
    assert os.path.exists(hostlib.make(str(tmp_path / "rf.exe"), ccflags="-DN_BETA=4 -DTRACK_REPLICAS"))
    assert os.path.exists(hostlib.make(str(tmp_path / "rf2.exe"), ccflags="-DN_BETA=4 -DTRACK_REPLICAS -DSWAP_EVEN_ODD -DADAPT"))


@pytest.mark.parametrize("name", ["simplesin", "pulse"])
@pytest.mark.parametrize("schedule", SCHEDULES)
def test_the_oracle_run_of_the_gpu_tests_really_flows(name, schedule):
    """the oracle's own replay of the ladder the GPU tests use shows at least one round trip and accepted swaps on
    every pair: a condition on the fixture, which the reference primitives alone must meet"""
    _, lad, rng, rf, attempts, _ = oracle_run(name, schedule)
    print(name, schedule, "round trips", rf.round_trips, "swapcount", lad.swapcount, "up", rf.up_fraction)
    check_flow_is_not_trivial(rf, attempts)
    assert rng.round == N_ROUNDS and sorted(rf.replica) == list(range(N_CHAIN))
    assert np.array_equal(rf.swapcount, lad.swapcount)
    assert [int(x) for x in rf.swapcount[:-1]] == [sum(1 for _, a, sw in attempts if a == p and sw) for p in range(N_CHAIN - 1)]
    assert rf.up_fraction[0] == 1 and rf.up_fraction[-1] == 0
    if schedule == "even_odd":
        assert len(attempts) == N_ROUNDS // 2 * 2 + N_ROUNDS // 2 * 2      # 5 chains: two pairs in every sweep
    else:
        assert len(attempts) == N_ROUNDS
