"""Ladder batches (apemost_hip_create_batch, include/apemost_hip.h): n_ladders independent ladders in one
sampler and one launch.  Everything through the C ABI.  The identity the tests rest on: RNG streams are addressed by
(seed, chain, slot, tick) and not by the launch shape, so ladder b of a batch is BIT FOR BIT the chain a stand-alone
sampler with seed seeds[b], ladder b's data and the same waves_per_chain produces -- `==` on the raw bits of every
sample row and every field of the final state.  Against the CPU oracle the repository's parity rule holds (DESIGN 7:
integer state exact, rows and final state rel 1e-9).  None of these tests runs anything into a time-out on purpose."""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler
from apemost_amd.state import ALL_FIELDS, LadderState
from oracle import oracle as orc
from tests.helpers import assert_match, make_pair

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EO, SRL, TWO = capi.FLAG_SWAP_EVEN_ODD, capi.FLAG_SINGLE_ROUND_LAUNCHES, capi.FLAG_TWO_BARRIER_STEP
N_DATA = {"simplesin": 256, "sine3": 300, "pulse": 257, "pulse_vrot": 200}
PER, N_ROUNDS, N_SWAP = 8, 120, 3


def bits(a):
    """the raw bits: NaN payloads and signed zeros count"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def ladders(name, n_ladders, per=PER, init_prob=False, n_data=None):
    """n_ladders different problems of one shape: own data (the workload's generator under another seed), own
    seed, own betas and step widths; (workloads, seeds, states, oracle ladders, oracle rngs)"""
    ws, seeds, sts, lads, rngs = [], [], [], [], []
    for b in range(n_ladders):
        w = wl.by_name(name, n_data=n_data or N_DATA[name], n_chain=per, seed=500 + 7 * b)
        seed = 1000 + 13 * b
        st, lad, rng = make_pair(w, per, beta_0=0.02 + 0.01 * b, seed=seed, init_prob=init_prob)
        ws.append(w), seeds.append(seed), sts.append(st), lads.append(lad), rngs.append(rng)
    return ws, seeds, sts, lads, rngs


def concat(sts):
    out = LadderState(sum(s.n_chain for s in sts), sts[0].n_par)
    for f in ALL_FIELDS:
        getattr(out, f)[...] = np.concatenate([getattr(s, f) for s in sts])
    return out


def run(s, n_chains, n_par, n_rounds, n_swap, parts=None):
    import torch
    d = torch.zeros((n_rounds * n_swap, n_chains, n_par + 2), dtype=torch.float64, device="cuda")
    done = 0
    for k in parts or [n_rounds]:
        s.run_sampler(k, n_swap, d[done * n_swap:].data_ptr())
        done += k
    assert done == n_rounds
    s.synchronize()
    assert s.round == (n_rounds, False)
    return s.get_state(), d.cpu().numpy()


def make_batch(ws, seeds, waves, flags=0, per=PER, **kw):
    w = ws[0]
    return HipSampler.batch(w.model, w.n_par, per, np.stack([x.data for x in ws]), seeds, waves_per_chain=waves,
                            flags=flags, **kw)


def check_batch_equals_standalone(name, waves, flags=0, n_ladders=3, parts_batch=None, parts_alone=None,
                                  expect_helper=None, **kw):
    ws, seeds, sts, _, _ = ladders(name, n_ladders)
    w = ws[0]
    batch = make_batch(ws, seeds, waves, flags, **kw)
    assert batch.n_ladders == n_ladders and batch.n_chains == n_ladders * PER
    n = C.c_int32(0)
    capi.check(batch.L.apemost_hip_n_ladders(batch._h, C.byref(n)))
    assert n.value == n_ladders
    assert batch.geometry[0] == waves
    policy, helper = batch.launch_policy, batch.ob_helper
    assert policy[0] == (waves in (4, 8) and not flags & TWO) and policy[2] == (1 if flags & SRL else 1024)
    if expect_helper is not None:
        assert helper == expect_helper
    batch.set_state(concat(sts))
    got, rows = run(batch, n_ladders * PER, w.n_par, N_ROUNDS, N_SWAP, parts_batch)
    batch.close()
    swaps = 0
    for b in range(n_ladders):
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=waves, flags=flags, **kw)
        assert alone.ob_helper == helper and alone.launch_policy[0] == policy[0]
        alone.set_state(sts[b])
        want, want_rows = run(alone, PER, w.n_par, N_ROUNDS, N_SWAP, parts_alone)
        alone.close()
        for f in ALL_FIELDS:
            assert np.array_equal(bits(batch.ladder_view(getattr(got, f), b)), bits(getattr(want, f))), (name, waves, flags, b, f)
        assert np.array_equal(bits(batch.ladder_view(rows, b)), bits(want_rows)), (name, waves, flags, b)
        assert want.swapcount[PER - 1] == 0
        swaps += int(want.swapcount.sum())
    assert swaps > 0 and len({bits(batch.ladder_view(rows, b)).tobytes() for b in range(n_ladders)}) == n_ladders
    return got, rows


@pytest.mark.parametrize("name,waves,flags,n_ladders", [
    ("simplesin", 1, 0, 3), ("simplesin", 2, 0, 16), ("sine3", 1, 0, 3), ("sine3", 2, 0, 3),        # two-phase
    ("simplesin", 4, 0, 1), ("simplesin", 4, 0, 3), ("simplesin", 4, 0, 16), ("simplesin", 8, 0, 3),   # one-barrier
    ("pulse", 8, 0, 3), ("simplesin", 4, SRL, 3), ("pulse", 8, SRL, 3), ("simplesin", 1, SRL, 3),
    ("simplesin", 8, TWO, 3), ("pulse_vrot", 1, 0, 3), ("pulse_vrot", 4, 0, 3), ("sine3", 4, 0, 3),
    ("simplesin", 4, EO, 3), ("simplesin", 1, EO, 16), ("pulse", 8, EO | SRL, 3),
    ("simplesin", 4, capi.FLAG_PROPOSAL_LOGISTIC, 3), ("simplesin", 2, capi.FLAG_PROPOSAL_UNIFORM, 3),
    ("simplesin", 4, EO | capi.FLAG_PROPOSAL_UNIFORM, 3)])
def test_a_batch_equals_standalone_samplers_bit_for_bit(name, waves, flags, n_ladders):
    """8 chains per ladder x 120 rounds x 3 steps, distinct seeds, data, betas and step widths per ladder; the
    two-phase kernels, the one-barrier kernels with the in-launch hand-off and with single-round launches, the
    even-odd schedule, both proposal laws; 1, 3 and 16 ladders"""
    check_batch_equals_standalone(name, waves, flags, n_ladders)


def test_pulse_with_the_helper_wavefront():
    check_batch_equals_standalone("pulse", 4, expect_helper=True)
    check_batch_equals_standalone("pulse", 4, EO, n_ladders=16, expect_helper=True)


def test_pulse_without_the_helper_wavefront_in_a_fresh_process():
    """APEMOST_OB_HELPER=0 is read when a sampler is created: a child process with it set"""
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from tests.test_gpu_ladder_batch import check_batch_equals_standalone\n"
            "check_batch_equals_standalone('pulse', 4, expect_helper=False)\nprint('CHILD OK')\n" % ROOT)
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, APEMOST_OB_HELPER="0"), cwd=ROOT,
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert out.returncode == 0 and b"CHILD OK" in out.stdout, out.stdout.decode(errors="replace")[-3000:]


@pytest.mark.parametrize("waves,flags", [(4, 0), (1, 0), (4, EO)])
def test_launch_boundaries_placed_differently_on_the_two_sides(waves, flags):
    check_batch_equals_standalone("simplesin", waves, flags, parts_batch=[7, 113], parts_alone=[50, 1, 69])


@pytest.mark.parametrize("waves", [1, 4])
def test_circular_parameters(waves):
    """the phase wraps around its box instead of being redrawn (bit 2)"""
    check_batch_equals_standalone("simplesin", waves, circular_params=1 << 2)


@pytest.mark.parametrize("name", ["simplesin", "pulse"])
def test_against_the_oracle(name):
    """4 x 8 chains with the engine's own geometry (32 chains: four likelihood waves in the one-barrier kernels): each
    ladder against orc.run_sampler seeded with that ladder's seed; integer state exact, rows and state rel 1e-9"""
    n_ladders = 4
    ws, seeds, sts, lads, rngs = ladders(name, n_ladders, n_data=1024)
    batch = make_batch(ws, seeds, 0)
    assert batch.geometry[0] == 4 and batch.launch_policy[0]        # what a ladder of 32 chains x 1024 points gets
    batch.set_state(concat(sts))
    got, rows = run(batch, n_ladders * PER, ws[0].n_par, N_ROUNDS, N_SWAP)
    for b in range(n_ladders):
        ref = orc.run_sampler(lads[b], rngs[b], N_ROUNDS, N_SWAP, record=True, n_threads=8)
        assert_match(got.slice(b * PER, (b + 1) * PER), lads[b], rngs[b], what="batch %s ladder %d" % (name, b))
        np.testing.assert_allclose(batch.ladder_view(rows, b), ref, rtol=1e-9, atol=1e-300)
        assert lads[b].swapcount.sum() > 0
        for a in range(PER - 1):
            assert got.swapcount[b * PER + a] <= batch.swap_attempts(a, 0, N_ROUNDS, ladder=b)
        assert sum(batch.swap_attempts(a, 0, N_ROUNDS, ladder=b) for a in range(PER - 1)) == N_ROUNDS
    assert [batch.swap_pair(r, ladder=1) for r in range(5)] == [capi.swap_pair(seeds[1], r, PER) for r in range(5)]
    batch.close()


@pytest.mark.parametrize("waves,flags", [(4, 0), (4, SRL), (1, 0), (4, EO), (8, EO | SRL)])
def test_swaps_never_cross_a_ladder_edge(waves, flags):
    """two ladders of 4 chains, every beta 1 -- r = 0 > ln U: every attempt swaps -- the upper ladder at the
    workload's own start point (far better than the lower ladder's, which sits at the far end of the offset's
    range: 1.3 off at sigma 0.5 over 256 points, some 800 in log-likelihood), every chain marked by its own offset,
    step widths of 1e-13 of the range so that a point stays recognisable: after 403 rounds every point of a ladder is
    one of that ladder's start points, the last chain of each ladder never counted a swap, and inside the ladders the
    points did move (seeds and round count for which the composed permutation is not the identity: every attempt
    swaps, so it follows from apemost_hip_swap_pair alone; even-odd sweeps of 4 chains have period 8)"""
    per, n_ladders, n_rounds = 4, 2, 403
    w = wl.simplesin(n_data=256, n_chain=per)
    rng_ = w.pmax - w.pmin
    sts = []
    for b in range(n_ladders):
        st = LadderState.from_params(per, w.start, w.pmin, w.pmax, rng_ * 1e-13)
        for i in range(per):
            st.params[i, 3] = (w.start[3] if b == 1 else w.pmin[3] + 0.9 * rng_[3]) + 1e-3 * rng_[3] * i
        st.params_best[:] = st.params
        sts.append(st)
    start = concat(sts)
    s = HipSampler.batch(w.model, w.n_par, per, w.data, seeds=[3, 5], waves_per_chain=waves, flags=flags)
    s.set_state(start)
    s.calc_model()                                                   # one call over both ladders
    s.synchronize()
    s0 = s.get_state()
    assert s0.prob[per:].min() > s0.prob[:per].max() + 100            # the upper ladder's points are far better
    got, _ = run(s, n_ladders * per, w.n_par, n_rounds, 2)
    s.close()
    marks = start.params[:, 3]
    for b in range(n_ladders):
        own, other = marks[b * per:(b + 1) * per], marks[(1 - b) * per:(2 - b) * per]
        for f in ("params", "params_best"):
            v = getattr(got, f)[b * per:(b + 1) * per, 3]
            assert np.all(np.abs(v[:, None] - own[None, :]).min(axis=1) < 1e-8 * rng_[3]), (b, f, v)
            assert np.all(np.abs(v[:, None] - other[None, :]).min(axis=1) > 1e-4 * rng_[3]), (b, f, v)
        assert got.swapcount[(b + 1) * per - 1] == 0
        assert got.swapcount[b * per:(b + 1) * per - 1].sum() > n_rounds // 2
        assert np.abs(got.params[b * per:(b + 1) * per, 3] - own).max() > 5e-4 * rng_[3]     # the points did move


@pytest.mark.parametrize("name,waves,segment", [("simplesin", 4, False), ("simplesin", 4, True), ("pulse", 8, False),
                                                 ("simplesin", 1, True)])
def test_calibration_of_a_batch_equals_three_standalone_calibrations(name, waves, segment, monkeypatch):
    """calibrate_chains over 3 x 8 chains with per-ladder data: status, sweep counts, step widths and the rest of the
    state bit for bit; once with a launch per block, so that segment boundaries fall inside"""
    if segment:
        monkeypatch.setenv("APEMOST_CALIB_SEGMENT_EVALS", "1")
    n_ladders = 3
    ws, seeds, sts, _, _ = ladders(name, n_ladders, init_prob=True)
    w = ws[0]
    cfg = capi.calib_defaults(burn_in_iterations=300, iter_limit=100000)
    batch = make_batch(ws, seeds, waves)
    batch.set_state(concat(sts))
    status, iters = batch.markov_chain_calibrate(0, n_ladders * PER, cfg)
    got = batch.get_state()
    if segment:
        assert batch.calibrate_stats()[0] > 50
    batch.close()
    for b in range(n_ladders):
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=waves)
        alone.set_state(sts[b])
        st1, it1 = alone.markov_chain_calibrate(0, PER, cfg)
        want = alone.get_state()
        alone.close()
        assert np.array_equal(status[b * PER:(b + 1) * PER], st1) and np.array_equal(iters[b * PER:(b + 1) * PER], it1), b
        assert it1.min() >= 200
        for f in ALL_FIELDS:
            assert np.array_equal(bits(getattr(got, f)[b * PER:(b + 1) * PER]), bits(getattr(want, f))), (b, f)
    assert len({iters[b * PER:(b + 1) * PER].tobytes() for b in range(n_ladders)}) == n_ladders


def test_calc_model_and_step_for_on_a_range_that_spans_two_ladders():
    n_ladders, first, count = 3, 5, 6                               # chains 5 .. 10: ladders 0 and 1
    ws, seeds, sts, _, _ = ladders("sine3", n_ladders)
    w = ws[0]
    batch = make_batch(ws, seeds, 2)
    batch.set_state(concat(sts))
    batch.calc_model(first, count)
    batch.synchronize()
    part = batch.get_state()
    batch.calc_model()
    import torch
    d = torch.zeros((5, n_ladders * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    batch.markov_chain_step_for(4, 5, d.data_ptr())
    batch.synchronize()
    got, rows = batch.get_state(), d.cpu().numpy()
    batch.close()
    for b in range(n_ladders):
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=2)
        alone.set_state(sts[b])
        alone.calc_model()
        alone.synchronize()
        st = alone.get_state()
        for c in range(b * PER, (b + 1) * PER):
            inside = first <= c < first + count
            for f in ("prob", "prior"):
                want = getattr(st, f)[c - b * PER] if inside else getattr(sts[b], f)[c - b * PER]
                assert bits(np.array([getattr(part, f)[c]]))[0] == bits(np.array([want]))[0], (c, f)
        d1 = torch.zeros((5, PER, w.n_par + 2), dtype=torch.float64, device="cuda")
        alone.markov_chain_step_for(4, 5, d1.data_ptr())
        alone.synchronize()
        want = alone.get_state()
        alone.close()
        for f in ALL_FIELDS:
            assert np.array_equal(bits(getattr(got, f)[b * PER:(b + 1) * PER]), bits(getattr(want, f))), (b, f)
        assert np.array_equal(bits(rows[:, b * PER:(b + 1) * PER]), bits(d1.cpu().numpy())), b
        assert want.params_accepts[:, 4].sum() + want.params_rejects[:, 4].sum() == 5 * PER


def test_what_a_batch_refuses_on_the_device_and_what_an_ordinary_sampler_answers():
    L = capi.lib()
    w = wl.simplesin(n_data=64, n_chain=4)
    s = HipSampler.batch(w.model, w.n_par, 4, w.data, seeds=[1, 2, 3])
    one = HipSampler.batch(w.model, w.n_par, 4, w.data, seeds=[9])
    plain = HipSampler(w.model, w.n_par, 4, w.data, seed=9)
    n = C.c_int32(0)
    for sampler, want in ((s, 3), (one, 1), (plain, 1)):
        capi.check(L.apemost_hip_n_ladders(sampler._h, C.byref(n)))
        assert n.value == want

    def refused(rc, code, needle):
        assert rc == code and needle in L.apemost_hip_last_error().decode(), (rc, L.apemost_hip_last_error())
    import torch
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    handles = (C.c_void_p * 1)(s._h)
    refused(L.apemost_hip_run_shards(handles, 1, 1, 1, None), capi.ERR_UNSUPPORTED, "ladder batch")
    mixed = (C.c_void_p * 2)(plain._h, s._h)
    refused(L.apemost_hip_run_shards(mixed, 2, 1, 1, None), capi.ERR_UNSUPPORTED, "ladder batch")
    refused(L.apemost_hip_edge_export(s._h, 0, buf.data_ptr()), capi.ERR_UNSUPPORTED, "not sharded")
    refused(L.apemost_hip_edge_import(s._h, 1, buf.data_ptr()), capi.ERR_UNSUPPORTED, "not sharded")
    refused(L.apemost_hip_edge_exchange(plain._h, s._h), capi.ERR_UNSUPPORTED, "not sharded")
    L.apemost_hip_set_chain_offset.argtypes = [C.c_void_p, C.c_int64]
    refused(L.apemost_hip_set_chain_offset(s._h, 0), capi.ERR_UNSUPPORTED, "not sharded")
    refused(int(L.apemost_hip_sampler_swap_pair(s._h, 0)), capi.ERR_INVALID, "ambiguous")
    with pytest.raises(ValueError, match="ladder="):
        s.swap_pair(0)
    with pytest.raises(capi.ApemostHipError, match="no single data matrix") as e:
        s.loglike(w.start, 1.0)
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert np.array_equal(bits(one.loglike(w.start, 1.0)[0]), bits(plain.loglike(w.start, 1.0)[0]))
    dp = w.data.ctypes.data_as(C.POINTER(C.c_double))
    refused(L.apemost_hip_set_data_ladder(s._h, 3, dp), capi.ERR_INVALID, "outside")
    refused(L.apemost_hip_set_data_ladder(plain._h, 1, dp), capi.ERR_INVALID, "outside")
    capi.check(L.apemost_hip_set_data_ladder(plain._h, 0, dp))
    with pytest.raises(capi.ApemostHipError, match="1, 2, 4 or 8 waves") as e:
        HipSampler.batch(w.model, w.n_par, 4, w.data, seeds=[1, 2], waves_per_chain=6)
    assert e.value.code == capi.ERR_INVALID
    from apemost_amd.distributed import HipShardEngine, ShardedLadder
    with pytest.raises(ValueError, match="ladder batch"):
        ShardedLadder(HipShardEngine(s, torch), 4, 0, 4, 0, 1)
    for sampler in (s, one, plain):
        sampler.close()


def test_replicas_share_one_data_matrix_and_feed_gelman_rubin():
    """apemost_hip_set_data gives every ladder the same matrix: 8 replicas of one problem differ by their seeds
    only, each equals the stand-alone sampler, and R-hat of the beta = 1 chains and the evidence per ladder come
    out of the rows and the on-device summary"""
    from apemost_amd.summary import gelman_rubin
    n_ladders, n_rounds, n_swap = 8, 400, 5
    w = wl.simplesin(n_data=256, n_chain=PER)
    st, _, _ = make_pair(w, PER, seed=1)
    seeds = list(range(40, 40 + n_ladders))
    s = HipSampler.batch(w.model, w.n_par, PER, w.data, seeds, waves_per_chain=4)
    s.set_state(concat([st] * n_ladders))
    import torch
    d = torch.zeros((n_rounds * n_swap, n_ladders * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    s.summary_begin(n_hist_chains=0, batch_size=n_rounds * n_swap)    # (no batch sums wanted: none closes, max_batches 0)
    s.run_sampler(n_rounds, n_swap, d.data_ptr())
    s.summary_accumulate(d.data_ptr(), n_rounds * n_swap, skip=n_rounds * n_swap // 2)
    rs = s.summary()
    s.synchronize()
    got, rows = s.get_state(), d.cpu().numpy()
    s.close()
    alone = HipSampler(w.model, w.n_par, PER, w.data, seed=seeds[5], waves_per_chain=4)
    alone.set_state(st)
    want, want_rows = run(alone, PER, w.n_par, n_rounds, n_swap)
    alone.close()
    assert np.array_equal(bits(rows[:, 5 * PER:6 * PER]), bits(want_rows))
    assert np.array_equal(bits(got.params[5 * PER:6 * PER]), bits(want.params))
    rhat = gelman_rubin(rows[n_rounds * n_swap // 2:], n_ladders)
    ev = rs.evidence_per_ladder(got.beta, n_ladders)
    print("R-hat", rhat, "evidence per replica", ev)
    assert rhat.shape == (w.n_par,) and np.all(np.isfinite(rhat)) and np.all(rhat > 0.99)
    assert ev.shape == (n_ladders,) and np.all(np.isfinite(ev)) and len(set(ev.tolist())) == n_ladders


def test_rate_floor_a_batch_is_at_least_as_fast_as_its_samplers_one_after_another():
    """16 ladders x 8 chains x 1024 points, simplesin, n_swap 15: the batch does the same work with one sixteenth
    of the launches and sixteen times the CUs busy, so it must be at least as fast as the same 16 samplers run one
    after another in this process: ratio >= 1.0, median of 5, no margin."""
    n_ladders, n_swap, n_rounds = 16, 15, 400
    ws, seeds, sts, _, _ = ladders("simplesin", n_ladders, n_data=1024)
    w = ws[0]
    batch = make_batch(ws, seeds, 0)
    batch.set_state(concat(sts))
    alone = []
    for b in range(n_ladders):
        a = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b])
        a.set_state(sts[b])
        alone.append(a)
    steps = n_ladders * PER * n_rounds * n_swap

    def time_batch():
        t = time.perf_counter()
        batch.run_sampler(n_rounds, n_swap)
        batch.synchronize()
        return steps / (time.perf_counter() - t)

    def time_alone():
        t = time.perf_counter()
        for a in alone:
            a.run_sampler(n_rounds, n_swap)
            a.synchronize()
        return steps / (time.perf_counter() - t)
    time_batch(), time_alone()                                       # warm-up
    rb, ra = [], []
    for _ in range(5):
        rb.append(time_batch())
        ra.append(time_alone())
    for s in alone + [batch]:
        s.close()
    mb, ma = float(np.median(rb)), float(np.median(ra))
    print("ladder batch rate floor: batch %.4g steps/s (runs %s), one after another %.4g steps/s (runs %s), ratio %.3f"
          % (mb, ["%.3g" % r for r in rb], ma, ["%.3g" % r for r in ra], mb / ma))
    assert mb / ma >= 1.0
