"""Ragged ladder batches (apemost_hip_create_batch_ragged, include/apemost_hip.h): one data set per
ladder, each of its own length, in one sampler and one launch.  The identity the tests rest on is the one of every
batch: ladder b is BIT FOR BIT the stand-alone sampler with n_data = len_b, seed seeds[b], ladder b's data and the same
waves_per_chain -- `==` on the raw bits of every sample row and every field of the final state.  The lengths are those
of tests/data_lengths.py, so that every loop regime of the likelihood a (model, waves) pair can reach occurs inside one
launch, with the ladders' matrices starting at odd offsets.  Against the CPU oracle the repository's parity rule holds
(DESIGN 7).  4 chains per ladder, 60 rounds of 3 steps."""
import ctypes as C
import time

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler
from apemost_amd.state import ALL_FIELDS, LadderState
from oracle import oracle as orc
from tests import data_lengths as dl
from tests import pointwise_ref, predict_ref
from tests.helpers import assert_match, make_pair

pytestmark = pytest.mark.gpu
EO, SRL, TWO = capi.FLAG_SWAP_EVEN_ODD, capi.FLAG_SINGLE_ROUND_LAUNCHES, capi.FLAG_TWO_BARRIER_STEP
PER, N_ROUNDS, N_SWAP = 4, 60, 3


def bits(a):
    """the raw bits: NaN payloads and signed zeros count"""
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def ladders(name, lengths, per=PER, init_prob=False):
    """one problem per length: own data (the workload's generator under another seed), own seed, own betas and
    step widths; (workloads, seeds, states, oracle ladders, oracle rngs)"""
    ws, seeds, sts, lads, rngs = [], [], [], [], []
    for b, n in enumerate(lengths):
        w = wl.by_name(name, n_data=int(n), n_chain=per, seed=500 + 7 * b)
        seed = 1000 + 13 * b
        st, lad, rng = make_pair(w, per, beta_0=0.02 + 0.01 * (b % 5), seed=seed, init_prob=init_prob)
        ws.append(w), seeds.append(seed), sts.append(st), lads.append(lad), rngs.append(rng)
    return ws, seeds, sts, lads, rngs


def concat(sts):
    out = LadderState(sum(s.n_chain for s in sts), sts[0].n_par)
    for f in ALL_FIELDS:
        getattr(out, f)[...] = np.concatenate([getattr(s, f) for s in sts])
    return out


def run(s, n_chains, n_par, n_rounds=N_ROUNDS, n_swap=N_SWAP):
    import torch
    d = torch.zeros((n_rounds * n_swap, n_chains, n_par + 2), dtype=torch.float64, device="cuda")
    s.run_sampler(n_rounds, n_swap, d.data_ptr())
    s.synchronize()
    assert s.round == (n_rounds, False)
    return s.get_state(), d.cpu().numpy()


def make_batch(ws, seeds, waves, flags=0, per=PER, **kw):
    w = ws[0]
    return HipSampler.batch(w.model, w.n_par, per, [x.data for x in ws], seeds, waves_per_chain=waves, flags=flags, **kw)


def ladder_n_data(s, b):
    n = C.c_int32(-1)
    capi.check(s.L.apemost_hip_ladder_n_data(s._h, b, C.byref(n)))
    return n.value


def check_ragged_equals_standalone(name, waves, lengths, flags=0, **kw):
    lengths = [int(n) for n in lengths]
    n_ladders = len(lengths)
    ws, seeds, sts, _, _ = ladders(name, lengths)
    w = ws[0]
    batch = make_batch(ws, seeds, waves, flags, **kw)
    assert batch.n_ladders == n_ladders and batch.n_chains == n_ladders * PER
    assert batch.n_data_per_ladder == lengths and batch.cfg.n_data == max(lengths)
    assert [ladder_n_data(batch, b) for b in range(n_ladders)] == lengths
    assert batch.geometry[0] == waves
    policy = batch.launch_policy
    assert policy[0] == (waves in (4, 8) and not flags & TWO) and policy[2] == (1 if flags & SRL else 1024)
    batch.set_state(concat(sts))
    got, rows = run(batch, n_ladders * PER, w.n_par)
    batch.close()
    for b in range(n_ladders):
        what = (name, waves, flags, b, lengths[b])
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=waves, flags=flags, **kw)
        alone.set_state(sts[b])
        want, want_rows = run(alone, PER, w.n_par)
        alone.close()
        for f in ALL_FIELDS:
            assert np.array_equal(bits(batch.ladder_view(getattr(got, f), b)), bits(getattr(want, f))), what + (f,)
        assert np.array_equal(bits(batch.ladder_view(rows, b)), bits(want_rows)), what
        assert want.swapcount[PER - 1] == 0 and int(want.swapcount.sum()) > 0, what
    assert len({bits(batch.ladder_view(rows, b)).tobytes() for b in range(n_ladders)}) == n_ladders
    return got, rows


SHAPES = [("simplesin", 1), ("simplesin", 2), ("sine3", 2), ("simplesin", 4), ("simplesin", 8), ("pulse", 8),
          ("pulse_vrot", 1), ("pulse_vrot", 4)]


@pytest.mark.parametrize("name,waves", SHAPES)
def test_every_loop_regime_in_one_launch_equals_the_standalone_samplers_bit_for_bit(name, waves):
    """one ladder per length of data_lengths.sampling_lengths, ascending: rows in registers, the pipelined passes,
    wide4 / wide2 / tail, a partial wave, idle waves and a staged vector over 64 KiB side by side in one grid"""
    lengths = dl.sampling_lengths(waves, name)
    reached = set().union(*[dl.regimes(n, waves, name) for n in lengths])
    assert reached == dl.reachable(waves, name) and len(set(lengths)) > 3
    check_ragged_equals_standalone(name, waves, lengths)


@pytest.mark.parametrize("order", ["descending", "shuffled"])
def test_the_order_of_the_lengths_does_not_matter(order):
    lengths = dl.sampling_lengths(4, "simplesin")
    lengths = lengths[::-1] if order == "descending" else list(np.random.RandomState(5).permutation(lengths))
    assert lengths != sorted(lengths)
    check_ragged_equals_standalone("simplesin", 4, lengths)


@pytest.mark.parametrize("policy", [1, 2])
@pytest.mark.parametrize("name,waves", [("simplesin", 4), ("pulse_vrot", 1)])
def test_staged_in_lds_and_read_through_l2(name, waves, policy):
    """lds_policy 1: every ladder's vector staged in an LDS block sized for the longest; 2: none staged"""
    check_ragged_equals_standalone(name, waves, dl.sampling_lengths(waves, name), lds_policy=policy)


@pytest.mark.parametrize("waves,flags", [(4, SRL), (4, EO), (8, TWO)])
def test_single_round_launches_even_odd_sweeps_and_the_two_barrier_step(waves, flags):
    check_ragged_equals_standalone("simplesin", waves, dl.sampling_lengths(waves, "simplesin"), flags)


def test_the_helper_kernel_that_keeps_the_grids_length_is_not_launched_on_unequal_lengths():
    """pulse_vrot, eight likelihood waves, data through L2: the stand-alone samplers step with the helper wavefront,
    and that one instantiation does not read a ladder's own length (ob_takes_ladder_length, pt_kernels.h); the ragged
    batch steps without the helper and gives the same chains"""
    lengths = dl.sampling_lengths(8, "pulse_vrot")
    w = wl.by_name("pulse_vrot", n_data=lengths[0], n_chain=PER)
    probe = HipSampler(w.model, w.n_par, PER, w.data, waves_per_chain=8, lds_policy=2)
    assert probe.ob_helper and probe.geometry == (8, False)
    probe.close()
    check_ragged_equals_standalone("pulse_vrot", 8, lengths, lds_policy=2)
    check_ragged_equals_standalone("pulse_vrot", 8, lengths, SRL, lds_policy=2)


def test_all_lengths_equal_is_the_sampler_create_batch_makes():
    ws, seeds, sts, _, _ = ladders("simplesin", [300, 300, 300])
    w = ws[0]
    out = []
    for ragged in (False, True):
        s = HipSampler.batch(w.model, w.n_par, PER, [x.data for x in ws], seeds, waves_per_chain=4, ragged=ragged)
        assert s.n_data_per_ladder == [300] * 3 and [ladder_n_data(s, b) for b in range(3)] == [300] * 3
        if ragged:                                       # one matrix for every ladder is legal again
            s.set_data(ws[1].data)
            for b in range(3):
                s.set_data(ws[b].data, ladder=b)
        s.set_state(concat(sts))
        out.append(run(s, 3 * PER, w.n_par) + (s.geometry, s.launch_policy))
        s.close()
    (st0, rows0, g0, p0), (st1, rows1, g1, p1) = out
    assert g0 == g1 and p0 == p1
    assert np.array_equal(bits(rows0), bits(rows1))
    for f in ALL_FIELDS:
        assert np.array_equal(bits(getattr(st0, f)), bits(getattr(st1, f))), f


@pytest.mark.parametrize("segment", [False, True])
def test_calibration_of_a_ragged_batch_equals_three_standalone_calibrations(segment, monkeypatch):
    """status, sweep counts and the state bit for bit; once with a launch per block, so that segment boundaries fall
    inside"""
    if segment:
        monkeypatch.setenv("APEMOST_CALIB_SEGMENT_EVALS", "1")
    lengths = dl.calibration_lengths(4, "simplesin")
    assert len(set(lengths)) == 3
    ws, seeds, sts, _, _ = ladders("simplesin", lengths, init_prob=True)
    w = ws[0]
    cfg = capi.calib_defaults(burn_in_iterations=100, iter_limit=100000)
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    status, iters = batch.markov_chain_calibrate(0, 3 * PER, cfg)
    got = batch.get_state()
    batch.close()
    for b in range(3):
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=4)
        alone.set_state(sts[b])
        st1, it1 = alone.markov_chain_calibrate(0, PER, cfg)
        want = alone.get_state()
        alone.close()
        assert np.array_equal(status[b * PER:(b + 1) * PER], st1) and np.array_equal(iters[b * PER:(b + 1) * PER], it1), b
        for f in ALL_FIELDS:
            assert np.array_equal(bits(getattr(got, f)[b * PER:(b + 1) * PER]), bits(getattr(want, f))), (b, f)


def test_calc_model_and_step_for_on_a_range_that_spans_two_ladders_of_different_length():
    import torch
    lengths, first, count = [65, 300, 130], 2, 4                    # chains 2 .. 5: ladders 0 and 1
    ws, seeds, sts, _, _ = ladders("sine3", lengths)
    w = ws[0]
    batch = make_batch(ws, seeds, 2)
    batch.set_state(concat(sts))
    batch.calc_model(first, count)
    batch.synchronize()
    part = batch.get_state()
    batch.calc_model()
    d = torch.zeros((5, 3 * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    batch.markov_chain_step_for(4, 5, d.data_ptr())
    batch.synchronize()
    got, rows = batch.get_state(), d.cpu().numpy()
    batch.close()
    for b in range(3):
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


@pytest.mark.parametrize("name", ["simplesin", "pulse"])
def test_against_the_oracle(name):
    """lengths 65 and 257 with the engine's own geometry: each ladder against orc.run_sampler seeded with that
    ladder's seed; integer state exact, rows and state rel 1e-9"""
    lengths = [65, 257]
    ws, seeds, sts, lads, rngs = ladders(name, lengths)
    batch = make_batch(ws, seeds, 0)
    batch.set_state(concat(sts))
    got, rows = run(batch, 2 * PER, ws[0].n_par)
    batch.close()
    for b in range(2):
        ref = orc.run_sampler(lads[b], rngs[b], N_ROUNDS, N_SWAP, record=True, n_threads=8)
        assert_match(got.slice(b * PER, (b + 1) * PER), lads[b], rngs[b], what="ragged %s ladder %d" % (name, b))
        np.testing.assert_allclose(batch.ladder_view(rows, b), ref, rtol=1e-9, atol=1e-300)
        assert lads[b].swapcount.sum() > 0


# ---- the folds ------------------------------------------------------------------------------------------------------
FOLD_LENGTHS = [1, 63, 64, 65, 130]


@pytest.fixture(scope="module")
def folded():
    """one ragged run shared by the fold tests, read-only: (workloads, seeds, states, the batch, its device rows)"""
    import torch
    ws, seeds, sts, _, _ = ladders("simplesin", FOLD_LENGTHS)
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    n_steps = N_ROUNDS * N_SWAP
    d = torch.zeros((n_steps, len(ws) * PER, ws[0].n_par + 2), dtype=torch.float64, device="cuda")
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.synchronize()
    yield ws, seeds, sts, batch, d
    batch.close()


def ladder_rows(d, b):
    return d[:, b * PER:(b + 1) * PER].contiguous()


def alone_for(ws, seeds, b):
    w = ws[b]
    return HipSampler(w.model, w.n_par, PER, w.data, seed=seeds[b], waves_per_chain=4)


def test_the_folds_over_sample_rows_alone_know_nothing_of_data_lengths(folded):
    """summary, joint, evidence and autocorr of a ragged batch: each equals the same fold fed ladder b's rows on a
    stand-alone sampler"""
    from apemost_amd.summary import batches_closed
    ws, seeds, sts, batch, d = folded
    w, n_l, n_steps = ws[0], len(ws), N_ROUNDS * N_SWAP
    bs = 7
    nb = batches_closed(n_steps, bs)
    chains = [b * PER for b in range(n_l)]
    batch.summary_begin(w.pmin, w.pmax, n_hist_chains=n_l * PER, nbins=50, batch_size=bs, max_batches=nb)
    batch.joint_begin(w.pmin, w.pmax, chains=chains, nbins=50)
    batch.evidence_begin(batch_size=bs, max_batches=nb)
    batch.autocorr_begin(chains=chains, max_lag=17)
    for f in ("summary", "joint", "evidence", "autocorr"):
        getattr(batch, f + "_accumulate")(d.data_ptr(), n_steps)
    rs, jt, ev, ac = batch.summary(), batch.joint(), batch.evidence(), batch.autocorr()
    for f in ("summary", "joint", "evidence", "autocorr"):
        getattr(batch, f + "_end")()
    evs, acs = ev.per_ladder(), ac.per_ladder()
    for b in range(n_l):
        alone, rows = alone_for(ws, seeds, b), ladder_rows(d, b)
        alone.summary_begin(w.pmin, w.pmax, n_hist_chains=PER, nbins=50, batch_size=bs, max_batches=nb)
        alone.joint_begin(w.pmin, w.pmax, chains=(0,), nbins=50)
        alone.evidence_begin(betas=sts[b].beta, batch_size=bs, max_batches=nb)
        alone.autocorr_begin(chains=(0,), max_lag=17)
        for f in ("summary", "joint", "evidence", "autocorr"):
            getattr(alone, f + "_accumulate")(rows.data_ptr(), n_steps)
        rs1, jt1, ev1, ac1 = alone.summary(), alone.joint(), alone.evidence(), alone.autocorr()
        alone.close()
        mine = slice(b * PER, (b + 1) * PER)               # (histograms and batch sums of every chain: [h][p][...])
        assert (rs.n, rs.n_batches, rs.batch_size) == (rs1.n, rs1.n_batches, rs1.batch_size) and rs1.n_batches == nb, b
        assert np.array_equal(bits(rs.prob_sum[mine]), bits(rs1.prob_sum)), b
        assert np.array_equal(rs.hist[mine], rs1.hist) and rs1.hist.sum() > 0, b
        assert np.array_equal(bits(rs.batch_sums[mine]), bits(rs1.batch_sums)), b
        assert int(jt.n[0]) == int(jt1.n[0]) and np.array_equal(jt.counts[b], jt1.counts[0]), b
        for f in ("origin", "sum", "cross"):
            assert np.array_equal(bits(getattr(jt, f)[b]), bits(getattr(jt1, f)[0])), (b, f)
        for f in ("origin", "sum", "sq", "batch", "m", "S"):
            assert np.array_equal(bits(getattr(evs[b], f)), bits(getattr(ev1, f))), (b, f)
        for f in ("origin", "sum", "lag", "head", "tail"):
            assert np.array_equal(bits(getattr(acs[b], f)), bits(getattr(ac1, f))), (b, f)


def feed(s, prefix, d_ptr, n_steps, cut, thin):
    """two accumulate calls cut at the odd step `cut`, the second one taking up the thinning where the first left it"""
    acc = getattr(s, prefix + "_accumulate")
    acc(d_ptr, cut, 0, thin)
    kept = (cut + thin - 1) // thin
    acc(d_ptr, n_steps, kept * thin, thin)


@pytest.mark.parametrize("thin", [1, 3])
def test_predict_at_the_data_of_a_ragged_batch(folded, thin):
    ws, seeds, sts, batch, d = folded
    n_l, n_steps, cut = len(ws), N_ROUNDS * N_SWAP, 77
    w = ws[0]
    chains = [b * PER for b in range(n_l)]
    kw = dict(nbins=16, lo=-3.0, hi=3.0, thin=thin)
    batch.predict_begin(chains=chains, **kw)
    feed(batch, "predict", d.data_ptr(), n_steps, cut, thin)
    got = batch.predict()
    # get -> set -> accumulate equals the uninterrupted fold
    batch.predict_begin(chains=chains, **kw)
    batch.predict_accumulate(d.data_ptr(), cut, 0, thin)
    half = batch.predict()
    batch.predict_end()
    batch.predict_begin(chains=chains, **kw)
    batch.predict_set(half)
    batch.predict_accumulate(d.data_ptr(), n_steps, ((cut + thin - 1) // thin) * thin, thin)
    again = batch.predict()
    lens = np.zeros(n_l, dtype=np.int32)
    capi.check(batch.L.apemost_hip_predict_lengths(batch._h, lens.ctypes.data_as(C.POINTER(C.c_int32))))
    batch.predict_end()
    assert lens.tolist() == FOLD_LENGTHS and got.lengths.tolist() == FOLD_LENGTHS and got.n_x == max(FOLD_LENGTHS)
    assert int(got.n[0]) == (n_steps + thin - 1) // thin
    predict_ref.assert_equals(again, got, "get, set, accumulate")
    assert again.lengths.tolist() == FOLD_LENGTHS
    for b, m in enumerate(FOLD_LENGTHS):                              # the padding holds the initial values
        for f in ("origin", "sum", "sq", "x"):
            assert not getattr(got, f)[b, m:].any(), (b, f)
        assert np.all(got.vmin[b, m:] == np.inf) and np.all(got.vmax[b, m:] == -np.inf) and not got.hist[b, m:].any()
    with pytest.raises(ValueError, match=r"per_ladder\(\)"):
        got.chi2(np.zeros(got.n_x), 0.5)
    lads = got.per_ladder()
    for b in range(n_l):
        alone, rows = alone_for(ws, seeds, b), ladder_rows(d, b)
        alone.predict_begin(chains=(0,), **kw)
        feed(alone, "predict", rows.data_ptr(), n_steps, cut, thin)
        one = alone.predict()
        alone.close()
        assert one.lengths is None and lads[b].n_x == FOLD_LENGTHS[b]
        predict_ref.assert_equals(lads[b], one, "ladder %d" % b)
        assert np.array_equal(bits(lads[b].x), bits(one.x)) and np.array_equal(lads[b].x[0], ws[b].data[:, 0])
        assert np.isfinite(lads[b].chi2(ws[b].data[:, 1], 0.5))
    # over a caller's grid nothing depends on the data: no lengths
    batch.predict_begin(chains=chains, x=np.linspace(0, 1, 7))
    batch.predict_accumulate(d.data_ptr(), n_steps)
    assert batch.predict().lengths is None
    batch.predict_end()


@pytest.mark.parametrize("thin", [1, 3])
def test_pointwise_of_a_ragged_batch(folded, thin):
    ws, seeds, sts, batch, d = folded
    n_l, n_steps, cut = len(ws), N_ROUNDS * N_SWAP, 77
    chains = [b * PER for b in range(n_l)]
    batch.pointwise_begin(chains=chains, thin=thin)
    feed(batch, "pointwise", d.data_ptr(), n_steps, cut, thin)
    got = batch.pointwise()
    batch.pointwise_begin(chains=chains, thin=thin)
    batch.pointwise_accumulate(d.data_ptr(), cut, 0, thin)
    half = batch.pointwise()
    batch.pointwise_end()
    batch.pointwise_begin(chains=chains, thin=thin)
    batch.pointwise_set(half)
    batch.pointwise_accumulate(d.data_ptr(), n_steps, ((cut + thin - 1) // thin) * thin, thin)
    again = batch.pointwise()
    lens = np.zeros(n_l, dtype=np.int32)
    capi.check(batch.L.apemost_hip_pointwise_lengths(batch._h, lens.ctypes.data_as(C.POINTER(C.c_int32))))
    # the tail on kept ladders of unequal length is the follow-up
    rc = batch.L.apemost_hip_pointwise_tail_begin(batch._h, 64)
    assert rc == capi.ERR_UNSUPPORTED and "follow-up" in batch.L.apemost_hip_last_error().decode()
    batch.pointwise_end()
    with pytest.raises(capi.ApemostHipError) as e:
        batch.pointwise_begin(chains=chains, tail=64)
    assert e.value.code == capi.ERR_UNSUPPORTED
    batch.pointwise_end()
    batch.pointwise_begin(chains=[chains[2], chains[2] + 1], tail=64)     # kept chains of one ladder: one length, a tail
    assert batch.pointwise_tail_capacity() == 64
    batch.pointwise_accumulate(d.data_ptr(), n_steps)
    one_len = batch.pointwise()
    assert one_len.lengths is None and one_len.n_data == FOLD_LENGTHS[2] and batch.pointwise_tail().count.shape == (2, 64)
    batch.pointwise_end()
    assert lens.tolist() == FOLD_LENGTHS and got.lengths.tolist() == FOLD_LENGTHS and got.n_data == max(FOLD_LENGTHS)
    pointwise_ref.assert_same_state(again, got, "get, set, accumulate")
    for b, m in enumerate(FOLD_LENGTHS):                              # the padding holds the initial values
        for f in pointwise_ref.STATE + ("x", "y"):
            assert not getattr(got, f)[b, m:].any(), (b, f)
        assert np.isnan(got.at_mean[b, m:]).all() and np.isfinite(got.at_mean[b, :m]).all()
    with pytest.raises(ValueError, match=r"per_ladder\(\)"):
        got.waic()
    lads = got.per_ladder()
    for b in range(n_l):
        alone, rows = alone_for(ws, seeds, b), ladder_rows(d, b)
        alone.pointwise_begin(chains=(0,), thin=thin)
        feed(alone, "pointwise", rows.data_ptr(), n_steps, cut, thin)
        one = alone.pointwise()
        alone.close()
        assert one.lengths is None and lads[b].n_data == FOLD_LENGTHS[b]
        pointwise_ref.assert_same_state(lads[b], one, "ladder %d" % b)
        for f in ("x", "y", "at_mean"):
            assert np.array_equal(bits(getattr(lads[b], f)), bits(getattr(one, f))), (b, f)
        assert lads[b].criteria_text() == one.criteria_text()


# ---- refusals and getters ---------------------------------------------------------------------------------------------
def test_refusals_and_getters():
    L = capi.lib()
    ws, seeds, _, _, _ = ladders("simplesin", [65, 64, 130])
    w = ws[0]
    s = make_batch(ws, seeds, 4)
    equal = HipSampler.batch(w.model, w.n_par, PER, w.data, seeds=[1, 2])
    plain = HipSampler(w.model, w.n_par, PER, w.data, seed=9)

    def refused(rc, code, needle):
        assert rc == code and needle in L.apemost_hip_last_error().decode(), (rc, L.apemost_hip_last_error())
    big = np.ascontiguousarray(ws[2].data)
    dp = big.ctypes.data_as(C.POINTER(C.c_double))
    refused(L.apemost_hip_set_data(s._h, dp), capi.ERR_INVALID, "set_data_ladder")
    refused(L.apemost_hip_set_data_ladder(s._h, 3, dp), capi.ERR_INVALID, "outside")
    refused(L.apemost_hip_set_data_ladder(s._h, -1, dp), capi.ERR_INVALID, "outside")
    capi.check(L.apemost_hip_set_data_ladder(s._h, 2, dp))
    with pytest.raises(ValueError, match="ladder=b"):
        s.set_data(ws[0].data)
    with pytest.raises(ValueError, match=r"\[64\]\[2\]"):
        s.set_data(ws[0].data, ladder=1)
    with pytest.raises(ValueError, match="outside"):
        s.set_data(ws[0].data, ladder=3)
    assert [ladder_n_data(s, b) for b in range(3)] == [65, 64, 130]
    assert [ladder_n_data(equal, b) for b in range(2)] == [65, 65] and ladder_n_data(plain, 0) == 65
    n = C.c_int32(0)
    refused(L.apemost_hip_ladder_n_data(s._h, 3, C.byref(n)), capi.ERR_INVALID, "outside")
    refused(L.apemost_hip_ladder_n_data(plain._h, 1, C.byref(n)), capi.ERR_INVALID, "outside")
    with pytest.raises(capi.ApemostHipError, match="no single data matrix") as e:
        s.loglike(w.start, 1.0)
    assert e.value.code == capi.ERR_UNSUPPORTED
    assert s.pointwise_loglike(w.start, ladder=2).shape == (130,) and s.pointwise_loglike(w.start, ladder=1).shape == (64,)
    assert s.predict_curve(w.start).shape == (65,)
    for sampler in (s, equal, plain):
        sampler.close()


# ---- rate floor ---------------------------------------------------------------------------------------------------------
def test_rate_floor_a_ragged_batch_is_at_least_as_fast_as_its_samplers_one_after_another():
    """16 ladders x 8 chains, simplesin, lengths spread evenly from 256 to 1024, four waves on both sides, n_swap 15:
    the batch's launch lasts about as long as its longest ladder's, which cannot exceed the sum of the 16 stand-alone
    runs, and it takes one sixteenth of the launches: ratio >= 1.0, median of 5 after a warm-up, no margin."""
    n_ladders, per, n_swap, n_rounds = 16, 8, 15, 400
    lengths = [int(n) for n in np.linspace(256, 1024, n_ladders).round()]
    ws, seeds, sts, _, _ = ladders("simplesin", lengths, per=per)
    w = ws[0]
    batch = make_batch(ws, seeds, 4, per=per)
    batch.set_state(concat(sts))
    alone = []
    for b in range(n_ladders):
        a = HipSampler(w.model, w.n_par, per, ws[b].data, seed=seeds[b], waves_per_chain=4)
        a.set_state(sts[b])
        alone.append(a)
    steps = n_ladders * per * n_rounds * n_swap

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
    print("ragged batch rate floor: batch %.4g steps/s (runs %s), one after another %.4g steps/s (runs %s), ratio %.3f"
          % (mb, ["%.3g" % r for r in rb], ma, ["%.3g" % r for r in ra], mb / ma))
    assert mb / ma >= 1.0
