"""On-device evidence fold (apemost_hip_evidence_*, pt_evidence.h) against tests/evidence_ref.py, a restatement that
shares nothing with the kernels.  The rule for every test: origin, sum, sq, batch and m compare with == on the bits (a
NaN by its position); S of a chain with a finite column to n 2^-50 relative against the exact sum -- each step adds at
most one ulp from exp (the device library's bound) and one from its multiply and add, under n 2^-51 in all, and the
tolerance gives a factor 2 over that."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.evidence import Evidence
from apemost_amd.sampler import HipSampler
from apemost_amd.summary import batches_closed
from tests import hostlib
from tests.evidence_ref import RefEvidence, assert_equals, same_floats
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu

FIELDS = ("origin", "sum", "sq", "batch", "m", "S")


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def same_evidence(a, b, what=""):
    """two Evidence objects, every field bit for bit (a NaN by its position)"""
    assert int(a.n[0]) == int(b.n[0]), what
    for f in FIELDS:
        assert same_floats(getattr(a, f), getattr(b, f)), (what, f)


def calls_of(pieces, thin, phase):
    """(first step, steps, skip) of consecutive calls over `pieces` steps each, keeping the global steps
    phase, phase + thin, ...; and the kept global steps"""
    out, first = [], 0
    for n in pieces:
        skip = (phase - first) % thin
        out.append((first, n, skip))
        first += n
    return out, np.arange(phase, first, thin)


# ---- hand-built rows ------------------------------------------------------------------------------------------------
def hand_built(n_steps=260, n_chains=300):
    """column n_par+1 per chain c by c % 8: values of the order of -10^3 .. -10^5 with unit spread; strictly
    increasing; strictly decreasing; constant; steps of at least 22 000 between consecutive samples, 5500 times the
    smallest coefficient that is not 0 (every exp underflows to 0, or the maximum moves); +inf, -inf and NaN inside,
    step 41 among them, which every test here keeps.  The coefficients go through both signs and 0, crossed
    with the column kinds."""
    rng = np.random.default_rng(86)
    t = np.arange(n_steps, dtype=np.float64)
    rows = rng.uniform(-1, 1, (n_steps, n_chains, 6))
    for c in range(n_chains):
        kind = c % 8
        noise = rng.standard_normal(n_steps)
        if kind == 0:
            v = -10.0 ** (3 + (c // 8) % 3) + noise
        elif kind == 1:
            v = -500.0 + 0.37 * t + 0.1 * np.sort(rng.uniform(0, 1, n_steps))
        elif kind == 2:
            v = -500.0 - 0.59 * t - 0.1 * np.sort(rng.uniform(0, 1, n_steps))
        elif kind == 3:
            v = np.full(n_steps, -1234.5)
        elif kind == 4:
            v = -50000.0 + 30000.0 * (t % 2) + 4000.0 * ((t // 2 + c) % 3) + noise
        else:
            v = -1000.0 + noise
            v[[41, n_steps // 2 + 1, n_steps - 60 + c % 11]] = (np.inf, -np.inf, np.nan)[kind - 5]
        rows[:, c, 5] = v
    up = np.array([0.0, 0.5, -0.3, 2.0])[(np.arange(n_chains) // 8) % 4]
    down = np.array([-1.0, -0.25, 0.7, 0.0])[(np.arange(n_chains) // 8 + np.arange(n_chains)) % 4]
    return rows, up, down


def test_hand_built_rows():
    """300 chains (five workgroups of the fold and a ragged one), three calls with skip 2 and thin 3, batch size 7: the
    first call ends on the sample that closes batch 3, the others inside a batch, and batches close inside every call"""
    rows, up, down = hand_built()
    pieces, thin, bs = [81, 92, 87], 3, 7
    calls, kept = calls_of(pieces, thin, 2)
    assert [len(np.arange(f + k, f + n, thin)) for f, n, k in calls] == [27, 30, 29] and 27 % bs == bs - 1
    w = wl.simplesin(n_data=16, n_chain=300)
    s = HipSampler(w.model, w.n_par, 300, w.data, seed=1)
    d = on_device(rows)
    nb = batches_closed(len(kept), bs)
    s.evidence_begin(betas=np.ones(300), batch_size=bs, max_batches=nb, coef_up=up, coef_down=down)
    for first, n, skip in calls:
        s.evidence_accumulate(d[first:].data_ptr(), n, skip, thin)
    got = s.evidence()
    s.close()
    ref = RefEvidence(rows[kept][:, :, 5], [up, down], bs, nb)
    assert int(ref.finite.sum()) == 37 * 5 + 4 and not ref.finite[[5, 6, 7]].any() and ref.finite[4]
    assert_equals(got, ref, "hand-built")
    # the kinds did what they are there for: a rescale at every step and none at all
    assert up[9] > 0 and got.m[0, 9] == up[9] * rows[kept[-1], 9, 5]          # increasing x: m is the last sample's
    assert down[2] > 0 and got.m[1, 2] == down[2] * rows[kept[0], 2, 5]       # decreasing x: m stays the first's
    assert np.isnan(got.sum[7]) and np.isinf(got.sum[5]) and np.isfinite(got.sum[[0, 1, 2, 3, 4]]).all()
    assert got.sq[3] == 0 and got.sum[3] == 0 and got.batch[3, 1] == 7 * -1234.5


# ---- staging --------------------------------------------------------------------------------------------------------
def numpy_fold(col, up, down, bs):
    """origin, sum, sq, batch from numpy's cumulative sums (which add in sample order), m as the maximum"""
    n, nc = col.shape
    d = col - col[0]
    nb = batches_closed(n, bs)
    starts = [0] + [k * bs - 1 for k in range(1, nb + 1)] + [n]
    if bs == 1:
        starts = list(range(n + 1))
    batch = np.zeros((nc, nb + 1))
    for k in range(nb + 1):
        if starts[k] < starts[k + 1]:
            batch[:, k] = np.cumsum(col[starts[k]:starts[k + 1]], axis=0)[-1]
    x = np.stack([up * col, down * col])
    return col[0], np.cumsum(d, axis=0)[-1], np.cumsum(d * d, axis=0)[-1], batch, x.max(axis=1), x


def check_numpy(got, col, up, down, bs, what):
    """the exact fields against numpy_fold with == on the bits.  S against the sum of numpy's exps taken by
    math.fsum: that reference is itself within 2^-52 of the exact sum (one ulp per exp, no summation error), which
    together with the device's n 2^-51 stays under the rule's n 2^-50 for every n >= 2"""
    import math
    origin, total, sq, batch, m, x = numpy_fold(col, up, down, bs)
    n = len(col)
    assert int(got.n[0]) == n, what
    for f, want in (("origin", origin), ("sum", total), ("sq", sq), ("batch", batch), ("m", m)):
        assert getattr(got, f).tobytes() == np.ascontiguousarray(want).tobytes(), (what, f)
    worst = 0.0
    for r in range(2):
        e = np.exp(x[r] - m[r])
        for c in range(col.shape[1]):
            want = math.fsum(e[:, c].tolist())
            worst = max(worst, abs(got.S[r, c] - want) / want)
    print("%s: n = %d, largest relative error of S %.3g = %.2f x 2^-53 (bound %.3g)" % (what, n, worst, worst * 2.0 ** 53,
                                                                                         n * 2.0 ** -50))
    assert worst <= n * 2.0 ** -50, (what, worst)


def test_many_chains_and_a_ragged_last_piece():
    """2048 chains bring the staged piece down to 2^20 / 2048 = 512 kept steps: the 700 kept steps of one call are one
    full piece and a ragged one of 188; batch size 26 closes batches in both and across the seam"""
    n_chains, n_steps, bs = 2048, 701, 26
    rng = np.random.default_rng(7)
    rows = rng.uniform(-1, 1, (n_steps, n_chains, 6))
    rows[:, :, 5] = -1000.0 - 3.0 * rng.uniform(0, 1, n_chains) + rng.standard_normal((n_steps, n_chains))
    up = rng.uniform(0.05, 1.5, n_chains)
    down = -rng.uniform(0.05, 1.0, n_chains)
    up[::5], down[::7] = 0.0, 0.4
    w = wl.simplesin(n_data=16, n_chain=n_chains)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    d = on_device(rows)
    s.evidence_begin(betas=np.ones(n_chains), batch_size=bs, max_batches=batches_closed(700, bs), coef_up=up, coef_down=down)
    s.evidence_accumulate(d.data_ptr(), n_steps, 1, 1)
    got = s.evidence()
    s.close()
    check_numpy(got, rows[1:, :, 5], up, down, bs, "2048 chains")
    ref = RefEvidence(rows[1:, ::256, 5], [up[::256], down[::256]], bs, batches_closed(700, bs))    # eight chains, exactly
    sub = Evidence(got.n, got.origin[::256], got.sum[::256], got.sq[::256], got.batch[::256], got.m[:, ::256],
                   got.S[:, ::256], np.ones(8), bs, up[::256], down[::256])
    assert_equals(sub, ref, "2048 chains, every 256th")


def test_one_chain_and_three_full_pieces():
    """one chain stages 2^18 kept steps per piece: 786 432 steps are three pieces, each exactly full"""
    n_steps, bs = 3 << 18, 886
    rng = np.random.default_rng(3)
    rows = np.zeros((n_steps, 1, 6))
    rows[:, 0, 5] = -1000.0 + 2.0 * np.sin(np.arange(n_steps) / 5000.0) + rng.standard_normal(n_steps)
    up, down = np.array([0.5]), np.array([-1.0])
    w = wl.simplesin(n_data=16, n_chain=1)
    s = HipSampler(w.model, w.n_par, 1, w.data, seed=1)
    d = on_device(rows)
    s.evidence_begin(betas=np.ones(1), batch_size=bs, max_batches=batches_closed(n_steps, bs), coef_up=up, coef_down=down)
    s.evidence_accumulate(d.data_ptr(), n_steps)
    got = s.evidence()
    s.close()
    check_numpy(got, rows[:, :, 5], up, down, bs, "one chain")


# ---- a real run -----------------------------------------------------------------------------------------------------
def test_a_real_run():
    """simplesin with 16 data points and 8 chains, two launches, the betas from the sampler: the device fold equals the
    restatement's fold of the rows read back, and origin n + sum is the run summary's prob_sum"""
    n_chain, n_rounds, n_swap, bs = 8, 30, 10, 17
    w = wl.simplesin(n_data=16, n_chain=n_chain)
    st, _, _ = make_pair(w, n_chain, seed=5)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=5)
    s.set_state(st)
    n_steps = 2 * n_rounds * n_swap
    d = torch.zeros((n_steps, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
    nb = batches_closed(n_steps, bs)
    s.evidence_begin(batch_size=bs, max_batches=nb)
    s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=bs, max_batches=nb)
    half = n_steps // 2
    for first in (0, half):
        s.run_sampler(n_rounds, n_swap, d[first:].data_ptr())
        s.evidence_accumulate(d[first:].data_ptr(), half)
        s.summary_accumulate(d[first:].data_ptr(), half)
    got, rs = s.evidence(), s.summary()
    s.close()
    betas = st.beta.copy()
    assert got.betas.tobytes() == betas.tobytes() and (betas > 0).all() and (np.diff(betas) < 0).all()
    up, down = Evidence.coefficients(betas)
    assert got.coef.tobytes() == np.array([up, down]).tobytes()
    rows = d.cpu().numpy()
    ref = RefEvidence(rows[:, :, w.n_par + 1], [up, down], bs, nb)
    assert ref.finite.all()
    assert_equals(got, ref, "a real run")
    total = got.origin * n_steps + got.sum
    assert np.all(np.abs(total - rs.prob_sum) <= 1e-12 * np.abs(rs.prob_sum)), (total, rs.prob_sum)
    assert abs(got.thermodynamic("rectangle") - rs.evidence(betas)) <= 1e-12 * abs(rs.evidence(betas))
    host = Evidence.from_rows(rows, betas, batch_size=bs, max_batches=nb)      # (its S is the host's exp: not compared)
    for f in ("origin", "sum", "sq", "batch", "m"):
        assert getattr(got, f).tobytes() == getattr(host, f).tobytes(), f
    for name, v in got.totals():
        assert np.isfinite(v), name


# ---- a ladder batch -------------------------------------------------------------------------------------------------
def test_a_batch_of_three_ladders_equals_three_samplers():
    from tests.test_gpu_ladder_batch import concat, ladders, make_batch, N_ROUNDS, N_SWAP, PER
    ws, seeds, sts, _, _ = ladders("simplesin", 3)
    w = ws[0]
    n_steps, bs = N_ROUNDS * N_SWAP, 18
    nb = batches_closed(n_steps, bs)
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    d = torch.zeros((n_steps, 3 * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    batch.evidence_begin(batch_size=bs, max_batches=nb)
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.evidence_accumulate(d.data_ptr(), n_steps)
    got = batch.evidence()
    batch.close()
    assert got.n_ladders == 3 and got.coef[0, PER] == 0 and got.coef[1, PER - 1] == -1
    lads = got.per_ladder()
    for b in range(3):
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=4)
        alone.set_state(sts[b])
        da = torch.zeros((n_steps, PER, w.n_par + 2), dtype=torch.float64, device="cuda")
        alone.evidence_begin(batch_size=bs, max_batches=nb)
        alone.run_sampler(N_ROUNDS, N_SWAP, da.data_ptr())
        alone.evidence_accumulate(da.data_ptr(), n_steps)
        one = alone.evidence()
        alone.close()
        same_evidence(lads[b], one, "ladder %d" % b)
        assert lads[b].coef.tobytes() == one.coef.tobytes() and np.isfinite(one.S).all()
        assert lads[b].stepping_stone("up") == one.stepping_stone("up")
    assert lads[0].sum.tobytes() != lads[1].sum.tobytes()


# ---- resume and refusals --------------------------------------------------------------------------------------------
def test_set_resumes_and_refusals_leave_the_fold_intact():
    rows, up, down = hand_built(n_steps=120, n_chains=96)
    fin = np.isfinite(rows[:, :, 5]).all(axis=0)
    rows[:, ~fin, 5] = -777.0                                 # (S is compared too: finite columns throughout)
    w = wl.simplesin(n_data=16, n_chain=96)
    s = HipSampler(w.model, w.n_par, 96, w.data, seed=1)
    d = on_device(rows)
    L = capi.lib()
    bs, nb = 7, batches_closed(120, 7)
    ev0 = Evidence.empty(np.ones(96), bs, nb, up, down)
    # without begin
    assert L.apemost_hip_evidence_accumulate(s._h, d.data_ptr(), 12, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_evidence_get(s._h, C.byref(ev0.view())) == capi.ERR_INVALID
    assert L.apemost_hip_evidence_set(s._h, C.byref(ev0.view())) == capi.ERR_INVALID
    s.evidence_begin(betas=np.ones(96), batch_size=bs, max_batches=nb, coef_up=up, coef_down=down)
    s.evidence_accumulate(d.data_ptr(), 120)
    whole = s.evidence()
    s.evidence_begin(betas=np.ones(96), batch_size=bs, max_batches=nb, coef_up=up, coef_down=down)
    s.evidence_accumulate(d.data_ptr(), 53)
    part = s.evidence()
    s.evidence_end()
    assert int(part.n[0]) == 53
    assert L.apemost_hip_evidence_get(s._h, C.byref(ev0.view())) == capi.ERR_INVALID       # ended
    s.evidence_begin(betas=np.ones(96), batch_size=bs, max_batches=nb, coef_up=up, coef_down=down)
    s.evidence_set(part)

    # every refusal, with the resumed fold open: it stays as it was
    dp = capi._dp

    def begin(batch_size=bs, max_batches=nb, up_=up, down_=down):
        cfg = capi.EvidenceConfig(batch_size=batch_size, max_batches=max_batches,
                                  coef_up=None if up_ is None else up_.ctypes.data_as(dp),
                                  coef_down=None if down_ is None else down_.ctypes.data_as(dp))
        return L.apemost_hip_evidence_begin(s._h, C.byref(cfg))
    bad = [up.copy(), up.copy(), down.copy()]
    bad[0][95], bad[1][0], bad[2][17] = np.nan, np.inf, -np.inf
    assert L.apemost_hip_evidence_begin(s._h, None) == capi.ERR_INVALID
    for kw in (dict(batch_size=0), dict(up_=bad[0]), dict(up_=bad[1]), dict(down_=bad[2]), dict(up_=None),
               dict(max_batches=1 << 41)):
        assert begin(**kw) == capi.ERR_INVALID, kw
    assert L.apemost_hip_evidence_accumulate(s._h, d[53:].data_ptr(), 67, 0, 0) == capi.ERR_INVALID        # thin 0
    assert L.apemost_hip_evidence_accumulate(s._h, None, 67, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_evidence_accumulate(s._h, d.data_ptr(), 120, 0, 1) == capi.ERR_INVALID           # batch nb + 1
    assert L.apemost_hip_evidence_get(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_evidence_accumulate(s._h, d.data_ptr(), 120, 120, 1) == capi.OK                  # keeps nothing
    same_evidence(s.evidence(), part, "after the refusals")
    s.evidence_accumulate(d[53:].data_ptr(), 67)
    same_evidence(s.evidence(), whole, "resumed")
    assert np.isfinite(whole.S).all() and whole.origin.tobytes() == rows[0, :, 5].tobytes()
    # a set whose n closes more batches than there is room for
    over = Evidence.empty(np.ones(96), bs, nb, up, down)
    over.n[0] = 7 * (nb + 1)
    assert L.apemost_hip_evidence_set(s._h, C.byref(over.view())) == capi.ERR_INVALID
    same_evidence(s.evidence(), whole, "after a refused set")
    # the sampler still steps
    st, _, _ = make_pair(w, 96, seed=1)
    s.set_state(st)
    dd = torch.zeros((15, 96, w.n_par + 2), dtype=torch.float64, device="cuda")
    s.run_sampler(3, 5, dd.data_ptr())
    s.synchronize()
    assert np.array_equal(s.get_state().n_iter, st.n_iter + 15)
    s.close()


# ---- the C host: APEMOST_DUMP=evidence,binary -------------------------------------------------------------------------
def test_c_host_evidence_token(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters = 8, 3000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    work = tmp_path / "evidence_binary"
    work.mkdir()
    (work / "params").write_text(w.params_file_text())
    (work / "data").write_text(w.data_file_text())
    env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP="evidence,binary")
    for phase in ("calibrate_first", "calibrate_rest", "run"):
        subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)

    def check(n):
        ev = Evidence.read(str(work / "evidence.bin"))
        _, _, probs = samples_bin.read(str(work / "samples.bin"))           # [iterations][n_beta][2]
        assert int(ev.n[0]) == n == len(probs) and ev.n_chains == n_beta and ev.n_ladders == 1 and ev.thin == 1
        assert ev.batch_size == int(np.sqrt(iters)) and ev.max_batches == batches_closed(n, ev.batch_size)
        up, down = Evidence.coefficients(ev.betas)
        assert ev.coef.tobytes() == np.array([up, down]).tobytes() and ev.betas[0] == 1.0
        ref = RefEvidence(probs[:, :, 1], [up, down], ev.batch_size, ev.max_batches)
        assert ref.finite.all()
        assert_equals(ev, ref, "C host, %d" % n)
        lines = (work / "evidence.txt").read_text().split("\n")
        totals = ev.totals()
        assert lines[-1] == "" and len(lines) == n_beta + len(totals) + 1
        table = np.array([[float(x) for x in l.split("\t")] for l in lines[:n_beta]])
        want = np.array([ev.betas, ev.mean_loglike(), ev.var_loglike(), ev.mcse(), ev.ln_mean_exp("up"),
                         ev.ln_mean_exp("down")]).T
        assert np.all(np.abs(table - want) <= 1e-12 * np.abs(want)), (table, want)
        for line, (name, v) in zip(lines[n_beta:], totals):
            got_name, got_v = line.split("\t")
            assert got_name == name and abs(float(got_v) - v) <= 1e-12 * abs(v), (line, v)
            assert np.isfinite(v), name
        return ev
    first = check(iters)
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = check(2 * iters)                                 # one fold of the combined length: samples.bin holds both
    assert second.origin.tobytes() == first.origin.tobytes() and second.batch_size == first.batch_size
    nb = first.n_batches
    assert second.batch[:, :nb].tobytes() == first.batch[:, :nb].tobytes()
