"""On-device joint marginals (apemost_hip_joint_*, pt_joint.h): pair histograms and moments equal
tests/joint_ref.py -- a restatement that shares nothing with the kernels -- with ==, on hand-built rows, on grids
that fill every cell of every band, over every call boundary, on real runs (where both projections are the run
summary's histograms), on a ladder batch, through joint_set and through the C host's APEMOST_DUMP=joint."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.joint import Joint, all_pairs, tri_index
from apemost_amd.sampler import HipSampler
from apemost_amd.summary import RunSummary, batches_closed
from tests import hostlib, summary_rows as sr
from tests.helpers import make_pair
from tests.joint_ref import RefJoint, assert_equals, same_floats
from tests.test_gpu_summary import _run

pytestmark = pytest.mark.gpu


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def same_joint(a, b):
    """two Joint objects, every field with == (the moments bit for bit, a NaN by its position)"""
    assert int(a.n[0]) == int(b.n[0]) and a.pairs.tolist() == b.pairs.tolist()
    assert np.array_equal(a.counts, b.counts)
    for f in ("origin", "sum", "cross"):
        assert same_floats(getattr(a, f), getattr(b, f)), f


# ---- hand-built rows against the restatement --------------------------------------------------------------------
HAND_CHAINS = [0, 1, 2, 299]


@pytest.fixture(scope="module")
def sampler300():
    w = wl.simplesin(n_data=16, n_chain=300)
    s = HipSampler(w.model, w.n_par, 300, w.data, seed=1)
    yield s
    s.close()


@pytest.mark.parametrize("box_set", ["A", "B"])
@pytest.mark.parametrize("nbins", [1, 37, 200, 512])
def test_joint_of_hand_built_rows(sampler300, box_set, nbins):
    """Every edge of every parameter with its two neighbours, the non-sorted edges of [1e15, 1e15+3], subnormals and
    non-finite values (tests/summary_rows.py), kept chains 0, 1, 2 and 299, all six pairs, in the three calls of
    summary_rows.CALLS.  Counts equal the restatement's with ==; the moments bit for bit (chains 1, 2 and 299 hold
    finite rows: origin and sum there are finite; a NaN -- inf - inf in a chain that saw an infinity, or in a cross
    sum that overflowed -- is compared by its position, its sign differs between machines)."""
    rows, boxes = sr.build_rows(box_set, nbins)
    lo, hi = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    d = on_device(rows)
    s = sampler300
    s.joint_begin(lo, hi, chains=HAND_CHAINS, nbins=nbins)
    for first, n, skip, thin in sr.CALLS:
        s.joint_accumulate(d[first:].data_ptr(), n, skip, thin)
    got = s.joint()
    s.joint_end()
    ref = RefJoint(rows[sr.kept_steps()], boxes, HAND_CHAINS, nbins)
    assert_equals(got, ref, finite_chains=(1, 2, 3), what="%s/%d" % (box_set, nbins))
    assert int(ref.counts.sum()) > 0 and int(ref.counts[:, :, nbins - 1, :].sum()) > 0 and int(ref.counts[:, :, :, nbins - 1].sum()) > 0


# ---- every cell of every band -----------------------------------------------------------------------------------
@pytest.mark.parametrize("nbins", [200, 512])
def test_every_cell_of_every_band(nbins):
    """one pair on a ladder of one chain: cell (a, b) receives 1 + (a nbins + b) mod 5 samples at its centre, in
    shuffled order, so that a band or a row stride that is one off cannot pass; at 512 the 786 432 rows are three
    staged pieces of 2^18, each exactly full (a ragged last piece: test_many_kept_chains_and_a_ragged_last_piece).  The
    moments against numpy's cumulative sums, which add in sample order."""
    w = wl.simplesin(n_data=16, n_chain=1)
    lo, hi = np.array([0.0, -3.0, 10.0, -1.0]), np.array([1.0, 5.0, 11.0, 1.0])
    jt0 = Joint.empty(1, 4, nbins, [(1, 3)], lo, hi)
    ex, ey = jt0.edges(1), jt0.edges(3)
    want = (1 + (np.arange(nbins)[:, None] * nbins + np.arange(nbins)[None, :]) % 5).astype(np.uint64)
    a, b = np.divmod(np.repeat(np.arange(nbins * nbins), want.ravel().astype(np.int64)), nbins)
    order = np.random.default_rng(nbins).permutation(len(a))
    a, b = a[order], b[order]
    rows = np.zeros((len(a), 1, 6))
    rows[:, 0, 0] = 0.5
    rows[:, 0, 1] = (ex[a] + ex[a + 1]) / 2
    rows[:, 0, 2] = 10.5
    rows[:, 0, 3] = (ey[b] + ey[b + 1]) / 2
    s = HipSampler(w.model, w.n_par, 1, w.data, seed=1)
    d = on_device(rows)
    s.joint_begin(lo, hi, chains=(0,), nbins=nbins, pairs=[(1, 3)])
    s.joint_accumulate(d.data_ptr(), len(rows))
    got = s.joint()
    s.close()
    assert int(got.n[0]) == len(rows) == int(want.sum())
    bad = np.argwhere(got.counts[0, 0] != want)
    assert len(bad) == 0, "first of %d differing cells: %s holds %d, expected %d" % (
        len(bad), tuple(bad[0]), got.counts[0, 0][tuple(bad[0])], want[tuple(bad[0])])
    dv = [rows[:, 0, p] - rows[0, 0, p] for p in range(4)]
    assert got.origin[0].tobytes() == rows[0, 0, :4].tobytes()
    for p in range(4):
        assert got.sum[0, p] == np.cumsum(dv[p])[-1], p
        for r in range(p, 4):
            assert got.cross[0, tri_index(4, p, r)] == np.cumsum(dv[p] * dv[r])[-1], (p, r)


def test_many_kept_chains_and_a_ragged_last_piece():
    """2048 kept chains of 4 parameters bring the staged piece down to 2^22 / 8192 = 512 kept steps: 700 kept steps are
    one full piece and a ragged one of 188, and the moments kernel runs 2048 x 14 entries over many workgroups.  Counts
    against np.searchsorted over GSL's edges, the moments against numpy's cumulative sums, which add in sample order."""
    from tests.joint_ref import bin_indices
    n_chains, n_steps, nbins = 2048, 701, 8
    w = wl.simplesin(n_data=16, n_chain=n_chains)
    lo, hi = np.array([0.0, -3.0, 10.0, -1.0]), np.array([1.0, 5.0, 11.0, 1.0])
    rng = np.random.default_rng(7)
    rows = np.zeros((n_steps, n_chains, 6))
    rows[:, :, :4] = lo + (hi - lo) * rng.uniform(-0.05, 1.05, (n_steps, n_chains, 4))    # a tenth lies outside
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    d = on_device(rows)
    s.joint_begin(lo, hi, chains=range(n_chains), nbins=nbins, pairs=[(0, 3), (1, 2)])
    s.joint_accumulate(d.data_ptr(), n_steps, 1, 1)          # 700 kept steps
    got = s.joint()
    s.close()
    kept = rows[1:]
    assert int(got.n[0]) == 700
    b = [bin_indices(kept[:, :, p].ravel(), sr.gsl_edges(lo[p], hi[p], nbins)).reshape(700, n_chains) for p in range(4)]
    chain = np.broadcast_to(np.arange(n_chains), (700, n_chains))
    for q, (i, j) in enumerate([(0, 3), (1, 2)]):
        ok = (b[i] >= 0) & (b[j] >= 0)
        want = np.zeros((n_chains, nbins, nbins), dtype=np.uint64)
        np.add.at(want, (chain[ok], b[i][ok], b[j][ok]), 1)
        assert np.array_equal(got.counts[:, q], want), q
        assert 0 < int(want.sum()) < 700 * n_chains
    dv = kept[:, :, :4] - kept[0, :, :4]
    assert got.origin.tobytes() == np.ascontiguousarray(kept[0, :, :4]).tobytes()
    assert got.sum.tobytes() == np.ascontiguousarray(np.cumsum(dv, axis=0)[-1]).tobytes()
    for i in range(4):
        for j in range(i, 4):
            want = np.cumsum(dv[:, :, i] * dv[:, :, j], axis=0)[-1]
            assert got.cross[:, tri_index(4, i, j)].tobytes() == want.tobytes(), (i, j)


# ---- call boundaries and thinning ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["simplesin16", "pulse16"])
def test_call_boundaries_and_thinning(case):
    w, s, d, _ = _run(case)
    n_steps = d.shape[0]
    rows = d.cpu().numpy()
    bs = 5

    def joint_of(pieces, skip=0, thin=1):
        s.joint_begin(w.pmin, w.pmax, chains=(0, 2, 15), nbins=200)
        off = 0
        for n in pieces:
            s.joint_accumulate(d[off:].data_ptr(), n, skip, thin)
            off += n
        return s.joint()

    one = joint_of([n_steps])
    same_joint(one, Joint.from_rows(rows, w.pmin, w.pmax, chains=(0, 2, 15), nbins=200))
    for pieces in ([1, 13, 50, n_steps - 64], [4, 4, 4, 4, n_steps - 16], [bs - 1, bs, bs + 1, n_steps - 3 * bs]):
        same_joint(joint_of(pieces), one)
    for skip, thin in ((0, 3), (2, 3), (6, 7)):
        got = joint_of([n_steps], skip, thin)
        assert int(got.n[0]) == len(rows[skip::thin])
        same_joint(got, Joint.from_rows(rows[skip::thin], w.pmin, w.pmax, chains=(0, 2, 15), nbins=200))
    s.close()


# ---- a real run closes on the summary ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["simplesin16", "pulse16"])
def test_a_real_run_closes_on_the_summary(case):
    w, s, d, _ = _run(case)
    n_steps = d.shape[0]
    s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=7, max_batches=batches_closed(n_steps, 7))
    s.joint_begin(w.pmin, w.pmax, chains=(0,), nbins=200)
    half = n_steps // 2
    for first, n in ((0, half), (half, n_steps - half)):
        s.summary_accumulate(d[first:].data_ptr(), n)
        s.joint_accumulate(d[first:].data_ptr(), n)
    rs, jt = s.summary(), s.joint()
    s.close()
    assert int(jt.n[0]) == rs.n == n_steps and len(jt.pairs) == w.n_par * (w.n_par - 1) // 2
    for q, (i, j) in enumerate(jt.pairs.tolist()):
        assert np.array_equal(jt.marginal(0, q, 0), rs.hist[0, i]), (i, j)
        assert np.array_equal(jt.marginal(0, q, 1), rs.hist[0, j]), (i, j)
        assert int(jt.counts[0, q].sum()) == n_steps
    same_joint(jt, Joint.from_rows(d.cpu().numpy(), w.pmin, w.pmax, chains=(0,), nbins=200))
    assert np.isfinite(jt.cov(0)).all()


def test_joint_does_not_change_the_chains():
    w = wl.pulse(n_data=257, n_chain=16)
    st, _, _ = make_pair(w, 16, seed=3)
    out = []
    for with_joint in (False, True):
        s = HipSampler(w.model, w.n_par, 16, w.data, seed=3)
        s.set_state(st)
        d = torch.zeros((2, 60, 16, w.n_par + 2), dtype=torch.float64, device="cuda")
        if with_joint:
            s.joint_begin(w.pmin, w.pmax, chains=(0, 7), nbins=200)
        for k in range(4):
            buf = d[k % 2]
            s.run_sampler(20, 3, buf.data_ptr())
            if with_joint:
                s.joint_accumulate(buf.data_ptr(), 60)
                capi.check(s.L.apemost_hip_samples_wait(s._h))    # before the buffer is written again
        s.synchronize()
        out.append((s.get_state(), d.cpu().numpy()))
        if with_joint:
            assert int(s.joint().n[0]) == 240
        s.close()
    for f in ("params", "params_best", "prob", "prior", "prob_best", "accept", "reject", "n_iter", "swapcount", "ticks",
              "step", "params_accepts", "params_rejects", "beta"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()


# ---- pair lists ---------------------------------------------------------------------------------------------------
def test_pair_lists():
    w, s, d, _ = _run("simplesin16")
    n_steps = d.shape[0]

    def joint_of(pairs):
        s.joint_begin(w.pmin, w.pmax, chains=(0, 3), nbins=64, pairs=pairs)
        s.joint_accumulate(d.data_ptr(), n_steps)
        return s.joint()

    full = joint_of(None)
    assert full.pairs.tolist() == [list(p) for p in all_pairs(4)]
    some = joint_of([(1, 3), (0, 2)])
    assert some.counts.shape == (2, 2, 64, 64)
    assert np.array_equal(some.counts[:, 0], full.counts[:, full.pair_index(1, 3)])
    assert np.array_equal(some.counts[:, 1], full.counts[:, full.pair_index(0, 2)])
    none = joint_of([])
    assert none.counts.shape == (2, 0, 64, 64) and int(none.n[0]) == n_steps
    for jt in (some, none):
        for f in ("origin", "sum", "cross"):
            assert getattr(jt, f).tobytes() == getattr(full, f).tobytes(), f
    s.close()


# ---- a ladder batch -------------------------------------------------------------------------------------------------
def test_a_batch_of_three_ladders():
    from tests.test_gpu_ladder_batch import concat, ladders, make_batch, N_ROUNDS, N_SWAP, PER
    ws, seeds, sts, _, _ = ladders("simplesin", 3)
    w = ws[0]
    n_steps = N_ROUNDS * N_SWAP
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    d = torch.zeros((n_steps, 3 * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    chains = [0, PER, 2 * PER]
    batch.joint_begin(w.pmin, w.pmax, chains=chains, nbins=200)
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.joint_accumulate(d.data_ptr(), n_steps)
    got = batch.joint()
    batch.close()
    rows = d.cpu().numpy()
    boxes = list(zip(w.pmin.tolist(), w.pmax.tolist()))
    assert_equals(got, RefJoint(rows, boxes, chains, 200), finite_chains=(0, 1, 2))
    for b in range(3):                                       # each ladder alone: the recount of its own rows
        alone = RefJoint(rows[:, b * PER:(b + 1) * PER], boxes, [0], 200)
        assert np.array_equal(got.counts[b], alone.counts[0]) and got.cross[b].tobytes() == alone.cross[0].tobytes()
    assert not np.array_equal(got.counts[0], got.counts[1])


# ---- joint_set: a resumed run -----------------------------------------------------------------------------------------
def test_set_resumes_an_accumulation():
    w, s, d, _ = _run("pulse16")
    n_steps = d.shape[0]
    cut = 101
    s.joint_begin(w.pmin, w.pmax, chains=(0, 5), nbins=200)
    s.joint_accumulate(d.data_ptr(), n_steps)
    whole = s.joint()
    s.joint_begin(w.pmin, w.pmax, chains=(0, 5), nbins=200)
    s.joint_accumulate(d.data_ptr(), cut)
    part = s.joint()
    s.joint_end()
    assert int(part.n[0]) == cut
    s.joint_begin(w.pmin, w.pmax, chains=(0, 5), nbins=200)
    s.joint_set(part)
    s.joint_accumulate(d[cut:].data_ptr(), n_steps - cut)
    same_joint(s.joint(), whole)
    assert whole.origin.tobytes() == d[0, [0, 5], :w.n_par].cpu().numpy().tobytes()
    s.close()


# ---- invalid arguments --------------------------------------------------------------------------------------------------
def test_invalid_arguments():
    n_chains = 96
    w = wl.simplesin(n_data=64, n_chain=n_chains)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    st, _, _ = make_pair(w, n_chains, seed=1)
    s.set_state(st)
    L = capi.lib()
    d = torch.zeros((12, n_chains, w.n_par + 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    jt = Joint.empty(1, 4, 10, all_pairs(4), w.pmin, w.pmax)
    # accumulate, get and set without begin
    assert L.apemost_hip_joint_accumulate(s._h, d.data_ptr(), 12, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_joint_get(s._h, C.byref(jt.view())) == capi.ERR_INVALID
    assert L.apemost_hip_joint_set(s._h, C.byref(jt.view())) == capi.ERR_INVALID
    assert L.apemost_hip_joint_begin(s._h, None) == capi.ERR_INVALID
    lo, hi = np.array(w.pmin, dtype=np.float64), np.array(w.pmax, dtype=np.float64)
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def begin(chains=(0,), nbins=10, pairs=None, lo_=lo, hi_=hi):
        ch = np.array(chains, dtype=np.int32)
        pr = None if pairs is None else np.array(pairs, dtype=np.int32).reshape(-1, 2)
        cfg = capi.JointConfig(n_keep=len(ch), chains=ch.ctypes.data_as(ip) if len(ch) else None, nbins=nbins,
                               n_pairs=0 if pr is None else len(pr), pairs=None if pr is None else pr.ctypes.data_as(ip),
                               lo=None if lo_ is None else lo_.ctypes.data_as(dp), hi=None if hi_ is None else hi_.ctypes.data_as(dp))
        return L.apemost_hip_joint_begin(s._h, C.byref(cfg))
    bad_hi, inf_lo, nan_hi = hi.copy(), lo.copy(), hi.copy()
    bad_hi[2], inf_lo[0], nan_hi[1] = lo[2], -np.inf, np.nan
    wide_lo, wide_hi = lo.copy(), hi.copy()
    wide_lo[3], wide_hi[3] = -1e308, 1e308                   # both finite, hi - lo is not
    for kw in (dict(chains=()), dict(chains=(0, 0)), dict(chains=(2, 1)), dict(chains=(n_chains,)), dict(chains=(-1,)),
               dict(chains=tuple(range(n_chains + 1))), dict(nbins=0), dict(nbins=513), dict(nbins=-1),
               dict(pairs=[(1, 1)]), dict(pairs=[(2, 1)]), dict(pairs=[(0, 4)]), dict(pairs=[(-1, 2)]),
               dict(pairs=[(0, 1), (2, 3), (0, 1)]),
               dict(hi_=bad_hi), dict(lo_=inf_lo), dict(hi_=nan_hi), dict(lo_=wide_lo, hi_=wide_hi), dict(lo_=None),
               dict(chains=tuple(range(86)), nbins=512)):    # 86 x 6 x 512^2 x 8 bytes = 2^30 + 8 MiB
        assert begin(**kw) == capi.ERR_INVALID, kw
        assert L.apemost_hip_joint_get(s._h, C.byref(jt.view())) == capi.ERR_INVALID, kw    # nothing was begun
    assert begin(chains=(0, 1, 2), nbins=512, pairs=[(0, 1), (2, 3)]) == capi.OK
    assert begin(nbins=512) == capi.OK and begin(nbins=1) == capi.OK and begin(pairs=[]) == capi.OK
    assert begin() == capi.OK
    assert L.apemost_hip_joint_accumulate(s._h, d.data_ptr(), 12, 0, 0) == capi.ERR_INVALID      # thin 0
    assert L.apemost_hip_joint_accumulate(s._h, None, 12, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_joint_get(s._h, None) == capi.ERR_INVALID
    assert L.apemost_hip_joint_accumulate(s._h, d.data_ptr(), 12, 12, 1) == capi.OK               # keeps nothing
    assert L.apemost_hip_joint_accumulate(s._h, d.data_ptr(), 12, 2, 3) == capi.OK
    assert L.apemost_hip_joint_get(s._h, C.byref(jt.view())) == capi.OK and int(jt.n[0]) == 4
    assert not jt.sum.any() and not jt.origin.any()          # (rows of zeros)
    # a begin that is refused leaves the joint begun before open, as it was
    assert begin(nbins=0) == capi.ERR_INVALID and begin(pairs=[(1, 0)]) == capi.ERR_INVALID
    assert L.apemost_hip_joint_accumulate(s._h, d.data_ptr(), 12, 0, 4) == capi.OK
    assert L.apemost_hip_joint_get(s._h, C.byref(jt.view())) == capi.OK and int(jt.n[0]) == 7
    s.joint_end()
    assert L.apemost_hip_joint_get(s._h, C.byref(jt.view())) == capi.ERR_INVALID
    # the sampler still steps
    before = s.get_state()
    s.run_sampler(3, 5, d.data_ptr())
    s.synchronize()
    after = s.get_state()
    assert np.array_equal(after.n_iter, before.n_iter + 15)
    s.close()


# ---- the C host: APEMOST_DUMP=summary,joint -----------------------------------------------------------------------------
def test_c_host_joint_token(tmp_path):
    n_beta, iters = 8, 6000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    work = tmp_path / "summary_joint"
    work.mkdir()
    (work / "params").write_text(w.params_file_text())
    (work / "data").write_text(w.data_file_text())
    env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP="summary,joint")
    for phase in ("calibrate_first", "calibrate_rest", "run"):
        subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    assert not [f for f in os.listdir(str(work)) if f.endswith(".prob.dump") or f.startswith("prob-chain") or f == "samples.bin"]

    def check(n):
        jt, rs = Joint.read(str(work / "joint.bin")), RunSummary.read(str(work / "summary.bin"))
        assert int(jt.n[0]) == rs.n == n and jt.nbins == 200 and jt.n_keep == 1 and jt.chains.tolist() == [0]
        assert jt.pairs.tolist() == [list(p) for p in all_pairs(w.n_par)]
        assert jt.lo.tobytes() == rs.lo.tobytes() and jt.hi.tobytes() == rs.hi.tobytes()
        for q, (i, j) in enumerate(jt.pairs.tolist()):
            assert np.array_equal(jt.marginal(0, q, 0), rs.hist[0, i]), (i, j)
            assert np.array_equal(jt.marginal(0, q, 1), rs.hist[0, j]), (i, j)
        out = tmp_path / ("text_%d" % n)
        out.mkdir()
        jt.write_text(out, w.names)
        names = sorted(os.listdir(str(out)))
        assert len(names) == len(jt.pairs) + 1
        for f in names:
            assert (work / f).read_bytes() == (out / f).read_bytes(), f
        assert np.isfinite(jt.corr(0)).all()
        return jt
    first = check(iters)
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = check(2 * iters)
    assert second.origin.tobytes() == first.origin.tobytes()
    assert int(second.counts.sum()) == 2 * int(first.counts.sum())
