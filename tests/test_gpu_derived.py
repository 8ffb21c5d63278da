"""On-device derived quantities (apemost_hip_derived_*, pt_derived.h): derived_eval gives numpy's bits for programs of
the exact group and the device library's functions within their measured error; the fold equals tests/derived_ref.py
-- a restatement that shares nothing with the kernels -- with == on hand-built rows, over piece and call boundaries,
at the limits of the specification, on real runs (where identity columns close on the run summary and the joint
fold), on a ladder batch and through derived_set; it leaves the chains alone and refuses what the header says; the C host's APEMOST_DUMP=derived writes the Python fold
of the same run's binary dump."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from apemost_amd import capi, derived as dv, workloads as wl
from apemost_amd.joint import tri_index
from apemost_amd.sampler import HipSampler
from apemost_amd.summary import RunSummary, batches_closed
from tests import derived_ref as ref, hostlib, summary_rows as sr
from tests.derived_ref import CHAINS, COLUMNS, EXTRA_BOXES, PAIRS, assert_equals_ref, special_rows
from tests.helpers import make_pair
from tests.joint_ref import bin_indices, same_floats
from tests.test_gpu_summary import _run

pytestmark = pytest.mark.gpu
NAMES = ["p0", "p1", "p2", "p3"]
FIELDS = ("hist", "batch", "nonfinite", "vmin", "vmax", "origin", "sum", "cross", "counts")


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def same_derived(a, b, what=""):
    """two Derived objects, every field with == (the sums bit for bit, a NaN by its position)"""
    assert int(a.n[0]) == int(b.n[0]) and a.pairs.tolist() == b.pairs.tolist(), what
    for f in FIELDS:
        x, y = np.asarray(getattr(a, f)), np.asarray(getattr(b, f))
        assert x.shape == y.shape, (what, f)
        assert (np.array_equal(x, y) if x.dtype == np.uint64 else same_floats(x, y)), (what, f)


@pytest.fixture(scope="module")
def small():
    """simplesin, 3 chains, 16 data points: the sampler of the tests that fold synthetic rows"""
    w = wl.simplesin(n_data=16, n_chain=3)
    s = HipSampler(w.model, w.n_par, 3, w.data, seed=1)
    yield s
    s.close()


@pytest.fixture(scope="module")
def sampler300():
    w = wl.simplesin(n_data=16, n_chain=300)
    s = HipSampler(w.model, w.n_par, 300, w.data, seed=1)
    yield s
    s.close()


# ---- 1. derived_eval, the exact group ---------------------------------------------------------------------------------------
def test_eval_of_the_exact_group_gives_numpys_bits(small):
    """64 generated programs -- every opcode of the group, one of depth 16, one of 256 instructions -- on 512 rows with
    subnormals, both zeros, infinities and NaNs: the device's bits are numpy's and the restatement's, a NaN by its
    position"""
    progs = ref.random_programs(29, 64, 4)
    programs = [dv.Program(code, consts) for code, consts in progs]
    assert ref.depth_of(progs[0][0]) == 16 and len(progs[1][0]) == 256 and all(p.uses_only_exact() for p in programs)
    rows = special_rows(512, seed=9)
    small.derived_begin(programs, [-1.0] * 64, [1.0] * 64, pairs=[], nbins=4)
    got = small.derived_eval(rows)
    small.derived_end()
    want = dv.eval_numpy(programs, rows)
    for c in range(64):
        bad = np.flatnonzero(~((got[:, c].view(np.uint64) == want[:, c].view(np.uint64)) | (np.isnan(got[:, c]) & np.isnan(want[:, c]))))
        assert len(bad) == 0, (c, programs[c].rpn(NAMES), rows[bad[0]], got[bad[0], c], want[bad[0], c])
    assert same_floats(got[:64], ref.values(progs, rows[:64]))
    assert 0.2 < np.isfinite(want).mean() < 1.0


# ---- 2. derived_eval, the library group -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["log", "exp", "sin", "cos", "atan2"])
def test_eval_of_the_library_group_within_its_measured_error(small, name):
    """each function over its fixed argument list (tests/derived_ref.library_arguments) against mpmath at 300 bits;
    the bound is the largest error measured on the card, rounded up to the next integer, plus one ulp"""
    args = ref.library_arguments()[name]
    rows = np.zeros((len(args[0]), 6))
    for i, a in enumerate(args):
        rows[:, i] = a
    small.derived_begin([dv.parse_rpn("p0 p1 atan2" if name == "atan2" else "p0 " + name, NAMES)], [-1.0], [1.0], nbins=4)
    got = small.derived_eval(rows)[:, 0]
    small.derived_end()
    err = ref.ulp_errors(name, args, got)
    worst = int(np.argmax(err))
    print("%s: largest error %.4f ulp at %r -> %r" % (name, err[worst], [a[worst] for a in args], got[worst]))
    assert ref.LIBRARY_BOUND_ULP == dict(log=2, exp=2, sin=2, cos=2, atan2=3)
    assert err[worst] <= ref.LIBRARY_BOUND_ULP[name], (name, err[worst])


# ---- 3. hand-built rows against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize("box_set", ["A", "B"])
@pytest.mark.parametrize("nbins", [1, 37, 512])
def test_fold_of_hand_built_rows(sampler300, box_set, nbins):
    """the rows of the summary's and the joint fold's tests, kept chains 0, 1, 2 and 299, the three calls of
    summary_rows.CALLS; the four identities and p1 - p0, p3 / p1, sqrt(abs(p0 p3)), min(p0, p1).  Everything equals the
    restatement; the identity columns equal what joint_* and summary_* return on the same rows.  p3 / p1 divides by the
    zeros of p1's pool, so every chain holds non-finite values: all sums are compared with a NaN by its position."""
    bs = 50
    rows, boxes = sr.build_rows(box_set, nbins)
    boxes = list(boxes) + EXTRA_BOXES[box_set]
    lo, hi = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    kept = rows[sr.kept_steps()]
    most = batches_closed(len(kept), bs)
    d = on_device(rows)
    s = sampler300
    s.derived_begin(COLUMNS, lo, hi, chains=CHAINS, nbins=nbins, pairs=PAIRS, batch_size=bs, max_batches=most)
    s.joint_begin(lo[:4], hi[:4], chains=CHAINS, nbins=nbins, pairs=[(0, 1), (2, 3)])
    s.summary_begin(lo[:4], hi[:4], n_hist_chains=3, nbins=nbins, batch_size=bs, max_batches=most)
    for first, n, skip, thin in sr.CALLS:
        for fold in ("derived", "joint", "summary"):
            getattr(s, fold + "_accumulate")(d[first:].data_ptr(), n, skip, thin)
    got, jt, rs = s.derived(), s.joint(), s.summary()
    on_card = np.stack([s.derived_eval(kept[:, ch]) for ch in CHAINS], axis=1)
    for fold in ("derived", "joint", "summary"):
        getattr(s, fold + "_end")()
    programs = [(p.code, p.consts) for p in got.programs]
    vals = np.zeros((len(kept), 300, len(COLUMNS)))
    for k, ch in enumerate(CHAINS):
        vals[:, ch] = ref.values(programs, kept[:, ch])
        assert same_floats(on_card[:, k], vals[:, ch]), ch            # derived_eval fixes the fold's meaning
    want = ref.RefDerived(vals, boxes, CHAINS, nbins, bs, PAIRS)
    assert_equals_ref(got, want, what="%s/%d" % (box_set, nbins))
    assert np.array_equal(got.nonfinite, (~np.isfinite(vals[:, CHAINS])).sum(axis=0)) and int(got.nonfinite.sum()) > 0
    assert int(got.hist[:, 4:].sum()) > 0 and int(got.counts[:, 2:].sum()) > 0
    # identity columns: the joint fold's and the run summary's
    assert np.array_equal(jt.counts, got.counts[:, :2])
    assert same_floats(jt.origin, got.origin[:, :4]) and same_floats(jt.sum, got.sum[:, :4])
    for i in range(4):
        for j in range(i, 4):
            assert same_floats(jt.cross[:, tri_index(4, i, j)], got.cross[:, tri_index(8, i, j)]), (i, j)
    assert np.array_equal(rs.hist, got.hist[:3, :4]) and same_floats(rs.batch_sums, got.batch[:3, :4])
    assert rs.n_batches == got.n_batches == most


# ---- 4. piece and call boundaries ----------------------------------------------------------------------------------------
N_KEPT = 3 * 64 + 17


@pytest.fixture(scope="module")
def boundary_rows():
    rng = np.random.default_rng(64)
    rows = np.zeros((3 + 7 * N_KEPT, 3, 6))
    rows[:, :, :4] = rng.normal(0.0, 2.0, rows[:, :, :4].shape)
    rows[:, :, 4:] = rng.normal(-20.0, 3.0, rows[:, :, 4:].shape)
    rows[5::97, 1, 1] = 0.0                                              # p3 / p1: infinities in chain 1
    return rows, on_device(rows)


BOUNDARY_COLUMNS = COLUMNS + ["like / 0.5", "floor(prob) + max(p2, p3)"]
BOUNDARY_LO, BOUNDARY_HI = [-6.0] * 8 + [-80.0, -40.0], [6.0] * 8 + [0.0, 0.0]


@pytest.mark.parametrize("thin,skip", [(1, 0), (7, 3)])
@pytest.mark.parametrize("bs,stage", [(1, 64), (2, 64), (50, 64), (50, 7)])
def test_piece_and_call_boundaries(small, boundary_rows, thin, skip, bs, stage):
    """3 * 64 + 17 kept steps: staged in pieces of 64 (or 7) and cut into calls after 1, 63, 64 and 65 kept steps, the
    fold has the bits of one call with the default staging, and of the host fold over what derived_eval returns.  A
    batch of 2 closes on sample 63 and 65, a batch of 50 on sample 49: ends of staged pieces."""
    rows, d = boundary_rows
    s = small
    kept = rows[skip::thin][:N_KEPT]
    kw = dict(chains=(0, 1, 2), nbins=37, pairs=[(0, 1), (4, 5), (5, 9)], batch_size=bs, max_batches=batches_closed(N_KEPT, bs))

    def fold(stage_steps, cuts):
        s.derived_begin(BOUNDARY_COLUMNS, BOUNDARY_LO, BOUNDARY_HI, stage_steps=stage_steps, **kw)
        for a, b in zip([0] + cuts, cuts + [N_KEPT]):
            first = skip + a * thin                                      # the call keeps the steps a .. b - 1
            s.derived_accumulate(d[first:].data_ptr(), (b - a - 1) * thin + 1, 0, thin)
        return s.derived()

    one = fold(0, [])
    assert int(one.n[0]) == N_KEPT
    if thin > 1:                                                         # ... and with the call's own skip
        s.derived_begin(BOUNDARY_COLUMNS, BOUNDARY_LO, BOUNDARY_HI, **kw)
        s.derived_accumulate(d.data_ptr(), skip + (N_KEPT - 1) * thin + 1, skip, thin)
        same_derived(s.derived(), one, "skip")
    same_derived(fold(stage, []), one, "pieces")
    same_derived(fold(stage, [1, 63, 64, 65]), one, "calls")
    same_derived(fold(0, [1, 63, 64, 65]), one, "calls, default staging")
    vals = np.stack([s.derived_eval(kept[:, ch]) for ch in range(3)], axis=1)
    host = dv.Derived.from_rows(kept, one.programs, BOUNDARY_LO, BOUNDARY_HI, values=vals, **kw)
    s.derived_end()
    same_derived(one, host, "host fold")
    assert one.n_batches == batches_closed(N_KEPT, bs) and int(one.nonfinite[1, 5]) > 0
    assert same_floats(vals[:, :, :8], dv.eval_numpy(one.programs[:8], kept.reshape(-1, 6)).reshape(N_KEPT, 3, 8))


# ---- 5. the limits at once -------------------------------------------------------------------------------------------------
def test_limits_at_once():
    """64 columns x 4 kept chains, column 0 of depth 16 and column 1 of 256 instructions: the default staging is
    2^22 / 256 = 16384 kept steps, and 16384 + 1000 are one full piece and a ragged one.  Counts against
    np.searchsorted over GSL's edges, the sums against numpy's cumulative sums, which add in sample order."""
    n_chains, n, nbins, bs = 4, 16384 + 1000, 16, 1000
    progs = ref.random_programs(31, 64, 4)
    programs = [dv.Program(code, consts) for code, consts in progs]
    assert dv.check(programs, 4)[0] == 16 and len(programs[1].code) == 256
    w = wl.simplesin(n_data=16, n_chain=n_chains)
    rng = np.random.default_rng(5)
    rows = rng.normal(0.0, 1.5, (n, n_chains, 6))
    pairs = [(0, 1), (2, 63), (62, 63)]
    lo, hi = np.full(64, -4.0), np.full(64, 4.0)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    d = on_device(rows)
    s.derived_begin(programs, lo, hi, chains=range(n_chains), nbins=nbins, pairs=pairs, batch_size=bs,
                    max_batches=batches_closed(n, bs))
    s.derived_accumulate(d.data_ptr(), n)
    got = s.derived()
    on_card = s.derived_eval(rows.reshape(-1, 6)[:4096])
    s.close()
    vals = dv.eval_numpy(programs, rows.reshape(-1, 6)).reshape(n, n_chains, 64)
    assert same_floats(on_card, vals.reshape(-1, 64)[:4096])
    assert int(got.n[0]) == n and got.n_batches == batches_closed(n, bs) == 17
    with np.errstate(all="ignore"):
        e = sr.gsl_edges(-4.0, 4.0, nbins)
        b = bin_indices(vals.ravel(), e).reshape(vals.shape)
        for k in range(n_chains):
            for c in range(64):
                v = vals[:, k, c]
                assert np.array_equal(got.hist[k, c], np.bincount(b[:, k, c][b[:, k, c] >= 0], minlength=nbins)), (k, c)
                assert int(got.nonfinite[k, c]) == int((~np.isfinite(v)).sum()), (k, c)
                ok = v[~np.isnan(v)]
                if len(ok):
                    assert got.vmin[k, c] == ok.min() and got.vmax[k, c] == ok.max(), (k, c)
                closes = [bs - 1 + bs * i for i in range(17)]            # sample counts that close a batch
                sums = [np.cumsum(part)[-1] for part in np.split(v, closes)]
                assert same_floats(got.batch[k, c], np.array(sums)), (k, c)
        dvs = vals - vals[0]
        assert same_floats(got.origin, vals[0]) and same_floats(got.sum, np.cumsum(dvs, axis=0)[-1])
        for i, j in ((0, 0), (0, 1), (1, 63), (17, 40), (63, 63)):
            assert same_floats(got.cross[:, tri_index(64, i, j)], np.cumsum(dvs[:, :, i] * dvs[:, :, j], axis=0)[-1]), (i, j)
    chain = np.broadcast_to(np.arange(n_chains)[None, :], (n, n_chains))
    for q, (i, j) in enumerate(pairs):
        ok = (b[:, :, i] >= 0) & (b[:, :, j] >= 0)
        want = np.zeros((n_chains, nbins, nbins), dtype=np.uint64)
        np.add.at(want, (chain[ok], b[:, :, i][ok], b[:, :, j][ok]), 1)
        assert np.array_equal(got.counts[:, q], want), q
    assert int(got.hist.sum()) > 0 and int(got.counts.sum()) > 0


# ---- 6. a real run closes on the summary and the evidence fold -------------------------------------------------------------
@pytest.mark.parametrize("case", ["simplesin16", "pulse16"])
def test_a_real_run_closes_on_the_summary_and_the_evidence(case):
    w, s, d, _ = _run(case)
    n_steps, bs = d.shape[0], 7
    most = batches_closed(n_steps, bs)
    beta0 = float(s.get_state(fields=("beta",)).beta[0])
    names = ["p%d" % i for i in range(w.n_par)]
    columns = names + [("loglike", "like / %r" % beta0)]
    lo, hi = list(w.pmin) + [-1e7], list(w.pmax) + [0.0]
    s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=bs, max_batches=most)
    s.evidence_begin(batch_size=bs, max_batches=most)
    s.derived_begin(columns, lo, hi, chains=(0,), nbins=200, batch_size=bs, max_batches=most)
    half = n_steps // 2
    for first, n in ((0, half), (half, n_steps - half)):
        for fold in ("summary", "evidence", "derived"):
            getattr(s, fold + "_accumulate")(d[first:].data_ptr(), n)
    rs, ev, got = s.summary(), s.evidence(), s.derived()
    s.close()
    assert int(got.n[0]) == rs.n == n_steps and got.names[-1] == "loglike"
    assert np.array_equal(got.hist[0, :w.n_par], rs.hist[0]) and int(got.hist[0, :w.n_par].sum()) == n_steps * w.n_par
    assert got.batch[0, :w.n_par].tobytes() == rs.batch_sums[0].tobytes() and got.n_batches == rs.n_batches
    assert int(got.nonfinite.sum()) == 0
    rows = d.cpu().numpy()
    assert got.vmin[0, :w.n_par].tolist() == rows[:, 0, :w.n_par].min(axis=0).tolist()
    assert got.vmax[0, :w.n_par].tolist() == rows[:, 0, :w.n_par].max(axis=0).tolist()
    # (prob - prior) / beta_0: the mean the evidence fold's moments of chain 0 give; the same bits where beta_0 is 1
    mean = float(got.mean(0)[w.n_par])
    if beta0 == 1.0:
        assert mean == float(ev.mean_loglike()[0])
    assert mean == pytest.approx(float(ev.mean_loglike()[0]), rel=1e-12)
    same_derived(got, dv.Derived.from_rows(rows, got.programs, lo, hi, chains=(0,), nbins=200, batch_size=bs,
                                           max_batches=most), case)


# ---- 7. a ladder batch -----------------------------------------------------------------------------------------------------
def test_a_batch_of_three_ladders():
    from tests.test_gpu_ladder_batch import concat, ladders, make_batch, N_ROUNDS, N_SWAP, PER
    ws, seeds, sts, _, _ = ladders("simplesin", 3)
    w = ws[0]
    n_steps = N_ROUNDS * N_SWAP
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    d = torch.zeros((n_steps, 3 * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    columns = ["p0", "p1 - p0", "p3 / p1", "sqrt(abs(p0 * p3))"]
    lo, hi = [w.pmin[0], -20.0, -5.0, 0.0], [w.pmax[0], 20.0, 5.0, 10.0]
    kw = dict(nbins=50, batch_size=6, max_batches=batches_closed(n_steps, 6))
    batch.derived_begin(columns, lo, hi, chains=[0, 2 * PER], **kw)
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.derived_accumulate(d.data_ptr(), n_steps)
    got = batch.derived()
    batch.close()
    rows = d.cpu().numpy()
    parts = got.per_ladder(2)
    assert len(parts) == 2 and [p.chains.tolist() for p in parts] == [[0], [2 * PER]]
    for part, b in zip(parts, (0, 2)):                       # each ladder alone: the fold of its own rows
        alone = dv.Derived.from_rows(rows[:, b * PER:(b + 1) * PER], got.programs, lo, hi, chains=(0,), **kw)
        same_derived(part, alone, "ladder %d" % b)
    assert not np.array_equal(parts[0].hist, parts[1].hist)


# ---- 8. derived_set: a resumed run -----------------------------------------------------------------------------------------
def test_set_resumes_an_accumulation():
    w, s, d, _ = _run("pulse16")
    n_steps, cut = d.shape[0], 101
    names = ["p%d" % i for i in range(w.n_par)]
    columns = [names[0], "%s - %s" % (names[1], names[0]), "like / 0.5", "sqrt(abs(%s))" % names[2]]
    lo, hi = [w.pmin[0], -50.0, -1e6, 0.0], [w.pmax[0], 50.0, 0.0, 100.0]
    kw = dict(chains=(0, 5), nbins=200, batch_size=4, max_batches=batches_closed(n_steps, 4))
    s.derived_begin(columns, lo, hi, **kw)
    s.derived_accumulate(d.data_ptr(), n_steps)
    whole = s.derived()
    s.derived_begin(columns, lo, hi, **kw)
    s.derived_accumulate(d.data_ptr(), cut)
    part = s.derived()
    s.derived_end()
    assert int(part.n[0]) == cut and part.n_batches == batches_closed(cut, 4)
    s.derived_begin(columns, lo, hi, **kw)
    s.derived_set(part)
    s.derived_accumulate(d[cut:].data_ptr(), n_steps - cut)
    same_derived(s.derived(), whole)
    assert whole.origin[:, 0].tobytes() == d[0, [0, 5], 0].cpu().numpy().tobytes()
    part.n_batches_[0] = 3                                   # a count of batches that does not follow from n
    part.n[0] = cut
    with pytest.raises(capi.ApemostHipError) as e:
        capi.check(s.L.apemost_hip_derived_set(s._h, C.byref(part.view())))
    assert e.value.code == capi.ERR_INVALID and "derived_set" in str(e.value)
    s.close()


# ---- 9. no effect on the chains ----------------------------------------------------------------------------------------------
def test_derived_does_not_change_the_chains():
    w = wl.pulse(n_data=257, n_chain=16)
    st, _, _ = make_pair(w, 16, seed=3)
    names = ["p%d" % i for i in range(w.n_par)]
    out = []
    for with_fold in (False, True):
        s = HipSampler(w.model, w.n_par, 16, w.data, seed=3)
        s.set_state(st)
        d = torch.zeros((2, 60, 16, w.n_par + 2), dtype=torch.float64, device="cuda")
        if with_fold:
            s.derived_begin([names[0], "%s / %s" % (names[1], names[0]), "exp(like)"], [0.0] * 3, [1.0] * 3, chains=(0, 7),
                            max_batches=240)
        for k in range(4):
            buf = d[k % 2]
            s.run_sampler(20, 3, buf.data_ptr())
            if with_fold:
                s.derived_accumulate(buf.data_ptr(), 60)
                capi.check(s.L.apemost_hip_samples_wait(s._h))    # before the buffer is written again
        s.synchronize()
        out.append((s.get_state(), d.cpu().numpy()))
        if with_fold:
            assert int(s.derived().n[0]) == 240
        s.close()
    for f in ("params", "params_best", "prob", "prior", "prob_best", "accept", "reject", "n_iter", "swapcount", "ticks",
              "step", "params_accepts", "params_rejects", "beta"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()


# ---- 10. invalid arguments -------------------------------------------------------------------------------------------------
def test_invalid_arguments_and_the_shared_wording():
    """every refusal of the specification is APEMOST_HIP_ERR_INVALID with the fold's name in the message, a refused begin
    leaves the open fold accumulating, and the shared checks read as tests/test_gpu_fold_contract.py holds the other
    folds to"""
    n_chains = 3
    w = wl.simplesin(n_data=16, n_chain=n_chains)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    L, h = s.L, s._h
    d = on_device(np.random.default_rng(3).normal(0.0, 1.0, (12, n_chains, 6)))
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    W = ref.word

    def last():
        return L.apemost_hip_last_error().decode()

    def fails(rc, msg=None):
        assert rc == capi.ERR_INVALID
        assert (last() == msg) if msg is not None else ("derived" in last()), last()

    view = capi.DerivedView()
    fails(L.apemost_hip_derived_accumulate(h, d.data_ptr(), 12, 0, 1), "derived_accumulate: no derived_begin")
    fails(L.apemost_hip_derived_get(h, C.byref(view)), "derived_get: no derived_begin")
    fails(L.apemost_hip_derived_set(h, C.byref(view)), "derived_set: no derived_begin")
    fails(L.apemost_hip_derived_begin(h, None), "derived_begin: config is NULL")
    out = np.zeros(12)
    fails(L.apemost_hip_derived_eval(h, 1, d.cpu().numpy().ctypes.data_as(dp), out.ctypes.data_as(dp)),
          "derived_eval: no derived_begin")

    def begin(code=(W(ref.COL, 0),), start=None, consts=(), n_const=None, chains=(0,), nbins=10, pairs=None, lo=(0.0,),
              hi=(1.0,), n_col=None, bs=1, most=100, stage=0):
        code_a = np.array(list(code) or [0], dtype=np.int32)
        start_a = np.array([0, len(code)] if start is None else start, dtype=np.int32)
        n_col = len(start_a) - 1 if n_col is None else n_col
        consts_a = np.array(list(consts) or [0.0])
        ch = np.array(list(chains) or [0], dtype=np.int32)
        pr = None if pairs is None else np.array(list(pairs) or [(0, 0)], dtype=np.int32).reshape(-1, 2)
        lo_a, hi_a = (None if v is None else np.array(v, dtype=np.float64) for v in (lo, hi))
        cfg = capi.DerivedConfig(n_keep=len(chains), chains=ch.ctypes.data_as(ip), n_col=n_col, code=code_a.ctypes.data_as(ip),
                                 start=start_a.ctypes.data_as(ip), n_const=len(consts) if n_const is None else n_const,
                                 consts=consts_a.ctypes.data_as(dp), nbins=nbins, n_pairs=0 if pairs is None else len(pairs),
                                 pairs=None if pr is None else pr.ctypes.data_as(ip),
                                 lo=None if lo_a is None else lo_a.ctypes.data_as(dp),
                                 hi=None if hi_a is None else hi_a.ctypes.data_as(dp), batch_size=bs, max_batches=most,
                                 stage_steps=stage)
        return L.apemost_hip_derived_begin(h, C.byref(cfg))

    two = dict(code=(W(ref.COL, 0), W(ref.COL, 1)), start=[0, 1, 2], lo=(0.0, 0.0), hi=(1.0, 1.0))
    refusals = [
        # section 1: the programs
        dict(code=(W(ref.COL, 0), W(ref.ADD))), dict(code=(W(ref.COL, 0),) * 17 + (W(ref.ADD),) * 16),
        dict(code=(W(ref.COL, 0), W(ref.COL, 0))), dict(code=(W(20),)), dict(code=(W(ref.COL, 6),)),
        dict(code=(W(ref.CONST, 1),), consts=(1.0,)), dict(code=(W(ref.CONST, 0),)), dict(code=(), start=[0, 0]),
        dict(code=(W(ref.COL, 0),) + (W(ref.NEG),) * 256), dict(start=[0], n_col=0, lo=(), hi=()),
        dict(code=(W(ref.COL, 0),) * 65, start=list(range(66)), lo=(0.0,) * 65, hi=(1.0,) * 65),
        dict(n_const=257), dict(n_const=-1), dict(start=[1, 2]),
        # section 2: the fold's configuration
        dict(chains=()), dict(chains=(0, 0)), dict(chains=(2, 1)), dict(chains=(n_chains,)), dict(chains=(-1,)),
        dict(chains=(0, 1, 2, 3)), dict(nbins=0), dict(nbins=513), dict(lo=None), dict(hi=None), dict(lo=(1.0,)),
        dict(lo=(-np.inf,)), dict(hi=(np.nan,)), dict(lo=(-1e308,), hi=(1e308,)), dict(bs=0), dict(most=1 << 41),
        dict(stage=(1 << 18) + 1), dict(two, pairs=[(1, 1)]), dict(two, pairs=[(1, 0)]), dict(two, pairs=[(0, 2)]),
        dict(two, pairs=[(-1, 1)]), dict(two, pairs=[(0, 1), (0, 1)]), dict(pairs=[(0, 1)]),
    ]
    for kw in refusals:
        fails(begin(**kw))
        assert last().startswith("derived_begin: "), (kw, last())
        fails(L.apemost_hip_derived_get(h, C.byref(view)), "derived_get: no derived_begin")     # nothing was begun
    # the shared wording, word for word
    fails(begin(chains=(1, 1)), "derived_begin: chains[1] = 1: local chain indices in [0,3), strictly increasing")
    fails(begin(chains=(0, 1, 2, 3)), "derived_begin: n_keep 4 outside [1,3], or no chains")
    fails(begin(lo=(1.0,)), "derived_begin: parameter 0: range [1, 1] invalid")
    fails(begin(chains=(1, 1), lo=(1.0,)), "derived_begin: chains[1] = 1: local chain indices in [0,3), strictly increasing")
    assert begin(stage=1 << 18) == capi.OK and begin(stage=1, nbins=512) == capi.OK
    assert begin(pairs=[], **two) == capi.OK and begin(pairs=[(0, 1)], **two) == capi.OK
    assert begin(most=2, bs=3) == capi.OK
    fails(L.apemost_hip_derived_accumulate(h, d.data_ptr(), 12, 0, 0), "derived_accumulate: bad arguments")
    fails(L.apemost_hip_derived_accumulate(h, None, 12, 0, 1), "derived_accumulate: bad arguments")
    fails(L.apemost_hip_derived_get(h, None), "derived view is NULL")
    fails(L.apemost_hip_derived_set(h, None), "derived view is NULL")
    fails(L.apemost_hip_derived_eval(h, 0, out.ctypes.data_as(dp), out.ctypes.data_as(dp)))
    fails(L.apemost_hip_derived_eval(h, 2, None, out.ctypes.data_as(dp)))
    # batches of 3 close on samples 2, 5, 8: with room for two, 8 samples are one too many and nothing is accumulated
    fails(L.apemost_hip_derived_accumulate(h, d.data_ptr(), 8, 0, 1))
    n = np.zeros(1, dtype=np.uint64)
    count = capi.DerivedView(n=n.ctypes.data_as(capi._up))
    assert L.apemost_hip_derived_accumulate(h, d.data_ptr(), 12, 12, 1) == capi.OK                 # keeps nothing
    assert L.apemost_hip_derived_accumulate(h, d.data_ptr(), 7, 0, 1) == capi.OK
    assert L.apemost_hip_derived_get(h, C.byref(count)) == capi.OK and int(n[0]) == 7
    # a begin that is refused leaves the fold begun before open and accumulating, as it was
    fails(begin(nbins=0))
    fails(begin(code=(W(ref.ADD),)))
    fails(L.apemost_hip_derived_accumulate(h, d.data_ptr(), 1, 0, 1))                               # (sample 8 closes batch 3)
    assert begin(most=100, bs=3) == capi.OK
    assert L.apemost_hip_derived_accumulate(h, d.data_ptr(), 12, 2, 3) == capi.OK
    fails(begin(stage=1 << 19))
    assert L.apemost_hip_derived_accumulate(h, d.data_ptr(), 12, 0, 4) == capi.OK
    assert L.apemost_hip_derived_get(h, C.byref(count)) == capi.OK and int(n[0]) == 7
    s.derived_end()
    fails(L.apemost_hip_derived_get(h, C.byref(count)), "derived_get: no derived_begin")
    # a second begin starts from nothing; the sampler still steps
    st, _, _ = make_pair(w, n_chains, seed=1)
    s.set_state(st)
    s.derived_begin(["p0", "p1"], [0.0, 0.0], [1.0, 1.0], batch_size=2, max_batches=10)
    s.derived_accumulate(d.data_ptr(), 12)
    s.derived_begin(["p2"], [0.0], [1.0], nbins=5, batch_size=2, max_batches=4)
    fresh = s.derived()
    assert int(fresh.n[0]) == 0 and fresh.hist.shape == (1, 1, 5) and fresh.batch.shape == (1, 1, 5)
    for f in ("hist", "batch", "nonfinite", "origin", "sum", "cross", "counts"):
        assert not np.asarray(getattr(fresh, f)).any(), f
    assert np.all(fresh.vmin == np.inf) and np.all(fresh.vmax == -np.inf)
    before = s.get_state()
    s.run_sampler(3, 5, d.data_ptr())
    s.synchronize()
    assert np.array_equal(s.get_state().n_iter, before.n_iter + 15)
    s.close()          # with the fold still open


# ---- 11. the C host: APEMOST_DUMP=summary,derived ----------------------------------------------------------------------------
def test_c_host_derived_token(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters = 8, 6000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    work = tmp_path / "summary_derived"
    work.mkdir()
    (work / "params").write_text(w.params_file_text())
    (work / "data").write_text(w.data_file_text())
    a, b = w.names[1], w.names[0]
    spec = "# functions of chain 0's parameters\nsplit -100 100 %s %s sub\nloglike -1e6 0 like 1 div   # (prob - prior) / beta\n" % (a, b)
    (work / "derived").write_text(spec)
    env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP="summary,derived,binary")
    for phase in ("calibrate_first", "calibrate_rest", "run"):
        subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)

    def check(n):
        _, params, probs = samples_bin.read(str(work / "samples.bin"))       # [n][1][n_par], [n][n_beta][2]
        rows = np.zeros((n, 1, w.n_par + 2))
        rows[:, 0, :w.n_par] = params[:, 0]
        rows[:, 0, w.n_par:] = probs[:, 0]
        got, rs = dv.Derived.read(str(work / "derived.bin")), RunSummary.read(str(work / "summary.bin"))
        assert int(got.n[0]) == rs.n == n and got.names == ["split", "loglike"] and got.row_names == list(w.names)
        assert got.chains.tolist() == [0] and got.pairs.tolist() == [[0, 1]] and got.nbins == 200
        assert got.programs == [dv.parse_rpn("%s %s sub" % (a, b), w.names), dv.parse_rpn("like 1 div", w.names)]
        host = dv.Derived.from_rows(rows, got.programs, [-100.0, -1e6], [100.0, 0.0], nbins=200, batch_size=got.batch_size,
                                    max_batches=got.max_batches)
        same_derived(got, host, "the C host, %d" % n)
        text = (work / "derived.txt").read_text()
        assert text == got.text() and [line.split("\t")[0] for line in text.splitlines()] == ["split", "loglike"]
        assert all(float(x) == float(x) for line in text.splitlines() for x in line.split("\t")[1:])
        for c, name in enumerate(got.names):
            table = np.loadtxt(str(work / (name + ".histogram")))
            assert table.shape == (200, 3) and table[:, 0].tolist() == [float("%.15e" % v) for v in got.edges(c)[:-1]]
            assert abs(table[:, 2].sum() - (got.hi[c] - got.lo[c]) / 200) < 1e-9 * (got.hi[c] - got.lo[c])
        return got
    first = check(iters)
    assert first.batch_size > 1 and first.n_batches == batches_closed(iters, first.batch_size)
    # --append resumes from the file with its batch size
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = check(2 * iters)
    assert second.origin.tobytes() == first.origin.tobytes() and second.batch_size == first.batch_size
    # a malformed line ends the run before the first launch, with its number; so does a missing file
    before = {f: (work / f).read_bytes() for f in ("derived.bin", "summary.bin", "samples.bin")}
    (work / "broken").write_text(spec + "bad 0 1 %s add\n" % a)
    for other in ("broken", "absent"):
        r = subprocess.run([exe, "run", "--append"], cwd=str(work), env=dict(env, APEMOST_DERIVED_FILE=other),
                           stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode != 0 and (b"broken: line 4: " in r.stderr if other == "broken" else b"absent" in r.stderr), r.stderr
        assert {f: (work / f).read_bytes() for f in before} == before
    # other columns than the file's: no append
    (work / "other").write_text(spec.replace("split", "gap"))
    assert subprocess.call([exe, "run", "--append"], cwd=str(work), env=dict(env, APEMOST_DERIVED_FILE="other"),
                           stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=300) != 0
    # alone the token writes no sample file
    only = tmp_path / "only"
    only.mkdir()
    for f in ("params", "data", "derived"):
        (only / f).write_bytes((work / f).read_bytes())
    env_only = dict(env, APEMOST_DUMP="derived")
    for phase in ("calibrate_first", "calibrate_rest", "run"):
        subprocess.check_call([exe, phase], cwd=str(only), env=env_only, stdout=subprocess.DEVNULL, timeout=300)
    assert not [f for f in os.listdir(str(only)) if f.endswith(".prob.dump") or f.startswith("prob-chain") or f == "samples.bin"]
    same_derived(dv.Derived.read(str(only / "derived.bin")), first, "the token alone")
