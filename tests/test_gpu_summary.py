"""On-device run summaries (apemost_hip_summary_*, pt_summary.h): the sums and counts equal host recounts of
the same rows bit for bit, whatever the call boundaries; they agree with the oracle; they leave the chains
alone; sharded ladders give the same summary; and the C host's APEMOST_DUMP=summary feeds `analyse`."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler
from apemost_amd.summary import RunSummary, batch_size_for, batches_closed
from oracle import oracle as orc
from tests import hostlib, summary_rows as sr
from tests.helpers import make_pair

pytestmark = pytest.mark.gpu

CASES = {
    "simplesin16": (lambda: wl.simplesin(n_data=256, n_chain=16), 16, 30, 10),
    "pulse16": (lambda: wl.pulse(n_data=257, n_chain=16), 16, 100, 3),
    "config2": (lambda: wl.simplesin(n_data=1024, n_chain=128), 128, 20, 15),
}
NBINS = 200


def _run(case, seed=5):
    make, n_chain, n_rounds, n_swap = CASES[case]
    w = make()
    st, lad, rng = make_pair(w, n_chain, seed=seed)
    s = HipSampler(w.model, w.n_par, n_chain, w.data, seed=seed)
    s.set_state(st)
    d = torch.zeros((n_rounds * n_swap, n_chain, w.n_par + 2), dtype=torch.float64, device="cuda")
    s.run_sampler(n_rounds, n_swap, d.data_ptr())
    s.synchronize()                                          # (torch reads the rows on a stream of its own)
    return w, s, d, (st, lad, rng, n_rounds, n_swap)


def _same(a, b):
    assert a.n == b.n and a.n_batches == b.n_batches
    assert np.array_equal(a.hist, b.hist)
    assert a.prob_sum.tobytes() == b.prob_sum.tobytes()
    assert a.batch_sums.tobytes() == b.batch_sums.tobytes()


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("hist_all", [False, True])
def test_summary_equals_host_recount(case, hist_all):
    w, s, d, _ = _run(case)
    n_steps, n_chain = d.shape[0], d.shape[1]
    nh = n_chain if hist_all else 1
    bs = 7
    s.summary_begin(w.pmin, w.pmax, n_hist_chains=nh, nbins=NBINS, batch_size=bs, max_batches=batches_closed(n_steps, bs))
    s.summary_accumulate(d.data_ptr(), n_steps)
    got = s.summary()
    rows = d.cpu().numpy()
    ref = RunSummary.from_rows(rows, nh, NBINS, bs, batches_closed(n_steps, bs), w.pmin, w.pmax)
    _same(got, ref)
    assert got.n == n_steps and int(got.hist[0].sum()) == n_steps * w.n_par
    s.close()


@pytest.mark.parametrize("case", ["simplesin16", "pulse16"])
def test_call_boundaries_and_thinning(case):
    w, s, d, _ = _run(case)
    n_steps, n_chain = d.shape[0], d.shape[1]
    rows = d.cpu().numpy()
    bs = 5
    mb = batches_closed(n_steps, bs)

    def summary_of(pieces, skip=0, thin=1):
        s.summary_begin(w.pmin, w.pmax, n_hist_chains=3, nbins=NBINS, batch_size=bs, max_batches=mb)
        off = 0
        for n in pieces:
            # the kept steps of one piece: skip + k thin within it (the host adjusts skip per piece)
            s.summary_accumulate(d[off:].data_ptr(), n, skip, thin)
            off += n
        return s.summary()

    one = summary_of([n_steps])
    _same(one, RunSummary.from_rows(rows, 3, NBINS, bs, mb, w.pmin, w.pmax))
    for pieces in ([1, 13, 50, n_steps - 64], [4, 4, 4, 4, n_steps - 16], [bs - 1, bs, bs + 1, n_steps - 3 * bs]):
        _same(summary_of(pieces), one)                       # batches span the calls
    for skip, thin in ((0, 3), (2, 3), (6, 7)):
        kept = rows[skip::thin]
        got = summary_of([n_steps], skip, thin)
        _same(got, RunSummary.from_rows(kept, 3, NBINS, bs, mb, w.pmin, w.pmax))
        # the pack kernel keeps the same steps
        packed = torch.zeros_like(d)
        host = torch.zeros(d.shape, dtype=torch.float64).pin_memory()
        n_kept = C.c_uint64(0)
        capi.check(capi.lib().apemost_hip_samples_pack_read_async(s._h, d.data_ptr(), n_steps, skip, thin, 0, 1,
                                                                  packed.data_ptr(), host.data_ptr(), None,
                                                                  C.byref(n_kept)))
        capi.check(capi.lib().apemost_hip_samples_wait(s._h))
        assert n_kept.value == got.n == len(kept)
        assert np.array_equal(host.numpy()[:n_kept.value], kept)
    s.close()


def test_summary_against_oracle():
    w, s, d, (st, lad, rng, n_rounds, n_swap) = _run("simplesin16", seed=17)
    n_steps = d.shape[0]
    s.summary_begin(w.pmin, w.pmax, n_hist_chains=16, nbins=NBINS, batch_size=17, max_batches=batches_closed(n_steps, 17))
    s.summary_accumulate(d.data_ptr(), n_steps)
    got = s.summary()
    ref_rows = orc.run_sampler(lad, rng, n_rounds, n_swap, record=True)
    ref = RunSummary.from_rows(ref_rows, 16, NBINS, 17, batches_closed(n_steps, 17), w.pmin, w.pmax)
    np.testing.assert_allclose(got.evidence(st.beta), ref.evidence(st.beta), rtol=1e-9)
    np.testing.assert_allclose(got.prob_sum, ref.prob_sum, rtol=1e-9)
    assert np.array_equal(got.hist, ref.hist)
    s.close()


def test_summary_does_not_change_the_chains():
    w = wl.pulse(n_data=257, n_chain=16)
    st, _, _ = make_pair(w, 16, seed=3)
    out = []
    for with_summary in (False, True):
        s = HipSampler(w.model, w.n_par, 16, w.data, seed=3)
        s.set_state(st)
        d = torch.zeros((2, 60, 16, w.n_par + 2), dtype=torch.float64, device="cuda")
        if with_summary:
            s.summary_begin(w.pmin, w.pmax, n_hist_chains=16, nbins=NBINS, batch_size=3, max_batches=200)
        for k in range(4):
            buf = d[k % 2]
            s.run_sampler(20, 3, buf.data_ptr())
            if with_summary:
                s.summary_accumulate(buf.data_ptr(), 60)
                capi.check(s.L.apemost_hip_samples_wait(s._h))    # before the buffer is written again
        s.synchronize()
        out.append((s.get_state(), d.cpu().numpy()))
        if with_summary:
            assert s.summary().n == 240
        s.close()
    for f in ("params", "params_best", "prob", "prior", "prob_best", "accept", "reject", "n_iter", "swapcount", "ticks"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()


def test_two_shards_give_the_same_summary():
    w = wl.pulse(n_data=96, n_chain=11)
    n_global, n_rounds, n_swap, seed, bs = 11, 120, 3, 29, 6
    n_steps = n_rounds * n_swap
    mb = batches_closed(n_steps, bs)
    st, _, _ = make_pair(w, n_global, seed=seed)
    whole = HipSampler(w.model, w.n_par, n_global, w.data, seed=seed)
    whole.set_state(st)
    dw = torch.zeros((n_steps, n_global, w.n_par + 2), dtype=torch.float64, device="cuda")
    whole.run_sampler(n_rounds, n_swap, dw.data_ptr())
    whole.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=NBINS, batch_size=bs, max_batches=mb)
    whole.summary_accumulate(dw.data_ptr(), n_steps)
    ref = whole.summary()
    whole.close()
    bounds = [(0, 5), (5, 11)]
    shards, bufs = [], []
    for j, (lo, hi) in enumerate(bounds):
        s = HipSampler(w.model, w.n_par, hi - lo, w.data, seed=seed, chain_offset=lo, n_chains_global=n_global)
        s.set_state(st.slice(lo, hi))
        s.summary_begin(w.pmin, w.pmax, n_hist_chains=1 if j == 0 else 0, nbins=NBINS, batch_size=bs, max_batches=mb)
        shards.append(s)
        bufs.append(torch.zeros((n_steps, hi - lo, w.n_par + 2), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()
    handles = (C.c_void_p * 2)(*[s._h for s in shards])
    ptrs = (C.c_void_p * 2)(*[b.data_ptr() for b in bufs])
    capi.check(capi.lib().apemost_hip_run_shards(handles, 2, n_rounds, n_swap, ptrs))
    for s in shards:
        s.synchronize()
    for s, b in zip(shards, bufs):
        s.summary_accumulate(b.data_ptr(), n_steps)
    got = RunSummary.concat([s.summary() for s in shards])
    _same(got, ref)
    for s in shards:
        s.close()


def test_invalid_arguments():
    w = wl.simplesin(n_data=64, n_chain=4)
    s = HipSampler(w.model, w.n_par, 4, w.data, seed=1)
    L = capi.lib()
    view = capi.SummaryView()
    assert L.apemost_hip_summary_accumulate(s._h, None, 0, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_summary_get(s._h, C.byref(view)) == capi.ERR_INVALID
    lo, hi = np.array(w.pmin, dtype=np.float64), np.array(w.pmax, dtype=np.float64)
    dp = C.POINTER(C.c_double)

    def begin(nh=1, nbins=10, bs=2, mb=10, lo_=lo, hi_=hi):
        c = capi.SummaryConfig(n_hist_chains=nh, nbins=nbins, batch_size=bs, max_batches=mb,
                               lo=lo_.ctypes.data_as(dp), hi=hi_.ctypes.data_as(dp))
        return L.apemost_hip_summary_begin(s._h, C.byref(c))
    bad_hi = hi.copy()
    bad_hi[2] = lo[2]
    inf_lo = lo.copy()
    inf_lo[0] = -np.inf
    nan_hi = hi.copy()
    nan_hi[1] = np.nan
    wide_lo, wide_hi = lo.copy(), hi.copy()
    wide_lo[3], wide_hi[3] = -1e308, 1e308                   # both finite, hi - lo is not
    for kw in (dict(hi_=bad_hi), dict(lo_=inf_lo), dict(hi_=nan_hi), dict(lo_=wide_lo, hi_=wide_hi), dict(nbins=0),
               dict(nbins=4097), dict(nh=-1), dict(nh=5), dict(bs=0)):
        assert begin(**kw) == capi.ERR_INVALID, kw
    assert begin(nh=4, nbins=4096) == capi.OK
    assert begin(bs=4, mb=2) == capi.OK
    d = torch.zeros((12, 4, w.n_par + 2), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    # batches close after samples 3 and 7, the third after 11: 11 samples would need max_batches 3
    assert L.apemost_hip_summary_accumulate(s._h, d.data_ptr(), 11, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_summary_accumulate(s._h, d.data_ptr(), 10, 0, 1) == capi.OK
    assert L.apemost_hip_summary_accumulate(s._h, d.data_ptr(), 1, 0, 1) == capi.ERR_INVALID
    assert L.apemost_hip_summary_accumulate(s._h, d.data_ptr(), 12, 0, 0) == capi.ERR_INVALID
    n = np.zeros(1, dtype=np.uint64)
    view.n = n.ctypes.data_as(C.POINTER(C.c_uint64))
    assert L.apemost_hip_summary_get(s._h, C.byref(view)) == capi.OK and int(n[0]) == 10
    s.summary_end()
    assert L.apemost_hip_summary_get(s._h, C.byref(view)) == capi.ERR_INVALID
    s.close()


# ---- hand-built rows against a restatement that shares nothing with the kernel (tests/summary_rows.py) ----------
@pytest.mark.parametrize("box_set,nbins,bs", [("A", 1, 1000), ("B", 1, 1), ("A", 2, 1), ("B", 2, 1000), ("A", 200, 1000),
                                              ("B", 200, 1), ("A", 200, 1), ("A", 4096, 1), ("B", 4096, 1000)])
def test_summary_of_hand_built_rows(box_set, nbins, bs):
    """Every edge of every parameter with its two neighbours, the box's corners, the widened top, zeros,
    subnormals, infinities, NaN of both signs and values far outside, over boxes where the spacing guess is off by
    one, a negative box and one of width 1e-300; 300 chains, all of them histogrammed (prob_sum spans two
    workgroups); 2300 kept steps in the first call (three passes, the last ragged), then two thinned calls;
    batch size 1 or 1000 (batch 1 straddles the first pass boundary).  Counts equal np.searchsorted over GSL's
    edges, prob_sum and the batch sums equal sequential float additions, all exactly; a sum that is NaN on the
    host (inf - inf in the columns that hold the non-finite values) must be NaN on the device."""
    n_chains = 300
    rows, boxes = sr.build_rows(box_set, nbins, n_chains)
    w = wl.simplesin(n_data=16, n_chain=n_chains)
    s = HipSampler(w.model, w.n_par, n_chains, w.data, seed=1)
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    n_kept = len(sr.kept_steps())
    mb = batches_closed(n_kept, bs)
    lo, hi = np.array([b[0] for b in boxes]), np.array([b[1] for b in boxes])
    s.summary_begin(lo, hi, n_hist_chains=n_chains, nbins=nbins, batch_size=bs, max_batches=mb)
    for first, n, skip, thin in sr.CALLS:
        s.summary_accumulate(d[first:].data_ptr(), n, skip, thin)
    got = s.summary()
    s.close()
    n, prob_sum, hist, batch = sr.expected(rows, boxes, nbins, bs, n_chains)
    assert got.n == n == n_kept and got.n_batches == mb
    assert got.prob_sum.tobytes() == prob_sum.tobytes()
    bad = np.argwhere(got.hist != hist)
    assert len(bad) == 0, "first of %d differing counts: chain %d parameter %d bin %d: %d, expected %d" % (
        (len(bad),) + tuple(bad[0]) + (got.hist[tuple(bad[0])], hist[tuple(bad[0])]))
    assert int(hist[1].sum()) > 0 and int(hist[:, :, nbins - 1].sum()) > 0
    for (h, p), (closed, part) in batch.items():
        want = np.array(closed + [part])
        have = got.batch_sums[h, p, :mb + 1]
        assert len(closed) == mb
        if h % 3:                                            # the finite columns: bit for bit
            assert have.tobytes() == want.tobytes(), (h, p)
        else:
            assert np.array_equal(np.isnan(have), np.isnan(want)), (h, p)
            ok = ~np.isnan(want)
            assert have[ok].tobytes() == want[ok].tobytes(), (h, p)


# ---- the device against the recorded reference: kernel -> summary.bin -> analyse -> fixture -------------------------
@pytest.mark.parametrize("case", ["simplesin", "pulse"])
def test_device_summary_through_analyse_equals_the_reference(case, golden_dir, tmp_path, tmp_path_factory):
    """rows parsed from the oracle-regenerated dump text of a recorded case, accumulated on the device in three
    uneven pieces; `analyse` with APEMOST_DUMP=summary on the summary.bin written from the device's numbers
    leaves the histogram files, the gnuplot file and the stdout that the compiled reference left, byte for byte"""
    from tests import test_reference_analyse as ra
    want, status = ra.fixture_analyse(golden_dir, case)
    files = ra.run_dumps(case, tmp_path_factory)
    rows = ra.parsed_rows(case, files)
    _, lo, hi = ra.box(case, files)
    n, n_beta, width = rows.shape
    w = rb_workload(case)
    s = HipSampler(w.model, w.n_par, n_beta, w.data, seed=1)
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    bs = batch_size_for(n)
    s.summary_begin(np.array(lo), np.array(hi), n_hist_chains=1, nbins=NBINS, batch_size=bs, max_batches=batches_closed(n, bs))
    off = 0
    for piece in (7, 1031, n - 1038):
        s.summary_accumulate(d[off:].data_ptr(), piece)
        off += piece
    got = s.summary()
    s.close()
    assert got.n == n
    got.write(str(tmp_path / "summary.bin"))
    ra.write_inputs(tmp_path, files, dumps=False)
    r = ra.run_host_analyse(ra.host_exe(case, tmp_path_factory), tmp_path, case, summary=True)
    assert r.returncode == status and r.stderr == b"", r.stderr.decode()
    ra.assert_equals_fixture(case, files, ra.collect(case, tmp_path, r), want,
                             "device summary -> analyse vs reference, case %s" % case)


def rb_workload(case):
    from oracle import ref_build as rb
    return rb.workload(case)


# ---- the C host: APEMOST_DUMP=summary ----------------------------------------------------------------------
def _inputs(work, w):
    work.mkdir(exist_ok=True)
    (work / "params").write_text(w.params_file_text())
    (work / "data").write_text(w.data_file_text())


def _lines(out, key):
    return [l.split("\r")[-1] for l in out.splitlines() if key in l]


def _explained(text_hist, summ_hist, values):
    """a bin that differs between the two histograms must hold a value that "%.15e" rounding moves across
    one of its edges"""
    a = [l.split() for l in text_hist.splitlines()]
    b = [l.split() for l in summ_hist.splitlines()]
    assert len(a) == len(b) == NBINS
    for la, lb in zip(a, b):
        assert la[:2] == lb[:2]
        if la[2] != lb[2]:
            e = [float(la[0]), float(la[1])]
            assert any(abs(v - x) <= 1e-15 * max(abs(v), abs(x)) for v in values for x in e), (la, lb)


def test_c_host_summary_mode(tmp_path):
    n_beta, iters = 8, 6000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    runs = {}
    for mode in ("text", "summary", "binary", "binary,summary"):
        work = tmp_path / mode.replace(",", "_")
        _inputs(work, w)
        env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP=mode)
        if mode == "text":
            del env["APEMOST_DUMP"]
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
        runs[mode] = work
    t, s = runs["text"], runs["summary"]
    for f in ("acceptance_rate.dump", "calibration_results"):
        assert (s / f).read_text() == (t / f).read_text(), f
    assert not [f for f in os.listdir(str(s)) if f.endswith(".prob.dump") or f.startswith("prob-chain")]
    assert (runs["binary,summary"] / "samples.bin").read_bytes() == (runs["binary"] / "samples.bin").read_bytes()
    rs = RunSummary.read(str(s / "summary.bin"))
    assert rs.n == iters and rs.batch_size == int(iters ** 0.5) and rs.n_batches == batches_closed(iters, rs.batch_size)
    assert RunSummary.read(str(runs["binary,summary"] / "summary.bin")).prob_sum.tobytes() == rs.prob_sum.tobytes()

    def analyse(work, mode):
        env = dict(os.environ)
        env.pop("APEMOST_DUMP", None)
        if mode:
            env["APEMOST_DUMP"] = mode
        r = subprocess.run([exe, "analyse"], cwd=str(work), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True, timeout=120)
        assert r.returncode == 0, r.stderr
        return r
    at, asu = analyse(t, None), analyse(s, "summary")
    for p, name in enumerate(w.names):
        vals = np.loadtxt(str(t / ("%s-chain-0.prob.dump" % name)))
        _explained((t / (name + ".histogram")).read_text(), (s / (name + ".histogram")).read_text(), vals)
    g = "marginal_distributions.gnuplot"
    assert (s / g).read_text() == (t / g).read_text()
    for key in ("Model probability", "mcmc error"):
        assert _lines(at.stdout, key) == _lines(asu.stdout, key), key
    assert asu.stderr == ""

    # --append continues the summary and keeps its batch size
    env = dict(os.environ, APEMOST_SEED="3")
    subprocess.check_call([exe, "run", "--append"], cwd=str(t), env={k: v for k, v in env.items() if k != "APEMOST_DUMP"},
                          stdout=subprocess.DEVNULL, timeout=300)
    subprocess.check_call([exe, "run", "--append"], cwd=str(s), env=dict(env, APEMOST_DUMP="summary"),
                          stdout=subprocess.DEVNULL, timeout=300)
    rs2 = RunSummary.read(str(s / "summary.bin"))
    assert rs2.n == 2 * iters and rs2.batch_size == rs.batch_size
    assert rs2.n_batches == batches_closed(2 * iters, rs.batch_size)
    assert int(rs2.hist.sum()) == 2 * int(rs.hist.sum())
    at2, as2 = analyse(t, None), analyse(s, "summary")
    for name in w.names:
        vals = np.loadtxt(str(t / ("%s-chain-0.prob.dump" % name)))
        assert len(vals) == 2 * iters
        _explained((t / (name + ".histogram")).read_text(), (s / (name + ".histogram")).read_text(), vals)
    assert _lines(at2.stdout, "Model probability") == _lines(as2.stdout, "Model probability")
    assert re.search(r"batch size %d recorded in summary.bin, floor\(sqrt\(%d values\)\) = %d"
                     % (rs.batch_size, 2 * iters, int((2 * iters) ** 0.5)), as2.stderr), as2.stderr
    assert (s / "acceptance_rate.dump").read_text() == (t / "acceptance_rate.dump").read_text()
