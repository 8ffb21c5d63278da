"""On-device peaks (apemost_hip_peaks_*, pt_peaks.h): every field of the view and the printed table equal
tests/peaks_ref.py -- the restatement of the reference's peaks.exe that tests/test_peaks_cpu.py holds to recorded
runs of the compiled tool -- with ==, over the column lengths at which a tiled sort changes path, hand-built
content, every call boundary, a real run, a ladder batch and the C host's APEMOST_DUMP=peaks."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from apemost_amd import capi, workloads as wl
from apemost_amd.sampler import HipSampler
from tests import hostlib
from tests.helpers import make_pair
from tests.peaks_ref import PEAKS_MAX, RefPeaks
from tests.test_peaks_cpu import fixture

pytestmark = pytest.mark.gpu

N_CHAINS, KEPT = 5, (1, 3)                                   # two kept chains that are not adjacent
LO = np.array([0.0, -3.0, 10.0, -1.0])
HI = np.array([10.0, 5.0, 11.0, 1.0])


@pytest.fixture(scope="module")
def sampler():
    w = wl.simplesin(n_data=16, n_chain=N_CHAINS)
    s = HipSampler(w.model, w.n_par, N_CHAINS, w.data, seed=1)
    yield s
    s.close()


def on_device(rows):
    d = torch.from_numpy(np.ascontiguousarray(rows)).cuda()
    torch.cuda.synchronize()
    return d


def assert_column(pk, k, p, values, lo, hi, what=""):
    r = RefPeaks(values, lo, hi)
    at = (what, k, p)
    assert int(pk.n_values[k, p]) == r.n_values, at
    assert int(pk.n_peaks[k, p]) == r.n_peaks, at
    assert np.array_equal(pk.left[k, p], r.left) and np.array_equal(pk.right[k, p], r.right), at
    assert np.array_equal(pk.q_set[k, p], r.q_set), at
    assert pk.q[k, p].tobytes() == r.q.tobytes(), at
    if r.n_peaks <= PEAKS_MAX:
        assert pk.table(p, k).tobytes() == r.table.tobytes(), at
        assert pk.text(p, k) == r.text, at
    return r


def assert_peaks(pk, rows, chains=KEPT, lo=LO, hi=HI, what=""):
    assert int(pk.n[0]) == len(rows), what
    return [[assert_column(pk, k, p, rows[:, c, p], lo[p], hi[p], what) for p in range(rows.shape[2] - 2)]
            for k, c in enumerate(chains)]


def content(n, seed):
    """rows [n][N_CHAINS][6].  Parameter 0: three modes and stray singles on a 1e-4 grid, duplicates, and values
    outside the box, NaN and both infinities among them; 1: a coarse grid over more than the box (many duplicates,
    both ends hit exactly); 2: one admitted value, the rest outside; 3: nothing admitted."""
    rng = np.random.RandomState(seed)
    rows = rng.uniform(-100, 100, (n, N_CHAINS, 6))
    for c in range(N_CHAINS):
        mode = rng.randint(0, 3, n)
        v = np.array([2.0, 5.5, 9.0])[mode] + rng.normal(0, 0.1, n) * (mode + 1)
        v = np.round(v * 1e4) / 1e4
        stray = rng.uniform(size=n) < 20.0 / n               # about twenty, whatever n is: they must not bridge the modes
        v[stray] = np.round(rng.uniform(0, 10, n)[stray] * 1e4) / 1e4
        special = rng.uniform(size=n)
        for value, share in ((np.nan, 0.01), (np.inf, 0.02), (-np.inf, 0.03), (10.5, 0.04), (-1e-9, 0.05)):
            v[(special > share - 0.01) & (special < share)] = value
        rows[:, c, 0] = v + 0.0                              # (no -0.0: the tool's order of the two zeros is open)
        rows[:, c, 1] = np.round(rng.uniform(-4, 6, n) * 2) / 2 + 0.0
        rows[:, c, 2] = rng.choice([9.5, 11.5, np.nan, 1e300], n)
        rows[n // 2, c, 2] = 10.25 + 0.125 * c
        rows[:, c, 3] = rng.choice([-1.0000000000000002, 1.0000000000000002, np.nan, np.inf], n)
    return rows


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4095, 4096, 4097, 3 * 4096 + 17, 2 ** 17 + 1])
def test_sizes_and_content(sampler, n):
    """one tile, the tile boundary, the first global stage, several global stages, and a length whose padding is
    far from a power of two"""
    rows = content(n, seed=n)
    d = on_device(rows)
    sampler.peaks_begin(LO, HI, chains=KEPT, capacity=n)
    sampler.peaks_accumulate(d.data_ptr(), n)
    refs = assert_peaks(sampler.peaks(), rows, what="n = %d" % n)
    for k in range(len(KEPT)):
        assert refs[k][3].n_values == 0 and refs[k][3].n_peaks == 0
        assert refs[k][2].n_values == 1 and refs[k][2].n_peaks == 1
    if n >= 4095:
        assert refs[0][0].n_peaks >= 3 and refs[0][0].n_values < n and refs[0][1].n_values < n
    sampler.peaks_end()


def fixture_rows(golden_dir, cases, extra=()):
    """the recorded cases as the columns of chain KEPT[0], shorter ones filled up with NaN, which the filter drops"""
    cols = [fixture(golden_dir, c)[:3] for c in cases] + list(extra)
    n = max(len(v) for v, _, _ in cols)
    rows = np.full((n, N_CHAINS, 6), np.nan)
    for p, (v, _, _) in enumerate(cols):
        rows[:len(v), KEPT[0], p] = v
        rows[:len(v), KEPT[1], p] = v[::-1]
    return rows, np.array([c[1] for c in cols]), np.array([c[2] for c in cols])


def test_cut_and_carry(sampler, golden_dir):
    """the exact gap, single-sample peaks that print the statistics of the peak before, 99 peaks"""
    cases = ["exact_gap", "modes_and_singles", "ninety_nine_peaks", "three_values"]
    rows, lo, hi = fixture_rows(golden_dir, cases)
    d = on_device(rows)
    sampler.peaks_begin(lo, hi, chains=KEPT, capacity=len(rows))
    sampler.peaks_accumulate(d.data_ptr(), len(rows))
    pk = sampler.peaks()
    refs = assert_peaks(pk, rows, lo=lo, hi=hi)
    assert refs[0][2].n_peaks == 99 and refs[0][0].n_peaks == 5
    for p, c in enumerate(cases):
        assert pk.text(p, 0) == pk.text(p, 1) == fixture(golden_dir, c)[3], c      # the compiled tool's own output
    sampler.peaks_end()


def test_100_peaks_are_refused_with_the_count(sampler, golden_dir):
    hundred = (np.arange(100) * 10.1, 0.0, 1000.0)
    rows, lo, hi = fixture_rows(golden_dir, ["equal_shares", "range_ends", "three_values"], extra=[hundred])
    d = on_device(rows)
    sampler.peaks_begin(lo, hi, chains=KEPT, capacity=len(rows))
    sampler.peaks_accumulate(d.data_ptr(), len(rows))
    from apemost_amd.peaks import Peaks
    pk = Peaks.empty(len(KEPT), 4)
    assert sampler.L.apemost_hip_peaks_get(sampler._h, C.byref(pk.view())) == capi.ERR_INVALID
    msg = sampler.L.apemost_hip_last_error().decode()
    assert "kept chain 0, parameter 3" in msg and "100 peaks" in msg, msg
    assert pk.n_peaks[:, 3].tolist() == [100, 100]
    assert_peaks(pk, rows, lo=lo, hi=hi)                     # the other columns, and the first 99 peaks of this one
    with pytest.raises(capi.ApemostHipError):
        sampler.peaks()
    sampler.peaks_end()


def test_call_boundaries_thinning_and_a_get_in_the_middle(sampler):
    n = 5000
    rows = content(n, seed=77)
    d = on_device(rows)
    for pieces, skip, thin in (([1, 13, 50, n - 64], 0, 1), ([n], 0, 3), ([n], 2, 3), ([n], 6, 7), ([64, n - 64], 2, 3)):
        sampler.peaks_begin(LO, HI, chains=KEPT, capacity=n)
        off = 0
        for i, piece in enumerate(pieces):
            # the kept steps of one piece: skip + k thin within it (the host adjusts skip per piece)
            first = (skip - off) % thin if off > skip else skip - off
            sampler.peaks_accumulate(d[off:].data_ptr(), piece, first, thin)
            off += piece
            if i == 1 and thin == 1:                         # a get in the middle, then more accumulates
                assert_peaks(sampler.peaks(), rows[:off], what="middle")
        assert_peaks(sampler.peaks(), rows[skip::thin], what="pieces %r skip %d thin %d" % (pieces, skip, thin))
        assert_peaks(sampler.peaks(), rows[skip::thin], what="a second get")   # the stored columns are intact
    sampler.peaks_end()


def test_capacity_and_invalid_arguments(sampler):
    L = sampler.L
    rows = content(12, seed=5)
    d = on_device(rows)
    from apemost_amd.peaks import Peaks
    pk = Peaks.empty(1, 4)
    sampler.peaks_end()
    assert L.apemost_hip_peaks_accumulate(sampler._h, d.data_ptr(), 1, 0, 1) == capi.ERR_INVALID     # no begin
    assert L.apemost_hip_peaks_get(sampler._h, C.byref(pk.view())) == capi.ERR_INVALID
    assert L.apemost_hip_peaks_begin(sampler._h, None) == capi.ERR_INVALID
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)

    def begin(chains=(0,), capacity=10, lo=LO, hi=HI):
        ch = np.array(chains, dtype=np.int32)
        lo, hi = np.array(lo, dtype=np.float64), np.array(hi, dtype=np.float64)
        cfg = capi.PeaksConfig(n_keep=len(ch), chains=ch.ctypes.data_as(ip), capacity=capacity, lo=lo.ctypes.data_as(dp),
                               hi=hi.ctypes.data_as(dp))
        return L.apemost_hip_peaks_begin(sampler._h, C.byref(cfg))
    bad_hi, nan_lo = HI.copy(), LO.copy()
    bad_hi[2], nan_lo[1] = LO[2], np.nan
    for kw in (dict(chains=()), dict(chains=(0, 0)), dict(chains=(2, 1)), dict(chains=(N_CHAINS,)), dict(chains=(-1,)),
               dict(capacity=0), dict(capacity=2 ** 30 + 1), dict(hi=bad_hi), dict(lo=nan_lo),
               dict(chains=tuple(range(N_CHAINS + 1)))):
        assert begin(**kw) == capi.ERR_INVALID, kw
    assert begin(capacity=10) == capi.OK
    assert L.apemost_hip_peaks_accumulate(sampler._h, d.data_ptr(), 8, 0, 1) == capi.OK
    assert L.apemost_hip_peaks_accumulate(sampler._h, d.data_ptr(), 3, 0, 1) == capi.ERR_INVALID    # 8 + 3 > 10
    assert "capacity" in L.apemost_hip_last_error().decode()
    assert L.apemost_hip_peaks_accumulate(sampler._h, d.data_ptr(), 12, 0, 0) == capi.ERR_INVALID   # thin 0
    assert L.apemost_hip_peaks_get(sampler._h, C.byref(pk.view())) == capi.OK and int(pk.n[0]) == 8   # did not move
    assert_peaks(pk, rows[:8], chains=(0,))
    assert L.apemost_hip_peaks_accumulate(sampler._h, d[8:].data_ptr(), 4, 1, 2) == capi.OK         # rows 9 and 11
    assert L.apemost_hip_peaks_get(sampler._h, C.byref(pk.view())) == capi.OK and int(pk.n[0]) == 10
    assert_peaks(pk, np.concatenate([rows[:8], rows[9::2]]), chains=(0,))
    sampler.peaks_end()


# ---- a real run ------------------------------------------------------------------------------------------------
RUNS = {"simplesin16": (lambda: wl.simplesin(n_data=256, n_chain=16), 30, 10),
        "pulse16": (lambda: wl.pulse(n_data=257, n_chain=16), 100, 3)}


@pytest.mark.parametrize("case", sorted(RUNS))
def test_a_real_run_and_the_chains_are_left_alone(case):
    make, n_rounds, n_swap = RUNS[case]
    w = make()
    st, _, _ = make_pair(w, 16, seed=5)
    n_steps = n_rounds * n_swap
    out = []
    for with_peaks in (False, True):
        s = HipSampler(w.model, w.n_par, 16, w.data, seed=5)
        s.set_state(st)
        d = torch.zeros((n_steps, 16, w.n_par + 2), dtype=torch.float64, device="cuda")
        if with_peaks:
            s.peaks_begin(w.pmin, w.pmax, chains=(0,), capacity=n_steps)
        half = n_rounds // 2
        for first, rounds in ((0, half), (half, n_rounds - half)):
            buf = d[first * n_swap:]
            s.run_sampler(rounds, n_swap, buf.data_ptr())
            if with_peaks:
                s.peaks_accumulate(buf.data_ptr(), rounds * n_swap)
                capi.check(s.L.apemost_hip_samples_wait(s._h))
        s.synchronize()
        rows = d.cpu().numpy()
        out.append((s.get_state(), rows))
        if with_peaks:
            pk = s.peaks()
            refs = assert_peaks(pk, rows, chains=(0,), lo=w.pmin, hi=w.pmax, what=case)
            assert all(r.n_values == n_steps and r.n_peaks >= 1 for r in refs[0])
        s.close()
    for f in ("params", "params_best", "prob", "prior", "prob_best", "accept", "reject", "n_iter", "swapcount", "ticks",
              "step", "params_accepts", "params_rejects", "beta"):
        assert getattr(out[0][0], f).tobytes() == getattr(out[1][0], f).tobytes(), f
    assert out[0][1].tobytes() == out[1][1].tobytes()


def test_a_batch_of_three_ladders_equals_three_samplers():
    from tests.test_gpu_ladder_batch import concat, ladders, make_batch, run, N_ROUNDS, N_SWAP, PER
    ws, seeds, sts, _, _ = ladders("simplesin", 3)
    w = ws[0]
    n_steps = N_ROUNDS * N_SWAP
    batch = make_batch(ws, seeds, 4)
    batch.set_state(concat(sts))
    d = torch.zeros((n_steps, 3 * PER, w.n_par + 2), dtype=torch.float64, device="cuda")
    batch.peaks_begin(w.pmin, w.pmax, chains=(0, PER, 2 * PER), capacity=n_steps)
    batch.run_sampler(N_ROUNDS, N_SWAP, d.data_ptr())
    batch.peaks_accumulate(d.data_ptr(), n_steps)
    got = batch.peaks()
    assert_peaks(got, d.cpu().numpy(), chains=(0, PER, 2 * PER), lo=w.pmin, hi=w.pmax)
    batch.close()
    for b in range(3):
        alone = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=4)
        alone.set_state(sts[b])
        da = torch.zeros((n_steps, PER, w.n_par + 2), dtype=torch.float64, device="cuda")
        alone.peaks_begin(w.pmin, w.pmax, chains=(0,), capacity=n_steps)
        alone.run_sampler(N_ROUNDS, N_SWAP, da.data_ptr())
        alone.peaks_accumulate(da.data_ptr(), n_steps)
        one = alone.peaks()
        alone.close()
        for f in ("n_values", "n_peaks", "left", "right", "q", "q_set"):
            assert getattr(got, f)[b].tobytes() == getattr(one, f)[0].tobytes(), (b, f)
        for p in range(w.n_par):
            assert got.text(p, b) == one.text(p, 0)


# ---- the C host: APEMOST_DUMP=peaks -----------------------------------------------------------------------------
def test_c_host_peaks_token(tmp_path):
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters = 8, 6000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    runs = {}
    for mode in ("binary:all", "summary,peaks", "summary", "binary:all,peaks"):
        work = tmp_path / mode.replace(",", "_").replace(":", "_")
        work.mkdir()
        (work / "params").write_text(w.params_file_text())
        (work / "data").write_text(w.data_file_text())
        env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP=mode)
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
        runs[mode] = work
    _, rows, _ = samples_bin.read(str(runs["binary:all"] / "samples.bin"))    # [iters][n_beta][n_par]
    assert rows.shape == (iters, n_beta, w.n_par)
    for mode in ("summary,peaks", "binary:all,peaks"):
        for p, name in enumerate(w.names):
            want = RefPeaks(rows[:, 0, p], w.pmin[p], w.pmax[p]).text
            assert (runs[mode] / (name + ".peaks")).read_text() == want, (mode, name)
    # without the token: the same files as before and no .peaks
    assert not [f for f in os.listdir(str(runs["summary"])) if f.endswith(".peaks")]
    assert not [f for f in os.listdir(str(runs["binary:all"])) if f.endswith(".peaks")]
    assert (runs["summary,peaks"] / "summary.bin").read_bytes() == (runs["summary"] / "summary.bin").read_bytes()
    assert (runs["binary:all,peaks"] / "samples.bin").read_bytes() == (runs["binary:all"] / "samples.bin").read_bytes()
    assert sorted(f for f in os.listdir(str(runs["summary,peaks"])) if not f.endswith(".peaks")) == \
        sorted(os.listdir(str(runs["summary"])))
