"""The C host's APEMOST_DUMP token `periodogram` (apemost_amd/host/src/run_periodogram.c, run_periodogram_device.c): a run
of the simplesin example writes periodogram.bin and periodogram.txt, and periodogram.bin reads back as the Python fold of
the same run.  The host computes the grid and the Lomb-Scargle weights itself, with libm's cos and sin where
periodogram.weights has numpy's: the two are held together to 1e-12 relative (sums of 70 terms of order one), and the
Python fold is begun with the file's own grid and weights, so that every word compares byte for byte."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import periodogram as pg, workloads as wl
from apemost_amd.sampler import HipSampler
from tests import hostlib
from tests.test_gpu_periodogram import assert_same, fold

pytestmark = pytest.mark.gpu

GRID = "0.02:0.9:45"


def run_phases(exe, work, env, phases=("calibrate_first", "calibrate_rest", "run")):
    for phase in phases:
        subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)


def test_c_host_periodogram_token(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters = 8, 600
    w = wl.simplesin(n_data=70, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=300 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    runs = {}
    for mode in ("binary,periodogram", "periodogram"):
        work = tmp_path / mode.replace(",", "_")
        work.mkdir()
        (work / "params").write_text(w.params_file_text())
        (work / "data").write_text(w.data_file_text())
        env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP=mode, APEMOST_PERIODOGRAM_FREQS=GRID)
        run_phases(exe, work, env)
        runs[mode] = (work, env)
    work, env = runs["binary,periodogram"]
    _, params, probs = samples_bin.read(str(work / "samples.bin"))       # [iters][1][n_par], [iters][n_beta][2]
    iters = len(params)                                       # (whole rounds: the last one runs past MAX_ITERATIONS)
    assert iters >= 600
    rows = np.zeros((iters, 1, w.n_par + 2))
    rows[:, 0, :w.n_par] = params[:, 0]
    rows[:, 0, w.n_par:] = probs[:, 0]
    got = pg.Periodogram.read(str(work / "periodogram.bin"))
    assert (got.n_keep, got.n_freq, got.thin, got.n_ladders, got.model, got.sigma) == (1, 45, 1, 1, 0, 0.5)
    assert int(got.n[0]) == iters and got.chains.tolist() == [0] and got.lengths.tolist() == [70]
    data = np.loadtxt(str(work / "data"))                     # what the host parsed
    # the grid, the level and the weights as the header of the token states them
    step = (0.9 - 0.02) / 44.0
    assert got.freqs.tolist() == [0.02 + j * step for j in range(45)]
    assert got.level.tolist() == [-math.log(0.01 / 45.0)]
    want = pg.weights(data[:, 0], got.freqs, "lomb_scargle", 0.5)
    worst = float(np.max(np.abs(got.weights[0] - want) / np.abs(want).max(axis=1, keepdims=True)))
    print("C weights against numpy's: worst relative difference %.3g" % worst)
    assert worst <= 1e-12
    s = HipSampler(w.model, w.n_par, 1, data, seed=1)
    mine = fold(s, rows, (0,), got.freqs, got.weights, got.level)
    s.close()
    assert_same(got, mine, "the C host")
    text = (work / "periodogram.txt").read_text()
    assert text == got.text()
    cols = np.array([[float(v) for v in ln.split("\t")] for ln in text.split("\n")[:-1]])
    assert cols.shape == (45, 7) and np.isfinite(cols).all() and (cols[:, 1] >= cols[:, 3]).all() and (cols[:, 1] <= cols[:, 4]).all()
    assert int(got.peak_counts.sum()) == iters and abs(cols[:, 6].sum() - 1.0) < 1e-12
    # alone the token writes no sample file
    only, _ = runs["periodogram"]
    assert not [f for f in os.listdir(str(only)) if f.endswith(".prob.dump") or f.startswith("prob-chain") or f == "samples.bin"]
    assert (only / "periodogram.bin").read_bytes() == (work / "periodogram.bin").read_bytes()
    assert (only / "periodogram.txt").read_text() == text
    # --append resumes from the file through periodogram_set
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = pg.Periodogram.read(str(work / "periodogram.bin"))
    assert int(second.n[0]) == 2 * iters and second.origin.tobytes() == got.origin.tobytes()
    assert int(second.peak_counts.sum()) == 2 * iters and np.all(second.pmax >= got.pmax) and np.all(second.pmin <= got.pmin)
    # another grid cannot be appended to; a malformed or missing grid and a misspelt token are refused
    for bad in (dict(env, APEMOST_PERIODOGRAM_FREQS="0.02:0.9:44"), dict(env, APEMOST_PERIODOGRAM_FREQS="0.02:0.9"),
                dict(env, APEMOST_PERIODOGRAM_FREQS="0.02:0.9:0"), dict(env, APEMOST_PERIODOGRAM_FREQS="0.9:0.02:45"),
                dict(env, APEMOST_PERIODOGRAM_FREQS="lo:hi:45"), dict(env, APEMOST_PERIODOGRAM_FREQS="0.02:nan:45"),
                dict(env, APEMOST_PERIODOGRAM_FREQS="0.02:0.9:45x"), dict(env, APEMOST_PERIODOGRAM_FREQS=""),
                dict(env, APEMOST_DUMP="binary,periodogramm")):
        run = subprocess.run([exe, "run", "--append"], cwd=str(work), env=bad, stdout=subprocess.DEVNULL,
                             stderr=subprocess.PIPE, timeout=300)
        assert run.returncode != 0, bad["APEMOST_PERIODOGRAM_FREQS"]
        if bad["APEMOST_DUMP"] == env["APEMOST_DUMP"] and bad["APEMOST_PERIODOGRAM_FREQS"] != "0.02:0.9:44":
            assert b"APEMOST_PERIODOGRAM_FREQS=lo:hi:n" in run.stderr, run.stderr
    assert pg.Periodogram.read(str(work / "periodogram.bin")).sum.tobytes() == second.sum.tobytes()   # refused before any file


def test_an_unbounded_run_is_refused(tmp_path):
    w = wl.simplesin(n_data=70, n_chain=8)
    exe = hostlib.make(str(tmp_path / "sine.exe"), ccflags="-DN_BETA=8 -DBURN_IN_ITERATIONS=300 -DMAX_ITERATIONS=0")
    (tmp_path / "params").write_text(w.params_file_text())
    (tmp_path / "data").write_text(w.data_file_text())
    env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP="periodogram", APEMOST_PERIODOGRAM_FREQS=GRID)
    run_phases(exe, tmp_path, env, ("calibrate_first", "calibrate_rest"))
    run = subprocess.run([exe, "run"], cwd=str(tmp_path), env=env, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=60)
    assert run.returncode != 0 and b"APEMOST_DUMP=periodogram needs a bounded run" in run.stderr, run.stderr
    assert not (tmp_path / "periodogram.bin").exists()
