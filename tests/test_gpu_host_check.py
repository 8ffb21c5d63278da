"""The C host's APEMOST_DUMP token `check` (apemost_amd/host/src/run_check.c, run_check_device.c): a run of the simplesin
example writes check.bin, check.txt and check_stats.txt, and check.bin reads back as the Python fold of the same run."""
import os
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import check as ck, workloads as wl
from apemost_amd.sampler import HipSampler
from tests import hostlib
from tests.test_gpu_check import assert_same_check, fold

pytestmark = pytest.mark.gpu


def test_c_host_check_token(tmp_path):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    n_beta, iters, bins = 8, 600, 32
    w = wl.simplesin(n_data=70, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"),
                       ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=300 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    runs = {}
    for mode in ("binary,check", "check"):
        work = tmp_path / mode.replace(",", "_")
        work.mkdir()
        (work / "params").write_text(w.params_file_text())
        (work / "data").write_text(w.data_file_text())
        env = dict(os.environ, APEMOST_SEED="3", APEMOST_DUMP=mode, APEMOST_CHECK_BINS=str(bins))
        for phase in ("calibrate_first", "calibrate_rest", "run"):
            subprocess.check_call([exe, phase], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
        runs[mode] = (work, env)
    work, env = runs["binary,check"]
    _, params, probs = samples_bin.read(str(work / "samples.bin"))       # [iters][1][n_par], [iters][n_beta][2]
    iters = len(params)                                       # (whole rounds: the last one runs past MAX_ITERATIONS)
    assert iters >= 600
    rows = np.zeros((iters, 1, w.n_par + 2))
    rows[:, 0, :w.n_par] = params[:, 0]
    rows[:, 0, w.n_par:] = probs[:, 0]
    got = ck.Check.read(str(work / "check.bin"))
    assert (got.n_keep, got.n_data, got.nbins, got.thin, got.n_ladders, got.model, got.sigma) == (1, 70, bins, 1, 1, 0, 0.5)
    assert int(got.n[0]) == iters and got.chains.tolist() == [0]
    data = np.loadtxt(str(work / "data"))                     # what the host parsed
    assert got.x[0].tobytes() == data[:, 0].tobytes() and got.y[0].tobytes() == data[:, 1].tobytes()
    s = HipSampler(w.model, w.n_par, 1, data, seed=1)
    mine = fold(s, rows, (0,), nbins=bins)
    s.close()
    assert got.edges.tobytes() == mine.edges.tobytes()
    assert_same_check(got, mine, "the C host")
    text = (work / "check.txt").read_text()
    assert text == got.text()
    assert (work / "check_stats.txt").read_text() == got.stats_text()
    cols = np.array([[float(v) for v in ln.split("\t")] for ln in text.split("\n")[:-1]])
    assert cols.shape == (70, 6) and np.isfinite(cols).all() and (cols[:, 4:] >= 0).all() and (cols[:, 4:] <= 1).all()
    assert (got.counts[0, :, :bins].sum(axis=1) == iters).all() and all(0 <= got.p_value(q)[0] <= 1 for q in range(3))
    # alone the token writes no sample file
    only, _ = runs["check"]
    assert not [f for f in os.listdir(str(only)) if f.endswith(".prob.dump") or f.startswith("prob-chain") or f == "samples.bin"]
    assert (only / "check.bin").read_bytes() == (work / "check.bin").read_bytes()
    assert (only / "check_stats.txt").read_text() == (work / "check_stats.txt").read_text()
    # --append resumes from the file; another number of slots, a malformed one and a misspelt token are refused
    subprocess.check_call([exe, "run", "--append"], cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=300)
    second = ck.Check.read(str(work / "check.bin"))
    assert int(second.n[0]) == 2 * iters and second.origin.tobytes() == got.origin.tobytes()
    assert (second.counts[0, :, :bins].sum(axis=1) == 2 * iters).all() and np.all(second.m >= got.m)
    for bad in (dict(env, APEMOST_CHECK_BINS="16"), dict(env, APEMOST_CHECK_BINS="0"), dict(env, APEMOST_CHECK_BINS="many"),
                dict(env, APEMOST_DUMP="binary,chek")):
        assert subprocess.call([exe, "run", "--append"], cwd=str(work), env=bad, stdout=subprocess.DEVNULL,
                               stderr=subprocess.DEVNULL, timeout=300) != 0
