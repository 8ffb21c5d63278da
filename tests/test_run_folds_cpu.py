"""The C host's file halves of the joint and evidence folds without a device (apemost_amd/host/src/run_joint.c and
run_evidence.c): each is built alone with a main of its own (tests/run_joint_check.c, tests/run_evidence_check.c) --
that the link succeeds without the device library is the check that they name none of its symbols -- plain and under
the address and undefined-behaviour sanitizers, reads a file that apemost_amd/joint.py or evidence.py wrote, writes it
back and writes the text files."""
import os
import subprocess

import numpy as np
import pytest

from apemost_amd.evidence import Evidence
from apemost_amd.joint import Joint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "apemost_amd", "host")
STRICT = ["-std=c99", "-ansi", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checkers(request, tmp_path_factory):
    """run_<fold>.c and its check program alone: no other source of the host layer, no device library"""
    out = tmp_path_factory.mktemp("run_folds_" + request.param)
    exes = {}
    for fold in ("joint", "evidence"):
        exes[fold] = str(out / ("run_%s_check" % fold))
        subprocess.check_call(["gcc"] + STRICT + (SANITIZE if request.param == "sanitized" else []) +
                              ["-I" + os.path.join(HOST, "include"), os.path.join(ROOT, "tests", "run_%s_check.c" % fold),
                               os.path.join(HOST, "src", "run_%s.c" % fold), "-o", exes[fold], "-lm"])
    return exes


def test_joint_reader_and_writers_stand_alone(checkers, tmp_path):
    """n_par = 3, nbins = 4, 9 samples: three pairs, and a triangle index that is not a square's"""
    rng = np.random.default_rng(7)
    lo, hi = [-1.0, 0.0, 10.0], [1.0, 2.5, 11.0]
    rows = np.zeros((9, 2, 5))
    rows[:, :, :3] = rng.uniform(np.array(lo) - 0.1, np.array(hi) + 0.1, (9, 2, 3))   # some values outside the box
    jt = Joint.from_rows(rows, lo, hi, chains=(0,), nbins=4, thin=3)
    assert jt.pairs.tolist() == [[0, 1], [0, 2], [1, 2]] and jt.cross.shape == (1, 6) and 0 < jt.counts.sum() < 27
    names = ["alpha", "beta", "gamma"]
    want = tmp_path / "want"
    want.mkdir()
    jt.write(str(tmp_path / "joint.bin"))
    jt.write_text(want, names)
    subprocess.check_call([checkers["joint"], "joint.bin", "copy.bin"] + names, cwd=str(tmp_path), env=ENV)
    assert (tmp_path / "copy.bin").read_bytes() == (tmp_path / "joint.bin").read_bytes()
    files = sorted(os.listdir(str(want)))
    assert files == ["alpha-beta.joint", "alpha-gamma.joint", "beta-gamma.joint", "correlation.matrix"]
    for f in files:
        assert (tmp_path / f).read_text() == (want / f).read_text(), f
    assert len((want / "alpha-beta.joint").read_text().split("\n")) == 4 * 5 + 1


@pytest.mark.parametrize("n,closed,open_batch", [(11, 3, False), (10, 2, True)])
def test_evidence_reader_and_writers_stand_alone(checkers, tmp_path, n, closed, open_batch):
    """3 chains, batch_size = 4, max_batches = 5.  11 samples: batch 0 holds 3, so sample 11 closes the third batch and
    the open one is empty; 10 samples: two closed batches and an open one that holds three.  evidence.txt holds
    logarithms, which the C library and Python may round differently: its numbers are held to the 1e-12 of the value
    that the device test of the token (tests/test_gpu_evidence.py) holds them to; the names and the shape are exact."""
    betas = [1.0, 0.4, 0.1]
    rng = np.random.default_rng(11)
    rows = rng.uniform(-1, 1, (n, 3, 6))
    rows[:, :, 5] = np.asarray(betas) * (-1000.0 + rng.standard_normal((n, 3)))
    ev = Evidence.from_rows(rows, betas, batch_size=4, max_batches=5, thin=2)
    assert ev.n_batches == closed and ev.batch.shape == (3, 6) and ev.batch[:, :closed].all()
    assert bool(ev.batch[:, closed].all()) == open_batch and not ev.batch[:, closed + 1:].any()
    ev.write(str(tmp_path / "evidence.bin"))
    subprocess.check_call([checkers["evidence"], "evidence.bin", "copy.bin", "evidence.txt"], cwd=str(tmp_path), env=ENV)
    assert (tmp_path / "copy.bin").read_bytes() == (tmp_path / "evidence.bin").read_bytes()
    got, want = (tmp_path / "evidence.txt").read_text().split("\n"), ev.text().split("\n")
    assert len(got) == len(want) == 3 + 11 + 1 and got[-1] == want[-1] == ""
    for g, w in zip(got[:-1], want[:-1]):
        g, w = g.split("\t"), w.split("\t")
        assert len(g) == len(w), (g, w)
        if len(w) == 2:                                                      # a total: its name, then its value
            assert g[0] == w[0], (g, w)
            g, w = g[1:], w[1:]
        for x, y in zip(g, w):
            assert np.isfinite(float(y)) and abs(float(x) - float(y)) <= 1e-12 * abs(float(y)), (g, w)
