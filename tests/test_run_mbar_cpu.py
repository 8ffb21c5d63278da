"""The C host's file half of the mbar fold without a device (apemost_amd/host/src/run_mbar.c): built alone with a main
of its own (tests/run_mbar_check.c) -- that the link succeeds without the device library is the check that it names
none of its symbols -- plain and under the address and undefined-behaviour sanitizers.  It reads a column that
apemost_amd/mbar.py wrote, writes it back, solves it with the passes in C and writes the solved state and mbar.txt;
solve_numpy on the same column is the reference.  libm's exp and log stand where numpy's do, so the free energies agree
to the solver's tolerance and the text to what that leaves: 1e-9 absolute on ln_z and the evidence, 1e-8 relative on
the other columns, and the block error, a spread of ten such numbers of the order of 1e-2, to 1e-6 relative."""
import os
import subprocess

import numpy as np
import pytest

from apemost_amd.mbar import Mbar
from tests import mbar_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "apemost_amd", "host")
STRICT = ["-std=c99", "-ansi", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("run_mbar_" + request.param) / "run_mbar_check")
    subprocess.check_call(["gcc"] + STRICT + (SANITIZE if request.param == "sanitized" else []) +
                          ["-I" + os.path.join(HOST, "include"), os.path.join(ROOT, "tests", "run_mbar_check.c"),
                           os.path.join(HOST, "src", "run_mbar.c"), "-o", exe, "-lm"])
    return exe


def test_reader_writer_solver_and_text_stand_alone(checker, tmp_path):
    """5 chains, 1639 kept steps: 8195 samples, two full tiles and one of 3; blocks of 163 and 164 steps"""
    betas, ell = mbar_ref.conjugate(5, 1639, 4, seed=21)
    mb = Mbar(ell, betas, thin=3)
    mb.write(str(tmp_path / "mbar.bin"))
    out = subprocess.check_output([checker, "mbar.bin", "copy.bin", "solved.bin", "mbar.txt"], cwd=str(tmp_path), env=ENV)
    assert (tmp_path / "copy.bin").read_bytes() == (tmp_path / "mbar.bin").read_bytes()
    used, _ = mb.solve_numpy()
    assert int(out.split()[0]) == used
    got = Mbar.read(str(tmp_path / "solved.bin"))
    assert got.ell.tobytes() == mb.ell.tobytes() and got.range == (0, 1639) and got.thin == 3
    assert np.all(np.abs(got.g - mb.g) <= 1e-9) and got.g[0] == 0
    mb.write(str(tmp_path / "python.bin"))
    raw_c, raw_py = (tmp_path / "solved.bin").read_bytes(), (tmp_path / "python.bin").read_bytes()
    g_at = 8 + 16 + 32 + 8 * 5 + 8
    assert raw_c[:g_at] == raw_py[:g_at] and raw_c[g_at + 40:] == raw_py[g_at + 40:]     # all but g: the same bytes
    lines, want = (tmp_path / "mbar.txt").read_text().split("\n"), mb.text().split("\n")
    assert len(lines) == len(want) == 5 + 2 and lines[-1] == want[-1] == ""
    for c in range(5):
        x, y = [float(v) for v in lines[c].split("\t")], [float(v) for v in want[c].split("\t")]
        assert len(x) == len(y) == 5 and x[0] == y[0] and abs(x[1] - y[1]) <= 1e-9
        assert all(abs(a - b) <= 1e-8 * abs(b) for a, b in zip(x[2:], y[2:])), (x, y)
    x, y = lines[5].split("\t"), want[5].split("\t")
    assert x[0] == y[0] == "ln_evidence" and abs(float(x[1]) - float(y[1])) <= 1e-9
    assert float(y[2]) > 0 and abs(float(x[2]) - float(y[2])) <= 1e-6 * float(y[2])


def test_refusals(checker, tmp_path):
    col = np.full((6, 2), -3.0)
    col[4, 1] = np.nan
    Mbar.from_rows(col, [1.0, 0.5]).write(str(tmp_path / "bad.bin"))
    r = subprocess.run([checker, "bad.bin", "copy.bin", "solved.bin", "mbar.txt"], cwd=str(tmp_path), env=ENV,
                       stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1 and "1 values that are not finite" in r.stderr
    betas, ell = mbar_ref.conjugate(3, 40, 4, seed=2)
    Mbar(ell, betas).write(str(tmp_path / "mbar.bin"))
    for env, word in ((dict(ENV, APEMOST_MBAR_TOL="0"), "APEMOST_MBAR_TOL"), (dict(ENV, APEMOST_MBAR_ITER="x"), "APEMOST_MBAR_ITER")):
        r = subprocess.run([checker, "mbar.bin", "copy.bin", "solved.bin", "mbar.txt"], cwd=str(tmp_path), env=env,
                           stderr=subprocess.PIPE, universal_newlines=True)
        assert r.returncode == 1 and word in r.stderr
    r = subprocess.run([checker, "mbar.bin", "copy.bin", "solved.bin", "mbar.txt"], cwd=str(tmp_path),
                       env=dict(ENV, APEMOST_MBAR_TOL="1e-300", APEMOST_MBAR_ITER="3"), stderr=subprocess.PIPE,
                       universal_newlines=True)
    assert r.returncode == 1 and "no convergence" in r.stderr
    with open(str(tmp_path / "mbar.bin"), "r+b") as f:
        f.truncate(200)
    r = subprocess.run([checker, "mbar.bin", "copy.bin", "solved.bin", "mbar.txt"], cwd=str(tmp_path), env=ENV,
                       stderr=subprocess.PIPE, universal_newlines=True)
    assert r.returncode == 1 and "truncated mbar file" in r.stderr
