"""The C host's file half of the reweight fold without a device (apemost_amd/host/src/run_reweight.c): built alone
with a main of its own (tests/run_reweight_check.c) -- that the link succeeds without the device library is the check
that it names none of its symbols -- plain and under the address and undefined-behaviour sanitizers.  It reads the sums
apemost_amd/reweight.py wrote from evaluate_numpy, writes them back and writes reweight.txt: the same bytes and the
same text as Python's, whose formulas are the same IEEE operations."""
import os
import subprocess

import numpy as np
import pytest

from apemost_amd.mbar import Mbar
from apemost_amd.reweight import Reweight
from tests.test_reweight_cpu import HI, LO, columns

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "apemost_amd", "host")
STRICT = ["-std=c99", "-ansi", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
for word in ("APEMOST_REWEIGHT_BINS", "APEMOST_REWEIGHT_BETAS"):
    ENV.pop(word, None)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("run_reweight_" + request.param) / "run_reweight_check")
    subprocess.check_call(["gcc"] + STRICT + (SANITIZE if request.param == "sanitized" else []) +
                          ["-I" + os.path.join(HOST, "include"), os.path.join(ROOT, "tests", "run_reweight_check.c"),
                           os.path.join(HOST, "src", "run_reweight.c"), "-o", exe, "-lm"])
    return exe


def sums(nbins, cols, targets):
    K, T = 5, 1639
    betas, ell, x, g = columns(K, T, "gauss", seed=21)
    k = len(cols)
    rw = Reweight(x[:k], cols, LO[:k], HI[:k], nbins, thin=3)
    return rw.evaluate_numpy(Mbar(ell, betas), targets, g=g, t0=100, t_count=1500)


@pytest.mark.parametrize("nbins,cols,targets", [(20, [0, 1, 2, 3], [1.0, 0.3, 0.0, 1.5]), (0, [2], [0.5]), (4096, [1, 5], [1.0])])
def test_reader_writer_and_text_stand_alone(checker, tmp_path, nbins, cols, targets):
    r = sums(nbins, cols, targets)
    r.write(str(tmp_path / "reweight.bin"))
    names = ["name%d" % c for c in cols]
    out = subprocess.check_output([checker, "reweight.bin", "copy.bin", "reweight.txt"] + names, cwd=str(tmp_path), env=ENV)
    assert out.decode() == "200 bins; 1\n"
    assert (tmp_path / "copy.bin").read_bytes() == (tmp_path / "reweight.bin").read_bytes()
    text = (tmp_path / "reweight.txt").read_text()
    assert text == r.text(names) and len(text.splitlines()) == len(targets) * len(cols)
    subprocess.check_call([checker, "reweight.bin", "copy.bin", "plain.txt"], cwd=str(tmp_path), env=ENV, stdout=subprocess.DEVNULL)
    assert (tmp_path / "plain.txt").read_text() == r.text()
    assert np.isfinite([float(v) for line in text.splitlines() for v in line.split("\t")[2:]]).all()


def test_a_variance_below_zero_prints_nan(checker, tmp_path):
    r = sums(0, [2], [0.5])
    r.cross[0, 0, 0] = -1.0
    r.write(str(tmp_path / "reweight.bin"))
    subprocess.check_call([checker, "reweight.bin", "copy.bin", "reweight.txt"], cwd=str(tmp_path), env=ENV, stdout=subprocess.DEVNULL)
    assert (tmp_path / "reweight.txt").read_text() == r.text() and "\tnan\t" in r.text()


def test_the_environment_and_refusals(checker, tmp_path):
    sums(3, [0, 1], [1.0]).write(str(tmp_path / "reweight.bin"))
    args = [checker, "reweight.bin", "copy.bin", "reweight.txt"]
    out = subprocess.check_output(args, cwd=str(tmp_path), env=dict(ENV, APEMOST_REWEIGHT_BINS="4096", APEMOST_REWEIGHT_BETAS="1,0.3,0,1.5e0"))
    assert out.decode() == "4096 bins; 1 0.29999999999999999 0 1.5\n"
    out = subprocess.check_output(args, cwd=str(tmp_path), env=dict(ENV, APEMOST_REWEIGHT_BETAS=",".join(["0.5"] * 64)))
    assert out.decode().count(" 0.5") == 64
    bad = [("APEMOST_REWEIGHT_BINS", v) for v in ("0", "4097", "x", "12x", "-3")]
    bad += [("APEMOST_REWEIGHT_BETAS", v) for v in ("-1", "1,,2", "1,", ",1", "x", "1;2", "inf", "nan", "1,-0.5", ",".join(["1"] * 65))]
    for word, value in bad:
        r = subprocess.run(args, cwd=str(tmp_path), env=dict(ENV, **{word: value}), stderr=subprocess.PIPE, stdout=subprocess.DEVNULL,
                           universal_newlines=True)
        assert r.returncode == 1 and word in r.stderr and "'%s'" % value in r.stderr, (word, value, r.stderr)
    raw = (tmp_path / "reweight.bin").read_bytes()
    for name, data, said in (("short.bin", raw[:-8], "truncated reweight file"), ("head.bin", raw[:30], "truncated reweight file"),
                             ("magic.bin", b"APEMOSTM" + raw[8:], "not a reweight file"),
                             ("cols.bin", raw[:20] + (17).to_bytes(4, "little") + raw[24:], "out of range")):
        (tmp_path / name).write_bytes(data)
        r = subprocess.run([checker, name, "copy.bin", "reweight.txt"], cwd=str(tmp_path), env=ENV, stderr=subprocess.PIPE,
                           stdout=subprocess.DEVNULL, universal_newlines=True)
        assert r.returncode == 1 and said in r.stderr, (name, r.stderr)
    r = subprocess.run([checker, "none.bin", "copy.bin", "reweight.txt"], cwd=str(tmp_path), env=ENV, stderr=subprocess.PIPE,
                       stdout=subprocess.DEVNULL, universal_newlines=True)
    assert r.returncode == 1 and "no such file" in r.stderr
