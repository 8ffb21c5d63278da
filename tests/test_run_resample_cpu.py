"""The C host's file half of resampling without a device (apemost_amd/host/src/run_reweight.c: resample.bin, the
<name>-reweighted-<t>.dump files, APEMOST_RESAMPLE_DRAWS and APEMOST_RESAMPLE_SEED): built alone with a main of its own
(tests/run_resample_check.c), plain and under the address and undefined-behaviour sanitizers.  The bytes are those
apemost_amd/reweight.py writes for the same arrays."""
import os
import subprocess

import numpy as np
import pytest

from apemost_amd.reweight import Resampled

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "apemost_amd", "host")
STRICT = ["-std=c99", "-ansi", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-g"]
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1")
for word in ("APEMOST_RESAMPLE_DRAWS", "APEMOST_RESAMPLE_SEED"):
    ENV.pop(word, None)


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("run_resample_" + request.param) / "run_resample_check")
    subprocess.check_call(["gcc"] + STRICT + (SANITIZE if request.param == "sanitized" else []) +
                          ["-I" + os.path.join(HOST, "include"), os.path.join(ROOT, "tests", "run_resample_check.c"),
                           os.path.join(HOST, "src", "run_reweight.c"), "-o", exe, "-lm"])
    return exe


def pythons(M, seed):
    out = []
    for t, bt in enumerate((1.0, 0.3)):
        r = Resampled([1, 4], bt, seed, M, 1, 5, 1639, 3, (100, 1500))
        r.shift = 49
        r.q_total[0] = (seed + t) % (1 << 64)
        m = np.arange(M)
        r.index[0] = m * (t + 1)
        for a in range(2):
            r.x[0, :, a] = (m + 1.0) / (a + 3.0) - float(t)
        out.append(r)
    return out


@pytest.mark.parametrize("M,seed", [(1, 0), (257, (1 << 64) - 1), (4096, 1 << 63)])
def test_the_files_are_pythons(checker, tmp_path, M, seed):
    env = dict(ENV, APEMOST_RESAMPLE_DRAWS=str(M), APEMOST_RESAMPLE_SEED=str(seed))
    out = subprocess.check_output([checker, "freq", "phase"], cwd=str(tmp_path), env=env)
    assert out.decode() == "%d draws; seed %d\n" % (M, seed)
    want = pythons(M, seed)
    Resampled.write_all(str(tmp_path / "python.bin"), want)
    assert (tmp_path / "resample.bin").read_bytes() == (tmp_path / "python.bin").read_bytes()
    back = Resampled.read_all(str(tmp_path / "resample.bin"))
    assert [b.beta for b in back] == [1.0, 0.3] and back[1].u == seed and back[1].x.tobytes() == want[1].x.tobytes()
    ours = tmp_path / "ours"
    ours.mkdir()
    for t, r in enumerate(want):
        for p in r.write_dumps(ours, ["freq", "phase"], t):
            assert (tmp_path / os.path.basename(p)).read_bytes() == open(p, "rb").read()
    assert sorted(os.listdir(str(ours))) == ["freq-reweighted-0.dump", "freq-reweighted-1.dump", "phase-reweighted-0.dump",
                                             "phase-reweighted-1.dump"]
    # without names: col<index>, as Python's
    plain = tmp_path / "plain"
    plain.mkdir()
    subprocess.check_call([checker], cwd=str(plain), env=env, stdout=subprocess.DEVNULL)
    assert sorted(os.listdir(str(plain))) == sorted(["resample.bin"] + [os.path.basename(p) for t, r in enumerate(want)
                                                                        for p in r.write_dumps(ours, None, t)])


def test_the_environment(checker, tmp_path):
    assert subprocess.check_output([checker], cwd=str(tmp_path), env=ENV).decode() == "0 draws; seed 0\n"
    assert subprocess.check_output([checker], cwd=str(tmp_path), env=dict(ENV, APEMOST_RESAMPLE_DRAWS="", APEMOST_RESAMPLE_SEED="")
                                   ).decode() == "0 draws; seed 0\n"
    assert subprocess.check_output([checker], cwd=str(tmp_path), env=dict(ENV, APEMOST_RESAMPLE_DRAWS="0", APEMOST_RESAMPLE_SEED="7")
                                   ).decode() == "0 draws; seed 7\n"
    assert os.listdir(str(tmp_path)) == []
    bad = [("APEMOST_RESAMPLE_DRAWS", v) for v in ("-1", "16777217", "1e3", "12 ", " 12", "+5", "x", "0x10", "99999999999999999999")]
    bad += [("APEMOST_RESAMPLE_SEED", v) for v in ("-1", "18446744073709551616", "1.5", "seed", "7,", "99999999999999999999")]
    for word, value in bad:
        r = subprocess.run([checker], cwd=str(tmp_path), env=dict(dict(ENV, APEMOST_RESAMPLE_DRAWS="8"), **{word: value}),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        assert r.returncode == 1 and r.stderr.decode().startswith(word + ": expected an integer") and value in r.stderr.decode(), (word, value)
        assert os.listdir(str(tmp_path)) == []
