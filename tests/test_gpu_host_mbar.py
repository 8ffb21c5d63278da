"""The C host's APEMOST_DUMP token `mbar` (apemost_amd/host/src/run_mbar.c, run_mbar_device.c): the sine example of 4
chains and 2000 iterations.  mbar.bin's store is the binary dump's column divided by the betas, on the bits; mbar.txt is
what apemost_amd/mbar.py prints for that file, up to libm's and numpy's exp against the device's (the tolerances of
tests/test_run_mbar_cpu.py); beside every other fold token the token changes no other file; two shards are refused
before any file is opened.  Only the executable and its environment are used."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import workloads as wl
from apemost_amd.mbar import Mbar
from tests import hostlib

pytestmark = pytest.mark.gpu

OTHERS = ["summary", "peaks", "joint", "derived", "evidence", "autocorr", "predict", "pointwise", "check", "periodogram"]
N_BETA, ITERS = 4, 2000


class Host:
    pass


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    top = tmp_path_factory.mktemp("host_mbar")
    h = Host()
    h.top = top
    h.exe = hostlib.make(str(top / "sine.exe"), ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=200 -DMAX_ITERATIONS=%d" % (N_BETA, ITERS))
    w = wl.simplesin(n_data=32, n_chain=N_BETA)
    h.template = top / "template"
    h.template.mkdir()
    (h.template / "params").write_text(w.params_file_text())
    (h.template / "data").write_text(w.data_file_text())
    a, b = w.names[1], w.names[0]
    (h.template / "derived").write_text("split -100 100 %s %s sub\nloglike -1e6 0 like 1 div\n" % (a, b))
    h.env = dict(os.environ, APEMOST_SEED="3", APEMOST_PERIODOGRAM_FREQS="0.05:2:16")
    for phase in ("calibrate_first", "calibrate_rest"):
        subprocess.check_call([h.exe, phase], cwd=str(h.template), env=h.env, stdout=subprocess.DEVNULL, timeout=120)
    return h


def run(h, name, dump, **env):
    work = h.top / name
    shutil.copytree(str(h.template), str(work))
    r = subprocess.run([h.exe, "run"], cwd=str(work), env=dict(h.env, APEMOST_DUMP=dump, **env), stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, timeout=300)
    return work, r


def test_store_free_energies_and_text(host):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    work, r = run(host, "binary_mbar", "binary,mbar")
    assert r.returncode == 0, r.stderr
    mb = Mbar.read(str(work / "mbar.bin"))
    _, _, probs = samples_bin.read(str(work / "samples.bin"))               # [iterations][n_beta][2]
    assert mb.n == ITERS == len(probs) and mb.n_chains == N_BETA and mb.n_ladders == 1 and mb.thin == 1
    assert mb.betas[0] == 1.0 and int(mb.n_bad[0]) == 0 and mb.range == (0, ITERS) and mb.g is not None
    assert mb.ell.tobytes() == Mbar.from_rows(probs[:, :, 1], mb.betas).ell.tobytes()
    device_g = mb.g.copy()
    host_mb = Mbar(mb.ell, mb.betas)
    host_mb.solve_numpy()
    print("free energies:", device_g, "numpy's - the device's:", host_mb.g - device_g)
    assert device_g[0] == 0 and np.all(np.abs(host_mb.g - device_g) <= 1e-9)
    lines, want = (work / "mbar.txt").read_text().split("\n"), mb.text().split("\n")
    assert len(lines) == len(want) == N_BETA + 2 and lines[-1] == want[-1] == ""
    for c in range(N_BETA):
        x, y = [float(v) for v in lines[c].split("\t")], [float(v) for v in want[c].split("\t")]
        assert len(x) == len(y) == 5 and x[0] == y[0] and abs(x[1] - y[1]) <= 1e-9, (x, y)
        assert all(abs(p - q) <= 1e-8 * abs(q) for p, q in zip(x[2:], y[2:])), (x, y)
    x, y = lines[N_BETA].split("\t"), want[N_BETA].split("\t")
    assert x[0] == y[0] == "ln_evidence" and abs(float(x[1]) - float(y[1])) <= 1e-9, (x, y)
    assert float(y[2]) > 0 and abs(float(x[2]) - float(y[2])) <= 1e-6 * float(y[2]), (x, y)


def test_the_token_changes_no_other_file(host):
    without, r = run(host, "others", ",".join(OTHERS))
    assert r.returncode == 0, r.stderr
    with_mbar, r = run(host, "others_mbar", ",".join(OTHERS + ["mbar"]))
    assert r.returncode == 0, r.stderr
    a, b = set(os.listdir(str(without))), set(os.listdir(str(with_mbar)))
    assert b - a <= {"mbar.bin", "mbar.txt"} and "mbar.bin" in b and a <= b
    for f in sorted(a):
        assert (without / f).read_bytes() == (with_mbar / f).read_bytes(), f


def test_two_shards_are_refused_before_any_file_is_opened(host):
    work, r = run(host, "two_shards", "binary,mbar", APEMOST_DEVICES="0,0")
    assert r.returncode == 1 and "APEMOST_DUMP=mbar needs the whole ladder on one device" in r.stderr.decode()
    assert set(os.listdir(str(work))) == set(os.listdir(str(host.template)))
    work, r = run(host, "bad_tol", "mbar", APEMOST_MBAR_TOL="-1")
    assert r.returncode == 1 and "APEMOST_MBAR_TOL" in r.stderr.decode()
    assert set(os.listdir(str(work))) == set(os.listdir(str(host.template)))
