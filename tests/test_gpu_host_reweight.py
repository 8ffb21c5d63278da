"""The C host's APEMOST_DUMP token `reweight` (apemost_amd/host/src/run_reweight.c, run_reweight_device.c): the sine
example of 4 chains and 2000 iterations.  reweight.bin and reweight.txt are, byte for byte, what apemost_amd/reweight.py
writes when the same rows (the binary dump of every chain's parameters) are loaded into a sampler's folds and evaluated
on the device from mbar.bin's free energies; evaluate_numpy on those rows agrees to what numpy's exp against the
device's leaves.  The token needs `mbar`, refuses malformed targets before any file is opened, and changes no byte of
mbar.bin.  Only the executable and its environment are used."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import workloads as wl
from apemost_amd.mbar import Mbar
from apemost_amd.reweight import Reweight, Reweighted
from apemost_amd.sampler import HipSampler
from tests import hostlib

pytestmark = pytest.mark.gpu

N_BETA, ITERS = 4, 2000
TARGETS = "1,0.3,0,1.5"


class Host:
    pass


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    top = tmp_path_factory.mktemp("host_reweight")
    h = Host()
    h.top = top
    h.exe = hostlib.make(str(top / "sine.exe"), ccflags="-DN_BETA=%d -DBURN_IN_ITERATIONS=200 -DMAX_ITERATIONS=%d" % (N_BETA, ITERS))
    h.w = wl.simplesin(n_data=32, n_chain=N_BETA)
    h.template = top / "template"
    h.template.mkdir()
    (h.template / "params").write_text(h.w.params_file_text())
    (h.template / "data").write_text(h.w.data_file_text())
    h.env = dict(os.environ, APEMOST_SEED="3")
    for word in ("APEMOST_REWEIGHT_BINS", "APEMOST_REWEIGHT_BETAS"):
        h.env.pop(word, None)
    for phase in ("calibrate_first", "calibrate_rest"):
        subprocess.check_call([h.exe, phase], cwd=str(h.template), env=h.env, stdout=subprocess.DEVNULL, timeout=120)
    return h


def run(h, name, dump, **env):
    work = h.top / name
    shutil.copytree(str(h.template), str(work))
    r = subprocess.run([h.exe, "run"], cwd=str(work), env=dict(h.env, APEMOST_DUMP=dump, **env), stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE, timeout=300)
    return work, r


def test_the_files_are_pythons_on_the_same_rows(host):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    w = host.w
    work, r = run(host, "all", "binary:all,mbar,reweight", APEMOST_REWEIGHT_BETAS=TARGETS, APEMOST_REWEIGHT_BINS="50")
    assert r.returncode == 0, r.stderr
    mb = Mbar.read(str(work / "mbar.bin"))
    _, params, probs = samples_bin.read(str(work / "samples.bin"))
    assert params.shape == (ITERS, N_BETA, w.n_par) and mb.g is not None and mb.range == (0, ITERS)
    rows = np.concatenate([params, probs], axis=2)
    got = Reweighted.read(str(work / "reweight.bin"))
    targets = [float(v) for v in TARGETS.split(",")]
    assert got.betas_t.tolist() == targets and got.nbins == 50 and got.cols.tolist() == list(range(w.n_par))
    assert (got.n, got.thin, got.range, got.n_chains, got.n_ladders) == (ITERS, 1, (0, ITERS), N_BETA, 1)
    assert got.lo.tolist() == list(w.pmin) and got.hi.tolist() == list(w.pmax)
    host_rw = Reweight.from_rows(rows, mb.betas, None, w.pmin, w.pmax, 50)
    assert host_rw.mbar.ell.tobytes() == mb.ell.tobytes()
    # the same rows through Python and the device
    s = HipSampler(w.model, w.n_par, N_BETA, w.data, seed=1)
    s.mbar_begin(ITERS, mb.betas)
    s.reweight_begin(None, w.pmin, w.pmax, 50)
    s.mbar_set(mb)
    s.reweight_set(host_rw)
    want = s.reweight().evaluate(s.mbar(), targets, g=mb.g, t0=0, t_count=ITERS)
    s.close()
    want.write(str(work / "python.bin"))
    assert (work / "python.bin").read_bytes() == (work / "reweight.bin").read_bytes()
    assert (work / "reweight.txt").read_text() == want.text(w.names)
    # and on the host, up to the exp
    numpy_ = host_rw.evaluate_numpy(mb, targets, g=mb.g, t0=0, t_count=ITERS)
    assert np.allclose(numpy_.mean(), got.mean(), rtol=1e-9, atol=0) and np.allclose(numpy_.ess(), got.ess(), rtol=1e-9)
    assert np.allclose(numpy_.mass(), got.mass(), rtol=0, atol=1e-12)
    for line in (work / "reweight.txt").read_text().splitlines():
        f = line.split("\t")
        assert len(f) == 5 and f[1] in w.names and np.isfinite([float(v) for v in f[2:]]).all()


def test_mbar_alone_writes_the_same_mbar_bin(host):
    alone, r = run(host, "mbar_alone", "mbar")
    assert r.returncode == 0, r.stderr
    both, r = run(host, "mbar_reweight", "mbar,reweight")
    assert r.returncode == 0, r.stderr
    a, b = set(os.listdir(str(alone))), set(os.listdir(str(both)))
    assert b - a == {"reweight.bin", "reweight.txt"} and a <= b
    for f in sorted(a):
        assert (alone / f).read_bytes() == (both / f).read_bytes(), f
    r_ = Reweighted.read(str(both / "reweight.bin"))
    assert r_.betas_t.tolist() == [1.0] and r_.nbins == 200                    # the defaults


def test_refusals_before_any_file_is_opened(host):
    for name, dump, env, said in (("no_mbar", "reweight", {}, "APEMOST_DUMP=reweight needs mbar in the same list"),
                                  ("no_mbar_summary", "summary,reweight", {}, "needs mbar in the same list"),
                                  ("bad_betas", "mbar,reweight", {"APEMOST_REWEIGHT_BETAS": "1,-2"}, "APEMOST_REWEIGHT_BETAS"),
                                  ("bad_list", "mbar,reweight", {"APEMOST_REWEIGHT_BETAS": "1,,2"}, "APEMOST_REWEIGHT_BETAS"),
                                  ("bad_bins", "mbar,reweight", {"APEMOST_REWEIGHT_BINS": "0"}, "APEMOST_REWEIGHT_BINS")):
        work, r = run(host, name, dump, **env)
        assert r.returncode == 1 and said in r.stderr.decode(), (name, r.stderr)
        assert set(os.listdir(str(work))) == set(os.listdir(str(host.template)))
