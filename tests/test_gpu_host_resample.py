"""The C host's APEMOST_RESAMPLE_DRAWS beside the APEMOST_DUMP token `reweight` (apemost_amd/host/src/run_reweight.c,
run_reweight_device.c): the sine example of 4 chains and 2000 iterations, two targets, 256 draws each.  resample.bin is,
byte for byte, what apemost_amd/reweight.py writes when the same rows (the binary dump of every chain's parameters) are
loaded into a sampler's folds and resampled on the device from mbar.bin's free energies; the text dumps are its x at
"%.15e".  A malformed value ends the program before any file is opened.  Only the executable and its environment are
used."""
import os
import sys

import numpy as np
import pytest

from apemost_amd.mbar import Mbar
from apemost_amd.reweight import Resampled, Reweight
from apemost_amd.sampler import HipSampler
from tests.test_gpu_host_reweight import ITERS, N_BETA, host, run  # noqa: F401 (host is the module's fixture)

pytestmark = pytest.mark.gpu

TARGETS = "1,0.3"
DRAWS, SEED = 256, 0x9E3779B97F4A7C15


def test_the_draws_are_pythons_on_the_same_rows(host):  # noqa: F811
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import samples_bin
    w = host.w
    work, r = run(host, "resample", "binary:all,mbar,reweight", APEMOST_REWEIGHT_BETAS=TARGETS,
                  APEMOST_RESAMPLE_DRAWS=str(DRAWS), APEMOST_RESAMPLE_SEED=str(SEED))
    assert r.returncode == 0, r.stderr
    got = Resampled.read_all(str(work / "resample.bin"))
    assert [g.beta for g in got] == [1.0, 0.3] and Resampled.read(str(work / "resample.bin"), 1).beta == 0.3
    mb = Mbar.read(str(work / "mbar.bin"))
    _, params, probs = samples_bin.read(str(work / "samples.bin"))
    rows = np.concatenate([params, probs], axis=2)
    for t, g in enumerate(got):
        assert (g.n_draws, g.u, g.n, g.thin, g.range, g.n_chains, g.n_ladders) == (DRAWS, SEED, ITERS, 1, (0, ITERS), N_BETA, 1)
        assert g.cols.tolist() == list(range(w.n_par)) and g.index.shape == (1, DRAWS) and g.x.shape == (1, DRAWS, w.n_par)
        assert np.all(np.diff(g.index[0].astype(np.int64)) >= 0) and int(g.index.max()) < ITERS * N_BETA
        # the draws are rows of the run: the parameters of step index div K, chain index mod K
        assert g.x[0].tobytes() == np.ascontiguousarray(params[g.step[0], g.chain[0]]).tobytes()
        for a, name in enumerate(w.names):
            lines = (work / ("%s-reweighted-%d.dump" % (name, t))).read_text().splitlines()
            assert lines == ["%.15e" % v for v in g.x[0, :, a].tolist()]
    # the same rows through Python and the device
    host_rw = Reweight.from_rows(rows, mb.betas, None, w.pmin, w.pmax, 200)
    s = HipSampler(w.model, w.n_par, N_BETA, w.data, seed=1)
    s.mbar_begin(ITERS, mb.betas)
    s.reweight_begin(None, w.pmin, w.pmax, 200)
    s.mbar_set(mb)
    s.reweight_set(host_rw)
    rw, dev_mb = s.reweight(), s.mbar()
    want = [rw.resample(dev_mb, bt, DRAWS, SEED, g=mb.g, t0=0, t_count=ITERS) for bt in (1.0, 0.3)]
    q_total = rw.evaluate(dev_mb, [1.0, 0.3], g=mb.g, t0=0, t_count=ITERS).q_total
    s.close()
    assert [int(v.q_total[0]) for v in want] == [int(v) for v in q_total[0]]
    Resampled.write_all(str(work / "python.bin"), want)
    assert (work / "python.bin").read_bytes() == (work / "resample.bin").read_bytes()
    # reweight.bin's q_total is the draws'
    from apemost_amd.reweight import Reweighted
    assert Reweighted.read(str(work / "reweight.bin")).q_total[0].tolist() == [int(g.q_total[0]) for g in got]


def test_malformed_values_end_the_program_before_any_file(host):  # noqa: F811
    for name, env, said in (("bad_draws", {"APEMOST_RESAMPLE_DRAWS": "-3"}, "APEMOST_RESAMPLE_DRAWS: expected an integer in 0 .. 16777216, got '-3'"),
                            ("many_draws", {"APEMOST_RESAMPLE_DRAWS": "16777217"}, "APEMOST_RESAMPLE_DRAWS"),
                            ("bad_seed", {"APEMOST_RESAMPLE_DRAWS": "8", "APEMOST_RESAMPLE_SEED": "x"},
                             "APEMOST_RESAMPLE_SEED: expected an integer in 0 .. 2^64 - 1, got 'x'")):
        work, r = run(host, name, "mbar,reweight", **env)
        assert r.returncode == 1 and said in r.stderr.decode(), (name, r.stderr)
        assert set(os.listdir(str(work))) == set(os.listdir(str(host.template)))
