"""The device likelihoods against values that the COMPILED REFERENCE printed (tests/golden/ref_runs/eval_*,
apps/eval_main.c:52-66): a check of HipSampler.loglike that does not pass through the CPU oracle at all.
Only tests/golden/ is read; the data is the workload's, in the units the fixture names."""
import numpy as np
import pytest

from apemost_amd.sampler import HipSampler
from oracle import ref_build as rb      # the list of cases and their inputs only: nothing here is compiled or run

pytestmark = pytest.mark.gpu


def _table(text):
    return np.array([[float(v) for v in line.split("\t")] for line in text.decode().splitlines()])


@pytest.mark.parametrize("waves", [1, 4])
@pytest.mark.parametrize("case", ["eval_pulse", "eval_pulse_vrot"])
def test_loglike_matches_recorded_eval_main(case, waves, golden_dir):
    """prob and prior of pulse and pulse_vrot at beta = 1 against eval_main's "%.15e" output, rel 1e-12 (the
    likelihood gate; the print itself rounds at 5e-16): 24 points across the box and five
    each at frequencies x 1e+-30 with heights and data x 1e+-200, 1100 points of data (ragged), one and four
    waves per chain.  With every height zero the reference aborts in gsl_sf_log(0) and printed nothing
    (recorded exit status -6); the device must give NaN there, ln 0 + d / 0."""
    fx = rb.read_bundle(rb.fixture_path(golden_dir, case))
    for name, sf, sh in rb.EVAL_UNITS:
        w, data = rb.eval_units(case, sf, sh)
        points = _table(fx["points_%s.txt" % name])
        s = HipSampler(w.model, w.n_par, 2, data, waves_per_chain=waves)
        prob, prior = s.loglike(points, np.ones(len(points)))
        s.close()
        if name == "heights_zero":
            assert fx["eval_%s.out" % name] == b""
            assert np.all(np.isnan(prob)), prob
            continue
        want = _table(fx["eval_%s.out" % name])
        assert want.shape == (len(points), 2) and np.all(np.isfinite(want))
        rel = np.max(np.abs(prob - want[:, 0]) / np.abs(want[:, 0]))
        print("%s %s waves=%d: max rel error of prob %.3g" % (case, name, waves, rel))
        np.testing.assert_allclose(prob, want[:, 0], rtol=1e-12, atol=0, err_msg="%s %d" % (name, waves))
        np.testing.assert_allclose(prior, want[:, 1], rtol=1e-12, atol=0, err_msg="%s %d" % (name, waves))
