"""tests/helpers.make_pair on ladders with a zero, a tiny or an equal beta (no GPU): the states every GPU
parity test starts from, and what the oracle does on them (tests/test_gpu_ladder_edges.py compares the
kernels with it)."""
import numpy as np
import pytest

from oracle import oracle as orc
from tests.helpers import make_pair, small_workloads


@pytest.mark.parametrize("name", ["simplesin", "pulse"])
def test_default_ladder_is_unchanged(name):
    """existing callers: chebyshev betas from beta_0 = 0.02, steps step0 * 0.3 * beta^-1/2 capped at the range"""
    w = small_workloads()[name]
    st, lad, _ = make_pair(w, 8, seed=3)
    for i in range(8):
        b = orc.get_chain_beta(orc.LADDER_CHEBYSHEV_BETA, i, 8, 0.02)
        assert st.beta[i] == b
        assert np.array_equal(st.step[i], np.minimum(w.step * 0.3 * b ** -0.5, w.pmax - w.pmin))
    assert np.array_equal(lad.beta, st.beta) and np.array_equal(lad.step, st.step)


def test_zero_and_tiny_betas_cap_the_step():
    w = small_workloads()["pulse"]
    st, lad, _ = make_pair(w, 8, beta_0=0.0, betas={6: 1e-310})
    assert st.beta[0] == 1.0 and st.beta[6] == 1e-310 and st.beta[7] == 0.0
    assert np.array_equal(st.step[7], w.pmax - w.pmin)       # beta^-1/2 infinite: the prior range
    assert np.array_equal(st.step[6], np.minimum(w.step * 0.3 * 1e-310 ** -0.5, w.pmax - w.pmin))
    assert np.all(np.isfinite(st.step)) and np.array_equal(lad.step, st.step)


def test_hot_chains_ladder_has_equal_betas():
    w = small_workloads()["sine3"]
    st, _, _ = make_pair(w, 8, beta_0=0.5, ladder_kind=orc.LADDER_HOT_CHAINS)
    assert np.all(st.beta == 0.5)
    assert np.array_equal(st.step, np.broadcast_to(np.minimum(w.step * 0.3 * 0.5 ** -0.5, w.pmax - w.pmin), st.step.shape))


@pytest.mark.parametrize("name", ["simplesin", "sine3", "pulse", "pulse_vrot"])
def test_oracle_moves_the_beta_zero_chain(name):
    """the reference at beta = 0 and 1e-310 samples the prior: those chains accept (all steps for the models
    without a prior, where prob_new == prob), and every recorded row is finite"""
    w = small_workloads()[name]
    st, lad, rng = make_pair(w, 8, seed=5, beta_0=0.0, betas={6: 1e-310})
    rows = orc.run_sampler(lad, rng, 40, 11, record=True)
    assert np.all(np.isfinite(rows))
    if name in ("simplesin", "sine3"):
        assert np.all(lad.accept[6:] == 440)
    else:
        assert np.all(lad.accept[6:] > 100) and np.all(lad.accept[6:] < 440)
