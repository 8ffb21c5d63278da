"""Ladder batches (apemost_hip_create_batch, include/apemost_hip.h) -- what can be checked without a GPU: the three
entry points are declared, exported and bound; what a batch cannot do is refused before any device is touched;
ladder_view slices ladder-major arrays; gelman_rubin is the classic between/within form."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi, workloads as wl
from apemost_amd.sampler import HipSampler, ladder_view
from apemost_amd.summary import RunSummary, gelman_rubin, ladder_evidences

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("apemost_hip_create_batch", "apemost_hip_n_ladders", "apemost_hip_set_data_ladder")


def test_header_declares_library_exports_and_capi_binds_the_entry_points():
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    build.build_hip()
    nm = subprocess.check_output(["nm", "-D", "--defined-only", build.HIP_LIB]).decode()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert re.search(r" T %s$" % name, nm, re.M), name
        assert name in capi.EXPORTS and getattr(L, name).argtypes, name
    assert "#define APEMOST_HIP_ABI_VERSION 3" in header          # entry points were added, no layout changed


def _cfg(**kw):
    base = dict(abi_version=capi.ABI_VERSION, device=0, model=wl.MODEL_SIMPLESIN, n_par=4, n_chains=4, n_data=16,
                n_cols=2, waves_per_chain=0, lds_policy=0, flags=0, chain_offset=0, n_chains_global=4, seed=1,
                sigma=0.5, hmin=1e-6)
    base.update(kw)
    return capi.Config(**base)


def _create_batch(cfg, seeds):
    build.build_hip()
    L = capi.lib()
    h = C.c_void_p()
    arr = (C.c_uint64 * max(len(seeds), 1))(*seeds) if seeds is not None else None
    rc = L.apemost_hip_create_batch(C.byref(cfg), len(seeds) if seeds is not None else 2, arr, C.byref(h))
    msg = L.apemost_hip_last_error().decode()
    assert rc != capi.OK or h.value
    if rc == capi.OK:
        L.apemost_hip_destroy(h)
    else:
        assert not h.value                       # no sampler is left behind
    return rc, msg


REFUSED = [
    (dict(model=wl.MODEL_USER, n_par=2, device_model_source=b"/nonexistent.hip"), "user-supplied"),
    (dict(flags=capi.FLAG_RANDOMSWAP), "RANDOMSWAP"),
    (dict(flags=capi.FLAG_ADAPT), "ADAPT"),
    (dict(flags=capi.FLAG_RWM), "RWM"),
    (dict(flags=capi.FLAG_TEST_REFUSE_COOPERATIVE), "TEST_REFUSE_COOPERATIVE"),
    (dict(flags=capi.FLAG_TEST_WITHHOLD_PUBLISH), "TEST_WITHHOLD_PUBLISH"),
    (dict(flags=capi.FLAG_COOPERATIVE_LAUNCH), "COOPERATIVE_LAUNCH"),
    (dict(flags=capi.FLAG_SWAP_EVEN_ODD | capi.FLAG_ADAPT), "ADAPT"),
    (dict(chain_offset=1, n_chains_global=5), "not sharded"),
    (dict(n_chains_global=8), "not sharded"),
]


@pytest.mark.parametrize("kw,needle", REFUSED)
def test_create_batch_refuses_what_a_batch_cannot_do_before_any_device_is_touched(kw, needle):
    """ERR_UNSUPPORTED and a message, on a machine with or without a GPU: the refusal comes first"""
    rc, msg = _create_batch(_cfg(**kw), [5, 6, 7])
    assert rc == capi.ERR_UNSUPPORTED and needle in msg and "create_batch" in msg, (rc, msg)


@pytest.mark.parametrize("cfg_kw,seeds,needle", [
    (dict(), [], "n_ladders"),
    (dict(), None, "seeds"),
    (dict(abi_version=99), [1, 2], "ABI version"),
    (dict(n_chains=0, n_chains_global=0), [1, 2], "chains"),
    (dict(n_chains=1500000, n_chains_global=1500000), [1, 2], "2000000"),
])
def test_create_batch_rejects_bad_arguments(cfg_kw, seeds, needle):
    rc, msg = _create_batch(_cfg(**cfg_kw), seeds)
    assert rc == capi.ERR_INVALID and needle in msg, (rc, msg)


def test_without_a_device_a_batch_is_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    rc, msg = _create_batch(_cfg(), [1, 2, 3])
    assert rc == capi.ERR_NO_DEVICE and "no HIP device" in msg
    with pytest.raises(capi.ApemostHipError):
        HipSampler.batch(wl.MODEL_SIMPLESIN, 4, 2, np.zeros((8, 2)), seeds=[1, 2])


def test_python_mirror_refuses_through_the_library():
    with pytest.raises(capi.ApemostHipError, match="RWM") as e:
        HipSampler(wl.MODEL_SIMPLESIN, 4, 2, np.zeros((8, 2)), seeds=[1, 2], flags=capi.FLAG_RWM)
    assert e.value.code == capi.ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="one matrix per ladder"):
        HipSampler.batch(wl.MODEL_SIMPLESIN, 4, 2, np.zeros((3, 8, 2)), seeds=[1, 2])


def test_sharded_ladder_refuses_a_batch():
    from apemost_amd.distributed import ShardedLadder

    class Engine:
        flags, n_ladders = 0, 3
    with pytest.raises(ValueError, match="ladder batch"):
        ShardedLadder(Engine(), 4, 0, 4, 0, 1)
    Engine.n_ladders = 1
    ShardedLadder(Engine(), 4, 0, 4, 0, 1)


def test_ladder_view_round_trips():
    n_ladders, per, n_par, n_steps = 3, 4, 5, 7
    rs = np.random.RandomState(2)
    rows = rs.normal(size=(n_steps, n_ladders * per, n_par + 2))
    params = rs.normal(size=(n_ladders * per, n_par))
    prob = rs.normal(size=n_ladders * per)
    for arr, axis in ((rows, 1), (params, 0), (prob, 0)):
        parts = [ladder_view(arr, b, n_ladders) for b in range(n_ladders)]
        assert all(p.shape[axis] == per for p in parts)
        assert np.array_equal(np.concatenate(parts, axis=axis), arr)
        assert np.shares_memory(parts[1], arr)                                 # views: writing a ladder writes the batch
    assert np.array_equal(ladder_view(rows, 2, n_ladders)[:, 1], rows[:, 2 * per + 1])
    assert np.array_equal(ladder_view(prob, 0, 1), prob)
    for bad in ((rows, 3, 3), (rows, -1, 3), (rows, 0, 5), (prob, 0, 0)):
        with pytest.raises(ValueError):
            ladder_view(*bad)


def test_gelman_rubin_is_about_one_for_one_normal_and_above_for_a_shifted_replica():
    """m = 8 replicas of n = 4000 independent N(0, 1) draws per parameter; thresholds from the formula itself.
    R-hat^2 = (n-1)/n + (B/n)/W.  The replica means have variance 1/n, so B/n, their sample variance over m, has
    expectation 1/n and relative standard deviation sqrt(2/(m-1)) = 0.53; W = 1 +- sqrt(2/(m n)) = 0.8 %.  Hence
    R-hat^2 = 1 + 0.53 z / n and R-hat - 1 = 6.7e-5 z with z of unit variance: "about 1" is asserted as
    |R-hat - 1| < 1e-3, fifteen standard deviations and a tenth of the conventional 1.01 threshold.
    One replica's mean shifted by d = 1: the sample variance of m means of which one is d and the others 0 is
    d^2/m = 0.125 while W stays 1, so R-hat = sqrt(1.125) = 1.0607; the cross term with the noise of the means is
    2 d / (m sqrt(n)) = 0.004 in R-hat^2, 0.002 in R-hat.  Asserted: within 0.01 of 1.0607 (five of those) and
    above 1.05, for the shifted parameter and chain only."""
    m, per, n, n_par = 8, 3, 4000, 2
    rs = np.random.RandomState(5)
    rows = rs.normal(size=(n, m * per, n_par + 2))
    r = gelman_rubin(rows, m)
    assert r.shape == (n_par,) and np.all(np.abs(r - 1) < 1e-3), r
    assert np.all(np.abs(gelman_rubin(rows, m, chain=2) - 1) < 1e-3)
    shifted = rows.copy()
    shifted[:, 5 * per + 0, 1] += 1.0                    # replica 5, its beta = 1 chain, parameter 1
    r2 = gelman_rubin(shifted, m)
    assert r2[1] > 1.05 and abs(r2[1] - np.sqrt(1.125)) < 0.01 and abs(r2[0] - 1) < 1e-3, r2
    assert np.all(np.abs(gelman_rubin(shifted, m, chain=1) - 1) < 1e-3)      # the other chains are untouched
    # the formula, written out
    x = shifted[:, 0::per, :n_par]
    w = np.mean([[np.var(x[:, j, p], ddof=1) for j in range(m)] for p in range(n_par)], axis=1)
    b_n = np.array([np.var([x[:, j, p].mean() for j in range(m)], ddof=1) for p in range(n_par)])
    np.testing.assert_allclose(r2, np.sqrt(((n - 1) / n * w + b_n) / w), rtol=1e-12)
    for bad in ((rows, 1), (rows, 5), (rows[:1], m)):
        with pytest.raises(ValueError):
            gelman_rubin(*bad)
    with pytest.raises(ValueError):
        gelman_rubin(rows, m, chain=per)


def test_evidence_per_ladder_is_the_existing_integrator_ladder_by_ladder():
    rs = np.random.RandomState(9)
    m, per, n = 3, 5, 100
    betas = np.tile(np.linspace(1.0, 0.1, per), m)
    prob_sum = rs.normal(-50 * n, 10, size=m * per)
    got = ladder_evidences(prob_sum, n, betas, m)
    for b in range(m):
        one = RunSummary(n, prob_sum[b * per:(b + 1) * per], np.zeros((0, 0, 0)), np.zeros((0, 0, 0)), 0, [], [], 1)
        assert got[b] == one.evidence(betas[b * per:(b + 1) * per])
    whole = RunSummary(n, prob_sum, np.zeros((0, 0, 0)), np.zeros((0, 0, 0)), 0, [], [], 1)
    assert np.array_equal(whole.evidence_per_ladder(betas, m), got) and got.std() > 0
    with pytest.raises(ValueError):
        ladder_evidences(prob_sum, n, betas, 4)
