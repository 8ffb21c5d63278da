"""Ragged ladder batches (apemost_hip_create_batch_ragged, include/apemost_hip.h) without a device: the
entry points exist, every argument error and every refusal comes back before a device is touched, the data layout is
the prefix sum the header states, and the Python objects of a ragged fold trim per ladder and refuse to reduce over
their padding."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from apemost_amd.pointwise import STATE, Pointwise
from apemost_amd.predict import Predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("apemost_hip_create_batch_ragged", "apemost_hip_ladder_n_data", "apemost_hip_predict_lengths",
       "apemost_hip_pointwise_lengths", "apemost_hip_ragged_layout")


def test_the_header_declares_the_library_exports_and_capi_binds_the_new_entry_points():
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in capi.EXPORTS, name
        assert getattr(L, name).argtypes is not None, name
    assert "#define APEMOST_HIP_ABI_VERSION 3" in header and capi.ABI_VERSION == 3


def config(**kw):
    w = wl.simplesin(n_data=64, n_chain=4)
    c = dict(abi_version=capi.ABI_VERSION, device=0, model=w.model, n_par=w.n_par, n_chains=4, n_data=-7, n_cols=2,
             n_chains_global=4, sigma=0.5, hmin=1e-6)
    c.update(kw)
    return capi.Config(**c)


def create(cfg, lengths, seeds=(1, 2, 3)):
    """(return code, last error) of create_batch_ragged; lengths / seeds None: a NULL pointer"""
    L = capi.lib()
    h = C.c_void_p()
    n = len(seeds) if seeds is not None else len(lengths)
    sp = None if seeds is None else (C.c_uint64 * n)(*seeds)
    lp = None if lengths is None else (C.c_int32 * len(lengths))(*lengths)
    rc = L.apemost_hip_create_batch_ragged(C.byref(cfg), n, sp, lp, C.byref(h))
    if rc == capi.OK:                                    # (a machine with a device)
        L.apemost_hip_destroy(h)
    else:
        assert not h.value
    return rc, L.apemost_hip_last_error().decode()


def test_argument_errors_come_back_before_any_device_is_touched():
    rc, msg = create(config(), None)
    assert rc == capi.ERR_INVALID and "n_data is NULL" in msg
    for bad in ([64, 0, 64], [64, 65, -1]):
        rc, msg = create(config(), bad)
        assert rc == capi.ERR_INVALID and "at least 1 row" in msg, msg
    # 10000 ladders of 2^31 - 1 rows of 65535 columns: 1.4e18 doubles, beyond the 2^60 the allocation's arithmetic takes
    n = 10000
    rc, msg = create(config(n_chains=1, n_chains_global=1, n_cols=65535), [2 ** 31 - 1] * n, seeds=list(range(n)))
    assert rc == capi.ERR_INVALID and "overflow" in msg, msg
    L = capi.lib()
    h = C.c_void_p()
    assert L.apemost_hip_create_batch_ragged(None, 1, None, None, C.byref(h)) == capi.ERR_INVALID
    n_data = C.c_int32(0)
    assert L.apemost_hip_ladder_n_data(None, 0, C.byref(n_data)) == capi.ERR_INVALID
    assert L.apemost_hip_predict_lengths(None, None) == capi.ERR_INVALID
    assert L.apemost_hip_pointwise_lengths(None, None) == capi.ERR_INVALID


@pytest.mark.parametrize("kw,code,needle", [
    (dict(model=wl.MODEL_USER, device_model_source=b"x.h"), capi.ERR_UNSUPPORTED, "user-supplied"),
    (dict(flags=capi.FLAG_RANDOMSWAP), capi.ERR_UNSUPPORTED, "RANDOMSWAP"),
    (dict(flags=capi.FLAG_ADAPT), capi.ERR_UNSUPPORTED, "ADAPT"),
    (dict(flags=capi.FLAG_RWM), capi.ERR_UNSUPPORTED, "RWM"),
    (dict(flags=capi.FLAG_TEST_REFUSE_COOPERATIVE), capi.ERR_UNSUPPORTED, "TEST_REFUSE_COOPERATIVE"),
    (dict(flags=capi.FLAG_TEST_WITHHOLD_PUBLISH), capi.ERR_UNSUPPORTED, "TEST_WITHHOLD_PUBLISH"),
    (dict(flags=capi.FLAG_COOPERATIVE_LAUNCH), capi.ERR_UNSUPPORTED, "COOPERATIVE_LAUNCH"),
    (dict(flags=capi.FLAG_USER_ONE_BARRIER), capi.ERR_UNSUPPORTED, "USER_ONE_BARRIER"),
    (dict(chain_offset=1, n_chains_global=8), capi.ERR_UNSUPPORTED, "not sharded"),
    (dict(n_chains_global=8), capi.ERR_UNSUPPORTED, "not sharded"),
    (dict(abi_version=2), capi.ERR_INVALID, "ABI version"),
    (dict(n_chains=0, n_chains_global=0), capi.ERR_INVALID, "chains in all"),
    (dict(n_chains=1000000, n_chains_global=1000000), capi.ERR_INVALID, "chains in all"),
    (dict(waves_per_chain=6), capi.ERR_INVALID, "1, 2, 4 or 8 waves"),
    (dict(n_par=5), capi.ERR_INVALID, "n_par = 4"),
    (dict(n_cols=1), capi.ERR_INVALID, "n_cols"),
    (dict(flags=1 << 20), capi.ERR_INVALID, "unknown bits"),
])
def test_every_refusal_of_create_batch_comes_back_from_create_batch_ragged(kw, code, needle):
    rc, msg = create(config(**kw), [1, 65, 64])
    if rc == capi.ERR_NO_DEVICE:     # (waves_per_chain 6 is found behind the device check, like in create_batch)
        assert needle == "1, 2, 4 or 8 waves"
        return
    assert rc == code and needle in msg, (rc, msg)


def test_seeds_are_needed_as_for_create_batch():
    rc, msg = create(config(), [1, 65, 64], seeds=None)
    assert rc == capi.ERR_INVALID and "seeds" in msg


def test_without_a_device_creation_is_an_error():
    """(where there is one, the same call makes a sampler)"""
    have = capi.lib().apemost_hip_device_info(0, None, 0, None, None) == capi.OK
    rc, msg = create(config(), [1, 65, 64])
    if have:
        assert rc == capi.OK, msg
    else:
        assert rc == capi.ERR_NO_DEVICE and msg


@pytest.mark.parametrize("n_cols", [2, 3])
def test_the_layout_is_the_prefix_sum_of_n_cols_times_n_data(n_cols):
    lengths = [1, 65, 64]
    off, longest, total = capi.ragged_layout(lengths, n_cols)
    assert off.tolist() == [0, n_cols, 66 * n_cols, 130 * n_cols] and longest == 65 and total == 130 * n_cols
    assert off.tolist() == np.concatenate([[0], np.cumsum(np.multiply(lengths, n_cols))]).tolist()
    # odd lengths put the next ladder at an odd offset: 8-byte alignment is all a ladder's matrix has
    assert off[1] % 2 == n_cols % 2
    equal, longest, total = capi.ragged_layout([7, 7, 7], n_cols)
    assert equal.tolist() == [b * n_cols * 7 for b in range(4)] and longest == 7     # create_batch's own layout
    with pytest.raises(capi.ApemostHipError) as e:
        capi.ragged_layout([3, 0], n_cols)
    assert e.value.code == capi.ERR_INVALID


# ---- the Python objects of a ragged fold, built by hand -----------------------------------------------------------
LENGTHS = np.array([1, 5, 3], dtype=np.int32)


def ragged_predict(nbins=4):
    k, n_x = len(LENGTHS), int(LENGTHS.max())
    rs = np.random.RandomState(3)
    x = np.zeros((k, n_x))
    pr = Predict.empty([0, 4, 8], x, 4, wl.MODEL_SIMPLESIN, nbins, -2.0, 2.0, 1, n_ladders=k)
    pr.n[0] = 10
    for j, m in enumerate(LENGTHS):
        pr.x[j, :m] = np.sort(rs.uniform(0, 1, m))
        for f in ("origin", "sum", "sq", "vmin", "vmax"):
            getattr(pr, f)[j, :m] = rs.normal(size=m)
        pr.hist[j, :m] = rs.randint(0, 5, size=(m, nbins))
    pr.lengths = LENGTHS.copy()
    return pr


def ragged_pointwise():
    k, n = len(LENGTHS), int(LENGTHS.max())
    rs = np.random.RandomState(4)
    pw = Pointwise.empty([0, 4, 8], np.zeros((k, n)), np.zeros((k, n)), 4, wl.MODEL_SIMPLESIN, 0.5, 1, n_ladders=k)
    pw.n[0] = 10
    for j, m in enumerate(LENGTHS):
        pw.x[j, :m], pw.y[j, :m] = rs.uniform(0, 1, m), rs.normal(size=m)
        for f in STATE:
            getattr(pw, f)[j, :m] = rs.uniform(0.5, 2.0, size=m)
        pw.at_mean[j, :m] = rs.normal(size=m)
    pw.lengths = LENGTHS.copy()
    return pw


def test_predict_per_ladder_trims_by_lengths_and_the_ragged_object_refuses_to_reduce():
    pr = ragged_predict()
    assert pr.is_ragged()
    lads = pr.per_ladder()
    assert [p.n_x for p in lads] == LENGTHS.tolist()
    for b, p in enumerate(lads):
        m = LENGTHS[b]
        assert p.lengths is None and not p.is_ragged() and p.n_keep == 1 and p.n_ladders == 1
        for f in ("x", "origin", "sum", "sq", "vmin", "vmax", "hist"):
            assert np.array_equal(getattr(p, f)[0], getattr(pr, f)[b, :m]), (b, f)
        y = np.zeros(m)
        assert np.isfinite(p.chi2(y, 0.5)) and len(p.text(y).splitlines()) == m     # every method works on it
        assert p.mean().shape == (m,) and p.median().shape == (m,)
    y = np.zeros(pr.n_x)
    for call in (lambda: pr.chi2(y, 0.5), lambda: pr.text(y), lambda: pr.write(os.devnull)):
        with pytest.raises(ValueError, match=r"per_ladder\(\)"):
            call()
    # the padding holds the initial values
    for b, m in enumerate(LENGTHS):
        assert not pr.sum[b, m:].any() and not pr.hist[b, m:].any()
        assert np.all(pr.vmin[b, m:] == np.inf) and np.all(pr.vmax[b, m:] == -np.inf)


def test_pointwise_per_ladder_trims_by_lengths_and_the_ragged_object_refuses_to_reduce(tmp_path):
    pw = ragged_pointwise()
    assert pw.is_ragged()
    lads = pw.per_ladder()
    assert [p.n_data for p in lads] == LENGTHS.tolist()
    for b, p in enumerate(lads):
        m = LENGTHS[b]
        assert p.lengths is None and not p.is_ragged()
        for f in STATE + ("x", "y", "at_mean"):
            assert np.array_equal(getattr(p, f)[0], getattr(pw, f)[b, :m]), (b, f)
        assert set(p.criteria()) and len(p.text().splitlines()) == m
        p.write(str(tmp_path / "pointwise.bin"))
        assert Pointwise.read(str(tmp_path / "pointwise.bin")).n_data == m
    other = ragged_pointwise()
    for name, call in [("lppd", pw.lppd), ("elpd_waic", pw.elpd_waic), ("elpd_loo", pw.elpd_loo),
                       ("waic", pw.waic), ("waic_se", pw.waic_se), ("looic", pw.looic), ("p_waic", pw.p_waic),
                       ("p_loo", pw.p_loo), ("p_dic", pw.p_dic), ("dic", pw.dic), ("compare", lambda: pw.compare(other)),
                       ("compare", lambda: lads[0].compare(other)), ("criteria", pw.criteria), ("text", pw.text),
                       ("write", lambda: pw.write(os.devnull))]:
        with pytest.raises(ValueError, match=r"per_ladder\(\)"):
            call()


def test_objects_without_lengths_or_with_equal_lengths_are_what_they_were():
    pr, pw = ragged_predict(), ragged_pointwise()
    for o, width in ((pr, pr.n_x), (pw, pw.n_data)):
        o.lengths = None
        assert not o.is_ragged() and [p.x.shape[1] for p in o.per_ladder()] == [width] * 3
        o.lengths = np.full(3, width, dtype=np.int32)
        assert not o.is_ragged() and [p.x.shape[1] for p in o.per_ladder()] == [width] * 3
    pw.waic(), pw.criteria(), pr.chi2(np.zeros(pr.n_x), 0.5), pr.text(np.zeros(pr.n_x))     # nothing raises
