"""What the held-out fold and K-fold cross-validation promise without a card: the ABI surface, the refusals that need no
device, apemost_amd/kfold.py (numpy), the restatement of the joint sum (tests/kfold_ref.py) and the header's summation
helpers built by the host compiler under the sanitizers (tests/joint_check.cpp, a program of its own)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi, kfold
from apemost_amd.pointwise import Pointwise
from apemost_amd.psis import Psis
from tests.kfold_ref import RefJoint, joint_sum

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "apemost_amd", "csrc")
NAMES = ["apemost_hip_pointwise_begin_at", "apemost_hip_pointwise_joint_get", "apemost_hip_pointwise_joint_set",
         "apemost_hip_pointwise_loglike_at"]


def bits(v):
    return np.float64(v).view(np.uint64)


# ---- the ABI ----------------------------------------------------------------------------------------------------------
def test_symbols_are_exported_and_declared():
    build.build_hip()
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS and getattr(L, name) is not None and ("int %s(" % name) in header, name
    assert "} apemost_hip_pointwise_at;" in header and "} apemost_hip_pointwise_joint_view;" in header
    assert "#define APEMOST_HIP_ABI_VERSION 3" in header and L.apemost_hip_abi_version() == 3
    assert [f for f, _ in capi.PointwiseAt._fields_] == ["n_at", "x", "y", "joint"]
    assert [f for f, _ in capi.PointwiseJointView._fields_] == ["n", "origin", "sum", "sq", "m", "S"]


def test_a_null_sampler_is_refused_by_every_new_entry_point():
    build.build_hip()
    L = capi.lib()
    ch, n_at, v = np.zeros(1, dtype=np.int32), np.ones(1, dtype=np.int32), np.zeros(1)
    cfg = capi.PointwiseConfig(n_keep=1, chains=ch.ctypes.data_as(C.POINTER(C.c_int32)))
    dp = v.ctypes.data_as(capi._dp)
    at = capi.PointwiseAt(n_at=n_at.ctypes.data_as(C.POINTER(C.c_int32)), x=dp, y=dp, joint=1)
    jt = kfold.Joint.empty((0,), (1,))
    for rc in (L.apemost_hip_pointwise_begin_at(None, C.byref(cfg), C.byref(at)),
               L.apemost_hip_pointwise_joint_get(None, C.byref(jt.view())),
               L.apemost_hip_pointwise_joint_set(None, C.byref(jt.view())),
               L.apemost_hip_pointwise_loglike_at(None, 1, dp, 1, dp, dp, dp)):
        assert rc == capi.ERR_INVALID and b"sampler is NULL" in L.apemost_hip_last_error()


# ---- kfold.folds and training_sets ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scheme", kfold.SCHEMES)
@pytest.mark.parametrize("n_data", [1, 2, 7, 64, 65])
def test_folds_partition_the_data(scheme, n_data):
    for k in sorted({1, 2, 3, n_data}):
        if k > n_data:
            with pytest.raises(ValueError):
                kfold.folds(n_data, k, scheme, seed=3)
            continue
        fs = kfold.folds(n_data, k, scheme, seed=3)
        assert len(fs) == k and all(len(f) >= 1 for f in fs)
        assert all(np.array_equal(f, np.sort(f)) for f in fs)
        assert np.array_equal(np.sort(np.concatenate(fs)), np.arange(n_data))
        sizes = [len(f) for f in fs]
        assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
        if scheme == "interleaved":
            assert all((f % k == b).all() for b, f in enumerate(fs))
        if scheme == "blocks":
            assert all((np.diff(f) == 1).all() for f in fs) and np.array_equal(np.concatenate(fs), np.arange(n_data))
    with pytest.raises(ValueError):
        kfold.folds(n_data, n_data + 1, scheme)
    with pytest.raises(ValueError):
        kfold.folds(n_data, 0, scheme)


def test_random_folds_reproduce_per_seed_and_schemes_are_checked():
    a, b, c = (kfold.folds(65, 4, "random", seed=s) for s in (11, 11, 12))
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    assert not all(np.array_equal(x, y) for x, y in zip(a, c))
    assert not all(np.array_equal(x, y) for x, y in zip(a, kfold.folds(65, 4, "blocks")))
    with pytest.raises(ValueError):
        kfold.folds(10, 2, "stratified")


def test_training_sets_keep_the_row_order():
    data = np.stack([np.arange(10.0), 100 + np.arange(10.0)], 1)
    fs = kfold.folds(10, 3)
    assert [f.tolist() for f in fs] == [[0, 3, 6, 9], [1, 4, 7], [2, 5, 8]]
    sets = kfold.training_sets(data, fs)
    assert [len(m) for m in sets] == [6, 7, 7]
    assert sets[0][:, 0].tolist() == [1, 2, 4, 5, 7, 8] and sets[2][:, 1].tolist() == [100, 101, 103, 104, 106, 107, 109]
    with pytest.raises(ValueError):
        kfold.training_sets(data, [fs[0], fs[1]])
    with pytest.raises(ValueError):
        kfold.training_sets(data, [fs[0], fs[1], fs[1]])


# ---- KFold from a hand-made state -------------------------------------------------------------------------------------
def hand_made():
    """7 data in 3 interleaved folds (3, 2, 2 rows), 4 kept samples: S_up = 4 exp(0) = n, so elpd_i = m_up exactly"""
    data = np.stack([10 + np.arange(7.0), -np.arange(7.0)], 1)
    fs = kfold.folds(7, 3)
    x = np.zeros((3, 3))
    y = np.zeros((3, 3))
    m_up = np.zeros((3, 3))
    for b, f in enumerate(fs):
        x[b, :len(f)], y[b, :len(f)] = data[f, 0], data[f, 1]
        m_up[b, :len(f)] = -0.5 * (1 + f)
    S_up = np.where(x != 0, 4.0, 0.0)
    z = np.zeros((3, 3))
    pw = Pointwise([4], z, z, z, m_up, S_up, z, z, z, np.zeros((3, 2)), np.zeros((3, 2)), [0, 4, 8], x, y, 2, 0, n_ladders=3)
    pw.lengths = np.array([3, 2, 2], dtype=np.int32)
    pw.heldout = True
    jt = kfold.Joint([4], [-3.0, -2.0, -1.0], [2.0, 4.0, 0.0], [3.0, 4.0, 0.0], [-2.5, -1.5, -1.0], [2.0, 4.0, 4.0],
                     [0, 4, 8], [3, 2, 2])
    return data, fs, pw, jt


def test_kfold_scatters_back_to_the_original_order():
    data, fs, pw, jt = hand_made()
    cv = kfold.KFold.from_state(pw, jt, fs)
    assert cv.n == 4 and cv.k == 3 and cv.n_data == 7 and cv.has_joint
    assert cv.elpd_i.tolist() == [-0.5 * (1 + i) for i in range(7)]
    assert cv.x.tolist() == data[:, 0].tolist() and cv.y.tolist() == data[:, 1].tolist()
    assert cv.fold_of.tolist() == [0, 1, 2, 0, 1, 2, 0] and all(np.array_equal(a, b) for a, b in zip(cv.folds(), fs))
    assert cv.elpd == -14.0
    e = cv.elpd_i
    assert cv.se == pytest.approx(math.sqrt(7 * e.var(ddof=1)), rel=1e-14)
    # lpd_joint = m + ln(S / n); joint_mean = origin + sum / n; joint_var = (sq - sum^2 / n) / (n - 1), never below 0
    assert cv.lpd_joint.tolist() == [-2.5 + math.log(0.5), -1.5, -1.0]
    assert cv.joint_mean.tolist() == [-2.5, -1.0, -1.0]
    assert cv.joint_var.tolist() == [(3.0 - 1.0) / 3, 0.0, 0.0]
    with pytest.raises(ValueError):
        kfold.KFold.from_state(pw, jt, [fs[0], fs[2], fs[1]][:2])
    with pytest.raises(ValueError):
        kfold.KFold.from_state(pw, jt, [fs[0][:2], fs[1], np.concatenate([fs[2], fs[0][2:]])])
    with pytest.raises(ValueError, match="held-out"):
        pw.per_ladder()[0].dic()
    none = kfold.KFold.from_state(pw, None, fs)
    assert not none.has_joint and np.isnan(none.lpd_joint).all() and none.elpd == cv.elpd


def test_kfold_compare_write_and_read(tmp_path):
    data, fs, pw, jt = hand_made()
    cv = kfold.KFold.from_state(pw, jt, fs)
    other = kfold.KFold(4, cv.x, cv.y, cv.elpd_i + np.array([0.5, 0.25, 0.5, 0.25, 0.5, 0.25, 0.5]), cv.fold_of)
    d = cv.elpd_i - other.elpd_i
    diff, se = cv.compare(other)
    assert diff == -2.75 and se == pytest.approx(math.sqrt(7 * d.var(ddof=1)), rel=1e-14)
    assert other.compare(cv)[0] == 2.75
    ps = Psis(4, other.elpd_i, np.zeros(7), np.zeros(7), np.ones(7), np.zeros(7, dtype=bool), other.elpd_i, cv.x, cv.y)
    assert cv.compare(ps) == (diff, se)
    z = np.zeros((1, 7))
    loo = Pointwise([4], z, z, z, z, z, -(other.elpd_i.reshape(1, 7)), z + 4.0, z, np.zeros((1, 2)), np.zeros((1, 2)), [0],
                    cv.x, cv.y, 2, 0)
    assert loo.elpd_loo().tolist() == other.elpd_i.tolist() and cv.compare(loo) == (diff, se)
    moved = kfold.KFold(4, cv.x + 1.0, cv.y, cv.elpd_i, cv.fold_of)
    with pytest.raises(ValueError, match="same data"):
        cv.compare(moved)
    with pytest.raises(ValueError, match="same data"):
        cv.compare(kfold.KFold(4, cv.x[:6], cv.y[:6], cv.elpd_i[:6], cv.fold_of[:6]))
    path = str(tmp_path / "kfold.bin")
    for one in (cv, other):
        one.write(path)
        back = kfold.KFold.read(path)
        assert back.text() == one.text() and back.has_joint == one.has_joint and (back.n, back.k, back.thin) == (4, 3, 1)
        for f in ("x", "y", "elpd_i", "fold_of", "lpd_joint", "joint_mean", "joint_var"):
            assert getattr(back, f).tobytes() == getattr(one, f).tobytes(), f
    lines = cv.text().split("\n")
    assert lines[0] == "n\t4" and lines[2].startswith("elpd\t-1.4") and len(lines) == 4 + 3 + 7 + 1
    open(path, "wb").write(open(path, "rb").read()[:-8])
    with pytest.raises(ValueError):
        kfold.KFold.read(path)


# ---- the joint sum ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 63, 64, 65, 130])
def test_joint_sum_of_small_integers_is_exact(L):
    terms = np.random.default_rng(L).integers(-1000, 1000, size=(3, L)).astype(np.float64)
    got = joint_sum(terms)
    assert got.shape == (3,) and got.tolist() == [math.fsum(t) for t in terms.tolist()]
    assert joint_sum(terms[1]) == got[1]


def test_joint_sum_follows_the_rule_where_the_order_matters():
    """3 terms over 2 lanes of 64: a = 1, b = 2^-53, c = 2^-53 at i = 0, 1, 64.  Lane 0 holds (0 + a) + c = 1 (the
    half ulp rounds to even), lane 1 holds b, and the tree gives 1 + 2^-53 = 1.  Left to right in another association,
    a + (b + c) = 1 + 2^-52: the next double."""
    a, h = 1.0, 2.0 ** -53
    terms = np.zeros(65)
    terms[0], terms[1], terms[64] = a, h, h
    assert joint_sum(terms) == 1.0 and a + (h + h) == 1.0 + 2.0 ** -52
    # and where a left-to-right sum loses what the lanes keep: i = 0 and i = 1 are added to each other only in the tree
    big = np.array([2.0 ** 53, 1.0, 1.0] + [0.0] * 61 + [-(2.0 ** 53)])      # lane 0: (2^53) + (-2^53) = 0
    left = 0.0
    for v in big.tolist():
        left = left + v
    assert joint_sum(big) == 2.0 and left == 0.0
    assert bits(joint_sum(np.array([-0.0]))) == bits(0.0)         # +0.0 + -0.0 is +0.0: the lane partial starts at +0.0
    assert np.isnan(joint_sum(np.array([1.0, np.nan, 2.0]))) and joint_sum(np.array([np.inf, 1.0])) == np.inf


def test_ref_joint_is_the_sequential_fold():
    J = [-3.0, -1.0, -2.0, -1.0]
    r = RefJoint(J)
    assert (r.n, r.origin, r.sum, r.sq, r.m) == (4, -3.0, 0.0 + 2.0 + 1.0 + 2.0, 4.0 + 1.0 + 4.0, -1.0)
    assert r.S == (1.0 * math.exp(-2.0) + 1.0) + math.exp(-1.0) + 1.0
    assert r.S_exact == pytest.approx(r.S, rel=1e-14) and r.lpd() == r.m + math.log(r.S / 4)
    assert RefJoint([2.5]).S == 1.0 and RefJoint([2.5]).sum == 0.0 and math.isnan(RefJoint([1.0, math.nan]).S)


def test_helpers_built_by_the_host_compiler_under_the_sanitizers(tmp_path):
    """joint_lane_partials and joint_tree_sum of pt_pointwise_joint.h, compiled for the host: the bits of J equal
    joint_sum's for every length the kernels treat differently, with terms of mixed magnitude and sign, zeros of both
    signs and non-finite values"""
    rng = np.random.default_rng(9)
    blocks = []
    for L in (1, 2, 3, 63, 64, 65, 127, 128, 129, 130, 1000):
        t = rng.standard_normal(L) * 10.0 ** rng.integers(-8, 9, L)
        blocks.append(t)
    blocks += [np.array([-0.0]), np.array([-0.0, -0.0]), np.array([1.0, np.inf, -3.0]), np.array([np.nan] + [1.0] * 70),
               np.array([1e308] * 3), np.array([2.0 ** 53, 1.0, 1.0] + [0.0] * 61 + [-(2.0 ** 53)])]
    src = tmp_path / "terms.txt"
    src.write_text("".join(" ".join("%016x" % int(b) for b in t.view(np.uint64)) + "\n" for t in blocks))
    exe = str(tmp_path / "joint_check")
    subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(HERE, "joint_check.cpp"), "-o", exe])
    run = subprocess.run([exe, str(src)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True,
                         timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    got = [int(w, 16) for w in run.stdout.split()]
    assert len(got) == len(blocks)
    for t, g in zip(blocks, got):
        want = joint_sum(t)
        if math.isnan(want):
            assert math.isnan(np.uint64(g).view(np.float64)), len(t)
        else:
            assert g == int(bits(want)), (len(t), g, want)
