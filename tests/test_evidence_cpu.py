"""The evidence fold without a device (apemost_amd/evidence.py): the entry points exist, Evidence.from_rows equals the
restatement of tests/evidence_ref.py, evidence.bin round-trips, the rectangle rule restates RunSummary.evidence, and on
a Gaussian with a closed form the estimators land where their theory says."""
import math
import os
import re

import numpy as np
import pytest

from apemost_amd import build, capi
from apemost_amd.evidence import Evidence
from apemost_amd.summary import RunSummary, batches_closed
from tests.evidence_ref import RefEvidence, assert_equals

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["apemost_hip_evidence_begin", "apemost_hip_evidence_accumulate", "apemost_hip_evidence_get",
           "apemost_hip_evidence_set", "apemost_hip_evidence_end"]


def test_header_declares_and_library_exports_the_entry_points():
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTS and getattr(L, name).argtypes, name
    assert "apemost_hip_evidence_config;" in header and "apemost_hip_evidence_view;" in header
    assert re.search(r"#define APEMOST_HIP_ABI_VERSION 3\b", header)
    assert capi.ABI_VERSION == 3 and L.apemost_hip_abi_version() == 3
    csrc = os.path.join(ROOT, "apemost_amd", "csrc")
    assert '#include "pt_evidence.h"' in open(os.path.join(csrc, "apemost_hip.hip")).read()
    for f in ("pt_device.h", "pt_onebarrier.h", "pt_kernels.h", "apemost_model.hip"):    # the round kernels do not see it
        assert "evidence" not in open(os.path.join(csrc, f)).read(), f


def _rows(seed, n, betas):
    """rows [n][n_chains][6] whose last column is of the order of -10^3 with unit spread"""
    rng = np.random.default_rng(seed)
    rows = rng.uniform(-1, 1, (n, len(betas), 6))
    rows[:, :, 5] = np.asarray(betas) * (-1000.0 + rng.standard_normal((n, len(betas))))
    return rows


@pytest.mark.parametrize("n,bs", [(1, 1), (2, 2), (57, 1), (57, 7), (200, 14)])
def test_from_rows_equals_the_restatement(n, bs):
    betas = [1.0, 0.5, 0.2, 0.01, 1.0, 0.3, 0.1, 0.05]                  # two ladders of four
    rows = _rows(n, n, betas)
    ev = Evidence.from_rows(rows, betas, batch_size=bs, n_ladders=2)
    assert ev.max_batches == batches_closed(n, bs) == ev.n_batches
    ref = RefEvidence(rows[:, :, 5], ev.coef, bs, ev.max_batches)
    assert_equals(ev, ref, "from_rows %d/%d" % (n, bs))
    assert Evidence.from_rows(rows[:, :, 5], betas, batch_size=bs, n_ladders=2).S.tobytes() == ev.S.tobytes()
    up, down = ev.coef
    assert up[0] == 0 and up[4] == 0 and down[3] == -1 and down[7] == -1
    assert up[1] == (1.0 - 0.5) / 0.5 and down[1] == -(0.5 - 0.2) / 0.5 and up[5] == (1.0 - 0.3) / 0.3
    lads = ev.per_ladder()
    assert len(lads) == 2 and lads[1].betas.tolist() == betas[4:] and lads[1].S.tobytes() == ev.S[:, 4:].tobytes()
    back = Evidence.concat(lads)
    for f in ("origin", "sum", "sq", "batch", "m", "S", "coef", "betas"):
        assert getattr(back, f).tobytes() == getattr(ev, f).tobytes(), f


def test_files_round_trip(tmp_path):
    betas = [1.0, 0.4, 0.1]
    ev = Evidence.from_rows(_rows(3, 90, betas), betas, batch_size=9, max_batches=14, thin=5)
    path = str(tmp_path / "evidence.bin")
    ev.write(path)
    raw = open(path, "rb").read()
    assert raw[:8] == b"APEMOSTE" and len(raw) == 56 + 8 * (3 * 6 + 4 * 3 + 3 * 15)
    back = Evidence.read(path)
    back.write(str(tmp_path / "again.bin"))
    assert open(str(tmp_path / "again.bin"), "rb").read() == raw
    for f in ("n", "origin", "sum", "sq", "batch", "m", "S", "coef", "betas"):
        assert getattr(back, f).tobytes() == getattr(ev, f).tobytes() and getattr(back, f).shape == getattr(ev, f).shape, f
    assert (back.batch_size, back.max_batches, back.thin, back.n_ladders) == (9, 14, 5, 1)
    (tmp_path / "bad.bin").write_bytes(b"APEMOSTJ" + raw[8:])
    with pytest.raises(ValueError):
        Evidence.read(str(tmp_path / "bad.bin"))
    (tmp_path / "short.bin").write_bytes(raw[:-8])
    with pytest.raises(ValueError):
        Evidence.read(str(tmp_path / "short.bin"))
    lines = ev.text().split("\n")
    assert lines[-1] == "" and len(lines) == 3 + len(ev.totals()) + 1
    assert [float(x) for x in lines[1].split("\t")][0] == 0.4 and lines[3].startswith("thermodynamic_rectangle\t")


@pytest.mark.parametrize("betas", [[1.0, 0.5, 0.0], [1.0, -0.5], [1.0, 0.5, 0.5], [0.5, 1.0], [1.0, float("nan")],
                                   [1.0, 0.5, 1.0, 1.0]])
def test_coefficients_refuse_a_bad_ladder(betas):
    with pytest.raises(ValueError):
        Evidence.coefficients(betas, 2 if len(betas) == 4 else 1)


def test_coefficients_refuse_unequal_ladders():
    with pytest.raises(ValueError):
        Evidence.coefficients([1.0, 0.5, 0.2], 2)
    with pytest.raises(ValueError):
        Evidence.from_rows(np.zeros((3, 2, 6)), [1.0, 0.5]).thermodynamic("simpson")
    with pytest.raises(ValueError):
        Evidence.from_rows(np.zeros((3, 4, 6)), [1.0, 0.5, 1.0, 0.5], n_ladders=2).thermodynamic()


def test_rectangle_restates_the_run_summary():
    betas = [1.0, 0.61, 0.33, 0.12, 0.04, 0.003]
    rows = _rows(5, 400, betas)
    ev = Evidence.from_rows(rows, betas, batch_size=20)
    rs = RunSummary.from_rows(rows, 0, 1, 20, 20, [0.0] * 4, [1.0] * 4)
    want = rs.evidence(betas)
    got = ev.thermodynamic("rectangle")
    assert abs(got - want) <= 1e-12 * abs(want), (got, want)
    total = ev.origin * 400 + ev.sum
    assert np.all(np.abs(total - rs.prob_sum) <= 1e-12 * np.abs(rs.prob_sum))


# ---- a Gaussian with a closed form ----------------------------------------------------------------------------------
# likelihood exp(-x^2 / 2), flat prior on [-20, 20]: Z(beta) = sqrt(2 pi / beta) erf(20 sqrt(beta / 2)) / 40
HALF, N_RUNGS, DRAWS, SEEDS = 20.0, 16, 4000, range(100, 148)


def ln_z(beta):
    return math.log(math.sqrt(2 * math.pi / beta) * math.erf(HALF * math.sqrt(beta / 2)) / (2 * HALF))


def gaussian_replica(seed, betas):
    """DRAWS exact draws per rung from exp(-beta x^2 / 2) on [-20, 20], by rejection from the untruncated normal; the
    Evidence of the column beta * loglike from numpy's sums (the estimators are under test here, not the fold)"""
    rng = np.random.default_rng(seed)
    col = np.zeros((DRAWS, len(betas)))
    for c, b in enumerate(betas):
        got = np.zeros(0)
        while len(got) < DRAWS:
            x = rng.standard_normal(DRAWS) / math.sqrt(b)
            got = np.concatenate([got, x[np.abs(x) <= HALF]])
        col[:, c] = b * (-0.5 * got[:DRAWS] ** 2)
    bs = int(math.sqrt(DRAWS))
    nb = batches_closed(DRAWS, bs)
    up, down = Evidence.coefficients(betas)
    d = col - col[0]
    starts = [0] + [k * bs - 1 for k in range(1, nb + 1)]                 # batch 0 holds bs - 1 samples
    batch = np.add.reduceat(col, starts, axis=0).T
    x = np.stack([up * col, down * col])                                  # [2][n][c]
    m = x.max(axis=1)
    return Evidence([DRAWS], col[0], d.sum(axis=0), (d * d).sum(axis=0), batch, m, np.exp(x - m[:, None, :]).sum(axis=1),
                    betas, bs, up, down)


@pytest.fixture(scope="module")
def gaussian():
    betas = np.geomspace(1.0, 0.01, N_RUNGS)
    return betas, [gaussian_replica(seed, betas) for seed in SEEDS]


def test_gaussian_builder_is_the_fold(gaussian):
    betas, reps = gaussian
    ev = reps[0]
    rng = np.random.default_rng(100)                                      # the first rung's draws again
    x = rng.standard_normal(DRAWS)
    col0 = -0.5 * x[np.abs(x) <= HALF] ** 2
    again = Evidence.from_rows(col0[:500, None], [1.0], batch_size=ev.batch_size)
    assert again.origin[0] == ev.origin[0] and ev.n_batches == 63 and ev.batch.shape == (N_RUNGS, 64)
    assert abs(ev.batch[0, :63].sum() + ev.batch[0, 63] - (ev.origin[0] * DRAWS + ev.sum[0])) < 1e-9
    assert again.batch[0, 0] == pytest.approx(ev.batch[0, 0], rel=1e-13)


def test_gaussian_estimators(gaussian):
    betas, reps = gaussian
    n = len(reps)
    truth, base_truth = ln_z(1.0) - ln_z(betas[-1]), ln_z(betas[-1])
    assert abs(truth + 2.2560) < 5e-5 and abs(base_truth + 0.514) < 5e-4

    def stats(f):
        v = np.array([f(ev) for ev in reps])
        return v.mean(), v.std(ddof=1)
    for direction in ("up", "down"):
        mean, sd = stats(lambda ev: ev.stepping_stone(direction, "down") - ev.base_term("down"))
        print("stepping stone %s: %.4f +- %.4f (truth %.4f)" % (direction, mean, sd, truth))
        assert abs(mean - truth) <= 4 * sd / math.sqrt(n), (direction, mean, sd)
    mean, sd = stats(lambda ev: ev.base_term("down"))
    print("base down: %.4f +- %.4f (truth %.4f); base rectangle: %.4f" % (mean, sd, base_truth,
                                                                         stats(lambda ev: ev.base_term("rectangle"))[0]))
    assert abs(mean - base_truth) <= 4 * sd / math.sqrt(n)
    off = {}
    for rule in ("rectangle", "trapezoid", "corrected"):
        mean, sd = stats(lambda ev: ev.thermodynamic(rule, "down") - ev.base_term("down"))
        print("%s: %.4f +- %.4f" % (rule, mean, sd))
        off[rule] = abs(mean - truth)
    assert off["corrected"] < off["trapezoid"] < off["rectangle"], off
    assert off["rectangle"] > 0.25 and off["corrected"] < 0.01, off
    spread = stats(lambda ev: ev.thermodynamic("trapezoid", "down") - ev.base_term("down"))[1]
    est = float(np.median([ev.error("trapezoid", "down") for ev in reps]))
    print("trapezoid: spread over replicas %.5f, error() %.5f" % (spread, est))
    assert spread / 2 <= est <= spread * 2
    one = reps[0]
    assert one.error("rectangle") > 0 and one.error("corrected", "rectangle") == one.error("trapezoid", "rectangle")
    assert np.all(np.abs(one.var_loglike()[0] - 0.5) < 0.1)                # Var[-x^2 / 2] = 1 / (2 beta^2) at beta = 1
