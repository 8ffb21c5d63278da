"""The CPU oracle against files that the COMPILED REFERENCE wrote (tests/golden/ref_runs/, recorded by
tests/golden/make_ref_runs.py from the binaries of oracle/ref_build.py).

Every GPU test compares a kernel with oracle/apemost_oracle.c; these tests compare the oracle with the
reference itself: calibrate_first, calibrate_rest and run, process by process, through the "%.15e"
calibration_results round trip, in the reference's RNG mode (ORC_RNG_GLOBAL_MT).  Everything is compared
byte for byte (acceptance rows as integers) with no tolerance: the same operations in the same order on
one libm with contraction off.

Where the reference tree is present a second test per case builds the case's binary through the recipe,
runs it again and asserts that the fresh files equal the committed ones, so that a fixture cannot go
stale or be edited by hand.  Where it is absent only that half is skipped, by name.

What this does not pin: the arithmetic library under the reference is this project's GSL surface
(apemost_amd/host/src/gslcompat.c), not real GSL -- see oracle/README.md.
"""
import json
import math
import os

import numpy as np
import pytest

from apemost_amd import workloads as wl
from oracle import oracle as orc
from oracle import ref_build as rb

RUN_CASES = sorted(c for c in rb.CASES if rb.CASES[c]["kind"] == "run")
EVAL_CASES = sorted(c for c in rb.CASES if rb.CASES[c]["kind"] == "eval")
MODEL = {"simplesin": wl.MODEL_SIMPLESIN, "pulse": wl.MODEL_PULSE, "pulse_vrot": wl.MODEL_PULSE_VROT}


def _fixture(golden_dir, case):
    """{relative name: bytes} of a committed case"""
    path = rb.fixture_path(golden_dir, case)
    assert os.path.exists(path), "no fixture for %s: run tests/golden/make_ref_runs.py" % case
    return rb.read_bundle(path)


def _c(fmt, v):
    """C's printf of one double (glibc spells the non-finite ones nan, -nan, inf, -inf)"""
    if math.isnan(v):
        return ("-nan" if math.copysign(1.0, v) < 0 else "nan").rjust(6 if fmt == "%6e" else 0)
    return fmt % v


def _inputs(case):
    """what the reference reads: the params table and the data matrix, through their text files"""
    w = rb.workload(case)
    rows = [line.split("\t") for line in w.params_file_text().splitlines()]
    col = lambda k: np.array([float(r[k]) for r in rows])
    data = np.array([[float(v) for v in line.split("\t")] for line in w.data_file_text().splitlines()])
    return w, col(0), col(1), col(2), col(4), data


def _ladder(case):
    """setup_chains (src/parallel_tempering_config.c:95-123) with the case's compile-time variants"""
    w, start, pmin, pmax, step, data = _inputs(case)
    m = rb.CASES[case]["macros"]
    lad = orc.Ladder.from_params(MODEL[rb.CASES[case]["model"]], m["N_BETA"], start, pmin, pmax, step, data)
    lad.randomswap, lad.adapt, lad.rwm = int("RANDOMSWAP" in m), int("ADAPT" in m), int("RWM" in m)
    lad.proposal = (orc.PROPOSAL_LOGISTIC if "PROPOSAL_LOGISTIC" in m else
                    orc.PROPOSAL_UNIFORM if "PROPOSAL_UNIFORM" in m else orc.PROPOSAL_GAUSSIAN)
    if m.get("CIRCULAR_PARAMS"):
        lad.circular = 1 << (m["CIRCULAR_PARAMS"] - 1)    # the macro lists parameters from 1
    return w, lad


def _calibration_text(lad, n):
    """write_calibrations_file, src/parallel_tempering_config.c:176-202"""
    return "".join("\t".join(_c("%.15e", v) for v in [lad.beta[j]] + list(lad.step[j]) + list(lad.params[j])) + "\n"
                   for j in range(n)).encode()


def _read_calibration(lad, text, n):
    """read_calibration_file, src/parallel_tempering_config.c:130-174"""
    p = lad.n_par
    for j, line in enumerate(text.decode().splitlines()[:n]):
        v = [float(x) for x in line.split("\t")]
        lad.beta[j], lad.step[j], lad.params[j] = v[0], v[1:1 + p], v[1 + p:1 + 2 * p]
        lad.params_best[j] = lad.params[j]


def _oracle_case(case, tmp_path):
    """the oracle through the phases of generic_main: {relative name: bytes} like ref_build.run_case"""
    m = rb.CASES[case]["macros"]
    seed, n_beta = rb.CASES[case]["gsl_seed"], m["N_BETA"]
    cfg = orc.calib_defaults(burn_in_iterations=m["BURN_IN_ITERATIONS"])
    progress = tmp_path / "calibration_progress.data"
    out, status = {}, []

    def finish():
        out["exit_status"] = "".join(status).encode()
        orc.set_progress_path(None)
        return out

    orc.set_progress_path(progress)
    # ---- calibrate_first (src/parallel_tempering.c:78-95): exit(1) where the oracle returns a status
    _, lad = _ladder(case)
    rc = orc.calibrate_first(lad, orc.Rng(orc.RNG_GLOBAL_MT, seed), cfg)
    status.append("calibrate_first %d\n" % (rc != orc.CALIB_OK))
    out["calibrate_first/calibration_progress.data"] = progress.read_bytes()
    if rc != orc.CALIB_OK:
        return finish()
    out["calibrate_first/calibration_results"] = _calibration_text(lad, 1)
    # ---- calibrate_rest (:115-207), a new process
    _, lad = _ladder(case)
    _read_calibration(lad, out["calibrate_first/calibration_results"], 1)
    rc = orc.calibrate_rest(lad, orc.Rng(orc.RNG_GLOBAL_MT, seed), cfg)[0]
    status.append("calibrate_rest %d\n" % (rc != orc.CALIB_OK))
    out["calibrate_rest/calibration_progress.data"] = progress.read_bytes()
    if rc != orc.CALIB_OK:
        return finish()
    out["calibrate_rest/calibration_results"] = _calibration_text(lad, n_beta)
    # ---- run (:209-250, :347-419), a new process: prob stays -1e10
    w, lad = _ladder(case)
    _read_calibration(lad, out["calibrate_rest/calibration_results"], n_beta)
    rng = orc.Rng(orc.RNG_GLOBAL_MT, seed)
    n_swap = m["N_SWAP"]
    rounds, it, acc = [], 0, []
    while it < m["MAX_ITERATIONS"]:
        rounds.append(orc.run_sampler(lad, rng, 1, n_swap, record=True))
        it += n_swap
        if it % m["PRINT_PROB_INTERVAL"] == 0:     # dump(), :308-326
            acc.append("%d" % it + "".join("\t%d" % a for a in lad.accept) + "\n")
    s = np.concatenate(rounds)
    p = lad.n_par
    out["run/acceptance_rate.dump"] = "".join(acc).encode()
    for k, name in enumerate(w.names):             # mcmc_dump_current, src/mcmc_dump.c:79-88
        out["run/%s-chain-0.prob.dump" % name] = "".join(_c("%.15e", v) + "\n" for v in s[:, 0, k]).encode()
    for i in range(n_beta):                        # src/parallel_tempering.c:399-401
        out["run/prob-chain%d.dump" % i] = "".join(_c("%6e", a) + "\t" + _c("%6e", b) + "\n"
                                                   for a, b in zip(s[:, i, p], s[:, i, p + 1])).encode()
    status.append("run 0\n")
    return finish()


def _where_digests_differ(got_text, want_text, raw, phase):
    """a digests.json that differs: name the file and the first block of lines that departs, and show the lines
    the oracle has there"""
    got, want, msg = json.loads(got_text), json.loads(want_text), []
    for name in sorted(set(got) | set(want)):
        g, w = got.get(name), want.get(name)
        if g == w:
            continue
        if g is None or w is None:
            msg.append("%s: stored whole on one side, as a digest on the other" % name)
            continue
        k = next((i for i, (a, b) in enumerate(zip(g["blocks"], w["blocks"])) if a != b),
                 min(len(g["blocks"]), len(w["blocks"])))
        lo = k * rb.DIGEST_BLOCK
        lines = raw["%s/%s" % (phase, name)].decode().splitlines()[lo:lo + rb.DIGEST_BLOCK]
        msg.append("%s: %d lines against the reference's %d; first departure inside lines %d-%d, where the oracle "
                   "has\n    %s" % (name, g["lines"], w["lines"], lo + 1, lo + rb.DIGEST_BLOCK, "\n    ".join(lines)))
    return "\n".join(msg)


def _assert_same_files(got, want, what, raw=None):
    assert sorted(got) == sorted(want), what
    problems = []
    for n in sorted(want):
        if n.endswith("acceptance_rate.dump"):
            rows = lambda b: [[int(v) for v in line.split()] for line in b.decode().splitlines()]
            if rows(got[n]) != rows(want[n]):
                problems.append("%s: rows %r, expected %r" % (n, rows(got[n]), rows(want[n])))
        elif got[n] != want[n] and n.endswith("digests.json") and raw is not None:
            problems.append("%s\n%s" % (n, _where_digests_differ(got[n], want[n], raw, n.rpartition("/")[0])))
        elif got[n] != want[n]:
            g, e = got[n].decode().splitlines(), want[n].decode().splitlines()
            k = next((i for i, (a, b) in enumerate(zip(g, e)) if a != b), min(len(g), len(e)))
            problems.append("%s differs at line %d of %d/%d:\n  got      %r\n  expected %r" %
                            (n, k + 1, len(g), len(e), g[k:k + 1], e[k:k + 1]))
    if problems:
        pytest.fail("%s:\n%s" % (what, "\n".join(problems)))


@pytest.mark.parametrize("case", RUN_CASES)
def test_oracle_reproduces_the_reference_run(case, golden_dir, tmp_path):
    """calibration_results after each calibration phase, calibration_progress.data, chain 0's parameter dumps
    and every chain's prob-chain<i>.dump byte for byte (the long ones through ref_build.digest_of and an excerpt;
    a mismatch is reported with the block of 100 lines where it starts and the oracle's lines there), every
    acceptance_rate.dump row as integers, and the
    exit status of each phase (a failed calibration included: pulse_vrot_calibration_fails)."""
    want = _fixture(golden_dir, case)
    want.pop("case.json")
    # the fourth phase's entries (analyse/..., its exit_status line) are tests/test_reference_analyse.py's
    want = {n: b for n, b in want.items() if not n.startswith("analyse/")}
    want["exit_status"] = b"".join(l for l in want["exit_status"].splitlines(True) if not l.startswith(b"analyse "))
    raw = _oracle_case(case, tmp_path)
    _assert_same_files(rb.to_fixture(case, raw), want, "oracle vs reference, case %s" % case, raw)


def _points(text):
    return np.array([[float(v) for v in line.split("\t")] for line in text.decode().splitlines()])


@pytest.mark.parametrize("case", EVAL_CASES)
def test_oracle_loglike_equals_eval_main(case, golden_dir):
    """apps/eval_main.c:52-66 prints prob and prior at "%.15e" with beta = 1; the oracle's values, printed the
    same way, are the same text -- across the workload's box and at the +-1e30 / +-1e200 unit scalings, with
    no tolerance (measured: none needed, the sums agree to the last printed digit).  With every height zero
    the reference prints nothing: gsl_sf_log(0) is a domain error and the process aborts (recorded exit status
    -6); the oracle defines that point as NaN (ln 0 + d / 0), which is what the device must give too."""
    fx = _fixture(golden_dir, case)
    status = dict(line.split() for line in fx["exit_status"].decode().splitlines())
    groups = rb.eval_groups(case)
    assert [g[0] for g in groups] == [u[0] for u in rb.EVAL_UNITS] == list(status)
    for (name, _, _, points_text), (_, sf, sh) in zip(groups, rb.EVAL_UNITS):
        assert fx["points_%s.txt" % name] == points_text.encode(), name
        _, data = rb.eval_units(case, sf, sh)
        data = np.array([[float("%.17e" % v) for v in row] for row in data])
        got = [orc.loglike(MODEL[rb.CASES[case]["model"]], p, data, beta=1.0) for p in _points(fx["points_%s.txt" % name])]
        if name == "heights_zero":
            assert status[name] == "-6" and fx["eval_%s.out" % name] == b""
            assert all(math.isnan(prob) for prob, _ in got)
            continue
        assert status[name] == "0"
        text = "".join("%s\t%s\n" % (_c("%.15e", prob), _c("%.15e", prior)) for prob, prior in got)
        _assert_same_files({name: text.encode()}, {name: fx["eval_%s.out" % name]}, case)


# ---- the fixtures against a fresh build of the reference (only where its tree is present) ----------------------

_need_ref = pytest.mark.skipif(not rb.have_reference(),
                               reason="reference tree not present: the fixture-freshness half is skipped, "
                                      "the oracle-versus-fixture half above still runs")


@_need_ref
@pytest.mark.parametrize("case", RUN_CASES + EVAL_CASES)
def test_fixture_equals_a_fresh_reference_run(case, golden_dir, tmp_path):
    import sys
    sys.path.insert(0, os.path.join(str(golden_dir)))
    try:
        import make_ref_runs
    finally:
        sys.path.pop(0)
    rb.build_case(case)
    got = make_ref_runs.fixture_files(case, str(tmp_path))
    want = _fixture(golden_dir, case)
    assert json.loads(want["case.json"]) == json.loads(got["case.json"])
    assert sorted(got) == sorted(want)
    for n in sorted(want):
        assert got[n] == want[n], "%s/%s is not what the reference writes today" % (case, n)


def test_fixture_set_is_complete_and_small(golden_dir):
    """every case of the recipe has a fixture, nothing else lies there, no case above the older largest
    fixture (testlc.dat) and the whole set stays under 160 KB (100 KB before the analyse phase was recorded:
    seven cases gained 37 KB of histogram digests, excerpts, gnuplot files and stdout)"""
    root = os.path.join(str(golden_dir), "ref_runs")
    assert sorted(os.listdir(root)) == sorted(rb.CASES)
    limit = os.path.getsize(os.path.join(str(golden_dir), "testlc.dat"))
    sizes = [os.path.getsize(rb.fixture_path(golden_dir, case)) for case in rb.CASES]
    assert max(sizes) <= limit and sum(sizes) <= 160 * 1024
