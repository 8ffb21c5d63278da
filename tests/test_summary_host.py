"""Run summaries without a GPU: the ABI and its binding, the summary kernel's code object, the batching rule
of batch_means_error(), and the C host's `analyse` reading summary.bin instead of the dump files."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import build, capi, workloads as wl
from apemost_amd.state import LadderState
from apemost_amd.summary import RunSummary, batch_index, batches_closed, batch_size_for
from tests import hostlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SUMMARY_SYMBOLS = ["apemost_hip_summary_begin", "apemost_hip_summary_accumulate", "apemost_hip_summary_get",
                   "apemost_hip_summary_set", "apemost_hip_summary_end"]


def test_summary_symbols_declared_bound_and_exported():
    build.build_hip()
    hdr = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    for name in SUMMARY_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in capi.EXPORTS
        assert getattr(capi.lib(), name).argtypes is not None
    assert "apemost_hip_summary_config" in hdr and "apemost_hip_summary_view" in hdr
    assert "#define APEMOST_HIP_ABI_VERSION 3" in hdr
    nm = subprocess.check_output(["nm", "-D", "--defined-only", build.HIP_LIB]).decode()
    exported = set(re.findall(r" T (apemost_hip_[a-z_0-9]+)", nm))
    assert set(SUMMARY_SYMBOLS) <= exported


def test_summary_kernel_compiles_for_gfx950_without_scratch(tmp_path):
    src = tmp_path / "summary_only.hip"
    src.write_text('#include "pt_summary.h"\n')
    obj = tmp_path / "summary_only.o"
    subprocess.check_call([build.HIPCC] + [f for f in build.HIP_FLAGS if f != "-shared"] +
                          ["-c", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC, "-o", str(obj), str(src)])
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    ks = [k for k in kernel_resources.kernels(str(obj)) if "summary_kernel" in k["demangled"]]
    assert len(ks) == 1
    k = ks[0]
    assert int(k["private_segment_fixed_size"]) == 0, k
    assert int(k["vgpr_spill_count"]) == 0 and int(k["sgpr_spill_count"]) == 0, k


def _reference_batches(total, bs):
    """batch_means_error()'s loop (apemost_amd/host/src/analyse.c), transcribed: the batch of every sample"""
    out, n, nb = [], 0, 0
    for _ in range(total):
        n += 1
        out.append(nb)
        if n % bs == bs - 1:
            nb += 1
    return out, nb


def test_batch_index_follows_batch_means_error():
    for bs in range(1, 10):
        for total in sorted({max(0, m * bs + d) for m in range(0, 5) for d in (-2, -1, 0, 1, 2)}):
            want, closed = _reference_batches(total, bs)
            assert [batch_index(i, bs) for i in range(total)] == want, (bs, total)
            assert batches_closed(total, bs) == closed, (bs, total)
    assert batch_size_for(99) == 9 and batch_size_for(100) == 10


def _rows(n, n_beta, w, seed):
    """synthetic sample rows, rounded so that "%.15e" and "%6e" both hold them exactly"""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, n_beta, w.n_par + 2))
    for p in range(w.n_par):
        rows[:, :, p] = rng.uniform(w.pmin[p], w.pmax[p], (n, n_beta))
    rows[:, :, w.n_par] = rng.normal(-50, 5, (n, n_beta))
    rows[:, :, w.n_par + 1] = rng.normal(-40, 5, (n, n_beta))
    rows[0, 0, 0] = w.pmax[0]                                # the top of the range lands in the last bin
    rows[1, 0, 1] = w.pmin[1]
    return np.vectorize(lambda v: float("%.6e" % v))(rows)


def _analyse_dirs(tmp_path, n, n_beta, ccflags=""):
    w = wl.simplesin(n_data=16, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"), ccflags="-DN_BETA=%d %s" % (n_beta, ccflags))
    st = LadderState.from_params(n_beta, w.start, w.pmin, w.pmax, w.step)
    for i in range(n_beta):
        st.beta[i] = 1.0 - i / n_beta
    rows = _rows(n, n_beta, w, seed=n)
    dirs = {}
    for mode in ("text", "summary"):
        d = tmp_path / mode
        d.mkdir()
        (d / "params").write_text(w.params_file_text())
        (d / "data").write_text(w.data_file_text())
        (d / "calibration_results").write_text(st.calibration_results_text())
        dirs[mode] = d
    t = dirs["text"]
    for p, name in enumerate(w.names):
        (t / ("%s-chain-0.prob.dump" % name)).write_text("".join("%.15e\n" % v for v in rows[:, 0, p]))
    for c in range(n_beta):
        (t / ("prob-chain%d.dump" % c)).write_text(
            "".join("%6e\t%6e\n" % (a, b) for a, b in rows[:, c, w.n_par:]))
    lo = np.array([float("%.15e" % v) for v in w.pmin])
    hi = np.array([float("%.15e" % v) for v in w.pmax])
    bs = batch_size_for(n)
    rs = RunSummary.from_rows(rows, 1, 200, bs, batches_closed(n, bs), lo, hi)
    rs.write(str(dirs["summary"] / "summary.bin"))
    return exe, dirs, w, rs, st


def _run(exe, cwd, env_extra, args=("analyse",)):
    env = dict(os.environ)
    env.pop("APEMOST_DUMP", None)
    env.update(env_extra)
    return subprocess.run([exe] + list(args), cwd=str(cwd), env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          universal_newlines=True)


def _lines(out, key):
    return [l.split("\r")[-1] for l in out.splitlines() if key in l]


def test_analyse_from_summary_matches_analyse_from_text_dumps(tmp_path):
    n, n_beta = 2500, 4
    exe, dirs, w, rs, st = _analyse_dirs(tmp_path, n, n_beta)
    text = _run(exe, dirs["text"], {})
    summ = _run(exe, dirs["summary"], {"APEMOST_DUMP": "summary"})
    assert text.returncode == 0, text.stderr
    assert summ.returncode == 0, summ.stderr
    for name in w.names:
        assert (dirs["summary"] / (name + ".histogram")).read_text() == (dirs["text"] / (name + ".histogram")).read_text()
    g = "marginal_distributions.gnuplot"
    assert (dirs["summary"] / g).read_text() == (dirs["text"] / g).read_text()
    for key in ("Model probability", "mcmc error"):
        a, b = _lines(text.stdout, key), _lines(summ.stdout, key)
        assert a and a == b, (key, a, b)
    assert summ.stderr == ""
    # and RunSummary's own numbers are those analyse prints
    ev = float(re.search(r"\] (-?[0-9.]+)", _lines(summ.stdout, "Model probability")[0]).group(1))
    assert abs(rs.evidence(st.beta) - ev) < 1e-5
    errs = [float(re.search(r": (-?[0-9.]+)", l).group(1)) for l in _lines(summ.stdout, "mcmc error")]
    for p, e in enumerate(errs):
        assert abs(rs.batch_means_error(p) - e) < 1e-6
    # no dump file was read: the summary directory has none
    assert not [f for f in os.listdir(str(dirs["summary"])) if f.endswith(".dump")]


def test_analyse_names_a_batch_size_that_no_longer_fits(tmp_path):
    n, n_beta = 400, 2
    exe, dirs, w, rs, st = _analyse_dirs(tmp_path, n, n_beta)
    # an interrupted run: batch size planned for 900 samples, 400 taken
    r2 = RunSummary(rs.n, rs.prob_sum, rs.hist, np.zeros((1, w.n_par, batches_closed(900, 30) + 1)),
                    batches_closed(n, 30), rs.lo, rs.hi, 30)
    r2.write(str(dirs["summary"] / "summary.bin"))
    out = _run(exe, dirs["summary"], {"APEMOST_DUMP": "summary"})
    assert out.returncode == 0, out.stderr
    assert re.search(r"batch size 30 recorded in summary.bin, floor\(sqrt\(400 values\)\) = 20", out.stderr), out.stderr
    assert len(_lines(out.stdout, "mcmc error")) == w.n_par


def test_summary_file_round_trip(tmp_path):
    w = wl.simplesin(n_data=16, n_chain=3)
    rows = _rows(77, 3, w, seed=5)
    rs = RunSummary.from_rows(rows, 2, 17, 8, batches_closed(77, 8) + 3, w.pmin, w.pmax, thin=4)
    rs.write(str(tmp_path / "s.bin"))
    back = RunSummary.read(str(tmp_path / "s.bin"))
    assert back.n == 77 and back.thin == 4 and back.batch_size == 8 and back.n_batches == batches_closed(77, 8)
    for a in ("prob_sum", "hist", "batch_sums", "lo", "hi"):
        assert np.array_equal(getattr(back, a), getattr(rs, a)), a
    # the per-chain sums are sequential sums of the rows
    s = 0.0
    for v in rows[:, 1, w.n_par + 1]:
        s += float(v)
    assert back.prob_sum[1] == s
    assert int(back.hist.sum()) == 2 * w.n_par * 77


def test_dump_spec_accepts_summary_and_rejects_bad_tokens(tmp_path):
    n_beta = 2
    exe, dirs, w, rs, st = _analyse_dirs(tmp_path, 50, n_beta, ccflags="-DMAX_ITERATIONS=10")
    for spec in ("summary", "summary,thin:3", "text,summary", "binary,summary"):
        r = _run(exe, dirs["summary"], {"APEMOST_DUMP": spec}, args=("run",))
        assert "APEMOST_DUMP: expected" not in r.stderr, (spec, r.stderr)
    for spec in ("summar", "summary:all", "bogus", "summary,foo"):
        r = _run(exe, dirs["summary"], {"APEMOST_DUMP": spec}, args=("run",))
        assert r.returncode == 1 and "APEMOST_DUMP: expected" in r.stderr and "summary" in r.stderr, (spec, r.stderr)


def test_histograms_minmax_with_summary_is_refused(tmp_path):
    exe, dirs, w, rs, st = _analyse_dirs(tmp_path, 50, 2, ccflags="-DHISTOGRAMS_MINMAX")
    r = _run(exe, dirs["summary"], {"APEMOST_DUMP": "summary"})
    assert r.returncode == 1 and "HISTOGRAMS_MINMAX" in r.stderr, r.stderr
    assert _run(exe, dirs["text"], {}).returncode == 0


# ---- the restatement that judges the kernel on hand-built rows (tests/summary_rows.py), checked on the CPU ----------
_nbins_exe = {}


@pytest.mark.parametrize("nbins", [1, 2, 200, 4096])
@pytest.mark.parametrize("box_set", ["A", "B"])
def test_restated_bins_equal_host_analyse_and_from_rows(box_set, nbins, tmp_path, tmp_path_factory):
    """The finite values of the hand-built rows that "%.15e" holds exactly, as dump files of chain 0, through the
    host's `analyse` in text mode (create_hist and gsl_histogram_increment in C): its counts are those of
    np.searchsorted over GSL's edges (summary_rows.bins_of) and those of RunSummary.from_rows"""
    from tests import summary_rows as sr
    rows, boxes = sr.build_rows(box_set, nbins, n_chains=30)
    if nbins not in _nbins_exe:
        _nbins_exe[nbins] = hostlib.make(str(tmp_path_factory.mktemp("nbins%d" % nbins) / "sine.exe"),
                                         ccflags="-DN_BETA=2 -DNBINS=%d" % nbins)
    names = ["amplitude", "frequency", "phase", "offset"]
    for p, (lo, hi) in enumerate(boxes):
        assert float("%.15e" % lo) == lo and float("%.15e" % hi) == hi
    (tmp_path / "params").write_text("".join("%.15e\t%.15e\t%.15e\t%s\t%.15e\n" % ((lo + hi) / 2, lo, hi, n, -1)
                                             for (lo, hi), n in zip(boxes, names)))
    (tmp_path / "data").write_text(wl.simplesin(n_data=16, n_chain=2).data_file_text())
    st = LadderState.from_params(2, [(lo + hi) / 2 for lo, hi in boxes], [b[0] for b in boxes], [b[1] for b in boxes],
                                 [-1.0] * 4)
    st.beta[1] = 0.5
    (tmp_path / "calibration_results").write_text(st.calibration_results_text())
    for c in range(2):
        (tmp_path / ("prob-chain%d.dump" % c)).write_text("%6e\t%6e\n" % (-50.0, -40.0))
    kept = {}
    for p, name in enumerate(names):
        v = np.concatenate([rows[:, h, p] for h in range(30)])
        v = v[np.isfinite(v)]
        v = np.array([x for x in v.tolist() if float("%.15e" % x) == x])
        assert len(v) > 1000
        kept[p] = v
        (tmp_path / ("%s-chain-0.prob.dump" % name)).write_text("".join("%.15e\n" % x for x in v))
    r = _run(_nbins_exe[nbins], tmp_path, {})
    assert r.returncode == 0, r.stderr
    for p, name in enumerate(names):
        lo, hi = boxes[p]
        e = sr.gsl_edges(lo, hi, nbins)
        want = sr.bins_of(kept[p], e)
        total = float(want.sum())
        assert 0 < total < len(kept[p])                      # some inside, some outside the box
        lines = [l.split() for l in (tmp_path / (name + ".histogram")).read_text().splitlines()]
        assert [l[0] for l in lines] == ["%.15e" % x for x in e[:-1]] and lines[-1][1] == "%.15e" % e[-1]
        scale = (hi - lo) / nbins / total
        assert [l[2] for l in lines] == ["%.15e" % (float(c) * scale) for c in want.tolist()], (name, nbins)
        rs = RunSummary.from_rows(kept[p].reshape(-1, 1, 1).repeat(3, axis=2), 1, nbins, 1, len(kept[p]), [lo], [hi])
        assert rs.hist[0, 0].tolist() == want.tolist(), (name, nbins)
