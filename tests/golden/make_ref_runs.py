#!/usr/bin/env python3
"""Records tests/golden/ref_runs/<case>/ from the COMPILED REFERENCE (oracle/ref_build.py).

Needs the reference tree ($APEMOST_REFERENCE, or ref_build.DEFAULT_REFERENCE); re-run with
    python tests/golden/make_ref_runs.py [case ...]
A case is stored as ONE text file, <case>/files.txt (ref_build.write_bundle): a "### name bytes" line, then
that file's bytes.  The names calibrate_first/..., calibrate_rest/... and run/... are files a reference binary
wrote in that phase, byte for byte; acceptance_rate.dump and calibration_results always whole.  A longer file
(the dumps of runs of 1000 steps and more, most calibration_progress.data) is held by <phase>/digests.json --
its SHA-256 and one per block of 100 lines -- and <name>.excerpt, its first and last lines
(ref_build.to_fixture).  Ours are also case.json (what the case is), exit_status (one line per phase that
ran) and points_*.txt (the stdin of eval_main).  analyse/... are what the fourth phase left: every
<name>.histogram (digested like the dumps), marginal_distributions.gnuplot and stdout, the latter without its
carriage-return progress segments (ref_build.cut_progress); an analyse-only case (kind "analyse") holds nothing
else, its run directory being that of the case it names with "of".  The inputs `params` and `data` come from
apemost_amd/workloads.py and are not stored.  tests/test_reference_pins.py runs the same binaries again where
the reference is present and asserts that nothing here has gone stale.

Size: no case above MAX_FILE (the largest older fixture, testlc.dat), the whole set under 160 KB.
"""
import json
import os
import shutil
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref_build as rb  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "ref_runs")
MAX_FILE = 77622


def case_json(case):
    c = rb.CASES[case]
    d = dict(kind=c["kind"], model=c["model"], n_data=c["n_data"], workload_seed=c["wl_seed"],
             macros=c["macros"], env=dict(GSL_RNG_SEED=str(c["gsl_seed"]), OMP_NUM_THREADS="1"))
    if "of" in c:
        d["of"] = c["of"]
    return json.dumps(d, sort_keys=True) + "\n"


def fixture_files(case, workdir):
    """{relative name: bytes} of a case's fixture, from a fresh run of its binary in workdir"""
    c = rb.CASES[case]
    files = {"case.json": case_json(case).encode()}
    if c["kind"] == "eval":
        groups = rb.eval_groups(case)
        outs = rb.eval_case(case, workdir, groups)
        for name, _, _, points in groups:
            files["points_%s.txt" % name] = points.encode()
            files["eval_%s.out" % name] = outs[name][0]
        files["exit_status"] = "".join("%s %d\n" % (name, outs[name][1]) for name, _, _, _ in groups).encode()
        return files
    got = rb.to_fixture(case, rb.run_case(case, workdir))
    files.update(got)
    return files


def main(cases):
    if not rb.have_reference():
        sys.exit("no reference tree at %s (set APEMOST_REFERENCE)" % rb.reference_dir())
    total = 0
    for case in cases or sorted(rb.CASES):
        rb.build_case(case)
        if "of" in rb.CASES[case]:
            rb.build_case(rb.CASES[case]["of"])
        with tempfile.TemporaryDirectory() as tmp:
            files = fixture_files(case, tmp)
        shutil.rmtree(os.path.join(OUT, case), ignore_errors=True)
        rb.write_bundle(rb.fixture_path(os.path.dirname(OUT), case), files)
        assert os.path.getsize(rb.fixture_path(os.path.dirname(OUT), case)) <= MAX_FILE, case
        size = sum(len(b) for b in files.values())
        total += size
        print("%-32s %3d files %7d bytes  %s" % (case, len(files), size,
                                                 files.get("exit_status", b"").decode().replace("\n", "; ")))
    print("total %d bytes" % total)


if __name__ == "__main__":
    main(sys.argv[1:])
