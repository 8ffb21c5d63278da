"""Recipe that compiles the REFERENCE (APEMoST itself) into oracle/_ref/, one binary per pinned case.

TEST INFRASTRUCTURE ONLY, like everything under oracle/.

The reference is named by path only: $APEMOST_REFERENCE, or the location tests/test_host_layer.py
uses.  Nothing of it is copied: its src/*.c, one apps/<model>.c and one of its mains are compiled in
place, with the reference Makefile's flags plus -ffp-contract=off, against this project's own
GSL-compatible surface (apemost_amd/host/gsl, apemost_amd/host/src/gslcompat.c) and the small
supplement under oracle/refgsl/.  oracle/_ref/ is git-ignored.

N_BETA, BURN_IN_ITERATIONS, MAX_ITERATIONS, N_SWAP and the variant macros are compile-time in the
reference, hence one binary per case.  The fourth phase, `analyse`, is recorded too: after a successful `run`
the cases of ANALYSE_AFTER_RUN run `analyse` in the same directory, and the cases of kind "analyse" run only
`analyse`, built with other macros of the reference's src/analyse.c (NBINS, HISTOGRAMS_MINMAX), in the run
directory of the case they name with `of`.  CASES below is the single list that this recipe,
tests/golden/make_ref_runs.py (which records tests/golden/ref_runs/) and tests/test_reference_pins.py
share.

Limits, stated plainly: the arithmetic library under the reference is this project's GSL surface, not
real GSL -- mt19937, gsl_ran_gaussian / _logistic / _flat are as restated in gslcompat.c (KATs in
tests/test_oracle_pins.py), gsl_sf_sin and gsl_sf_log are libm's.  The recorded runs therefore fix the
reference's control flow, draw order and operation order, not GSL's last-ulp special functions.

-DDUMP_ALL_CHAINS is never passed: with it the reference's report() reads chains[n_beta]
(src/parallel_tempering.c:40-50) and the run ends in a segmentation fault.  The default already gives
chain 0's <name>-chain-0.prob.dump and every chain's prob-chain<i>.dump.
"""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
OUT_DIR = os.path.join(_HERE, "_ref")
_HOST = os.path.join(_ROOT, "apemost_amd", "host")
DEFAULT_REFERENCE = "/root/reference"   # as tests/test_host_layer.py

# the reference Makefile's CFLAGS (Makefile:9,15) without the warning switches, plus contraction off;
# -ansi after -std=c99 is the Makefile's own order (under gnu99 src/mcmc_parser.c:37's strnlen clashes)
CFLAGS = ["-O3", "-std=c99", "-fopenmp", "-fPIC", "-ansi", "-DWITHOUT_GARBAGE_COLLECTOR", "-ffp-contract=off"]
LDFLAGS = ["-lm", "-lgomp"]


def reference_dir():
    return os.environ.get("APEMOST_REFERENCE", DEFAULT_REFERENCE)


def have_reference():
    return os.path.isdir(os.path.join(reference_dir(), "src"))


def _run(model, n_data, gsl_seed=0, wl_seed=None, **macros):
    return dict(kind="run", model=model, n_data=n_data, wl_seed=wl_seed, gsl_seed=gsl_seed, macros=macros)


def _analyse(cases, of, **macros):
    """an analyse-only case: the run case `of` with other compile-time macros of src/analyse.c"""
    c = cases[of]
    return dict(c, kind="analyse", of=of, macros=dict(c["macros"], **macros))


# macro value None = defined without a value (-DRANDOMSWAP).  Every run phase is 1000 steps or more with a
# hundred or more swap attempts (N_SWAP explicit); PRINT_PROB_INTERVAL is lowered so that acceptance_rate.dump
# has ten and more rows.  Dumps of that length are stored as digests and excerpts: to_fixture().
CASES = {
    # all three phases, the default build
    "simplesin": _run("simplesin", 64, N_BETA=4, BURN_IN_ITERATIONS=1000, N_SWAP=20, MAX_ITERATIONS=2000,
                      PRINT_PROB_INTERVAL=100),
    "pulse": _run("pulse", 128, N_BETA=3, BURN_IN_ITERATIONS=1000, N_SWAP=10, MAX_ITERATIONS=1500,
                  PRINT_PROB_INTERVAL=100),
    "pulse_vrot": _run("pulse_vrot", 128, N_BETA=3, BURN_IN_ITERATIONS=1000, N_SWAP=10, MAX_ITERATIONS=1500,
                       PRINT_PROB_INTERVAL=100),
    # another seed (of the generator and of the data), more chains, an N_SWAP that divides nothing
    "simplesin_seed7": _run("simplesin", 48, gsl_seed=7, wl_seed=99, N_BETA=6, BURN_IN_ITERATIONS=600, N_SWAP=7,
                            MAX_ITERATIONS=1400, PRINT_PROB_INTERVAL=70),
    # the compile-time variants, on simplesin
    "simplesin_randomswap": _run("simplesin", 64, N_BETA=3, BURN_IN_ITERATIONS=600, N_SWAP=10, MAX_ITERATIONS=1000,
                                 PRINT_PROB_INTERVAL=100, RANDOMSWAP=None),
    "simplesin_adapt": _run("simplesin", 64, N_BETA=3, BURN_IN_ITERATIONS=600, N_SWAP=10, MAX_ITERATIONS=1000,
                            PRINT_PROB_INTERVAL=100, ADAPT=None),
    "simplesin_rwm": _run("simplesin", 64, N_BETA=3, BURN_IN_ITERATIONS=600, N_SWAP=10, MAX_ITERATIONS=1000,
                          PRINT_PROB_INTERVAL=100, RWM=None),
    "simplesin_logistic": _run("simplesin", 64, N_BETA=3, BURN_IN_ITERATIONS=600, N_SWAP=10, MAX_ITERATIONS=1000,
                               PRINT_PROB_INTERVAL=100, PROPOSAL_LOGISTIC=None),
    "simplesin_uniform": _run("simplesin", 64, N_BETA=3, BURN_IN_ITERATIONS=600, N_SWAP=10, MAX_ITERATIONS=1000,
                              PRINT_PROB_INTERVAL=100, PROPOSAL_UNIFORM=None),
    # parameter 3 (index 2, the phase) wraps: src/markov_chain.h:34-46, src/markov_chain.c:241-265
    "simplesin_circular": _run("simplesin", 64, N_BETA=3, BURN_IN_ITERATIONS=600, N_SWAP=10, MAX_ITERATIONS=1000,
                               PRINT_PROB_INTERVAL=100, CIRCULAR_PARAMS=3),
    # -DADAPT acts only past 20000 counted parameter updates (src/parallel_tempering.c:284-287), 5000 steps of a
    # four-parameter chain: a run long enough to rescale
    "simplesin_adapt_long": dict(_run("simplesin", 32, gsl_seed=0, N_BETA=3, BURN_IN_ITERATIONS=600, N_SWAP=50,
                                      MAX_ITERATIONS=6500, PRINT_PROB_INTERVAL=500, ADAPT=None)),
    # a calibration that fails: calibrate_rest leaves with exit status 1
    "pulse_vrot_calibration_fails": _run("pulse_vrot", 200, N_BETA=6, BURN_IN_ITERATIONS=500, N_SWAP=10,
                                         MAX_ITERATIONS=100, PRINT_PROB_INTERVAL=50),
    # apps/eval_main.c:52-66 on parameter points read from stdin
    "eval_pulse": dict(kind="eval", model="pulse", n_data=1100, wl_seed=None, gsl_seed=0, macros={}),
    "eval_pulse_vrot": dict(kind="eval", model="pulse_vrot", n_data=1100, wl_seed=None, gsl_seed=0, macros={}),
}
# `analyse` alone, with the histogram range taken from the data and with another bin count
CASES["simplesin_analyse_minmax"] = _analyse(CASES, "simplesin", HISTOGRAMS_MINMAX=None)
CASES["simplesin_analyse_nbins37"] = _analyse(CASES, "simplesin", NBINS=37)
CASES["pulse_analyse_minmax"] = _analyse(CASES, "pulse", HISTOGRAMS_MINMAX=None)

# the run cases whose binary also runs `analyse` after `run` (the variant cases differ in how the chain moves,
# not in what analyse does with a dump, and are left out to keep the fixtures small)
ANALYSE_AFTER_RUN = ("simplesin", "simplesin_seed7", "pulse", "pulse_vrot")
ANALYSE_CASES = sorted(ANALYSE_AFTER_RUN) + sorted(c for c in CASES if CASES[c]["kind"] == "analyse")


def exe_path(case):
    return os.path.join(OUT_DIR, case + ".exe")


def command(case, ref=None):
    """the compiler call of one case (a list of arguments)"""
    ref = ref or reference_dir()
    c = CASES[case]
    src = sorted(os.path.join(ref, "src", f) for f in os.listdir(os.path.join(ref, "src")) if f.endswith(".c"))
    main = "eval_main.c" if c["kind"] == "eval" else "generic_main.c"
    cmd = ["gcc", "-I", os.path.join(ref, "src")] + CFLAGS
    cmd += ["-I", os.path.join(_HOST, "gsl"), "-I", os.path.join(_HERE, "refgsl")]
    for k, v in sorted(c["macros"].items()):
        cmd.append("-D%s" % k if v is None else "-D%s=%s" % (k, v))
    if "RWM" in c["macros"]:   # the reference's -DRWM does not compile as published: oracle/refgsl/rwm_compat.h
        cmd += ["-include", os.path.join(_HERE, "refgsl", "rwm_compat.h")]
    cmd += src + [os.path.join(ref, "apps", c["model"] + ".c"), os.path.join(ref, "apps", main),
                  os.path.join(_HOST, "src", "gslcompat.c")]
    return cmd + ["-o", exe_path(case)] + LDFLAGS


def _stamp(case, ref):
    """what the binary was built from: the command line and the modification times of its inputs"""
    cmd = command(case, ref)
    deps = [a for a in cmd if a.endswith((".c", ".h")) and os.path.isfile(a)]
    for d in (os.path.join(ref, "src"), os.path.join(_HOST, "gsl", "gsl"), os.path.join(_HERE, "refgsl", "gsl")):
        deps += [os.path.join(d, f) for f in sorted(os.listdir(d)) if f.endswith(".h")]
    return " ".join(cmd) + "\n" + "".join("%s %d\n" % (d, os.stat(d).st_mtime_ns) for d in deps)


def build_case(case, ref=None, force=False):
    ref = ref or reference_dir()
    os.makedirs(OUT_DIR, exist_ok=True)
    exe, stamp_file, stamp = exe_path(case), exe_path(case) + ".stamp", _stamp(case, ref)
    if not force and os.path.exists(exe) and os.path.exists(stamp_file):
        with open(stamp_file) as f:
            if f.read() == stamp:
                return exe
    subprocess.check_call(command(case, ref))
    with open(stamp_file, "w") as f:
        f.write(stamp)
    return exe


def build(cases=None, force=False, jobs=4):
    """Every case's binary into oracle/_ref/.  Returns [] without touching anything where the reference tree
    is absent (the GPU machine)."""
    if not have_reference():
        return []
    with ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(lambda c: build_case(c, force=force), cases or sorted(CASES)))


# ---- inputs of a case (ours: apemost_amd/workloads.py) and running its binary ---------------------------------

def workload(case):
    from apemost_amd import workloads as wl
    c = CASES[case]
    kw = dict(n_data=c["n_data"], n_chain=c["macros"].get("N_BETA", 2))
    if c["wl_seed"] is not None:
        kw["seed"] = c["wl_seed"]
    return wl.by_name(c["model"], **kw)


PHASES = ("calibrate_first", "calibrate_rest", "run")


def run_files(case):
    """names of the files a finished `run` phase leaves that are pinned"""
    w, n_beta = workload(case), CASES[case]["macros"]["N_BETA"]
    return (["acceptance_rate.dump"] + ["%s-chain-0.prob.dump" % n for n in w.names] +
            ["prob-chain%d.dump" % i for i in range(n_beta)])


def _env(case):
    env = dict(os.environ)
    env["GSL_RNG_SEED"] = str(CASES[case]["gsl_seed"])
    env["OMP_NUM_THREADS"] = "1"
    env.pop("GSL_RNG_TYPE", None)
    return env


def run_case(case, workdir):
    """Run a `run` case's binary through its phases in workdir, stopping at the first phase that fails.
    Returns {relative name: bytes}: "exit_status", and per phase the files the reference wrote.  An `analyse`
    case runs the phases of the case it is `of` with that case's binary (which must be built) and records only
    its own `analyse`."""
    if CASES[case]["kind"] == "analyse":
        run_case(CASES[case]["of"], workdir)
        out = run_analyse(case, workdir)
        out["exit_status"] = b"analyse %d\n" % out.pop("analyse/exit_status")
        return out
    w, exe, out, status = workload(case), exe_path(case), {}, []
    os.makedirs(workdir, exist_ok=True)
    with open(os.path.join(workdir, "params"), "w") as f:
        f.write(w.params_file_text())
    with open(os.path.join(workdir, "data"), "w") as f:
        f.write(w.data_file_text())
    for phase in PHASES:
        with open(os.path.join(workdir, phase + ".log"), "wb") as log:
            rc = subprocess.call([exe, phase], cwd=workdir, env=_env(case), stdout=log, stderr=subprocess.STDOUT)
        status.append("%s %d\n" % (phase, rc))
        names = run_files(case) if phase == "run" else ["calibration_results", "calibration_progress.data"]
        if rc != 0:   # a failed calibration writes no calibration_results of its own; its progress log is kept
            names = [n for n in names if n == "calibration_progress.data"]
        for n in names:
            with open(os.path.join(workdir, n), "rb") as f:
                out["%s/%s" % (phase, n)] = f.read()
        if rc != 0:
            break
    if case in ANALYSE_AFTER_RUN and rc == 0:
        out.update(run_analyse(case, workdir))
        status.append("analyse %d\n" % out.pop("analyse/exit_status"))
    out["exit_status"] = "".join(status).encode()
    return out


def analyse_files(case):
    """names of the files `analyse` writes"""
    return ["%s.histogram" % n for n in workload(case).names] + ["marginal_distributions.gnuplot"]


def cut_progress(stdout):
    """stdout without its progress segments: of every line what follows the last carriage return"""
    return "\n".join(line.split("\r")[-1] for line in stdout.decode().split("\n")).encode()


def run_analyse(case, workdir):
    """`analyse` of the case's binary in workdir, which holds a finished run: {"analyse/<file>": bytes} with the
    histogram files, the gnuplot file, "analyse/stdout" (cut_progress) and "analyse/exit_status" (an int)"""
    r = subprocess.run([exe_path(case), "analyse"], cwd=workdir, env=_env(case), stdout=subprocess.PIPE,
                       stderr=subprocess.DEVNULL)
    out = {"analyse/stdout": cut_progress(r.stdout), "analyse/exit_status": r.returncode}
    for n in analyse_files(case):
        with open(os.path.join(workdir, n), "rb") as f:
            out["analyse/" + n] = f.read()
    return out


# unit scalings of tests/test_gpu_parity.py::test_pulse_loglike_over_a_wide_range_of_units: frequencies (and
# 1 / lifetime) times sf, heights and data times sh
EVAL_UNITS = [("unit", 1.0, 1.0), ("heights_zero", 1.0, 1.0), ("f1e30_h1e200", 1e30, 1e200), ("f1e-30_h1e-200", 1e-30, 1e-200),
              ("f1e30_h1e-200", 1e30, 1e-200), ("f1e-30_h1e200", 1e-30, 1e200)]


def eval_units(case, sf, sh):
    """(data, params rows) of an eval case in other units: the workload's data scaled; the caller scales points"""
    w = workload(case)
    data = w.data.copy()
    data[:, 0] *= sf
    data[:, 1] *= sh
    return w, data


def eval_groups(case):
    """[(name, params_text, data_text, points_text)] of an eval case.  Group "unit": 24 points across the
    workload's box; group "heights_zero": one point with every height zero, where the reference does not
    print NaN but ABORTS -- gsl_sf_log(0) is a GSL domain error (apps/pulse.c:49, quirk Q8), and gslcompat.c
    keeps that; the other groups: 5 points each in scaled units.  eval_main asserts min <= v <= max (apps/eval_main.c:58-59), so the params file gets
    bounds that hold every scaling; points travel as %.17e, which scanf reads back exactly."""
    import numpy as np
    w = workload(case)
    pulse = CASES[case]["model"] == "pulse"
    heights, freqs = ([3, 5], [2, 4]) if pulse else ([4, 6], [2, 3, 5])
    rs = np.random.RandomState(5)
    base = w.pmin + (w.pmax - w.pmin) * rs.uniform(0.2, 0.8, size=(5, w.n_par))
    wide = w.pmin + (w.pmax - w.pmin) * rs.uniform(0.05, 0.95, size=(24, w.n_par))
    zero = base[:1].copy()
    zero[:, heights] = 0.0
    params_text = "".join("%.15e\t%.15e\t%.15e\t%s\t%.15e\n" % (s, -1e300, 1e300, n, 1.0)
                          for s, n in zip(w.start, w.names))
    out = []
    for name, sf, sh in EVAL_UNITS:
        _, data = eval_units(case, sf, sh)
        pts = (wide if name == "unit" else zero if name == "heights_zero" else base).copy()
        pts[:, 0] /= sf
        pts[:, freqs] *= sf
        pts[:, heights] *= sh
        data_text = "".join("\t".join("%.17e" % v for v in row) + "\n" for row in data)
        points_text = "".join("\t".join("%.17e" % v for v in row) + "\n" for row in pts)
        out.append((name, params_text, data_text, points_text))
    return out


DIGEST_ABOVE = 2048   # a file longer than this is recorded as digests and an excerpt
DIGEST_BLOCK = 100    # lines per block digest
EXCERPT = (4, 2)      # lines kept readable from the head and the tail


def digest_of(data):
    """what stands for a long file: its length, its SHA-256, and a short SHA-256 of every DIGEST_BLOCK lines,
    so that a mismatch is located to within one block"""
    import hashlib
    lines = data.splitlines(True)
    return dict(bytes=len(data), lines=len(lines), sha256=hashlib.sha256(data).hexdigest(),
                blocks=[hashlib.sha256(b"".join(lines[i:i + DIGEST_BLOCK])).hexdigest()[:8]
                        for i in range(0, len(lines), DIGEST_BLOCK)])


def to_fixture(case, got):
    """{relative name: bytes} as stored under tests/golden/ref_runs/<case>/, from what run_case() returned (or
    from what the oracle wrote in its place).  acceptance_rate.dump, calibration_results and analyse's stdout and
    gnuplot file are always stored whole.  Any other file longer than DIGEST_ABOVE (the dumps of a run of a thousand steps and more, a long
    calibration_progress.data) is replaced by an entry in <phase>/digests.json -- digest_of(): byte for byte
    still, and located to a block of DIGEST_BLOCK lines -- and by <name>.excerpt, its first and last lines as
    the reference wrote them."""
    import json
    out, digests = {}, {}
    for n in sorted(got):
        phase, _, base = n.rpartition("/")
        if (base in ("acceptance_rate.dump", "calibration_results") or n in ("analyse/stdout", "analyse/marginal_distributions.gnuplot")
                or len(got[n]) <= DIGEST_ABOVE):
            out[n] = got[n]
            continue
        digests.setdefault(phase, {})[base] = digest_of(got[n])
        lines = got[n].splitlines(True)
        out[n + ".excerpt"] = b"".join(lines[:EXCERPT[0]]) + b"...\n" + b"".join(lines[-EXCERPT[1]:])
    for phase, d in digests.items():   # one line per file
        out[phase + "/digests.json"] = ("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(d[k], sort_keys=True))
                                                            for k in sorted(d)) + "\n}\n").encode()
    return out


# ---- a case's fixture is ONE text file, tests/golden/ref_runs/<case>/files.txt: for every file a header line
# "### <relative name> <bytes>", then exactly that many bytes as the reference wrote them, then a newline.
# (One file per case and not a directory of twenty: the set is reviewed and diffed as fourteen files.)

def write_bundle(path, files):
    os.makedirs(os.path.dirname(path), exist_ok=True)
    with open(path, "wb") as f:
        for n in sorted(files):
            f.write(("### %s %d\n" % (n, len(files[n]))).encode() + files[n] + b"\n")


def read_bundle(path):
    out = {}
    with open(path, "rb") as f:
        while True:
            head = f.readline()
            if not head:
                return out
            mark, name, size = head.decode().split()
            assert mark == "###", head
            out[name] = f.read(int(size))
            assert len(out[name]) == int(size) and f.read(1) == b"\n", name


def fixture_path(golden_dir, case):
    return os.path.join(str(golden_dir), "ref_runs", case, "files.txt")


def eval_case(case, workdir, groups):
    """Run an `eval` case: groups = [(name, params_text, data_text, points_text)]; returns {name: (stdout bytes,
    exit status)}, the status as Python reports it (-6: ended by SIGABRT)"""
    out = {}
    for name, params_text, data_text, points_text in groups:
        d = os.path.join(workdir, name)
        os.makedirs(d, exist_ok=True)
        for fn, text in (("params", params_text), ("data", data_text)):
            with open(os.path.join(d, fn), "w") as f:
                f.write(text)
        r = subprocess.run([exe_path(case)], cwd=d, env=_env(case), input=points_text.encode(),
                           stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        out[name] = (r.stdout, r.returncode)
    return out


if __name__ == "__main__":
    if not have_reference():
        sys.exit("no reference tree at %s (set APEMOST_REFERENCE)" % reference_dir())
    for p in build(sys.argv[1:] or None):
        print(p)
