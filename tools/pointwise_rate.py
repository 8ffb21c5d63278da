"""What the on-device pointwise log-likelihood fold costs, all in one session on one card.

  * The fold alone, per built-in model: chain 0 of a 128-chain ladder over the model's workload of 1024 data points, the
    term of every one of the 1024 data.  The rows of 16 launches laid end to end (30 720 kept steps, four staged
    pieces) are folded again and again for at least a second; the rate is in term evaluations per second, kept samples
    x data, and in ms per 10^6 kept samples.
  * Config 2 end to end through the summary sink, a double-buffered run loop as the C host's run phase drives it, in
    chain steps per second: with the run summary's fold alone, on the parent commit (--parent-tree: a checkout of it
    with its library built, whose own Python package is used, since this commit's bindings ask for symbols the
    parent's library does not have) and on this one, and with the pointwise fold of chain 0 beside it.  The fold keeps up
    with the run where its ms per 10^6 kept samples of chain 0 stay below the time the ladder takes to produce them,
    10^6 x chains / (the parent's steps/s).
  * bench.py's default line, once on this commit and once in the parent's tree: the value with no fold begun.

    python tools/pointwise_rate.py [--seconds 1.2] [--reps 5] [--parent-tree /path/to/parent/checkout]
                                 [--out profiles/pointwise_rates.txt]

Every repetition is a process of its own (start, one warm-up run, one short run that sizes the timed run to at least a
second, one timed run with the wall clock around the whole loop), and the cases take turns.  Median, minimum and
maximum.  No figure is fixed in advance."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG = dict(workload="simplesin", chains=128, n_data=1024, burn_in=10000, rounds=128)
MODELS = ("simplesin", "sine3", "pulse", "pulse_vrot")
LAUNCHES = 16                                                # launches whose rows make one call of the fold alone
MODES = ("summary", "summary,pointwise")


def setup(tree, workload=None, calibrate=True):
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    if tree:
        sys.path.insert(0, os.path.abspath(tree))
    from apemost_amd import capi, workloads as wl
    from apemost_amd.sampler import HipSampler, get_chain_beta
    from apemost_amd.state import LadderState
    c = CONFIG
    n, R = c["chains"], c["rounds"]
    w = wl.by_name(workload or c["workload"], n_data=c["n_data"], n_chain=n)
    n_swap = max(1, 2000 // n)
    steps = R * n_swap
    st = LadderState.from_params(n, w.start, w.pmin, w.pmax, w.step * 0.3)
    for i in range(n):
        st.beta[i] = get_chain_beta(0, i, n, 0.02)
        st.step[i] = np.minimum(st.step[i] * st.beta[i] ** -0.5, w.pmax - w.pmin)
    s = HipSampler(w.model, w.n_par, n, w.data, seed=2024)
    s.set_state(st)
    s.calc_model(0, n)
    if calibrate:
        s.markov_chain_calibrate(0, n, capi.calib_defaults(burn_in_iterations=c["burn_in"]))
    rows = [C.c_void_p(), C.c_void_p()]
    for r in rows:
        capi.check(s.L.apemost_hip_samples_alloc(s._h, steps, C.byref(r)))
    return capi, w, s, rows, n, R, n_swap, steps


def finish(capi, s, rows, out):
    for r in rows:
        capi.check(s.L.apemost_hip_samples_free(s._h, r))
    s.close()
    print(json.dumps(out), flush=True)


def worker_run(mode, seconds, tree):
    """the run loop of one case in this process, on the package of `tree`; prints one JSON line"""
    capi, w, s, rows, n, R, n_swap, steps = setup(tree)
    from apemost_amd.summary import batches_closed
    with_fold = "pointwise" in mode

    def run(batches):
        kept = batches * steps
        bs = int(kept ** 0.5)
        s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=bs, max_batches=batches_closed(kept, bs))
        if with_fold:
            s.pointwise_begin(chains=(0,))
        s.synchronize()
        t0 = time.perf_counter()
        s.run_sampler(R, n_swap, rows[0])
        for b in range(batches):
            k = b & 1
            s.summary_accumulate(rows[k], steps)
            if with_fold:
                s.pointwise_accumulate(rows[k], steps)
            if b + 1 < batches:
                s.run_sampler(R, n_swap, rows[k ^ 1])        # the device goes on while this batch is folded
            capi.check(s.L.apemost_hip_samples_wait(s._h))
        s.synchronize()
        return time.perf_counter() - t0

    probe = 200
    run(probe)                                               # the warm-up
    t = run(probe)                                           # sizes the timed run, with a tenth to spare
    batches = max(probe, int(np.ceil(1.1 * probe * seconds / t)))
    t = run(batches)
    out = dict(mode=mode, chains=n, steps=steps, batches=batches, kept=batches * steps, time=t,
               library=capi.library_path(), device="%s (%d CUs)" % capi.device_info(0)[:2])
    if with_fold:
        pw = s.pointwise()
        c = pw.criteria()
        out.update(n=int(pw.n[0]), n_data=pw.n_data, waic=c["waic"], looic=c["looic"], dic=c["dic"],
                   min_ess=float(pw.loo_ess().min()))
    finish(capi, s, rows, out)


def worker_fold(workload, seconds):
    """the fold alone: the rows of LAUNCHES launches, accumulated in one call each time, until at least `seconds` have
    passed"""
    capi, w, s, rows, n, R, n_swap, steps = setup(None, workload, calibrate=False)
    row_bytes = n * (w.n_par + 2) * 8
    big = C.c_void_p()
    capi.check(s.L.apemost_hip_samples_alloc(s._h, LAUNCHES * steps, C.byref(big)))
    rows.append(big)
    for b in range(LAUNCHES):
        s.run_sampler(R, n_swap, C.c_void_p(big.value + b * steps * row_bytes))
    s.synchronize()
    steps *= LAUNCHES

    def run(calls):
        s.pointwise_begin(chains=(0,))
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            s.pointwise_accumulate(big, steps)
        capi.check(s.L.apemost_hip_samples_wait(s._h))
        return time.perf_counter() - t0

    probe = 4
    run(probe)
    t = run(probe)
    calls = max(probe, int(np.ceil(1.1 * probe * seconds / t)))
    t = run(calls)
    pw = s.pointwise(at_mean=False)
    assert int(pw.n[0]) == calls * steps
    finish(capi, s, rows, dict(mode="fold", workload=workload, calls=calls, kept=calls * steps, n_data=pw.n_data,
                               time=t, steps=steps, evals=calls * steps * pw.n_data,
                               device="%s (%d CUs)" % capi.device_info(0)[:2]))


def spawn(args, tree=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    cmd += ["--parent-tree", tree] if tree else []
    out = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=300).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def bench_value(tree):
    """the value of bench.py's default line, run in `tree`"""
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "1"], cwd=os.path.abspath(tree), stdout=subprocess.PIPE,
                         universal_newlines=True, check=True, timeout=300).stdout
    return float(json.loads([l for l in out.splitlines() if l.startswith("{")][-1])["value"])


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    med = float(np.median(v))
    return med, "median %.4e  (%.4e .. %.4e, spread %.2f %%)" % (med, v.min(), v.max(), 100 * (v.max() - v.min()) / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workload", default="simplesin", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker == "fold":
        return worker_fold(a.workload, a.seconds)
    if a.worker:
        return worker_run(a.worker, a.seconds, a.parent_tree)
    lines = []
    folds = {}
    for _ in range(a.reps):
        for model in MODELS:
            r = spawn(["--worker", "fold", "--workload", model, "--seconds", str(a.seconds)])
            assert r["time"] >= 1.0, r
            folds.setdefault(model, []).append(r)
    first = folds[MODELS[0]][0]
    lines.append("# %s" % first["device"])
    lines.append("# the fold alone: chain 0 of a 128-chain ladder, %d data, calls of %d kept steps; %d processes per "
                 "case, taking turns, each one timed run of at least a second" % (first["n_data"], first["steps"], a.reps))
    fold_ms = {}
    for model in MODELS:
        got = folds[model]
        _, text = stats([x["evals"] / x["time"] for x in got])
        fold_ms[model], _ = stats([1e3 * x["time"] / x["kept"] * 1e6 for x in got])
        lines.append("  %-10s term evaluations/s %s, %.2f ms per 10^6 kept samples, %.1f us per call" % (
            model, text, fold_ms[model], float(np.median([1e6 * x["time"] / x["calls"] for x in got]))))
        print(lines[-1], flush=True)
    cases = [("parent", "summary", a.parent_tree)] if a.parent_tree else []
    cases += [("this commit", m, None) for m in MODES]
    runs = {}
    for _ in range(a.reps):                                  # the cases take turns, one process per repetition
        for label, mode, tree in cases:
            r = spawn(["--worker", mode, "--seconds", str(a.seconds)], tree)
            assert r["time"] >= 1.0, r
            runs.setdefault((label, mode), []).append(r)
    first = runs[cases[0][:2]][0]
    lines.append("# config 2 end to end: simplesin, %d chains, batches of %d steps, the pointwise fold of chain 0 over the "
                 "%d data; %d processes per case, taking turns, each one warm-up run and one timed "
                 "run of at least a second" % (first["chains"], first["steps"], CONFIG["n_data"], a.reps))
    med, spread = {}, {}
    for label, mode, tree in cases:
        rate = np.array([x["chains"] * x["kept"] / x["time"] for x in runs[label, mode]])
        med[label, mode], text = stats(rate)
        spread[label, mode] = 100 * (rate.max() - rate.min()) / med[label, mode]
        lines.append("  %-11s %-16s steps/s %s, %d .. %d batches" % (
            label, mode, text, min(x["batches"] for x in runs[label, mode]), max(x["batches"] for x in runs[label, mode])))
        print(lines[-1], flush=True)
    last = runs["this commit", "summary,pointwise"][-1]
    lines.append("  chain 0 of the last summary,pointwise run: %d samples at %d data, waic %.3f, looic %.3f, dic %.3f, smallest "
                 "effective sample size of the leave-one-out weights %.1f" % (
                     last["n"], last["n_data"], last["waic"], last["looic"], last["dic"], last["min_ess"]))
    base = med["this commit", "summary"]
    lines.append("  summary,pointwise against summary: %+.2f %%" % (100 * (med["this commit", "summary,pointwise"] - base) / base))
    if a.parent_tree:
        lines.append("  summary         this commit against the parent: %+.2f %% (the parent's spread: %.2f %%)" % (
            100 * (base - med["parent", "summary"]) / med["parent", "summary"], spread["parent", "summary"]))
        lines.append("  summary,pointwise against the parent's summary: %+.2f %%" % (
            100 * (med["this commit", "summary,pointwise"] - med["parent", "summary"]) / med["parent", "summary"]))
        produce = 1e3 * 1e6 * first["chains"] / med["parent", "summary"]
        lines.append("  the ladder produces 10^6 kept samples of chain 0 in %.1f ms (10^6 x %d / the parent's steps/s); the fold "
                     "of %s takes %.1f ms of them: it %s" % (produce, first["chains"], CONFIG["workload"],
                                                             fold_ms[CONFIG["workload"]],
                                                             "keeps up" if fold_ms[CONFIG["workload"]] < produce else
                                                             "does NOT keep up: fold every thin-th sample"))
    here = bench_value(ROOT)
    lines.append("# bench.py --gpus 1, once on each commit (no fold begun)")
    lines.append("  this commit %.4e Metropolis steps/s" % here)
    if a.parent_tree:
        parent = bench_value(a.parent_tree)
        lines.append("  parent      %.4e Metropolis steps/s; this commit against the parent: %+.2f %%" % (
            parent, 100 * (here - parent) / parent))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
