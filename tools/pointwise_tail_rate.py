"""What the tail of the pointwise fold costs (apemost_hip_pointwise_tail_*), all in one session on one card.  Modelled on
tools/pointwise_rate.py, whose set-up it uses.

  * The fold alone against fold + tail at capacity 3001 (what 10^6 kept samples need), per built-in model: chain 0 of a
    128-chain ladder over the model's workload of 1024 data.  The rows of 16 launches laid end to end (30 720 kept steps)
    are folded again and again for at least a second; ms per 10^6 kept samples.
  * The share of the compact kernel: one process of the simplesin fold + tail case under rocprofv3's kernel trace (a run
    of its own, never a timed one), the kernels' summed durations.  Left out with a note where rocprofv3 is not there.
  * Config 2 end to end through the summary sink, the run loop of tools/pointwise_rate.py, in chain steps per second:
    `summary` on the parent commit (--parent-tree: a checkout of it with its library built) and on this one,
    `summary,pointwise` without and with the tail, and with the tail folding every second sample (thin:2).  Fold +
    tail keeps up with the run where its ms per 10^6 kept samples of chain 0 stay below the time the ladder takes to
    produce them, 10^6 x chains / (the parent's steps/s); where it does not, the smallest thin at which it does is
    stated.  The end-to-end cases say what the run itself loses with the folds queued behind the summary's on one
    stream.
  * bench.py's default line, once on this commit and once in the parent's tree.

    python tools/pointwise_tail_rate.py [--seconds 1.2] [--reps 3] [--capacity 3001] [--parent-tree DIR]
                                      [--out profiles/pointwise_tail_rates.txt]

Every repetition is a process of its own and the cases take turns.  Median, minimum and maximum.  No figure is fixed in
advance."""
import argparse
import csv
import ctypes as C
import glob
import json
import math
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pointwise_rate as base  # noqa: E402

MODELS = base.MODELS
MODES = ("summary", "summary,pointwise", "summary,pointwise,tail", "summary,pointwise,tail,thin:2")


def worker_run(mode, seconds, tree, capacity):
    capi, w, s, rows, n, R, n_swap, steps = base.setup(tree)
    from apemost_amd.summary import batches_closed
    with_fold, with_tail = "pointwise" in mode, "tail" in mode
    thin = int(mode.rsplit("thin:", 1)[1]) if "thin:" in mode else 1     # (a batch's steps are a multiple of it)

    def run(batches):
        kept = batches * steps
        bs = int(kept ** 0.5)
        s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=bs, max_batches=batches_closed(kept, bs))
        if with_fold:
            s.pointwise_begin(chains=(0,), **(dict(tail=capacity) if with_tail else {}))
        s.synchronize()
        t0 = time.perf_counter()
        s.run_sampler(R, n_swap, rows[0])
        for b in range(batches):
            k = b & 1
            s.summary_accumulate(rows[k], steps)
            if with_fold:
                s.pointwise_accumulate(rows[k], steps, 0, thin)
            if b + 1 < batches:
                s.run_sampler(R, n_swap, rows[k ^ 1])        # the device goes on while this batch is folded
            capi.check(s.L.apemost_hip_samples_wait(s._h))
        s.synchronize()
        return time.perf_counter() - t0

    probe = 200
    run(probe)
    t = run(probe)
    batches = max(probe, int(np.ceil(1.1 * probe * seconds / t)))
    t = run(batches)
    out = dict(mode=mode, chains=n, steps=steps, batches=batches, kept=batches * steps, time=t,
               device="%s (%d CUs)" % capi.device_info(0)[:2])
    if with_tail:
        from apemost_amd import psis
        res = psis.psis(s.pointwise(at_mean=False), s.pointwise_tail())
        tab = res.k_table()
        out.update(n=res.n, tail_len=int(res.tail_len.max()), good=len(tab["good"]), bad=len(tab["bad"]),
                   very_bad=len(tab["very bad"]), k_max=float(res.k.max()))
    base.finish(capi, s, rows, out)


def worker_fold(workload, seconds, capacity, calls=None):
    """the fold alone (capacity 0) or fold + tail: the rows of base.LAUNCHES launches, accumulated in one call each time"""
    capi, w, s, rows, n, R, n_swap, steps = base.setup(None, workload, calibrate=False)
    row_bytes = n * (w.n_par + 2) * 8
    big = C.c_void_p()
    capi.check(s.L.apemost_hip_samples_alloc(s._h, base.LAUNCHES * steps, C.byref(big)))
    rows.append(big)
    for b in range(base.LAUNCHES):
        s.run_sampler(R, n_swap, C.c_void_p(big.value + b * steps * row_bytes))
    s.synchronize()
    steps *= base.LAUNCHES

    def run(count):
        s.pointwise_begin(chains=(0,), **(dict(tail=capacity) if capacity else {}))
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(count):
            s.pointwise_accumulate(big, steps)
        capi.check(s.L.apemost_hip_samples_wait(s._h))
        return time.perf_counter() - t0

    if calls is None:
        probe = 4
        run(probe)
        t = run(probe)
        calls = max(probe, int(np.ceil(1.1 * probe * seconds / t)))
    t = run(calls)
    pw = s.pointwise(at_mean=False)
    assert int(pw.n[0]) == calls * steps
    base.finish(capi, s, rows, dict(mode="fold", workload=workload, capacity=capacity, calls=calls, kept=calls * steps,
                                    n_data=pw.n_data, time=t, steps=steps, device="%s (%d CUs)" % capi.device_info(0)[:2]))


def spawn(args, tree=None):
    cmd = [sys.executable, os.path.abspath(__file__)] + args
    cmd += ["--parent-tree", tree] if tree else []
    out = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=300).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def kernel_shares(capacity):
    """{kernel name: summed ns} of one simplesin fold + tail process under rocprofv3's kernel trace, or a string saying why
    there is none"""
    tool = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(tool):
        return "rocprofv3 is not installed"
    with tempfile.TemporaryDirectory() as d:
        cmd = [tool, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
               "--worker", "fold", "--workload", "simplesin", "--capacity", str(capacity), "--calls", "8"]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return "rocprofv3 gave no kernel trace (exit status %d)" % r.returncode
        total = {}
        with open(files[0]) as f:
            for row in csv.DictReader(f):
                name = row.get("Kernel_Name", "")
                if "pointwise" in name:
                    short = name.split("(")[0].split("<")[0].split("::")[-1]
                    total[short] = total.get(short, 0) + int(row["End_Timestamp"]) - int(row["Start_Timestamp"])
        return total or "the trace names no pointwise kernel"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--capacity", type=int, default=3001)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--workload", default="simplesin", help=argparse.SUPPRESS)
    ap.add_argument("--calls", type=int, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker == "fold":
        return worker_fold(a.workload, a.seconds, a.capacity, a.calls)
    if a.worker:
        return worker_run(a.worker, a.seconds, a.parent_tree, a.capacity)
    lines, folds = [], {}
    for _ in range(a.reps):
        for model in MODELS:
            for cap in (0, a.capacity):
                r = spawn(["--worker", "fold", "--workload", model, "--seconds", str(a.seconds), "--capacity", str(cap)])
                assert r["time"] >= 1.0, r
                folds.setdefault((model, cap), []).append(r)
    first = folds[MODELS[0], 0][0]
    lines.append("# %s" % first["device"])
    lines.append("# the fold alone against fold + tail (capacity %d): chain 0 of a 128-chain ladder, %d data, calls of %d "
                 "kept steps; %d processes per case, taking turns, each one timed run of at least a second; ms per 10^6 "
                 "kept samples" % (a.capacity, first["n_data"], first["steps"], a.reps))
    ms = {}
    for model in MODELS:
        for cap in (0, a.capacity):
            ms[model, cap], text = base.stats([1e3 * x["time"] / x["kept"] * 1e6 for x in folds[model, cap]])
            lines.append("  %-10s %-12s %s" % (model, "fold + tail" if cap else "fold", text))
            print(lines[-1], flush=True)
        lines.append("  %-10s the tail adds %.1f %% to the fold" % (model, 100 * (ms[model, a.capacity] / ms[model, 0] - 1)))
    shares = kernel_shares(a.capacity)
    if isinstance(shares, str):
        lines.append("# the kernels' shares: not measured: %s" % shares)
    else:
        whole = float(sum(shares.values()))
        lines.append("# the kernels' shares of one simplesin fold + tail process under rocprofv3 --kernel-trace (8 calls, a "
                     "run of its own): " + ", ".join("%s %.1f %%" % (k, 100 * v / whole) for k, v in sorted(shares.items())))
    print(lines[-1], flush=True)
    cases = [("parent", "summary", a.parent_tree)] if a.parent_tree else []
    cases += [("this commit", m, None) for m in MODES]
    runs = {}
    for _ in range(a.reps):
        for label, mode, tree in cases:
            r = spawn(["--worker", mode, "--seconds", str(a.seconds), "--capacity", str(a.capacity)], tree)
            assert r["time"] >= 1.0, r
            runs.setdefault((label, mode), []).append(r)
    first = runs[cases[0][:2]][0]
    lines.append("# config 2 end to end: simplesin, %d chains, batches of %d steps, the folds of chain 0 over the %d data; %d "
                 "processes per case, taking turns, each one warm-up run and one timed run of at least a second" % (
                     first["chains"], first["steps"], base.CONFIG["n_data"], a.reps))
    med = {}
    for label, mode, tree in cases:
        med[label, mode], text = base.stats([x["chains"] * x["kept"] / x["time"] for x in runs[label, mode]])
        lines.append("  %-11s %-22s steps/s %s" % (label, mode, text))
        print(lines[-1], flush=True)
    assert first["steps"] % 2 == 0
    last = runs["this commit", MODES[2]][-1]
    lines.append("  chain 0 of the last run with the tail: %d samples, tail length %d, Pareto k good / bad / very bad at %d / %d / "
                 "%d data, largest k %.3f" % (last["n"], last["tail_len"], last["good"], last["bad"], last["very_bad"], last["k_max"]))
    ours = med["this commit", "summary"]
    for mode in MODES[1:]:
        lines.append("  %s against summary: %+.2f %%" % (mode, 100 * (med["this commit", mode] - ours) / ours))
    yard = med["parent", "summary"] if a.parent_tree else ours
    if a.parent_tree:
        lines.append("  summary, this commit against the parent: %+.2f %%" % (100 * (ours - yard) / yard))
    produce = 1e3 * 1e6 * first["chains"] / yard
    cost = ms[base.CONFIG["workload"], a.capacity]
    lines.append("  the ladder produces 10^6 kept samples of chain 0 in %.1f ms (10^6 x %d / %s steps/s); fold + tail of %s takes "
                 "%.1f ms of them: it %s" % (produce, first["chains"], "the parent's" if a.parent_tree else "this commit's summary",
                                             base.CONFIG["workload"], cost,
                                             "keeps up" if cost < produce else
                                             "does NOT keep up: it does from thin:%d on" % int(math.ceil(cost / produce))))
    for mode in MODES[2:]:
        lines.append("  end to end with %s the run takes %.1f ms per 10^6 steps of a chain, against %.1f ms with summary alone" % (
            mode, 1e3 * 1e6 * first["chains"] / med["this commit", mode], 1e3 * 1e6 * first["chains"] / ours))
    here = base.bench_value(ROOT)
    lines.append("# bench.py --gpus 1, once on each commit (no fold begun)")
    lines.append("  this commit %.4e Metropolis steps/s" % here)
    if a.parent_tree:
        parent = base.bench_value(a.parent_tree)
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
