"""What on-device joint marginals cost on BASELINE config 2 (simplesin, 128 chains, 1024 points, built as bench.py
builds it), all in one session on one card:
  * the end-to-end rate of a run that folds every batch into the run summary (APEMOST_DUMP=summary) on the parent
    commit (--parent-tree: a checkout of it with its library built, whose own Python package and bench.py are used,
    since this commit's bindings ask for symbols the parent's library does not have) and on this one, and of one
    that also folds chain 0's rows into the pair histograms and moments (summary,joint), over 3 10^6 iterations;
  * bench.py's config 2 on both libraries;
  * the wall time of joint_get;
  * with --profile, in a separate `rocprofv3 --kernel-trace --stats` run of the summary,joint loop: the device time
    per batch of the three joint kernels against that of the round kernel for the same batch.

    python tools/joint_rate.py [--iterations 3000000] [--reps 5] [--parent-tree /path/to/parent/checkout]
                               [--profile] [--out profiles/joint_rates.txt]

Every repetition is a process of its own (one library per process: start, calibration, one warm-up run, one timed
run with the wall clock around the whole loop, batches double-buffered as the C host's run phase does), and the
cases take turns, so that the spread of a case holds what differs between processes -- repetitions inside one
process agree to 0.1 % and would understate it.  Each timed run must last at least a second.  Median, minimum and
maximum.  Two conditions are stated at the end: the joint kernels' device time per batch is below the round
kernel's, and bench.py and the summary rate of this commit lie within the parent's own spread in this session."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIG2 = dict(workload="simplesin", chains=128, n_data=1024, burn_in=10000, rounds=128)


def bench(tree):
    tree = tree or ROOT
    out = subprocess.run([sys.executable, os.path.join(tree, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5"],
                         cwd=tree, stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=600).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def worker(mode, iterations, reps, tree):
    """the run loop of one case in this process, on the package of `tree`; prints one JSON line"""
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    if tree:
        sys.path.insert(0, os.path.abspath(tree))
    from apemost_amd import capi, workloads as wl
    from apemost_amd.sampler import HipSampler, get_chain_beta
    from apemost_amd.state import LadderState
    from apemost_amd.summary import batches_closed
    c = CONFIG2
    n, R = c["chains"], c["rounds"]
    w = wl.by_name(c["workload"], n_data=c["n_data"], n_chain=n)
    n_swap = max(1, 2000 // n)
    steps = R * n_swap
    batches = (iterations + steps - 1) // steps
    kept = batches * steps
    st = LadderState.from_params(n, w.start, w.pmin, w.pmax, w.step * 0.3)
    for i in range(n):
        st.beta[i] = get_chain_beta(0, i, n, 0.02)
        st.step[i] = np.minimum(st.step[i] * st.beta[i] ** -0.5, w.pmax - w.pmin)
    s = HipSampler(w.model, w.n_par, n, w.data, seed=2024)
    s.set_state(st)
    s.calc_model(0, n)
    s.markov_chain_calibrate(0, n, capi.calib_defaults(burn_in_iterations=c["burn_in"]))
    rows = [C.c_void_p(), C.c_void_p()]
    for r in rows:
        capi.check(s.L.apemost_hip_samples_alloc(s._h, steps, C.byref(r)))
    bs = int(kept ** 0.5)
    with_joint = mode == "summary,joint"

    def run():
        s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=bs, max_batches=batches_closed(kept, bs))
        if with_joint:
            s.joint_begin(w.pmin, w.pmax, chains=(0,), nbins=200)
        s.synchronize()
        t0 = time.perf_counter()
        s.run_sampler(R, n_swap, rows[0])
        for b in range(batches):
            k = b & 1
            s.summary_accumulate(rows[k], steps)
            if with_joint:
                s.joint_accumulate(rows[k], steps)
            if b + 1 < batches:
                s.run_sampler(R, n_swap, rows[k ^ 1])        # the device goes on while this batch is folded
            capi.check(s.L.apemost_hip_samples_wait(s._h))
        s.synchronize()
        t = time.perf_counter() - t0
        s.summary_end()
        return t

    run()
    times = [run() for _ in range(reps)]
    out = dict(mode=mode, chains=n, kept=kept, batches=batches, steps=steps, times=times, library=capi.library_path(),
               device="%s (%d CUs)" % capi.device_info(0)[:2])
    if with_joint:
        gets = []
        for _ in range(reps + 1):                            # the accumulator of the last repetition is still there
            t0 = time.perf_counter()
            jt = s.joint()
            gets.append(time.perf_counter() - t0)
        out["gets"] = gets[1:]
        out["n"] = int(jt.n[0])
        out["corr01"] = float(jt.corr(0)[0, 1])
        s.joint_end()
    for r in rows:
        capi.check(s.L.apemost_hip_samples_free(s._h, r))
    s.close()
    print(json.dumps(out), flush=True)


def spawn(mode, iterations, reps, tree, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--worker", mode, "--iterations", str(iterations),
                          "--reps", str(reps)] + (["--parent-tree", tree] if tree else [])
    out = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=1100).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def spread(values):
    v = np.array(values)
    return np.median(v), v.min(), v.max()


def profile(iterations):
    """device time per batch of the joint kernels and of the round kernel, from rocprofv3's kernel statistics of one
    short summary,joint loop (the program itself goes after `--`)"""
    d = tempfile.mkdtemp(prefix="joint_prof_")
    r = spawn("summary,joint", iterations, 1, None,
              prefix=["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--"])
    stats = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
    assert stats, "no kernel statistics under %s" % d
    total, calls = {}, {}
    with open(stats[0]) as f:
        for row in csv.DictReader(f):
            total[row["Name"]] = total.get(row["Name"], 0) + int(row["TotalDurationNs"])
            calls[row["Name"]] = calls.get(row["Name"], 0) + int(row["Calls"])
    shutil.rmtree(d, ignore_errors=True)
    n_batches = 2 * r["batches"]                             # the warm-up run and one repetition
    joint = {k: v for k, v in total.items() if "joint_" in k}
    rounds = {k: v for k, v in total.items() if "pt_round" in k}
    summ = {k: v for k, v in total.items() if "summary_kernel" in k}
    assert joint and rounds, sorted(total)
    lines = ["  rocprofv3 --kernel-trace --stats, %d batches of %d steps x %d chains:" % (n_batches, r["steps"], r["chains"])]
    for k in sorted(rounds) + sorted(summ) + sorted(joint):
        lines.append("    %-60s %6d calls, %10.1f us per batch" % (k[:60], calls[k], total[k] / 1e3 / n_batches))
    j, rk = sum(joint.values()) / 1e3 / n_batches, sum(rounds.values()) / 1e3 / n_batches
    lines.append("    joint kernels %.1f us per batch, round kernel %.1f us per batch: %.2f %% of it" % (j, rk, 100 * j / rk))
    return lines, j < rk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--profile-iterations", type=int, default=200000)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iterations, a.reps, a.parent_tree)
    lines, rates, ok = [], {}, []
    cases = [("parent", "summary", a.parent_tree)] if a.parent_tree else []
    cases += [("this commit", "summary", None), ("this commit", "summary,joint", None)]
    runs = {}
    for _ in range(a.reps):                                  # the cases take turns, one process per repetition
        for label, mode, tree in cases:
            r = spawn(mode, a.iterations, 1, tree)
            assert min(r["times"]) >= 1.0, r["times"]
            runs.setdefault((label, mode), []).append(r)
    for label, mode, tree in cases:
        r = dict(runs[label, mode][0])
        r["times"] = [x["times"][0] for x in runs[label, mode]]
        if "gets" in r:
            r["gets"] = [x["gets"][0] for x in runs[label, mode]]
        if not lines:
            lines += ["# %s" % r["device"],
                      "# config 2: %d chains, %d iterations in %d batches of %d steps; %d processes per case, taking turns, "
                      "each one warm-up run and one timed run" % (r["chains"], r["kept"], r["batches"], r["steps"], a.reps)]
        rates[label, mode] = r["chains"] * r["kept"] / np.array(r["times"])
        med, lo, hi = spread(rates[label, mode])
        lines.append("  %-11s %-14s steps/s median %.4e  (%.4e .. %.4e, spread %.2f %%)" % (
            label, mode, med, lo, hi, 100 * (hi - lo) / med))
        print(lines[-1], flush=True)
        if "gets" in r:
            med, lo, hi = spread(r["gets"])
            lines.append("  joint_get of %d samples, 6 pairs x 200 x 200: median %.4f s  (%.4f .. %.4f); corr(0, 1) = %.4f"
                         % (r["n"], med, lo, hi, r["corr01"]))
            print(lines[-1], flush=True)
    benches = {}
    sides = ([("parent", a.parent_tree)] if a.parent_tree else []) + [("this commit", None)]
    for _ in range(a.reps):                                  # taking turns as well
        for label, tree in sides:
            benches.setdefault(label, []).append(bench(tree)["value"])
    for label, tree in sides:
        med, lo, hi = spread(benches[label])
        lines.append("  bench.py config 2, %-11s: median %.4e  (%.4e .. %.4e) steps/s" % (label, med, lo, hi))
        print(lines[-1], flush=True)
    if a.parent_tree:
        for what, parent, this in (("summary rate", rates["parent", "summary"], rates["this commit", "summary"]),
                                   ("bench.py", benches["parent"], benches["this commit"])):
            (pm, plo, phi), tm = spread(parent), float(np.median(this))
            good = abs(tm - pm) <= phi - plo
            ok.append(good)
            lines.append("  %s: this commit's median %.4e against the parent's %.4e, difference %.2f %%, parent's spread %.2f %%: %s"
                         % (what, tm, pm, 100 * (tm - pm) / pm, 100 * (phi - plo) / pm, "within" if good else "OUTSIDE"))
            print(lines[-1], flush=True)
    if a.profile:
        more, good = profile(a.profile_iterations)
        ok.append(good)
        lines += more + ["  joint kernels below the round kernel per batch: %s" % ("yes" if good else "NO")]
        print("\n".join(more + lines[-1:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if all(ok) else 1


if __name__ == "__main__":
    sys.exit(main())
