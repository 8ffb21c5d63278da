"""What on-device derived quantities cost on BASELINE config 2 (simplesin, 128 chains, 1024 points, built as bench.py
builds it): the device time per batch of the fold's kernels -- derived_gather_kernel, derived_marginal_kernel and the
joint fold's pair and moments kernels behind them -- beside that of the round kernel that wrote the batch's rows, from
a `rocprofv3 --kernel-trace --stats` run of a summary,derived loop; and the end-to-end rate of that loop against the
summary alone.

    python tools/derived_rate.py [--iterations 3000000] [--reps 5] [--profile-iterations 200000]
                                 [--out profiles/derived_rates.txt]

The columns are the ones a user of the sine models asks for: A cos 2 pi phi and A sin 2 pi phi (library group), a
difference and a ratio of parameters (exact group) and (prob - prior) / beta.  Every repetition is a process of its own
(start, calibration, one warm-up run, one timed run, batches double-buffered as the C host's run phase does), the cases
taking turns; median, minimum and maximum.  The profile is a run of its own: counters and timed runs do not mix.  The
condition stated at the end: the fold's kernels take less device time per batch than the round kernel."""
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
COLUMNS = ["p1 * cos(2 * 3.141592653589793 * p2)", "p1 * sin(2 * 3.141592653589793 * p2)", "p3 - p1", "p3 / p1", "like / 1.0"]
LO, HI = [-50.0, -50.0, -50.0, -50.0, -1e7], [50.0, 50.0, 50.0, 50.0, 0.0]
KERNELS = ("derived_", "joint_pair", "joint_moments")


def worker(mode, iterations, reps):
    """the run loop of one case in this process; prints one JSON line"""
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
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
    most = batches_closed(kept, bs)
    with_derived = mode == "summary,derived"

    def run():
        s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=bs, max_batches=most)
        if with_derived:
            s.derived_begin(COLUMNS, LO, HI, chains=(0,), nbins=200, batch_size=bs, max_batches=most)
        s.synchronize()
        t0 = time.perf_counter()
        s.run_sampler(R, n_swap, rows[0])
        for b in range(batches):
            k = b & 1
            s.summary_accumulate(rows[k], steps)
            if with_derived:
                s.derived_accumulate(rows[k], steps)
            if b + 1 < batches:
                s.run_sampler(R, n_swap, rows[k ^ 1])        # the device goes on while this batch is folded
            capi.check(s.L.apemost_hip_samples_wait(s._h))
        s.synchronize()
        t = time.perf_counter() - t0
        s.summary_end()
        return t

    run()
    times = [run() for _ in range(reps)]
    out = dict(mode=mode, chains=n, kept=kept, batches=batches, steps=steps, times=times,
               device="%s (%d CUs)" % capi.device_info(0)[:2])
    if with_derived:
        t0 = time.perf_counter()
        dv = s.derived()
        out["get"] = time.perf_counter() - t0
        out["n"] = int(dv.n[0])
        out["nonfinite"] = int(dv.nonfinite.sum())
        s.derived_end()
    for r in rows:
        capi.check(s.L.apemost_hip_samples_free(s._h, r))
    s.close()
    print(json.dumps(out), flush=True)


def spawn(mode, iterations, reps, prefix=()):
    cmd = list(prefix) + [sys.executable, os.path.abspath(__file__), "--worker", mode, "--iterations", str(iterations),
                          "--reps", str(reps)]
    out = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=1100).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def profile(iterations):
    """device time per batch of the fold's kernels and of the round kernel, from rocprofv3's kernel statistics of one
    short summary,derived loop (the program itself goes after `--`)"""
    d = tempfile.mkdtemp(prefix="derived_prof_")
    r = spawn("summary,derived", iterations, 1,
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
    fold = {k: v for k, v in total.items() if any(part in k for part in KERNELS)}
    rounds = {k: v for k, v in total.items() if "pt_round" in k}
    summ = {k: v for k, v in total.items() if "summary_kernel" in k}
    assert fold and rounds, sorted(total)
    lines = ["  rocprofv3 --kernel-trace --stats, %d batches of %d steps x %d chains, %d columns:" % (
        n_batches, r["steps"], r["chains"], len(COLUMNS))]
    for k in sorted(rounds) + sorted(summ) + sorted(fold):
        lines.append("    %-60s %6d calls, %10.1f us per batch" % (k[:60], calls[k], total[k] / 1e3 / n_batches))
    j, rk = sum(fold.values()) / 1e3 / n_batches, sum(rounds.values()) / 1e3 / n_batches
    lines.append("    derived fold %.1f us per batch, round kernel %.1f us per batch: %.2f %% of it" % (j, rk, 100 * j / rk))
    return lines, j < rk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--profile-iterations", type=int, default=200000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "derived_rates.txt"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.iterations, a.reps)
    lines, runs = [], {}
    modes = ("summary", "summary,derived")
    for _ in range(a.reps):                                  # the cases take turns, one process per repetition
        for mode in modes:
            r = spawn(mode, a.iterations, 1)
            assert min(r["times"]) >= 1.0, r["times"]
            runs.setdefault(mode, []).append(r)
    for mode in modes:
        r = runs[mode][0]
        if not lines:
            lines += ["# %s" % r["device"],
                      "# config 2: %d chains, %d iterations in %d batches of %d steps; %d processes per case, taking turns, "
                      "each one warm-up run and one timed run" % (r["chains"], r["kept"], r["batches"], r["steps"], a.reps)]
        rate = r["chains"] * r["kept"] / np.array([x["times"][0] for x in runs[mode]])
        lines.append("  %-16s steps/s median %.4e  (%.4e .. %.4e, spread %.2f %%)" % (
            mode, np.median(rate), rate.min(), rate.max(), 100 * (rate.max() - rate.min()) / np.median(rate)))
        print(lines[-1], flush=True)
        if "get" in r:
            gets = np.array([x["get"] for x in runs[mode]])
            lines.append("  derived_get of %d samples, %d columns, all pairs x 200 x 200: median %.4f s  (%.4f .. %.4f); "
                         "%d non-finite values" % (r["n"], len(COLUMNS), np.median(gets), gets.min(), gets.max(), r["nonfinite"]))
            print(lines[-1], flush=True)
    more, good = profile(a.profile_iterations)
    lines += more + ["  derived fold below the round kernel per batch: %s" % ("yes" if good else "NO")]
    print("\n".join(more + lines[-1:]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    return 0 if good else 1


if __name__ == "__main__":
    sys.exit(main())
