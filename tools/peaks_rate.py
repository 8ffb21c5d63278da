"""What on-device peaks cost on BASELINE config 2 (simplesin, 128 chains, 1024 points, built as bench.py builds it):
the end-to-end rate of a run that folds every batch into the run summary (APEMOST_DUMP=summary) against one that also
keeps chain 0's columns for peaks (summary,peaks), over 3 10^6 iterations; the wall time of peaks_get at that size; and
bench.py's config 2 on this build of the library and, with --parent-lib, on the parent commit's in the same session.

    python tools/peaks_rate.py [--iterations 3000000] [--reps 5] [--parent-lib /path/to/libapemost_hip.so]
                               [--out profiles/peaks_rates.txt]

Per case: one warm-up run, then `reps` timed repetitions (wall clock around the whole loop, batches double-buffered as
the C host's run phase does); each repetition must last at least a second.  Median, minimum and maximum."""
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

CONFIG2 = dict(workload="simplesin", chains=128, n_data=1024, burn_in=10000, rounds=128)


def bench(lib):
    env = dict(os.environ)
    if lib:
        env["APEMOST_HIP_LIB"] = lib
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "40", "--warmup", "5"],
                         env=env, stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=600).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iterations", type=int, default=3000000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
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
    batches = (a.iterations + steps - 1) // steps
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
    name, cus, _ = capi.device_info(0)
    lines = ["# %s (%d CUs), library %s" % (name, cus, capi.library_path()),
             "# config 2: %d chains, %d iterations in %d batches of %d steps; %d repetitions after one warm-up run"
             % (n, kept, batches, steps, a.reps)]

    def run(with_peaks):
        s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=bs, max_batches=batches_closed(kept, bs))
        if with_peaks:
            s.peaks_begin(w.pmin, w.pmax, chains=(0,), capacity=kept)
        s.synchronize()
        t0 = time.perf_counter()
        s.run_sampler(R, n_swap, rows[0])
        for b in range(batches):
            k = b & 1
            s.summary_accumulate(rows[k], steps)
            if with_peaks:
                s.peaks_accumulate(rows[k], steps)
            if b + 1 < batches:
                s.run_sampler(R, n_swap, rows[k ^ 1])        # the device goes on while this batch is folded
            capi.check(s.L.apemost_hip_samples_wait(s._h))
        s.synchronize()
        t = time.perf_counter() - t0
        s.summary_end()
        return t

    for label, with_peaks in (("summary", False), ("summary,peaks", True)):
        run(with_peaks)                                      # (peaks_begin drops the columns of the run before)
        times = []
        for _ in range(a.reps):
            times.append(run(with_peaks))
            assert times[-1] >= 1.0, times
        rates = n * kept / np.array(times)
        lines.append("  %-14s steps/s median %.4e  (%.4e .. %.4e, spread %.2f %%)" % (
            label, np.median(rates), rates.min(), rates.max(), 100 * (rates.max() - rates.min()) / np.median(rates)))
        print(lines[-1], flush=True)
    gets = []
    for _ in range(a.reps + 1):                              # the columns of the last repetition are still there
        t0 = time.perf_counter()
        pk = s.peaks()
        gets.append(time.perf_counter() - t0)
    gets = np.array(gets[1:])
    lines.append("  peaks_get of %d samples x %d parameters: median %.4f s  (%.4f .. %.4f); peaks per parameter %s"
                 % (kept, w.n_par, np.median(gets), gets.min(), gets.max(), pk.n_peaks[0].tolist()))
    print(lines[-1], flush=True)
    s.peaks_end()
    for r in rows:
        capi.check(s.L.apemost_hip_samples_free(s._h, r))
    s.close()
    for label, lib in (("this commit", None), ("parent", a.parent_lib)):
        if label == "parent" and not lib:
            continue
        values = [bench(lib)["value"] for _ in range(a.reps)]
        lines.append("  bench.py config 2, %-11s: median %.4e  (%.4e .. %.4e) steps/s" % (
            label, np.median(values), min(values), max(values)))
        print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
