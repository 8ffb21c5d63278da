"""What the on-device evidence fold costs on BASELINE configs 2 (simplesin, 128 chains, 1024 points) and 4 (pulse, 256
chains, 1024 points, one step per round), built as bench.py builds them, all in one session on one card.  Per config
the end-to-end rate, in chain steps per second, of a double-buffered run loop as the C host's run phase drives it:
  * with no fold at all (the rows are only waited for) and with the run summary's fold, on the parent commit
    (--parent-tree: a checkout of it with its library built, whose own Python package is used, since this commit's
    bindings ask for symbols the parent's library does not have) and on this one;
  * with the evidence fold on all chains, alone and together with the summary's.

    python tools/evidence_rate.py [--seconds 1.2] [--reps 5] [--parent-tree /path/to/parent/checkout]
                                  [--out profiles/evidence_rates.txt]

Every repetition is a process of its own (one library per process: start, calibration, one warm-up run, one short run
that sizes the timed run to at least a second, one timed run with the wall clock around the whole loop), and the cases
take turns, so that the spread of a case holds what differs between processes.  Median, minimum and maximum of 5.  No
figure is fixed in advance; the last lines state each fold's cost against the run without it in this session."""
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

CONFIGS = {
    2: dict(workload="simplesin", chains=128, n_data=1024, n_swap=0, burn_in=10000, rounds=128),
    4: dict(workload="pulse", chains=256, n_data=1024, n_swap=1, burn_in=2000, rounds=256),
}
MODES = ("none", "summary", "evidence", "summary,evidence")


def worker(config, mode, seconds, tree):
    """the run loop of one case in this process, on the package of `tree`; prints one JSON line"""
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    if tree:
        sys.path.insert(0, os.path.abspath(tree))
    from apemost_amd import capi, workloads as wl
    from apemost_amd.sampler import HipSampler, get_chain_beta
    from apemost_amd.state import LadderState
    from apemost_amd.summary import batches_closed
    c = CONFIGS[config]
    n, R = c["chains"], c["rounds"]
    w = wl.by_name(c["workload"], n_data=c["n_data"], n_chain=n)
    n_swap = c["n_swap"] or max(1, 2000 // n)
    steps = R * n_swap
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
    with_summary, with_evidence = "summary" in mode, "evidence" in mode

    def run(batches):
        kept = batches * steps
        bs = int(kept ** 0.5)
        if with_summary:
            s.summary_begin(w.pmin, w.pmax, n_hist_chains=1, nbins=200, batch_size=bs, max_batches=batches_closed(kept, bs))
        if with_evidence:
            s.evidence_begin(batch_size=bs, max_batches=batches_closed(kept, bs))
        s.synchronize()
        t0 = time.perf_counter()
        s.run_sampler(R, n_swap, rows[0])
        for b in range(batches):
            k = b & 1
            if with_summary:
                s.summary_accumulate(rows[k], steps)
            if with_evidence:
                s.evidence_accumulate(rows[k], steps)
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
    out = dict(config=config, mode=mode, chains=n, steps=steps, batches=batches, kept=batches * steps, time=t,
               library=capi.library_path(), device="%s (%d CUs)" % capi.device_info(0)[:2])
    if with_evidence:
        ev = s.evidence()
        out["n"] = int(ev.n[0])
        out["corrected"] = ev.thermodynamic("corrected", "down")
        out["stepping_stone"] = ev.stepping_stone("up", "down")
        out["rectangle"] = ev.thermodynamic("rectangle")
    for r in rows:
        capi.check(s.L.apemost_hip_samples_free(s._h, r))
    s.close()
    print(json.dumps(out), flush=True)


def spawn(config, mode, seconds, tree):
    cmd = [sys.executable, os.path.abspath(__file__), "--worker", mode, "--config", str(config), "--seconds", str(seconds)]
    cmd += ["--parent-tree", tree] if tree else []
    out = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=300).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--configs", type=int, nargs="+", default=[2, 4], choices=sorted(CONFIGS))
    ap.add_argument("--parent-tree", default=None)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    ap.add_argument("--config", type=int, default=2, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.config, a.worker, a.seconds, a.parent_tree)
    lines = []
    for config in a.configs:
        cases = [("parent", m, a.parent_tree) for m in ("none", "summary")] if a.parent_tree else []
        cases += [("this commit", m, None) for m in MODES]
        runs = {}
        for _ in range(a.reps):                              # the cases take turns, one process per repetition
            for label, mode, tree in cases:
                r = spawn(config, mode, a.seconds, tree)
                assert r["time"] >= 1.0, r
                runs.setdefault((label, mode), []).append(r)
        first = runs[cases[0][:2]][0]
        if not lines:
            lines.append("# %s" % first["device"])
        lines.append("# config %d: %s, %d chains, batches of %d steps; %d processes per case, taking turns, each one warm-up "
                     "run and one timed run of at least a second" % (config, CONFIGS[config]["workload"], first["chains"],
                                                                     first["steps"], a.reps))
        med = {}
        for label, mode, tree in cases:
            rate = np.array([x["chains"] * x["kept"] / x["time"] for x in runs[label, mode]])
            med[label, mode] = float(np.median(rate))
            lines.append("  %-11s %-16s steps/s median %.4e  (%.4e .. %.4e, spread %.2f %%), %d .. %d batches" % (
                label, mode, med[label, mode], rate.min(), rate.max(), 100 * (rate.max() - rate.min()) / med[label, mode],
                min(x["batches"] for x in runs[label, mode]), max(x["batches"] for x in runs[label, mode])))
            print(lines[-1], flush=True)
        last = runs["this commit", "summary,evidence"][-1]
        lines.append("  ln p(D|M,I) of the last summary,evidence run, %d samples: rectangle %.4f, corrected trapezoid %.4f, "
                     "stepping stone %.4f" % (last["n"], last["rectangle"], last["corrected"], last["stepping_stone"]))
        base = med["this commit", "none"]
        for mode in MODES[1:]:
            lines.append("  %-16s against no fold: %+.2f %%" % (mode, 100 * (med["this commit", mode] - base) / base))
        lines.append("  summary,evidence against summary: %+.2f %%" % (
            100 * (med["this commit", "summary,evidence"] - med["this commit", "summary"]) / med["this commit", "summary"]))
        if a.parent_tree:
            for mode in ("none", "summary"):
                lines.append("  %-16s this commit against the parent: %+.2f %%" % (
                    mode, 100 * (med["this commit", mode] - med["parent", mode]) / med["parent", mode]))
        print("\n".join(lines[-7:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
