"""What the pointwise fold at the caller's data and the joint predictive of a block cost, all in one session on one card.

Three folds over the same rows at the same (n_keep, n_data, n), in the same process, taking turns:
  * plain        apemost_hip_pointwise_begin: the kept chains scored on the sampler's own data;
  * at           apemost_hip_pointwise_begin_at at the same data, joint = 0.  The kernel is the same and so are its
                 arguments: the rate should be the plain fold's within the run-to-run spread;
  * at+joint     the same with joint = 1: behind every piece of the fold the two joint kernels
                 (apemost_amd/csrc/pt_pointwise_joint.h).  Their cost per kept sample x datum is the difference to `at`,
                 set against the fold's own: both evaluate one term, so the same order is expected.

The rows are those of LAUNCHES launches of a simplesin ladder of 8 chains over 1024 data, laid end to end (30 720 kept
steps, four staged pieces); the first 4 chains are kept.  Every fold is run again and again for at least --seconds; the
rate is in term evaluations per second, kept samples x kept chains x data.

    python tools/heldout_rate.py [--seconds 1.0] [--reps 3] [--out profiles/heldout_rates.txt]

Every repetition is a process of its own (start, one warm-up run per fold, one short run that sizes the timed run, one
timed run with the wall clock around the whole loop).  Median, minimum and maximum.  No figure is fixed in advance."""
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

CONFIG = dict(chains=8, keep=4, n_data=1024, rounds=128, n_swap=15)
LAUNCHES = 16
MODES = ("plain", "at", "at+joint")


def worker(seconds):
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    from apemost_amd import capi, workloads as wl
    from apemost_amd.sampler import HipSampler, get_chain_beta
    from apemost_amd.state import LadderState
    c = CONFIG
    n, keep = c["chains"], list(range(c["keep"]))
    w = wl.simplesin(n_data=c["n_data"], n_chain=n)
    steps = c["rounds"] * c["n_swap"]
    st = LadderState.from_params(n, w.start, w.pmin, w.pmax, w.step * 0.3)
    for i in range(n):
        st.beta[i] = get_chain_beta(0, i, n, 0.02)
        st.step[i] = np.minimum(st.step[i] * st.beta[i] ** -0.5, w.pmax - w.pmin)
    s = HipSampler(w.model, w.n_par, n, w.data, seed=2024)
    s.set_state(st)
    s.calc_model(0, n)
    row_bytes = n * (w.n_par + 2) * 8
    big = C.c_void_p()
    capi.check(s.L.apemost_hip_samples_alloc(s._h, LAUNCHES * steps, C.byref(big)))
    for b in range(LAUNCHES):
        s.run_sampler(c["rounds"], c["n_swap"], C.c_void_p(big.value + b * steps * row_bytes))
    s.synchronize()
    steps *= LAUNCHES

    def run(mode, calls):
        if mode == "plain":
            s.pointwise_begin(chains=keep)
        else:
            s.pointwise_begin(chains=keep, at=w.data[:, :2], joint=mode == "at+joint")
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            s.pointwise_accumulate(big, steps)
        capi.check(s.L.apemost_hip_samples_wait(s._h))
        return time.perf_counter() - t0

    probe, out = 2, dict(device="%s (%d CUs)" % capi.device_info(0)[:2], steps=steps, keep=len(keep), n_data=c["n_data"])
    calls = {}
    for mode in MODES:
        run(mode, probe)                                     # the warm-up
        calls[mode] = max(probe, int(np.ceil(1.1 * probe * seconds / run(mode, probe))))
    for mode in MODES:                                       # the timed runs take turns
        t = run(mode, calls[mode])
        pw = s.pointwise(at_mean=False)
        assert int(pw.n[0]) == calls[mode] * steps
        out[mode] = dict(time=t, calls=calls[mode], evals=calls[mode] * steps * len(keep) * c["n_data"])
        if mode == "at+joint":
            out["lpd_joint"] = s.pointwise_joint().lpd().tolist()
    s.pointwise_end()
    capi.check(s.L.apemost_hip_samples_free(s._h, big))
    s.close()
    print(json.dumps(out), flush=True)


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    med = float(np.median(v))
    return med, "median %.4e  (%.4e .. %.4e, spread %.2f %%)" % (med, v.min(), v.max(), 100 * (v.max() - v.min()) / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.seconds)
    got = []
    for _ in range(a.reps):
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--seconds", str(a.seconds)],
                             stdout=subprocess.PIPE, universal_newlines=True, check=True, timeout=300).stdout
        got.append(json.loads([l for l in out.splitlines() if l.startswith("{")][-1]))
    first = got[0]
    lines = ["# %s" % first["device"],
             "# simplesin, %d kept chains x %d data, calls of %d kept steps; %d processes, in each the three folds take "
             "turns, each one timed run of at least %.1f s" % (first["keep"], first["n_data"], first["steps"], a.reps,
                                                              a.seconds)]
    rate, cost = {}, {}
    for mode in MODES:
        r = [x[mode]["evals"] / x[mode]["time"] for x in got]
        rate[mode], text = stats(r)
        cost[mode] = float(np.median([1e12 * x[mode]["time"] / x[mode]["evals"] for x in got]))
        lines.append("  %-9s term evaluations/s %s, %.2f ps per kept sample x datum" % (mode, text, cost[mode]))
    lines.append("  at against plain: %+.2f %%" % (100 * (rate["at"] - rate["plain"]) / rate["plain"]))
    joint = float(np.median([1e12 * (x["at+joint"]["time"] / x["at+joint"]["evals"] - x["at"]["time"] / x["at"]["evals"])
                             for x in got]))
    lines.append("  the joint kernels: %.2f ps per kept sample x datum, %.2f of the fold's %.2f" % (
        joint, joint / cost["at"], cost["at"]))
    lines.append("  lpd_joint of the last run's blocks: %s" % " ".join("%.6e" % v for v in got[-1]["lpd_joint"]))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
