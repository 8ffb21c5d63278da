"""What the predictive checks' fold costs beside the pointwise fold, all in one session on one card.

Two folds over the same rows at the same (n_keep, n_data, n), in the same process, taking turns:
  * pointwise    apemost_hip_pointwise_begin: one kernel per piece, one term per kept sample x datum;
  * check        apemost_hip_check_begin with 256 slots over the null quantiles: three kernels per piece
                 (apemost_amd/csrc/pt_check.h).  The fold evaluates the same curve and term and, on top, the predictive
                 CDF (erfc for the sine models); the statistics' kernel evaluates the curve and the CDF a second time.

The rows are those of LAUNCHES launches of a simplesin ladder of 8 chains over 1024 data, laid end to end (30 720 kept
steps, four staged pieces); the first 4 chains are kept.  Every fold is run again and again for at least --seconds; the
rate is in term evaluations per second, kept samples x kept chains x data.

    python tools/check_rate.py [--seconds 1.0] [--reps 3] [--out profiles/check_rates.txt]

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
MODES = ("pointwise", "check")


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
        if mode == "pointwise":
            s.pointwise_begin(chains=keep)
            accumulate = s.pointwise_accumulate
        else:
            s.check_begin(chains=keep)
            accumulate = s.check_accumulate
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            accumulate(big, steps)
        capi.check(s.L.apemost_hip_samples_wait(s._h))
        return time.perf_counter() - t0

    probe, out = 2, dict(device="%s (%d CUs)" % capi.device_info(0)[:2], steps=steps, keep=len(keep), n_data=c["n_data"])
    calls = {}
    for mode in MODES:
        run(mode, probe)                                     # the warm-up
        calls[mode] = max(probe, int(np.ceil(1.1 * probe * seconds / run(mode, probe))))
    for mode in MODES:                                       # the timed runs take turns
        t = run(mode, calls[mode])
        got = s.pointwise(at_mean=False) if mode == "pointwise" else s.check()
        assert int(got.n[0]) == calls[mode] * steps
        out[mode] = dict(time=t, calls=calls[mode], evals=calls[mode] * steps * len(keep) * c["n_data"])
        if mode == "check":
            out["p_values"] = [got.p_value(q)[0] for q in range(3)]
    s.pointwise_end()
    s.check_end()
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
             "# simplesin, %d kept chains x %d data, calls of %d kept steps; %d processes, in each the two folds take "
             "turns, each one timed run of at least %.1f s" % (first["keep"], first["n_data"], first["steps"], a.reps,
                                                              a.seconds)]
    rate, cost = {}, {}
    for mode in MODES:
        r = [x[mode]["evals"] / x[mode]["time"] for x in got]
        rate[mode], text = stats(r)
        cost[mode] = float(np.median([1e12 * x[mode]["time"] / x[mode]["evals"] for x in got]))
        lines.append("  %-9s term evaluations/s %s, %.2f ps per kept sample x datum" % (mode, text, cost[mode]))
    lines.append("  check against pointwise: %.2f of its rate, %.2f ps more per kept sample x datum" % (
        rate["check"] / rate["pointwise"], cost["check"] - cost["pointwise"]))
    lines.append("  upper-tail p-values of FIT, EXTREME and SERIAL in the last run: %s" % " ".join("%.4f" % v for v in got[-1]["p_values"]))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
