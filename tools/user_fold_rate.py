"""What the folds of a user-supplied device model's optional hooks cost beside the built-in folds, in one session on
one card.

The posterior predictive and the pointwise log-likelihood fold of examples/device_models/simplesin2_hooks.hip
(apemost_amd/csrc/pt_user_fold.h: the hooks apemost_user_curve and apemost_user_pointwise) against the same two folds
of the built-in simplesin model at the same shape: chain 0 of a one-chain sampler over 1024 data, 65 536 kept steps a
call (eight staged pieces), no histograms.  The rows are the same draws for both models -- amplitude and frequency about
0.9 and 0.2 with the noise of a converged chain; the built-in model gets simplesin2's fixed phase 0.3312 and a zero
offset as its third and fourth parameter -- so both folds see the same curves.  The call is repeated for at least a
second; the rate is kept samples x data per second.  Also reported: hiprtc's time for the analysis module, the second
run-time module that holds the hooks' kernels.

    python tools/user_fold_rate.py [--seconds 1.2] [--reps 3] [--out profiles/user_fold_rates.txt]

Every repetition is a process of its own (start, one warm-up run, one short run that sizes the timed run, one timed run
with the wall clock around the whole loop), and the cases take turns.  Median, minimum and maximum.  No figure is fixed
in advance."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_DATA, KEPT = 1024, 65536
CASES = [(model, fold) for fold in ("predict", "pointwise") for model in ("simplesin2_hooks", "simplesin")]


def worker(model, fold, seconds):
    import torch
    from apemost_amd import capi, workloads as wl
    from apemost_amd.sampler import HipSampler
    rng = np.random.default_rng(7)
    x = 100 + 0.5 * np.arange(N_DATA)
    data = np.stack([x, 0.9 * np.sin(2 * np.pi * (0.2 * x + 0.3312)) + rng.normal(0, 0.5, N_DATA)], 1)
    user = model != "simplesin"
    n_par = 2 if user else 4
    rows = np.zeros((KEPT, 1, n_par + 2))
    rows[:, 0, :2] = np.array([0.9, 0.2]) + np.array([0.02, 2e-5]) * rng.standard_normal((KEPT, 2))
    if not user:
        rows[:, 0, 2] = 0.3312
    rows[:, 0, n_par:] = -700.0
    d = torch.from_numpy(rows).cuda()
    torch.cuda.synchronize()
    if user:
        src = os.path.join(ROOT, "apemost_amd", "host", "examples", "device_models", model + ".hip")
        s = HipSampler(wl.MODEL_USER, n_par, 1, data, seed=1, device_model_source=src)
        compile_seconds = s.user_hooks[2]
    else:
        s = HipSampler(wl.MODEL_SIMPLESIN, n_par, 1, data, seed=1)
        compile_seconds = 0.0

    def run(calls):
        getattr(s, fold + "_begin")(chains=(0,))
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            getattr(s, fold + "_accumulate")(d.data_ptr(), KEPT)
        capi.check(s.L.apemost_hip_samples_wait(s._h))
        return time.perf_counter() - t0

    probe = 2
    run(probe)
    t = run(probe)
    calls = max(probe, int(np.ceil(1.1 * probe * seconds / t)))
    t = run(calls)
    got = s.predict() if fold == "predict" else s.pointwise(at_mean=False)
    assert int(got.n[0]) == calls * KEPT
    mean = float(np.mean(got.mean(0) if fold == "predict" else got.mean_loglike(0)))
    s.close()
    print(json.dumps(dict(model=model, fold=fold, calls=calls, kept=calls * KEPT, time=t, evals=calls * KEPT * N_DATA,
                          compile_seconds=compile_seconds, mean=mean,
                          device="%s (%d CUs)" % capi.device_info(0)[:2])), flush=True)


def spawn(args):
    out = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, stdout=subprocess.PIPE,
                         universal_newlines=True, check=True, timeout=300).stdout
    return json.loads([l for l in out.splitlines() if l.startswith("{")][-1])


def stats(v):
    v = np.asarray(v, dtype=np.float64)
    med = float(np.median(v))
    return med, "median %.4e  (%.4e .. %.4e, spread %.2f %%)" % (med, v.min(), v.max(), 100 * (v.max() - v.min()) / med)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.2)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--worker", nargs=2, default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker[0], a.worker[1], a.seconds)
    runs = {}
    for _ in range(a.reps):                                  # the cases take turns, one process per repetition
        for case in CASES:
            r = spawn(["--worker", case[0], case[1], "--seconds", str(a.seconds)])
            assert r["time"] >= 1.0, r
            runs.setdefault(case, []).append(r)
    first = runs[CASES[0]][0]
    lines = ["# %s" % first["device"],
             "# the fold alone: chain 0 of a one-chain sampler, %d data, calls of %d kept steps, no histograms; %d processes "
             "per case, taking turns, each one timed run of at least a second" % (N_DATA, KEPT, a.reps)]
    med = {}
    for case in CASES:
        got = runs[case]
        med[case], text = stats([x["evals"] / x["time"] for x in got])
        lines.append("  %-17s %-10s kept samples x data per second %s, %.1f ms per 10^6 kept samples, mean value %.6g" % (
            case[0], case[1], text, float(np.median([1e3 * x["time"] / x["kept"] * 1e6 for x in got])), got[-1]["mean"]))
    for fold in ("predict", "pointwise"):
        lines.append("  %-10s the user fold runs at %.2f of the built-in fold's rate" % (
            fold, med["simplesin2_hooks", fold] / med["simplesin", fold]))
    secs = [x["compile_seconds"] for c in CASES if c[0] != "simplesin" for x in runs[c]]
    lines.append("# hiprtc's time for the analysis module of simplesin2_hooks.hip (every process compiles it once): %s s" %
                 stats(secs)[1])
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
