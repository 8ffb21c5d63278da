"""What the residual periodogram's fold does per second, beside the predictive checks' fold, in one session on one card.

Folds over the same rows, in the same process, taking turns:
  * periodogram   apemost_hip_periodogram_begin at 1024 and at 4096 frequencies, Lomb-Scargle weights: five kernels per
                  piece (apemost_amd/csrc/pt_periodogram.h), of which periodogram_sum_kernel does 2 n L n_freq fused
                  multiply-adds in fp64;
  * check         apemost_hip_check_begin with 256 slots over the null quantiles, for scale.

The rows are those of LAUNCHES launches of a simplesin ladder of 8 chains over 1024 data (BASELINE config 2's data
length), laid end to end (7 680 kept steps); chain 0 is kept.  Every fold is run again and again for at least
--seconds.  The periodogram's rate is given in kept samples per second and as the share of the chip's vector fp64 peak
that its 2 n L n_freq multiply-adds reach: PEAK_FMA = 78.6e12 / 2 per second, AMD's figure for the MI355X's vector
fp64 (256 CUs x 4 SIMDs x 16 lanes per clock at 2.4 GHz; the clock a run really holds is lower, so the share understates
what the kernel does with the cycles it gets).

    python tools/periodogram_rate.py [--seconds 1.0] [--reps 3] [--out profiles/periodogram_rates.txt]

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

CONFIG = dict(chains=8, n_data=1024, rounds=32, n_swap=15)
LAUNCHES = 16
GRIDS = (1024, 4096)
MODES = tuple("periodogram_%d" % g for g in GRIDS) + ("check",)
PEAK_FMA = 78.6e12 / 2


def worker(seconds):
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    from apemost_amd import capi, workloads as wl
    from apemost_amd.sampler import HipSampler, get_chain_beta
    from apemost_amd.state import LadderState
    c = CONFIG
    n = c["chains"]
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
    span = w.data[-1, 0] - w.data[0, 0]
    grids = {g: np.linspace(1.0 / span, 0.99, g) for g in GRIDS}       # up to the Nyquist frequency of the 0.5 spacing

    def run(mode, calls):
        if mode == "check":
            s.check_begin(chains=[0])
            accumulate = s.check_accumulate
        else:
            s.periodogram_begin(chains=[0], freqs=grids[int(mode.split("_")[1])])
            accumulate = s.periodogram_accumulate
        s.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            accumulate(big, steps)
        capi.check(s.L.apemost_hip_samples_wait(s._h))
        return time.perf_counter() - t0

    probe = 2
    out = dict(device="%s (%d CUs)" % capi.device_info(0)[:2], steps=steps, n_data=c["n_data"])
    calls = {}
    for mode in MODES:
        run(mode, 1)                                         # the warm-up
        calls[mode] = max(probe, int(np.ceil(1.1 * probe * seconds / run(mode, probe))))
    for mode in MODES:                                       # the timed runs take turns
        t = run(mode, calls[mode])
        got = s.check() if mode == "check" else s.periodogram()
        assert int(got.n[0]) == calls[mode] * steps
        out[mode] = dict(time=t, calls=calls[mode], samples=calls[mode] * steps)
        if mode != "check":
            out[mode]["peak"] = list(got.peak_frequency()) + [got.peak_mean()]
    s.check_end()
    s.periodogram_end()
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
    peak_fma = PEAK_FMA
    lines = ["# %s: vector fp64 peak taken as %.3e FMA/s" % (first["device"], peak_fma),
             "# simplesin, chain 0 kept, %d data, calls of %d kept steps; %d processes, in each the folds take turns, each "
             "one timed run of at least %.1f s" % (first["n_data"], first["steps"], a.reps, a.seconds)]
    rate = {}
    for mode in MODES:
        rate[mode], text = stats([x[mode]["samples"] / x[mode]["time"] for x in got])
        lines.append("  %-17s kept samples/s %s" % (mode, text))
    for g in GRIDS:
        mode = "periodogram_%d" % g
        fma = 2.0 * first["n_data"] * g * rate[mode]
        lines.append("  %-17s %.3e FMA/s in the sums, %.3f of the peak; %.3f of the check fold's rate; peak frequency %.6f "
                     "(share %.3f, mean height %.3f)" % (mode, fma, fma / peak_fma,
                                                          rate[mode] / rate["check"], *got[-1][mode]["peak"]))
    text = "\n".join(lines) + "\n"
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
