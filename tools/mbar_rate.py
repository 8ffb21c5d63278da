"""What one MBAR iteration costs at BASELINE config 2's ladder (128 chains, betas as bench.py sets them) with 10^4 and
10^5 kept steps: on the device (apemost_hip_mbar_iterate on a store loaded with mbar_set) and on the host (Mbar's numpy
passes, the same estimator in the same order, on --threads host threads), on the same column.  An iteration is
2 K N exponentials with N = K T samples; both rates are given in sample-exponentials per second.

    python tools/mbar_rate.py [--steps 10000 100000] [--threads 16] [--reps 5] [--out profiles/mbar_rates.txt]

The column is synthetic (the conjugate Gaussian problem of tests/mbar_ref.py in 4 dimensions: the cost does not depend
on the values).  Device: two warm-up iterations, one call of 20 that sizes the timed call to at least a second, then
--reps timed calls of that many iterations, the wall clock around each call (it returns when g is on the host); median,
minimum and maximum.  Host: one warm-up iteration and the median of three (two at 10^5 steps).  No figure is fixed in
advance; the last line of each size states the ratio."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    from apemost_amd import capi, workloads as wl
    from apemost_amd.mbar import Mbar
    from apemost_amd.sampler import HipSampler, get_chain_beta
    K = a.chains
    betas = np.array([get_chain_beta(0, i, K, 0.02) for i in range(K)])
    w = wl.simplesin(n_data=16, n_chain=K)
    s = HipSampler(w.model, w.n_par, K, w.data, seed=1)
    lines = ["# %s (%d CUs); host: numpy %s on %d threads" % (capi.device_info(0)[:2] + (np.__version__, a.threads)),
             "# config 2's ladder: %d chains, beta %.4g .. %.4g; one iteration = 2 K N exponentials, N = K T" % (K, betas[0], betas[-1])]
    rng = np.random.default_rng(2)
    for T in a.steps:
        ell = -0.5 * rng.chisquare(4, (T, K)) / (1.0 + betas)
        host = Mbar(ell, betas, threads=a.threads)
        g = host.start()
        exps = 2.0 * K * K * T
        s.mbar_begin(T, betas)
        s.mbar_set(host)
        dev = Mbar(ell, betas, sampler=s)
        dev.iterate(g, 2)
        t0 = time.perf_counter()
        dev.iterate(g, 20)
        per = (time.perf_counter() - t0) / 20
        n_iter = max(3, int(np.ceil(1.3 * a.seconds / per)))
        times = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            dev.iterate(g, n_iter)
            times.append((time.perf_counter() - t0) / n_iter)
        assert min(times) * n_iter >= a.seconds, (times, n_iter)
        g_dev, _ = dev.iterate(g, 1)
        s.mbar_end()
        d_med = float(np.median(times))
        lines.append("T = %d kept steps, N = %d samples, %.3e exponentials per iteration" % (T, K * T, exps))
        lines.append("  device  %d calls of %d iterations: %.4f ms per iteration median (%.4f .. %.4f), %.3e sample-exponentials/s"
                     % (a.reps, n_iter, 1e3 * d_med, 1e3 * min(times), 1e3 * max(times), exps / d_med))
        print("\n".join(lines[-2:]), flush=True)
        host.iterate(g, 1)
        h_times = []
        for _ in range(3 if T <= 20000 else 2):
            t0 = time.perf_counter()
            g_host, _ = host.iterate(g, 1)
            h_times.append(time.perf_counter() - t0)
        h_med = float(np.median(h_times))
        lines.append("  host    %d iterations on %d threads: %.1f ms per iteration median (%.1f .. %.1f), %.3e sample-exponentials/s"
                     % (len(h_times), a.threads, 1e3 * h_med, 1e3 * min(h_times), 1e3 * max(h_times), exps / h_med))
        lines.append("  device against host: %.1f times the rate" % (h_med / d_med))
        lines.append("  one iteration from the same g: the two differ by at most %.3g" % float(np.abs(g_dev - g_host).max()))
        print("\n".join(lines[-3:]), flush=True)
    s.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
