"""What one reweighted evaluation costs at BASELINE config 2's ladder (128 chains, betas as bench.py sets them) with
10^4 and 10^5 kept steps: the parameters as columns, 200 bins, one target; on the device (apemost_hip_reweight_evaluate
on stores loaded with mbar_set and reweight_set) and on the host (Reweight.evaluate_numpy, the same estimator in the
same order, its row pass on --threads host threads), on the same columns.

    python tools/reweight_rate.py [--steps 10000 100000] [--threads 16] [--reps 5] [--out profiles/reweight_rates.txt]

The columns are synthetic (the conjugate Gaussian problem of tests/mbar_ref.py in 4 dimensions with its draws: the cost
does not depend on the values).  Device: two warm-up evaluations, one call of 10 that sizes the timed call to at least
a second, then --reps timed calls of that many evaluations, the wall clock around each call (an evaluation returns when
its sums are on the host); median, minimum and maximum.  An evaluation is the row pass (K exponentials per sample, what
apemost_hip_mbar_evaluate does too: it is timed beside it for the same target), then per target the maxima, e and q, the
moments, the histograms and the finish.  The kernels behind the row pass read at least 8 (2 + n_cols) bytes per sample
and do one exponential; the line `bandwidth` says which share of --hbm (the card's peak, 8 TB/s) those bytes over the
time of the whole evaluation, and over that time less apemost_hip_mbar_evaluate's, come to.  Host: one evaluation
(median of two at 10^4).  No figure is fixed in advance."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(call, reps, seconds):
    call(2)
    t0 = time.perf_counter()
    call(10)
    per = (time.perf_counter() - t0) / 10
    n = max(3, int(np.ceil(1.3 * seconds / per)))
    times = []
    for _ in range(reps):
        t0 = time.perf_counter()
        call(n)
        times.append((time.perf_counter() - t0) / n)
    assert min(times) * n >= seconds, (times, n)
    return n, times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, nargs="+", default=[10000, 100000])
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--bins", type=int, default=200)
    ap.add_argument("--hbm", type=float, default=8.0e12, help="the card's peak memory bandwidth, bytes per second")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    from apemost_amd import capi, workloads as wl
    from apemost_amd.mbar import Mbar
    from apemost_amd.reweight import Reweight
    from apemost_amd.sampler import HipSampler, get_chain_beta
    K, D = a.chains, 4
    betas = np.array([get_chain_beta(0, i, K, 0.02) for i in range(K)])
    w = wl.simplesin(n_data=16, n_chain=K)
    s = HipSampler(w.model, w.n_par, K, w.data, seed=1)
    lo, hi = [-4.0] * D, [4.0] * D
    lines = ["# %s (%d CUs); host: numpy %s, the row pass on %d threads" % (capi.device_info(0)[:2] + (np.__version__, a.threads)),
             "# config 2's ladder: %d chains, beta %.4g .. %.4g; %d columns, %d bins, one target (beta = 1)" % (K, betas[0], betas[-1], D, a.bins)]
    rng = np.random.default_rng(2)
    for T in a.steps:
        x = rng.standard_normal((D, T, K)) / np.sqrt(1.0 + betas)
        ell = -0.5 * (x * x).sum(axis=0)
        host_mb = Mbar(ell, betas, threads=a.threads)
        g = host_mb.start()
        host_rw = Reweight(x, np.arange(D), lo, hi, a.bins)
        s.mbar_begin(T, betas)
        s.reweight_begin(np.arange(D), lo, hi, a.bins)
        s.mbar_set(host_mb)
        s.reweight_set(host_rw)
        dev_mb = Mbar(ell, betas, sampler=s)
        dev_rw = Reweight(x, np.arange(D), lo, hi, a.bins, sampler=s)
        n, times = timed(lambda k: [dev_rw.evaluate(dev_mb, [1.0], g=g, t0=0, t_count=T) for _ in range(k)], a.reps, a.seconds)
        n_mb, times_mb = timed(lambda k: [dev_mb.evaluate([1.0], g=g, t0=0, t_count=T) for _ in range(k)], a.reps, a.seconds)
        got = dev_rw.evaluate(dev_mb, [1.0], g=g, t0=0, t_count=T)
        s.mbar_end()
        d_med, mb_med = float(np.median(times)), float(np.median(times_mb))
        N, bytes_ = K * T, 8.0 * (2 + D) * K * T
        lines.append("T = %d kept steps, N = %d samples, %.3e bytes at 8 (2 + %d) per sample" % (T, N, bytes_, D))
        lines.append("  device  %d calls of %d evaluations: %.4f ms per evaluation median (%.4f .. %.4f), %.3e samples/s"
                     % (a.reps, n, 1e3 * d_med, 1e3 * min(times), 1e3 * max(times), N / d_med))
        lines.append("  mbar_evaluate, the same target (row pass, maxima, four sums): %d calls of %d: %.4f ms median (%.4f .. %.4f)"
                     % (a.reps, n_mb, 1e3 * mb_med, 1e3 * min(times_mb), 1e3 * max(times_mb)))
        lines.append("  bandwidth: %.3e B/s over the whole evaluation, %.2f %% of %.3g B/s; %.3e B/s over it less mbar_evaluate's time, %.2f %%"
                     % (bytes_ / d_med, 100 * bytes_ / d_med / a.hbm, a.hbm, bytes_ / max(d_med - mb_med, 1e-9),
                        100 * bytes_ / max(d_med - mb_med, 1e-9) / a.hbm))
        print("\n".join(lines[-4:]), flush=True)
        h_times = []
        for _ in range(2 if T <= 20000 else 1):
            t0 = time.perf_counter()
            want = host_rw.evaluate_numpy(host_mb, [1.0], g=g, t0=0, t_count=T)
            h_times.append(time.perf_counter() - t0)
        h_med = float(np.median(h_times))
        lines.append("  host    %d evaluations: %.1f ms per evaluation median, %.3e samples/s" % (len(h_times), 1e3 * h_med, N / h_med))
        lines.append("  device against host: %.1f times the rate" % (h_med / d_med))
        lines.append("  the two: means differ by at most %.3g, ESS %.1f and %.1f, histograms by at most %.3g of q_total"
                     % (float(np.abs(got.mean() - want.mean()).max()), float(got.ess()[0]), float(want.ess()[0]),
                        float(np.abs(got.mass() - want.mass()).max())))
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
