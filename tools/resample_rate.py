"""What one resampling costs at BASELINE config 2's ladder (128 chains, betas as bench.py sets them) with 10^5 kept steps
and four columns, for M = 4096 and M = 2^20 draws at one target: on the device (apemost_hip_reweight_resample on stores
loaded with mbar_set and reweight_set) and on the host (Reweight.resample_numpy, the same rule, its row pass on
--threads host threads), on the same columns.

    python tools/resample_rate.py [--steps 100000] [--draws 4096 1048576] [--threads 16] [--reps 5] [--out profiles/resample_rates.txt]

The columns are synthetic (the conjugate Gaussian problem of tests/mbar_ref.py in 4 dimensions with its draws: the cost
does not depend on the values).  Device: two warm-up calls, one call of 10 that sizes the timed call to at least a
second, then --reps timed calls of that many resamplings, the wall clock around each call (a resampling returns when its
draws are on the host); median, minimum and maximum.  The split is by calls that stop earlier, each timed the same way:
    weights   apemost_hip_reweight_weights with no host array: the row pass, the maxima, e and q;
    scan      apemost_hip_reweight_resample with one draw, less `weights`: the tile sums, their scan, C of every
              sample (and a search of one thread);
    search    the whole resampling less the one with one draw: the search of M threads, the gather of n_cols values
              per draw and their copy to the host.
apemost_hip_reweight_evaluate of the same target (profiles/reweight_rates.txt) is timed beside them: the yardstick.
Host: one resample_numpy per M.  No figure is fixed in advance."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100000)
    ap.add_argument("--draws", type=int, nargs="+", default=[4096, 1 << 20])
    ap.add_argument("--chains", type=int, default=128)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0x9E3779B97F4A7C15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    from reweight_rate import timed
    from apemost_amd import capi, workloads as wl
    from apemost_amd.mbar import Mbar
    from apemost_amd.reweight import Reweight
    from apemost_amd.sampler import HipSampler, get_chain_beta
    K, D, T = a.chains, 4, a.steps
    betas = np.array([get_chain_beta(0, i, K, 0.02) for i in range(K)])
    w = wl.simplesin(n_data=16, n_chain=K)
    s = HipSampler(w.model, w.n_par, K, w.data, seed=1)
    lo, hi = [-4.0] * D, [4.0] * D
    lines = ["# %s (%d CUs); host: numpy %s, the row pass on %d threads" % (capi.device_info(0)[:2] + (np.__version__, a.threads)),
             "# config 2's ladder: %d chains, beta %.4g .. %.4g; %d columns, one target (beta = 1), u = %#x" % (K, betas[0], betas[-1], D, a.seed)]
    rng = np.random.default_rng(2)
    x = rng.standard_normal((D, T, K)) / np.sqrt(1.0 + betas)
    ell = -0.5 * (x * x).sum(axis=0)
    host_mb = Mbar(ell, betas, threads=a.threads)
    g = host_mb.start()
    host_rw = Reweight(x, np.arange(D), lo, hi, 200)
    s.mbar_begin(T, betas)
    s.reweight_begin(np.arange(D), lo, hi, 200)
    s.mbar_set(host_mb)
    s.reweight_set(host_rw)
    dev_mb = Mbar(ell, betas, sampler=s)
    dev_rw = Reweight(x, np.arange(D), lo, hi, 200, sampler=s)
    gp = g.ctypes.data_as(capi._dp)
    N = K * T

    def call(M):
        """k resamplings of M draws into arrays allocated once"""
        import ctypes as C
        index, xs, q = np.zeros(M, dtype=np.uint32), np.zeros((M, D)), np.zeros(1, dtype=np.uint64)
        out = capi.ReweightDraws(index=index.ctypes.data_as(C.POINTER(C.c_uint32)), x=xs.ctypes.data_as(capi._dp),
                                 q_total=q.ctypes.data_as(capi._up))
        return lambda k: [capi.check(s.L.apemost_hip_reweight_resample(s._h, 0, T, gp, 1.0, M, a.seed, C.byref(out)))
                          for _ in range(k)]

    def ms(times):
        return "%.4f ms median (%.4f .. %.4f)" % (1e3 * float(np.median(times)), 1e3 * min(times), 1e3 * max(times))
    n_e, t_eval = timed(lambda k: [dev_rw.evaluate(dev_mb, [1.0], g=g, t0=0, t_count=T) for _ in range(k)], a.reps, a.seconds)
    n_w, t_w = timed(lambda k: [capi.check(s.L.apemost_hip_reweight_weights(s._h, 0, T, gp, 1.0, None, None)) for _ in range(k)],
                     a.reps, a.seconds)
    n_1, t_1 = timed(call(1), a.reps, a.seconds)
    ev, wt, one = float(np.median(t_eval)), float(np.median(t_w)), float(np.median(t_1))
    lines.append("T = %d kept steps, N = %d samples" % (T, N))
    lines.append("  reweight_evaluate, the same target, 200 bins: %d calls of %d: %s" % (a.reps, n_e, ms(t_eval)))
    lines.append("  weights (row pass, maxima, e and q):          %d calls of %d: %s" % (a.reps, n_w, ms(t_w)))
    lines.append("  resample, one draw:                           %d calls of %d: %s" % (a.reps, n_1, ms(t_1)))
    lines.append("  scan (one draw less weights): %.4f ms; it reads q twice and writes C once, 24 bytes per sample: %.3e B/s"
                 % (1e3 * (one - wt), 24.0 * N / max(one - wt, 1e-9)))
    print("\n".join(lines[-5:]), flush=True)
    for M in a.draws:
        n_m, t_m = timed(call(M), a.reps, a.seconds)
        med = float(np.median(t_m))
        got = dev_rw.resample(dev_mb, 1.0, M, a.seed, g=g, t0=0, t_count=T)
        t0 = time.perf_counter()
        want = host_rw.resample_numpy(host_mb, 1.0, M, a.seed, g=g, t0=0, t_count=T)
        h = time.perf_counter() - t0
        lines.append("M = %d draws" % M)
        lines.append("  device  %d calls of %d resamplings: %s, %.3e samples/s" % (a.reps, n_m, ms(t_m), N / med))
        lines.append("  split: weights %.4f ms, scan %.4f ms, search with gather and copy %.4f ms; against evaluate's %.4f ms: %.2f"
                     % (1e3 * wt, 1e3 * (one - wt), 1e3 * (med - one), 1e3 * ev, med / ev))
        lines.append("  host    1 resampling: %.1f ms; device against host: %.1f times the rate" % (1e3 * h, h / med))
        lines.append("  the two: %d of %d indices differ (numpy's exp against the device's), q_total by %.3g of it; means differ by at most %.3g"
                     % (int((got.index != want.index).sum()), M,
                        abs(int(got.q_total[0]) - int(want.q_total[0])) / float(want.q_total[0]),
                        float(np.abs(got.mean() - want.mean()).max())))
        print("\n".join(lines[-5:]), flush=True)
    s.mbar_end()
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
