"""Metropolis steps/s with and without replica-flow tracking (APEMOST_HIP_FLAG_TRACK_REPLICAS) on the shard workloads
of BASELINE configs 2 and 4 (built as bench.py builds them: same workload, ladder, calibration, rounds per batch,
sample rows written), timed with HIP events (apemost_hip_timer_*), under the default swap schedule and even-odd sweeps;
and, from the tracked runs, the ladder's round-trip rate, up-moving fractions and the betas suggest_betas gives.

    python tools/replica_flow_rate.py [--configs 2,4] [--reps 5] [--min-seconds 1.0] [--out profiles/replica_flow_rates.txt]
    APEMOST_HIP_LIB=/path/to/other/libapemost_hip.so python tools/replica_flow_rate.py --track off

Per case: one warm-up batch run, then `reps` timed repetitions of at least `min-seconds` each; median, minimum and
maximum of the repetitions.  The second form times another build of the library (the parent commit's) without the
flag."""
import argparse
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# bench.py's CONFIGS rows for one GPU (n_swap 0: 2000 // chains, the per-GPU-ladder rule)
CONFIGS = {2: dict(workload="simplesin", chains=128, n_data=1024, n_swap=0, burn_in=10000, rounds=128),
           4: dict(workload="pulse", chains=256, n_data=1024, n_swap=1, burn_in=2000, rounds=256)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default="2,4")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--schedules", default="default,even_odd")
    ap.add_argument("--track", default="off,on")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    os.environ.setdefault("APEMOST_NO_TORCH", "1")
    from apemost_amd import capi, workloads as wl
    from apemost_amd.sampler import HipSampler, get_chain_beta
    from apemost_amd.state import LadderState
    even_odd = getattr(capi, "FLAG_SWAP_EVEN_ODD", 2048)
    track = getattr(capi, "FLAG_TRACK_REPLICAS", 4096)
    # (randomswap: the reference's other one-pair-per-round schedule; it runs the variant kernels with and without
    # tracking, which the default schedule does only with it)
    flags_of = {"default": 0, "even_odd": even_odd, "randomswap": capi.FLAG_RANDOMSWAP}
    np.set_printoptions(precision=4, linewidth=200)
    name, cus, _ = capi.device_info(0)
    lines = ["# %s (%d CUs), library %s" % (name, cus, capi.library_path()),
             "# %d repetitions of >= %.1f s after one warm-up run; steps/s = chains x steps / HIP-event time" % (a.reps, a.min_seconds),
             "# config schedule track      steps/s median  (min .. max)               launches/rep  rounds/rep"]
    examples = []
    for cfg_id in [int(c) for c in a.configs.split(",")]:
        c = CONFIGS[cfg_id]
        n, R = c["chains"], c["rounds"]
        w = wl.by_name(c["workload"], n_data=c["n_data"], n_chain=n)
        n_swap = c["n_swap"] or max(1, 2000 // n)
        st = LadderState.from_params(n, w.start, w.pmin, w.pmax, w.step * 0.3)
        for i in range(n):
            st.beta[i] = get_chain_beta(0, i, n, 0.02)
            st.step[i] = np.minimum(st.step[i] * st.beta[i] ** -0.5, w.pmax - w.pmin)
        # one calibration (the default schedule's sampler: the calibration has no swaps), the same state for every schedule
        s = HipSampler(w.model, w.n_par, n, w.data, seed=2024)
        s.set_state(st)
        s.calc_model(0, n)
        status, _ = s.markov_chain_calibrate(0, n, capi.calib_defaults(burn_in_iterations=c["burn_in"]))
        calibrated = s.get_state()
        s.close()
        for sched, tr in [(x, y) for x in a.schedules.split(",") for y in a.track.split(",")]:
            s = HipSampler(w.model, w.n_par, n, w.data, seed=2024, flags=flags_of[sched] | (track if tr == "on" else 0))
            s.set_state(calibrated)
            rows = C.c_void_p()
            capi.check(s.L.apemost_hip_samples_alloc(s._h, R * n_swap, C.byref(rows)))

            def timed(batches):
                capi.check(s.L.apemost_hip_timer_begin(s._h))
                for _ in range(batches):
                    s.run_sampler(R, n_swap, rows)
                s.synchronize()
                ms, launches = C.c_float(0), C.c_uint64(0)
                capi.check(s.L.apemost_hip_timer_end(s._h, C.byref(ms), C.byref(launches)))
                return ms.value * 1e-3, launches.value

            t, _ = timed(4)                                  # warm-up, and the size of a repetition
            t, _ = timed(4)
            batches = max(4, int(np.ceil(4 * a.min_seconds * 1.15 / t)))
            rates, launches = [], 0
            for _ in range(a.reps):
                t, launches = timed(batches)
                assert t >= a.min_seconds * 0.9, t
                rates.append(n * batches * R * n_swap / t)
            rates = np.array(rates)
            ob, coop, max_rounds = s.launch_policy
            lines.append("  %d      %-9s %-3s   %.4e  (%.4e .. %.4e, spread %.2f %%)  %12d  %10d   # one-barrier %d helper %d"
                         % (cfg_id, sched, tr, np.median(rates), rates.min(), rates.max(),
                            100 * (rates.max() - rates.min()) / np.median(rates), launches, batches * R, ob, s.ob_helper))
            if tr == "on":
                rf, rounds = s.replica_flow(), s.round[0]
                examples += ["# config %d, %s schedule, %d chains, %d rounds of %d steps:" % (cfg_id, sched, n, rounds, n_swap),
                             "#   round trips %d (%.3e per round), replicas with at least one %d, barrier %.2f"
                             % (rf.round_trips.sum(), rf.round_trip_rate(rounds), (rf.round_trips > 0).sum(), rf.barrier),
                             "#   up fraction at rungs 0, n/8, .. n-1: %s" % rf.up_fraction[np.linspace(0, n - 1, 9).astype(int)],
                             "#   rejection of pairs 0, n/8, ..:        %s" % rf.rejection[np.linspace(0, n - 2, 9).astype(int)],
                             "#   betas now at rungs 0, n/8, .. n-1:    %s" % rf.beta[np.linspace(0, n - 1, 9).astype(int)],
                             "#   suggest_betas at the same rungs:      %s" % rf.suggest_betas()[np.linspace(0, n - 1, 9).astype(int)]]
            print(lines[-1], flush=True)
            capi.check(s.L.apemost_hip_samples_free(s._h, rows))
            s.close()
    text = "\n".join(lines + examples) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
