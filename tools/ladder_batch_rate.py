#!/usr/bin/env python
"""Metropolis steps/s of many small ladders on one device, three ways:

  (a) sequential   the stand-alone samplers one after another (run, synchronise, next);
  (b) concurrent   the stand-alone samplers launched back to back on their own streams and synchronised together:
                   the best arrangement a library without ladder batches offers;
  (c) batch        one ladder batch (apemost_hip_create_batch).

Shapes (n_ladders x chains per ladder x data points): 16 x 8 x 1024 simplesin (n_swap 15), 32 x 8 x 1024 pulse
(n_swap 1: every step hands off) and 8 x 16 x 8192 sine3 (n_swap 15).  Every figure is the median of --repeats runs of
at least --seconds each (the rounds per run are sized from a first timed run), with the spread (max - min) / median
beside it.  A library without apemost_hip_create_batch (the parent commit's, selected with APEMOST_HIP_LIB) gives
(a) and (b) only.  One JSON line per shape and arrangement.

    python tools/ladder_batch_rate.py [--arrangements a,b,c] [--shapes simplesin,pulse,sine3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = {
    "simplesin": dict(n_ladders=16, per=8, n_data=1024, n_swap=15),
    "pulse": dict(n_ladders=32, per=8, n_data=1024, n_swap=1),
    "sine3": dict(n_ladders=8, per=16, n_data=8192, n_swap=15),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arrangements", default="a,b,c")
    ap.add_argument("--shapes", default="simplesin,pulse,sine3")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    from apemost_amd import capi, workloads as wl
    from apemost_amd.sampler import HipSampler
    from apemost_amd.state import ALL_FIELDS, LadderState
    from tests.helpers import make_pair

    has_batch = hasattr(capi.lib(), "apemost_hip_create_batch")
    for name in args.shapes.split(","):
        sh = SHAPES[name]
        n_ladders, per, n_swap = sh["n_ladders"], sh["per"], sh["n_swap"]
        ws = [wl.by_name(name, n_data=sh["n_data"], n_chain=per, seed=500 + 7 * b) for b in range(n_ladders)]
        seeds = [1000 + 13 * b for b in range(n_ladders)]
        sts = [make_pair(ws[b], per, seed=seeds[b], init_prob=True)[0] for b in range(n_ladders)]
        w = ws[0]
        for arr in args.arrangements.split(","):
            if arr == "c" and not has_batch:
                continue
            if arr == "c":
                whole = LadderState(n_ladders * per, w.n_par)
                for f in ALL_FIELDS:
                    getattr(whole, f)[...] = np.concatenate([getattr(s, f) for s in sts])
                samplers = [HipSampler.batch(w.model, w.n_par, per, np.stack([x.data for x in ws]), seeds)]
                samplers[0].set_state(whole)
            else:
                samplers = []
                for b in range(n_ladders):
                    s = HipSampler(w.model, w.n_par, per, ws[b].data, seed=seeds[b])
                    s.set_state(sts[b])
                    samplers.append(s)

            def once(n_rounds):
                t = time.perf_counter()
                if arr == "a":
                    for s in samplers:
                        s.run_sampler(n_rounds, n_swap)
                        s.synchronize()
                else:
                    for s in samplers:
                        s.run_sampler(n_rounds, n_swap)
                    for s in samplers:
                        s.synchronize()
                return time.perf_counter() - t

            once(64)                                     # warm-up: code objects loaded, clocks up
            probe = 256
            t = once(probe)
            n_rounds = max(probe, int(probe * args.seconds * 1.1 / t) + 1)
            rates = []
            for _ in range(args.repeats):
                t = once(n_rounds)
                rates.append(n_ladders * per * n_rounds * n_swap / t)
            med = float(np.median(rates))
            print(json.dumps(dict(shape="%d x %d x %d %s" % (n_ladders, per, sh["n_data"], name), n_swap=n_swap,
                                  arrangement={"a": "sequential", "b": "concurrent", "c": "batch"}[arr],
                                  waves=samplers[0].geometry[0], one_barrier=samplers[0].launch_policy[0],
                                  rounds_per_run=n_rounds, seconds_per_run=round(n_ladders * per * n_rounds * n_swap / med, 3),
                                  steps_per_s=med, spread=(max(rates) - min(rates)) / med,
                                  runs=[float("%.5g" % r) for r in rates])), flush=True)
            for s in samplers:
                s.close()


if __name__ == "__main__":
    main()
