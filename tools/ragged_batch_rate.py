#!/usr/bin/env python
"""Metropolis steps/s of a ragged ladder batch on one device, three arrangements in one session:

  (a) ragged      one batch of 16 ladders x 8 chains, simplesin, data lengths spread evenly from 256 to 1024
                  (apemost_hip_create_batch_ragged), four waves per chain, n_swap 15;
  (b) sequential  the same 16 ladders as stand-alone samplers, four waves per chain, one after another (run,
                  synchronise, next);
  (c) ceiling     an equal batch of 16 x 8 x 1024 (apemost_hip_create_batch): what the ragged batch's launch costs
                  if it lasts as long as its longest ladder's.

Every figure is the median of --repeats runs of at least --seconds each (the rounds per run are sized from a first
timed run), with the spread (max - min) / median beside it.  One JSON line per arrangement, then the ratios.

    python tools/ragged_batch_rate.py > profiles/ragged_batch_rates.txt
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_LADDERS, PER, N_SWAP, WAVES, SHORTEST, LONGEST = 16, 8, 15, 4, 256, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arrangements", default="a,b,c")
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()

    from apemost_amd import workloads as wl
    from apemost_amd.sampler import HipSampler
    from apemost_amd.state import ALL_FIELDS, LadderState
    from tests.helpers import make_pair

    ragged = [int(n) for n in np.linspace(SHORTEST, LONGEST, N_LADDERS).round()]
    seeds = [1000 + 13 * b for b in range(N_LADDERS)]
    med = {}
    for arr in args.arrangements.split(","):
        lengths = [LONGEST] * N_LADDERS if arr == "c" else ragged
        ws = [wl.by_name("simplesin", n_data=lengths[b], n_chain=PER, seed=500 + 7 * b) for b in range(N_LADDERS)]
        sts = [make_pair(ws[b], PER, seed=seeds[b], init_prob=True)[0] for b in range(N_LADDERS)]
        w = ws[0]
        if arr == "b":
            samplers = []
            for b in range(N_LADDERS):
                s = HipSampler(w.model, w.n_par, PER, ws[b].data, seed=seeds[b], waves_per_chain=WAVES)
                s.set_state(sts[b])
                samplers.append(s)
        else:
            whole = LadderState(N_LADDERS * PER, w.n_par)
            for f in ALL_FIELDS:
                getattr(whole, f)[...] = np.concatenate([getattr(s, f) for s in sts])
            samplers = [HipSampler.batch(w.model, w.n_par, PER, [x.data for x in ws], seeds, waves_per_chain=WAVES)]
            samplers[0].set_state(whole)
            assert samplers[0].n_data_per_ladder == lengths

        def once(n_rounds):
            t = time.perf_counter()
            for s in samplers:
                s.run_sampler(n_rounds, N_SWAP)
                s.synchronize()
            return time.perf_counter() - t

        once(64)                                     # warm-up: code objects loaded, clocks up
        probe = 256
        t = once(probe)
        n_rounds = max(probe, int(probe * args.seconds * 1.1 / t) + 1)
        rates = []
        for _ in range(args.repeats):
            t = once(n_rounds)
            rates.append(N_LADDERS * PER * n_rounds * N_SWAP / t)
        med[arr] = float(np.median(rates))
        print(json.dumps(dict(shape="%d x %d x %s simplesin" % (N_LADDERS, PER, "%d..%d" % (min(lengths), max(lengths))
                                                                 if arr != "c" else str(LONGEST)),
                              data_rows=sum(lengths), n_swap=N_SWAP,
                              arrangement={"a": "ragged batch", "b": "sequential", "c": "equal batch (ceiling)"}[arr],
                              waves=samplers[0].geometry[0], one_barrier=samplers[0].launch_policy[0],
                              rounds_per_run=n_rounds,
                              seconds_per_run=round(N_LADDERS * PER * n_rounds * N_SWAP / med[arr], 3),
                              steps_per_s=med[arr], spread=(max(rates) - min(rates)) / med[arr],
                              runs=[float("%.5g" % r) for r in rates])), flush=True)
        for s in samplers:
            s.close()
    ratios = {}
    if "a" in med and "b" in med:
        ratios["ragged_over_sequential"] = med["a"] / med["b"]
    if "a" in med and "c" in med:
        ratios["ragged_over_ceiling"] = med["a"] / med["c"]
    if ratios:
        print(json.dumps(ratios), flush=True)


if __name__ == "__main__":
    main()
