"""CPU restatement of replica-flow tracking (APEMOST_HIP_FLAG_TRACK_REPLICAS, include/apemost_hip.h): the checker of
tests/test_replica_flow_cpu.py and tests/test_gpu_replica_flow.py.  TEST INFRASTRUCTURE ONLY.

replay() applies the five rules of the specification to a list of swap attempts (round, lower rung, swapped).  The
lists come from the oracle's own primitives: tests/even_odd_ref.py for even-odd sweeps, and attempts_default() for the
reference's schedules -- the oracle a round at a time (orc.run_steps, the RWM / ADAPT blocks, orc.tempering_interaction),
the pair from the engine's schedule function (apemost_hip_swap_pair; -DRANDOMSWAP: word 1 of the attempt's Philox
block through orc_swap_pair_index), `swapped` from the difference of swapcount."""
import ctypes as C

import numpy as np

from apemost_amd import capi
from apemost_amd.replica_flow import ReplicaFlow, initial
from oracle import oracle as orc
from tests import even_odd_ref as eo

SWAP_SUBSEQUENCE = 1 << 63


def replay(n_chain, attempts, start=None):
    """the six arrays after `attempts` = [(r, a, swapped), ...], as a ReplicaFlow; start: a ReplicaFlow to go on from"""
    if start is None:
        replica, heading = initial(n_chain)
        n_up, n_down, att, trips = (np.zeros(n_chain, dtype=np.uint64) for _ in range(4))
    else:
        replica, heading, n_up, n_down, att, trips = (getattr(start, k).copy() for k in
                                                      ("replica", "heading", "n_up", "n_down", "attempts", "round_trips"))
    for _, a, swapped in attempts:
        assert 0 <= a < n_chain - 1
        b = a + 1
        if swapped:                                      # 1. the label follows params
            replica[[a, b]] = replica[[b, a]]
            heading[[a, b]] = heading[[b, a]]
        if a == 0:                                       # 2. the bottom end closes a round trip
            if heading[0] == 2:
                trips[replica[0]] += 1
            heading[0] = 1
        if b == n_chain - 1:                             # 3. the top end
            heading[b] = 2
        for rung in (a, b):                              # 4.
            if heading[rung] == 1:
                n_up[rung] += 1
            elif heading[rung] == 2:
                n_down[rung] += 1
        att[a] += 1                                      # 5.
    return ReplicaFlow(replica, heading, n_up, n_down, att, trips)


def attempts_default(lad, rng, n_rounds, n_swap, record=False, n_threads=1):
    """orc_run_sampler a round at a time under the default or the -DRANDOMSWAP schedule (lad.randomswap), with the
    list of attempts; (attempts, rows)"""
    assert lad.chain_offset == 0
    n, seed = lad.n_chain, int(rng.c.seed)
    attempts, rows = [], []
    for _ in range(n_rounds):
        out = orc.run_steps(lad, rng, n_swap, record=record, n_threads=n_threads)
        if record:
            rows.append(out)
        if lad.rwm:
            for c in range(n):
                orc.rwm(lad, rng, c)
        if lad.adapt:
            st = lad.c_state()
            for c in range(n):
                orc.lib().orc_adapt(C.byref(st), c)
        r = rng.round
        before = lad.swapcount.copy()
        orc.tempering_interaction(lad, rng)
        assert rng.round == r + 1
        if n < 2:
            continue
        if lad.randomswap:
            # (word 0, the swap_probability draw, is compared with 1.0 / 1: every uniform is below it)
            u = int(orc.philox_stream(seed, SWAP_SUBSEQUENCE, 1, start=4 * r + 1)[0]) / 4294967296.0
            a = int(orc.lib().orc_swap_pair_index(C.c_double(u), n))
        else:
            a = capi.swap_pair(seed, r, n)
        diff = lad.swapcount.astype(np.int64) - before.astype(np.int64)
        assert diff.sum() in (0, 1) and (diff.sum() == 0 or diff[a] == 1), (r, a, diff)
        attempts.append((r, a, bool(diff[a])))
    return attempts, (np.concatenate(rows) if record else None)


def attempts_even_odd(lad, rng, n_rounds, n_swap, record=False, n_threads=1):
    attempts = []
    rows = eo.run_sampler(lad, rng, n_rounds, n_swap, record=record, attempts=attempts, n_threads=n_threads)
    return attempts, rows


def oracle_flow(lad, rng, n_rounds, n_swap, even_odd=False, record=False, n_threads=1, start=None):
    """run the oracle and replay its attempts: (ReplicaFlow with the ladder's betas and swap counts, attempts, rows)"""
    fn = attempts_even_odd if even_odd else attempts_default
    attempts, rows = fn(lad, rng, n_rounds, n_swap, record=record, n_threads=n_threads)
    rf = replay(lad.n_chain, attempts, start=start)
    rf.beta, rf.swapcount = lad.beta.copy(), lad.swapcount.astype(np.uint64)
    return rf, attempts, rows
