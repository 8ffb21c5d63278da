"""CPU restatement of the even-odd swap schedule (APEMOST_HIP_FLAG_SWAP_EVEN_ODD, include/apemost_hip.h),
built from the oracle's exported primitives: the checker of tests/test_even_odd_cpu.py and
tests/test_gpu_even_odd.py.  TEST INFRASTRUCTURE ONLY.

Only the schedule is new.  A round is the oracle's own steps (orc.run_steps), then, with -DRWM / -DADAPT, the
oracle's own blocks in orc_run_sampler's order (RWM, ADAPT, then the swap attempt), then SWEEP r = rng.round:
every pair (a, a+1) with a % 2 == r % 2 is decided by check_swap_probability (orc_swap_decision,
src/parallel_tempering_interaction.c:25-42) with U = word 0 of Philox block r of subsequence 2^63 + 1 + a, and
applied as parallel_tempering_do_swap does (src/parallel_tempering_interaction.c:99-123): params exchanged, prob
left (quirk Q1), the larger prob_best and its point copied over the smaller (Q3), swapcount of the lower chain.
Whole ladders only (chain_offset 0)."""
import ctypes as C
import math

import numpy as np

from oracle import oracle as orc

SWAP_SUBSEQUENCE = 1 << 63


def sweep_pairs(r, n_chain):
    """lower chains of the pairs of sweep r"""
    return list(range(r % 2, n_chain - 1, 2))


def do_swap(lad, a):
    """parallel_tempering_do_swap, src/parallel_tempering_interaction.c:99-123"""
    b = a + 1
    lad.params[[a, b]] = lad.params[[b, a]]
    if lad.prob_best[a] > lad.prob_best[b]:
        lad.prob_best[b] = lad.prob_best[a]
        lad.params_best[b] = lad.params_best[a]
    else:
        lad.prob_best[a] = lad.prob_best[b]
        lad.params_best[a] = lad.params_best[b]


def sweep(lad, rng, attempts=None):
    """swap attempt rng.round under the even-odd schedule; attempts (a list) receives (sweep, pair, swapped)"""
    assert lad.chain_offset == 0
    r, seed = rng.round, int(rng.c.seed)
    for a in sweep_pairs(r, lad.n_chain):
        u = int(orc.philox_stream(seed, SWAP_SUBSEQUENCE + 1 + a, 1, start=4 * r)[0]) / 4294967296.0
        ln_u = math.log(u) if u > 0 else -math.inf
        swapped = orc.lib().orc_swap_decision(lad.beta[a], lad.beta[a + 1], lad.prob[a], lad.prob[a + 1], ln_u, None)
        if swapped:
            do_swap(lad, a)
            lad.swapcount[a] += 1
        if attempts is not None:
            attempts.append((r, a, bool(swapped)))
    rng.round = r + 1


def run_sampler(lad, rng, n_rounds, n_swap, record=False, attempts=None, n_threads=1):
    """orc_run_sampler with the sweep in the place of tempering_interaction"""
    rows = []
    for _ in range(n_rounds):
        out = orc.run_steps(lad, rng, n_swap, record=record, n_threads=n_threads)
        if record:
            rows.append(out)
        if lad.rwm:
            for c in range(lad.n_chain):
                orc.rwm(lad, rng, c)
        if lad.adapt:
            st = lad.c_state()
            for c in range(lad.n_chain):
                orc.lib().orc_adapt(C.byref(st), c)
        sweep(lad, rng, attempts)
    return np.concatenate(rows) if record else None
