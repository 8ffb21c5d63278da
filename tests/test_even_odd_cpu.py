"""Even-odd swap sweeps (APEMOST_HIP_FLAG_SWAP_EVEN_ODD), the parts that need no GPU: the flag and its documentation,
the C host's -DSWAP_EVEN_ODD, the CPU restatement of the schedule the GPU tests check against
(tests/even_odd_ref.py), and the variant kernels' build for gfx950."""
import os
import re
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi
from oracle import oracle as orc
from tests import even_odd_ref as eo
from tests import hostlib
from tests.helpers import make_pair, small_workloads

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the ladders of the GPU tests: 120 rounds x 3 steps, seed 23 (every pair attempted 60 times)
N_ROUNDS, N_SWAP, SEED = 120, 3, 23
LADDERS = [("simplesin", 8), ("simplesin", 7), ("simplesin", 9), ("pulse", 8), ("pulse_vrot", 8), ("sine3", 8)]
# two chains: with seed 23 the restatement never swaps in 120 rounds (the default schedule 7 times: other uniforms).
# Seed 11, 120 rounds: the restatement swaps 30 times in its 60 even sweeps (the default schedule 14 times).
TWO_CHAINS = dict(n_rounds=120, seed=11)


def test_flag_value_and_documentation():
    hdr = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    m = re.search(r"APEMOST_HIP_FLAG_SWAP_EVEN_ODD\s*=\s*(\d+)", hdr)
    assert m and int(m.group(1)) == capi.FLAG_SWAP_EVEN_ODD == 2048
    assert re.search(r"#define APEMOST_HIP_ABI_VERSION 3\b", hdr) and capi.ABI_VERSION == 3
    doc = hdr[hdr.index("Even-odd swap sweeps"):hdr.index("APEMOST_HIP_FLAG_SWAP_EVEN_ODD = 2048")]
    for phrase in ("a % 2 == r % 2", "APEMOST_HIP_SWAP_SUBSEQUENCE + 1 + a", "APEMOST_HIP_FLAG_RANDOMSWAP",
                   "APEMOST_HIP_FLAG_TEST_WITHHOLD_PUBLISH", "prob is not exchanged", "sits it"):
        assert phrase in doc, phrase
    for name in ("DESIGN.md", "README.md", "INTEGRATION.md"):
        assert "SWAP_EVEN_ODD" in open(os.path.join(ROOT, name)).read(), name


def test_c_host_builds_with_the_macro_strict_and_refuses_it_with_randomswap(tmp_path):
    """-DSWAP_EVEN_ODD on the application's compile line under the reference's -Werror -ansi -pedantic; together with
    -DRANDOMSWAP the build stops"""
    build.build_hip()
    exe = hostlib.make(str(tmp_path / "eo.exe"), ccflags="-DN_BETA=4 -DSWAP_EVEN_ODD")
    assert os.path.exists(exe)
    assert os.path.exists(hostlib.make(str(tmp_path / "eo2.exe"), ccflags="-DN_BETA=4 -DSWAP_EVEN_ODD -DPROPOSAL_UNIFORM -DADAPT"))
    with pytest.raises(subprocess.CalledProcessError):
        subprocess.check_call(["make", "-s", "-C", hostlib.HOST, "OUT=" + str(tmp_path / "no.exe"),
                               "CCFLAGS=-DN_BETA=4 -DSWAP_EVEN_ODD -DRANDOMSWAP"], stderr=subprocess.DEVNULL)
    assert not os.path.exists(str(tmp_path / "no.exe"))


def test_every_pair_is_attempted_exactly_in_the_sweeps_of_its_parity():
    w = small_workloads()["simplesin"]
    for n_chain in (2, 7, 8):
        st, lad, rng = make_pair(w, n_chain, seed=SEED)
        attempts = []
        eo.run_sampler(lad, rng, 11, 2, attempts=attempts)
        assert rng.round == 11
        want = [(r, a) for r in range(11) for a in range(n_chain - 1) if a % 2 == r % 2]
        assert [(r, a) for r, a, _ in attempts] == want, n_chain
        # the pairs of a sweep are disjoint
        for r in range(11):
            pairs = [a for rr, a, _ in attempts if rr == r]
            assert all(b - a >= 2 for a, b in zip(pairs, pairs[1:]))
    # two chains: the only pair is pair 0, attempted (and swapped) in even sweeps only
    assert eo.sweep_pairs(0, 2) == [0] and eo.sweep_pairs(1, 2) == [] and eo.sweep_pairs(1, 1) == []


def test_equal_betas_of_one_swap_at_every_attempt():
    """with all betas 1 the criterion is exactly 0 (p_b + p_a - (p_a + p_b)) and ln U < 0 for every U < 1"""
    w = small_workloads()["simplesin"]
    st, lad, rng = make_pair(w, 6, seed=SEED, init_prob=True)
    lad.beta[:] = 1.0
    for c in range(6):
        orc.calc_model(lad, c)
    attempts = []
    eo.run_sampler(lad, rng, 20, 2, attempts=attempts)
    assert len(attempts) == 10 * 3 + 10 * 2 and all(sw for _, _, sw in attempts)
    assert list(lad.swapcount) == [10, 10, 10, 10, 10, 0]


def test_do_swap_keeps_prob_and_copies_the_better_best_point():
    """quirks Q1 and Q3 of parallel_tempering_do_swap, as the oracle's own tempering_interaction applies them"""
    w = small_workloads()["simplesin"]
    st, lad, rng = make_pair(w, 2, seed=1, init_prob=True)
    lad.params[1] += 0.01
    lad.prob_best[:] = [-5.0, -3.0]
    lad.params_best[0], lad.params_best[1] = 1.0, 2.0
    prob, p0, p1 = lad.prob.copy(), lad.params[0].copy(), lad.params[1].copy()
    eo.do_swap(lad, 0)
    assert np.array_equal(lad.params[0], p1) and np.array_equal(lad.params[1], p0)
    assert np.array_equal(lad.prob, prob)
    assert list(lad.prob_best) == [-3.0, -3.0] and np.all(lad.params_best == 2.0)


def _counts(name, n_chain, n_rounds=N_ROUNDS, seed=SEED):
    w = small_workloads()[name]
    st, lad, rng = make_pair(w, n_chain, seed=seed)
    eo.run_sampler(lad, rng, n_rounds, N_SWAP, n_threads=8)
    st0, lad0, rng0 = make_pair(w, n_chain, seed=seed)
    orc.run_sampler(lad0, rng0, n_rounds, N_SWAP, n_threads=8)
    return lad.swapcount[:n_chain - 1].astype(np.int64), int(lad0.swapcount.sum())


def check_schedule_really_swaps(swapcount, default_total, n_rounds, first_round=0):
    """the conditions of the issue on a ladder's swap counts under the flag (shared with the GPU tests)"""
    n_pairs = len(swapcount)
    attempts = [sum(1 for r in range(first_round, first_round + n_rounds) if r % 2 == a % 2) for a in range(n_pairs)]
    assert swapcount.sum() >= 1.5 * default_total, (swapcount, default_total)
    assert all(swapcount[a] <= attempts[a] for a in range(n_pairs)), (swapcount, attempts)
    assert (swapcount == 0).sum() <= 1, swapcount


@pytest.mark.parametrize("name,n_chain", LADDERS)
def test_the_restatement_swaps_more_than_the_default_schedule(name, n_chain):
    """a condition on the fixtures, which the reference primitives alone must meet: so a change of the small
    workloads is caught without a GPU"""
    swapcount, default_total = _counts(name, n_chain)
    print(name, n_chain, swapcount, default_total)
    check_schedule_really_swaps(swapcount, default_total, N_ROUNDS)


def test_two_chains_swap_in_the_restatement():
    swapcount, default_total = _counts("simplesin", 2, TWO_CHAINS["n_rounds"], TWO_CHAINS["seed"])
    print(swapcount, default_total)
    assert 1 <= swapcount[0] <= TWO_CHAINS["n_rounds"] // 2


def test_variant_translation_unit_compiles_for_gfx950(tmp_path):
    """the kernels that carry the schedule: one variant translation unit (simplesin, MODEL + kVariantModel = 8),
    cross-compiled as build_hip() compiles it; no GPU needed"""
    obj = str(tmp_path / "model_8.o")
    flags = [f for f in build.HIP_FLAGS if f != "-shared"]
    subprocess.check_call([build.HIPCC] + flags + ["-c", "-I" + os.path.join(ROOT, "include"), "-I" + build.CSRC,
                                                   "-DAPEMOST_TU_MODEL=8", "-o", obj, os.path.join(build.CSRC, "apemost_model.hip")])
    assert os.path.getsize(obj) > 100000
    src = open(os.path.join(build.CSRC, "pt_kernels.h")).read() + open(os.path.join(build.CSRC, "pt_device.h")).read()
    assert "kVariantEvenOdd" in src and 8 in build.MODEL_TUS
