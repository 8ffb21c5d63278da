"""The optional hooks of a user-supplied device model (include/apemost_device_model.h: apemost_user_curve,
apemost_user_pointwise) without a device: the analysis translation unit -- what the engine compiles on the first
predict_* or pointwise_* call of such a sampler -- compiles for gfx950, and which hooks a source has is read off the
compilation, not off its text; the header, the library and HipSampler have the query; Predict and Pointwise files of
model 4 round-trip and leave the evaluation to the device."""
import os
import re

import numpy as np
import pytest

from apemost_amd import build, capi, device_model
from apemost_amd import workloads as wl
from apemost_amd.pointwise import STATE, Pointwise, loglike_numpy
from apemost_amd.predict import Predict, curve_numpy

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "apemost_amd", "host", "examples", "device_models")

TERM_AND_FINISH = '''#include "apemost_device_model.h"
__device__ double apemost_user_term(const apemost_model_ctx *ctx, int i) {
    const double r = ctx->params[0] + ctx->params[1] * APEMOST_DATA(ctx, i, 0) - APEMOST_DATA(ctx, i, 1);
    return r * r;
}
__device__ double apemost_user_finish(const apemost_model_ctx *ctx, double sum, double beta, double *prior) {
    (void)prior;
    return beta * sum / (-2 * ctx->sigma * ctx->sigma);
}
'''
POINTWISE_HOOK = '''#define APEMOST_USER_POINTWISE 1
__device__ double apemost_user_pointwise(const apemost_model_ctx *ctx, int i) {
    return apemost_user_term(ctx, i) / (-2 * ctx->sigma * ctx->sigma);
}
'''


@pytest.mark.parametrize("name", ["simplesin2_hooks", "bernoulli_hooks"])
def test_the_examples_with_hooks_compile_and_report_both(name):
    path = os.path.join(MODELS, name + ".hip")
    ok, log, size, hooks = device_model.compile_check(path, analysis=True)
    assert ok and size > 10000, log
    assert hooks == ("curve", "pointwise")
    # and they are device models like the others: the round module compiles, default kernels and one-barrier ones
    ok, log, size = device_model.compile_check(path, one_barrier=True)
    assert ok and size > 10000, log


def test_the_examples_keep_term_and_finish_of_their_originals():
    """the functions apemost_user_term and apemost_user_finish, text for text"""
    def function(text, name):
        m = re.search(r"__device__ double %s\(.*?\n}\n" % name, text, re.S)
        assert m, name
        return m.group(0)
    for hooks, original in (("simplesin2_hooks", "simplesin2"), ("bernoulli_hooks", "bernoulli_example")):
        a, b = (open(os.path.join(MODELS, f + ".hip")).read() for f in (hooks, original))
        for name in ("apemost_user_term", "apemost_user_finish"):
            assert function(a, name) == function(b, name), (hooks, name)


def test_a_source_without_hooks_compiles_and_reports_none():
    ok, log, size, hooks = device_model.compile_check(os.path.join(MODELS, "bernoulli_example.hip"), analysis=True)
    assert ok and size > 0, log
    assert hooks == ()


def test_one_hook_only(tmp_path):
    src = tmp_path / "pointwise_only.hip"
    src.write_text(TERM_AND_FINISH + POINTWISE_HOOK)
    ok, log, _, hooks = device_model.compile_check(str(src), analysis=True)
    assert ok, log
    assert hooks == ("pointwise",)


def test_a_macro_without_its_function_names_the_function(tmp_path):
    src = tmp_path / "no_function.hip"
    src.write_text(TERM_AND_FINISH + "#define APEMOST_USER_CURVE 1\n")
    ok, log, _, hooks = device_model.compile_check(str(src), analysis=True)
    assert not ok and hooks == ()
    assert "apemost_user_curve" in log


def test_a_comment_that_names_the_macro_announces_nothing(tmp_path):
    src = tmp_path / "comment.hip"
    src.write_text(TERM_AND_FINISH + "/* #define APEMOST_USER_CURVE 1 would announce apemost_user_curve() */\n"
                   "// APEMOST_USER_CURVE\n" + POINTWISE_HOOK)
    ok, log, _, hooks = device_model.compile_check(str(src), analysis=True)
    assert ok, log
    assert hooks == ("pointwise",)


def test_the_command_line_takes_analysis(tmp_path):
    import subprocess
    import sys
    src = tmp_path / "pointwise_only.hip"
    src.write_text(TERM_AND_FINISH + POINTWISE_HOOK)
    out = subprocess.run([sys.executable, "-m", "apemost_amd.device_model", "--analysis", str(src)], cwd=ROOT,
                         stdout=subprocess.PIPE, universal_newlines=True, timeout=300)
    assert out.returncode == 0 and "hooks: pointwise" in out.stdout and "curve" not in out.stdout, out.stdout


def test_header_library_and_sampler_have_the_query():
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    assert re.search(r"\bint apemost_hip_user_hooks\(", header)
    L = capi.lib()
    assert "apemost_hip_user_hooks" in capi.EXPORTS and L.apemost_hip_user_hooks.argtypes
    from apemost_amd.sampler import HipSampler
    assert isinstance(HipSampler.user_hooks, property)
    contract = open(os.path.join(ROOT, "include", "apemost_device_model.h")).read()
    for word in ("APEMOST_USER_CURVE", "APEMOST_USER_POINTWISE", "apemost_user_curve", "apemost_user_pointwise",
                 "pure functions of (ctx, i)"):
        assert word in contract, word


def test_the_round_kernels_sources_do_not_mention_the_hooks():
    csrc = os.path.join(ROOT, "apemost_amd", "csrc")
    for f in ("pt_device.h", "pt_onebarrier.h", "pt_kernels.h", "apemost_model.hip"):
        text = open(os.path.join(csrc, f)).read()
        assert "apemost_user_curve" not in text and "apemost_user_pointwise" not in text and "pt_user_fold" not in text, f


def test_files_of_model_4_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    K, D, P, B = 2, 5, 3, 4
    pw = Pointwise([7], *[rng.normal(size=(K, D)) for _ in STATE], rng.normal(size=(K, P)), rng.normal(size=(K, P)),
                   [0, 2], rng.normal(size=(K, D)), np.zeros((K, D)), P, wl.MODEL_USER, 0.37, 3)
    pw.write(str(tmp_path / "pointwise.bin"))
    back = Pointwise.read(str(tmp_path / "pointwise.bin"))
    assert back.model == wl.MODEL_USER == 4 and (back.n_keep, back.n_data, back.n_par, back.thin, back.sigma) == (K, D, P, 3, 0.37)
    for f in STATE + ("par_origin", "par_sum", "x", "y"):
        assert getattr(back, f).tobytes() == getattr(pw, f).tobytes(), f
    assert back.chains.tolist() == [0, 2] and int(back.n[0]) == 7
    assert back.text() == pw.text()
    pr = Predict([7], *[rng.normal(size=(K, D)) for _ in range(5)], rng.integers(0, 9, (K, D, B)).astype(np.uint64),
                 rng.normal(size=K), rng.normal(size=(K, P)), [3, 6], [0, 2], rng.normal(size=(K, D)), P, wl.MODEL_USER,
                 -1.0, 2.0, 3)
    pr.write(str(tmp_path / "predict.bin"))
    back = Predict.read(str(tmp_path / "predict.bin"))
    assert back.model == 4 and (back.n_keep, back.n_x, back.n_par, back.nbins, back.thin, back.lo, back.hi) == (K, D, P, B, 3, -1.0, 2.0)
    for f in ("origin", "sum", "sq", "vmin", "vmax", "hist", "best_prob", "best_params", "best_n", "x"):
        assert getattr(back, f).tobytes() == getattr(pr, f).tobytes(), f
    assert back.default_kind() == "difference"
    # the device is the only evaluator of a user model
    with pytest.raises(ValueError):
        curve_numpy(wl.MODEL_USER, np.zeros(P), np.zeros(D))
    with pytest.raises(ValueError):
        loglike_numpy(wl.MODEL_USER, np.zeros(P), np.zeros((D, 2)))
    with pytest.raises(ValueError):
        back.text(np.zeros(D))                                # (no best-fit curve without a sampler)
    assert back.text(np.zeros(D), best=np.zeros(D)).count("\n") == D
