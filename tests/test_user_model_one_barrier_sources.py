"""CPU: the one-barrier kernels of a user-supplied device likelihood (APEMOST_HIP_FLAG_USER_ONE_BARRIER) compile
for gfx950 from the reference's three other example likelihoods, as apemost_hip_create hands them to hiprtc under
the flag: round and calibration kernels for the default instantiation, the round kernels only for a variant one."""
import os
import re
import subprocess
import sys
import tempfile

import pytest

from apemost_amd import capi, device_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = os.path.join(ROOT, "apemost_amd", "host", "examples", "device_models")
READELF = "/opt/rocm/lib/llvm/bin/llvm-readelf"


def _kernel_notes(code):
    """{kernel symbol: {note: value}} from the code object's metadata (as tools/kernel_resources.py reads it)"""
    with tempfile.NamedTemporaryFile(suffix=".co") as f:
        f.write(code)
        f.flush()
        notes = subprocess.check_output([READELF, "--notes", f.name]).decode()
    out, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s+(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if k == "name":
            cur = out.setdefault(v, {})
        elif k in ("vgpr_count", "vgpr_spill_count", "private_segment_fixed_size"):
            cur[k] = int(v)
    return out


def test_flag_value_matches_the_header():
    text = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    assert int(re.search(r"APEMOST_HIP_FLAG_USER_ONE_BARRIER\s*=\s*(\d+)", text).group(1)) == capi.FLAG_USER_ONE_BARRIER == 1024


@pytest.mark.parametrize("name", ["simplesin2", "bernoulli_example", "normal"])
def test_one_barrier_kernels_of_the_example_models_compile(name):
    src = os.path.join(MODELS, name + ".hip")
    ok, log, code = device_model.compile_check(src, one_barrier=True, code=True)
    assert ok, log
    notes = _kernel_notes(code)
    for w in (4, 8):
        for kern in ("pt_round_ob_kernelILi4ELi%dELb0ELb0E" % w, "pt_calibrate_ob_kernelILi4ELi%dELb0ELb0E" % w):
            assert any(kern in k for k in notes), (kern, sorted(notes))
    if name in ("simplesin2", "bernoulli_example"):
        # the round kernel of four likelihood waves keeps everything in registers
        (r4,) = [v for k, v in notes.items() if "pt_round_ob_kernelILi4ELi4ELb0ELb0E" in k]
        assert r4["private_segment_fixed_size"] == 0 and r4["vgpr_spill_count"] == 0, r4
    # the logistic-proposal instantiation: the round kernels only (the variants calibrate on the two-phase step)
    ok, log, code = device_model.compile_check(src, variant=True, one_barrier=True, code=True)
    assert ok, log
    notes = _kernel_notes(code)
    assert any("pt_round_ob_kernelILi12ELi4ELb0ELb0E" in k for k in notes), sorted(notes)
    assert not any("pt_calibrate_ob_kernel" in k for k in notes)


def test_the_command_line_names_the_one_barrier_kernels():
    r = subprocess.run([sys.executable, "-m", "apemost_amd.device_model", "--one-barrier", os.path.join(MODELS, "normal.hip")],
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert r.returncode == 0 and b"compiles" in r.stdout, r.stdout
