"""The tail of the pointwise fold without a GPU: the new symbols, the refusals that need no sampler, and the host build of
pt_pointwise_tail.h's inline helpers under the sanitizers (tests/tail_check.cpp, a program of its own)."""
import ctypes as C
import os
import subprocess

import numpy as np

from apemost_amd import build, capi
from apemost_amd.psis import PointwiseTail

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "apemost_amd", "csrc")
NAMES = ["apemost_hip_pointwise_tail_begin", "apemost_hip_pointwise_tail_get", "apemost_hip_pointwise_tail_set",
         "apemost_hip_pointwise_tail_capacity"]


def test_symbols_are_exported_and_declared():
    build.build_hip()
    L = capi.lib()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    for name in NAMES:
        assert name in capi.EXPORTS and getattr(L, name) is not None and ("int %s(" % name) in header, name
    assert "apemost_hip_pointwise_tail_view" in header and "#define APEMOST_HIP_ABI_VERSION 3" in header
    assert [f for f, _ in capi.PointwiseTailView._fields_] == ["count", "values"]
    assert L.apemost_hip_abi_version() == 3


def test_refusals_before_any_device_work():
    """without a card no sampler exists (tests/test_abi_errors.py): what can be refused here is the NULL sampler, and for
    tail_begin the capacity, which is looked at before the sampler's device is"""
    build.build_hip()
    L = capi.lib()
    t = PointwiseTail.empty((0,), 3, 4)
    cap = C.c_int32(7)
    for rc in (L.apemost_hip_pointwise_tail_begin(None, 8), L.apemost_hip_pointwise_tail_get(None, C.byref(t.view())),
               L.apemost_hip_pointwise_tail_set(None, C.byref(t.view())),
               L.apemost_hip_pointwise_tail_capacity(None, C.byref(cap))):
        assert rc == capi.ERR_INVALID and b"sampler is NULL" in L.apemost_hip_last_error()
    assert cap.value == 7


def test_helpers_built_by_the_host_compiler_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "tail_check")
    subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC,
                           "-I" + os.path.join(ROOT, "include"), "-Xarch_host", "-fsanitize=address,undefined",
                           "-Xarch_host", "-fno-sanitize-recover=all", os.path.join(HERE, "tail_check.cpp"), "-o", exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, universal_newlines=True, timeout=600)
    assert run.returncode == 0, run.stderr[-2000:]
    sets = {f[0]: (int(f[1]), int(f[2])) for f in (line.split() for line in run.stdout.splitlines())}
    for name in ("sizes", "layout", "network", "network_sizes", "order"):
        assert name in sets and sets[name][1] == 0, (name, sets)
    assert sets["sizes"][0] == 4095 and sets["network_sizes"][0] == 8191 and sets["layout"][0] == 2 * 3 * 2048 * 64
    assert sets["network"][0] == sum(range(2, 8193)) and sets["order"][0] == 7


def test_the_c_hosts_tail_file_reader_and_writer(tmp_path):
    """tests/pointwise_tail_check.c: the C host's reader and writer with a main of their own, built the way the
    run_pointwise.c check of tests/test_pointwise_cpu.py is.  The file's bytes survive the round trip, unused slots that
    hold something are written as 0 (PointwiseTail.write's bytes), the capacity rule is psis.capacity_for, and files of
    another kind are refused."""
    from apemost_amd.psis import capacity_for
    host = os.path.join(ROOT, "apemost_amd", "host")
    exe = str(tmp_path / "pointwise_tail_check")
    subprocess.check_call(["gcc", "-std=c99", "-ansi", "-pedantic", "-Wall", "-Wextra", "-Werror", "-O1", "-g",
                           "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(host, "include"),
                           os.path.join(HERE, "pointwise_tail_check.c"), os.path.join(host, "src", "run_pointwise.c"),
                           "-o", exe, "-lm"])
    rng = np.random.default_rng(4)
    count = np.array([[0, 1, 5, 3, 5, 2, 5]])
    values = -np.sort(-rng.standard_normal((1, 7, 5)), axis=2)
    values[0, 2, :2] = [np.inf, 0.0]
    values[0, 4, 3:] = [-0.0, -np.inf]
    t = PointwiseTail(count, values, 5, [0], 12345, thin=3)
    mine, dirty, out = str(tmp_path / "mine.bin"), str(tmp_path / "dirty.bin"), str(tmp_path / "out.bin")
    t.write(mine)
    raw = open(mine, "rb").read()
    # the same file with something in the unused slots, as pointwise_tail_get may leave them
    head = 56 + 4 + 8 * 7
    body = np.frombuffer(raw[head:], "<f8").reshape(7, 5).copy()
    body[np.arange(5)[None, :] >= count[0][:, None]] = 7.5
    open(dirty, "wb").write(raw[:head] + body.tobytes())
    for src in (mine, dirty):
        assert subprocess.run([exe, src, out], timeout=60).returncode == 0
        assert open(out, "rb").read() == raw
    for n in (1, 2, 10, 100, 3000, 20000, 10 ** 6, 1860000, 1870000, 10 ** 9):
        got = subprocess.run([exe, "capacity", str(n)], stdout=subprocess.PIPE, universal_newlines=True, timeout=60)
        assert got.returncode == 0 and int(got.stdout) == capacity_for(n), n
    open(dirty, "wb").write(b"APEMOSTW" + raw[8:])
    assert subprocess.run([exe, dirty, out], stderr=subprocess.PIPE, timeout=60).returncode == 1      # another magic
    open(dirty, "wb").write(raw[:-8])
    assert subprocess.run([exe, dirty, out], stderr=subprocess.PIPE, timeout=60).returncode == 1      # truncated
    two = PointwiseTail(np.ones((2, 3)), np.zeros((2, 3, 4)), 4, [0, 1], 9)
    two.write(dirty)
    assert subprocess.run([exe, dirty, out], timeout=60).returncode == 4                               # two kept chains
    assert subprocess.run([exe, str(tmp_path / "none.bin"), out], timeout=60).returncode == 2


def test_unused_slots_are_cleared():
    t = PointwiseTail(np.array([[1, 3]]), np.arange(8.0).reshape(1, 2, 4) + 1, 4, [0], 9)
    t.clear_unused()
    assert t.values.tolist() == [[[1.0, 0, 0, 0], [5.0, 6.0, 7.0, 0]]]
