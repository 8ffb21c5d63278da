"""The text sample dumps formatted on the device (apemost_amd/csrc/pt_text.h): the ABI
(apemost_hip_samples_text_read_async, HipSampler.samples_text) against glibc's snprintf on rows full of special
values, its buffer checks, and the C host's default text sink against the binary sink of the same run, every
file formatted with libc."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from apemost_amd import capi, workloads as wl
from tests import hostlib

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_libc = C.CDLL(None)
_libc.snprintf.restype = C.c_int


def _fmt(fmt, *vals):
    buf = C.create_string_buffer(64)
    n = _libc.snprintf(buf, 64, fmt, *[C.c_double(float(v)) for v in vals])
    return buf.raw[:n]


def _param_text(values):
    return b"".join(_fmt(b"%.15e\n", v) for v in values)


def _prob_text(pairs):
    return b"".join(_fmt(b"%6e\t%6e\n", a, b) for a, b in pairs)


def _specials():
    bits = [0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000, 0x7FF8000000000000,
            0xFFF8000000000000, 0x7FF0000000000001, 0x0000000000000001, 0x000FFFFFFFFFFFFF, 0x8000000000000001,
            0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x0010000000000000]
    v = list(np.array(bits, dtype=np.uint64).view(np.float64))
    v += [2.0 ** -11, 9.9999999e99, -9.9999999e99, 4.8828125e-04, 1e22, 1e-300, 0.5, 1.0, 9.5, 123456785.0]
    v += [np.ldexp(1.0, k) for k in range(-1074, 1024, 37)]
    return np.array(v, dtype=np.float64)


def _rows(n_steps, n_chains, n_par, seed=7):
    rs = np.random.RandomState(seed)
    rows = rs.normal(size=(n_steps, n_chains, n_par + 2)) * 10.0 ** rs.randint(-8, 9, size=(n_steps, n_chains, n_par + 2))
    hi, lo = (rs.randint(0, 2 ** 32, size=800).astype(np.uint64) for _ in range(2))
    pool = np.concatenate([_specials(), ((hi << np.uint64(32)) | lo).view(np.float64)])
    mask = rs.uniform(size=rows.shape) < 0.2
    rows[mask] = pool[rs.randint(0, len(pool), size=int(mask.sum()))]
    rows[0, 0, : len(_specials())] = _specials()[: n_par + 2]
    return rows


def _expected(rows, skip, thin, n_param_chains):
    kept = rows[skip::thin]
    n_par = rows.shape[2] - 2
    out = [_param_text(kept[:, c, p]) for c in range(n_param_chains) for p in range(n_par)]
    out += [_prob_text(kept[:, c, n_par:]) for c in range(rows.shape[1])]
    return out


def _sampler(n_chains):
    from apemost_amd.sampler import HipSampler
    w = wl.simplesin(n_data=64, n_chain=n_chains)
    return HipSampler(w.model, w.n_par, n_chains, w.data, seed=3), w.n_par


def test_samples_text_matches_libc_on_special_values():
    import torch
    n_chains, n_steps = 6, 2400
    s, n_par = _sampler(n_chains)
    rows = _rows(n_steps, n_chains, n_par)
    d = torch.tensor(rows, device="cuda")
    for skip, thin, npc in ((0, 1, 1), (2, 7, n_chains), (5, 3, 0), (0, 1, n_chains)):
        got = s.samples_text(d.data_ptr(), n_steps, skip, thin, npc)
        want = _expected(rows, skip, thin, npc)
        assert len(got) == len(want) == npc * n_par + n_chains
        for i, (g, w_) in enumerate(zip(got, want)):
            assert g == w_, (skip, thin, npc, i)
    # a batch that keeps no step: every stream empty
    assert s.samples_text(d.data_ptr(), 4, 9, 10, 1) == [b""] * (n_par + n_chains)
    s.close()


def test_samples_text_checks_every_buffer():
    import torch
    n_chains, n_steps, skip, thin, npc = 5, 700, 1, 2, 2
    s, n_par = _sampler(n_chains)
    rows = _rows(n_steps, n_chains, n_par, seed=11)
    d = torch.tensor(rows, device="cuda")
    torch.cuda.synchronize()
    n_streams, text_bytes, scratch_bytes = s.samples_text_bound(n_steps, skip, thin, npc)
    kept = len(range(skip, n_steps, thin))
    assert n_streams == npc * n_par + n_chains
    assert text_bytes == kept * (npc * n_par * 24 + n_chains * 30)
    L, h = s.L, s._h
    scratch = C.c_void_p()
    capi.check(L.apemost_hip_device_alloc(h, scratch_bytes, C.byref(scratch)))
    host = (C.c_char * (text_bytes + 64))()
    C.memset(host, 0xAB, len(host))
    offsets = np.full(n_streams + 2, 7, dtype=np.uint64)

    def read(sb, tc, no):
        return L.apemost_hip_samples_text_read_async(h, d.data_ptr(), n_steps, skip, thin, npc, scratch, sb,
                                                     C.addressof(host), tc, offsets.ctypes.data_as(capi._up), no)
    try:
        for sb, tc, no in ((scratch_bytes - 1, text_bytes, n_streams + 1), (scratch_bytes, text_bytes - 1, n_streams + 1),
                           (scratch_bytes, text_bytes, n_streams)):
            assert read(sb, tc, no) == capi.ERR_INVALID
            capi.check(L.apemost_hip_samples_wait(h))
            assert bytes(host) == b"\xab" * len(host) and (offsets == 7).all()     # nothing copied
        assert L.apemost_hip_samples_text_bound(h, n_steps, skip, 0, npc, None, None, None) == capi.ERR_INVALID
        assert L.apemost_hip_samples_text_bound(h, n_steps, skip, thin, n_chains + 1, None, None, None) == capi.ERR_INVALID
        capi.check(read(scratch_bytes, text_bytes, n_streams + 1))
        capi.check(L.apemost_hip_samples_wait(h))
    finally:
        capi.check(L.apemost_hip_device_free(h, scratch))
    off = offsets[: n_streams + 1].astype(np.int64)
    assert off[0] == 0 and (np.diff(off) >= 0).all() and off[-1] <= text_bytes and offsets[n_streams + 1] == 7
    text = bytes(host)
    want = _expected(rows, skip, thin, npc)
    assert off[-1] == sum(len(x) for x in want)
    assert [text[off[i]:off[i + 1]] for i in range(n_streams)] == want
    assert text[text_bytes:] == b"\xab" * 64                                       # nothing beyond the bound
    s.close()


# ---- the C host's text sink against its binary sink ----------------------------------------------------------
def _inputs(work, w):
    work.mkdir(parents=True, exist_ok=True)
    (work / "params").write_text(w.params_file_text())
    (work / "data").write_text(w.data_file_text())


def _libc_files(samples_bin, names):
    """what the text sink must write, formatted with libc from samples.bin"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import samples_bin as sb
    hdr, params, probs = sb.read(samples_bin)
    files = {}
    for c in range(hdr["n_param_chains"]):
        for p, name in enumerate(names):
            files["%s-chain-%d.prob.dump" % (name, c)] = _param_text(params[:, c, p])
    for c in range(hdr["n_beta"]):
        files["prob-chain%d.dump" % c] = _prob_text(probs[:, c])
    return files


def _run(exe, work, mode, extra_env=None, args=("run",), limit=None):
    env = dict(os.environ, APEMOST_SEED="3")
    env.pop("APEMOST_DUMP", None)
    if mode:
        env["APEMOST_DUMP"] = mode
    env.update(extra_env or {})
    subprocess.check_call([exe] + list(args), cwd=str(work), env=env, stdout=subprocess.DEVNULL, timeout=600,
                          preexec_fn=limit)


def _assert_text_equals_binary(text_dir, bin_dir, names, n_beta):
    files = _libc_files(str(bin_dir / "samples.bin"), names)
    assert "prob-chain%d.dump" % (n_beta - 1) in files
    for f, want in files.items():
        assert (text_dir / f).read_bytes() == want, f
    for f in ("acceptance_rate.dump", "calibration_results"):
        assert (text_dir / f).read_bytes() == (bin_dir / f).read_bytes(), f
    return files


def _calibrated(tmp_path, exe, w, name):
    base = tmp_path / name
    _inputs(base, w)
    for phase in ("calibrate_first", "calibrate_rest"):
        _run(exe, base, None, args=(phase,))
    return base


def test_c_host_text_sink_equals_libc_formatted_binary_sink(tmp_path):
    n_beta, iters = 8, 6000
    w = wl.simplesin(n_data=128, n_chain=n_beta)
    flags = "-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d" % (n_beta, iters)
    exe = hostlib.make(str(tmp_path / "sine.exe"), ccflags=flags)
    base = _calibrated(tmp_path, exe, w, "calib")
    runs = {}
    for mode in ("text", "binary", "thin:7", "binary,thin:7", "text,summary", "two_shards"):
        work = tmp_path / mode.replace(":", "_").replace(",", "_")
        shutil.copytree(str(base), str(work))
        if mode == "two_shards":
            _run(exe, work, None, {"APEMOST_DEVICES": "0,0"})
        else:
            _run(exe, work, None if mode == "text" else mode)
        runs[mode] = work
    files = _assert_text_equals_binary(runs["text"], runs["binary"], w.names, n_beta)
    assert len(files["prob-chain0.dump"].splitlines()) == iters
    _assert_text_equals_binary(runs["thin:7"], runs["binary,thin:7"], w.names, n_beta)
    for mode in ("text,summary", "two_shards"):
        for f in files:
            assert (runs[mode] / f).read_bytes() == files[f], (mode, f)
    assert (runs["text,summary"] / "summary.bin").exists()

    # analyse reads the same files, so it prints the same; and run --append appends the same lines
    for f, data in files.items():
        (runs["binary"] / f).write_bytes(data)
    outs = []
    for mode in ("text", "binary"):
        r = subprocess.run([exe, "analyse"], cwd=str(runs[mode]), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           universal_newlines=True, timeout=300, env={k: v for k, v in os.environ.items() if k != "APEMOST_DUMP"})
        assert r.returncode == 0, r.stderr
        outs.append(([l.split("\r")[-1] for l in r.stdout.splitlines() if "Model probability" in l or "mcmc error" in l],
                     [(runs[mode] / f).read_bytes() for f in [n + ".histogram" for n in w.names] +
                      ["marginal_distributions.gnuplot"]]))
    assert outs[0] == outs[1]
    for mode in ("text", "binary"):
        for f in files:                                 # (the binary run's copies are not part of its append)
            if mode == "binary":
                (runs[mode] / f).unlink()
        _run(exe, runs[mode], None if mode == "text" else mode, args=("run", "--append"))
    files2 = _assert_text_equals_binary(runs["text"], runs["binary"], w.names, n_beta)
    assert len(files2["prob-chain0.dump"].splitlines()) == 2 * iters


def test_c_host_text_sink_all_chains(tmp_path):
    """-DDUMP_ALL_CHAINS: every chain's parameter files, through the same device streams"""
    n_beta, iters = 6, 3000
    w = wl.simplesin(n_data=96, n_chain=n_beta)
    flags = "-DN_BETA=%d -DBURN_IN_ITERATIONS=600 -DMAX_ITERATIONS=%d -DDUMP_ALL_CHAINS" % (n_beta, iters)
    exe = hostlib.make(str(tmp_path / "sine_all.exe"), ccflags=flags)
    base = _calibrated(tmp_path, exe, w, "calib")
    runs = {}
    for mode in ("text", "binary"):
        work = tmp_path / mode
        shutil.copytree(str(base), str(work))
        _run(exe, work, None if mode == "text" else mode)
        runs[mode] = work
    files = _assert_text_equals_binary(runs["text"], runs["binary"], w.names, n_beta)
    assert "%s-chain-%d.prob.dump" % (w.names[0], n_beta - 1) in files


def test_c_host_text_sink_more_chains_than_file_descriptors(tmp_path):
    """1100 chains under RLIMIT_NOFILE = 1024: prob-chain files opened per batch, same bytes as libc"""
    n_beta, iters = 1100, 40
    w = wl.simplesin(n_data=64, n_chain=n_beta)
    exe = hostlib.make(str(tmp_path / "sine.exe"), ccflags="-DN_BETA=%d -DN_SWAP=2 -DMAX_ITERATIONS=%d" % (n_beta, iters))
    from apemost_amd.state import LadderState
    from apemost_amd.sampler import get_chain_beta
    st = LadderState.from_params(n_beta, w.start, w.pmin, w.pmax, w.step * 0.3)
    for i in range(n_beta):
        st.beta[i] = get_chain_beta(0, i, n_beta, 0.05)
    import resource
    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)

    def limit():
        resource.setrlimit(resource.RLIMIT_NOFILE, (min(1024, hard), hard))
    runs = {}
    for mode in ("text", "binary"):
        work = tmp_path / mode
        _inputs(work, w)
        (work / "calibration_results").write_text(st.calibration_results_text())
        _run(exe, work, None if mode == "text" else mode, limit=limit)
        runs[mode] = work
    _assert_text_equals_binary(runs["text"], runs["binary"], w.names, n_beta)
