"""The C host's run phase over its table of folds (apemost_amd/host/src/run_fold.c): all eight APEMOST_DUMP fold tokens
at once write what each writes alone, the refusals of an unbounded run come in the table's order whatever the list's,
and the two folds with a per-shard loop write the same bytes on two shards as on one.  Only the executable and its
environment are used."""
import os
import shutil
import subprocess

import pytest

from apemost_amd import workloads as wl
from tests import hostlib

pytestmark = pytest.mark.gpu

TOKENS = ["summary", "peaks", "joint", "derived", "evidence", "autocorr", "predict", "pointwise"]
INPUTS = {"params", "data", "derived", "calibration_results"}
BOUNDED = "APEMOST_DUMP=%s needs a bounded run (MAX_ITERATIONS > 0): %s\n"
BATCH_SIZE_WHY = "the batch size of the error estimate is fixed before the first sample"


class Host:
    pass


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    """the sine example of 4 chains, bounded and unbounded, and a calibrated directory to copy per run"""
    top = tmp_path_factory.mktemp("host_run_folds")
    h = Host()
    h.top = top
    flags = "-DN_BETA=4 -DBURN_IN_ITERATIONS=200 -DMAX_ITERATIONS=%d"
    h.exe = hostlib.make(str(top / "sine.exe"), ccflags=flags % 600)
    h.unbounded = hostlib.make(str(top / "sine_unbounded.exe"), ccflags=flags % 0)
    w = wl.simplesin(n_data=32, n_chain=4)
    h.template = top / "template"
    h.template.mkdir()
    (h.template / "params").write_text(w.params_file_text())
    (h.template / "data").write_text(w.data_file_text())
    a, b = w.names[1], w.names[0]
    (h.template / "derived").write_text("split -100 100 %s %s sub\nloglike -1e6 0 like 1 div   # (prob - prior) / beta\n" % (a, b))
    h.env = dict(os.environ, APEMOST_SEED="3")
    for phase in ("calibrate_first", "calibrate_rest"):
        subprocess.check_call([h.exe, phase], cwd=str(h.template), env=h.env, stdout=subprocess.DEVNULL, timeout=120)
    h.runs = {}
    return h


def run(h, name, dump, exe=None, **env):
    """one run phase in a fresh copy of the template: (directory, completed process)"""
    work = h.top / name
    shutil.copytree(str(h.template), str(work))
    r = subprocess.run([exe or h.exe, "run"], cwd=str(work), env=dict(h.env, APEMOST_DUMP=dump, **env),
                       stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, timeout=120)
    return work, r


def written(h, name, dump):
    """the files a run of its own wrote for `dump` (each run is made once)"""
    if name not in h.runs:
        work, r = run(h, name, dump)
        assert r.returncode == 0, r.stderr
        h.runs[name] = {f: (work / f).read_bytes() for f in os.listdir(str(work))}
    return h.runs[name]


def no_sample_files(files):
    return not [f for f in files if f == "samples.bin" or f.endswith(".prob.dump") or f.startswith("prob-chain")]


def fold_files(files):
    """what a fold can have written: not the inputs, not the run's own acceptance and calibration logs"""
    return {f for f in files if f not in INPUTS and not f.startswith(("acceptance_rate", "calibration"))}


@pytest.mark.parametrize("token", TOKENS)
def test_all_tokens_at_once_equal_each_alone(host, token):
    every = written(host, "all", ",".join(TOKENS))
    alone = written(host, token, token)
    assert no_sample_files(every) and no_sample_files(alone)
    for f in sorted(alone):
        assert f in every and alone[f] == every[f], f
    others = set()
    for t in TOKENS:
        if t != token:
            others |= fold_files(written(host, t, t))
    own = fold_files(alone) - others
    print(token, sorted(own))
    assert own, (token, sorted(alone))


def test_refusals_of_an_unbounded_run_come_in_the_table_order(host):
    """summary opens first whatever the list's order, and evidence before predict.  (That joint,autocorr runs unbounded is
    not tested: no host test stops an unbounded run.)"""
    _, r = run(host, "unbounded_summary", "pointwise,peaks,summary", exe=host.unbounded)
    assert r.returncode == 1 and r.stderr.decode() == BOUNDED % ("summary", BATCH_SIZE_WHY), r.stderr
    _, r = run(host, "unbounded_evidence", "predict,evidence", exe=host.unbounded)
    assert r.returncode == 1 and r.stderr.decode() == BOUNDED % ("evidence", BATCH_SIZE_WHY), r.stderr


def test_two_shards_write_the_bytes_of_one(host):
    one = written(host, "one_shard", "summary,evidence")
    work, r = run(host, "two_shards", "summary,evidence", APEMOST_DEVICES="0,0")
    assert r.returncode == 0, r.stderr
    for f in ("summary.bin", "evidence.bin"):
        assert (work / f).read_bytes() == one[f], f
