"""On-device peaks, the parts that need no device.  tests/peaks_ref.py, a numpy restatement of the reference's
peaks.exe (tools/peaks.c), reproduces recorded runs of the compiled tool byte for byte (tests/golden/peaks/<case>:
in.txt, args.txt = min max, out.txt = the tool's stdout); apemost_hip_peaks_table, the library's host function,
equals the restatement on those cases and on 200 random columns; the host/device helpers of pt_peaks.h, built by
the host compiler, order keys as numbers, round-trip and count indices as integer arithmetic does; and the header
declares what the library exports."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from apemost_amd import build, capi
from apemost_amd.peaks import Peaks
from tests.peaks_ref import PEAKS_MAX, RefPeaks

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "apemost_amd", "csrc")
CASES = ["equal_shares", "exact_gap", "modes_and_singles", "ninety_nine_peaks", "range_ends", "three_values"]
ENTRIES = ["apemost_hip_peaks_begin", "apemost_hip_peaks_accumulate", "apemost_hip_peaks_get", "apemost_hip_peaks_end",
           "apemost_hip_peaks_table"]


def fixture(golden_dir, case):
    d = os.path.join(golden_dir, "peaks", case)
    lo, hi = (float(x) for x in open(os.path.join(d, "args.txt")).read().split())
    values = np.array([float(x) for x in open(os.path.join(d, "in.txt")).read().split()])
    return values, lo, hi, open(os.path.join(d, "out.txt")).read()


def view_of(refs, n_par=1):
    """the view a device would hand out for these columns (one kept chain per n_par of them), built in numpy"""
    k = len(refs) // n_par
    return Peaks(0, np.array([r.n_values for r in refs]).reshape(k, n_par),
                 np.array([r.n_peaks for r in refs]).reshape(k, n_par),
                 np.array([r.left for r in refs]).reshape(k, n_par, PEAKS_MAX),
                 np.array([r.right for r in refs]).reshape(k, n_par, PEAKS_MAX),
                 np.array([r.q for r in refs]).reshape(k, n_par, PEAKS_MAX, 3),
                 np.array([r.q_set for r in refs]).reshape(k, n_par, PEAKS_MAX))


@pytest.mark.parametrize("case", CASES)
def test_restatement_reproduces_the_recorded_tool(case, golden_dir):
    values, lo, hi, want = fixture(golden_dir, case)
    assert RefPeaks(values, lo, hi).text == want


def test_fixtures_show_what_they_are_for(golden_dir):
    lines = {c: fixture(golden_dir, c)[3].splitlines()[1:] for c in CASES}
    assert lines["three_values"] == ["5.000000\t5.000000\t0.000000\t0.666667", "0.000000\t0.000000\t0.000000\t0.333333"]
    assert len(lines["ninety_nine_peaks"]) == 99
    # a one-sample peak behind a large one prints the large one's median
    big = lines["modes_and_singles"][0].split("\t")[:3]
    assert sum(l.split("\t")[:3] == big for l in lines["modes_and_singles"][2:]) >= 1
    # shares 0.3, 0.3, 0.4 by position: the selection sort leaves the equal ones in reverse order of position
    med = [float(l.split("\t")[0]) for l in lines["equal_shares"]]
    assert [l.split("\t")[3] for l in lines["equal_shares"]] == ["0.400000", "0.300000", "0.300000"] and med[1] > med[2]
    # 10 and 11 stay together, 11 and 12.000000000000002 split
    r = RefPeaks(*fixture(golden_dir, "exact_gap")[:3])
    s = r.sorted.tolist()
    assert 10.0 in s and 11.0 in s and 12.000000000000002 in s
    assert s.index(11.0) not in r.left[:r.n_peaks].tolist() and s.index(12.000000000000002) in r.left[:r.n_peaks].tolist()
    values, lo, hi, _ = fixture(golden_dir, "range_ends")
    r = RefPeaks(values, lo, hi)
    assert r.sorted[0] == lo and r.sorted[-1] == hi and np.nextafter(hi, np.inf) in values and r.n_values < len(values)


def random_column(rng):
    """clusters and singles on a 1e-4 grid over a random box, some values outside it, some NaN"""
    lo = float(rng.uniform(-50, 50))
    hi = lo + float(10 ** rng.uniform(-2, 3))
    parts = []
    for _ in range(rng.randint(0, 12)):
        centre = rng.uniform(lo - 0.1 * (hi - lo), hi + 0.1 * (hi - lo))
        parts.append(centre + rng.normal(0, (hi - lo) * 10 ** rng.uniform(-4, -1.5), rng.randint(1, 60)))
    if rng.randint(0, 4) == 0:
        parts.append(rng.uniform(lo, hi, rng.randint(1, 200)))
    v = np.round(np.concatenate(parts + [np.zeros(0)]) * 1e4) / 1e4
    if len(v) and rng.randint(0, 3) == 0:
        v[rng.randint(0, len(v))] = np.nan
    if rng.randint(0, 3) == 0:
        v = np.concatenate([v, [lo, hi, lo - 1.0, np.inf]])
    rng.shuffle(v)
    return v, lo, hi


def test_peaks_table_equals_the_restatement(golden_dir):
    build.build_hip()
    rng = np.random.RandomState(99)
    refs = [RefPeaks(*fixture(golden_dir, c)[:3]) for c in CASES]
    refs += [RefPeaks(*random_column(rng)) for _ in range(200)]
    refs = [r for r in refs if r.n_peaks <= PEAKS_MAX]
    assert len(refs) >= 200 and any(r.n_values == 0 for r in refs) and max(r.n_peaks for r in refs) == PEAKS_MAX
    n_par = 2
    refs = refs[:len(refs) // n_par * n_par]
    pk = view_of(refs, n_par)
    for i, r in enumerate(refs):
        got = pk.table(i % n_par, i // n_par)
        assert got.shape == r.table.shape and got.tobytes() == r.table.tobytes(), (i, got, r.table)
        assert pk.text(i % n_par, i // n_par) == r.text


def test_peaks_table_refuses_a_column_with_100_peaks():
    build.build_hip()
    r = RefPeaks(np.arange(100) * 10.1, 0.0, 1000.0)
    assert r.n_peaks == 100
    with pytest.raises(capi.ApemostHipError) as e:
        view_of([r]).table(0)
    assert e.value.code == capi.ERR_INVALID
    out, rows = np.zeros((PEAKS_MAX, 4)), C.c_uint32(0)
    assert capi.lib().apemost_hip_peaks_table(None, 1, 0, 0, out.ctypes.data_as(capi._dp), C.byref(rows)) == capi.ERR_INVALID


def test_helpers_built_by_the_host_compiler(tmp_path):
    exe = str(tmp_path / "peaks_check")
    subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-ffp-contract=off", "-I" + CSRC,
                           os.path.join(HERE, "peaks_check.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, universal_newlines=True, timeout=300, check=True).stdout
    sets, counts = {}, {}
    for line in out.splitlines():
        f = line.split()
        if f[0] == "count":
            counts[int(f[1])] = tuple(int(x) for x in f[2:])
        else:
            sets[f[0]] = (int(f[1]), int(f[2]))
    for name in ("round_trip", "excluded_key", "sorted_by_key", "pair_order", "filter_and_gap"):
        assert name in sets and sets[name][1] == 0, (name, sets)
    assert sets["round_trip"][0] >= 10 ** 6 and sets["sorted_by_key"][0] >= 990000, sets
    assert sorted(counts) == list(range(1, 10001))
    for n, c in counts.items():
        assert c == (n // 4, n * 2 // 4, n * 3 // 4), (n, c)


def test_header_declares_and_library_exports_the_entry_points():
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTS and getattr(L, name) is not None
    assert "apemost_hip_peaks_config;" in header and "apemost_hip_peaks_view;" in header
    assert capi.ABI_VERSION == 3 and L.apemost_hip_abi_version() == 3
    # the model translation units do not see the peaks header
    assert '#include "pt_peaks.h"' in open(os.path.join(CSRC, "apemost_hip.hip")).read()
    for f in os.listdir(CSRC):
        if f != "apemost_hip.hip" and os.path.isfile(os.path.join(CSRC, f)):
            assert "pt_peaks.h" not in open(os.path.join(CSRC, f)).read().replace("// pt_peaks.h --", ""), f
