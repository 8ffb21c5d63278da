"""Derived quantities without a device: the ABI declares and exports the entry points, apemost_hip_derived_check accepts
and refuses what the specification says, the host interpreter (apemost_amd/derived.py) equals directly written numpy
expressions and the restatement of tests/derived_ref.py bit for bit, the host fold equals the restatement, the joint
fold and the run summary on identity columns, the estimators hold against exact rational arithmetic, and derived.bin
round-trips; the C host's parser takes and refuses the lines parse_rpn does, and its files are the Python module's."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from apemost_amd import build, capi, derived as dv
from apemost_amd.joint import Joint
from apemost_amd.summary import RunSummary, batches_closed
from tests import derived_ref as ref, hostlib, summary_rows as sr
from tests.derived_ref import CHAINS, COLUMNS, EXTRA_BOXES, PAIRS, assert_equals_ref, special_rows
from tests.joint_ref import same_floats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "apemost_amd", "csrc")
ENTRIES = ["apemost_hip_derived_check", "apemost_hip_derived_begin", "apemost_hip_derived_accumulate",
           "apemost_hip_derived_get", "apemost_hip_derived_set", "apemost_hip_derived_end", "apemost_hip_derived_eval"]
NAMES = ["p0", "p1", "p2", "p3"]


def same_bits(a, b):
    """bit for bit where neither is a NaN, NaN exactly where the other is"""
    return same_floats(a, b)


# ---- ABI ----------------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points():
    build.build_hip()
    header = open(os.path.join(ROOT, "include", "apemost_hip.h")).read()
    L = capi.lib()
    for name in ENTRIES:
        assert re.search(r"\bint %s\(" % name, header), name
        assert name in capi.EXPORTS and getattr(L, name).argtypes, name
    assert "apemost_hip_derived_config;" in header and "apemost_hip_derived_view;" in header
    assert capi.ABI_VERSION == 3 and L.apemost_hip_abi_version() == 3
    for i, name in enumerate(dv.OPS):
        assert re.search(r"APEMOST_DERIVED_%s = %d\b" % (name.upper(), i), header), name
    assert ref.POPS_PUSHES.keys() == set(range(len(dv.OPS)))
    # the model translation units do not see the new header; the joint and summary kernels are called, not restated
    assert '#include "pt_derived.h"' in open(os.path.join(CSRC, "apemost_hip.hip")).read()
    for f in os.listdir(CSRC):
        if f != "apemost_hip.hip" and os.path.isfile(os.path.join(CSRC, f)):
            assert "pt_derived.h" not in open(os.path.join(CSRC, f)).read().replace("// pt_derived.h --", ""), f
    text = open(os.path.join(CSRC, "pt_derived.h")).read()
    assert "summary_edge(" in text and "summary_bin(" in text and '#include "pt_joint.h"' in text


# ---- apemost_hip_derived_check ------------------------------------------------------------------------------------------
def _native(programs, n_par=4):
    return dv.check_native([dv.Program(code, consts) for code, consts in programs], n_par)


def _refused(programs, part, n_par=4):
    with pytest.raises(capi.ApemostHipError) as e:
        _native(programs, n_par)
    assert e.value.code == capi.ERR_INVALID and "derived_check" in str(e.value) and part in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        dv.check([dv.Program(code, consts) for code, consts in programs], n_par)


def test_derived_check_table():
    build.build_hip()
    W = ref.word
    deep = [W(ref.COL, 0)] * 16 + [W(ref.ADD)] * 15
    long_ = [W(ref.COL, 1)] + [W(ref.NEG)] * 255
    assert _native([(deep, [])]) == [16] and _native([(long_, [])]) == [1]
    assert _native([([W(ref.COL, 5)], []), ([W(ref.CONST, 0), W(ref.DUP), W(ref.SWAP), W(ref.ATAN2)], [1.5])]) == [1, 2]
    assert dv.check([dv.Program(deep), dv.Program(long_)], 4) == [16, 1]
    _refused([([W(ref.COL, 0), W(ref.ADD)], [])], "underflow")
    _refused([([W(ref.SWAP)], [])], "underflow")
    _refused([([W(ref.DUP)], [])], "underflow")
    _refused([([W(ref.COL, 0)] * 17 + [W(ref.ADD)] * 16, [])], "depth 17")
    _refused([([W(ref.COL, 0), W(ref.COL, 1)], [])], "leaves 2 values")
    _refused([(deep, []), ([W(ref.COL, 0), W(ref.DUP)], [])], "column 1 leaves 2")
    _refused([([W(20)], [])], "unknown opcode 20")
    _refused([([W(255)], [])], "unknown opcode 255")
    _refused([([W(ref.COL, 6)], [])], "COL 6")
    _refused([([W(ref.COL, 3)], [])], "COL 3", n_par=1)
    _refused([([W(ref.CONST, 1)], [2.0])], "CONST 1")
    _refused([([W(ref.CONST, 0)], [])], "CONST 0")
    _refused([([], [])], "0 instructions")
    _refused([(long_ + [W(ref.NEG)], [])], "257 instructions")
    _refused([], "0 columns")
    _refused([([W(ref.COL, 0)], [])] * 65, "65 columns")
    assert _native([([W(ref.COL, 0)], [])] * 64) == [1] * 64
    # final depth 0 cannot be written (every instruction leaves at least one value), so an empty program stands for it;
    # a negative instruction word is an unknown opcode or an operand out of range, never accepted
    with pytest.raises(capi.ApemostHipError):
        _native([([-1], [])])


# ---- the host interpreter -------------------------------------------------------------------------------------------------
def _np_min(b, t):
    return np.where(b < t, b, t)


def _np_max(b, t):
    return np.where(b > t, b, t)


EXPRESSIONS = [
    ("p1 - p0", "p1 p0 sub", lambda r: r[:, 1] - r[:, 0]),
    ("p3 / p1", "p3 p1 div", lambda r: r[:, 3] / r[:, 1]),
    ("sqrt(abs(p0 * p3))", "p0 p3 mul abs sqrt", lambda r: np.sqrt(np.abs(r[:, 0] * r[:, 3]))),
    ("min(p0, p1)", "p0 p1 min", lambda r: _np_min(r[:, 0], r[:, 1])),
    ("max(p2, -p3) + 0.1", "p2 p3 neg max 0.1 add", lambda r: _np_max(r[:, 2], -r[:, 3]) + 0.1),
    ("like / 0.25", "like 0.25 div", lambda r: r[:, 5] / 0.25),
    ("floor(prob * 3) - inv(p2)", "prob 3.0 mul floor p2 inv sub", lambda r: np.floor(r[:, 4] * 3.0) - 1.0 / r[:, 2]),
    ("-(p0 + p1) * (p2 - 1e300) / 2", "p0 p1 add neg p2 1e300 sub mul 2.0 div",
     lambda r: -(r[:, 0] + r[:, 1]) * (r[:, 2] - 1e300) / 2.0),
    ("p0 * cos(2 * 3.141592653589793 * p1)", "p0 2.0 3.141592653589793 mul p1 mul cos mul",
     lambda r: r[:, 0] * np.cos(2.0 * 3.141592653589793 * r[:, 1])),
    ("atan2(p0, p1) + log(abs(p2)) + exp(p3) + sin(p0)", "p0 p1 atan2 p2 abs log add p3 exp add p0 sin add",
     lambda r: np.arctan2(r[:, 0], r[:, 1]) + np.log(np.abs(r[:, 2])) + np.exp(r[:, 3]) + np.sin(r[:, 0])),
]


def test_compile_and_parse_equal_the_written_expression():
    rows = special_rows()
    for expr, rpn, direct in EXPRESSIONS:
        a, b = dv.compile(expr, NAMES), dv.parse_rpn(rpn, NAMES)
        assert a == b, (a.rpn(NAMES), b.rpn(NAMES))
        with np.errstate(all="ignore"):
            want = direct(rows)
        for p in (a, b):
            got = dv.eval_numpy(p, rows)
            assert same_bits(got, want), (expr, np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))[:5])
        assert dv.parse_rpn(a.rpn(NAMES), NAMES) == a                 # the text form round-trips
        assert np.isfinite(want).any()


def test_stack_words():
    rows = special_rows()
    p = dv.parse_rpn("p0 dup mul p1 swap sub", NAMES)                  # p1 - p0 * p0
    with np.errstate(all="ignore"):
        assert same_bits(dv.eval_numpy(p, rows), rows[:, 1] - rows[:, 0] * rows[:, 0])
    assert p.uses_only_exact() and not dv.compile("sin(p0)", NAMES).uses_only_exact()
    two = dv.eval_numpy([p, dv.compile("p2", NAMES)], rows)
    assert two.shape == (len(rows), 2) and same_bits(two[:, 1], rows[:, 2])


@pytest.mark.parametrize("expr", ["q", "p0.real", "len(p0)", "p0 < p1", "p0 ** 2", "p0 if p1 else p2", "[p0]", "p0 % p1",
                                  "sqrt(p0, p1)", "min(p0)", "abs(x=p0)", "(lambda: p0)()", "True", "'a'", "1j", "+p0",
                                  "p0 +", "np.sin(p0)", "__import__('os')", "not p0", "p0 and p1"])
def test_compile_refuses(expr):
    with pytest.raises(ValueError):
        dv.compile(expr, NAMES)


@pytest.mark.parametrize("text", ["", "p0 p1", "add", "p0 q add", "p0 1.0.0 add", "col", "const", "p0 dup", "p0 p1 ADD"])
def test_parse_rpn_refuses(text):
    with pytest.raises(ValueError):
        dv.parse_rpn(text, NAMES)
    with pytest.raises(ValueError):
        dv.compile("p0", ["p0", "sin"])                                  # a reserved word as a parameter name


def test_pack_shares_constants_and_rebases_their_indices():
    a, b = dv.compile("p0 * 2 + 0.5", NAMES), dv.compile("0.5 - p1 / 2", NAMES)
    code, start, consts = dv.pack([a, b])
    assert start.tolist() == [0, len(a.code), len(a.code) + len(b.code)] and sorted(consts.tolist()) == [0.5, 2.0]
    rows = special_rows(64)
    rebuilt = [dv.Program(code[start[c]:start[c + 1]].tolist(), consts.tolist()) for c in range(2)]
    for p, q in zip((a, b), rebuilt):
        assert same_bits(dv.eval_numpy(p, rows), dv.eval_numpy(q, rows))
    z = dv.pack([dv.compile("p0 + 0.0", NAMES), dv.parse_rpn("p0 -0.0 add", NAMES)])[2]
    assert len(z) == 2                                                   # 0.0 and -0.0 are two constants


# ---- the host fold --------------------------------------------------------------------------------------------------------
def test_eval_numpy_equals_the_restatement_on_generated_programs():
    rows = special_rows(96, seed=5)
    progs = ref.random_programs(17, 200, 4)
    assert ref.depth_of(progs[0][0]) == 16 and len(progs[1][0]) == 256
    want = ref.values(progs, rows)
    programs = [dv.Program(code, consts) for code, consts in progs]
    assert dv.check(programs[:64], 4) == [ref.depth_of(code) for code, _ in progs[:64]]
    assert dv.check_native(programs[:64], 4) == dv.check(programs[:64], 4)
    got = dv.eval_numpy(programs, rows)
    for c in range(len(progs)):
        assert same_bits(got[:, c], want[:, c]), (c, programs[c].rpn(NAMES))
    finite = np.isfinite(want)
    assert 0.2 < finite.mean() and (~finite).any()


@pytest.mark.parametrize("box_set", ["A", "B"])
def test_from_rows_equals_the_restatement(box_set):
    nbins, bs = 37, 50
    rows, boxes = sr.build_rows(box_set, nbins)
    kept = rows[sr.kept_steps()]
    boxes = list(boxes) + EXTRA_BOXES[box_set]
    programs = [dv.compile(e, NAMES) for e in COLUMNS]
    got = dv.Derived.from_rows(kept, programs, [b[0] for b in boxes], [b[1] for b in boxes], chains=CHAINS, nbins=nbins,
                               pairs=PAIRS, batch_size=bs)
    vals = np.zeros((len(kept), 300, len(COLUMNS)))
    for ch in CHAINS:
        vals[:, ch] = ref.values([(p.code, p.consts) for p in programs], kept[:, ch])
    want = ref.RefDerived(vals, boxes, CHAINS, nbins, bs, PAIRS)
    assert_equals_ref(got, want, finite_chains=(), what=box_set)
    assert np.array_equal(got.nonfinite, (~np.isfinite(vals[:, CHAINS])).sum(axis=0))
    assert int(got.nonfinite.sum()) > 0 and int(got.hist.sum()) > 0
    # the identity columns are the joint fold's and the run summary's
    jt = Joint.from_rows(kept, [b[0] for b in boxes[:4]], [b[1] for b in boxes[:4]], chains=CHAINS, nbins=nbins,
                         pairs=[(0, 1), (2, 3)])
    assert np.array_equal(jt.counts, got.counts[:, :2])
    assert same_bits(jt.origin, got.origin[:, :4]) and same_bits(jt.sum, got.sum[:, :4])
    for i in range(4):
        for j in range(i, 4):
            from apemost_amd.joint import tri_index
            assert same_bits(jt.cross[:, tri_index(4, i, j)], got.cross[:, tri_index(8, i, j)]), (i, j)
    rs = RunSummary.from_rows(kept, 3, nbins, bs, batches_closed(len(kept), bs), [b[0] for b in boxes[:4]],
                              [b[1] for b in boxes[:4]])
    assert np.array_equal(rs.hist, got.hist[:3, :4]) and same_bits(rs.batch_sums, got.batch[:3, :4])
    n, _, hist, batch = sr.expected(rows, boxes[:4], nbins, bs, 3)
    assert n == int(got.n[0]) and np.array_equal(hist, got.hist[:3, :4])
    for (h, p), (closed, part) in batch.items():
        assert same_bits(got.batch[h, p, :len(closed)], np.array(closed)) and same_bits(got.batch[h, p, len(closed)], part)


# ---- estimators -----------------------------------------------------------------------------------------------------------
def test_mean_and_covariance_against_rational_arithmetic():
    """the columns f2 - f1 (narrow: both near 5 with a common part) and h2 / h1: mean and covariance from the sums about
    the first sample against exact rational arithmetic on the computed values, within the bound of recursive
    summation that tests/test_joint_cpu.py uses: 4 gamma_n (sum |d_i d_j| + sum |d_i| sum |d_j| / n) / (n - 1)"""
    n = 5000
    rng = np.random.default_rng(23)
    rows = np.zeros((n, 1, 6))
    common = rng.normal(5.0, 0.3, n)
    rows[:, 0, 0], rows[:, 0, 1] = common, common + 1e-4 * (1 + rng.standard_normal(n))
    rows[:, 0, 2], rows[:, 0, 3] = rng.uniform(1, 2, n), rng.uniform(1, 2, n)
    programs = [dv.compile("p1 - p0", NAMES), dv.compile("p3 / p2", NAMES)]
    d = dv.Derived.from_rows(rows, programs, [-1e-3, 0.0], [1e-3, 3.0], nbins=50, batch_size=70)
    vals = dv.eval_numpy(programs, rows[:, 0])
    cols = [[Fraction(v) for v in vals[:, c].tolist()] for c in range(2)]
    totals = [sum(c) for c in cols]
    gamma = n * 2.0 ** -53 / (1 - n * 2.0 ** -53)
    dd = [np.abs(vals[:, c] - vals[0, c]) for c in range(2)]
    mean, cov = d.mean(0), d.cov(0)
    for i in range(2):
        assert abs(Fraction(float(mean[i])) - totals[i] / n) <= 4 * gamma * float(dd[i].sum()) / n + 2.0 ** -52 * abs(float(mean[i]))
        for j in range(2):
            exact = (sum(x * y for x, y in zip(cols[i], cols[j])) - totals[i] * totals[j] / n) / (n - 1)
            bound = 4 * gamma * (float((dd[i] * dd[j]).sum()) + float(dd[i].sum()) * float(dd[j].sum()) / n) / (n - 1)
            assert abs(Fraction(float(cov[i, j])) - exact) <= bound, (i, j)
    assert d.sd(0)[0] == np.sqrt(cov[0, 0]) and d.corr(0)[0, 0] == 1.0
    # quantiles from the histogram: within a bin's width of the sample quantile; min and max are the sample's
    for c in range(2):
        width = (d.hi[c] - d.lo[c]) / d.nbins
        for q in (0.1, 0.5, 0.9):
            assert abs(d.quantile(q, c) - np.quantile(vals[:, c], q)) <= width, (c, q)
        assert d.min(0)[c] == vals[:, c].min() and d.max(0)[c] == vals[:, c].max()
        e, dens = d.marginal(c)
        assert abs(float((dens * width).sum()) - 1.0) < 1e-12 and len(e) == d.nbins + 1
    # the batch-means error as RunSummary computes it from the same batch sums about the same mean
    rs = RunSummary(n, np.zeros(1), d.hist, d.batch, d.n_batches, d.lo, d.hi, 70)
    for c in range(2):
        assert d.mcse(0)[c] == rs.batch_means_error(c, 0, mean=float(mean[c]))
    lines = d.text().splitlines()
    assert len(lines) == 2 and lines[0].split("\t")[0] == "d0" and int(lines[0].split("\t")[1]) == n
    assert float(lines[1].split("\t")[2]) == pytest.approx(float(mean[1]), rel=1e-14) and lines[0].split("\t")[7] == "0"


# ---- files --------------------------------------------------------------------------------------------------------------
def test_derived_bin_round_trip(tmp_path):
    rows, boxes = sr.build_rows("A", 8, n_chains=6)
    kept = rows[:200]
    boxes = list(boxes) + EXTRA_BOXES["A"]
    names = ["freq", "amp", "phase", "off"]
    programs = [dv.compile(e.replace("p0", "freq").replace("p1", "amp").replace("p2", "phase").replace("p3", "off"), names)
                for e in COLUMNS]
    d = dv.Derived.from_rows(kept, programs, [b[0] for b in boxes], [b[1] for b in boxes], chains=(0, 4), nbins=8,
                             pairs=PAIRS, batch_size=9, names=["c%d" % c for c in range(8)], row_names=names, thin=3)
    path = str(tmp_path / "derived.bin")
    d.write(path)
    e = dv.Derived.read(path)
    assert int(e.n[0]) == 200 and e.thin == 3 and e.batch_size == 9 and e.names == d.names and e.row_names == names
    assert e.programs == d.programs and [p.rpn(names) for p in e.programs] == [p.rpn(names) for p in programs]
    assert e.chains.tolist() == [0, 4] and e.pairs.tolist() == [list(p) for p in PAIRS]
    for f in ("hist", "batch", "nonfinite", "vmin", "vmax", "origin", "sum", "cross", "counts", "lo", "hi"):
        assert np.asarray(getattr(e, f)).tobytes() == np.asarray(getattr(d, f)).tobytes(), f
    raw = open(path, "rb").read()
    assert raw[:8] == b"APEMOSTD" and b"amp freq sub" in raw
    open(path, "wb").write(raw + b"\0")
    with pytest.raises(ValueError):
        dv.Derived.read(path)
    with pytest.raises(ValueError):
        dv.Derived.empty(programs, [0.0] * 8, [1.0] * 8).write(path)      # no names to write the programs with


# ---- the C host's parser and files, without a device -------------------------------------------------------------------------
class RunDerived(C.Structure):
    """run_derived of apemost_amd/host/include/run_derived.h"""
    _fields_ = ([(f, C.c_uint32) for f in ("n_par", "n_col", "nbins", "n_pairs", "n_const")] +
                [(f, C.c_uint64) for f in ("n", "thin", "bs", "max_batches")] +
                [(f, C.POINTER(C.c_char_p)) for f in ("names", "rpn", "row_names")] +
                [("code", C.POINTER(C.c_int32)), ("start", C.POINTER(C.c_int32))] +
                [(f, C.POINTER(C.c_double)) for f in ("consts", "lo", "hi")] + [("pairs", C.POINTER(C.c_int32))] +
                [(f, C.c_void_p) for f in ("hist", "batch", "nonfinite", "vmin", "vmax", "origin", "sum", "cross", "counts")])


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    build.build_hip()
    lib = hostlib.make(str(tmp_path_factory.mktemp("derived_host") / "libhost.so"), ccflags="-DN_BETA=4", shared=True)
    L = C.CDLL(lib)
    L.run_derived_parse.argtypes = [C.c_char_p, C.c_uint, C.POINTER(C.c_char_p), C.POINTER(RunDerived), C.c_char_p]
    L.run_derived_free.argtypes = [C.POINTER(RunDerived)]
    L.run_derived_read.argtypes = [C.c_char_p, C.POINTER(RunDerived)]
    L.run_derived_write.argtypes = [C.c_char_p, C.POINTER(RunDerived)]
    L.run_derived_write_text.argtypes = [C.POINTER(RunDerived)]
    return L


def c_parse(L, text, names=("freq", "amp", "phase", "off")):
    r, msg = RunDerived(), C.create_string_buffer(400)
    arr = (C.c_char_p * len(names))(*[n.encode() for n in names])
    rc = L.run_derived_parse(text.encode(), len(names), arr, C.byref(r), msg)
    out = None
    if rc == 0:
        out = dict(names=[r.names[c].decode() for c in range(r.n_col)], rpn=[r.rpn[c].decode() for c in range(r.n_col)],
                   lo=[r.lo[c] for c in range(r.n_col)], hi=[r.hi[c] for c in range(r.n_col)],
                   start=[r.start[c] for c in range(r.n_col + 1)], consts=[r.consts[k] for k in range(r.n_const)])
        out["code"] = [r.code[i] for i in range(out["start"][-1])]
    L.run_derived_free(C.byref(r))
    return rc, msg.value.decode(), out


RPN_LINES = ["amp freq sub", "off amp div", "freq off mul abs sqrt", "freq amp min", "like 0.25 div", "prob 3 mul floor phase inv sub",
             "amp 2 3.141592653589793 mul phase mul cos mul", "freq amp atan2 phase abs log add off exp add", "freq dup mul amp swap sub",
             "1e300 -0.0 max neg", "freq 5e-324 add", ".5 freq sub", "freq 1e5 mul", "inf freq min", "nan freq add",
             # refused by both
             "", "freq amp", "add", "freq q add", "freq 1.0.0 add", "col", "const", "freq dup", "freq amp ADD", "freq 0x10 add",
             "freq amp sub sub", "freq 1e add", "freq " * 17 + "add " * 16]


def test_c_parser_accepts_and_refuses_what_parse_rpn_does(host):
    names = ["freq", "amp", "phase", "off"]
    accepted = []
    for i, rpn in enumerate(RPN_LINES):
        try:
            p = dv.parse_rpn(rpn, names)
        except ValueError:
            p = None
        rc, msg, out = c_parse(host, "# a comment\n\nq%d -1.5 2e3 %s # trailing\n" % (i, rpn))
        assert (rc == 0) == (p is not None), (rpn, rc, msg)
        if p is None:
            assert rc in (3, -1) and (msg.startswith("line 3: ") or not rpn), (rpn, rc, msg)
            continue
        assert out["names"] == ["q%d" % i] and out["lo"] == [-1.5] and out["hi"] == [2000.0]
        assert dv.Program(out["code"], out["consts"]) == p and dv.parse_rpn(out["rpn"][0], names) == p, rpn
        accepted.append(rpn)
    assert len(accepted) == 15
    # a whole file: the programs of pack(), constants shared; and the lines a file may not hold
    text = "".join("c%d 0 1 %s\n" % (i, rpn) for i, rpn in enumerate(accepted))
    rc, msg, out = c_parse(host, text)
    assert rc == 0, msg
    code, start, consts = dv.pack([dv.parse_rpn(rpn, names) for rpn in accepted])
    assert out["start"] == start.tolist() and len(out["consts"]) == len(consts)
    assert [dv.Program(out["code"][a:b], out["consts"]) for a, b in zip(out["start"], out["start"][1:])] == \
        [dv.parse_rpn(rpn, names) for rpn in accepted]
    for bad, line in (("a 0 1 freq\nb 1 1 freq\n", 2), ("a 0 1 freq\n\nb 0 x freq\n", 3), ("a 0 1\n", 1), ("a 0 1 freq\na 0 2 amp\n", 2),
                      ("a/b 0 1 freq\n", 1), ("a 0 inf freq\n", 1), ("a -1e308 1e308 freq\n", 1), ("a nan 1 freq\n", 1),
                      ("a 0 1 freq amp\n", 1), ("ok 0 1 freq\n" * 1 + "".join("c%d 0 1 freq\n" % i for i in range(64)), 65)):
        rc, msg, _ = c_parse(host, bad)
        assert rc == line and msg.startswith("line %d: " % line), (bad[:40], rc, msg)
    assert c_parse(host, "# nothing\n\n")[0] == -1
    assert c_parse(host, "".join("c%d 0 1 freq\n" % i for i in range(64)))[0] == 0


def test_c_host_reads_and_writes_the_same_files(host, tmp_path, monkeypatch):
    """derived.bin of the Python writer through the C reader and writer: the same bytes; derived.txt of the C writer:
    apemost_amd/derived.py's text; <name>.histogram: lines `lower upper value` on the summary's edges, the values scaled
    as analyse scales a parameter's histogram"""
    rows, boxes = sr.build_rows("A", 8, n_chains=6)
    kept = rows[:300, 1:2]                                                # a chain of finite rows
    names = ["freq", "amp", "phase", "off"]
    programs = [dv.parse_rpn(t, names) for t in ("freq", "amp freq sub", "off 2.5 div", "freq off mul abs sqrt")]
    lo, hi = [0.1, -40.0, -4.0, 0.0], [50.0, 12.0, 0.0, 20.0]
    d = dv.Derived.from_rows(kept, programs, lo, hi, nbins=8, batch_size=17, max_batches=40, names=["f", "split", "o", "g"],
                             row_names=names, thin=2)
    monkeypatch.chdir(tmp_path)
    d.write("derived.bin")
    r = RunDerived()
    assert host.run_derived_read(b"derived.bin", C.byref(r)) == 0 and host.run_derived_read(b"none.bin", C.byref(RunDerived())) == -1
    assert (r.n_col, r.nbins, r.n, r.thin, r.bs, r.max_batches) == (4, 8, 300, 2, 17, 40)
    host.run_derived_write(b"again.bin", C.byref(r))
    host.run_derived_write_text(C.byref(r))
    host.run_derived_free(C.byref(r))
    assert (tmp_path / "again.bin").read_bytes() == (tmp_path / "derived.bin").read_bytes()
    assert (tmp_path / "derived.txt").read_text() == d.text()
    for c, name in enumerate(d.names):
        table = np.loadtxt(str(tmp_path / (name + ".histogram")))
        e, dens = d.marginal(c)
        assert table.shape == (8, 3) and table[:, 0].tolist() == [float("%.15e" % v) for v in e[:-1]]
        assert table[:, 1].tolist() == [float("%.15e" % v) for v in e[1:]]
        scaled = RunSummary(300, np.zeros(1), d.hist, d.batch, d.n_batches, d.lo, d.hi, 17).histogram_density(c)[1]
        assert table[:, 2].tolist() == [float("%.15e" % v) for v in scaled]     # counts * width / total, as analyse scales
        np.testing.assert_allclose(table[:, 2] / ((d.hi[c] - d.lo[c]) / 8) ** 2, dens, rtol=1e-14)
