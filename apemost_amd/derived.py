"""Derived quantities: the posterior of functions of the parameters, from what apemost_hip_derived_get hands out.

A derived column is a small stack program over one sample row x[0 .. n_par+1] (x[n_par]: prob, x[n_par+1]: prob -
prior); include/apemost_hip.h has the specification and the opcode numbers.  This module builds programs -- from an
infix expression (`compile`) or from the text form used in files (`parse_rpn`, `Program.rpn`) -- interprets them
on the host (`eval_numpy`, one numpy call per opcode: bitwise what the device computes for the exact group), and holds
one view of the fold in a `Derived`: per kept chain and column the run summary's histogram and batch sums, the count
of non-finite values with the least and the greatest value, and a `Joint` over the columns for mean, covariance,
correlation and pair densities.

The text form: tokens separated by blanks, read left to right.  A parameter name, `prob` or `like` (column n_par+1)
pushes that column, a number pushes a constant, and the opcode names in lower case act on the stack: dup swap add sub
mul div neg abs inv sqrt floor min max log exp sin cos atan2.  `f2 f1 sub` is f2 - f1; `y x atan2` is atan2(y, x).

derived.bin (little-endian), version 1:
    char[8]  "APEMOSTD"
    uint32   version, n_keep, n_col, nbins, n_pairs, n_par
    uint64   n, thin, batch_size, max_batches, n_batches
    int32    chains[n_keep]
    int32    pairs[n_pairs][2]
    double   lo[n_col], hi[n_col]
    per column: uint32 len_name, char name[len_name], uint32 len_rpn, char rpn[len_rpn]      (utf-8, not terminated)
    uint32   n_row_names; per name: uint32 len, char[len]            (the names the RPN text refers to; may be 0)
    uint64   hist[n_keep][n_col][nbins]
    double   batch[n_keep][n_col][max_batches + 1]                   (slot n_batches: the open batch)
    uint64   nonfinite[n_keep][n_col]
    double   vmin[n_keep][n_col], vmax[n_keep][n_col]
    double   origin[n_keep][n_col], sum[n_keep][n_col]
    double   cross[n_keep][n_col (n_col + 1) / 2]                    (upper triangle, row by row)
    uint64   counts[n_keep][n_pairs][nbins][nbins]
"""
import ast
import math
import struct

import numpy as np

from . import capi
from .joint import Joint, all_pairs, bins_of
from .summary import batches_closed, edges as summary_edges

MAGIC = b"APEMOSTD"
VERSION = 1
_HEAD = struct.Struct("<8s6I5Q")

# the opcode numbers of include/apemost_hip.h
OPS = ("col", "const", "dup", "swap", "add", "sub", "mul", "div", "neg", "abs", "inv", "sqrt", "floor", "min", "max",
       "log", "exp", "sin", "cos", "atan2")
OP = {name: i for i, name in enumerate(OPS)}
EXACT = frozenset(OPS[:15])            # ... whose results are correctly rounded: bitwise numpy's
MAX_COLUMNS, MAX_CODE, MAX_CONSTS, MAX_DEPTH = 64, 256, 256, 16
_UNARY = ("neg", "abs", "inv", "sqrt", "floor", "log", "exp", "sin", "cos")
_BINARY = ("add", "sub", "mul", "div", "min", "max", "atan2")
_ARITY = dict([(f, 1) for f in _UNARY] + [(f, 2) for f in _BINARY])
_BINOP = {ast.Add: "add", ast.Sub: "sub", ast.Mult: "mul", ast.Div: "div"}


def ins(op, operand=0):
    """one instruction word: the opcode in the low 8 bits, the operand in the high 24"""
    return OP[op] | (int(operand) << 8)


def _bits(v):
    return struct.pack("<d", v)


class Program:
    """one column's program: `code` (instruction words, CONST operands index `consts`) and `consts`"""

    def __init__(self, code, consts=()):
        self.code = [int(c) for c in code]
        self.consts = [float(c) for c in consts]

    def _const(self, v):
        v = float(v)
        for k, have in enumerate(self.consts):
            if _bits(have) == _bits(v):
                return k
        self.consts.append(v)
        return len(self.consts) - 1

    def push_col(self, c):
        self.code.append(ins("col", c))

    def push_const(self, v):
        self.code.append(ins("const", self._const(v)))

    def op(self, name):
        self.code.append(ins(name))

    def uses_only_exact(self):
        return all(OPS[c & 255] in EXACT for c in self.code)

    def rpn(self, names):
        """the text form; parse_rpn(p.rpn(names), names) is this program again"""
        cols = list(names) + ["prob", "like"]
        out = []
        for c in self.code:
            op, arg = OPS[c & 255], c >> 8
            out.append(cols[arg] if op == "col" else repr(self.consts[arg]) if op == "const" else op)
        return " ".join(out)

    def __eq__(self, other):
        return (isinstance(other, Program) and self.rpn_words() == other.rpn_words())

    def rpn_words(self):
        return [(c & 255, _bits(self.consts[c >> 8]) if c & 255 == OP["const"] else c >> 8) for c in self.code]


def _columns(names):
    names = list(names)
    cols = {name: i for i, name in enumerate(names)}
    for reserved in OPS + ("prob", "like"):
        if reserved in cols:
            raise ValueError("parameter name %r is a reserved word" % reserved)
    cols["prob"], cols["like"] = len(names), len(names) + 1
    return cols


def parse_rpn(text, names):
    """the program of the text form over the parameter names `names`"""
    cols = _columns(names)
    p = Program([])
    for tok in text.split():
        if tok in cols:
            p.push_col(cols[tok])
        elif tok in OP and tok not in ("col", "const"):
            p.op(tok)
        else:
            try:
                p.push_const(float(tok))
            except ValueError:
                raise ValueError("token %r is neither a column, a number nor an operation" % tok) from None
    check([p], len(names))
    return p


def compile(expr, names):     # noqa: A001 (the name the module's users expect)
    """the program of an infix expression: parameter names, prob, like, numbers, + - * /, unary minus and the
    functions abs inv sqrt floor min max log exp sin cos atan2 neg; every other construct is refused"""
    cols = _columns(names)
    p = Program([])

    def emit(node):
        if isinstance(node, ast.BinOp) and type(node.op) in _BINOP:
            emit(node.left)
            emit(node.right)
            p.op(_BINOP[type(node.op)])
        elif isinstance(node, ast.UnaryOp) and isinstance(node.op, ast.USub):
            emit(node.operand)
            p.op("neg")
        elif isinstance(node, ast.Constant) and type(node.value) in (int, float):
            p.push_const(node.value)
        elif isinstance(node, ast.Name):
            if node.id not in cols:
                raise ValueError("unknown name %r" % node.id)
            p.push_col(cols[node.id])
        elif isinstance(node, ast.Call):
            if not isinstance(node.func, ast.Name) or node.func.id not in _ARITY or node.keywords:
                raise ValueError("only %s may be called" % ", ".join(sorted(_ARITY)))
            if len(node.args) != _ARITY[node.func.id]:
                raise ValueError("%s takes %d argument(s)" % (node.func.id, _ARITY[node.func.id]))
            for a in node.args:
                emit(a)
            p.op(node.func.id)
        else:
            raise ValueError("%s is not allowed in a derived column" % type(node).__name__)

    try:
        tree = ast.parse(expr, mode="eval")
    except SyntaxError as e:
        raise ValueError("not an expression: %s" % e) from None
    emit(tree.body)
    check([p], len(names))
    return p


def check(programs, n_par):
    """what apemost_hip_derived_check verifies, on the host: the depth every program reaches; ValueError otherwise"""
    if not 1 <= len(programs) <= MAX_COLUMNS:
        raise ValueError("%d columns outside [1,%d]" % (len(programs), MAX_COLUMNS))
    depths = []
    for c, p in enumerate(programs):
        if not 1 <= len(p.code) <= MAX_CODE:
            raise ValueError("column %d: %d instructions outside [1,%d]" % (c, len(p.code), MAX_CODE))
        depth = deepest = 0
        for i, word in enumerate(p.code):
            op, arg = word & 255, word >> 8
            if op >= len(OPS) or word < 0:
                raise ValueError("column %d, instruction %d: unknown opcode %d" % (c, i, op))
            name = OPS[op]
            if name == "col" and arg > n_par + 1:
                raise ValueError("column %d, instruction %d: COL %d beyond n_par + 1" % (c, i, arg))
            if name == "const" and arg >= len(p.consts):
                raise ValueError("column %d, instruction %d: CONST %d of %d" % (c, i, arg, len(p.consts)))
            pops, pushes = ((0, 1) if name in ("col", "const") else (1, 2) if name == "dup" else (2, 2) if name == "swap"
                            else (_ARITY[name], 1))
            if depth < pops:
                raise ValueError("column %d, instruction %d: stack underflow" % (c, i))
            depth += pushes - pops
            if depth > MAX_DEPTH:
                raise ValueError("column %d, instruction %d: stack depth %d above %d" % (c, i, depth, MAX_DEPTH))
            deepest = max(deepest, depth)
        if depth != 1:
            raise ValueError("column %d leaves %d values, not 1" % (c, depth))
        depths.append(deepest)
    return depths


def pack(programs):
    """(code int32[], start int32[n_col + 1], consts float64[]) of the C ABI: the programs one after the other over one
    table of constants (equal bit patterns share a slot)"""
    table = Program([])
    code, start = [], [0]
    for p in programs:
        for word in p.code:
            if word & 255 == OP["const"]:
                word = ins("const", table._const(p.consts[word >> 8]))
            code.append(word)
        start.append(len(code))
    if len(table.consts) > MAX_CONSTS:
        raise ValueError("%d constants, more than %d" % (len(table.consts), MAX_CONSTS))
    return (np.array(code, dtype=np.int32), np.array(start, dtype=np.int32), np.array(table.consts, dtype=np.float64))


def check_native(programs, n_par):
    """apemost_hip_derived_check on the packed programs: the depths, or ApemostHipError (no device is needed)"""
    import ctypes as C
    # (a CONST operand beyond its program's constants cannot be packed: it goes beyond all constants, unshared)
    total = sum(len(p.consts) for p in programs)
    code, start, consts = [], [0], []
    if all(0 <= w >> 8 < len(p.consts) for p in programs for w in p.code if w & 255 == OP["const"]):
        code, start, consts = pack(programs)
        code, start, programs_left = code.tolist(), start.tolist(), []
    else:
        programs_left = programs
    for p in programs_left:
        for word in p.code:
            if word & 255 == OP["const"] and word >= 0:
                k = word >> 8
                word = ins("const", len(consts) + k if k < len(p.consts) else total + k - len(p.consts))
            code.append(word)
        start.append(len(code))
        consts += p.consts
    code, start = np.array(code if code else [0], dtype=np.int32), np.array(start, dtype=np.int32)
    depth = np.zeros(max(len(programs), 1), dtype=np.int32)
    ip = C.POINTER(C.c_int32)
    capi.check(capi.lib().apemost_hip_derived_check(n_par, len(programs), code.ctypes.data_as(ip), start.ctypes.data_as(ip),
                                                    len(consts), depth.ctypes.data_as(ip)))
    return depth[:len(programs)].tolist()


def _eval_one(p, rows):
    x = np.asarray(rows, dtype=np.float64)
    stack = []
    with np.errstate(all="ignore"):
        for word in p.code:
            name, arg = OPS[word & 255], word >> 8
            if name == "col":
                stack.append(x[:, arg])
            elif name == "const":
                stack.append(np.full(len(x), p.consts[arg]))
            elif name == "dup":
                stack.append(stack[-1])
            elif name == "swap":
                stack[-1], stack[-2] = stack[-2], stack[-1]
            elif name in _UNARY:
                t = stack.pop()
                stack.append(np.negative(t) if name == "neg" else np.abs(t) if name == "abs" else
                             np.divide(1.0, t) if name == "inv" else getattr(np, name)(t))
            else:
                t = stack.pop()
                b = stack.pop()
                stack.append(np.add(b, t) if name == "add" else np.subtract(b, t) if name == "sub" else
                             np.multiply(b, t) if name == "mul" else np.divide(b, t) if name == "div" else
                             np.where(b < t, b, t) if name == "min" else np.where(b > t, b, t) if name == "max" else
                             np.arctan2(b, t))
    return np.array(stack[0], dtype=np.float64)


def eval_numpy(program, rows):
    """the host interpreter: the values of a Program for the rows [n][n_par+2] as [n], of a list of them as
    [n][n_col].  One numpy call per opcode; for programs of the exact group the bits the device gives."""
    if isinstance(program, Program):
        return _eval_one(program, rows)
    rows = np.asarray(rows, dtype=np.float64)
    out = np.zeros((len(rows), len(program)))
    for c, p in enumerate(program):
        out[:, c] = _eval_one(p, rows)
    return out


def _lesser(a, b):
    return b if (b < a or (b == a and math.copysign(1.0, b) < 0)) else a


def _greater(a, b):
    return b if (b > a or (b == a and math.copysign(1.0, b) > 0)) else a


class Derived:
    def __init__(self, joint, hist, batch, nonfinite, vmin, vmax, programs, batch_size=1, names=None, row_names=None,
                 n_par=None):
        self.joint = joint                                                # a Joint over the columns
        self.n = joint.n
        self.n_keep, self.n_col = joint.n_keep, joint.n_par
        self.nbins, self.lo, self.hi, self.chains, self.pairs = joint.nbins, joint.lo, joint.hi, joint.chains, joint.pairs
        self.hist = np.ascontiguousarray(hist, dtype=np.uint64).reshape(self.n_keep, self.n_col, self.nbins)
        self.batch = np.ascontiguousarray(batch, dtype=np.float64)        # [k][c][max_batches + 1]
        assert self.batch.ndim == 3 and self.batch.shape[:2] == (self.n_keep, self.n_col)
        self.nonfinite = np.ascontiguousarray(nonfinite, dtype=np.uint64).reshape(self.n_keep, self.n_col)
        self.vmin = np.ascontiguousarray(vmin, dtype=np.float64).reshape(self.n_keep, self.n_col)
        self.vmax = np.ascontiguousarray(vmax, dtype=np.float64).reshape(self.n_keep, self.n_col)
        self.programs = list(programs)
        assert len(self.programs) == self.n_col
        self.batch_size = int(batch_size)
        self.n_batches_ = np.zeros(1, dtype=np.uint64)
        self.names = ["d%d" % c for c in range(self.n_col)] if names is None else list(names)
        if row_names is None and n_par is not None:
            row_names = ["p%d" % i for i in range(n_par)]
        self.row_names = None if row_names is None else list(row_names)      # the names the RPN text is written with
        assert len(self.names) == self.n_col

    # (the Joint's own, under the names a user of this class expects)
    origin = property(lambda self: self.joint.origin)
    sum = property(lambda self: self.joint.sum)
    cross = property(lambda self: self.joint.cross)
    counts = property(lambda self: self.joint.counts)
    thin = property(lambda self: self.joint.thin)

    @property
    def max_batches(self):
        return self.batch.shape[2] - 1

    @property
    def n_batches(self):
        return batches_closed(int(self.n[0]), self.batch_size)

    @classmethod
    def empty(cls, programs, lo, hi, chains=(0,), nbins=200, pairs=None, batch_size=1, max_batches=0, names=None,
              row_names=None, thin=1, n_par=None):
        n_col, n_keep = len(programs), len(chains)
        pairs = all_pairs(n_col) if pairs is None else pairs
        jt = Joint.empty(n_keep, n_col, nbins, pairs, lo, hi, chains, thin)
        return cls(jt, np.zeros((n_keep, n_col, nbins), dtype=np.uint64), np.zeros((n_keep, n_col, max_batches + 1)),
                   np.zeros((n_keep, n_col), dtype=np.uint64), np.full((n_keep, n_col), np.inf),
                   np.full((n_keep, n_col), -np.inf), programs, batch_size, names, row_names, n_par)

    def view(self):
        """the apemost_hip_derived_view over this object's arrays"""
        j = self.joint
        return capi.DerivedView(n=j.n.ctypes.data_as(capi._up), hist=self.hist.ctypes.data_as(capi._up),
                                batch=self.batch.ctypes.data_as(capi._dp), n_batches=self.n_batches_.ctypes.data_as(capi._up),
                                counts=j.counts.ctypes.data_as(capi._up), origin=j.origin.ctypes.data_as(capi._dp),
                                sum=j.sum.ctypes.data_as(capi._dp), cross=j.cross.ctypes.data_as(capi._dp),
                                nonfinite=self.nonfinite.ctypes.data_as(capi._up), vmin=self.vmin.ctypes.data_as(capi._dp),
                                vmax=self.vmax.ctypes.data_as(capi._dp))

    @classmethod
    def from_rows(cls, rows, programs, lo, hi, chains=(0,), nbins=200, pairs=None, batch_size=1, max_batches=None,
                  names=None, row_names=None, thin=1, values=None):
        """the host fold of sample rows [n][n_chains][n_par+2] (already thinned): what the device computes, for tests
        and for existing dumps.  values: [n][n_chains][n_col] to fold in place of eval_numpy's (those of
        HipSampler.derived_eval, where a program uses the library group)."""
        rows = np.asarray(rows, dtype=np.float64)
        n, n_chains, w = rows.shape
        n_col = len(programs)
        if max_batches is None:
            max_batches = batches_closed(n, batch_size)
        if values is None:
            values = eval_numpy(programs, rows.reshape(n * n_chains, w)).reshape(n, n_chains, n_col)
        values = np.asarray(values, dtype=np.float64)
        # the joint part is the Joint's own host fold over rows whose "parameters" are the computed columns
        as_rows = np.zeros((n, n_chains, n_col + 2))
        as_rows[:, :, :n_col] = values
        jt = Joint.from_rows(as_rows, lo, hi, chains, nbins, pairs, thin)
        dv = cls.empty(programs, lo, hi, chains, nbins, jt.pairs, batch_size, max_batches, names, row_names, thin, w - 2)
        dv.joint = jt
        dv.n = jt.n
        for k, ch in enumerate(chains):
            for c in range(n_col):
                v = values[:, ch, c]
                b = bins_of(v, summary_edges(float(jt.lo[c]), float(jt.hi[c]), nbins))
                dv.hist[k, c] = np.bincount(b[b >= 0], minlength=nbins)
                part, nb, mn, mx, bad = 0.0, 0, math.inf, -math.inf, 0
                for i, x in enumerate(v.tolist(), 1):
                    part += x
                    if i % batch_size == batch_size - 1:
                        dv.batch[k, c, nb] = part
                        part, nb = 0.0, nb + 1
                    if x == x:
                        mn, mx = _lesser(mn, x), _greater(mx, x)
                    if not math.isfinite(x):
                        bad += 1
                dv.batch[k, c, nb] = part
                dv.vmin[k, c], dv.vmax[k, c], dv.nonfinite[k, c] = mn, mx, bad
        return dv

    def per_ladder(self, n_ladders):
        """one Derived per ladder of a batch: the kept chains, ladder-major, in equal shares"""
        if n_ladders < 1 or self.n_keep % n_ladders:
            raise ValueError("%d kept chains are not %d equal ladders" % (self.n_keep, n_ladders))
        per = self.n_keep // n_ladders
        out = []
        for b in range(n_ladders):
            k = slice(b * per, (b + 1) * per)
            j = self.joint
            jt = Joint(j.n.copy(), j.counts[k], j.origin[k], j.sum[k], j.cross[k], j.pairs, j.lo, j.hi, j.nbins, j.chains[k],
                       j.thin)
            out.append(Derived(jt, self.hist[k], self.batch[k], self.nonfinite[k], self.vmin[k], self.vmax[k], self.programs,
                               self.batch_size, self.names, self.row_names))
        return out

    # -- what it gives ------------------------------------------------------------------------
    def mean(self, k=0):
        return self.joint.mean(k)

    def cov(self, k=0):
        return self.joint.cov(k)

    def corr(self, k=0):
        return self.joint.corr(k)

    def density(self, k, q):
        return self.joint.density(k, q)

    def sd(self, k=0):
        with np.errstate(all="ignore"):
            return np.sqrt(np.diag(self.cov(k)))

    def edges(self, c):
        return self.joint.edges(c)

    def min(self, k=0):
        return self.vmin[k]

    def max(self, k=0):
        return self.vmax[k]

    def marginal(self, c, k=0):
        """(edges, density) of column c: counts / (counted * nominal bin width)"""
        h = self.hist[k, c].astype(np.float64)
        with np.errstate(all="ignore"):
            return self.edges(c), h / (h.sum() * ((self.hi[c] - self.lo[c]) / self.nbins))

    def quantile(self, q, c, k=0):
        """the q-quantile (0 <= q <= 1) of the counted values of column c, linear inside its bin; NaN where nothing
        was counted"""
        if not 0 <= q <= 1:
            raise ValueError("quantile %r outside [0, 1]" % (q,))
        e = self.edges(c)
        h = self.hist[k, c].astype(np.float64)
        cum = np.cumsum(h)
        if cum[-1] == 0:
            return float("nan")
        rank = q * cum[-1]
        b = int(np.searchsorted(cum, rank, side="left"))
        while h[b] == 0:
            b += 1
        below = cum[b] - h[b]
        return float(e[b] + (rank - below) / h[b] * (e[b + 1] - e[b]))

    def mcse(self, k=0):
        """[n_col]: batch_means_error() over the closed batches about the column's mean, as RunSummary has it: every
        batch sum divided by batch_size, sqrt(sum d^2 / n_batches).  NaN without a closed batch."""
        nb = self.n_batches
        out = np.full(self.n_col, np.nan)
        if nb == 0:
            return out
        mean = self.mean(k).tolist()
        for c in range(self.n_col):
            err = 0.0
            for s in self.batch[k, c, :nb].tolist():
                d = s / self.batch_size - mean[c]
                err += d * d
            out[c] = math.sqrt(err / nb) if err == err and err >= 0 else float("nan")
        return out

    def text(self, k=0):
        """derived.txt: one line per column, `name n mean sd mcse min max nonfinite`, tab separated, "%.15e\""""
        mean, sd, mcse = self.mean(k), self.sd(k), self.mcse(k)
        fmt = lambda v: "nan" if v != v else "%.15e" % v      # noqa: E731
        return "".join("%s\t%d\t%s\t%s\t%s\t%s\t%s\t%d\n" % (
            self.names[c], int(self.n[0]), fmt(float(mean[c])), fmt(float(sd[c])), fmt(float(mcse[c])),
            fmt(float(self.vmin[k, c])), fmt(float(self.vmax[k, c])), int(self.nonfinite[k, c])) for c in range(self.n_col))

    # -- derived.bin ----------------------------------------------------------------------------
    def _arrays(self):
        j = self.joint
        return ((self.hist, "<u8"), (self.batch, "<f8"), (self.nonfinite, "<u8"), (self.vmin, "<f8"), (self.vmax, "<f8"),
                (j.origin, "<f8"), (j.sum, "<f8"), (j.cross, "<f8"), (j.counts, "<u8"))

    def write(self, path, row_names=None):
        """row_names: the parameter names the RPN text is written with (default: those given at construction)"""
        row_names = row_names or self.row_names
        if row_names is None:
            raise ValueError("the names of the rows' parameters are needed to write the programs as text")
        j = self.joint
        with open(path, "wb") as f:
            f.write(_HEAD.pack(MAGIC, VERSION, self.n_keep, self.n_col, self.nbins, len(self.pairs), len(row_names),
                               int(self.n[0]), j.thin, self.batch_size, self.max_batches, self.n_batches))
            for a, t in ((self.chains, "<i4"), (self.pairs, "<i4"), (self.lo, "<f8"), (self.hi, "<f8")):
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

            def put(s):
                raw = s.encode("utf-8")
                f.write(struct.pack("<I", len(raw)) + raw)
            for name, p in zip(self.names, self.programs):
                put(name)
                put(p.rpn(row_names))
            f.write(struct.pack("<I", len(row_names)))
            for name in row_names:
                put(name)
            for a, t in self._arrays():
                f.write(np.ascontiguousarray(a, dtype=t).tobytes())

    @classmethod
    def read(cls, path):
        with open(path, "rb") as f:
            raw = f.read()
        (magic, version, n_keep, n_col, nbins, n_pairs, n_par, n, thin, bs, max_batches,
         n_batches) = _HEAD.unpack_from(raw, 0)
        if magic != MAGIC or version != VERSION:
            raise ValueError("%s: not a derived file of version %d" % (path, VERSION))
        off = _HEAD.size

        def take(count, dtype):
            nonlocal off
            a = np.frombuffer(raw, dtype=dtype, count=count, offset=off)
            off += a.itemsize * count
            return a.copy()

        def get():
            nonlocal off
            (length,) = struct.unpack_from("<I", raw, off)
            s = raw[off + 4:off + 4 + length].decode("utf-8")
            off += 4 + length
            return s
        chains, pairs = take(n_keep, "<i4"), take(2 * n_pairs, "<i4").reshape(n_pairs, 2)
        lo, hi = take(n_col, "<f8"), take(n_col, "<f8")
        named = [(get(), get()) for _ in range(n_col)]
        (n_names,) = struct.unpack_from("<I", raw, off)
        off += 4
        row_names = [get() for _ in range(n_names)]
        if n_names != n_par:
            raise ValueError("%s: %d row names, the head says %d" % (path, n_names, n_par))
        programs = [parse_rpn(text, row_names) for _, text in named]
        tri, nk = n_col * (n_col + 1) // 2, n_keep * n_col
        hist = take(nk * nbins, "<u8")
        batch = take(nk * (max_batches + 1), "<f8").reshape(n_keep, n_col, max_batches + 1)
        nonfinite, vmin, vmax = take(nk, "<u8"), take(nk, "<f8"), take(nk, "<f8")
        origin, total = take(nk, "<f8").reshape(n_keep, n_col), take(nk, "<f8").reshape(n_keep, n_col)
        cross = take(n_keep * tri, "<f8").reshape(n_keep, tri)
        counts = take(n_keep * n_pairs * nbins * nbins, "<u8")
        if off != len(raw):
            raise ValueError("%s: %d bytes, expected %d" % (path, len(raw), off))
        if n_batches != batches_closed(n, bs):
            raise ValueError("%s: n_batches %d does not follow from n = %d" % (path, n_batches, n))
        jt = Joint([n], counts, origin, total, cross, pairs, lo, hi, nbins, chains, thin)
        return cls(jt, hist, batch, nonfinite, vmin, vmax, programs, bs, [name for name, _ in named], row_names)
