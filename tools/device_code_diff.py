#!/usr/bin/env python3
"""Is the gfx950 device code of two source trees the same?  For every translation unit of the product library
(build.MODEL_TUS and the ABI unit, which holds the folds and the test hooks) the device-only assembly of both trees
is compiled with the product flags and compared, after the one symbol that hashes the unit's text
(__hip_cuid_<hash>) is replaced by a fixed word.  Equal assembly is equal behaviour and equal speed, so this is how a
refactor of the kernel headers shows both.  It only diffs: nothing is looked for in the assembly.  No GPU needed.

    python tools/device_code_diff.py --against <git revision>        # this tree against a revision of it
    python tools/device_code_diff.py <tree A> <tree B>

Exit status 0 and one sha256 per unit when all units are equal; 1 and the first differing kernel of every unit that
differs otherwise.  --jobs (default: APEMOST_BUILD_JOBS, else 8; never more than 8) compiles run side by side.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys
import tarfile
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from apemost_amd import build  # noqa: E402

UNITS = ["abi"] + ["model_%d" % k for k in build.MODEL_TUS]
CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def unit_command(unit, out):
    """build_hip's compile line for the unit, device assembly instead of an object; paths relative to the tree"""
    flags = [f for f in build.HIP_FLAGS if f not in ("-shared", "-fPIC")] + ["--cuda-device-only", "-S"]
    csrc = os.path.join("apemost_amd", "csrc")
    cmd = [build.HIPCC] + flags + ["-Iinclude", "-I" + csrc]
    if unit == "abi":
        return cmd + ["-o", out, os.path.join(csrc, "apemost_hip.hip")]
    return cmd + ["-DAPEMOST_TU_MODEL=" + unit[len("model_"):], "-o", out, os.path.join(csrc, "apemost_model.hip")]


def assemble(tree, outdir, jobs, units=UNITS):
    """{unit: normalised device assembly} of the tree; the .s files are left in outdir"""
    os.makedirs(outdir, exist_ok=True)

    def run(unit):
        out = os.path.join(os.path.abspath(outdir), unit + ".s")
        subprocess.check_call(unit_command(unit, out), cwd=tree)
        return CUID.sub("__hip_cuid_X", open(out).read())

    with ThreadPoolExecutor(jobs) as pool:
        return dict(zip(units, pool.map(run, units)))


def first_difference(a, b):
    """(symbol, line number, line of a, line of b) at the first line where the two assemblies part"""
    la, lb = a.splitlines(), b.splitlines()
    symbol = "<before the first symbol>"
    for n in range(max(len(la), len(lb))):
        x = la[n] if n < len(la) else "<end of file>"
        y = lb[n] if n < len(lb) else "<end of file>"
        if x != y:
            return symbol, n + 1, x, y
        m = re.match(r"^([A-Za-z_][\w$.]*):", x)
        if m:
            symbol = m.group(1)
    return None


def demangle(symbol):
    try:
        return subprocess.run(["c++filt", symbol], stdout=subprocess.PIPE, check=True).stdout.decode().strip()
    except (OSError, subprocess.CalledProcessError):
        return symbol


def export(revision, into):
    """the revision's files (git archive) under `into`"""
    tar = os.path.join(into, "tree.tar")
    subprocess.check_call(["git", "-C", ROOT, "archive", "-o", tar, revision, "apemost_amd/csrc", "include"])
    tree = os.path.join(into, "tree")
    with tarfile.open(tar) as t:
        t.extractall(tree)
    return tree


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("trees", nargs="*", help="two source trees; or one (default: this one) with --against")
    ap.add_argument("--against", metavar="REV", help="compare the tree with this git revision of it")
    ap.add_argument("--jobs", type=int, default=int(os.environ.get("APEMOST_BUILD_JOBS", "8")))
    ap.add_argument("--keep", metavar="DIR", help="leave the .s files under DIR/a and DIR/b")
    args = ap.parse_args()
    if len(args.trees) > 1 if args.against else len(args.trees) != 2:
        ap.error("give two trees, or --against REV with at most one tree")
    jobs = max(1, min(8, args.jobs))
    with tempfile.TemporaryDirectory() as tmp:
        work = args.keep or tmp
        if args.against:
            tree_a, tree_b = export(args.against, tmp), (args.trees[0] if args.trees else ROOT)
        else:
            tree_a, tree_b = args.trees
        asm_a = assemble(tree_a, os.path.join(work, "a"), jobs)
        asm_b = assemble(tree_b, os.path.join(work, "b"), jobs)
    differ = 0
    for unit in UNITS:
        d = first_difference(asm_a[unit], asm_b[unit])
        if d:
            differ += 1
            print("%-9s DIFFERS in %s (line %d)\n    a: %s\n    b: %s" % (unit, demangle(d[0]), d[1], d[2], d[3]))
        else:
            print("%-9s %s" % (unit, hashlib.sha256(asm_b[unit].encode()).hexdigest()))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
