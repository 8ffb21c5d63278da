"""The kernel sources carry no experiment switches: a variant that was measured and dropped is a row in DESIGN.md 9 and
a commit in the history, not a branch behind a macro that nothing compiles.  What the preprocessor may still test
under apemost_amd/csrc/ is listed here -- the build's structure, the user-supplied model's hooks and the diagnostic
twin's stamps -- and a macro that is not on the list fails the first test.  The twin's two forms are the only
compile-time variants of the kernels left; one development build each (pulse model, four likelihood waves: with and
without the helper wavefront), cross-compiled for gfx950 -- no GPU needed."""
import os
import re

from apemost_amd import build

ALLOWED_MACROS = {
    # how the library is cut into translation units, and the development builds' subsets
    "APEMOST_TU_MODEL", "APEMOST_SINGLE_TU", "APEMOST_DEV_MODELS", "APEMOST_DEV_WAVES", "APEMOST_DEV_VARIANTS",
    # a user-supplied model compiled at run time, and its optional hooks
    "__HIPCC_RTC__", "APEMOST_USER_MODEL", "APEMOST_USER_CURVE", "APEMOST_USER_POINTWISE",
    # the diagnostic twin (tools/ob_profile.py, tools/stamp_profile.py)
    "APEMOST_STAMPS", "APEMOST_STAMP_WAVE", "APEMOST_STAMP_PHASES",
    # the compiler's own
    "__HIP_DEVICE_COMPILE__",
}
CONDITIONAL = re.compile(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$")


def macros_tested(path):
    """{macro: first line number} of every name a conditional directive of the file tests; a header guard (#ifndef X
    with #define X on the next line) is not a switch"""
    found = {}
    lines = open(path).read().splitlines()
    for n, line in enumerate(lines):
        m = CONDITIONAL.match(line)
        if not m:
            continue
        expr = re.sub(r"//.*|/\*.*?\*/", "", m.group(2))
        names = [w for w in re.findall(r"[A-Za-z_]\w*", expr) if w != "defined"]
        if m.group(1) == "ifndef" and len(names) == 1 and n + 1 < len(lines) and \
                re.match(r"^\s*#\s*define\s+%s\s*$" % re.escape(names[0]), lines[n + 1]):
            continue
        for w in names:
            found.setdefault(w, n + 1)
    return found


def test_the_sources_test_no_macro_that_is_not_listed():
    stray = []
    for root, _, files in os.walk(build.CSRC):
        for f in sorted(files):
            if f.endswith((".h", ".hip")):
                path = os.path.join(root, f)
                stray += ["%s:%d: %s" % (os.path.relpath(path, build.ROOT), n, w)
                          for w, n in macros_tested(path).items() if w not in ALLOWED_MACROS]
    assert not stray, "compile-time switches in the kernel sources (resolve them, or list them here with a reason):\n" + "\n".join(stray)


def test_the_diagnostic_builds_compile(tmp_path):
    for n, extra in enumerate((["-DAPEMOST_STAMPS"], ["-DAPEMOST_STAMPS", "-DAPEMOST_STAMP_PHASES"])):
        out = build.build_dev([1], [4], out=str(tmp_path / ("stamps%d.so" % n)), extra=extra)
        assert os.path.getsize(out) > 100000
