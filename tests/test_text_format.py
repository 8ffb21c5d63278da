"""The device text formatter (apemost_amd/csrc/pt_text.h) built for the host and compared with glibc's snprintf
byte for byte, in both conversions of the text sink ("%.15e\\n" and "%6e\\t%6e\\n"): 10^7 random bit patterns,
10^6 values in sample ranges, every power of two and its neighbours, the neighbours of every power of ten,
values next to 7- and 16-digit half-way points, exact ties at both precisions, and the special values
(tests/text_format_check.cpp)."""
import os
import subprocess

from apemost_amd import build

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "apemost_amd", "csrc")


def _driver(tmp_path):
    exe = str(tmp_path / "text_format_check")
    subprocess.check_call([build.HIPCC, "--offload-arch=gfx950", "-O2", "-std=c++17", "-I" + CSRC,
                           os.path.join(HERE, "text_format_check.cpp"), "-o", exe, "-lpthread"])
    return exe


def test_formatter_matches_glibc_snprintf(tmp_path):
    out = subprocess.run([_driver(tmp_path)], stdout=subprocess.PIPE, universal_newlines=True, timeout=1200,
                         check=True).stdout
    sets = {}
    for line in out.splitlines():
        f = line.split()
        if len(f) == 3 and not line.startswith("MISMATCH"):
            sets[f[0]] = (int(f[1]), int(f[2]))
    assert "MISMATCH" not in out, out
    assert sets["random_bits"][0] >= 10 ** 7 and sets["typical"][0] >= 10 ** 6, sets
    assert sets["powers_of_two"][0] == 2 * 3 * (1023 + 1074 + 1), sets
    for name in ("random_bits", "typical", "powers_of_two", "powers_of_ten", "near_halfway", "exact_ties", "special"):
        assert name in sets and sets[name][1] == 0, (name, sets)
