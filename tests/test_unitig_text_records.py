"""CPU check of the unitig text formatter (krust_amd/csrc/unitig_text.hip.h): what the device runs on its LDS image are __host__
__device__ inlines, and tests/unitig_text_check.cpp compiles their host twin with a plain g++ beside the host writers of
krust_amd/host/kmerust_host.h (unitig_header, gfa_segment_tags, gfa_segment_line, gfa_link_line) and compares the two: record lengths
and bytes at every digit edge of the index, the length, the count sum and both link indices, k = 1 and k = 32, circular or not, both
signs on both sides of a link, every record cut at every offset as a tile edge cuts it, and km against snprintf("%.1f") on the ties,
L = 0, cs < L, cs >= 2^53, cs = 2^64 - 1 and 600 000 seeded random pairs.  The program has its own main, so it runs under ASan and
UBSan as well."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "asan-ubsan"])
def test_host_twin_matches_the_host_writers(tmp_path, flags):
    exe = str(tmp_path / "unitig_text_check")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "unitig_text_check.cpp")],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and p.stdout.startswith("unitig_text_check ok "), p.stdout[-2000:] + p.stderr[-3000:]
    assert "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-3000:]
    assert int(p.stdout.split()[2]) > 700_000


def test_tile_constant_is_mirrored():
    """native.UNI_TEXT_TILE is UT_TILE of the header, and the two format constants are the header's."""
    import re
    import sys
    sys.path.insert(0, ROOT)
    from krust_amd import native
    h = open(os.path.join(ROOT, "krust_amd", "csrc", "unitig_text.hip.h")).read()
    assert int(re.search(r"constexpr uint32_t UT_TILE = (\d+);", h).group(1)) == native.UNI_TEXT_TILE
    abi = open(os.path.join(ROOT, "include", "kmerhip.h")).read()
    assert int(re.search(r"#define KH_UNI_TEXT_FASTA (\d+)", abi).group(1)) == native.KH_UNI_TEXT_FASTA
    assert int(re.search(r"#define KH_UNI_TEXT_GFA\s+(\d+)", abi).group(1)) == native.KH_UNI_TEXT_GFA
