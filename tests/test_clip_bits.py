"""kh_clip_beats (krust_amd/csrc/unitig_bits.h: the text the device and this check compile) against the comparator of the rule in Python
(tests/test_clip_ref.py), on the grid tests/clip_bits_check.cpp prints -- plain, and as a stand-alone program under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def beats(kmers_b, sum_b, idx_b, cand_b, kmers_i, sum_i, idx_i):
    """The rule, as include/kmerhip.h words it (tests/test_clip_ref.py has the same comparator; it is repeated here so that this file
    needs nothing the oracle library builds)."""
    if not cand_b:
        return True
    if (kmers_b, sum_b) != (kmers_i, sum_i):
        return (kmers_b, sum_b) > (kmers_i, sum_i)
    return idx_b < idx_i


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_clip_beats_on_the_grid(tmp_path, flags):
    exe = str(tmp_path / "clip_bits_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "clip_bits_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout[-2000:] + p.stderr
    lines = p.stdout.splitlines()
    assert lines[-1] == f"clip_bits_check ok {len(lines) - 1}" and len(lines) - 1 == 6 * 5 * 6 * 5 * 4 * 2
    seen = set()
    for line in lines[:-1]:
        kb, sb, ib, cb, ki, si, ii, got = (int(x) for x in line.split())
        assert got == int(beats(kb, sb, ib, bool(cb), ki, si, ii)), line
        seen.add((cb, kb == ki, sb == si, (ib > ii) - (ib < ii), got))
    # the grid reaches every branch: a non-candidate, a decision by KMERS, by COUNT_SUM, by index either way, and equal indices
    assert {(0, True, True, 1, 1), (1, False, True, 1, 1), (1, False, True, -1, 0), (1, True, False, 1, 1), (1, True, False, -1, 0),
            (1, True, True, -1, 1), (1, True, True, 1, 0), (1, True, True, 0, 0)} <= seen
    sums = {int(line.split()[1]) for line in lines[:-1]}
    assert {0, 1 << 32, (1 << 64) - 1} <= sums


def test_the_comparator_is_the_reference_s():
    """The comparator above and ClipRef's agree wherever the grid's values go (no device; needs the oracle library only to import)."""
    import test_clip_ref as R
    vals = (0, 1, 21, 1 << 32, (1 << 64) - 1)
    for kb in vals:
        for sb in vals:
            for ki in vals:
                for si in vals:
                    for ib, ii in ((0, 1), (1, 0), (7, 7)):
                        for cb in (False, True):
                            assert R.beats(kb, sb, ib, cb, ki, si, ii) == beats(kb, sb, ib, cb, ki, si, ii)
