"""kh_pop_beats and kh_mul_64x64 (krust_amd/csrc/unitig_bits.h: the text the device and this check compile) against Python integers, on
the pairs tests/pop_bits_check.cpp prints -- plain, and as a stand-alone program under ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def beats(kmers_b, sum_b, idx_b, kmers_i, sum_i, idx_i):
    """The rule, as include/kmerhip.h words it (tests/test_pop_ref.py has the same comparator; it is repeated here so that this file
    needs nothing the oracle library builds)."""
    pb, pi = sum_b * kmers_i, sum_i * kmers_b            # exact: Python integers
    if pb != pi:
        return pb > pi
    if kmers_b != kmers_i:
        return kmers_b > kmers_i
    return idx_b < idx_i


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_pop_beats_on_the_grid(tmp_path, flags):
    exe = str(tmp_path / "pop_bits_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "pop_bits_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout[-2000:] + p.stderr
    lines = p.stdout.splitlines()
    muls = [l for l in lines if l.startswith("mul ")]
    pairs = [l for l in lines[:-1] if not l.startswith("mul ")]
    assert lines[-1] == f"pop_bits_check ok {len(pairs)}" and len(muls) == 100 and len(pairs) == 7 * 8 * 7 * 8 * 3 + 5 * 7 * 7 * 2 + 4000
    past64 = 0
    for line in muls:
        a, b, hi, lo = (int(x) for x in line.split()[1:])
        assert (hi << 64) | lo == a * b and lo < 1 << 64, line
        past64 += hi > 0
    assert past64 >= 30
    seen = set()
    wide = 0
    for line in pairs:
        kb, sb, ib, ki, si, ii, got, back = (int(x) for x in line.split())
        assert ib != ii and got == int(beats(kb, sb, ib, ki, si, ii)) and back == int(beats(ki, si, ii, kb, sb, ib)), line
        assert got != back, line                                        # total and antisymmetric: exactly one of two beats the other
        pb, pi = sb * ki, si * kb
        wide += pb >> 64 != 0 and pi >> 64 != 0 and pb != pi and (pb & ((1 << 64) - 1) > pi & ((1 << 64) - 1)) != (pb > pi)
        seen.add(("mean" if pb != pi else "kmers" if kb != ki else "index", got))
    # every branch both ways, and products past 2^64 whose LOW words alone would have decided the other way
    assert seen == {(w, g) for w in ("mean", "kmers", "index") for g in (0, 1)} and wide > 0, (seen, wide)
    vals = {int(line.split()[1]) for line in pairs} | {int(line.split()[0]) for line in pairs}
    assert {(1 << 64) - 1, (1 << 64) - 2, 1 << 63, (1 << 31) - 1, (1 << 31) - 2} <= vals


def test_the_comparator_is_the_reference_s():
    """The comparator above and PopRef's agree (no device; needs the oracle library only to import)."""
    import test_pop_ref as R
    vals = (0, 1, 2, 3, 6, 21, 1 << 32, (1 << 63) + 5, (1 << 64) - 1)
    for kb in vals[1:]:
        for sb in vals:
            for ki in vals[1:]:
                for si in vals:
                    for ib, ii in ((0, 1), (1, 0)):
                        assert R.beats(kb, sb, ib, ki, si, ii) == beats(kb, sb, ib, ki, si, ii)
