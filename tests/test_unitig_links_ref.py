"""The oriented-successor arithmetic of the unitig construction (include/kmerhip.h; krust_amd/csrc/unitig_bits.h, the __host__
__device__ helper unitig.hip includes) without a GPU: compiled for the host (tests/unitig_bits_check.cpp, plain and under ASan +
UBSan, a stand-alone program) and compared, for every k = 1..32 and seeded keys, with string arithmetic -- w[1:] + c, min(t, rc(t)),
which sign the successor is entered with, palindromes, homopolymer loops and hairpins, and which bit of the kh_graph_* mask says so."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def keys_of(k, rng):
    """Canonical strings of length k: random ones, homopolymers, strings with a hairpin successor (w[1:] + c == rc(w)), and at even k
    palindromes and their neighbours."""
    strs = [bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8)) for _ in range(40)]
    strs += [b"A" * k, b"C" * k, (b"AC" * k)[:k], (b"A" * (k - 1) + b"T")[:k], (b"T" + b"A" * (k - 1))[:k], b"G" * k]
    for _ in range(4):   # hairpins: w = a + m with m[1:] + c == rc(a + m): take t = rc(w) = w[1:] + c, i.e. w[1:] = rc(w)[:-1]
        h = bytes(rng.choice(list(b"ACGT"), (k + 1) // 2).astype(np.uint8))
        w = (h + revcomp(h)[(1 if k % 2 == 0 else 2):])[:k] if k > 1 else h
        strs.append(w)
    if k % 2 == 0:
        half = bytes(rng.choice(list(b"ACGT"), k // 2).astype(np.uint8))
        pal = half + revcomp(half)
        strs += [pal, (b"AT" * k)[:k], (b"A" + pal)[:k], (pal + b"C")[1:]]
    return sorted(set(min(s, revcomp(s)) for s in strs if len(s) == k))


@pytest.fixture(scope="module", params=[[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def exe(request, tmp_path_factory):
    path = str(tmp_path_factory.mktemp("unitig_bits") / "unitig_bits_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *request.param, "-o", path, os.path.join(ROOT, "tests", "unitig_bits_check.cpp")],
                   check=True)
    return path


SAN = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}


def run(exe, lines):
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, env={**os.environ, **SAN})
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-2000:]
    return [l.split() for l in p.stdout.splitlines()]


def test_successors_for_every_k(exe):
    rng = np.random.default_rng(12)
    lines, strs = [], []
    for k in range(1, 33):
        for s in keys_of(k, rng):
            assert O.canonical(s) == (O.pack(s), False)
            lines.append(f"{k} {O.pack(s)}")
            strs.append(s)
    got = run(exe, lines)
    assert len(got) == len(strs)
    seen = {"pal": 0, "loop": 0, "hairpin": 0, "minus": 0, "ypal": 0}
    for s, g in zip(strs, got):
        k = len(s)
        assert int(g[0]) == (1 if revcomp(s) == s else 0), s
        assert g[1].encode() == s and g[2].encode() == revcomp(s), s
        seen["pal"] += int(g[0])
        for sign in (0, 1):
            w = s if sign == 0 else revcomp(s)
            for c in range(4):
                y, ysign, ypal, selfl, bit, nb = (int(v) for v in g[3 + 6 * (4 * sign + c):9 + 6 * (4 * sign + c)])
                t = w[1:] + b"ACGT"[c:c + 1]
                ty = min(t, revcomp(t))
                assert y == O.pack(ty) and ysign == (0 if t == ty else 1) and ypal == (1 if t == revcomp(t) else 0), (s, sign, c)
                assert selfl == (1 if ty == s else 0), (s, sign, c)
                # the mask bit that says so: the right neighbour by c for +, the left neighbour by the complement of c for -
                assert bit == (c if sign == 0 else 4 + (3 - c)) and nb == y, (s, sign, c)
                if sign == 0:
                    assert ty == min(s[1:] + b"ACGT"[c:c + 1], revcomp(s[1:] + b"ACGT"[c:c + 1]))
                else:
                    left = b"ACGT"[3 - c:4 - c] + s[:-1]
                    assert ty == min(left, revcomp(left))
                seen["minus"] += ysign
                seen["ypal"] += ypal
                if ty == s:
                    seen["loop" if t == w else "hairpin"] += 1
    assert all(v > 0 for v in seen.values()), seen   # palindromes, homopolymer loops and hairpins were among the keys


def test_special_cases(exe):
    g = run(exe, ["1 0", "1 1", f"4 {O.pack(b'ACGT')}", f"21 {O.pack(b'A' * 21)}", f"3 {O.pack(b'AAT')}", f"32 {O.pack(b'A' * 32)}"])
    # k = 1: A's successors by A, C, G, T are A+, C+, C-, A- (G and T are entered as the reverse of C and A)
    assert [g[0][3 + 6 * c:6 + 6 * c] for c in range(4)] == [["0", "0", "0"], ["1", "0", "0"], ["1", "1", "0"], ["0", "1", "0"]]
    assert g[2][0] == "1" and g[2][1] == g[2][2] == "ACGT"                       # a palindrome spells the same both ways
    assert g[3][3:7] == ["0", "0", "0", "1"] and g[5][3:7] == ["0", "0", "0", "1"]   # A^k + A is A^k itself: the loop, also at k = 32
    aat = O.pack(b"AAT")
    assert [int(v) for v in g[4][3 + 6 * 3:3 + 6 * 3 + 4]] == [aat, 1, 0, 1]     # AAT + T = ATT = rc(AAT): the hairpin, entered as -
