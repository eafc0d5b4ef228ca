"""The bit formulas of the de Bruijn neighbours (include/kmerhip.h; krust_amd/csrc/graph_bits.h, the __host__ __device__ helper
graph.hip includes) without a GPU: compiled for the host (tests/graph_bits_check.cpp) and compared, for every k = 1..32 and seeded
keys, with string arithmetic -- O.unpack, s[1:] + c / c + s[:-1], O.canonical.  Catches the k = 32 shifts and the complement of the
reverse neighbour."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MASK64 = (1 << 64) - 1


def revcomp(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


def keys_of(k, rng):
    """Canonical strings of length k: random ones, the two homopolymer classes, a palindrome at even k, and strings whose
    neighbours flip strand (they start or end in a run)."""
    strs = [bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8)) for _ in range(48)]
    strs += [b"A" * k, b"C" * k, (b"AC" * k)[:k], (b"A" * (k - 1) + b"T")[:k], (b"T" + b"A" * (k - 1))[:k], (b"G" * k)]
    if k % 2 == 0:
        half = bytes(rng.choice(list(b"ACGT"), k // 2).astype(np.uint8))
        strs += [half + revcomp(half), (b"AT" * k)[:k]]
    return [min(s, revcomp(s)) for s in strs]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("graph_bits") / "graph_bits_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-o", path,
                    os.path.join(ROOT, "tests", "graph_bits_check.cpp")], check=True)
    return path


def test_neighbours_and_validity_for_every_k(exe):
    rng = np.random.default_rng(11)
    lines, want = [], []
    for k in range(1, 33):
        for s in keys_of(k, rng):
            x = O.pack(s)
            assert O.canonical(s) == (x, False) and O.unpack(x, k) == s.decode()
            right = [O.canonical(s[1:] + bytes([c]))[0] for c in b"ACGT"]
            left = [O.canonical(bytes([c]) + s[:-1])[0] for c in b"ACGT"]
            lines.append(f"{k} {x}")
            want.append([1] + right + left)
            r = O.pack(revcomp(s))
            if r != x:                      # the non-canonical word of the same k-mer: no key
                lines.append(f"{k} {r}")
                want.append([0])
            for bit in (2 * k, 2 * k + 1, 63):   # a bit at or above 2k: no key of this k
                if bit < 64 and bit >= 2 * k:
                    lines.append(f"{k} {x | (1 << bit)}")
                    want.append([0])
        lines.append(f"{k} {MASK64}")       # the all-ones word: T^k is not canonical, and at k < 32 bits stand above 2k
        want.append([0])
    p = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr, p.stderr[-2000:]
    got = [[int(v) for v in l.split()] for l in p.stdout.splitlines()]
    assert len(got) == len(want)
    for line, g, w in zip(lines, got, want):
        if w[0] == 0:
            assert g[0] == 0, line
        else:
            assert g == w, (line, g, w)


def test_special_cases_follow_the_formulas(exe):
    """A homopolymer is its own neighbour, at k = 1 every key is everyone's neighbour, a palindrome's two sides mirror each other."""
    k1 = subprocess.run([exe], input="1 0\n1 1\n", capture_output=True, text=True).stdout.splitlines()
    assert k1[0].split() == ["1", "0", "1", "1", "0", "0", "1", "1", "0"]      # A: neighbours canon(A, C, G, T) = A, C, C, A on both sides
    assert k1[1].split() == ["1", "0", "1", "1", "0", "0", "1", "1", "0"]      # C: the same letters
    a21 = subprocess.run([exe], input="21 0\n", capture_output=True, text=True).stdout.split()
    assert a21[0] == "1" and int(a21[1]) == 0 and int(a21[5]) == 0             # A^21 + A and A + A^21 are A^21
    pal = O.pack(b"ACGT")
    g = [int(v) for v in subprocess.run([exe], input=f"4 {pal}\n", capture_output=True, text=True).stdout.split()]
    assert g[0] == 1 and [g[1 + c] for c in range(4)] == [g[5 + (3 - c)] for c in range(4)]   # right by c == left by complement(c)
