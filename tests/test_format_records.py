"""CPU check of the record formatter (krust_amd/csrc/format.hip.h): the functions the device runs on its LDS staging buffer
are __host__ __device__ inlines, and tests/format_check.cpp compiles their host twin with a plain g++.  The expected bytes
are built here, in Python, from the formats of the reference's output_counts (src/run.rs:441-486):
    fasta  >{count}\\n{kmer}\\n        tsv  {kmer}\\t{count}\\n        json  serde_json's pretty form
for every k = 1..32, the keys 0, 4^k - 1 and random ones, and counts at every decimal digit boundary up to 2^64 - 1;
record_len() must be the number of bytes written, and the JSON document framing must parse for 0, 1 and 3 records."""
import json
import os
import random
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FASTA, TSV, JSON = 1, 2, 3

COUNTS = sorted({1, 2, 9, 2**32 - 1, 2**32, 2**32 + 5, 2**63, 2**64 - 1}
                | {10**e for e in range(1, 20)} | {10**e - 1 for e in range(1, 20)} | {10**e + 1 for e in range(1, 20)})


def unpack(key, k):
    return "".join("ACGT"[(key >> (2 * (k - 1 - i))) & 3] for i in range(k))


def record(fmt, k, key, count, first):
    km = unpack(key, k)
    if fmt == FASTA:
        return f">{count}\n{km}\n".encode()
    if fmt == TSV:
        return f"{km}\t{count}\n".encode()
    return (("[\n" if first else ",\n") + f'  {{\n    "kmer": "{km}",\n    "count": {count}\n  }}').encode()


def document(fmt, k, recs):
    body = b"".join(record(fmt, k, key, c, i == 0) for i, (key, c) in enumerate(recs))
    if fmt != JSON:
        return body
    return body + b"\n]\n" if recs else b"[]\n"


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("format_check") / "format_check"
    src = os.path.join(ROOT, "tests", "format_check.cpp")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(cases):
        r = subprocess.run([str(exe)], input="".join(c + "\n" for c in cases), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "FORMAT_CHECK_DONE" and len(lines) == len(cases) + 1, lines[-3:]
        out = []
        for case, line in zip(cases, lines):
            assert not line.startswith("ERR"), (case, line)
            want, wrote, *hx = line.split()
            out.append((int(want), int(wrote), bytes.fromhex(hx[0] if hx else "")))
        return out
    return run


def test_every_k_format_and_digit_boundary(checker):
    rng = random.Random(20260207)
    cases, expect = [], []
    for k in range(1, 33):
        keys = [0, 4**k - 1] + [rng.randrange(4**k) for _ in range(3)]
        for fmt in (FASTA, TSV, JSON):
            for ci, count in enumerate(COUNTS):
                key = keys[ci % len(keys)]
                first = ci & 1
                cases.append(f"R {fmt} {k} {key} {count} {first}")
                expect.append(record(fmt, k, key, count, first))
            for key in keys:  # every key at an ordinary count too
                cases.append(f"R {fmt} {k} {key} 7 0")
                expect.append(record(fmt, k, key, 7, 0))
    got = checker(cases)
    for case, exp, (want, wrote, data) in zip(cases, expect, got):
        assert data == exp, case
        assert want == wrote == len(exp), f"record_len differs from the bytes written: {case}"


def test_document_framing(checker):
    rng = random.Random(5)
    cases, expect = [], []
    for k in (1, 5, 21, 32):
        for fmt in (FASTA, TSV, JSON):
            for n in (0, 1, 3):
                recs = [(rng.randrange(4**k), rng.choice(COUNTS)) for _ in range(n)]
                cases.append(f"D {fmt} {k} {n} " + " ".join(f"{key} {c}" for key, c in recs))
                expect.append((fmt, k, recs, document(fmt, k, recs)))
    got = checker(cases)
    for case, (fmt, k, recs, exp), (want, wrote, data) in zip(cases, expect, got):
        assert data == exp, case
        assert want == wrote == len(exp), case
        if fmt == JSON:
            parsed = json.loads(data)
            assert parsed == [{"kmer": unpack(key, k), "count": c} for key, c in recs]
            assert data == (json.dumps(parsed, indent=2) + "\n").encode()  # serde_json's pretty form is Python's indent=2
        elif not recs:
            assert data == b""
