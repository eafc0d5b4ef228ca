"""CPU check of the table / partition geometry arithmetic (krust_amd/csrc/geom_bits.h: kh_geom_of_regions, kh_x_of, kh_p1_of,
kh_bucket_of_x, kh_start_of_x, kh_xlo_k, kh_x_zero_bits, kh_below_region, kh_hash_of_below, kh_below_bits) and the table hash of
kmer_bits.h, compiled for the host by g++ as the device compiles them: tests/geometry_check.cpp holds them to plain 128-bit
integer arithmetic for every k = 1..32, every region count in REGIONS and all 4^k keys when k <= 10 (2^20 distinct random keys otherwise):

* region = p1 * b2 + floor(x * b2 / 2^32) < regions, and non-decreasing in the left-aligned hash H;
* kh_hash_of_below(region, kh_below_region(H)) == H wherever kh_below_bits <= 32 (the top p1_bits + 32 + log2 b2 bits of H beyond that)
  -- the round trip every exchange unit and the 8-byte table image rest on --, the geometries with 2k <= p1_bits (a 10-bit level-1
  digit and a 2k-bit hash: k <= 5) and kh_x_zero_bits at its clamp (z >= 32) among them;
* the low p1_bits + 32 - 2k bits of x - kh_xlo_k(bucket) are zero (the exchange units keep their count field there), and
  kh_x_zero_bits is exactly that number (31 at the clamp);
* distinct keys of one region have distinct `below` words.

One run of the checker serves every case; the test id names the geometry, the message the k and the first keys that failed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = list(range(1, 33))
REGIONS = [1 << j for j in range(11)] + [1024 * b2 for b2 in (2, 3, 5, 24, 40, 100, 160, 640, 800, 1024)]


def _rid(regions):
    return f"regions{regions}" if regions <= 1024 else f"regions1024x{regions >> 10}"


@pytest.fixture(scope="module")
def checker_run(tmp_path_factory):
    exe = tmp_path_factory.mktemp("geometry") / "geometry_check"
    src = os.path.join(ROOT, "tests", "geometry_check.cpp")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-pthread", "-o", str(exe), src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    nthreads = max(1, min(8, len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)))
    r = subprocess.run([str(exe), str(nthreads)], capture_output=True, text=True, timeout=1200)
    rows = {}
    for m in re.finditer(r"^GEOM k=(\d+) regions=(\d+) keys=(\d+) (OK|FAIL \d+)$", r.stdout, re.M):
        rows[(int(m.group(1)), int(m.group(2)))] = (int(m.group(3)), m.group(4))
    return r, rows


@pytest.mark.parametrize("regions", REGIONS, ids=_rid)
def test_geometry_arithmetic_every_k(checker_run, regions):
    r, rows = checker_run
    bad = []
    for k in KS:
        assert (k, regions) in rows, f"the checker reported nothing for k={k} regions={regions}: rc={r.returncode} {r.stderr[-2000:]}"
        nkeys, verdict = rows[(k, regions)]
        assert nkeys == min(4 ** k, 1 << 20), (k, regions, nkeys)   # every key of a small k
        if verdict != "OK":
            bad.append(f"k={k}: {verdict}")
    mine = [line for line in r.stderr.splitlines() if f" regions={regions} " in line]
    assert not bad, f"{_rid(regions)}: {bad}\n" + "\n".join(mine[:40])


def test_checker_saw_every_case_and_the_hash(checker_run):
    r, rows = checker_run
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    assert "HASH k=" not in r.stdout, r.stderr[-3000:]
    assert f"GEOMETRY_OK {len(KS)} x {len(REGIONS)}" in r.stdout
    assert sorted(rows) == sorted((k, n) for k in KS for n in REGIONS)
