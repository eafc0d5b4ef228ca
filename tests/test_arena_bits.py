"""CPU check of the arena level 2's bin geometry (krust_amd/csrc/arena_bits.h, used by part2_arena_kernel): for every bucket
count the arena path can get -- 32..1024 as powers of two, every other count from 33 to 1023 -- with the kernel instance, payload
size and flush unit the host picks for it, (bucket, byte rank) -> address must be injective into the bins and aligned for the
payload, never the trash word, and a unit's 16-byte words must be where the flush reads them.  The header is plain host
arithmetic (the device compiles the same functions); tests/arena_bits_check.cpp walks the geometries."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bin_addresses_for_every_geometry(tmp_path):
    exe = tmp_path / "arena_bits_check"
    src = os.path.join(ROOT, "tests", "arena_bits_check.cpp")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-o", str(exe), src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "ARENA_BITS_OK 1986 geometries" in r.stdout
