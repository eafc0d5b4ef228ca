"""CPU check of the device radix sort's pass plan (krust_amd/csrc/sort.hip.h): for every k = 1..32 the passes cover the bits
0 .. 2k - 1 of a packed key exactly once and nothing at or above 2k, least significant digit first, in the documented number of
passes, ceil(2k / 8).  The helpers are host-and-device inlines: what runs here is what sort.hip plans its launches with."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass_plan_covers_the_key_bits_for_every_k(tmp_path):
    exe = tmp_path / "sort_plan_check"
    src = os.path.join(ROOT, "tests", "sort_plan_check.cpp")
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), src], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "SORT_PLAN_OK 32" in r.stdout
