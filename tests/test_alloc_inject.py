"""KMERHIP_ALLOC_FAIL / KMERHIP_ALLOC_TRACE without a device: the arming logic of krust_amd/csrc/alloc_inject.h through the
stand-alone check program tests/alloc_inject_check.cpp (its own main, nothing preloaded), plain and under ASan + UBSan -- as
tests/test_cli_args.py drives tests/cli_args_check.cpp; that both are switches of the test build only; and that every device and
pinned-host allocation and release of the library goes through the four wrappers of ctx.hip.h."""
import glob
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "krust_amd", "lib")
CSRC = os.path.join(ROOT, "krust_amd", "csrc")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_the_arming_logic(tmp_path, flags):
    exe = str(tmp_path / "alloc_inject_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", *flags, "-o", exe, os.path.join(ROOT, "tests", "alloc_inject_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "alloc_inject_check ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout + p.stderr


def test_the_header_is_pure():
    """No HIP, no lock, nothing of the library: the check program above is all that is needed to test it."""
    with open(os.path.join(CSRC, "alloc_inject.h")) as f:
        text = f.read()
    assert set(re.findall(r'#include\s+([<"][^>"]+[>"])', text)) == {"<cstdint>", "<cstring>"}
    assert "hip" not in re.sub(r"//.*", "", text).lower()


def test_alloc_switches_are_in_the_test_build_only():
    product, testing = os.path.join(LIB, "libkmerhip.so"), os.path.join(LIB, "libkmerhip_testing.so")
    assert os.path.exists(product) and os.path.exists(testing), "the libraries are not built: make -C krust_amd/csrc"
    with open(testing, "rb") as f:
        t = f.read()
    with open(product, "rb") as f:
        p = f.read()
    for name in (b"KMERHIP_ALLOC_FAIL", b"KMERHIP_ALLOC_TRACE"):
        assert name in t, name
        assert name not in p, name


def test_every_allocation_goes_through_the_wrappers():
    """Outside the four wrappers no source of the library calls the runtime's allocation or release functions (a name inside a
    string -- the error texts -- or a comment is not a call)."""
    calls = re.compile(r"\bhip(?:Host)?(?:Malloc|Free)\s*\(")
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*"))):
        if not path.endswith((".hip", ".h")):
            continue
        with open(path) as f:
            text = f.read()
        if path.endswith("ctx.hip.h"):  # the wrappers themselves: the one place that may
            lo, hi = text.index("#if KH_TESTING\nbool alloc_inject_fails"), text.index("inline hipError_t pin_free(void *p) { return hipHostFree(p); }")
            assert len(calls.findall(text[lo:hi])) == 7  # 4 in the test build's, 3 of the product's before the last line
            text = text[:lo] + text[hi:].split("\n", 1)[1]
        for i, line in enumerate(text.split("\n"), 1):
            code = re.sub(r'"(?:[^"\\]|\\.)*"', '""', line)
            code = re.sub(r"//.*", "", code)
            if calls.search(code):
                found.append("%s:%d" % (os.path.basename(path), i))
    assert not found, found
