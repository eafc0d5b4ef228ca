"""The host side of kh_unitigs_* and `kmerust unitigs` without a device: the four symbols are declared, exported, bound and weak in the
host layer; unitig_header() and unitig_summary() on hand-made rows (tests/unitigs_check.cpp, also under ASan + UBSan: header and
summary formatting, N50 of no unitig, one unitig and ties, COUNT_SUM near 2^64); the options of the sub-command, and its refusal
against the sanitizer build's stub library, which has none of the four."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
ASAN_BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust_asan")
NEW = ("kh_unitigs_begin", "kh_unitigs_copy_device", "kh_unitigs_copy", "kh_unitigs_end")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_declared_mapped_bound_and_weak():
    from krust_amd import native
    header = re.sub(r"/\*.*?\*/", "", _read("include", "kmerhip.h"), flags=re.S)
    mapfile = _read("krust_amd", "csrc", "kmerhip.map")
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in kmerhip.h"
        assert name in mapfile, f"{name} is not listed in kmerhip.map"
        assert name in native.SYMBOLS, f"{name} is not in native.SYMBOLS"
        assert re.search(r"pub fn %s\(" % name, _read("bindings", "rust", "src", "lib.rs")), f"{name} is not in the Rust crate"
        assert re.search(r"\bfn %s\(" % name, _read("INTEGRATION.md")), f"{name} is not in INTEGRATION.md"
        assert re.search(r"#pragma weak %s\b" % name, _read("krust_amd", "host", "kmerust_host.cpp")), f"{name} is not weak in the host layer"
        assert not re.search(name, _read("tests", "host_asan", "stub_kmerhip.cpp"))  # the stub is what exercises the refusal
    assert re.search(r"global:\s*kh_\*;", mapfile)
    for word in ("UNI_WORDS", "UNI_START", "UNI_KMERS", "UNI_COUNT_SUM", "UNI_FLAGS", "UNI_CIRCULAR"):
        value = int(re.search(r"#define\s+KH_%s\s+(\d+)" % word, header).group(1))
        assert getattr(native, word) == value, word
    assert (native.UNI_WORDS, native.UNI_START, native.UNI_KMERS, native.UNI_COUNT_SUM, native.UNI_FLAGS, native.UNI_CIRCULAR) == (4, 0, 1, 2, 3, 1)
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header)
    assert [len(native.SYMBOLS[n][1]) for n in NEW] == [4, 5, 5, 1]
    for m in ("unitigs", "unitigs_begin", "unitigs_copy", "unitigs_copy_device", "unitigs_end"):
        assert callable(getattr(native.DeviceCounter, m))
    assert re.search(r"pub fn unitigs\(", _read("bindings", "rust", "src", "lib.rs"))
    assert "unitig.hip" in _read("krust_amd", "csrc", "Makefile") and "unitig_bits.h" in _read("krust_amd", "csrc", "Makefile")
    assert "unitig.hip" in _read("krust_amd", "csrc", "ctx.hip.h")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_header_and_summary(tmp_path, flags):
    """The stand-alone check program (its own main, nothing preloaded), plain and under ASan + UBSan."""
    exe = str(tmp_path / "unitigs_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "unitigs_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "unitigs_check ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout + p.stderr


def _run(binary, *args, env=None):
    p = subprocess.run([binary, *args], capture_output=True, text=True, env=None if env is None else {**os.environ, **env})
    return p.returncode, p.stdout, (p.stderr.splitlines() or [""])[0]


@pytest.mark.parametrize("args,first", [
    (["unitigs"], "error: the following required arguments were not provided:"),
    (["unitigs", "-m", "2"], "error: the following required arguments were not provided:"),
    (["unitigs", "a.kmix", "b.kmix"], "error: unexpected argument 'b.kmix' found"),
    (["unitigs", "a.kmix", "-f", "tsv"], "error: invalid value 'tsv' for '--format <FORMAT>'"),
    (["unitigs", "a.kmix", "-f", "json"], "error: invalid value 'json' for '--format <FORMAT>'"),
    (["unitigs", "a.kmix", "-f"], "error: a value is required for '--format <FORMAT>' but none was supplied"),
    (["unitigs", "a.kmix", "-m", "x"], "error: invalid value 'x' for '--min-count <MIN_COUNT>': invalid digit found in string"),
    (["unitigs", "a.kmix", "--min-count=-1"], "error: invalid value '-1' for '--min-count <MIN_COUNT>': invalid digit found in string"),
    (["unitigs", "a.kmix", "--sorted"], "error: unexpected argument '--sorted' found"),
    (["unitigs", "a.kmix", "-q"], "error: unexpected argument '-q' found"),
])
def test_usage_errors(args, first):
    rc, out, err = _run(BIN, *args)
    assert rc == 2 and out == "" and err == first, (rc, out, err)


def test_options_parse_up_to_the_index(tmp_path):
    """Every accepted spelling gets as far as opening the index: exit 1 with the loader's message, not a usage error."""
    missing = str(tmp_path / "none.kmix")
    for args in (["unitigs", missing], ["unitigs", missing, "-m", "3", "-f", "fasta"], ["unitigs", "-fsummary", "--min-count=9223372036854775807", missing],
                 ["unitigs", "--format=summary", missing, "-m2"]):
        p = subprocess.run([BIN, *args], capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith("Application error:\n unitigs: "), (args, p.stderr)


def test_help_names_the_sub_command():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "kmerust unitigs <INDEX> [-m <MIN_COUNT>] [-f fasta|summary]" in p.stdout and "CR:i:1" in p.stdout


def test_refusal_against_a_library_without_the_entry_points(tmp_path):
    """make asan's binary links the stub library, which has no kh_unitigs_*: the command refuses with a message, clean under ASan + UBSan."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "krust_amd", "host"), "asan"], stdout=subprocess.DEVNULL)
    san = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    for extra in ([], ["-f", "summary"], ["-f", "fasta", "-m", "2"]):
        p = subprocess.run([ASAN_BIN, "unitigs", str(tmp_path / "a.kmix"), *extra], capture_output=True, text=True, timeout=120, env={**os.environ, **san})
        assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        assert p.returncode == 1 and p.stdout == "" and "unitigs needs a kmerhip library with kh_unitigs_begin" in p.stderr, p.stderr
    rc, out, err = _run(ASAN_BIN, "unitigs", "a.kmix", "-f", "tsv", env=san)
    assert rc == 2 and err == "error: invalid value 'tsv' for '--format <FORMAT>'"
