"""The host side of kh_graph_* and `kmerust graph` without a device: the three symbols are declared, exported, bound and weak in the
host layer; graph_summary() and format_graph_line() on hand-made words (tests/graph_check.cpp, also under ASan + UBSan); the options
of the sub-command, and its refusal against the sanitizer build's stub library, which has none of the three."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
ASAN_BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust_asan")
NEW = ("kh_graph_stats", "kh_graph_masks_device", "kh_graph_masks")


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
        assert re.search(r"#pragma weak %s\b" % name, _read("krust_amd", "host", "kmerust_host.cpp")), f"{name} is not weak in the host layer"
        assert not re.search(name, _read("tests", "host_asan", "stub_kmerhip.cpp"))  # the stub is what exercises the refusal
    assert re.search(r"global:\s*kh_\*;", mapfile)
    for word in ("GRAPH_WORDS", "GRAPH_NODES", "GRAPH_KMERS"):
        value = int(re.search(r"#define\s+KH_%s\s+(\d+)" % word, header).group(1))
        assert getattr(native, word) == value, word
    assert native.GRAPH_WORDS == 258 and [native.GRAPH_RIGHT(c) for c in range(4)] == [1, 2, 4, 8] and [native.GRAPH_LEFT(c) for c in range(4)] == [16, 32, 64, 128]
    assert re.search(r"#define\s+KH_GRAPH_RIGHT\(c\)\s+\(1u << \(c\)\)", header) and re.search(r"#define\s+KH_GRAPH_LEFT\(c\)\s+\(16u << \(c\)\)", header)
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header)
    assert len(native.SYMBOLS["kh_graph_stats"][1]) == 3 and len(native.SYMBOLS["kh_graph_masks"][1]) == 5 and len(native.SYMBOLS["kh_graph_masks_device"][1]) == 5
    for m in ("graph_stats", "graph_masks", "graph_masks_device"):
        assert callable(getattr(native.DeviceCounter, m))
    assert "graph.hip" in _read("krust_amd", "csrc", "Makefile") and "graph.hip" in _read("krust_amd", "csrc", "ctx.hip.h")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_summary_and_line_formatter(tmp_path, flags):
    """The stand-alone check program (its own main, nothing preloaded), plain and under ASan + UBSan."""
    exe = str(tmp_path / "graph_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "graph_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "graph_check ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout + p.stderr


def _run(binary, *args, env=None):
    p = subprocess.run([binary, *args], capture_output=True, text=True, env=None if env is None else {**os.environ, **env})
    return p.returncode, p.stdout, (p.stderr.splitlines() or [""])[0]


@pytest.mark.parametrize("args,first", [
    (["graph"], "error: the following required arguments were not provided:"),
    (["graph", "-m", "2"], "error: the following required arguments were not provided:"),
    (["graph", "a.kmix", "b.kmix"], "error: unexpected argument 'b.kmix' found"),
    (["graph", "a.kmix", "-f", "fasta"], "error: invalid value 'fasta' for '--format <FORMAT>'"),
    (["graph", "a.kmix", "-f"], "error: a value is required for '--format <FORMAT>' but none was supplied"),
    (["graph", "a.kmix", "-m", "x"], "error: invalid value 'x' for '--min-count <MIN_COUNT>': invalid digit found in string"),
    (["graph", "a.kmix", "--min-count=-1"], "error: invalid value '-1' for '--min-count <MIN_COUNT>': invalid digit found in string"),
    (["graph", "a.kmix", "--sorted=1"], "error: unexpected argument '--sorted=1' found"),
    (["graph", "a.kmix", "--sortedd"], "error: unexpected argument '--sortedd' found"),
    (["graph", "a.kmix", "-q"], "error: unexpected argument '-q' found"),
    (["graph", "a.kmix", "--min-count-a", "2"], "error: unexpected argument '--min-count-a' found"),
])
def test_usage_errors(args, first):
    rc, out, err = _run(BIN, *args)
    assert rc == 2 and out == "" and err == first, (rc, out, err)


def test_options_parse_up_to_the_index(tmp_path):
    """Every accepted spelling gets as far as opening the index: exit 1 with the loader's message, not a usage error."""
    missing = str(tmp_path / "none.kmix")
    for args in (["graph", missing], ["graph", missing, "-m", "3", "-f", "tsv", "--sorted"], ["graph", "-fjson", "--min-count=9223372036854775807", missing],
                 ["graph", "--format=summary", missing, "-m2"]):
        p = subprocess.run([BIN, *args], capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith("Application error:\n graph: "), (args, p.stderr)


def test_help_names_the_sub_command():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "kmerust graph <INDEX> [-m <MIN_COUNT>] [-f summary|tsv|json] [--sorted]" in p.stdout and "deg_<l>_<r>" in p.stdout


def test_refusal_against_a_library_without_the_entry_points(tmp_path):
    """make asan's binary links the stub library, which has no kh_graph_*: the command refuses with a message, clean under ASan + UBSan."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "krust_amd", "host"), "asan"], stdout=subprocess.DEVNULL)
    san = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    for extra in ([], ["-f", "tsv", "--sorted"], ["-f", "json", "-m", "2"]):
        p = subprocess.run([ASAN_BIN, "graph", str(tmp_path / "a.kmix"), *extra], capture_output=True, text=True, timeout=120, env={**os.environ, **san})
        assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        assert p.returncode == 1 and p.stdout == "" and "graph needs a kmerhip library with kh_graph_stats" in p.stderr, p.stderr
    rc, out, err = _run(ASAN_BIN, "graph", "a.kmix", "-f", "fasta", env=san)
    assert rc == 2 and err == "error: invalid value 'fasta' for '--format <FORMAT>'"
