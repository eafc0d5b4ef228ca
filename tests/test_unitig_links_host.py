"""The host side of kh_unitigs_links_* and `kmerust gfa` without a device: the three symbols are declared, exported, bound and weak in
the host layer; the link-word macros of the header agree with the Python helpers; the link word, the enter-sign decision, the GFA
line formatters and the link summary on hand-made input (tests/unitig_links_check.cpp, also under ASan + UBSan); the options of the
sub-command, and its refusal against the sanitizer build's stub library, which has none of the three."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
ASAN_BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust_asan")
NEW = ("kh_unitigs_begin_linked", "kh_unitigs_links_copy_device", "kh_unitigs_links_copy")


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
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header)
    assert [len(native.SYMBOLS[n][1]) for n in NEW] == [5, 3, 3]
    for m in ("unitigs_linked", "unitigs_begin_linked", "unitigs_links_copy", "unitigs_links_copy_device"):
        assert callable(getattr(native.DeviceCounter, m))
    assert re.search(r"pub fn unitigs_linked\(", _read("bindings", "rust", "src", "lib.rs"))
    assert "Unitigs" in _read("krust_amd", "csrc", "ctx.hip.h") and "n_links" in _read("krust_amd", "csrc", "ctx.hip.h")


def _macro(header, name):
    """A one-argument macro of the header as a Python function (its body is C integer arithmetic without side effects)."""
    m = re.search(r"#define\s+%s\(w\)\s+(.*)" % name, header)
    assert m, name
    body = re.sub(r"\((?:uint32_t|uint64_t)\)", "", m.group(1))
    body = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)[uU]?(?:ll|LL)?\b", r"\1", body)
    assert re.fullmatch(r"[\sw()0-9A-Fa-fx>&|+*-]+", body), body
    return lambda w: eval(body, {"__builtins__": {}}, {"w": w})


def test_header_macros_agree_with_the_python_helpers():
    from krust_amd import native
    import numpy as np
    header = _read("include", "kmerhip.h")
    frm, fs, to, ts = (_macro(header, "KH_UNI_LINK_" + n) for n in ("FROM", "FROM_SIGN", "TO", "TO_SIGN"))
    ids = (0, 1, 2, 77, 65535, 65536, 2 ** 30, 2 ** 31 - 3, 2 ** 31 - 2)
    words = []
    for a in ids:
        for b in ids:
            for sa in (0, 1):
                for sb in (0, 1):
                    w = native.uni_link_word(a, sa, b, sb)
                    assert w == ((2 * a + sa) << 32) | (2 * b + sb) and w < 2 ** 64
                    assert (frm(w), fs(w), to(w), ts(w)) == (a, sa, b, sb), (a, sa, b, sb)
                    assert (native.uni_link_from(w), native.uni_link_from_sign(w), native.uni_link_to(w), native.uni_link_to_sign(w)) == (a, sa, b, sb)
                    words.append(w)
    cols = native.uni_link_fields(np.array(words, dtype=np.uint64))
    assert all(c.dtype == np.uint32 for c in cols)
    assert [tuple(int(c[i]) for c in cols) for i in range(len(words))] == [(frm(w), fs(w), to(w), ts(w)) for w in words]
    assert sorted(words) == sorted(words, key=lambda w: (frm(w), fs(w), to(w), ts(w)))      # the word order is the field order


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_link_arithmetic_gfa_lines_and_summary(tmp_path, flags):
    """The stand-alone check program (its own main, nothing preloaded), plain and under ASan + UBSan."""
    exe = str(tmp_path / "unitig_links_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "unitig_links_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "unitig_links_check ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout + p.stderr


def _run(binary, *args, env=None):
    p = subprocess.run([binary, *args], capture_output=True, text=True, env=None if env is None else {**os.environ, **env})
    return p.returncode, p.stdout, (p.stderr.splitlines() or [""])[0]


@pytest.mark.parametrize("args,first", [
    (["gfa"], "error: the following required arguments were not provided:"),
    (["gfa", "-m", "2"], "error: the following required arguments were not provided:"),
    (["gfa", "a.kmix", "b.kmix"], "error: unexpected argument 'b.kmix' found"),
    (["gfa", "a.kmix", "-f", "tsv"], "error: invalid value 'tsv' for '--format <FORMAT>'"),
    (["gfa", "a.kmix", "-f", "fasta"], "error: invalid value 'fasta' for '--format <FORMAT>'"),
    (["gfa", "a.kmix", "-f"], "error: a value is required for '--format <FORMAT>' but none was supplied"),
    (["gfa", "a.kmix", "-m", "x"], "error: invalid value 'x' for '--min-count <MIN_COUNT>': invalid digit found in string"),
    (["gfa", "a.kmix", "--min-count=-1"], "error: invalid value '-1' for '--min-count <MIN_COUNT>': invalid digit found in string"),
    (["gfa", "a.kmix", "--sorted"], "error: unexpected argument '--sorted' found"),
])
def test_usage_errors(args, first):
    rc, out, err = _run(BIN, *args)
    assert rc == 2 and out == "" and err == first, (rc, out, err)


def test_options_parse_up_to_the_index(tmp_path):
    """Every accepted spelling gets as far as opening the index: exit 1 with the loader's message, not a usage error."""
    missing = str(tmp_path / "none.kmix")
    for args in (["gfa", missing], ["gfa", missing, "-m", "3", "-f", "gfa"], ["gfa", "-fsummary", "--min-count=9223372036854775807", missing],
                 ["gfa", "--format=summary", missing, "-m2"]):
        p = subprocess.run([BIN, *args], capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and p.stderr.startswith("Application error:\n gfa: "), (args, p.stderr)


def test_help_names_the_sub_command():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "       kmerust gfa <INDEX> [-m <MIN_COUNT>] [-f gfa|summary]\n" in p.stdout and "VN:Z:1.0" in p.stdout
    assert "       kmerust unitigs <INDEX> [-m <MIN_COUNT>] [-f fasta|summary]\n" in p.stdout      # the old line, byte for byte


def test_refusal_against_a_library_without_the_entry_points(tmp_path):
    """make asan's binary links the stub library, which has no kh_unitigs_begin_linked: the command refuses with a message, clean under
    ASan + UBSan."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "krust_amd", "host"), "asan"], stdout=subprocess.DEVNULL)
    san = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    for extra in ([], ["-f", "summary"], ["-f", "gfa", "-m", "2"]):
        p = subprocess.run([ASAN_BIN, "gfa", str(tmp_path / "a.kmix"), *extra], capture_output=True, text=True, timeout=120, env={**os.environ, **san})
        assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        assert p.returncode == 1 and p.stdout == "" and "gfa needs a kmerhip library with kh_unitigs_begin_linked" in p.stderr, p.stderr
    rc, out, err = _run(ASAN_BIN, "gfa", "a.kmix", "-f", "tsv", env=san)
    assert rc == 2 and err == "error: invalid value 'tsv' for '--format <FORMAT>'"
