"""The host side of kh_clip_tips_into and `kmerust clip` without a device: the symbol is declared, exported, bound and weak in the host
layer; the KH_CLIP_* words of the header agree with the Python and Rust constants; the argument parser, the stop rule of the round loop and
the stderr line on hand-made input (tests/clip_host_check.cpp, also under ASan + UBSan); the usage errors of the sub-command, and its
refusal against the sanitizer build's stub library, which has no kh_clip_tips_into."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
ASAN_BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust_asan")
NAME = "kh_clip_tips_into"
WORDS = ("UNITIGS", "CANDIDATES", "CLIPPED", "CLIPPED_KMERS", "CLIPPED_COUNT", "KEPT_KMERS", "KEPT_COUNT", "LINKS")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbol_declared_mapped_bound_and_weak():
    from krust_amd import native
    header = re.sub(r"/\*.*?\*/", "", _read("include", "kmerhip.h"), flags=re.S)
    mapfile = _read("krust_amd", "csrc", "kmerhip.map")
    assert re.search(r"\bint\s+%s\s*\(" % NAME, header), f"{NAME} is not declared in kmerhip.h"
    assert NAME in mapfile and re.search(r"global:\s*kh_\*;", mapfile)
    assert NAME in native.SYMBOLS and len(native.SYMBOLS[NAME][1]) == 5
    assert re.search(r"pub fn %s\(" % NAME, _read("bindings", "rust", "src", "lib.rs")) and re.search(r"pub fn clip_tips_into\(", _read("bindings", "rust", "src", "lib.rs"))
    assert re.search(r"\bfn %s\(" % NAME, _read("INTEGRATION.md"))
    assert re.search(r"#pragma weak %s\b" % NAME, _read("krust_amd", "host", "kmerust_host.cpp"))
    assert not re.search(NAME, _read("tests", "host_asan", "stub_kmerhip.cpp"))       # the stub is what exercises the refusal
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header) and native.ABI_VERSION == 2
    assert callable(native.DeviceCounter.clip_tips_into)
    assert re.search(r"KH_HD bool kh_clip_beats\(", _read("krust_amd", "csrc", "unitig_bits.h"))
    for kernel in ("clip_candidate_kernel", "clip_decide_kernel", "clip_keep_kernel"):
        assert re.search(r"\bvoid %s\(" % kernel, _read("krust_amd", "csrc", "unitig.hip")), kernel


def test_header_words_agree_with_the_bindings():
    from krust_amd import native
    header = _read("include", "kmerhip.h")
    rust = _read("bindings", "rust", "src", "lib.rs")
    assert int(re.search(r"#define\s+KH_CLIP_WORDS\s+(\d+)", header).group(1)) == native.CLIP_WORDS == len(WORDS) == len(native.CLIP_NAMES)
    assert re.search(r"pub const CLIP_WORDS: usize = 8;", rust)
    for i, w in enumerate(WORDS):
        assert int(re.search(r"#define\s+KH_CLIP_%s\s+(\d+)" % w, header).group(1)) == i == getattr(native, "CLIP_" + w)
        assert native.CLIP_NAMES[i] == w.lower()
        assert re.search(r"pub const CLIP_%s: usize = %d;" % (w, i), rust)


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_parser_stop_rule_and_round_line(tmp_path, flags):
    """The stand-alone check program (its own main, nothing preloaded), plain and under ASan + UBSan."""
    exe = str(tmp_path / "clip_host_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "clip_host_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "clip_host_check ok" in p.stdout and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout + p.stderr


def _run(binary, *args, env=None):
    p = subprocess.run([binary, *args], capture_output=True, text=True, env=None if env is None else {**os.environ, **env})
    return p.returncode, p.stdout, (p.stderr.splitlines() or [""])[0]


@pytest.mark.parametrize("args,first", [
    (["clip"], "error: the following required arguments were not provided:"),
    (["clip", "--rounds", "2"], "error: the following required arguments were not provided:"),
    (["clip", "a.kmix", "b.kmix"], "error: unexpected argument 'b.kmix' found"),
    (["clip", "a.kmix", "-f", "gfa"], "error: invalid value 'gfa' for '--format <FORMAT>'"),
    (["clip", "a.kmix", "-f"], "error: a value is required for '--format <FORMAT>' but none was supplied"),
    (["clip", "a.kmix", "--max-kmers", "x"], "error: invalid value 'x' for '--max-kmers <L>': invalid digit found in string"),
    (["clip", "a.kmix", "--rounds=-1"], "error: invalid value '-1' for '--rounds <R>': invalid digit found in string"),
    (["clip", "a.kmix", "-m", "99999999999999999999"], "error: invalid value '99999999999999999999' for '--min-count <MIN_COUNT>': number too large to fit in target type"),
    (["clip", "a.kmix", "--bubbles"], "error: unexpected argument '--bubbles' found"),
])
def test_usage_errors(args, first):
    rc, out, err = _run(BIN, *args)
    assert rc == 2 and out == "" and err == first, (rc, out, err)


def test_options_parse_up_to_the_index(tmp_path):
    """Every accepted spelling gets as far as opening the index: exit 1 with the loader's message, not a usage error."""
    missing = str(tmp_path / "none.kmix")
    for args in (["clip", missing], ["clip", missing, "-m", "3", "-f", "tsv", "--sorted"], ["clip", "--rounds=0", "--max-kmers", "63", missing, "-q"],
                 ["clip", "--format=histogram", missing, "--save", str(tmp_path / "o.kmix")]):
        p = subprocess.run([BIN, *args], capture_output=True, text=True)
        assert p.returncode == 1 and p.stdout == "" and "Application error:\n clip: " in p.stderr, (args, p.stderr)


def test_help_names_the_sub_command():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert p.returncode == 0
    assert "       kmerust clip <INDEX> [-m <MIN_COUNT>] [--max-kmers <L>] [--rounds <R>] [-f <FORMAT>] [--save <SAVE>] [--sorted] [-q]\n" in p.stdout
    assert "       kmerust gfa <INDEX> [-m <MIN_COUNT>] [-f gfa|summary]\n" in p.stdout      # the old line, byte for byte


def test_refusal_against_a_library_without_the_entry_point(tmp_path):
    """make asan's binary links the stub library, which has no kh_clip_tips_into: the command refuses with a message, clean under
    ASan + UBSan."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "krust_amd", "host"), "asan"], stdout=subprocess.DEVNULL)
    san = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    for extra in ([], ["--rounds", "0"], ["-f", "tsv", "-m", "2", "--sorted"]):
        p = subprocess.run([ASAN_BIN, "clip", str(tmp_path / "a.kmix"), *extra], capture_output=True, text=True, timeout=120, env={**os.environ, **san})
        assert "AddressSanitizer" not in p.stderr and "runtime error:" not in p.stderr and "LeakSanitizer" not in p.stderr, p.stderr[-3000:]
        assert p.returncode == 1 and p.stdout == "" and "clip needs a kmerhip library with kh_clip_tips_into" in p.stderr, p.stderr
    rc, out, err = _run(ASAN_BIN, "clip", "a.kmix", "-f", "gfa", env=san)
    assert rc == 2 and err == "error: invalid value 'gfa' for '--format <FORMAT>'"
