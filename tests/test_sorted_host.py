"""The host side of `kmerust --sorted` without a device: the two symbols are declared, exported and bound; the N-way merge of the
ranks' sorted lists and the kh_result_copy + host sort fallback (tests/sorted_merge_check.cpp); the flag on the command line, and
-- with the sanitizer build's stub library, which has neither kh_result_sorted nor a text stream -- a whole run through the
fallback route."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
ASAN_BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust_asan")
NEW = ("kh_result_sorted", "kh_result_sorted_device")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_declared_mapped_and_bound():
    from krust_amd import native
    header = re.sub(r"/\*.*?\*/", "", _read("include", "kmerhip.h"), flags=re.S)
    mapfile = _read("krust_amd", "csrc", "kmerhip.map")
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in kmerhip.h"
        assert name in native.SYMBOLS and len(native.SYMBOLS[name][1]) == 6, f"{name} is not in native.SYMBOLS"
        assert re.search(r"pub fn %s\(" % name, _read("bindings", "rust", "src", "lib.rs")), f"{name} is not in the Rust crate"
        assert re.search(r"#pragma weak %s\b" % name, _read("krust_amd", "host", "kmerust_host.cpp")), f"{name} is not weak in the host layer"
    assert re.search(r"global:\s*kh_\*;", mapfile)
    assert int(re.search(r"#define\s+KH_OUT_SORTED\s+(0x[0-9a-fA-F]+)u", header).group(1), 16) == native.KH_OUT_SORTED == 0x100
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header)
    assert callable(native.DeviceCounter.result_sorted) and callable(native.DeviceCounter.result_sorted_device)
    assert not re.search(r"kh_result_sorted", _read("tests", "host_asan", "stub_kmerhip.cpp"))  # the stub is what exercises the fallback


def test_merge_and_fallback(tmp_path):
    exe = str(tmp_path / "sorted_merge_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "sorted_merge_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "sorted_merge_check ok" in p.stdout, p.stdout + p.stderr


def _run(binary, *args, env=None):
    p = subprocess.run([binary, *args], capture_output=True, text=True, env=None if env is None else {**os.environ, **env})
    return p.returncode, p.stdout, (p.stderr.splitlines() or [""])[0]


def test_help_names_the_flag():
    rc, out, _ = _run(BIN, "--help")
    assert rc == 0 and "--sorted" in out and "[--save <SAVE>] [--sorted] [-q]" in out


@pytest.mark.parametrize("args,first", [
    (["5", "x.fa", "--sorted=1"], "error: unexpected argument '--sorted=1' found"),
    (["5", "x.fa", "--sort"], "error: unexpected argument '--sort' found"),
    (["5", "x.fa", "--sorted", "--sortedd"], "error: unexpected argument '--sortedd' found"),
    (["combine", "union", "a.kmix", "b.kmix", "--sorted", "--sorte"], "error: unexpected argument '--sorte' found"),
    (["compare", "a.kmix", "b.kmix", "--sorted"], "error: unexpected argument '--sorted' found"),
    (["query", "a.kmix", "--sequences", "x.fa", "--sorted"], "error: unexpected argument '--sorted' found"),
])
def test_unknown_flags_near_it_still_fail(args, first):
    rc, out, err = _run(BIN, *args)
    assert rc == 2 and out == "" and err == first, (rc, out, err)


def test_sorted_runs_on_the_sanitized_binary(fixtures_dir, tmp_path):
    """make asan's binary: the stub library has no kh_result_sorted and no text stream, so --sorted takes kh_result_copy and the
    host sort; it counts nothing, so the documents are empty ones -- what is checked is that the flag parses, every route runs
    clean under ASan + UBSan and exits 0, and that flags near it still fail as before."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "krust_amd", "host"), "asan"], stdout=subprocess.DEVNULL)
    san = {"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"}
    fa = os.path.join(fixtures_dir, sorted(n for n in os.listdir(fixtures_dir) if n.endswith(".fa"))[0])

    def run(*args):
        p = subprocess.run([ASAN_BIN, *args], capture_output=True, timeout=120, env={**os.environ, **san})
        assert b"AddressSanitizer" not in p.stderr and b"runtime error:" not in p.stderr and b"LeakSanitizer" not in p.stderr, \
            p.stderr[-3000:].decode(errors="replace")
        return p

    for extra, doc in ((["-f", "tsv"], b""), (["-f", "fasta"], b""), (["-f", "json"], b"[]\n"), (["-f", "histogram"], None),
                       (["-f", "tsv", "--devices", "0,0,0"], b""), (["-f", "tsv", "--save", str(tmp_path / "s.kmix")], b"")):
        p = run("5", fa, "--quiet", "--sorted", *extra)
        assert p.returncode == 0, (extra, p.stderr[-2000:])
        plain = run("5", fa, "--quiet", *extra)
        assert plain.returncode == 0 and p.stdout == plain.stdout and (doc is None or p.stdout == doc), (extra, p.stdout[:200])
    p = run("5", fa, "--quiet", "--sorted", "--sortedx")
    assert p.returncode == 2 and p.stderr.splitlines()[0] == b"error: unexpected argument '--sortedx' found"
