"""CPU side of the per-base abundance feature (kh_profile / `kmerust query <INDEX> --sequences <PATH>`): the ABI's declarations
and exports, the line writer of the command (compiled into tests/profile_lines_check.cpp with a plain g++ and driven with
hand-made profiles), and the command line where no device is needed -- usage errors, the refusal without a GPU, the old
two-argument form, and the sanitizer build's clean refusal."""
import os
import re
import struct
import subprocess
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "krust_amd", "host")
BIN = os.path.join(HOST, "kmerust")
ASAN_BIN = os.path.join(HOST, "kmerust_asan")
NO = 0xFFFFFFFF


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_header_declares_and_libraries_export_the_profile_calls():
    import ctypes as C
    with open(os.path.join(ROOT, "include", "kmerhip.h")) as f:
        h = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    h1 = " ".join(h.split())
    assert "#define KH_PROFILE_NO_WINDOW 0xFFFFFFFFu" in h1
    assert "int kh_profile_device(kh_ctx *ctx, const uint8_t *d_bases, const uint8_t *d_qual, uint64_t n, uint32_t *d_out);" in h1
    assert "int kh_profile(kh_ctx *ctx, const uint8_t *bases, const uint8_t *qual, uint64_t n, uint32_t *out);" in h1
    assert "#define KMERHIP_ABI_VERSION 2" in h1
    import krust_amd
    krust_amd.lib()
    from krust_amd import native
    assert native.PROFILE_NO_WINDOW == 0xFFFFFFFF
    assert {"kh_profile", "kh_profile_device"} <= set(native.SYMBOLS)
    for so in ("libkmerhip.so", "libkmerhip_testing.so"):
        raw = C.CDLL(os.path.join(os.path.dirname(native.LIB_PATH), so))
        assert hasattr(raw, "kh_profile") and hasattr(raw, "kh_profile_device"), so
    assert hasattr(native.DeviceCounter, "profile") and hasattr(native.DeviceCounter, "profile_device")


# ---- the line writer ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def writer(tmp_path_factory):
    exe = tmp_path_factory.mktemp("profile_lines") / "profile_lines_check"
    srcs = [os.path.join(ROOT, "tests", "profile_lines_check.cpp"), os.path.join(HOST, "kmerust_host.cpp"),
            os.path.join(ROOT, "tests", "host_asan", "stub_kmerhip.cpp")]
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), *srcs, "-lz", "-pthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(k, fmt, first, bases, prof):
        assert len(bases) == len(prof)
        case = f"{k} {fmt} {first} {bases.hex() or '-'} {','.join(str(v) for v in prof) or '-'}\n"
        r = subprocess.run([str(exe)], input=case, capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "PROFILE_LINES_CHECK_DONE" and len(lines) == 2 and not lines[0].startswith("ERR"), lines
        n, hx = lines[0].split()
        return int(n), (b"" if hx == "-" else bytes.fromhex(hx))
    return run


def _profile_of(recs, k, values):
    """A hand-made profile of the flat form of recs: values[r][i] for window start i of record r, NO_WINDOW elsewhere."""
    bases, prof = b"", []
    for r, vals in zip(recs, values):
        starts = max(len(r) - k + 1, 0)
        assert len(vals) == starts
        bases += r + b"\n"
        prof += list(vals) + [NO] * (len(r) + 1 - starts)
    return bases, prof


def test_line_writer_both_formats(writer):
    k = 3
    recs = [b"ACGTAC", b"AC", b"", b"ACNGTAC", b"GGGG", b"TTT"]
    values = [[5, 0, 7, 2], [], [], [NO, NO, NO, NO, 9], [NO, NO], [0xFFFFFFFE]]
    bases, prof = _profile_of(recs, k, values)
    n, out = writer(k, "profile", 0, bases, prof)
    assert n == 6
    assert out == b"5 0 7 2\n\n\n- - - - 9\n- -\n4294967294\n"
    n, out = writer(k, "summary", 0, bases, prof)
    assert n == 6
    assert out == (b"0\t4\t3\t0\t7\t14\n"      # windows, present, min, max, sum
                   b"1\t0\t0\t0\t0\t0\n"        # shorter than k
                   b"2\t0\t0\t0\t0\t0\n"        # empty
                   b"3\t1\t1\t9\t9\t9\n"
                   b"4\t0\t0\t0\t0\t0\n"        # all NO_WINDOW
                   b"5\t1\t1\t4294967294\t4294967294\t4294967294\n")   # a saturated entry
    # the sum is a u64: four saturated windows
    bases, prof = _profile_of([b"ACGTAC"], k, [[0xFFFFFFFE] * 4])
    assert writer(k, "summary", 7, bases, prof) == (1, b"7\t4\t4\t4294967294\t4294967294\t17179869176\n")
    assert writer(k, "summary", 0, b"", []) == (0, b"")


def test_line_writer_ordinals_continue_across_batches(writer):
    k = 2
    b1, p1 = _profile_of([b"ACG", b"T"], k, [[1, 2], []])
    b2, p2 = _profile_of([b"GG", b"", b"CCC"], k, [[3], [], [0, NO]])
    n1, o1 = writer(k, "summary", 0, b1, p1)
    n2, o2 = writer(k, "summary", n1, b2, p2)
    assert (n1, n2) == (2, 3)
    assert o1 + o2 == b"0\t2\t2\t1\t2\t3\n1\t0\t0\t0\t0\t0\n2\t1\t1\t3\t3\t3\n3\t0\t0\t0\t0\t0\n4\t1\t0\t0\t0\t0\n"
    assert writer(k, "profile", n1, b2, p2) == (3, b"3\n\n0 -\n")


# ---- command line ----------------------------------------------------------------------------------------------------------------
def _kmix(path, k, pairs):
    """A KMIX v1 index as `kmerust --save` writes it (src/index.rs:222-300): magic, version, k, count, pairs, CRC32 of all before it."""
    body = b"KMIX" + struct.pack("<BBQ", 1, k, len(pairs)) + b"".join(struct.pack("<QQ", key, c) for key, c in pairs)
    with open(path, "wb") as f:
        f.write(body + struct.pack("<I", zlib.crc32(body) & 0xFFFFFFFF))


def _run(binary, *args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([binary, *args], capture_output=True, timeout=120, env=e)


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """An index the old form answers from; made by the binary itself where a device is there, else written by hand in the same layout."""
    d = tmp_path_factory.mktemp("idx")
    path = str(d / "simple.kmix")
    pairs = [(0b00011011, 3), (0b00000000, 2)]   # k = 4: ACGT x 3, AAAA x 2
    _kmix(path, 4, pairs)
    r = _run(BIN, "query", path, "ACGT")
    if r.returncode != 0:
        pytest.fail("the hand-written index does not load: " + r.stderr.decode())
    return path


def test_old_query_form_is_unchanged(index):
    r = _run(BIN, "query", index, "ACGT")
    assert (r.returncode, r.stdout, r.stderr) == (0, b"3\n", b"")
    r = _run(BIN, "query", index, "tttt")            # canonical of TTTT is AAAA
    assert (r.returncode, r.stdout) == (0, b"2\n")
    r = _run(BIN, "query", index, "CCCC")
    assert (r.returncode, r.stdout) == (0, b"0\n")
    r = _run(BIN, "query", index, "ACG")
    assert r.returncode == 1 and r.stderr == b"Query error:\n k-mer length mismatch: query has 3 bases, index has k=4\n"
    r = _run(BIN, "query", index)
    assert r.returncode == 2 and b"the following required arguments were not provided: <INDEX> <KMER>" in r.stderr


def test_malformed_invocations_are_usage_errors(index, fixtures_dir):
    fa = os.path.join(fixtures_dir, "simple.fa")
    for args, text in ((["query", index, "--sequences"], b"a value is required for '--sequences <PATH>' but none was supplied"),
                       (["query", index, "--sequences", fa, "-f", "tsv"], b"invalid value 'tsv' for '--format <FORMAT>'\n  [possible values: summary, profile]"),
                       (["query", "--sequences", fa], b"the following required arguments were not provided:\n  <INDEX>"),
                       (["query", index, "--sequences", fa, "--bogus"], b"unexpected argument '--bogus' found"),
                       (["query", index, "--sequences", fa, "-Q", "x"], b"invalid value 'x' for '--min-quality <MIN_QUALITY>'")):
        for binary in (BIN, ASAN_BIN) if os.path.exists(ASAN_BIN) else (BIN,):
            r = _run(binary, *args)
            assert r.returncode == 2 and r.stdout == b"", (args, r)
            assert r.stderr.startswith(b"error: " + text) and r.stderr.endswith(b"\n\nFor more information, try '--help'.\n"), (args, r.stderr)
    r = _run(BIN, "query", index, "--sequences", "/nonexistent/reads.fq")
    assert r.returncode == 1 and r.stderr.endswith(b"Problem with arguments:\n File not found: /nonexistent/reads.fq\n")
    r = _run(BIN, "--help")
    assert b"kmerust query <INDEX> --sequences <PATH>" in r.stdout


def test_without_a_device_the_new_form_refuses_with_the_no_device_text(index, fixtures_dir):
    if not _no_gpu():
        pytest.skip("a GPU is present (tests/test_gpu_profile.py runs the command there)")
    r = _run(BIN, "query", index, "--sequences", os.path.join(fixtures_dir, "simple.fa"), "-q")
    assert r.returncode == 1 and r.stdout == b""
    assert r.stderr == b"Application error:\n kh_create: no usable HIP device\n", r.stderr


def test_sanitizer_build_refuses_the_new_form_cleanly(index, fixtures_dir):
    """Built against the recording stub, which has neither kh_profile nor kh_merge_pairs: a clear message and exit 1, not a
    link error, and no sanitizer report."""
    subprocess.check_call(["make", "-C", HOST, "asan"], stdout=subprocess.DEVNULL)
    for fmt in ("summary", "profile"):
        r = _run(ASAN_BIN, "query", index, "--sequences", os.path.join(fixtures_dir, "simple.fq"), "-Q", "20", "-f", fmt,
                 env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
        assert r.returncode == 1 and r.stdout == b"", r
        assert b"query --sequences needs a kmerhip library with kh_profile" in r.stderr
        assert b"Sanitizer" not in r.stderr and b"runtime error" not in r.stderr, r.stderr[-3000:]
        assert b"output-format: " + fmt.encode() in r.stderr and b"min-quality: 20" in r.stderr
    r = _run(ASAN_BIN, "query", index, "ACGT")
    assert (r.returncode, r.stdout) == (0, b"3\n")
