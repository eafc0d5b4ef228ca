"""CPU side of `kmerust filter` and of the device summary of `kmerust query --sequences`: the keep rule from hand-made rows of
kh_profile_records, the record writer, the summary lines from rows, the reader with headers on the committed fixtures
(tests/filter_check.cpp, compiled with the host library's source and the recording kh_* stub by a plain g++), and the command
line where no device is needed."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "krust_amd", "host")
BIN = os.path.join(HOST, "kmerust")
SAT = 0xFFFFFFFE
NONE = 0xFFFFFFFF


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = tmp_path_factory.mktemp("filter_check") / "filter_check"
    srcs = [os.path.join(ROOT, "tests", "filter_check.cpp"), os.path.join(HOST, "kmerust_host.cpp"),
            os.path.join(ROOT, "tests", "host_asan", "stub_kmerhip.cpp")]
    r = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-o", str(exe), *srcs, "-lz", "-pthread"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def run(*cases):
        r = subprocess.run([str(exe)], input="".join(c + "\n" for c in cases), capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = r.stdout.splitlines()
        assert lines[-1] == "FILTER_CHECK_DONE" and len(lines) == len(cases) + 1, lines
        return lines[:-1]
    return run


def _hex(b):
    return b.hex() or "-"


def _unhex(s):
    return b"" if s == "-" else bytes.fromhex(s)


def _row(windows, in_range, present=None):
    return ",".join(str(x) for x in (windows, in_range if present is None else present, in_range, 0, 9, 0, 0, NONE))


def test_keep_rule_from_hand_made_rows(check):
    cases = [  # (min_kmers, min_fraction, windows, in_range) -> kept
        ((1, 0.0, 10, 1), 1), ((1, 0.0, 10, 0), 0),
        ((1, 0.0, 0, 0), 0), ((0, 0.0, 0, 0), 0),          # windows == 0 is never kept, whatever N and F
        ((0, 0.0, 5, 0), 1),
        ((3, 0.0, 10, 2), 0), ((3, 0.0, 10, 3), 1),
        ((1, 0.5, 10, 5), 1), ((1, 0.5, 10, 4), 0),        # the F * windows tie is kept
        ((1, 0.5, 9, 5), 1), ((1, 0.5, 9, 4), 0),
        ((1, 1.0, 130, 130), 1), ((1, 1.0, 130, 129), 0),
        ((6, 0.5, 10, 5), 0),                              # both conditions
        ((1, 0.25, 4096, 1024), 1), ((1, 0.25, 4096, 1023), 0),
    ]
    got = check(*[f"keep 1 {SAT} {n} {f} {_row(w, r)}" for (n, f, w, r), _ in cases])
    assert [int(g) for g in got] == [want for _, want in cases]
    # only windows and in_range decide: present, min, max, sum and first_low do not
    assert check(f"keep 2 5 1 0 7,7,0,3,9,50,1,0", f"keep 2 5 1 0 7,0,1,0,0,0,0,{NONE}") == ["0", "1"]


def test_record_writer_fasta_and_fastq(check):
    got = check(f"record {_hex(b'seq1 some text')} {_hex(b'ACGTacgtN')} -",
                f"record {_hex(b'r/1')} {_hex(b'ACGTN')} {_hex(b'II#I~')}",
                "record - - -",
                f"record {_hex(b'e')} - {_hex(b'')}")
    assert _unhex(got[0]) == b">seq1 some text\nACGTacgtN\n"
    assert _unhex(got[1]) == b"@r/1\nACGTN\n+\nII#I~\n"
    assert _unhex(got[2]) == b">\n\n"
    assert _unhex(got[3]) == b">e\n\n"      # (no quality pointer: FASTA)


def test_record_starts_and_summary_lines(check):
    got = check(f"starts {_hex(b'ACGT' + bytes([10]) + bytes([10]) + b'GG' + bytes([10]))}", f"starts {_hex(b'AC' + bytes([10]) + b'G')}", "starts -",
                f"summary 7 4,3,0,0,7,14,0,{NONE},0,0,0,0,0,0,0,{NONE},4,4,4,{SAT},{SAT},{(4 * SAT) & 0xFFFFFFFF},{(4 * SAT) >> 32},1",
                "summary 0 -")
    assert got[0] == "0,5,6,9" and got[1] == "0,3,4" and got[2] == "0"
    assert _unhex(got[3]) == b"7\t4\t3\t0\t7\t14\n8\t0\t0\t0\t0\t0\n9\t4\t4\t4294967294\t4294967294\t17179869176\n"
    assert _unhex(got[4]) == b""


def _parse_read(line):
    head, *recs = line.split(" |")
    fields = head.split()
    return int(fields[0]), fields[1:], [[_unhex(x) for x in r.split()] for r in recs]


def test_reader_with_headers_on_the_fixtures(check, fixtures_dir):
    fq, fa, wn = (os.path.join(fixtures_dir, f) for f in ("simple.fq", "simple.fa", "with_n.fq"))
    got = check(f"read {fq} auto 0 1", f"read {fq}.gz auto 0 1", f"read {fa} auto 0 1", f"read {wn} auto 1 1",
                f"read {fq} auto 0 0", f"read {fq} auto 1 0", f"read {fa} auto 1 0")
    # FASTQ with the option: headers, sequences and qualities come back, -Q or not
    for line in got[:2]:
        n, batches, recs = _parse_read(line)
        assert n == 2 and batches == ["batch:2:2:17:17"]
        assert recs == [[b"seq1", b"ACGTACGT", b"IIIIIIII"], [b"seq2", b"GATTACA", b"IIIIIII"]]
    n, batches, recs = _parse_read(got[2])
    assert n == 2 and batches == ["batch:2:2:17:0"] and recs == [[b"seq1", b"ACGTACGT"], [b"seq2", b"GATTACA"]]
    n, batches, recs = _parse_read(got[3])
    assert n == 2 and recs == [[b"seq1", b"ACGTNACGT", b"IIIIIIIII"], [b"seq2", b"NNNGATTACANNN", b"IIIIIIIIIIIII"]]
    # without the option a Batch is what it was: no headers, qualities only when asked for (and never for FASTA)
    n, batches, recs = _parse_read(got[4])
    assert n == 2 and batches == ["batch:2:0:17:0"] and recs == [[b"ACGTACGT"], [b"GATTACA"]]
    n, batches, recs = _parse_read(got[5])
    assert batches == ["batch:2:0:17:17"] and recs == [[b"ACGTACGT", b"IIIIIIII"], [b"GATTACA", b"IIIIIII"]]
    n, batches, recs = _parse_read(got[6])
    assert batches == ["batch:2:0:17:0"]


def _run(*args):
    return subprocess.run([BIN, *args], capture_output=True, timeout=120)


def test_filter_usage_errors_and_a_missing_index(fixtures_dir, tmp_path):
    fa = os.path.join(fixtures_dir, "simple.fa")
    idx = str(tmp_path / "missing.kmix")
    for args, text in ((["filter"], b"the following required arguments were not provided:\n  <INDEX>\n  <PATH>"),
                       (["filter", idx], b"the following required arguments were not provided:\n  <PATH>"),
                       (["filter", idx, fa, "extra"], b"unexpected argument 'extra' found"),
                       (["filter", idx, fa, "--bogus"], b"unexpected argument '--bogus' found"),
                       (["filter", idx, fa, "--min-count"], b"a value is required for '--min-count <LO>' but none was supplied"),
                       (["filter", idx, fa, "--min-count", "x"], b"invalid value 'x' for '--min-count <LO>'"),
                       (["filter", idx, fa, "--max-count", "4294967296"], b"invalid value '4294967296' for '--max-count <HI>': number too large"),
                       (["filter", idx, fa, "--min-kmers=-1"], b"invalid value '-1' for '--min-kmers <N>'"),
                       (["filter", idx, fa, "--min-fraction", "half"], b"invalid value 'half' for '--min-fraction <F>': invalid float literal"),
                       (["filter", idx, fa, "--min-fraction", "1.5"], b"invalid value '1.5' for '--min-fraction <F>': must be between 0 and 1"),
                       (["filter", idx, fa, "-i", "bam"], b"invalid value 'bam' for '--input-format <INPUT_FORMAT>'\n  [possible values: auto, fasta, fastq]"),
                       (["filter", idx, fa, "-Q", "x"], b"invalid value 'x' for '--min-quality <MIN_QUALITY>'")):
        r = _run(*args)
        assert r.returncode == 2 and r.stdout == b"", (args, r)
        assert r.stderr.startswith(b"error: " + text) and r.stderr.endswith(b"\n\nFor more information, try '--help'.\n"), (args, r.stderr)
    r = _run("filter", idx, "/nonexistent/reads.fq")
    assert r.returncode == 1 and r.stderr.endswith(b"Problem with arguments:\n File not found: /nonexistent/reads.fq\n")
    # a missing index file: the banner, then the loader's message, exit 1, nothing on stdout
    r = _run("filter", idx, fa, "--min-count", "2", "-v")
    assert r.returncode == 1 and r.stdout == b""
    assert b"index: " + idx.encode() in r.stderr and b"input-format: fasta (auto-detected)" in r.stderr
    assert r.stderr.endswith(b"Application error:\n failed to read index file '" + idx.encode() + b"': No such file or directory\n"), r.stderr
    r = _run("filter", idx, fa, "-q")
    assert r.returncode == 1 and r.stderr == b"Application error:\n failed to read index file '" + idx.encode() + b"': No such file or directory\n"
    r = _run("--help")
    assert b"kmerust filter <INDEX> <PATH>" in r.stdout and b"--min-fraction <F>" in r.stdout
