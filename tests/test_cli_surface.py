"""The command-line surface of `kmerust`, recorded: for every argument vector below whose outcome is decided before anything touches the
device -- usage errors, --help / --version, a missing data file, a missing or malformed index, `query <INDEX> <KMER>` on a hand-made
index, the banner of `query --sequences` / `filter` in front of an index that cannot be read -- exit status, stdout and stderr are the
bytes in tests/golden/cli_surface.json.  That file was written by the binary of the commit BEFORE the commands were moved onto one
argument parser (cli_args.h) -- a6b6a4d, "Tip clipping on the device" --, so the test compares the parser with what it replaced, not
with itself:

    python tests/test_cli_surface.py --record <that commit's krust_amd/host/kmerust>

The one thing that parser changes on purpose, numbers of 20 digits, is not recorded but asserted (NUMBERS and BOUNDED, below).
All paths are relative and the commands run in the repository root, so the banners hold no directory of this checkout."""
import json
import os
import struct
import subprocess
import sys
import zlib

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
GOLDEN = os.path.join(ROOT, "tests", "golden", "cli_surface.json")

FA = "tests/fixtures/simple.fa"
FQ = "tests/fixtures/low_quality.fq"
NO_FA = "tests/fixtures/none.fa"
K7 = "tests/golden/cli_surface_k7.kmix"        # k = 7: GATTACA (9156) 42 times, AAAAAAA (0) 7 times
BAD = "tests/golden/cli_surface_crc.kmix"      # the same with a wrong checksum
NO_IX = "tests/golden/none.kmix"
U64 = "18446744073709551615"                   # 2^64 - 1
OVER = "18446744073709551616"                  # 2^64
NINES = "9" * 20


def kmix(k, pairs, corrupt=False):
    """A KMIX v1 index: magic, version, k, number of pairs, the pairs, CRC32 of all before it."""
    body = b"KMIX" + bytes([1, k]) + struct.pack("<Q", len(pairs)) + b"".join(struct.pack("<QQ", key, c) for key, c in pairs)
    return body + struct.pack("<I", zlib.crc32(body) ^ (1 if corrupt else 0))


COUNT = [
    [], ["--help"], ["-h"], ["--version"], ["-V"], ["5", "-h", "--bogus"], ["--bogus", "-h"], ["-V", "-h"], ["--help=1"],
    ["5", NO_FA], ["5", NO_FA, "-q"], ["32", NO_FA], ["1", NO_FA, "extra"], ["-q"], ["--quiet", "-m", "2"],
    ["0", NO_FA], ["33", NO_FA], ["abc", NO_FA], ["", NO_FA], ["-", NO_FA], ["-5", NO_FA], ["+5", NO_FA], ["5x", NO_FA], ["9999999999999999999", NO_FA],
    [NINES, NO_FA], ["5", NO_FA, "--"], ["5", "--", NO_FA], ["5", NO_FA, "--sorted=1"], ["5", NO_FA, "--quiet=1"], ["5", NO_FA, "-qq"], ["5", NO_FA, "-x"],
    ["5", NO_FA, "--format"], ["5", NO_FA, "-f"], ["5", NO_FA, "-f", "xml"], ["5", NO_FA, "-fxml"], ["5", NO_FA, "--format=xml"], ["5", NO_FA, "-f=json"],
    ["5", NO_FA, "--format="], ["5", NO_FA, "-fjson"], ["5", NO_FA, "-f", "tsv"], ["5", NO_FA, "--format=histogram"], ["5", NO_FA, "--format", "fasta"],
    ["5", NO_FA, "-i"], ["5", NO_FA, "-i", "bam"], ["5", NO_FA, "-ibam"], ["5", NO_FA, "--input-format=FASTA"], ["5", NO_FA, "-ifastq"],
    ["5", NO_FA, "-m"], ["5", NO_FA, "-m", "x"], ["5", NO_FA, "-m", "-1"], ["5", NO_FA, "-m", "+1"], ["5", NO_FA, "-m", "1x"], ["5", NO_FA, "--min-count="],
    ["5", NO_FA, "-m2"], ["5", NO_FA, "--min-count", "9999999999999999999"],
    ["5", NO_FA, "-Q"], ["5", NO_FA, "-Q", "255"], ["5", NO_FA, "-Q", "256"], ["5", NO_FA, "-Q300"], ["5", NO_FA, "--min-quality=q"], ["5", NO_FA, "-Q", "-1"],
    ["5", NO_FA, "--save"], ["5", NO_FA, "--save", "o.kmix"], ["5", NO_FA, "--save=", "--sorted"],
    ["5", NO_FA, "--gpus"], ["5", NO_FA, "--gpus", "0"], ["5", NO_FA, "--gpus", "00"], ["5", NO_FA, "--gpus", "64"], ["5", NO_FA, "--gpus", "65"],
    ["5", NO_FA, "--gpus=two"], ["5", NO_FA, "--devices"], ["5", NO_FA, "--devices", "0,2,5"], ["5", NO_FA, "--devices", "1023"],
    ["5", NO_FA, "--devices", "1024"], ["5", NO_FA, "--devices", "0,"], ["5", NO_FA, "--devices", ",1"], ["5", NO_FA, "--devices=0,x"], ["5", NO_FA, "--devices", ""],
    ["5", NO_FA, "--max-kmers", "3"], ["5", NO_FA, "--sequences", FA], ["5", NO_FA, "-v"], ["5", NO_FA, "-c", "min"], ["5", NO_FA, "--__batch-kb", "4"],
    ["-f", "xml", "--bogus"], ["--bogus", "-f", "xml"], ["5", "-m", "x", "-Q", "999"], ["5", "-Q", "999", "-m", "x"], ["0", "-m", "x"], ["0", "a", "b"],
    ["queryx", NO_FA], ["Query", K7, "GATTACA"], ["__parse"],
]

QUERY = [
    ["query"], ["query", K7], ["query", K7, "GATTACA"], ["query", K7, "tgtaatc"], ["query", K7, "TTTTTTT"], ["query", K7, "ACGTACG"], ["query", K7, "ACGT"],
    ["query", K7, "ACGTNCG"], ["query", K7, "ACGT\tCG"], ["query", K7, "GATTACA", "extra"], ["query", K7, "-q"], ["query", K7, "-"], ["query", "-", "GATTACA"],
    ["query", NO_IX, "GATTACA"], ["query", BAD, "GATTACA"], ["query", FA, "GATTACA"], ["query", "-h"], ["query", "--help", "x"], ["query", K7, "--sequence"],
    ["query", K7, "--sequencesx"], ["query", "--seq", K7],
]

QUERY_SEQUENCES = [
    ["query", NO_IX, "--sequences", FA], ["query", NO_IX, "--sequences=" + FA], ["query", "--sequences", FA, NO_IX], ["query", BAD, "--sequences", FA],
    ["query", NO_IX, "--sequences", FA, "-q"], ["query", NO_IX, "--sequences", FA, "--quiet"], ["query", NO_IX, "--sequences", NO_FA],
    ["query", NO_IX, "--sequences", FA, "-f", "profile"], ["query", NO_IX, "--sequences", FA, "-fsummary"], ["query", NO_IX, "--sequences", FA, "--format=profile"],
    ["query", NO_IX, "--sequences", FA, "-f", "tsv"], ["query", NO_IX, "--sequences", FA, "-f"], ["query", NO_IX, "--sequences", FA, "-i", "fastq"],
    ["query", NO_IX, "--sequences", FA, "-ifasta"], ["query", NO_IX, "--sequences", FA, "--input-format=auto"], ["query", NO_IX, "--sequences", FA, "-i", "bam"],
    ["query", NO_IX, "--sequences", FA, "-Q", "20"], ["query", NO_IX, "--sequences", FQ, "-Q20"], ["query", NO_IX, "--sequences", FQ, "--min-quality=255", "-i", "fasta"],
    ["query", NO_IX, "--sequences", FA, "-Q", "256"], ["query", NO_IX, "--sequences", FA, "-Q", "x"], ["query", NO_IX, "--sequences", FA, "-Q"],
    ["query", NO_IX, "--sequences", FA, "--__batch-kb", "4"], ["query", NO_IX, "--sequences", FA, "--__batch-kb=4194304"],
    ["query", NO_IX, "--sequences", FA, "--__batch-kb", "4194305"], ["query", NO_IX, "--sequences", FA, "--__batch-kb"],
    ["query", "--sequences"], ["query", "--sequences", FA], ["query", "--sequences=" + FA], ["query", "--sequences="], ["query", NO_IX, "--sequences=", "-q"],
    ["query", NO_IX, "--sequences", "-q"], ["query", NO_IX, K7, "--sequences", FA], ["query", NO_IX, "--sequences", FA, "-h"], ["query", NO_IX, "--sequences", FA, "--help"],
    ["query", NO_IX, "--sequences", FA, "-V"], ["query", NO_IX, "--sequences", FA, "--"], ["query", NO_IX, "--sequences", FA, "-5"],
    ["query", NO_IX, "--sequences", FA, "--sorted"], ["query", NO_IX, "--sequences", FA, "-m", "2"], ["query", NO_IX, "--sequences", FA, "--quiet=1"],
    ["query", "-", "--sequences", FA], ["query", "-f", "tsv", "--bogus", "--sequences", FA], ["query", "--bogus", "-f", "tsv", "--sequences", FA],
    ["query", "-Q", "x", "--sequences"], ["query", "--sequences", FA, "-f", "x"], ["query", NO_IX, "--sequences", "-", "-Q", "3"],
]

FILTER = [
    ["filter"], ["filter", NO_IX], ["filter", "-q"], ["filter", NO_IX, "-v"], ["filter", NO_IX, FA], ["filter", NO_IX, FA, "-q"], ["filter", BAD, FA],
    ["filter", NO_IX, NO_FA], ["filter", NO_IX, FA, "extra"], ["filter", "-", FA], ["filter", NO_IX, FA, "-v"], ["filter", NO_IX, FA, "--invert", "--quiet"],
    ["filter", NO_IX, FA, "-i", "fastq"], ["filter", NO_IX, FA, "-ifasta"], ["filter", NO_IX, FA, "--input-format=auto"], ["filter", NO_IX, FA, "-i", "bam"],
    ["filter", NO_IX, FA, "-i"], ["filter", NO_IX, FA, "-Q", "20"], ["filter", NO_IX, FQ, "-Q20"], ["filter", NO_IX, FQ, "--min-quality=0", "-i", "fasta"],
    ["filter", NO_IX, FA, "-Q", "256"], ["filter", NO_IX, FA, "-Q", "1x"], ["filter", NO_IX, FA, "--min-count", "3"], ["filter", NO_IX, FA, "--min-count=4294967295"],
    ["filter", NO_IX, FA, "--min-count", "4294967296"], ["filter", NO_IX, FA, "--min-count", "x"], ["filter", NO_IX, FA, "--min-count"],
    ["filter", NO_IX, FA, "-m", "3"], ["filter", NO_IX, FA, "--max-count", "9"], ["filter", NO_IX, FA, "--max-count=4294967295"],
    ["filter", NO_IX, FA, "--max-count", "4294967296"], ["filter", NO_IX, FA, "--max-count", "-1"], ["filter", NO_IX, FA, "--min-kmers", "5"],
    ["filter", NO_IX, FA, "--min-kmers=9999999999999999999"], ["filter", NO_IX, FA, "--min-kmers", ""], ["filter", NO_IX, FA, "--min-kmers"],
    ["filter", NO_IX, FA, "--min-fraction", "0.5"], ["filter", NO_IX, FA, "--min-fraction=1"], ["filter", NO_IX, FA, "--min-fraction", "1e-3"],
    ["filter", NO_IX, FA, "--min-fraction", "0"], ["filter", NO_IX, FA, "--min-fraction", "1.5"], ["filter", NO_IX, FA, "--min-fraction", "-0.5"],
    ["filter", NO_IX, FA, "--min-fraction", "half"], ["filter", NO_IX, FA, "--min-fraction", ""], ["filter", NO_IX, FA, "--min-fraction", "0.5x"],
    ["filter", NO_IX, FA, "--min-fraction", "nan"], ["filter", NO_IX, FA, "--min-fraction", "1e"], ["filter", NO_IX, FA, "--min-fraction"],
    ["filter", NO_IX, FA, "--__batch-kb", "4"], ["filter", NO_IX, FA, "--__batch-kb", "4194305"], ["filter", NO_IX, FA, "-h"], ["filter", NO_IX, FA, "--help"],
    ["filter", NO_IX, FA, "-V"], ["filter", NO_IX, FA, "--"], ["filter", NO_IX, FA, "-5"], ["filter", NO_IX, FA, "--invert=1"], ["filter", NO_IX, FA, "-f", "tsv"],
    ["filter", NO_IX, "-", "-Q", "3"], ["filter", NO_IX, FA, "--sorted"], ["filter", "--min-count", "x", "--bogus"], ["filter", "--bogus", "--min-count", "x"],
    ["filter", NO_IX, FA, "--min-count", "7", "--max-count", "3", "--min-kmers", "2", "--min-fraction", "0.25", "-v", "-Q", "3"],
]


def two_indexes(cmd, lead):
    """compare (lead = []) and combine (lead = [an operation]) share their options."""
    ok = [cmd, *lead, NO_IX, K7]
    return [
        [cmd], [cmd, *lead, "--quiet"], [cmd, *lead, NO_IX], ok, [cmd, *lead, K7, NO_IX], [cmd, *lead, BAD, K7], [cmd, *lead, K7, BAD], [*ok, "extra"], [*ok, "-q"],
        [*ok, "--quiet"], [cmd, *lead, "-", K7], [cmd, "-q"], [*ok, "--min-count-a", "3"], [*ok, "--min-count-a=3", "--min-count-b", "4"],
        [*ok, "--min-count-b=9999999999999999999"], [*ok, "--min-count-a", "x"], [*ok, "--min-count-b", "-1"], [*ok, "--min-count-a"], [*ok, "--min-count-b="],
        [*ok, "-f", "tsv"], [*ok, "-fjson"], [*ok, "--format=json"], [*ok, "-f", "fasta"], [*ok, "-f", "histogram"], [*ok, "-f", "summary"], [*ok, "-f"],
        [*ok, "-c", "min"], [*ok, "-cmax"], [*ok, "--calc=left"], [*ok, "--calc", "right"], [*ok, "-c", "sum"], [*ok, "-c", "avg"], [*ok, "-c"],
        [*ok, "-m", "2"], [*ok, "-m2"], [*ok, "--min-count=2"], [*ok, "-m", "x"], [*ok, "--save", "o.kmix"], [*ok, "--save=o.kmix"], [*ok, "--save"],
        [*ok, "--sorted"], [*ok, "--sorted=1"], [*ok, "-h"], [*ok, "--help"], [*ok, "-V"], [*ok, "--"], [*ok, "-5"], [*ok, "--quiet=1"], [*ok, "--gpus", "2"],
        [cmd, *lead, "-f", "x", "--bogus"], [cmd, *lead, "--bogus", "-f", "x"],
    ]


COMPARE = two_indexes("compare", [])
COMBINE = two_indexes("combine", ["union"]) + [
    ["combine", "intersect", NO_IX, K7], ["combine", "subtract", NO_IX, K7], ["combine", "count-subtract", NO_IX, K7, "-c", "min"],
    ["combine", "merge", NO_IX, K7], ["combine", "merge"], ["combine", "merge", NO_IX], ["combine", "", NO_IX, K7], ["combine", "-", NO_IX, K7],
    ["combine", NO_IX, K7], ["combine", "merge", NO_IX, K7, "extra"], ["combine", "merge", "--bogus"], ["combine", "merge", "-f", "x"],
    ["combine", "UNION", NO_IX, K7], ["combine", "-q", "union", "-m", "3", NO_IX, "--min-count-a", "2", K7, "--min-count-b", "4", "--save", "o.kmix"],
]


def one_index(cmd, formats, sorted_ok):
    """graph, unitigs, gfa and clip: an index, -m and -f."""
    return [
        [cmd], [cmd, NO_IX], [cmd, BAD], [cmd, FA], [cmd, "-"], [cmd, NO_IX, "extra"], [cmd, "-m", "2"], [cmd, NO_IX, "-m", "2"], [cmd, NO_IX, "-m2"],
        [cmd, "--min-count=2", NO_IX], [cmd, NO_IX, "--min-count", "9999999999999999999"], [cmd, NO_IX, "-m"], [cmd, NO_IX, "-m", "x"], [cmd, NO_IX, "-m", "-1"],
        [cmd, NO_IX, "-m", "+1"], [cmd, NO_IX, "-m", "1x"], [cmd, NO_IX, "--min-count="], [cmd, NO_IX, "-m", ""],
        *[[cmd, NO_IX, "-f", f] for f in formats], [cmd, NO_IX, "-f" + formats[0]], [cmd, NO_IX, "--format=" + formats[-1]], [cmd, NO_IX, "--format", formats[0]],
        [cmd, NO_IX, "-f", "xml"], [cmd, NO_IX, "-f", formats[0].upper()], [cmd, NO_IX, "-f"], [cmd, NO_IX, "--format="], [cmd, NO_IX, "-f=" + formats[0]],
        [cmd, NO_IX, "--sorted"], [cmd, NO_IX, "--sorted=1"], [cmd, NO_IX, "-q"], [cmd, NO_IX, "--quiet"], [cmd, NO_IX, "--quiet=1"], [cmd, NO_IX, "-h"],
        [cmd, NO_IX, "--help"], [cmd, NO_IX, "-V"], [cmd, NO_IX, "--version"], [cmd, NO_IX, "--"], [cmd, "--", NO_IX], [cmd, NO_IX, "-5"], [cmd, NO_IX, "--save", "o.kmix"],
        [cmd, NO_IX, "--rounds", "2"], [cmd, NO_IX, "-i", "fasta"], [cmd, "-f", "xml", "--bogus"], [cmd, "--bogus", "-f", "xml"], [cmd, "-m", "x", "-f", "xml"],
        [cmd, "-f", "xml", "-m", "x"], [cmd, NO_IX, "-m", "3", "-f", formats[-1], *(["--sorted"] if sorted_ok else [])],
    ]


GRAPH = one_index("graph", ["summary", "tsv", "json"], True) + [["graph", NO_IX, "-f", "fasta"], ["graph", NO_IX, "-f", "gfa"]]
UNITIGS = one_index("unitigs", ["fasta", "summary"], False) + [["unitigs", NO_IX, "-f", "tsv"], ["unitigs", NO_IX, "-f", "gfa"]]
GFA = one_index("gfa", ["gfa", "summary"], False) + [["gfa", NO_IX, "-f", "fasta"], ["gfa", NO_IX, "-f", "tsv"]]
CLIP = one_index("clip", ["fasta", "tsv", "json", "histogram"], True) + [
    ["clip", NO_IX, "--max-kmers", "63"], ["clip", NO_IX, "--max-kmers=0"], ["clip", NO_IX, "--max-kmers", "x"], ["clip", NO_IX, "--max-kmers"],
    ["clip", NO_IX, "--max-kmers", U64], ["clip", NO_IX, "--max-kmers", OVER], ["clip", NO_IX, "--rounds", "0"], ["clip", NO_IX, "--rounds=-1"],
    ["clip", NO_IX, "--rounds"], ["clip", NO_IX, "--rounds", NINES], ["clip", NO_IX, "-m", U64], ["clip", NO_IX, "-m", OVER], ["clip", NO_IX, "-m", "0" * 21],
    ["clip", NO_IX, "--save=o.kmix", "-q", "--sorted"], ["clip", NO_IX, "--save"], ["clip", NO_IX, "-f", "gfa"],
]

VECTORS = COUNT + QUERY + QUERY_SEQUENCES + FILTER + COMPARE + COMBINE + GRAPH + UNITIGS + GFA + CLIP

# Numbers of 20 digits: the parser the commands share takes them up to 2^64 - 1 and calls a larger one too large, as `clip` always
# did; the commit that wrote the fixture called both "invalid digit found in string" everywhere but in `clip`.  Not recorded: asserted.
# (arguments, the option as messages name it); the None among the arguments is where the number under test goes.
NUMBERS = [
    (["5", NO_FA, "-m", None], "--min-count <MIN_COUNT>"),
    (["filter", NO_IX, FA, "-q", "--min-kmers", None], "--min-kmers <N>"), (["compare", NO_IX, K7, "-q", "--min-count-a", None], "--min-count-a <N>"),
    (["combine", "union", NO_IX, K7, "-q", "--min-count-b", None], "--min-count-b <N>"), (["combine", "union", NO_IX, K7, "-q", "-m", None], "--min-count <MIN_COUNT>"),
    (["graph", NO_IX, "-m", None], "--min-count <MIN_COUNT>"), (["unitigs", NO_IX, "--min-count", None], "--min-count <MIN_COUNT>"),
    (["gfa", NO_IX, "-m", None], "--min-count <MIN_COUNT>"),
]
BOUNDED = [  # options whose maximum is below 2^64 - 1: every 20-digit number is too large for them
    (["5", NO_FA, "-Q", None], "--min-quality <MIN_QUALITY>"), (["5", NO_FA, "--gpus", None], "--gpus <N>"), (["5", NO_FA, "--devices", None], "--devices <LIST>"),
    (["filter", NO_IX, FA, "--min-count", None], "--min-count <LO>"), (["filter", NO_IX, FA, "--max-count", None], "--max-count <HI>"),
    (["query", NO_IX, "--sequences", FA, "-Q", None], "--min-quality <MIN_QUALITY>"), (["query", NO_IX, "--sequences", FA, "--__batch-kb", None], "--__batch-kb <N>"),
    (["filter", NO_IX, FA, "--__batch-kb", None], "--__batch-kb <N>"),
]


def run(binary, args):
    p = subprocess.run([binary, *args], stdin=subprocess.DEVNULL, capture_output=True, cwd=ROOT, timeout=60)
    return {"status": p.returncode, "stdout": p.stdout.decode("latin-1"), "stderr": p.stderr.decode("latin-1")}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_the_index_fixtures_are_what_the_vectors_take_them_for():
    assert open(os.path.join(ROOT, K7), "rb").read() == kmix(7, [(9156, 42), (0, 7)])
    assert open(os.path.join(ROOT, BAD), "rb").read() == kmix(7, [(9156, 42), (0, 7)], corrupt=True)
    assert not os.path.exists(os.path.join(ROOT, NO_IX)) and not os.path.exists(os.path.join(ROOT, NO_FA))


def test_every_command_has_its_vectors_and_each_is_recorded(golden):
    for name, group in (("count", COUNT), ("query", QUERY), ("query --sequences", QUERY_SEQUENCES), ("filter", FILTER), ("compare", COMPARE),
                        ("combine", COMBINE), ("graph", GRAPH), ("unitigs", UNITIGS), ("gfa", GFA), ("clip", CLIP)):
        assert len(group) >= 15, name
    keys = [json.dumps(v) for v in VECTORS]
    assert len(set(keys)) == len(keys) and set(keys) == set(golden["vectors"])
    statuses = {r["status"] for r in golden["vectors"].values()}
    assert statuses == {0, 1, 2}


@pytest.mark.parametrize("args", VECTORS, ids=lambda v: " ".join(v) or "(none)")
def test_recorded_outcome(golden, args):
    assert run(BIN, args) == golden["vectors"][json.dumps(args)]


@pytest.mark.parametrize("tail,what", NUMBERS, ids=lambda x: " ".join(a or "N" for a in x) if isinstance(x, list) else None)
def test_a_number_of_20_digits(tail, what):
    at = lambda n: run(BIN, [n if a is None else a for a in tail])
    usage = lambda n, why: {"status": 2, "stdout": "", "stderr": f"error: invalid value '{n}' for '{what}': {why}\n\nFor more information, try '--help'.\n"}
    accepted, below = at(U64), at("9999999999999999999")          # 2^64 - 1 gets as far as 19 nines always did: to the file that is not there
    assert accepted["status"] == 1 and accepted["stdout"] == "" and accepted["stderr"] == below["stderr"].replace("9999999999999999999", U64)
    for n in (OVER, NINES):
        assert at(n) == usage(n, "number too large to fit in target type")
    for n in ("", "-1", "+1", "1x", "0" * 21):
        assert at(n) == usage(n, "invalid digit found in string")


@pytest.mark.parametrize("tail,what", BOUNDED, ids=lambda x: " ".join(a or "N" for a in x) if isinstance(x, list) else None)
def test_a_number_of_20_digits_where_the_option_has_a_maximum(tail, what):
    for n in (U64, OVER, NINES):
        r = run(BIN, [n if a is None else a for a in tail])
        assert r == {"status": 2, "stdout": "", "stderr": f"error: invalid value '{n}' for '{what}': number too large to fit in target type\n\nFor more information, try '--help'.\n"}


if __name__ == "__main__":  # --record <binary>: write the fixture from that binary's answers (the index files too)
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_cli_surface.py --record <kmerust binary>"
    for path, corrupt in ((K7, False), (BAD, True)):
        with open(os.path.join(ROOT, path), "wb") as f:
            f.write(kmix(7, [(9156, 42), (0, 7)], corrupt))
    with open(GOLDEN, "w") as f:
        json.dump({"vectors": {json.dumps(v): run(os.path.abspath(sys.argv[2]), v) for v in VECTORS}}, f, indent=0, sort_keys=True)
        f.write("\n")
