"""kh_unitigs_paths* without a device: the reference that tests/test_gpu_paths.py holds the kernels to -- a plain loop over the words of
locate_ref (tests/test_locate_ref.py) --, tried on that file's hand-built graphs, whose answers can be read off the page; the three
properties the header promises (expansion, reverse complement, links) on random reads; the predicate of krust_amd/csrc/paths_bits.h,
compiled by the host compiler, against the Python one; the mirrors of the two entry points and the constants; and the command line,
which this feature does not touch."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import test_locate_ref as R
from krust_amd import native
from test_gpu_unitigs import rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
U64 = np.uint64
NO_WINDOW, ABSENT = native.LOC_NO_WINDOW, native.LOC_ABSENT
NAMES = ("kh_unitigs_paths_device", "kh_unitigs_paths")
STATE, OFFSET, QSTART, QEND = native.RUN_STATE, native.RUN_OFFSET, native.RUN_QSTART, native.RUN_QEND


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def continues(a, b):
    """The header's rule for two consecutive words: both places, one high word, the offset one further in the sign's direction."""
    a, b = int(a), int(b)
    if a >= ABSENT or b >= ABSENT or a >> 32 != b >> 32:
        return False
    la, lb = a & 0xFFFFFFFF, b & 0xFFFFFFFF
    return lb == la - 1 if (a >> 32) & 1 else lb == la + 1


def paths_ref(words, rec_start, n_unitigs=0):
    """(run_start, rows, cover) of kh_unitigs_paths for the words of kh_unitigs_locate and nrec + 1 ascending offsets: a loop over the
    window starts of every record that opens a row at a place which does not continue its predecessor inside the record."""
    W = [int(w) for w in words]
    rs = [int(x) for x in rec_start]
    assert all(a <= b for a, b in zip(rs, rs[1:])) and rs[-1] <= len(W)
    rows, run_start = [], []
    for r in range(len(rs) - 1):
        run_start.append(len(rows))
        for i in range(rs[r], rs[r + 1]):
            if W[i] >= ABSENT:
                continue
            if i > rs[r] and continues(W[i - 1], W[i]):
                rows[-1][QEND] = i + 1 - rs[r]
            else:
                rows.append([W[i] >> 32, W[i] & 0xFFFFFFFF, i - rs[r], i + 1 - rs[r]])
    run_start.append(len(rows))
    cover = np.zeros((n_unitigs, native.COV_WORDS), dtype=U64)
    for st, _, qs, qe in rows:
        if n_unitigs:
            cover[st >> 1, native.COV_WINDOWS] += U64(qe - qs)
            cover[st >> 1, native.COV_RUNS] += U64(1)
    return np.array(run_start, dtype=U64), np.array(rows, dtype=np.uint32).reshape(-1, native.RUN_WORDS), cover


def expand(run_start, rows, rec_start, n):
    """The words the rows stand for, NO_WINDOW wherever no run lies: what expanding every run gives."""
    out = np.full(n, NO_WINDOW, dtype=U64)
    for r in range(len(rec_start) - 1):
        for st, off, qs, qe in rows[int(run_start[r]):int(run_start[r + 1])].tolist():
            for i in range(qs, qe):
                j = off + (i - qs) * (-1 if st & 1 else 1)
                at = int(rec_start[r]) + i
                assert out[at] == U64(NO_WINDOW) and 0 <= j < 1 << 32, "two runs over one window start"
                out[at] = U64((st << 32) | j)
    return out


def places_inside(words, rec_start):
    """The place words of W inside the records, NO_WINDOW elsewhere: what expand() must give."""
    w = np.asarray(words, dtype=U64)
    inside = np.zeros(w.size, dtype=bool)
    inside[int(rec_start[0]):int(rec_start[-1])] = True
    return np.where(inside & native.loc_is_place(w), w, U64(NO_WINDOW))


def mirrored(rows, windows):
    """The rows of one record as the reverse complement of the record has them (no palindromic k-mer among the windows)."""
    out = []
    for st, off, qs, qe in reversed(rows.tolist()):
        last = off + (qe - qs - 1) * (-1 if st & 1 else 1)
        out.append([st ^ 1, last, windows - qe, windows - qs])
    return np.array(out, dtype=np.uint32).reshape(-1, native.RUN_WORDS)


def paths_of(ref, k, read, rec_start=None):
    words = R.locate_ref(ref.rows, ref.bases, k, read)
    rs = [0, len(read)] if rec_start is None else rec_start
    run_start, rows, cover = paths_ref(words, rs, ref.rows.shape[0])
    assert np.array_equal(expand(run_start, rows, rs, len(read)), places_inside(words, rs))
    assert int(cover[:, native.COV_RUNS].sum()) == rows.shape[0] == int(run_start[-1])
    assert int(cover[:, native.COV_WINDOWS].sum()) == int(np.sum(places_inside(words, rs) != U64(NO_WINDOW)))
    return run_start.tolist(), rows.tolist(), words


# ---- the reference on graphs small enough to read -------------------------------------------------------------------------------------------
def test_chain_forwards_is_one_plus_run_and_backwards_one_minus_run():
    k = 5
    ref, _ = R.graph_of([R.CHAIN], k)
    seq = ref.bases
    assert paths_of(ref, k, seq)[:2] == ([0, 1], [[0, 0, 0, 8]])
    assert paths_of(ref, k, rc(seq))[:2] == ([0, 1], [[1, 7, 0, 8]])           # OFFSET = L - 1: a '-' run descends from it


def test_circle_walked_twice_round_breaks_at_every_closing_link():
    k, unit = 4, b"ACGGTC"
    circ = (unit * 3)[:len(unit) + k - 1]
    ref, _ = R.graph_of([circ], k)
    assert int(ref.rows[0, native.UNI_FLAGS]) == native.UNI_CIRCULAR
    read = (unit * 4)[:2 * len(unit) + k - 1 + 3]
    run_start, rows, words = paths_of(ref, k, read)
    f = [x for x in R.fields(words) if not isinstance(x, int)]
    wraps = sum(1 for a, b in zip(f, f[1:]) if abs(a[2] - b[2]) == 5)
    assert wraps in (2, 3) and len(rows) == wraps + 1 and run_start == [0, wraps + 1]
    sign = rows[0][STATE] & 1
    for a, b in zip(rows, rows[1:]):
        assert a[QEND] == b[QSTART] and a[STATE] == b[STATE]                    # the closing link: no gap, the same unitig and sign
        assert b[OFFSET] == (5 if sign else 0) and a[OFFSET] + (a[QEND] - a[QSTART] - 1) * (-1 if sign else 1) == (0 if sign else 5)
    assert rows[0][QSTART] == 0 and rows[-1][QEND] == len(read) - k + 1


def test_fork_is_two_runs_joined_by_a_link():
    k = 5
    stem, a, b = b"GATTACAGG", b"ACATTCG", b"CTGAACT"
    recs = [stem + a, stem + b]
    ref, _ = R.graph_of(recs, k)
    links = set(R.links_of_ref(ref, k))
    ends = []
    for r in recs + [rc(recs[0])]:                                              # (the third walks from a branch back into the stem)
        run_start, rows, _ = paths_of(ref, k, r)
        assert len(rows) == 2 and rows[0][QEND] == rows[1][QSTART] and rows[0][QSTART] == 0 and rows[1][QEND] == len(r) - k + 1
        assert (rows[0][STATE] << 32) | rows[1][STATE] in links
        ends.append(rows[1][STATE] >> 1)
    assert ends[0] != ends[1] and ends[2] not in ends[:2]                       # the two branches, and the stem


def test_homopolymer_every_window_is_a_run_of_its_own():
    k = 3
    ref, _ = R.graph_of([b"AAAAAAA"], k)
    assert paths_of(ref, k, b"AAAAAA")[:2] == ([0, 4], [[0, 0, i, i + 1] for i in range(4)])
    assert paths_of(ref, k, b"TTTTTT")[:2] == ([0, 4], [[1, 0, i, i + 1] for i in range(4)])


def test_an_n_and_a_kmer_below_min_count_split_a_run():
    k = 5
    ref, _ = R.graph_of([R.CHAIN], k)
    seq = ref.bases
    read = seq[:7] + b"N" + seq[3:]
    assert paths_of(ref, k, read)[:2] == ([0, 2], [[0, 0, 0, 3], [0, 3, 8, 13]])   # five window starts without a window between them
    other = {b"A": b"C", b"C": b"A", b"G": b"T", b"T": b"G"}[seq[5:6]]
    mut = seq[:5] + other + seq[6:]
    ref2, _ = R.graph_of([seq, seq, mut], k, mc=2)                             # the k-mers over the substitution are counted once
    assert ref2.bases in (seq, rc(seq))
    run_start, rows, words = paths_of(ref2, k, mut)
    assert R.fields(words)[1:6] == [ABSENT] * 5
    sign = rows[0][STATE] & 1
    assert [r[QSTART:] for r in rows] == [[0, 1], [6, 8]] and [r[OFFSET] for r in rows] == ([7, 1] if sign else [0, 6])
    ref1, _ = R.graph_of([seq, seq, mut], k, mc=1)
    rows1 = paths_of(ref1, k, mut)[1]                                           # at min_count 1 they are nodes: no gap
    assert len(rows1) > 1 and all(a[QEND] == b[QSTART] for a, b in zip(rows1, rows1[1:]))


def test_two_records_cut_a_run_in_two():
    k = 5
    ref, _ = R.graph_of([R.CHAIN], k)
    seq = ref.bases
    assert paths_of(ref, k, seq, [0, 3, len(seq)])[:2] == ([0, 1, 2], [[0, 0, 0, 3], [0, 3, 0, 5]])
    assert paths_of(ref, k, rc(seq), [0, 3, len(seq)])[:2] == ([0, 1, 2], [[1, 7, 0, 3], [1, 4, 0, 5]])


def test_empty_records_records_without_a_window_and_records_that_do_not_cover_the_buffer():
    k = 5
    ref, _ = R.graph_of([R.CHAIN], k)
    seq = ref.bases
    flat = seq + b"N" + seq                                                     # 25 bytes: windows at 0 .. 7 and 13 .. 20
    rs = [1, 1, 4, 4, 9, 13, 20]
    run_start, rows, _ = paths_of(ref, k, flat, rs)
    assert run_start == [0, 0, 1, 1, 2, 2, 3]
    assert rows == [[0, 1, 0, 3], [0, 4, 0, 4], [0, 0, 0, 7]]
    assert paths_of(ref, k, flat, [3, 3])[:2] == ([0, 0], [])
    assert paths_of(ref, k, flat, [25, 25, 25])[:2] == ([0, 0, 0], [])
    assert paths_of(ref, k, b"", [0, 0])[:2] == ([0, 0], [])


# ---- the three properties on random reads ---------------------------------------------------------------------------------------------------
def test_expansion_reverse_complement_and_links_on_random_reads():
    k = 5                                                                       # (odd: no palindromes)
    rng = np.random.default_rng(17)
    genome = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=260))
    reads = []
    for i in range(200):
        m = int(rng.integers(k, 60))
        a = int(rng.integers(0, len(genome) - m))
        r = bytearray(genome[a:a + m])
        for p in np.flatnonzero(rng.random(m) < 0.03):
            r[p] = b"ACGT"[int(rng.integers(0, 4))]
        reads.append(rc(bytes(r)) if i % 2 else bytes(r))
    ref, _ = R.graph_of(reads[:120], k)                                         # (the other eighty meet k-mers that are no nodes)
    links = set(R.links_of_ref(ref, k))
    L = [int(r[native.UNI_KMERS]) for r in ref.rows]
    assert len(L) > 50
    joined = gaps = multi = 0
    for r in reads:
        run_start, rows, words = paths_of(ref, k, r)                            # (expansion: checked inside)
        back = paths_of(ref, k, rc(r))[1]
        assert back == mirrored(np.array(rows, dtype=np.uint32).reshape(-1, 4), len(r) - k + 1).tolist(), r
        multi += len(rows) > 1
        for a, b in zip(rows, rows[1:]):
            assert a[QEND] <= b[QSTART]
            if a[QEND] < b[QSTART]:
                gaps += 1
                continue
            sa, sb = a[STATE] & 1, b[STATE] & 1
            last = a[OFFSET] + (a[QEND] - a[QSTART] - 1) * (-1 if sa else 1)
            assert last == (0 if sa else L[a[STATE] >> 1] - 1) and b[OFFSET] == (L[b[STATE] >> 1] - 1 if sb else 0), (a, b)
            assert (a[STATE] << 32) | b[STATE] in links, (a, b)
            joined += 1
    assert joined > 200 and gaps > 20 and multi > 100, (joined, gaps, multi)


# ---- paths_bits.h through the host compiler ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"]], ids=["plain", "asan-ubsan"])
def test_paths_bits_agree_with_the_python_predicate(tmp_path, flags):
    exe = str(tmp_path / "paths_bits_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", *flags, "-o", exe, os.path.join(ROOT, "tests", "paths_bits_check.cpp")],
                   check=True)
    p = subprocess.run([exe], capture_output=True, text=True,
                       env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0:exitcode=97", "UBSAN_OPTIONS": "print_stacktrace=1:halt_on_error=1"})
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout[-2000:] + p.stderr
    lines = p.stdout.splitlines()
    assert lines[-1] == "paths_bits_check ok %d" % (len(lines) - 1) and len(lines) - 1 == 90 * 90 + 8000
    yes = 0
    for line in lines[:-1]:
        a, b, cont, place, state, offset = (int(x) for x in line.split())
        assert cont == int(continues(a, b)) and place == int(a < ABSENT) and (state, offset) == (a >> 32, a & 0xFFFFFFFF), line
        yes += cont
    assert 1500 < yes < 2600                                                    # both answers, often


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------------
def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_declared_mapped_and_bound():
    raw = _read("include", "kmerhip.h")
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    mapfile, rust, integ = _read("krust_amd", "csrc", "kmerhip.map"), _read("bindings", "rust", "src", "lib.rs"), _read("INTEGRATION.md")
    sig = (r"\bint\s+%s\s*\(kh_ctx \*ctx, const uint8_t \*\w+, const uint8_t \*\w+, uint64_t n, const uint64_t \*\w+,\s*uint64_t nrec, "
           r"uint64_t \*\w+, uint32_t \*\w+, uint64_t run_cap, uint64_t \*\w+, uint64_t \*n_runs\)")
    for name in NAMES:
        assert re.search(sig % name, header), name
        assert name in mapfile and re.search(r"global:\s*kh_\*;", mapfile)
        assert name in native.SYMBOLS and native.SYMBOLS[name] == native.SYMBOLS[NAMES[0]]
        assert re.search(r"pub fn %s\(" % name, rust) and re.search(r"\bfn %s\(" % name, integ), name
    assert header.index("kh_unitigs_locate(") < header.index("kh_unitigs_paths_device(") < header.index("kh_clip_tips_into(")   # behind the locate section
    macros = {"RUN_WORDS": 4, "RUN_STATE": 0, "RUN_OFFSET": 1, "RUN_QSTART": 2, "RUN_QEND": 3, "COV_WORDS": 2, "COV_WINDOWS": 0, "COV_RUNS": 1}
    assert {m: int(v) for m, v in re.findall(r"^#define\s+KH_((?:RUN|COV)_\w+)\s+(\d+)\b", raw, flags=re.M)} == macros
    for const, value in macros.items():
        assert getattr(native, const) == value
        assert re.search(r"pub const %s: usize = %d;" % (const, value), rust), const
    assert re.search(r"pub fn unitigs_paths\(", rust)
    assert callable(native.DeviceCounter.unitigs_paths) and callable(native.DeviceCounter.unitigs_paths_device)
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header) and native.ABI_VERSION == 2
    reading = raw[raw.index("Allocation failures"):raw.index("A WRITING call")]
    assert "kh_unitigs_paths / kh_unitigs_paths_device" in reading               # the rule of the reading calls names them
    paths = _read("krust_amd", "csrc", "paths.hip")
    for kernel in ("path_flags_kernel", "path_emit_kernel", "path_cover_kernel"):
        assert re.search(r"\bvoid %s\(" % kernel, paths), kernel
    for name in NAMES:
        assert re.search(r'extern "C" int %s\(' % name, paths)
    make = _read("krust_amd", "csrc", "Makefile")
    assert re.search(r"^SRCS\s*:=.*\bpaths\.hip\b", make, flags=re.M) and "paths_bits.h" in make
    ctx = _read("krust_amd", "csrc", "ctx.hip.h")
    at = ctx.index("// ---- locate.hip")
    assert re.search(r"\bint locate_index\(", ctx[at:]) and re.search(r"\bint locate_range\(", ctx[at:])
    assert len(re.findall(r"\bint locate_index\(kh_ctx", paths + _read("krust_amd", "csrc", "locate.hip"))) == 1   # the one index, not a second copy


def test_the_libraries_export_the_symbols():
    import ctypes as C
    native.lib()
    for so in ("libkmerhip.so", "libkmerhip_testing.so"):
        for name in NAMES:
            assert hasattr(C.CDLL(os.path.join(os.path.dirname(native.LIB_PATH), so)), name), (so, name)


def test_the_command_line_is_untouched():
    """A library feature: --help is the recorded one, byte for byte, and the host layer does not name the entries."""
    with open(os.path.join(ROOT, "tests", "golden", "cli_surface.json")) as f:
        golden = json.load(f)["vectors"][json.dumps(["--help"])]
    p = subprocess.run([BIN, "--help"], stdin=subprocess.DEVNULL, capture_output=True, cwd=ROOT, timeout=60)
    assert {"status": p.returncode, "stdout": p.stdout.decode("latin-1"), "stderr": p.stderr.decode("latin-1")} == golden
    assert "unitigs_paths" not in golden["stdout"] and "run_cap" not in golden["stdout"]
    for f in ("kmerust.cpp", "kmerust_host.cpp", "kmerust_host.h", "cli_args.h"):
        assert "kh_unitigs_paths" not in _read("krust_amd", "host", f), f
