"""kh_unitigs_locate* without a device: the reference in Python strings that tests/test_gpu_locate.py holds the kernels to, tried on
hand-built graphs whose answers can be read off the page; the word macros of include/kmerhip.h against the Python packer; the mirrors
of the two entry points and the two constants; and the command line, which this feature does not touch.

The reference never sees the library's place map.  It takes rows and bases of unitigs -- here those of the string walk of
tests/test_gpu_unitigs.py (Ref), on the device what kh_unitigs_copy returns, which that file holds to the same walk -- and builds
{Q[j:j+k]: (u, j, 0)}, then setdefault(rc(Q[j:j+k]), (u, j, 1)); every window of the input is looked up in that dict, with the window
rule of kh_profile restated: a window starts at i when the k bytes from i are all in ACGTacgt (and, with qualities and a threshold,
all of at least that quality) and lie inside the buffer."""
import json
import os
import re
import subprocess

import numpy as np

from krust_amd import native
from test_gpu_unitigs import Ref, canon, rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
U64 = np.uint64
NO_WINDOW, ABSENT = native.LOC_NO_WINDOW, native.LOC_ABSENT
NAMES = ("kh_unitigs_locate_device", "kh_unitigs_locate")
VALID = frozenset(b"ACGTacgt")


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def place_dict(rows, bases, k):
    """window string -> (unitig, offset, sign) for every k-mer of every unitig and its reverse complement (a palindrome: +)."""
    b = bases.tobytes() if isinstance(bases, np.ndarray) else bytes(bases)
    places = {}
    for u, row in enumerate(np.asarray(rows, dtype=U64).reshape(-1, native.UNI_WORDS)):
        st, L = int(row[native.UNI_START]), int(row[native.UNI_KMERS])
        for j in range(L):
            w = b[st + j:st + j + k]
            assert len(w) == k and w not in places, (u, j, w)     # every node lies in exactly one unitig exactly once
            places[w] = (u, j, 0)
    for w, (u, j, _) in list(places.items()):
        r = rc(w)
        assert places.setdefault(r, (u, j, 1))[:2] == (u, j), (w, r)   # (its mirror is no other node)
    return places


def window_starts(flat, k, qual=None, minq=None):
    """A bool per byte: kh_profile writes a count there (the window rule of counting)."""
    data = bytes(flat)
    n = len(data)
    good = np.fromiter((c in VALID for c in data), dtype=bool, count=n)
    if qual is not None and minq is not None and minq >= 0:
        good &= np.frombuffer(bytes(qual), dtype=np.uint8) >= min(minq + 33, 255)
    run = np.zeros(n + 1, dtype=np.int64)                      # run[i]: good bytes from i on, without a gap
    for i in range(n - 1, -1, -1):
        run[i] = run[i + 1] + 1 if good[i] else 0
    return run[:n] >= k


def locate_ref(rows, bases, k, flat, qual=None, minq=None, places=None):
    """The n words of kh_unitigs_locate for the flat buffer, from strings."""
    places = place_dict(rows, bases, k) if places is None else places
    data = bytes(flat)
    starts = window_starts(data, k, qual, minq)
    out = np.full(len(data), NO_WINDOW, dtype=U64)
    upper = data.upper()
    for i in np.flatnonzero(starts):
        p = places.get(upper[i:i + k])
        out[i] = U64(ABSENT) if p is None else U64(native.loc_word(p[0], p[2], p[1]))
    return out


def string_counts(records, k):
    """canonical string -> count over the windows of the records (upper case ACGT only: the hand-built inputs)."""
    S = {}
    for r in records:
        for i in range(len(r) - k + 1):
            c = canon(r[i:i + k])
            S[c] = S.get(c, 0) + 1
    return S


def graph_of(records, k, mc=1):
    ref = Ref({s: c for s, c in string_counts(records, k).items() if c >= mc}, k)
    return ref, place_dict(ref.rows, ref.bases, k)


def fields(words):
    """[(unitig, sign, offset) or the special] per word."""
    return [int(w) if int(w) >= ABSENT else (int(w) >> 33, (int(w) >> 32) & 1, int(w) & 0xFFFFFFFF) for w in words]


def check_walk(words, rows, links, k):
    """The rule of the header for every two consecutive places; returns how many pairs crossed a link."""
    L = [int(r[native.UNI_KMERS]) for r in rows]
    linkset = set(int(w) for w in links)
    f, crossed = fields(words), 0
    for a, b in zip(f, f[1:]):
        if isinstance(a, int) or isinstance(b, int):
            continue
        (u, s, j), (v, t, i) = a, b
        if (u, s) == (v, t) and i == (j + 1 if s == 0 else j - 1):
            continue
        assert j == (L[u] - 1 if s == 0 else 0) and i == (0 if t == 0 else L[v] - 1), (a, b)
        assert native.uni_link_word(u, s, v, t) in linkset, (a, b)
        crossed += 1
    return crossed


def links_of_ref(ref, k):
    """The link words of a Ref, from strings: every end state's successors, entered at an end of their unitig."""
    b, rows = ref.bases, ref.rows
    seqs = [b[int(r[0]):int(r[0]) + int(r[1]) + k - 1] for r in rows]
    first = {}
    for u, q in enumerate(seqs):
        first.setdefault(q[:k], (u, 0))                        # (tested first: a palindromic unitig is entered as +)
        first.setdefault(rc(q)[:k], (u, 1))
    out = set()
    for u, q in enumerate(seqs):
        for s, w in ((0, q[-k:]), (1, rc(q)[-k:])):
            for c in (b"A", b"C", b"G", b"T"):
                t = w[1:] + c
                if canon(t) in ref.S:
                    v = first[t]
                    out.add(native.uni_link_word(u, s, v[0], v[1]))
    return sorted(out)


# ---- the reference on graphs small enough to read -------------------------------------------------------------------------------------------
CHAIN = b"ACCGTTGACTAG"   # k = 5: eight k-mers, none twice, none a mirror of another


def test_chain_forwards_and_as_its_reverse_complement():
    k = 5
    ref, places = graph_of([CHAIN], k)
    assert ref.rows.shape[0] == 1 and int(ref.rows[0, native.UNI_KMERS]) == 8
    seq = ref.bases
    assert seq in (CHAIN, rc(CHAIN))
    fwd = fields(locate_ref(ref.rows, ref.bases, k, seq))
    assert fwd[:8] == [(0, 0, j) for j in range(8)] and fwd[8:] == [NO_WINDOW] * 4
    back = fields(locate_ref(ref.rows, ref.bases, k, rc(seq)))
    assert back[:8] == [(0, 1, 7 - j) for j in range(8)] and back[8:] == [NO_WINDOW] * 4


def test_circle_walked_twice_round():
    k, unit = 4, b"ACGGTCA"[:6]                                  # ACGGTC: six k-mers round the circle at k = 4
    circ = (unit * 3)[:len(unit) + k - 1]
    ref, places = graph_of([circ], k)
    assert ref.rows.shape[0] == 1 and int(ref.rows[0, native.UNI_FLAGS]) == native.UNI_CIRCULAR and int(ref.rows[0, native.UNI_KMERS]) == 6
    read = (unit * 4)[:2 * len(unit) + k - 1 + 3]               # twice round and three more
    f = fields(locate_ref(ref.rows, ref.bases, k, read))
    got = [x for x in f if not isinstance(x, int)]
    assert len(got) == len(read) - k + 1 and all(u == 0 for u, _, _ in got)
    s = got[0][1]
    assert all(x[1] == s for x in got)
    for a, b in zip(got, got[1:]):
        assert b[2] == (a[2] + (1 if s == 0 else -1)) % 6      # the offsets wrap L - 1 -> 0 (or 0 -> L - 1)
    wraps = sum(1 for a, b in zip(got, got[1:]) if abs(a[2] - b[2]) == 5)
    assert wraps in (2, 3)                                       # fifteen windows round a circle of six
    assert check_walk(locate_ref(ref.rows, ref.bases, k, read), ref.rows, links_of_ref(ref, k), k) == wraps   # each over the closing link


def test_fork():
    k = 5
    stem, a, b = b"GATTACAGG", b"ACATTCG", b"CTGAACT"
    recs = [stem + a, stem + b]
    ref, places = graph_of(recs, k)
    assert ref.rows.shape[0] == 3
    links = links_of_ref(ref, k)
    for r in recs + [rc(recs[0])]:
        words = locate_ref(ref.rows, ref.bases, k, r)
        assert all(not isinstance(x, int) for x in fields(words)[:len(r) - k + 1])
        assert check_walk(words, ref.rows, links, k) == 1      # one step from the stem into a branch (or back)
    assert len({fields(locate_ref(ref.rows, ref.bases, k, r))[len(r) - k][0] for r in recs}) == 2


def test_palindrome_at_k4():
    k = 4
    ref, places = graph_of([b"ACGT"], k)
    assert places == {b"ACGT": (0, 0, 0)}
    for read in (b"ACGT", rc(b"ACGT"), b"acgt"):
        assert fields(locate_ref(ref.rows, ref.bases, k, read))[0] == (0, 0, 0)   # + both times


def test_homopolymer():
    k = 3
    ref, places = graph_of([b"AAAAAAA"], k)
    assert ref.rows.shape[0] == 1 and int(ref.rows[0, native.UNI_KMERS]) == 1
    assert fields(locate_ref(ref.rows, ref.bases, k, b"AAAAAA"))[:4] == [(0, 0, 0)] * 4
    assert fields(locate_ref(ref.rows, ref.bases, k, b"TTTTTT"))[:4] == [(0, 1, 0)] * 4


def test_n_and_lower_case():
    k = 5
    ref, places = graph_of([CHAIN], k)
    seq = ref.bases
    read = seq[:7].lower() + b"N" + seq[3:]
    f = fields(locate_ref(ref.rows, ref.bases, k, read))
    assert f[:3] == [(0, 0, 0), (0, 0, 1), (0, 0, 2)] and f[3:8] == [NO_WINDOW] * 5
    assert f[8:8 + 5] == [(0, 0, j) for j in range(3, 8)] and f[13:] == [NO_WINDOW] * 4
    assert len(f) == len(read)


def test_a_kmer_below_min_count_is_absent():
    k = 5
    recs = [CHAIN, CHAIN, CHAIN[:8] + b"T"]                      # the third ends in k-mers seen once
    ref, places = graph_of(recs, k, mc=2)
    f = fields(locate_ref(ref.rows, ref.bases, k, recs[2]))
    assert f[:3] != [ABSENT] * 3 and not isinstance(f[0], int)
    assert f[4] == ABSENT                                        # TTGAT: counted once, below min_count
    assert all(x == NO_WINDOW for x in f[5:])
    ref1, _ = graph_of(recs, k, mc=1)
    assert ABSENT not in fields(locate_ref(ref1.rows, ref1.bases, k, recs[2]))


def test_qualities_mask_windows():
    k = 3
    ref, places = graph_of([b"ACGTTGCA"], k)
    qual = bytes([33 + 30] * 4 + [33 + 5] + [33 + 30] * 3)
    starts = window_starts(b"ACGTTGCA", k, qual, 20)
    assert starts.tolist() == [True, True, False, False, False, True, False, False]
    assert window_starts(b"ACGTTGCA", k, qual, None).tolist() == [True] * 6 + [False] * 2


# ---- the header's macros against the Python packer --------------------------------------------------------------------------------------
def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def _macros():
    """name -> (argument or None, body as a Python expression) of the KH_LOC_* macros, read from the header text."""
    header = _read("include", "kmerhip.h")
    out = {}
    for name, arg, body in re.findall(r"^#define\s+(KH_LOC_\w+)(?:\((\w)\))?\s+(.+?)\s*$", header, flags=re.M):
        body = body.replace("~0ull", "0xFFFFFFFFFFFFFFFF").replace("(uint32_t)", "").replace("(uint64_t)", "")
        body = re.sub(r"\b(0x[0-9A-Fa-f]+|\d+)(?:ull|u)\b", r"\1", body)
        out[name] = (arg or None, body)
    return out


def _call(macros, name, w=None):
    arg, body = macros[name]
    for other in macros:
        if macros[other][0] is None:
            body = re.sub(r"\b%s\b" % other, "(%s)" % macros[other][1], body)
    return eval(body, {}, {arg: w} if arg else {})


def test_word_macros_of_the_header():
    m = _macros()
    assert set(m) == {"KH_LOC_NO_WINDOW", "KH_LOC_ABSENT", "KH_LOC_IS_PLACE", "KH_LOC_UNITIG", "KH_LOC_SIGN", "KH_LOC_OFFSET"}
    assert _call(m, "KH_LOC_NO_WINDOW") == NO_WINDOW == 2 ** 64 - 1 and _call(m, "KH_LOC_ABSENT") == ABSENT == 2 ** 64 - 2
    for u, s, j in [(0, 0, 0), (0, 1, 0), (5, 0, 7), (2 ** 31 - 2, 1, 2 ** 32 - 1), (123456, 1, 2 ** 31)]:
        w = native.loc_word(u, s, j)
        assert w < ABSENT and _call(m, "KH_LOC_IS_PLACE", w)
        assert (_call(m, "KH_LOC_UNITIG", w), _call(m, "KH_LOC_SIGN", w), _call(m, "KH_LOC_OFFSET", w)) == (u, s, j)
        cols = native.loc_unpack(np.array([w], dtype=U64))
        assert [int(c[0]) for c in cols] == [u, s, j] and bool(native.loc_is_place([w])[0])
        assert w >> 32 == native.uni_link_word(u, s, 0, 0) >> 32       # the state encoding of a link word's halves
    assert not _call(m, "KH_LOC_IS_PLACE", NO_WINDOW) and not _call(m, "KH_LOC_IS_PLACE", ABSENT)
    assert native.loc_is_place([NO_WINDOW, ABSENT]).tolist() == [False, False]
    bits = _read("krust_amd", "csrc", "locate_bits.h")
    assert re.search(r"KH_HD uint64_t kh_loc_word\(", bits) and re.search(r"KH_HD uint64_t kh_loc_result\(", bits)


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------------
def test_symbols_declared_mapped_and_bound():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "kmerhip.h"), flags=re.S)
    mapfile, rust, integ = _read("krust_amd", "csrc", "kmerhip.map"), _read("bindings", "rust", "src", "lib.rs"), _read("INTEGRATION.md")
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(kh_ctx \*ctx, const uint8_t \*\w+, const uint8_t \*\w+, uint64_t n, uint64_t \*\w+\)" % name, header), name
        assert name in mapfile and re.search(r"global:\s*kh_\*;", mapfile)
        assert name in native.SYMBOLS and native.SYMBOLS[name] == native.SYMBOLS["kh_profile"]
        assert re.search(r"pub fn %s\(" % name, rust) and re.search(r"\bfn %s\(" % name, integ), name
    for const, value in (("LOC_NO_WINDOW", "!0u64"), ("LOC_ABSENT", "!0u64 - 1")):
        assert re.search(r"#define\s+KH_%s\b" % const, header)
        assert re.search(r"pub const %s: u64 = %s;" % (const, re.escape(value)), rust)
    assert re.search(r"pub fn unitigs_locate\(", rust)
    assert callable(native.DeviceCounter.unitigs_locate) and callable(native.DeviceCounter.unitigs_locate_device) and callable(native.loc_unpack)
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header) and native.ABI_VERSION == 2
    locate = _read("krust_amd", "csrc", "locate.hip")
    for kernel in ("locate_index_kernel", "locate_kernel"):
        assert re.search(r"\bvoid %s\(" % kernel, locate), kernel
    for name in NAMES:
        assert re.search(r'extern "C" int %s\(' % name, locate)
    assert "locate.hip" in _read("krust_amd", "csrc", "Makefile")


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
    assert "locate" not in golden["stdout"]
    for f in ("kmerust.cpp", "kmerust_host.cpp", "kmerust_host.h", "cli_args.h"):
        assert "kh_unitigs_locate" not in _read("krust_amd", "host", f), f
