"""kh_unitigs_link_support* without a device: link_support_ref, the plain loop that tests/test_gpu_link_support.py holds the kernel to,
tried on graphs whose answers can be read off the page (tests/test_locate_ref.py builds them from strings); against check_links of
tests/test_gpu_paths.py on the rows of paths_ref; native.link_mirror; support_bits.h through the host compiler; the mirrors of the two
entry points and the constants."""
import os
import re
import subprocess

import numpy as np

import test_locate_ref as R
import test_paths_ref as P
from krust_amd import native
from test_gpu_paths import check_links
from test_gpu_unitigs import rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, U32 = np.uint64, np.uint32
NAMES = ("kh_unitigs_link_support_device", "kh_unitigs_link_support")
STATE, QSTART, QEND = native.RUN_STATE, native.RUN_QSTART, native.RUN_QEND
PAIRS, ADJACENT, CREDITED, MISSING = native.SUP_PAIRS, native.SUP_ADJACENT, native.SUP_CREDITED, native.SUP_MISSING
MASK = (1 << 64) - 1


# ---- the reference ----------------------------------------------------------------------------------------------------------------------
def link_support_ref(run_start, rows, links, support0=None):
    """(support, stats) of kh_unitigs_link_support: per record, every two consecutive rows are a pair; a pair whose QEND equals the next
    QSTART is adjacent; an adjacent pair whose word (STATE_i << 32) | STATE_i+1 is link l adds one to support[l] (modulo 2^64), any
    other is missing.  support0: what the counters hold before."""
    rs = [int(x) for x in run_start]
    rows = np.asarray(rows, dtype=U32).reshape(-1, native.RUN_WORDS).tolist()
    index = {int(w): i for i, w in enumerate(links)}
    assert len(index) == len(links) and all(a <= b for a, b in zip(rs, rs[1:])) and rs[-1] <= len(rows)
    support = [0] * len(index) if support0 is None else [int(x) for x in support0]
    stats = [0, 0, 0, 0]
    for r in range(len(rs) - 1):
        for i in range(rs[r], rs[r + 1] - 1):
            a, b = rows[i], rows[i + 1]
            stats[PAIRS] += 1
            if a[QEND] != b[QSTART]:
                continue
            stats[ADJACENT] += 1
            l = index.get((a[STATE] << 32) | b[STATE])
            if l is None:
                stats[MISSING] += 1
            else:
                stats[CREDITED] += 1
                support[l] = (support[l] + 1) & MASK
    return np.array(support, dtype=U64), np.array(stats, dtype=U64)


class _G:
    def __init__(self, links):
        self.links = links


def rows_of(ref, k, reads):
    """One record per read: (run_start, rows) of paths_ref."""
    flat = b"N".join(reads)
    rs, at = [], 0
    for r in reads:
        rs.append(at)
        at += len(r) + 1
    rs.append(len(flat))
    run_start, rows, _ = P.paths_ref(R.locate_ref(ref.rows, ref.bases, k, flat), rs, ref.rows.shape[0])
    return run_start, rows


# ---- graphs small enough to read ------------------------------------------------------------------------------------------------------------
def test_fork_with_reads_through_either_exit():
    k = 5
    stem, a, b = b"GATTACAGG", b"ACATTCG", b"CTGAACT"
    recs = [stem + a, stem + b]
    ref, _ = R.graph_of(recs, k)
    links = R.links_of_ref(ref, k)
    assert ref.rows.shape[0] == 3 and len(links) == 4                          # stem -> a, stem -> b and their mirrors
    reads = [recs[0], recs[0], recs[1], rc(recs[1])]
    run_start, rows = rows_of(ref, k, reads)
    assert run_start.tolist() == [0, 2, 4, 6, 8]
    support, stats = link_support_ref(run_start, rows, links)
    assert stats.tolist() == [4, 4, 4, 0]
    word = lambda i: (int(rows[i, STATE]) << 32) | int(rows[i + 1, STATE])
    into_a, into_b, back = word(0), word(4), word(6)
    assert word(2) == into_a and into_a != into_b and back == int(native.link_mirror([into_b])[0])
    want = {into_a: 2, into_b: 1, back: 1}
    assert support.tolist() == [want.get(w, 0) for w in links] and 0 in support.tolist()


def test_circle_walked_two_and_a_half_times():
    k, unit = 4, b"ACGGTC"
    ref, _ = R.graph_of([(unit * 3)[:len(unit) + k - 1]], k)
    links = R.links_of_ref(ref, k)
    assert links == [native.uni_link_word(0, 0, 0, 0), native.uni_link_word(0, 1, 0, 1)]
    seq = ref.bases[:len(unit)]                                                # the reported reading: the read starts at offset 0
    read = (seq * 4)[:(5 * len(unit)) // 2 + k - 1]
    for r, want in ((read, [2, 0]), (rc(read), [0, 2])):
        run_start, rows = rows_of(ref, k, [r])
        assert rows.shape[0] == 3
        support, stats = link_support_ref(run_start, rows, links)
        assert support.tolist() == want and stats.tolist() == [2, 2, 2, 0]


def test_the_last_row_of_a_record_never_pairs_with_the_first_of_the_next():
    links = [native.uni_link_word(0, 0, 1, 0)]
    rows = [[0, 0, 0, 5], [2, 0, 5, 9]]                                         # QEND 5 == QSTART 5, and 0+ -> 1+ is a link
    support, stats = link_support_ref([0, 2], rows, links)
    assert support.tolist() == [1] and stats.tolist() == [1, 1, 1, 0]
    support, stats = link_support_ref([0, 1, 2], rows, links)                   # the same rows as two records
    assert support.tolist() == [0] and stats.tolist() == [0, 0, 0, 0]
    support, stats = link_support_ref([0, 1, 1, 2], rows, links)                # ... with an empty record between them
    assert support.tolist() == [0] and stats.tolist() == [0, 0, 0, 0]


def test_a_gap_between_two_runs_is_a_pair_and_not_adjacent():
    links = [native.uni_link_word(0, 0, 1, 0)]
    support, stats = link_support_ref([0, 2], [[0, 0, 0, 5], [2, 0, 6, 9]], links)
    assert support.tolist() == [0] and stats.tolist() == [1, 0, 0, 0]


def test_a_word_that_is_no_link_is_missing():
    links = [native.uni_link_word(0, 0, 1, 0), native.uni_link_word(1, 1, 0, 1)]
    rows = [[0, 0, 0, 5], [3, 0, 5, 9], [0, 0, 9, 12], [2, 0, 12, 13]]          # 0+ -> 1-: no link; 1- -> 0+: no link; 0+ -> 1+: a link
    support, stats = link_support_ref([0, 4], rows, links)
    assert support.tolist() == [1, 0] and stats.tolist() == [3, 3, 1, 2]
    support, stats = link_support_ref([0, 4], rows, links, support0=[MASK, 7])   # added, modulo 2^64
    assert support.tolist() == [0, 7]


# ---- against check_links on the rows of paths_ref ---------------------------------------------------------------------------------------------
def _random_reads(k, seed=17):
    rng = np.random.default_rng(seed)
    genome = bytes(b"ACGT"[i] for i in rng.integers(0, 4, size=260))
    reads = []
    for i in range(200):
        m = int(rng.integers(k, 60))
        a = int(rng.integers(0, len(genome) - m))
        r = bytearray(genome[a:a + m])
        for p in np.flatnonzero(rng.random(m) < 0.03):
            r[p] = b"ACGT"[int(rng.integers(0, 4))]
        reads.append(rc(bytes(r)) if i % 2 else bytes(r))
    return reads


def test_credited_is_what_check_links_counts_and_nothing_is_missing():
    k = 5
    reads = _random_reads(k)
    ref, _ = R.graph_of(reads[:120], k)
    links = np.array(R.links_of_ref(ref, k), dtype=U64)
    run_start, rows = rows_of(ref, k, reads)
    support, stats = link_support_ref(run_start, rows, links)
    joined = check_links(rows, run_start, _G(links))
    assert joined > 200 and int(stats[CREDITED]) == joined == int(support.sum()) and int(stats[MISSING]) == 0
    assert int(stats[PAIRS]) > int(stats[ADJACENT]) == joined                   # some pairs have a gap
    assert (support >= 2).any() and (support == 0).any()
    back = rows_of(ref, k, [rc(r) for r in reads])                              # the strand property: the mirror words are credited
    mirrored, _ = link_support_ref(back[0], back[1], links)
    where = {int(w): i for i, w in enumerate(links)}
    perm = [where[int(w)] for w in native.link_mirror(links)]
    assert np.array_equal(mirrored, support[perm])


def test_link_mirror_is_an_involution_and_stays_in_the_list():
    k = 5                                                                       # (odd: no palindromic unitig, whose sign counts as either)
    ref, _ = R.graph_of(_random_reads(k)[:120], k)
    links = np.array(R.links_of_ref(ref, k), dtype=U64)
    m = native.link_mirror(links)
    assert m.dtype == U64 and links.size > 50
    assert np.array_equal(native.link_mirror(m), links)
    assert set(m.tolist()) == set(links.tolist())
    assert int(native.link_mirror([native.uni_link_word(3, 0, 7, 1)])[0]) == native.uni_link_word(7, 0, 3, 1)


# ---- support_bits.h through the host compiler -------------------------------------------------------------------------------------------------
CHECK = r"""
#include <cstdio>
#include "support_bits.h"
int main() {
    unsigned long long x = 88172645463325252ull;
    int n = 0;
    for (int i = 0; i < 4000; ++i) {
        x ^= x << 13; x ^= x >> 7; x ^= x << 17;
        const uint32_t a = (uint32_t)(x >> 32) >> (i % 3 ? 20 : 0), b = (uint32_t)x >> (i % 5 ? 22 : 0);
        const uint64_t w = kh_sup_word(a, b);
        printf("%u %u %llu %llu %d\n", a, b, (unsigned long long)w, (unsigned long long)kh_sup_mirror(w), kh_sup_adjacent(a, i % 2 ? a : b));
        ++n;
    }
    printf("support_bits_check ok %d\n", n);
    return 0;
}
"""


def test_support_bits_agree_with_the_python_helpers(tmp_path):
    src, exe = tmp_path / "support_bits_check.cpp", str(tmp_path / "support_bits_check")
    src.write_text(CHECK)
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-I", os.path.join(ROOT, "krust_amd", "csrc"), "-o", exe, str(src)], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stdout[-2000:] + p.stderr
    lines = p.stdout.splitlines()
    assert lines[-1] == "support_bits_check ok 4000" and len(lines) == 4001
    for i, line in enumerate(lines[:-1]):
        a, b, w, m, adj = (int(x) for x in line.split())
        assert w == (a << 32) | b and m == int(native.link_mirror([w])[0]) and adj == int(i % 2 == 1 or a == b), line


# ---- the mirrors ------------------------------------------------------------------------------------------------------------------------------
def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_declared_mapped_and_bound():
    raw = _read("include", "kmerhip.h")
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    mapfile, rust, integ = _read("krust_amd", "csrc", "kmerhip.map"), _read("bindings", "rust", "src", "lib.rs"), _read("INTEGRATION.md")
    sig = (r"\bint\s+%s\s*\(kh_ctx \*ctx, const uint64_t \*\w+, uint64_t nrec, const uint32_t \*\w+, uint64_t n_runs,\s*"
           r"uint64_t \*\w+, uint64_t cap, uint64_t \*out\s*\)")
    for name in NAMES:
        assert re.search(sig % name, header), name
        assert name in mapfile and name in native.SYMBOLS and native.SYMBOLS[name] == native.SYMBOLS[NAMES[0]]
        assert re.search(r"pub fn %s\(" % name, rust) and re.search(r"\bfn %s\(" % name, integ), name
    assert header.index("kh_unitigs_paths(") < header.index("kh_unitigs_link_support_device(") < header.index("kh_clip_tips_into(")
    macros = {"SUP_WORDS": 4, "SUP_PAIRS": 0, "SUP_ADJACENT": 1, "SUP_CREDITED": 2, "SUP_MISSING": 3}
    assert {m: int(v) for m, v in re.findall(r"^#define\s+KH_(SUP_\w+)\s+(\d+)\b", raw, flags=re.M)} == macros
    for const, value in macros.items():
        assert getattr(native, const) == value
        assert re.search(r"pub const %s: usize = %d;" % (const, value), rust), const
    assert re.search(r"pub fn unitigs_link_support\(", rust) and re.search(r"pub const fn link_mirror\(", rust)
    assert callable(native.DeviceCounter.unitigs_link_support) and callable(native.DeviceCounter.unitigs_link_support_device)
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header) and native.ABI_VERSION == 2
    reading = raw[raw.index("Allocation failures"):raw.index("A WRITING call")]
    assert "kh_unitigs_link_support / kh_unitigs_link_support_device" in reading
    unit = _read("krust_amd", "csrc", "support.hip")
    for kernel in ("link_index_kernel", "link_support_kernel"):
        assert re.search(r"\bvoid %s\(" % kernel, unit), kernel
    for name in NAMES:
        assert re.search(r'extern "C" int %s\(' % name, unit)
    make = _read("krust_amd", "csrc", "Makefile")
    assert re.search(r"^SRCS\s*:=.*\bsupport\.hip\b", make, flags=re.M) and "support_bits.h" in make
    assert "locate_index(" not in unit and "un.where" not in unit              # the calls never touch the place map
    import test_gpu_link_support as GS                                           # the tile the GPU tests state is the kernel's
    per = int(re.search(r"constexpr int SUP_PER = (\d+);", unit).group(1))
    assert re.search(r"constexpr int SUP_TILE = BLOCK \* SUP_PER;", unit) and GS.T == 256 * per


def test_the_libraries_export_the_symbols():
    import ctypes as C
    native.lib()
    for so in ("libkmerhip.so", "libkmerhip_testing.so"):
        for name in NAMES:
            assert hasattr(C.CDLL(os.path.join(os.path.dirname(native.LIB_PATH), so)), name), (so, name)
