"""kh_graph_stats / kh_graph_masks / kh_graph_masks_device -- the de Bruijn graph degrees of a count table -- against numpy.

Expected values never come from the library.  The node set S is O.OracleMap's counts of the same flat buffer that was pushed (or the
chosen pairs that were merged), thresholded; the masks are the two formulas of include/kmerhip.h in numpy -- eight neighbour key
arrays, np.minimum(forward, reverse) for canon, membership in the sorted S --; the 256 words are np.bincount of those masks."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_join as T
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
ALL = (1 << 64) - 1
MINS = [0, 1, 2, 3, 4, ALL]
STAR_SEED = 5


# ---- expected values: numpy ------------------------------------------------------------------------------------------------
def kmask(k):
    return U64(ALL if k >= 32 else (1 << (2 * k)) - 1)


def np_revcomp(x, k):
    """Reverse complement of packed k-mers (low 2k bits of x), letter by letter."""
    x = np.asarray(x, dtype=U64)
    r = np.zeros_like(x)
    for i in range(k):
        r = (r << U64(2)) | (U64(3) - ((x >> U64(2 * i)) & U64(3)))
    return r


def np_valid(x, k):
    x = np.asarray(x, dtype=U64)
    m = kmask(k)
    return ((x & ~m) == 0) & (x <= np_revcomp(x & m, k))


def np_neighbours(x, k):
    """(8, n): rows 0..3 the right neighbours by A, C, G, T, rows 4..7 the left ones -- canon(s[1:] + c), canon(c + s[:-1])."""
    x = np.asarray(x, dtype=U64)
    m, top = kmask(k), U64(2 * (k - 1))
    r = np_revcomp(x, k)
    out = np.empty((8, x.size), dtype=U64)
    for c in range(4):
        out[c] = np.minimum(((x << U64(2)) | U64(c)) & m, (r >> U64(2)) | (U64(3 - c) << top))
        out[4 + c] = np.minimum((x >> U64(2)) | (U64(c) << top), ((r << U64(2)) | U64(3 - c)) & m)
    return out


def np_masks(words, S, k):
    """The mask of every word against the sorted node set S; 0 for a word that is no canonical key of this k."""
    words = np.asarray(words, dtype=U64)
    S = np.asarray(S, dtype=U64)
    valid = np_valid(words, k)
    nb = np_neighbours(words & kmask(k), k)
    if k <= 12:   # membership by a table over the whole key space
        dense = np.zeros(1 << (2 * k), dtype=bool)
        dense[S] = True
        member = lambda a: dense[a]
    else:
        member = lambda a: np.isin(a, S)
    masks = np.zeros(words.size, dtype=np.uint8)
    for j in range(8):
        masks |= (member(nb[j]).astype(np.uint8) << np.uint8(j))
    return np.where(valid, masks, np.uint8(0)).astype(np.uint8)


def node_set(keys, counts, mc):
    sel = counts >= U64(max(mc, 1))
    return keys[sel], counts[sel]


def np_words(keys, counts, mc, k, masks=None):
    """The KH_GRAPH_WORDS words over the pairs (keys sorted): bincount of the masks of S, |S|, the count sum modulo 2^64."""
    sk, sc = node_set(keys, counts, mc)
    w = np.zeros(native.GRAPH_WORDS, dtype=U64)
    w[:256] = np.bincount(np_masks(sk, sk, k) if masks is None else masks, minlength=256).astype(U64)
    w[native.GRAPH_NODES] = sk.size
    w[native.GRAPH_KMERS] = np.sum(sc, dtype=U64)
    return w


def degree_cells(words):
    cells = np.zeros((5, 5), dtype=np.int64)
    for m in range(256):
        cells[bin(m >> 4).count("1"), bin(m & 15).count("1")] += int(words[m])
    return cells


def revcomp_bytes(s):
    return s[::-1].translate(bytes.maketrans(b"ACGT", b"TGCA"))


# ---- the main input: reads, and 256 stars whose centre i has exactly the neighbours mask value i names ------------------------
def star_records(k, seed=STAR_SEED):
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(256):
        s = bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8))
        s = min(s, revcomp_bytes(s))                                  # the centre's canonical string
        star = [s]
        star += [s[1:] + bytes([b"ACGT"[c]]) for c in range(4) if i & (1 << c)]
        star += [bytes([b"ACGT"[c]]) + s[:-1] for c in range(4) if i & (16 << c)]
        recs += star * (i % 3 + 1)                                    # thresholds cut stars
    return recs


_MAIN = {}


def main_input(k):
    """(flat buffer, sorted keys, counts) of the 2 000 reads and the stars, counted once by the oracle."""
    if k not in _MAIN:
        reads, _ = O.synth_reads(77, 1 << 20, 150, 0, 2000, with_qual=False)
        stars = b"N" + b"N".join(star_records(k)) + b"N"
        stars += b"N" * (-(reads.size + len(stars)) % 302)   # the buffer's midpoint is a read boundary: the "grown" table pushes it in two halves
        flat = np.concatenate((np.asarray(reads), np.frombuffer(stars, dtype=np.uint8)))
        assert flat.size // 2 < reads.size and (flat.size // 2) % 151 == 0
        m = O.OracleMap()
        m.process(flat, k)
        keys, counts = m.arrays()
        _MAIN[k] = (flat, np.asarray(keys, dtype=U64).copy(), np.asarray(counts, dtype=U64).copy())
    return _MAIN[k]


_WORDS = {}


def main_words(k, mc):
    if (k, mc) not in _WORDS:
        _, keys, counts = main_input(k)
        _WORDS[(k, mc)] = np_words(keys, counts, mc, k)
    return _WORDS[(k, mc)]


def check_table(dc, keys, counts, k, mins=MINS):
    """Every check of one table: the words, and the masks aligned with result() and with result_sorted()."""
    for mc in mins:
        sk, sc = node_set(keys, counts, mc)
        smasks = np_masks(sk, sk, k)                  # numpy's masks of S, in ascending key order
        want = np_words(keys, counts, mc, k, smasks)
        got = dc.graph_stats(mc)
        assert got.dtype == U64 and got.size == native.GRAPH_WORDS
        assert np.array_equal(got, want), (mc, np.flatnonzero(got != want)[:8])
        assert int(got[native.GRAPH_NODES]) == sk.size and int(got[native.GRAPH_KMERS]) == int(np.sum(sc, dtype=U64))
        assert int(np.sum(got[:256], dtype=U64)) == int(got[native.GRAPH_NODES])
        for gk, gc in (dc.result(max(mc, 1), sort=False), dc.result_sorted(max(mc, 1))):
            o = np.argsort(gk, kind="stable")
            assert np.array_equal(gk[o], sk) and np.array_equal(gc[o], sc)         # the pairs are S ...
            masks = dc.graph_masks(gk, mc)
            assert masks.dtype == np.uint8 and masks.size == gk.size
            assert np.array_equal(masks[o], smasks), mc                             # ... and the masks line up with them


FORMS = [(21, f) for f in ("wide", "image", "regions3072", "grown")] + [(k, f) for k in (31, 32) for f in ("wide", "regions3072", "grown")]


@pytest.mark.parametrize("k", [21, 31, 32])
def test_the_input_covers_every_mask_and_every_degree_cell(k):
    """Precondition, from the numpy values alone: at min_count 1 all 256 mask values and all 25 (left, right) degree cells occur."""
    w = main_words(k, 1)
    assert (w[:256] > 0).all(), np.flatnonzero(w[:256] == 0)
    assert (degree_cells(w) > 0).all()
    assert int(main_words(k, 2)[native.GRAPH_NODES]) < int(w[native.GRAPH_NODES]) and int(main_words(k, 3)[native.GRAPH_NODES]) > 0   # thresholds cut


@pytest.mark.parametrize("k,form", FORMS, ids=[f"k{k}-{f}" for k, f in FORMS])
def test_table_forms(k, form, monkeypatch):
    flat, keys, counts = main_input(k)
    w = main_words(k, 1)
    assert (w[:256] > 0).all() and (degree_cells(w) > 0).all()
    with T.table(form, k, flat, monkeypatch) as dc:
        before = T.stats_of(dc)
        check_table(dc, keys, counts, k)
        assert T.stats_of(dc) == before   # only read, in the form it was in


# ---- keys that are not nodes, and words that are not keys ------------------------------------------------------------------------
@pytest.mark.parametrize("k,form", [(21, "wide"), (21, "image"), (31, "wide"), (32, "wide")], ids=["k21-wide", "k21-image", "k31-wide", "k32-wide"])
def test_keys_that_are_not_nodes_or_not_keys(k, form, monkeypatch):
    flat, keys, counts = main_input(k)
    rng = np.random.default_rng(9)
    m = kmask(k)
    # absent canonical keys: the neighbours of present keys that the table lacks (every one extends into S), then random ones
    near = np.setdiff1d(np_neighbours(keys, k).reshape(-1), keys)
    cand = (rng.integers(0, 1 << 63, size=100_000, dtype=np.int64).astype(U64) * U64(2) + rng.integers(0, 2, size=100_000).astype(U64)) & m
    far = np.minimum(cand, np_revcomp(cand, k))
    absent = np.concatenate((rng.permutation(near)[:keys.size], far[~np.isin(far, keys)]))
    assert near.size >= keys.size and absent.size > 300_000 and np_valid(absent, k).all() and not np.isin(absent, keys).any()
    nonpal = keys[np_revcomp(keys, k) != keys]
    parts = [np.stack((keys, absent[:keys.size]), axis=1).reshape(-1)]       # absent canonical keys next to present ones
    junk = []
    if k < 32:
        junk.append(keys[:4096] | (U64(1) << U64(2 * k)))                    # a bit at 2k
        junk.append(keys[:4096] | (U64(1) << U64(63)))                       # ... at 63
    if k < 31:
        junk.append(keys[:4096] | (U64(1) << U64(2 * k + 1)))                # ... at 2k + 1
    junk.append(np.full(3, ALL, dtype=U64))                                  # the all-ones word
    junk.append(np_revcomp(nonpal[:4096], k))                                # non-canonical words
    junk = np.concatenate(junk)
    assert not np_valid(junk, k).any()
    parts += [junk, np.full(64 * 5, keys[123], dtype=U64), absent[keys.size:]]   # ... one key in every lane of several waves
    words = np.concatenate(parts)
    assert words.size > 2 * 256 * 1024
    with T.table(form, k, flat, monkeypatch) as dc:
        for mc in (1, 2, ALL):
            sk, _ = node_set(keys, counts, mc)
            want = np_masks(words, sk, k)
            got = dc.graph_masks(words, mc)
            assert np.array_equal(got, want), (mc, np.flatnonzero(got != want)[:8])
            j0 = 2 * keys.size
            assert not got[j0:j0 + junk.size].any()                          # every word that is no key: 0
            if mc == 2:                                                        # present keys below the threshold still extend into S
                below = np.flatnonzero(counts < 2)
                assert below.size > 1000 and got[2 * below].any() and np.array_equal(got[2 * below], np_masks(keys[below], sk, k))
            if mc == 1:
                assert got[1:2 * keys.size:2].all()                            # the absent keys next to present ones all extend into S
        one = dc.graph_masks(keys[77:78], 1)                                   # n = 1
        assert one.size == 1 and one[0] == np_masks(keys[77:78], keys, k)[0]
        L = native.lib()
        assert L.kh_graph_masks(dc._h, None, 0, 1, None) == native.KH_OK      # n = 0 with NULL
        assert L.kh_graph_masks_device(dc._h, None, 0, 1, None) == native.KH_OK
        assert dc.graph_masks(np.empty(0, dtype=U64)).size == 0


# ---- small k, where the arithmetic changes ------------------------------------------------------------------------------------------
def canonical_keys(k):
    x = np.arange(1 << (2 * k), dtype=U64)
    return x[x <= np_revcomp(x, k)]


@pytest.mark.parametrize("which", ["half", "full"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 11])
def test_small_k(k, which):
    rng = np.random.default_rng(100 + k)
    if k == 11:
        if which == "half":
            reads, _ = O.synth_reads(77, 1 << 20, 150, 0, 2000, with_qual=False)   # (255 mask values and 24 cells on the CPU)
            flat = np.concatenate((np.asarray(reads), np.frombuffer(b"N" + b"A" * 11 + b"N", dtype=np.uint8)))
            m = O.OracleMap()
            m.process(flat, k)
            keys, counts = (np.asarray(a, dtype=U64).copy() for a in m.arrays())
        else:
            keys = canonical_keys(k)
            counts = rng.integers(1, 5, size=keys.size).astype(U64)
    else:
        every = canonical_keys(k)
        pal = every[np_revcomp(every, k) == every]
        if which == "half":
            keys = np.union1d(rng.choice(every, size=max(every.size // 2, 1), replace=False), np.concatenate(([0], pal[:1]))).astype(U64)
        else:
            keys = every
        counts = rng.integers(1, 5, size=keys.size).astype(U64)
    hom = np.array([sum(c << (2 * i) for i in range(k)) for c in range(4)], dtype=U64)
    assert np.isin(hom, keys).any()                                              # S holds a homopolymer ...
    if k % 2 == 0:
        assert (np_revcomp(keys, k) == keys).any()                               # ... and at even k a palindrome
    with native.DeviceCounter(k) as dc:
        if k == 11 and which == "half":
            dc.push(flat)
        else:
            dc.merge_pairs(keys, counts)
        check_table(dc, keys, counts, k)
        every = canonical_keys(k) if k < 11 else np.unique(np.concatenate((keys, canonical_keys(k)[::7])))
        for mc in (1, 3):                                                          # keys inside and outside S alike
            sk, _ = node_set(keys, counts, mc)
            assert np.array_equal(dc.graph_masks(every, mc), np_masks(every, sk, k))
        if k == 1 and which == "full":
            w1 = dc.graph_stats(1)                                                     # A and C: every present key is everyone's neighbour
            assert int(w1[0xFF]) == 2 and int(w1[native.GRAPH_NODES]) == 2 and list(dc.graph_masks(np.array([0, 1, 2, 3], dtype=U64), 1)) == [0xFF, 0xFF, 0, 0]


# ---- the device form -----------------------------------------------------------------------------------------------------------------
def test_device_form_alignments_and_canaries():
    import torch
    k = 21
    flat, keys, counts = main_input(k)
    nmax = 2049
    want_all = np_masks(keys[:nmax], keys, k)
    dev = torch.device("cuda:0")
    with native.DeviceCounter(k, device=0) as dc:
        dc.push(flat)
        dc.finish()
        d_keys = torch.from_numpy(keys[:nmax].view(np.int64).copy()).to(dev)
        assert d_keys.data_ptr() % 8 == 0
        raw = torch.empty(64 + 16 + nmax + 64 + 16 + 16, dtype=torch.uint8, device=dev)
        pad = (-raw.data_ptr()) % 16
        for off in range(4):
            for n in (1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 2048, 2049):
                raw.fill_(0xAB)
                torch.cuda.synchronize()
                start = pad + 64 + off
                assert (raw.data_ptr() + start) % 16 == off
                dc.graph_masks_device(d_keys.data_ptr(), n, raw.data_ptr() + start, 1)
                host = raw.cpu().numpy()
                assert np.array_equal(host[start:start + n], want_all[:n]), (off, n)
                assert (host[:start] == 0xAB).all() and (host[start + n:] == 0xAB).all(), (off, n)   # the canaries, and everything else
        # keys at any alignment: the same bytes at 1, 4 and 7 bytes off an 8-byte boundary
        kraw = torch.zeros(8 * nmax + 16, dtype=torch.uint8, device=dev)
        kbytes = torch.from_numpy(keys[:nmax].view(np.uint8).copy()).to(dev)
        for koff in (1, 4, 7):
            kraw[koff:koff + 8 * nmax] = kbytes
            raw.fill_(0xAB)
            torch.cuda.synchronize()
            dc.graph_masks_device(kraw.data_ptr() + koff, 257, raw.data_ptr() + pad + 64 + 1, 1)
            host = raw.cpu().numpy()
            assert np.array_equal(host[pad + 65:pad + 65 + 257], want_all[:257]) and (host[:pad + 65] == 0xAB).all() and (host[pad + 65 + 257:] == 0xAB).all()
        # the masks line up with the pairs result_sorted_device just produced
        n = int(main_words(k, 2)[native.GRAPH_NODES])
        dk = torch.empty(n, dtype=torch.int64, device=dev)
        dcnt = torch.empty(n, dtype=torch.int64, device=dev)
        dm = torch.empty(n, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        assert dc.result_sorted_device(dk.data_ptr(), dcnt.data_ptr(), n, 2) == n
        dc.graph_masks_device(dk, n, dm, 2)
        sk, _ = node_set(keys, counts, 2)
        assert np.array_equal(dk.cpu().numpy().view(U64), sk) and np.array_equal(dm.cpu().numpy(), np_masks(sk, sk, k))


# ---- the reader contract ------------------------------------------------------------------------------------------------------------------
def test_reader_contract(monkeypatch):
    k = 21
    flat, keys, counts = main_input(k)
    with T.table("image", k, flat, monkeypatch) as dc:
        st0 = {f: v for f, v in dc.finish().items() if f in ("distinct", "slot_bytes", "table_slots", "grows", "kmers")}
        r0 = dc.result()
        whole = b"".join(dc.result_text("tsv"))
        # a text stream begun before the calls still delivers the same bytes
        dc.result_text_begin("tsv")
        buf = np.empty(1 << 16, dtype=np.uint8)
        n = dc.result_text_next(buf)
        got = [buf[:n].tobytes()]
        assert 0 < n < len(whole)
        assert np.array_equal(dc.graph_stats(2), main_words(k, 2))
        assert np.array_equal(dc.graph_masks(keys[:5000], 1), np_masks(keys[:5000], keys, k))
        import torch
        dk = torch.from_numpy(keys[:300].view(np.int64).copy()).to("cuda:0")
        dm = torch.zeros(300, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        dc.graph_masks_device(dk, 300, dm, 1)
        assert np.array_equal(dm.cpu().numpy(), np_masks(keys[:300], keys, k))
        while True:
            n = dc.result_text_next(buf)
            if n == 0:
                break
            got.append(buf[:n].tobytes())
        assert b"".join(got) == whole
        st1 = {f: v for f, v in dc.finish().items() if f in st0}
        r1 = dc.result()
        assert st1 == st0 and st1["slot_bytes"] == 8 and np.array_equal(r0[0], r1[0]) and np.array_equal(r0[1], r1[1])
    # a pending push is counted first
    with native.DeviceCounter(k, capacity_hint=3_000_000) as dc:
        dc.push(flat)
        assert np.array_equal(dc.graph_stats(1), main_words(k, 1))
    with native.DeviceCounter(k, capacity_hint=3_000_000) as dc:
        dc.push(flat)
        assert np.array_equal(dc.graph_masks(keys[:1000], 1), np_masks(keys[:1000], keys, k))
    # an empty table: no node, every mask 0
    with native.DeviceCounter(k) as dc:
        assert not dc.graph_stats(1).any() and not dc.graph_masks(keys[:100], 1).any()


def test_refusals():
    k = 21
    flat, keys, counts = main_input(k)
    L = native.lib()
    out = np.zeros(native.GRAPH_WORDS, dtype=U64)
    masks = np.zeros(16, dtype=np.uint8)
    with native.DeviceCounter(k) as sh:
        sh.set_shard(0, 2)
        mine = keys[:64][np.array([native.owner(int(x), k, 2) == 0 for x in keys[:64]])]
        assert mine.size > 0
        sh.merge_pairs(mine, np.ones(mine.size, dtype=U64))
        assert L.kh_graph_stats(sh._h, 1, out.ctypes.data) == native.KH_ERR_STATE
        assert b"shard" in L.kh_last_error(sh._h)
        assert L.kh_graph_masks(sh._h, keys.ctypes.data, 16, 1, masks.ctypes.data) == native.KH_ERR_STATE
        assert L.kh_graph_masks_device(sh._h, keys.ctypes.data, 16, 1, masks.ctypes.data) == native.KH_ERR_STATE   # (refused before a pointer is used)
        assert not out.any() and not masks.any()
        assert sh.finish()["distinct"] == mine.size and np.array_equal(sh.lookup(mine), np.ones(mine.size, dtype=U64))   # usable afterwards
    with native.DeviceCounter(k, capacity_hint=3_000_000) as dc:
        dc.push(flat)
        BAD = native.KH_ERR_BAD_ARG
        assert L.kh_graph_stats(dc._h, 1, None) == BAD
        assert L.kh_graph_masks(dc._h, None, 4, 1, masks.ctypes.data) == BAD and L.kh_graph_masks(dc._h, keys.ctypes.data, 4, 1, None) == BAD
        assert L.kh_graph_masks_device(dc._h, None, 4, 1, masks.ctypes.data) == BAD and L.kh_graph_masks_device(dc._h, keys.ctypes.data, 4, 1, None) == BAD
        assert L.kh_graph_stats(None, 1, out.ctypes.data) == BAD and L.kh_graph_masks(None, keys.ctypes.data, 4, 1, masks.ctypes.data) == BAD
        # no memory for the scratch of 2^40 keys: KH_ERR_OOM, and the context is not poisoned
        assert L.kh_graph_masks(dc._h, keys.ctypes.data, C.c_uint64(1 << 40), 1, masks.ctypes.data) == native.KH_ERR_OOM
        assert np.array_equal(dc.graph_stats(1), main_words(k, 1))   # none of it poisoned the context


def test_product_library_once():
    """The same words on the library as it ships (no test switches): a child process that loads libkmerhip.so."""
    child = r"""
import sys, os
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["KMERHIP_LIB"] = "libkmerhip.so"
import numpy as np, torch
from krust_amd import native
import test_gpu_graph as G
k = 21
flat, keys, counts = G.main_input(k)
with native.DeviceCounter(k, capacity_hint=3_000_000, path="partition") as a, native.DeviceCounter(k, path="direct") as b:
    a.push(flat)
    b.push(flat)
    assert a.finish()["slot_bytes"] == 8 and b.finish()["slot_bytes"] == 16
    for dc in (a, b):
        G.check_table(dc, keys, counts, k, mins=[1, 2])
print("RESULT ok", native.LIB_PATH)
"""
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + child], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout and "libkmerhip.so" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
