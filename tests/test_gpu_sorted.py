"""The device radix sort behind kh_result_sorted / kh_result_sorted_device and KH_OUT_SORTED text streams (krust_amd/csrc/sort.hip,
sort.hip.h, format.hip): the pairs of a table in ascending key order, whatever the table's size, geometry or form.

Expected values are numpy sorts of what this file wrote (wide tables are kh_merge_pairs of chosen canonical keys, as in
tests/test_gpu_readside.py) or of the oracle's counts; equality is exact.  A count is derived from its key by a fixed mix, so
a count that travels with the wrong key is seen.  Output arrays carry canaries on both sides.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_format import empty_doc, ends_at_record_end, record
from test_gpu_readside import CANARY, PAD, _env, _revcomp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
SEED = 20260207
NCPU = max(1, min(os.cpu_count() or 1, 16))
TILE = 4096        # sort.hip.h SORT_TILE: a power of two, so the 2^p +- 1 sizes below are its edges
FORMATS = ("fasta", "tsv", "json")


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import krust_amd
    krust_amd.lib()  # ImportError if the HIP extension is missing: no silent fallback
    return krust_amd


# ---- keys, counts, and the calls with canaries ---------------------------------------------------------------------------
def mix(keys):
    """The count that belongs to a key: 1 .. 2^24, from a fixed multiplicative mix."""
    return ((np.asarray(keys, dtype=U64) * U64(0x9E3779B97F4A7C15)) >> U64(40)) + U64(1)


def canonical_only(keys, k):
    keys = np.unique(np.asarray(keys, dtype=U64))
    return keys[keys <= _revcomp(keys, k)]


def random_keys(k, n, rng):
    """n distinct canonical k-mers (fewer where 4^k has no more), in random order."""
    if 2 * k <= 16:
        keys = canonical_only(np.arange(1 << (2 * k), dtype=U64), k)
    else:
        raw = rng.integers(0, 1 << 64, size=2 * n + 64, dtype=U64) >> U64(64 - 2 * k)
        keys = np.unique(np.minimum(raw, _revcomp(raw, k)))
    keys = keys[rng.permutation(keys.size)[:n]]
    assert keys.size == n or 2 * k <= 16
    return keys


def build(K, k, keys, counts, **kw):
    dc = K.DeviceCounter(k, **kw)
    if keys.size:
        dc.merge_pairs(np.ascontiguousarray(keys), np.ascontiguousarray(counts))
    return dc


def want(keys, counts, mc=1):
    o = np.argsort(keys, kind="stable")
    keys, counts = keys[o], counts[o]
    sel = counts >= U64(max(mc, 1))
    return keys[sel], counts[sel]


def sorted_host(K, dc, cap, mc=1):
    """kh_result_sorted into host arrays of capacity cap between canaries: (rc, n, keys, counts) -- the arrays whole, canaries included."""
    keys = np.full(cap + 2 * PAD, CANARY, dtype=U64)
    cnts = np.full(cap + 2 * PAD, CANARY, dtype=U64)
    n = C.c_uint64(123456789)
    rc = K.lib().kh_result_sorted(dc._h, keys.ctypes.data + 8 * PAD, cnts.ctypes.data + 8 * PAD, cap, mc, C.byref(n))
    return rc, n.value, keys, cnts


def sorted_device(K, dc, cap, mc=1):
    import torch
    dk = torch.full((cap + 2 * PAD,), CANARY, dtype=torch.int64, device="cuda")
    dn = torch.full((cap + 2 * PAD,), CANARY, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    n = C.c_uint64(123456789)
    rc = K.lib().kh_result_sorted_device(dc._h, dk.data_ptr() + 8 * PAD, dn.data_ptr() + 8 * PAD, cap, mc, C.byref(n))
    torch.cuda.synchronize()
    return rc, n.value, dk.cpu().numpy().view(U64), dn.cpu().numpy().view(U64)


def inside(arr, n):
    assert (arr[:PAD] == U64(CANARY)).all() and (arr[PAD + n:] == U64(CANARY)).all(), "written outside the first n entries"
    return arr[PAD:PAD + n]


def check_both_forms(K, dc, wk, wc, mc=1):
    """Host and device form with cap == size: exactly the expected arrays, nothing outside them."""
    need = wk.size
    assert dc.result_size(mc) == need
    for call in (sorted_host, sorted_device):
        rc, n, gk, gc = call(K, dc, need, mc)
        assert rc == K.native.KH_OK and n == need, (call.__name__, rc, n, need)
        gk, gc = inside(gk, need), inside(gc, need)
        bad = np.flatnonzero((gk != wk) | (gc != wc))
        assert bad.size == 0, (call.__name__, need, bad[:5], [hex(int(x)) for x in gk[bad[:5]]], [hex(int(x)) for x in wk[bad[:5]]])


# ---- sizes ----------------------------------------------------------------------------------------------------------------
SIZES = [0, 1, 2, 63, 64, 65] + [s for p in range(8, 18) for s in ((1 << p) - 1, 1 << p, (1 << p) + 1, 3 * (1 << p) + 5)]


def test_sizes_at_k21(K):
    """Every size on one context (kh_reset between them): below a wave, the tile's edges (2^12 +- 1), several tiles, tile counts
    that are no multiple of anything."""
    assert TILE - 1 in SIZES and TILE in SIZES and TILE + 1 in SIZES
    rng = np.random.default_rng(SEED)
    pool = random_keys(21, max(SIZES), rng)
    with K.DeviceCounter(21) as dc:
        for n in SIZES:
            dc.reset()
            keys = pool[rng.permutation(pool.size)[:n]]
            counts = mix(keys)
            if n:
                dc.merge_pairs(keys, counts)
            check_both_forms(K, dc, *want(keys, counts))


# ---- key widths -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 5, 16, 31, 32])
def test_key_widths(K, k):
    """2k <= 8 (k = 1: both canonical keys; k = 4: one whole digit), 2k no multiple of the digit (k = 5: 8 + 2 bits; k = 31: 7 x 8 + 6),
    32 bits, and k = 32 with the top bit set."""
    rng = np.random.default_rng(SEED + k)
    keys = random_keys(k, 30_000, rng)
    if k == 1:
        assert sorted(keys.tolist()) == [0, 1]  # A and C (G and T are their reverse complements)
    if k == 32:  # k-mers that start with G and end with C are canonical and >= 2^63
        raw = rng.integers(0, 1 << 64, size=20_000, dtype=U64)
        g_c = (raw & ~(U64(3) << U64(62)) & ~U64(3)) | (U64(2) << U64(62)) | U64(1)
        g_c = canonical_only(g_c, 32)
        assert g_c.size > 5000 and int(g_c.min()) >= 1 << 63
        keys = np.unique(np.concatenate([keys, g_c]))
        keys = keys[rng.permutation(keys.size)]
    counts = mix(keys)
    with build(K, k, keys, counts) as dc:
        check_both_forms(K, dc, *want(keys, counts))


# ---- key patterns ---------------------------------------------------------------------------------------------------------
def _patterns():
    """name -> keys (k = 31, canonical), in insertion order.  A k-mer that starts with A and does not end with T is canonical:
    its reverse complement starts with C, G or T."""
    k = 31
    rng = np.random.default_rng(SEED + 100)
    rand = random_keys(k, 70_000, rng)
    out = {"ascending": np.sort(rand), "descending": np.sort(rand)[::-1].copy(), "random": rand}
    base = U64((int(rng.integers(0, 1 << 60)) & ~3) | 1)  # first base A, last base C

    def vary(shift, bits):
        v = np.arange(1 << bits, dtype=U64) << U64(shift)
        return canonical_only((base & ~(U64((1 << bits) - 1) << U64(shift))) | v, k)

    out["lowest-digit-only"] = vary(0, 8)         # (the keys that end with T and lose against their reverse complement drop out)
    out["highest-digit-only"] = vary(56, 6)       # pass 7 takes the 6 bits 56 .. 61
    out["one-middle-digit-only"] = vary(24, 8)    # every other pass sees one digit value: what a digit-skip would skip
    out["two-low-digits-only"] = vary(0, 16)      # many tiles, six passes that move nothing
    # one value of digit 1 (bits 8 .. 15) holds 20,000 keys -- more than four tiles --, every other value one key
    a_first = (rng.integers(0, 1 << 60, size=21_000, dtype=U64) & ~U64(3)) | U64(1)   # starts with A, ends with C: canonical
    heavy = np.unique((a_first[:20_600] & ~(U64(0xFF) << U64(8))) | (U64(0x5A) << U64(8)))[:20_000]
    lone = (a_first[20_600:20_855] & ~(U64(0xFF) << U64(8))) | (np.array([d for d in range(256) if d != 0x5A], dtype=U64) << U64(8))
    skew = np.unique(np.concatenate([heavy, lone]))
    assert skew.size == 20_255 and (skew <= _revcomp(skew, k)).all()
    out["one-heavy-digit-value"] = skew[rng.permutation(skew.size)]
    return out


PATTERNS = _patterns()


@pytest.mark.parametrize("name", sorted(PATTERNS))
def test_key_patterns_at_k31(K, name):
    keys = PATTERNS[name]
    assert keys.size >= 30 and np.unique(keys).size == keys.size
    counts = mix(keys)
    with build(K, 31, keys, counts) as dc:
        check_both_forms(K, dc, *want(keys, counts))
        rc, n, gk, gc = sorted_device(K, dc, keys.size)   # the same input gives the same output on every run
        rc2, n2, gk2, gc2 = sorted_device(K, dc, keys.size)
        assert rc == rc2 == K.native.KH_OK and np.array_equal(gk, gk2) and np.array_equal(gc, gc2)


# ---- counts and min_count -------------------------------------------------------------------------------------------------
BIG_COUNTS = [1, 2, 3, 2**32 - 1, 2**32, 2**32 + 1, 2**40, 2**63, 2**64 - 1]


@pytest.fixture(scope="module")
def big_table(K):
    rng = np.random.default_rng(SEED + 200)
    keys = random_keys(21, 9000, rng)
    counts = np.array(BIG_COUNTS, dtype=U64)[np.arange(keys.size) % len(BIG_COUNTS)]
    dc = build(K, 21, keys, counts)
    yield dc, keys, counts
    dc.close()


@pytest.mark.parametrize("mc", [0, 1, 2, 3, 2**32, 2**64 - 1], ids=lambda mc: f"mc{mc}")
def test_min_count_and_wide_counts(K, big_table, mc):
    dc, keys, counts = big_table
    wk, wc = want(keys, counts, mc)
    assert wk.size > 0 and (mc > 1 or wk.size == keys.size) and int(wc.max()) == 2**64 - 1
    check_both_forms(K, dc, wk, wc, mc)


def test_cap_too_small_writes_nothing(K, big_table):
    dc, keys, counts = big_table
    N = K.native
    wk, wc = want(keys, counts, 2)
    need = wk.size
    for call in (sorted_host, sorted_device):
        rc, n, gk, gc = call(K, dc, need - 1, 2)
        assert rc == N.KH_ERR_RANGE and n == 0, (call.__name__, rc, n)
        assert (gk == U64(CANARY)).all() and (gc == U64(CANARY)).all(), call.__name__   # every entry still the canary
        assert dc.result_size(2) == need                                                # the context goes on answering
        rc, n, gk, gc = call(K, dc, need, 2)
        assert rc == N.KH_OK and n == need
        assert np.array_equal(inside(gk, need), wk) and np.array_equal(inside(gc, need), wc)
        rc, n, gk, gc = call(K, dc, need + 7, 2)                                        # room to spare: nothing behind n
        assert rc == N.KH_OK and n == need and np.array_equal(inside(gk, need), wk) and np.array_equal(inside(gc, need), wc)


def test_empty_table_takes_null_arrays(K):
    with K.DeviceCounter(21) as dc:
        for name in ("kh_result_sorted", "kh_result_sorted_device"):
            n = C.c_uint64(5)
            assert getattr(K.lib(), name)(dc._h, None, None, 0, 1, C.byref(n)) == K.native.KH_OK and n.value == 0
        k_, c_ = dc.result_sorted()
        assert k_.size == 0 and c_.size == 0


# ---- both table forms -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 25])
def test_both_table_forms_give_the_same_arrays(K, k):
    """A partitioned count of synthetic reads against the oracle, read as the count left it (k = 21: the 8-byte image) and again
    from a count with KMERHIP_NARROW=0 (the 16-byte table): equal arrays, and the call converts nothing."""
    bases, _ = O.synth_reads(SEED, 1 << 20, 150, 0, 200_000, with_qual=False)
    m = O.OracleMap()
    m.scan_flat(bases, k, nthreads=NCPU)
    okeys, ocnts = m.arrays()
    got = []
    for narrow in ("1", "0"):
        with _env("KMERHIP_NARROW", narrow):
            with K.DeviceCounter(k, capacity_hint=50_000_000, path="partition") as dc:
                dc.push(bases)
                st = dc.finish()
                assert st["part_batches"] >= 1 and st["distinct"] == okeys.size
                gk, gc = dc.result_sorted()
                st2 = dc.finish()
                assert all(st2[f] == st[f] for f in ("slot_bytes", "distinct", "kmers", "grows")), (st, st2)
                check_both_forms(K, dc, okeys, ocnts)
                got.append((st["slot_bytes"], gk, gc))
    assert got[1][0] == 16 and (k != 21 or got[0][0] == 8), [g[0] for g in got]
    for _, gk, gc in got:
        assert np.array_equal(gk, okeys) and np.array_equal(gc, ocnts)


# ---- text -----------------------------------------------------------------------------------------------------------------
def kmers_of(keys, k):
    """The k-mer strings of packed keys (first base most significant), as bytes."""
    shifts = (U64(2) * np.arange(k - 1, -1, -1, dtype=U64))[None, :]
    codes = ((np.asarray(keys, dtype=U64)[:, None] >> shifts) & U64(3)).astype(np.intp)
    return [row.tobytes() for row in np.frombuffer(b"ACGT", dtype=np.uint8)[codes]]


def document(fmt, k, keys, counts):
    """What a sorted stream must deliver for these (already ascending) pairs: the records in that order and json's framing."""
    recs = [record(fmt, km.decode(), int(c), first=(i == 0)) for i, (km, c) in enumerate(zip(kmers_of(keys, k), counts.tolist()))]
    if not recs:
        return empty_doc(fmt), recs
    return b"".join(recs) + (b"\n]\n" if fmt == "json" else b""), recs


def fetch(dc, fmt, mc=1, cap=1 << 20, device=False, sorted=True, between=None):
    import torch
    nr, nb = dc.result_text_begin(fmt, mc, sorted=sorted)
    buf = torch.empty(cap + 7, dtype=torch.uint8, device="cuda:0")[7:] if device else np.empty(cap, dtype=np.uint8)
    pieces = []
    while True:
        n = dc.result_text_device(buf) if device else dc.result_text_next(buf)
        if n == 0:
            break
        assert n <= cap
        pieces.append(bytes(buf[:n].cpu().numpy()) if device else buf[:n].tobytes())
        if between:
            between()
    return nr, nb, pieces


@pytest.fixture(scope="module")
def text_table(K):
    rng = np.random.default_rng(SEED + 300)
    k = 21
    keys = random_keys(k, 5000, rng)
    counts = mix(keys)
    counts[::7] = np.array(BIG_COUNTS, dtype=U64)[np.arange(counts[::7].size) % len(BIG_COUNTS)]   # records of every length
    dc = build(K, k, keys, counts)
    yield dc, k, keys, counts
    dc.close()


@pytest.mark.parametrize("fmt", FORMATS)
def test_sorted_text_is_the_records_in_key_order(K, text_table, fmt):
    dc, k, keys, counts = text_table
    for mc in (1, 3, 2**32):
        wk, wc = want(keys, counts, mc)
        whole, recs = document(fmt, k, wk, wc)
        nr_u, nb_u, unsorted = fetch(dc, fmt, mc, sorted=False)
        nr, nb, pieces = fetch(dc, fmt, mc, cap=64 << 20)
        assert (nr, nb) == (nr_u, nb_u) == (wk.size, len(whole)), (mc, nr, nb, nr_u, nb_u)     # totals as for the unsorted stream
        assert len(pieces) == 1 and pieces[0] == whole, mc
        if mc == 1:
            assert b"".join(unsorted) != whole                                              # (the table's own order is another one)
    wk, wc = want(keys, counts)
    whole, recs = document(fmt, k, wk, wc)
    largest = max(len(r) for r in recs) + (2 if fmt == "json" else 0)
    for cap, device in ((largest, False), (4096, False), (1 << 20, False), (4096, True), (1 << 20, True), (len(whole) + 16, True)):
        _, nb, pieces = fetch(dc, fmt, cap=cap, device=device)
        assert nb == len(whole) and b"".join(pieces) == whole, (cap, device)
        assert all(ends_at_record_end(fmt, p, i == len(pieces) - 1) for i, p in enumerate(pieces)), (cap, device)
        if cap == largest:
            assert len(pieces) >= wk.size // 2


def test_readers_between_pieces_and_what_ends_the_stream(K, text_table):
    dc, k, keys, counts = text_table
    N = K.native
    wk, wc = want(keys, counts)
    whole, _ = document("tsv", k, wk, wc)
    hist = dc.histogram()

    def readers():
        assert dc.result_size() == wk.size
        assert dc.lookup(wk[:3]).tolist() == wc[:3].tolist()
        assert dc.histogram() == hist

    _, _, pieces = fetch(dc, "tsv", cap=4096, between=readers)
    assert len(pieces) > 10 and b"".join(pieces) == whole
    # kh_result_sorted between pieces takes the stream's scratch: the stream ends, a new begin restarts it
    dc.result_text_begin("tsv", sorted=True)
    buf = np.empty(4096, dtype=np.uint8)
    assert dc.result_text_next(buf) > 0
    gk, gc = dc.result_sorted()
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)
    with pytest.raises(K.KmerHipError) as ei:
        dc.result_text_next(buf)
    assert ei.value.status == N.KH_ERR_STATE
    assert b"".join(fetch(dc, "tsv", cap=1 << 20)[2]) == whole
    # a bit beside the three formats and KH_OUT_SORTED
    nr, nb = C.c_uint64(0), C.c_uint64(0)
    assert K.lib().kh_result_text_begin(dc._h, 0x200 | N.KH_OUT_TSV, 1, C.byref(nr), C.byref(nb)) == N.KH_ERR_BAD_ARG
    assert K.lib().kh_result_text_begin(dc._h, N.KH_OUT_SORTED, 1, C.byref(nr), C.byref(nb)) == N.KH_ERR_BAD_ARG
    assert b"".join(fetch(dc, "tsv", cap=1 << 20)[2]) == whole   # the context is usable


def test_sorted_text_of_an_empty_table(K):
    with K.DeviceCounter(21) as dc:
        for fmt in FORMATS:
            nr, nb, pieces = fetch(dc, fmt)
            assert nr == 0 and b"".join(pieces) == empty_doc(fmt) and nb == len(empty_doc(fmt))


# ---- geometry independence ------------------------------------------------------------------------------------------------
def test_the_same_pairs_in_three_geometries(K):
    rng = np.random.default_rng(SEED + 400)
    k = 21
    keys = random_keys(k, 70_000, rng)
    counts = mix(keys)
    wk, wc = want(keys, counts)
    whole, _ = document("tsv", k, wk, wc)
    unsorted, slots = [], []
    for env in ({"KMERHIP_TABLE_REGIONS": "1024"}, {"KMERHIP_TABLE_REGIONS": "5120"}, {"KMERHIP_POW2_TABLE": "1"}):
        (name, value), = env.items()
        with _env(name, value):
            with build(K, k, keys, counts, capacity_hint=600_000) as dc:
                slots.append(dc.finish()["table_slots"])
                check_both_forms(K, dc, wk, wc)
                assert b"".join(fetch(dc, "tsv", cap=1 << 20)[2]) == whole          # byte-identical sorted documents
                unsorted.append(b"".join(fetch(dc, "tsv", cap=8 << 20, sorted=False)[2]))
    assert slots[0] == 1024 * 4096 and slots[1] == 5120 * 4096 and slots[2] & (slots[2] - 1) == 0, slots
    lines = [sorted(u.splitlines()) for u in unsorted]
    assert lines[0] == lines[1] == lines[2] == whole.splitlines()                  # permutations of each other ...
    assert len({u for u in unsorted}) >= 2                                          # ... that differ: the test can see an order


# ---- shards ---------------------------------------------------------------------------------------------------------------
def test_shard_tables_give_their_own_keys_in_order(K):
    rng = np.random.default_rng(SEED + 500)
    k = 21
    keys = random_keys(k, 60_000, rng)
    counts = mix(keys)
    wk, wc = want(keys, counts)
    owner = O.owners(K, keys, k, 2)
    parts = []
    for i in (0, 1):
        mine = owner == i
        assert mine.sum() > 20_000
        with K.DeviceCounter(k) as dc:
            dc.set_shard(i, 2)
            dc.merge_pairs(np.ascontiguousarray(keys[mine]), np.ascontiguousarray(counts[mine]))
            sk, sc = want(keys[mine], counts[mine])
            check_both_forms(K, dc, sk, sc)
            gk, gc = dc.result_sorted()
            assert (gk[1:] > gk[:-1]).all()
            parts.append((gk, gc))
    mk = np.concatenate([p[0] for p in parts])
    mc = np.concatenate([p[1] for p in parts])
    o = np.argsort(mk, kind="stable")
    assert np.array_equal(mk[o], wk) and np.array_equal(mc[o], wc)                  # the merge of the two is the full table's result


# ---- the product library --------------------------------------------------------------------------------------------------
CHILD = r'''
import json, os, sys
import numpy as np
import krust_amd
from krust_amd import native
assert native.LIB_PATH.endswith("libkmerhip.so"), native.LIB_PATH
rng = np.random.default_rng(7)
k = 31
raw = rng.integers(0, 1 << 64, size=50_000, dtype=np.uint64) >> np.uint64(2)
keys = np.unique(np.array([krust_amd.canonical(int(x), k)[0] for x in raw[:12_000]], dtype=np.uint64))
keys = keys[rng.permutation(keys.size)]
counts = (keys * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(40)) + np.uint64(1)
with krust_amd.DeviceCounter(k) as dc:
    dc.merge_pairs(keys, counts)
    gk, gc = dc.result_sorted()
    text = b"".join(dc.result_text("tsv", sorted=True))
o = np.argsort(keys)
assert np.array_equal(gk, keys[o]) and np.array_equal(gc, counts[o])
want = b"".join(f"{krust_amd.unpack(int(a), k)}\t{int(b)}\n".encode() for a, b in zip(keys[o], counts[o]))
assert text == want
print("RESULT " + json.dumps({"pairs": int(gk.size), "bytes": len(text)}))
'''


def test_sorted_through_the_product_library():
    env = dict(os.environ)
    env.pop("KMERHIP_LIB", None)
    p = subprocess.run([sys.executable, "-c", f"import sys; sys.path.insert(0, {ROOT!r})\n" + CHILD], capture_output=True, text=True,
                       env=env, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert res["pairs"] > 11_000 and res["bytes"] > 11_000 * 33
