"""The kernels that READ a finished table -- table_count / table_compact / table_hist / table_lookup (kernels.hip.h), their
8-byte-image twins ntable_* (partition.hip.h) and the host halves kh_result_size / kh_result_copy / kh_result_copy_device /
kh_histogram / kh_lookup (kmerhip.hip) -- on tables whose counts are CHOSEN: every tier edge of the histogram kernels
(3 | 4, 2047 | 2048, 65535 | 65536), more than 2^16 counts in the `big` tier (the second pass of kh_histogram), 32- and 64-bit
extremes, output arrays that are too small, and lookups of words no table can hold.

Counts do not come from reads here.  A wide table is kh_merge_pairs of a (key, count) list; an image is a packed region export
(one u64 per pair: count << 32 | hash bits) whose upper words are rewritten on the host and merged back.  What a table must
answer is computed in plain Python / numpy from the lists this file wrote; the image is additionally held to a 16-byte twin
built from the same pairs.

Run with `pytest -m gpu` on an MI355X."""
import contextlib
import ctypes as C
import os
from collections import Counter

import numpy as np
import pytest

import oracle_lib as O
from test_gpu_parity import _table_unhash  # the inverse of the table hash, restated once (O.table_hash_np: the forward one)

pytestmark = pytest.mark.gpu

SEED = 20260131
NCPU = max(1, min(os.cpu_count() or 1, 16))
U64 = np.uint64
CANARY = 0x5A5A5A5A5A5A5A5A
PAD = 64  # canary entries on each side of an output array

# ---- 1. the count list -------------------------------------------------------------------------------------------------
# every tier edge several times; 64 / 65 times = a whole wave / a wave and one lane with the same value
EDGES = {1: 64, 2: 65, 3: 64, 4: 64, 5: 65, 2046: 7, 2047: 65, 2048: 64, 2049: 65, 65534: 9, 65535: 65, 65536: 64, 65537: 65}
GIANTS = {2**31 - 1: 5, 2**31: 6}            # (an image takes at most one of these per region: a region's total stays < 2^32)
BIG_VALUES = (65538, 70001, 99991, 1 << 17, (1 << 20) + 3, 1 << 21)
BIG_BLOCK = 66_000                           # > 2^16 entries of the `big` tier: kh_histogram needs its second pass
WIDE_ONLY = {2**32 - 1: 3, 2**32: 4, 2**32 + 1: 3, 2**40: 2, 2**63: 3, 2**64 - 1: 3}
SPREAD = 6000                                # entries over 6 .. 2045 (LDS bins) and over 2050 .. 65533 (dense array), each
MIN_COUNTS = [0, 1, 2, 3, 4, 5, 2047, 2048, 2049, 65535, 65536, 65537, 2**31, 2**32, 2**64 - 1]


def count_list(n, wide):
    """(ordinary counts in a fixed shuffled order, the giants): n counts in all, from a fixed seed."""
    rng = np.random.default_rng(SEED)
    fixed = [np.full(reps, v, dtype=U64) for v, reps in EDGES.items()]
    fixed.append(np.array(BIG_VALUES, dtype=U64)[rng.integers(0, len(BIG_VALUES), size=BIG_BLOCK)])
    fixed.append(rng.integers(6, 2046, size=SPREAD).astype(U64))
    fixed.append(rng.integers(2050, 65534, size=SPREAD).astype(U64))
    if wide:
        fixed += [np.full(reps, v, dtype=U64) for v, reps in WIDE_ONLY.items()]
    giants = np.concatenate([np.full(reps, v, dtype=U64) for v, reps in GIANTS.items()])
    fixed = np.concatenate(fixed)
    bulk = n - fixed.size - giants.size
    assert bulk > n // 4, "the key set is too small for the list and a bulk of 1 .. 3 beside it"
    ordinary = np.concatenate([fixed, rng.choice(np.array([1, 2, 3], dtype=U64), size=bulk, p=[0.7, 0.2, 0.1])])
    return ordinary[rng.permutation(ordinary.size)], giants


def _revcomp(x, k):
    x = ~np.ascontiguousarray(x, dtype=U64)
    x = ((x >> U64(2)) & U64(0x3333333333333333)) | ((x & U64(0x3333333333333333)) << U64(2))
    x = ((x >> U64(4)) & U64(0x0F0F0F0F0F0F0F0F)) | ((x & U64(0x0F0F0F0F0F0F0F0F)) << U64(4))
    return x.byteswap() >> U64(64 - 2 * k)


def draw_keys(K, k, n, rng, avoid=None):
    """n distinct canonical k-mers (packed), none of them in `avoid`."""
    raw = rng.integers(0, 1 << 64, size=n + n // 4 + 64, dtype=U64) >> U64(64 - 2 * k)
    canon = np.minimum(raw, _revcomp(raw, k))
    for i in range(0, raw.size, max(1, raw.size // 50)):  # (the numpy canonical form, pinned on the library's)
        assert K.canonical(int(raw[i]), k)[0] == int(canon[i])
    keys = np.unique(canon)
    if avoid is not None:
        keys = keys[~np.isin(keys, avoid)]
    assert keys.size >= n
    return keys[rng.permutation(keys.size)[:n]]


@contextlib.contextmanager
def _env(name, value):
    old = os.environ.get(name)
    os.environ[name] = value
    try:
        yield
    finally:
        if old is None:
            del os.environ[name]
        else:
            os.environ[name] = old


class Table:
    """One context and what plain Python says it holds."""

    def __init__(self, dc, k, keys, counts, slot_bytes, stats):
        o = np.argsort(keys, kind="stable")
        self.dc, self.k, self.keys, self.counts = dc, k, np.ascontiguousarray(keys[o]), np.ascontiguousarray(counts[o])
        assert np.unique(self.keys).size == self.keys.size
        self.hist = sorted(Counter(self.counts.tolist()).items())
        self.slot_bytes, self.stats = slot_bytes, stats
        assert stats["slot_bytes"] == slot_bytes and stats["distinct"] == self.keys.size

    def want(self, mc):
        sel = self.counts >= U64(max(mc, 1))
        return self.keys[sel], self.counts[sel]

    def want_hist(self, mc):
        return [(c, f) for c, f in self.hist if c >= max(mc, 1)]


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import krust_amd
    krust_amd.lib()  # ImportError if the HIP extension is missing: no silent fallback
    return krust_amd


# ---- 2. wide tables ----------------------------------------------------------------------------------------------------
N_WIDE = 120_000


def _wide_table(K, k, hint, seed):
    rng = np.random.default_rng(seed)
    keys = draw_keys(K, k, N_WIDE, rng)
    ordinary, giants = count_list(N_WIDE, wide=True)
    counts = np.concatenate([ordinary, giants])[rng.permutation(N_WIDE)]
    dc = K.DeviceCounter(k, capacity_hint=hint)
    dc.merge_pairs(keys, counts)
    return Table(dc, k, keys, counts, 16, dc.finish())   # (kmers, the sum of the counts, wraps here: not asserted)


@pytest.fixture(scope="module")
def wide_k21(K):
    t = _wide_table(K, 21, 400_000, 1)
    assert t.stats["grows"] == 0
    yield t
    t.dc.close()


@pytest.fixture(scope="module")
def wide_k32(K):
    t = _wide_table(K, 32, 400_000, 2)   # keys use all 64 bits
    assert t.stats["grows"] == 0 and int(t.keys.max()) >> 62
    yield t
    t.dc.close()


@pytest.fixture(scope="module")
def wide_grown(K):
    t = _wide_table(K, 21, 1, 3)
    assert t.stats["grows"] >= 1
    yield t
    t.dc.close()


# ---- 3. the image ------------------------------------------------------------------------------------------------------
IMAGE_K, IMAGE_HINT, IMAGE_REGIONS = 21, 3_000_000, 1 << 11   # 2^11 regions: 31 hash bits below the region index


@pytest.fixture(scope="module")
def sender(K):
    """A few thousand reads counted on the partition path, and its packed exports for one owner and for two."""
    import torch
    bases, _ = O.synth_reads(SEED, 1 << 18, 150, 0, 2000, with_qual=False)
    m = O.OracleMap()
    m.scan_flat(bases, IMAGE_K, nthreads=NCPU)
    okeys, ocnts = m.arrays()
    out = {"keys": okeys, "counts": ocnts}
    with K.DeviceCounter(IMAGE_K, capacity_hint=IMAGE_HINT, path="partition") as dc:
        dc.push(bases)
        st = dc.finish()
        n, R = st["distinct"], st["table_slots"] // 4096
        assert R == IMAGE_REGIONS and n == okeys.size and n > 150_000, (R, n)
        for nparts in (1, 2):
            dp = torch.empty(n, dtype=torch.int64, device="cuda")
            rc = torch.empty(R, dtype=torch.int32, device="cuda")
            parts, R2 = dc.export_regions_packed_device(nparts, dp.data_ptr(), n, rc.data_ptr(), R)
            assert R2 == R and int(parts.sum()) == n
            out[nparts] = (dp.cpu().numpy().view(U64).copy(), rc.cpu().numpy().astype(np.int64), parts)
    return out


def _merge_packed(K, pairs, region_counts, shard, narrow):
    """A fresh context made shard `shard` from ONE sender's packed pairs; (context, stats)."""
    import torch
    dp = torch.from_numpy(pairs.view(np.int64).copy()).cuda()
    rc = torch.from_numpy(region_counts.astype(np.int32)).cuda()
    torch.cuda.synchronize()
    with _env("KMERHIP_NARROW", "1" if narrow else "0"):
        dc = K.DeviceCounter(IMAGE_K, capacity_hint=IMAGE_HINT)
        dc.set_shard(*shard)
        dc.merge_regions_packed_device(IMAGE_REGIONS, [dp.data_ptr()], [rc.data_ptr()])
        st = dc.finish()
    torch.cuda.synchronize()
    return dc, st


@pytest.fixture(scope="module")
def image(K, sender):
    pairs, rc, _ = sender[1]
    n = pairs.size
    ordinary, giants = count_list(n, wide=False)
    # the pairs are in region order: a giant goes to a region of its own choice, at most one per region
    rng = np.random.default_rng(SEED + 1)
    start = np.concatenate([[0], np.cumsum(rc)])
    regions = rng.permutation(np.flatnonzero(rc > 0))[:giants.size]
    at = start[regions] + rng.integers(0, rc[regions])
    counts = np.empty(n, dtype=U64)
    rest = np.ones(n, dtype=bool)
    rest[at] = False
    counts[at], counts[rest] = giants, ordinary
    assert int(counts.max()) < 1 << 32
    region_of_pair = np.repeat(np.arange(IMAGE_REGIONS), rc)
    totals = np.bincount(region_of_pair, weights=counts.astype(np.float64), minlength=IMAGE_REGIONS)
    assert totals.max() < 2.0**32 - 2.0**12, "a region that takes in 2^32 occurrences widens the shard"
    rewritten = (counts << U64(32)) | (pairs & U64(0xFFFFFFFF))
    # the reference: the same pairs as a 16-byte table, tied to the list written above ...
    twin, st = _merge_packed(K, rewritten, rc, (0, 1), narrow=False)
    assert st["slot_bytes"] == 16 and st["distinct"] == n
    tk, tc = twin.result()
    twin.close()
    assert np.array_equal(np.sort(tc), np.sort(counts))
    assert np.array_equal(tk, sender["keys"])   # (the keys the oracle found in the reads: rewriting counts moved none)
    # ... then the image itself
    dc, st = _merge_packed(K, rewritten, rc, (0, 1), narrow=True)
    assert st["slot_bytes"] == 8, "the merge did not leave the 8-byte image: this would not test the ntable_* kernels"
    yield Table(dc, IMAGE_K, tk, tc, 8, st)
    dc.close()


@pytest.fixture(scope="module")
def image_half(K, sender):
    """Shard 0 of two as an image: owner 0's half of the two-owner export, with the counts the reads gave."""
    pairs, rc, parts = sender[2]
    dc, st = _merge_packed(K, pairs[:int(parts[0])], rc[:IMAGE_REGIONS // 2], (0, 2), narrow=True)
    assert st["slot_bytes"] == 8
    mine = O.owners(K, sender["keys"], IMAGE_K, 2) == 0
    assert int(mine.sum()) == int(parts[0])
    yield Table(dc, IMAGE_K, sender["keys"][mine], sender["counts"][mine], 8, st)
    dc.close()


TABLES = ["wide_k21", "wide_k32", "wide_grown", "image"]


@pytest.fixture
def table(request):
    return request.getfixturevalue(request.param)


def test_the_image_is_the_wide_twin(image):
    """Section 3: sorted result() of the image == the 16-byte twin's arrays, exactly (the fixture tied the twin to the list)."""
    k, c = image.dc.result()
    assert np.array_equal(k, image.keys) and np.array_equal(c, image.counts)


# ---- 4. size, histogram and pairs for every min_count -------------------------------------------------------------------
@pytest.mark.parametrize("mc", MIN_COUNTS, ids=lambda mc: f"mc{mc}")
@pytest.mark.parametrize("table", TABLES, indirect=True)
def test_size_histogram_and_pairs(table, mc):
    wk, wc = table.want(mc)
    if mc in (1, 65536):  # kh_histogram's list starts with 2^16 entries: these calls cannot do with one pass
        assert int((table.counts >= U64(65536)).sum()) > 1 << 16
    assert table.dc.result_size(mc) == wk.size
    assert table.dc.histogram(mc) == table.want_hist(mc)
    gk, gc = table.dc.result(mc)
    assert np.array_equal(gk, wk) and np.array_equal(gc, wc)


# ---- 5. arrays that are too small ---------------------------------------------------------------------------------------
def _canary_arrays(cap):
    a = np.full(cap + 2 * PAD, CANARY, dtype=U64)
    b = np.full(cap + 2 * PAD, CANARY, dtype=U64)
    return a, b


def _only_inside_changed(arr, n):
    return bool((arr[:PAD] == U64(CANARY)).all() and (arr[PAD + n:] == U64(CANARY)).all())


@pytest.mark.parametrize("table", ["wide_k21", "image"], indirect=True)
def test_histogram_into_arrays_that_are_too_small(K, table):
    N = K.native
    mc = 2
    full = table.want_hist(mc)
    lines = len(full)
    assert lines > 4096  # (what native.py's first attempt offers: its retry is what hid this path)
    for cap in (0, 1, lines - 1, lines):
        cnt, frq = _canary_arrays(cap)
        n = C.c_uint64(123456789)
        rc = K.lib().kh_histogram(table.dc._h, mc, cnt.ctypes.data + 8 * PAD, frq.ctypes.data + 8 * PAD, cap, C.byref(n))
        assert rc == (N.KH_OK if cap == lines else N.KH_ERR_RANGE), (cap, rc)
        assert n.value == cap
        assert list(zip(cnt[PAD:PAD + cap].tolist(), frq[PAD:PAD + cap].tolist())) == full[:cap]  # the ascending prefix
        assert _only_inside_changed(cnt, cap) and _only_inside_changed(frq, cap), cap
        assert table.dc.result_size(mc) == table.want(mc)[0].size  # the context goes on answering


@pytest.mark.parametrize("table", ["wide_k21", "image"], indirect=True)
def test_result_copy_device_into_arrays_that_are_too_small(K, table):
    import torch
    N = K.native
    mc = 2
    wk, wc = table.want(mc)
    need = wk.size
    for cap in (0, 1, 63, 64, 65, need - 1, need):
        dk = torch.full((cap + PAD,), CANARY, dtype=torch.int64, device="cuda")
        dn = torch.full((cap + PAD,), CANARY, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        n = C.c_uint64(123456789)
        rc = K.lib().kh_result_copy_device(table.dc._h, dk.data_ptr(), dn.data_ptr(), cap, mc, C.byref(n))
        torch.cuda.synchronize()
        assert rc == (N.KH_OK if cap == need else N.KH_ERR_RANGE), (cap, rc)
        assert n.value == cap
        gk, gc = dk.cpu().numpy().view(U64), dn.cpu().numpy().view(U64)
        assert (gk[cap:] == U64(CANARY)).all() and (gc[cap:] == U64(CANARY)).all(), cap   # nothing behind cap
        gk, gc = gk[:cap], gc[:cap]
        assert np.unique(gk).size == cap                                                    # cap DISTINCT pairs of the map
        at = np.minimum(np.searchsorted(wk, gk), need - 1)
        assert np.array_equal(wk[at], gk) and np.array_equal(wc[at], gc), cap
        if cap == need:
            o = np.argsort(gk)
            assert np.array_equal(gk[o], wk) and np.array_equal(gc[o], wc)
    assert table.dc.result_size(mc) == need


@pytest.mark.parametrize("table", ["wide_k21", "image"], indirect=True)
def test_result_copy_into_host_arrays_that_are_too_small(K, table):
    N = K.native
    mc = 2
    wk, wc = table.want(mc)
    need = wk.size
    keys, cnts = _canary_arrays(need)
    n = C.c_uint64(123456789)
    rc = K.lib().kh_result_copy(table.dc._h, keys.ctypes.data + 8 * PAD, cnts.ctypes.data + 8 * PAD, need - 1, mc, C.byref(n))
    assert rc == N.KH_ERR_RANGE and n.value == 0
    assert (keys == U64(CANARY)).all() and (cnts == U64(CANARY)).all()   # nothing at all is written
    rc = K.lib().kh_result_copy(table.dc._h, keys.ctypes.data + 8 * PAD, cnts.ctypes.data + 8 * PAD, need, mc, C.byref(n))
    assert rc == N.KH_OK and n.value == need
    assert _only_inside_changed(keys, need) and _only_inside_changed(cnts, need)
    o = np.argsort(keys[PAD:PAD + need])
    assert np.array_equal(keys[PAD:PAD + need][o], wk) and np.array_equal(cnts[PAD:PAD + need][o], wc)


# ---- 6. lookup -----------------------------------------------------------------------------------------------------------
GRID_THREADS = 2 * 256 * 1024  # the most threads a launch gets: more probes than this and the grid-stride loop turns


@pytest.mark.parametrize("table", ["wide_k21", "wide_k32", "image", "image_half"], indirect=True)
def test_lookup_of_what_is_there_and_of_what_cannot_be(K, request, table):
    k, keys, counts = table.k, table.keys, table.counts
    rng = np.random.default_rng(SEED + 2)
    for key in [int(x) for x in keys[:: keys.size // 40]]:  # the restated hash, pinned on the library's
        assert K.owner(key, k, 1 << 20) == int(O.table_hash_np(np.array([key], dtype=U64), k)[0]) >> (2 * k - 20)
        assert _table_unhash(int(O.table_hash_np(np.array([key], dtype=U64), k)[0]), k) == key
    probes, expect = [], []

    def add(p, e):
        probes.append(np.asarray(p, dtype=U64))
        expect.append(np.broadcast_to(np.asarray(e, dtype=U64), probes[-1].shape))

    # duplicates inside one wave (probe i is lane i % 64 of its wave): one key 64 times, then two keys in turns
    add(np.full(64, keys[7]), counts[7])
    add(keys[[11, 13] * 32], counts[[11, 13] * 32])
    add(keys, counts)                                                   # every key that is there
    holds = keys
    if request.node.callspec.params["table"] == "image_half":           # the other shard's keys, present in the sender: 0
        everyone = request.getfixturevalue("sender")["keys"]
        other = everyone[~np.isin(everyone, keys)]
        assert other.size > 50_000
        add(other, 0)
        holds = everyone
    add(draw_keys(K, k, keys.size, rng, avoid=holds), 0)                # as many canonical keys that are not
    # absent keys whose probe run starts where a present key's does: the hash of a present key with only its lowest bits
    # changed names the same region and the same start slot (both come from the top of the hash)
    sample = keys[rng.permutation(keys.size)[:2000]]
    near = np.array([_table_unhash(int(h) ^ j, k) for h in O.table_hash_np(sample, k).tolist() for j in (1, 2, 3)], dtype=U64)
    near = near[~np.isin(near, holds)]
    assert near.size > 5000
    add(near, 0)
    if k < 32:                                                          # words with bits above the k-mer's 2k
        for bit in (2 * k, 2 * k + 1, 63):
            add(sample | U64(1 << bit), 0)
        add(keys[:64] | (U64(0xFFFFFFFFFFFFFFFF) << U64(2 * k)), 0)
    add([0xFFFFFFFFFFFFFFFF], 0)                                        # the all-ones word (the wide table's free marker)
    size = sum(p.size for p in probes)
    if size <= GRID_THREADS + 4096:                                     # (present keys again, until the stride loop turns)
        reps = (GRID_THREADS + 4096 - size) // keys.size + 1
        add(np.tile(keys, reps), np.tile(counts, reps))
    probes, expect = np.concatenate(probes), np.concatenate(expect)
    assert probes.size > GRID_THREADS
    o = rng.permutation(probes.size - 128) + 128                        # (the duplicates keep their lanes)
    probes[128:], expect[128:] = probes[o], expect[o]
    got = table.dc.lookup(probes)
    bad = np.flatnonzero(got != expect)
    assert bad.size == 0, [(hex(int(probes[i])), int(got[i]), int(expect[i])) for i in bad[:8]]
    # n == 1, and n == 0 with NULL pointers
    assert table.dc.lookup(keys[5:6]).tolist() == [int(counts[5])]
    assert K.lib().kh_lookup(table.dc._h, None, 0, None) == K.native.KH_OK


# ---- 7. all of it only read ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("table", TABLES + ["image_half"], indirect=True)
def test_reading_changed_nothing(table):
    st = table.dc.finish()
    assert (st["distinct"], st["slot_bytes"], st["table_slots"], st["grows"]) == tuple(
        table.stats[f] for f in ("distinct", "slot_bytes", "table_slots", "grows"))
    k, c = table.dc.result()
    assert np.array_equal(k, table.keys) and np.array_equal(c, table.counts)
