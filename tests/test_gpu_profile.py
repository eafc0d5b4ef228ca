"""kh_profile / kh_profile_device -- the table's count at every window start of new sequences -- against the oracle.

Expected values come from the oracle only: the table is O.count_records of the counted records, and every position is
O.from_sub (is the window a k-mer) + O.canonical + OracleMap.get, with the quality rule min_quality.saturating_add(33).
Large inputs use a vectorised numpy twin of that, which every test that uses it first checks against the oracle primitives
window by window on at least 2,000 positions.

kh_set_shard takes a power-of-two shard count, so the 3-shard case is what a 3-rank kh_merge_across leaves (the pairs route:
every rank an ordinary table that holds its owner's keys); the 2-shard cases are hash-range shards, wide and as the image."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
NO = native.PROFILE_NO_WINDOW if hasattr(native, "PROFILE_NO_WINDOW") else 0xFFFFFFFF
SAT = 0xFFFFFFFE
KS = [1, 2, 5, 11, 16, 17, 21, 25, 31, 32]


# ---- expected values -------------------------------------------------------------------------------------------------------
def thr_of(minq):
    return min(int(minq) + 33, 255)  # min_quality.saturating_add(33) on u8


def oracle_profile(flat, k, table, qual=None, minq=None, positions=None):
    """Entry by entry from the oracle primitives.  table: an OracleMap, or a dict key -> count."""
    flat = bytes(flat)
    n = len(flat)
    get = table.get if hasattr(table, "get") else None
    out = np.full(n, NO, dtype=np.uint32)
    thr = thr_of(minq) if (qual is not None and minq is not None) else None
    q = bytes(qual) if qual is not None else None
    for i in (range(n) if positions is None else positions):
        if i + k > n:
            continue
        w = flat[i:i + k]
        norm, err = O.from_sub(w)
        if norm is None:
            continue
        if thr is not None and min(q[i:i + k]) < thr:
            continue
        key, _ = O.canonical(norm)
        c = get(key)
        out[i] = min(int(c or 0), SAT)
    return out


_CODE = np.full(256, 255, dtype=np.uint8)
for _i, _ch in enumerate(b"ACGT"):
    _CODE[_ch] = _i
    _CODE[_ch + 32] = _i


def np_profile(flat, k, keys, counts, qual=None, minq=None):
    """The numpy twin (checked against oracle_profile by its users)."""
    flat = np.frombuffer(bytes(flat), dtype=np.uint8) if not isinstance(flat, np.ndarray) else flat
    n = flat.size
    out = np.full(n, NO, dtype=np.uint32)
    nw = n - k + 1
    if nw <= 0:
        return out
    code = _CODE[flat]
    bad = code == 255
    if qual is not None and minq is not None:
        bad |= np.asarray(qual, dtype=np.uint8) < thr_of(minq)
    cs = np.concatenate(([0], np.cumsum(bad, dtype=np.int64)))
    good = (cs[k:] - cs[:-k]) == 0
    c64 = (code & 3).astype(np.uint64)
    fwd = np.zeros(nw, dtype=np.uint64)
    rc = np.zeros(nw, dtype=np.uint64)
    for j in range(k):
        fwd |= c64[j:j + nw] << np.uint64(2 * (k - 1 - j))
        rc |= (np.uint64(3) - c64[j:j + nw]) << np.uint64(2 * j)
    canon = np.minimum(fwd, rc)
    keys = np.asarray(keys, dtype=np.uint64)
    counts = np.asarray(counts, dtype=np.uint64)
    val = np.zeros(nw, dtype=np.uint64)
    if keys.size:
        pos = np.minimum(np.searchsorted(keys, canon), keys.size - 1)
        hit = keys[pos] == canon
        val[hit] = counts[pos[hit]]
    out[:nw][good] = np.minimum(val, np.uint64(SAT)).astype(np.uint32)[good]
    return out


def check_twin(flat, k, m, keys, counts, qual=None, minq=None, npos=2000, seed=1):
    n = len(flat)
    pos = np.unique(np.concatenate((np.random.default_rng(seed).integers(0, n, size=npos + 500), np.arange(min(n, 300)),
                                    np.arange(max(0, n - 300), n))))
    assert pos.size >= min(npos, n)
    want = oracle_profile(flat, k, m, qual, minq, positions=pos.tolist())
    got = np_profile(flat, k, keys, counts, qual, minq)
    assert np.array_equal(got[pos], want[pos]), "the numpy twin differs from the oracle primitives"
    return got


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def dirty_records(seed, k, n=40, maxlen=120):
    """N runs, lower case, IUPAC codes, a CR at a line end, and records of length k-1, k, k+1."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTacgtNRYKMn", dtype=np.uint8)
    p = np.array([.2, .2, .2, .2, .03, .03, .03, .03, .02, .01, .01, .01, .02, .01])
    recs = [alpha[rng.choice(alpha.size, size=int(rng.integers(1, maxlen)), p=p / p.sum())].tobytes() for _ in range(n)]
    clean = lambda m: np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=m)].tobytes()
    recs += [clean(max(k - 1, 1)), clean(k), clean(k + 1), clean(40) + b"NNNNNNNN" + clean(50), clean(30) + b"\r", b"N" * 20]
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def flat_of(recs):
    return np.frombuffer(b"".join(r + b"\n" for r in recs), dtype=np.uint8).copy()


def quals_for(rng, recs, filler_every=3):
    """Quality strings over the whole byte range; every third record carries the 0xFF filler (a record without qualities)."""
    out = []
    for i, r in enumerate(recs):
        if i % filler_every == 0:
            out.append(b"\xff" * len(r))
        else:
            out.append(bytes(rng.choice(np.array([33, 35, 40, 52, 53, 54, 73, 125, 126, 127, 200, 254, 255], dtype=np.uint8), size=len(r))))
    return out


def flat_qual(quals):
    return np.frombuffer(b"".join(q + b"\n" for q in quals), dtype=np.uint8).copy()


def dev_profile(dc, flat, qual=None, shift=5):
    """kh_profile_device on torch tensors, the buffers at an odd offset of their allocations."""
    import torch
    n = len(flat)
    tb = torch.empty(n + shift + 64, dtype=torch.uint8, device="cuda:0")
    tb[shift:shift + n] = torch.from_numpy(np.ascontiguousarray(flat))
    tq = None
    if qual is not None:
        tq = torch.empty(n + shift + 3 + 64, dtype=torch.uint8, device="cuda:0")
        tq[shift + 3:shift + 3 + n] = torch.from_numpy(np.ascontiguousarray(qual))
    to = torch.full((n + 8,), 0x7BADBEEF, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dc.profile_device(tb.data_ptr() + shift, None if tq is None else tq.data_ptr() + shift + 3, n, to.data_ptr() + 4)
    res = to.cpu().numpy().view(np.uint32)
    assert res[0] == 0x7BADBEEF and (res[n + 1:] == 0x7BADBEEF).all(), "kh_profile_device wrote outside its n entries"
    return res[1:n + 1].copy()


def stats_pair(dc):
    st = dc.finish()
    return st["kmers"], st["distinct"], st["slot_bytes"]


# ---- k and masking -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_k_without_and_with_qualities(k):
    rng = np.random.default_rng(100 + k)
    counted = dirty_records(1000 + k, k)
    fresh = dirty_records(2000 + k, k, n=25)          # never counted: valid windows read 0 (or a shared short k-mer's count)
    query = counted[::2] + fresh
    fq = flat_of(query)
    cq, qq = quals_for(rng, counted), quals_for(rng, query)
    for minq in (None, 0, 20, 93, 255):
        m = O.count_records(counted, k, quals=cq if minq is not None else None, min_quality=minq)
        qual = flat_qual(qq) if minq is not None else None
        want = oracle_profile(fq, k, m, qual, minq)
        with native.DeviceCounter(k, min_quality=minq) as dc:
            dc.push(flat_of(counted), flat_qual(cq) if minq is not None else None)
            before = stats_pair(dc)
            got_d = dev_profile(dc, fq, qual)
            got_h = dc.profile(fq, qual)
            assert np.array_equal(got_d, want), (k, minq, np.flatnonzero(got_d != want)[:10])
            assert np.array_equal(got_h, want), (k, minq, np.flatnonzero(got_h != want)[:10])
            assert stats_pair(dc) == before
            # qualities given to a context without a threshold mask nothing
            if minq is None:
                assert np.array_equal(dc.profile(fq, flat_qual(qq)), want)


@pytest.mark.parametrize("k", [1, 5, 21, 32])
def test_short_and_empty_inputs(k):
    recs = dirty_records(7, k)
    m = O.count_records(recs, k)
    with native.DeviceCounter(k) as dc:
        dc.push(flat_of(recs))
        for n in sorted({0, 1, k - 1, k, k + 1, 15, 16, 17}):
            buf = np.frombuffer((b"ACGTTGCAAGGCTTAACCGGTTAACGTACGTAGCTAGCTAGGATC" * 2)[:n], dtype=np.uint8).copy()
            want = oracle_profile(buf, k, m)
            if n < k:
                assert (want == NO).all()
            assert np.array_equal(dc.profile(buf), want), n
            if n:
                assert np.array_equal(dev_profile(dc, buf), want), n
        # n == 0 is KH_OK, with or without pointers
        assert native.lib().kh_profile(dc._h, None, None, 0, None) == 0
        assert native.lib().kh_profile_device(dc._h, None, None, 0, None) == 0


# ---- shapes at size ------------------------------------------------------------------------------------------------------------
def test_one_100kb_record_and_unseen_sequences():
    k = 21
    rng = np.random.default_rng(5)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    genome = acgt[rng.integers(0, 4, size=100_000)]
    genome[5000:5040] = ord("N")
    genome[70_000:70_300] |= 32      # a soft-masked stretch: lower case counts (ACGTacgt)
    rec = genome.tobytes()
    m = O.count_records([rec], k)
    keys, counts = m.arrays()
    flat = np.frombuffer(rec + b"\n", dtype=np.uint8).copy()
    want = check_twin(flat, k, m, keys, counts)
    other = np.frombuffer(acgt[rng.integers(0, 4, size=30_000)].tobytes() + b"\nNNNN\n", dtype=np.uint8).copy()
    want_other = check_twin(other, k, m, keys, counts, seed=2)
    assert (want_other[:29_980] == 0).all() and (want_other[29_980:] == NO).all()   # never counted: 0 where valid, NO_WINDOW elsewhere
    with native.DeviceCounter(k) as dc:
        dc.push(flat)
        assert np.array_equal(dev_profile(dc, flat), want)
        assert np.array_equal(dc.profile(flat), want)
        assert np.array_equal(dev_profile(dc, other), want_other)
        assert np.array_equal(dc.profile(other), want_other)
        # a window of the record and its reverse complement read the same count
        assert int(want[100]) >= 1


@pytest.mark.parametrize("k", [5, 21, 32])
def test_record_edges_around_16_and_4096(k):
    """Separators at every offset around multiples of 16 and 4096, and buffer ends (n) there too, at several alignments."""
    rng = np.random.default_rng(40 + k)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    body = acgt[rng.integers(0, 4, size=3 * 4096 + 64)].copy()
    edges = [base + d for base in (16, 32, 48, 4096, 8192, 12288) for d in range(-3, 4)]
    m = O.count_records(bytes(body).split(b"\n"), k)
    keys, counts = m.arrays()
    full = check_twin(body, k, m, keys, counts)
    with native.DeviceCounter(k) as dc:
        dc.push(body)
        for e in edges:      # one record edge at a time, at every offset around the multiples
            one = body.copy()
            one[e] = ord("\n")
            want = np_profile(one, k, keys, counts)
            assert (want[max(e - k + 1, 0):e + 1] == NO).all()
            assert np.array_equal(dev_profile(dc, one), want), e
            assert np.array_equal(dc.profile(one), want), e
        two = body.copy()    # ... and all of them at once
        two[edges] = ord("\n")
        assert np.array_equal(dev_profile(dc, two), check_twin(two, k, m, keys, counts, seed=3))
        for n in [4096 + d for d in range(-2, 3)] + [4096 + k - 1 + d for d in (-1, 0, 1)] + [8192 + 15, 8192 + 16, 8192 + 17, body.size]:
            want = np_profile(body[:n], k, keys, counts)
            assert np.array_equal(want[:n - k + 1], full[:n - k + 1])
            for shift in (0, 1, 4, 15):
                assert np.array_equal(dev_profile(dc, body[:n], shift=shift), want), (n, shift)
        for start in range(0, 18):   # the data at every alignment of its first byte
            want = np_profile(body[start:], k, keys, counts)
            assert np.array_equal(dev_profile(dc, body[start:], shift=0), want), start


# ---- host form against device form -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,minq", [(21, None), (31, 20), (2, None)])
def test_host_form_equals_device_form_in_chunks(k, minq, monkeypatch):
    bases, qual = O.synth_reads(77, 1 << 18, 150, 0, 2000)
    bases, qual = np.asarray(bases), np.asarray(qual)
    m = O.OracleMap()
    m.process(bases, k, qual=qual if minq is not None else None, min_quality=minq)
    keys, counts = m.arrays()
    q = qual if minq is not None else None
    want = check_twin(bases, k, m, keys, counts, q, minq)
    with native.DeviceCounter(k, min_quality=minq) as dc, native.PinnedArray(bases.size) as pb, native.PinnedArray(bases.size) as pq, \
            native.PinnedArray(bases.size + 64, dtype=np.uint32) as po:
        dc.push(bases, q)
        dev = dev_profile(dc, bases, q)
        assert np.array_equal(dev, want)
        pb.array[:] = bases
        pq.array[:] = qual
        for chunk_kb in ("4", "64", None):
            if chunk_kb is None:
                monkeypatch.delenv("KMERHIP_PROFILE_CHUNK_KB", raising=False)
            else:
                monkeypatch.setenv("KMERHIP_PROFILE_CHUNK_KB", chunk_kb)
            chunk = int(chunk_kb or 1 << 30) << 10
            for shift in range(0, 40 if chunk_kb == "4" else 3):
                # (the chunk edges fall `shift` bytes later in the reads each time: every offset of an edge inside a read and its overlap)
                sb = np.concatenate((np.full(shift, ord("N"), np.uint8), bases))
                sq = None if q is None else np.concatenate((np.full(shift, 255, np.uint8), qual))
                got = dc.profile(sb, sq)
                assert (got[:shift] == NO).all()
                assert np.array_equal(got[shift:], dev), (chunk_kb, shift, np.flatnonzero(got[shift:] != dev)[:8])
                for e in range(chunk, sb.size, chunk):    # the k-1 entries in front of every chunk edge: the overlap
                    assert np.array_equal(got[e - (k - 1):e + k], np.concatenate((np.full(shift, NO, np.uint32), dev))[e - (k - 1):e + k])
            # pinned input and pinned output: no bounce
            po.array[:] = 0x7BADBEEF
            got = dc.profile(pb.array, pq.array if q is not None else None, out=po.array)
            assert np.array_equal(got, dev) and (po.array[bases.size:] == 0x7BADBEEF).all(), chunk_kb
            # pinned input, pageable output and the other way round
            assert np.array_equal(dc.profile(pb.array, pq.array if q is not None else None), dev)
            assert np.array_equal(dc.profile(bases, q, out=po.array), dev)


# ---- table forms --------------------------------------------------------------------------------------------------------------------
def _reads(seed, n):
    b, _ = O.synth_reads(seed, 1 << 20, 150, 0, n, with_qual=False)
    return np.asarray(b)


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("form", ["direct", "partition", "narrow0", "regions3072", "grown"])
def test_table_forms(k, form, monkeypatch):
    # (a table of 2^11 regions, from the hint: the level-1 digit is 10 bits, and the image applies while the 2k - 10 hash bits below
    #  it fit its 32: k <= 21)
    if form == "partition" and k > 21:
        pytest.skip(f"k = {k}: the 8-byte image holds 32 hash bits below the level-1 digit; this table's keys have 2k - 10 = {2 * k - 10}")
    if form == "narrow0":
        monkeypatch.setenv("KMERHIP_NARROW", "0")
    if form == "regions3072":
        monkeypatch.setenv("KMERHIP_TABLE_REGIONS", "3072")
    reads = _reads(300 + k, 6000 if form != "grown" else 12000)
    m = O.OracleMap()
    m.process(reads, k)
    keys, counts = m.arrays()
    query = np.concatenate((reads[:151 * 1500], _reads(900 + k, 500)))
    want = check_twin(query, k, m, keys, counts)
    hint = 0 if form in ("grown", "regions3072") else 3_000_000
    path = {"direct": "direct", "partition": "partition", "narrow0": "partition"}.get(form)
    with native.DeviceCounter(k, capacity_hint=hint, path=path) as dc:
        if form == "grown":
            half = 151 * 6000
            dc.push(reads[:half])
            dc.finish()
            dc.push(reads[half:])
        else:
            dc.push(reads)
        st = dc.finish()
        print(f"k={k} {form}: slot_bytes {st['slot_bytes']} table_slots {st['table_slots']} grows {st['grows']} part_batches {st['part_batches']}")
        if form == "direct":
            assert st["slot_bytes"] == 16 and st["part_batches"] == 0
        if form == "partition":
            assert st["slot_bytes"] == 8 and st["part_batches"] >= 1
        if form == "narrow0":
            assert st["slot_bytes"] == 16 and st["part_batches"] >= 1
        if form == "regions3072":
            assert st["table_slots"] == 3072 * 4096
        if form == "grown" and k >= 16:
            assert st["grows"] >= 1
        got = dev_profile(dc, query)
        assert np.array_equal(got, want), np.flatnonzero(got != want)[:10]
        assert np.array_equal(dc.profile(query), want)
        st2 = dc.finish()
        assert (st2["slot_bytes"], st2["kmers"], st2["distinct"], st2["grows"]) == (st["slot_bytes"], st["kmers"], st["distinct"], st["grows"])


# ---- shards ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nsh", [2, 4])
def test_set_shard_and_merged_pairs_wide(nsh):
    k = 21
    reads = _reads(11, 3000)
    m = O.OracleMap()
    m.process(reads, k)
    keys, counts = m.arrays()
    full = check_twin(reads, k, m, keys, counts)
    import krust_amd
    owners = O.owners(krust_amd, keys, k, nsh)
    total = np.zeros(reads.size, dtype=np.uint64)
    for r in range(nsh):
        with native.DeviceCounter(k, capacity_hint=1_000_000) as dc:
            dc.set_shard(r, nsh)
            dc.merge_pairs(keys[owners == r], counts[owners == r])
            assert dc.finish()["slot_bytes"] == 16
            got = dev_profile(dc, reads)
            assert np.array_equal(got == NO, full == NO)
            mine = np_profile(reads, k, keys[owners == r], counts[owners == r])
            assert np.array_equal(got, mine), "a foreign key's entry is not 0"
            assert np.array_equal(dc.profile(reads), mine)
            total += np.where(got == NO, 0, got).astype(np.uint64)
    assert np.array_equal(total[full != NO], full[full != NO].astype(np.uint64))


@pytest.mark.parametrize("world,k,path,slot_bytes", [(2, 19, "partition", 8), (2, 31, None, 16), (3, 21, None, None)])
def test_shards_after_merge_across(world, k, path, slot_bytes):
    """After kh_merge_across (a group of ranks on one device): hash-range shards as the 8-byte image and as the 16-byte table, and
    the three tables the pairs route leaves.  The sum over the ranks at valid positions is the full-table profile."""
    n_reads = 60_000
    full_b = _reads(21, n_reads)
    m = O.OracleMap()
    m.process(full_b, k)
    keys, counts = m.arrays()
    query = np.concatenate((full_b[:151 * 4000], _reads(99, 500)))
    full = check_twin(query, k, m, keys, counts)
    import krust_amd
    owners = O.owners(krust_amd, keys, k, world)
    per = n_reads // world
    total = np.zeros(query.size, dtype=np.uint64)
    with native.DeviceGroup(k, [0] * world, capacity_hint=3_000_000, path=path) as g:
        for r, dc in enumerate(g.counters):
            lo, hi = r * per, (n_reads if r == world - 1 else (r + 1) * per)
            dc.push(full_b[lo * 151: hi * 151])
        infos = g.merge()
        for r, dc in enumerate(g.counters):
            st = dc.finish()
            print(f"world {world} k={k} rank {r}: {infos[r]['path']}, slot_bytes {st['slot_bytes']}")
            if slot_bytes is not None:
                assert st["slot_bytes"] == slot_bytes
            sel = owners == r
            mine = np_profile(query, k, keys[sel], counts[sel])
            got = dev_profile(dc, query)
            assert np.array_equal(got, mine), (r, np.flatnonzero(got != mine)[:10])
            assert np.array_equal(dc.profile(query), mine)
            assert dc.finish()["slot_bytes"] == st["slot_bytes"]
            total += np.where(got == NO, 0, got).astype(np.uint64)
    assert np.array_equal(total[full != NO], full[full != NO].astype(np.uint64))
    assert (total[full == NO] == 0).all()


# ---- saturation -----------------------------------------------------------------------------------------------------------------------
def test_counts_saturate_at_fffffffe():
    k = 21
    seqs = [b"ACGTTGCAAGGCTTAACCGGT", b"GGGTTTAAACCCGGGTTTAAC", b"ACACACGTGTGTACACACGTT", b"TTGACCAGTAGGACCATTGAC"]
    given = [(1 << 32) + 5, 0xFFFFFFFE, 0xFFFFFFFD, 7]
    keys = np.array([O.canonical(s)[0] for s in seqs], dtype=np.uint64)
    buf = np.frombuffer(b"\n".join(seqs) + b"\n", dtype=np.uint8).copy()
    with native.DeviceCounter(k) as dc:
        dc.merge_pairs(keys, np.array(given, dtype=np.uint64))
        for got in (dc.profile(buf), dev_profile(dc, buf)):
            starts = got[::22][:4].tolist()
            assert starts == [0xFFFFFFFE, 0xFFFFFFFE, 0xFFFFFFFD, 7], starts
            assert (np.delete(got, np.arange(0, 88, 22)) == NO).all()


# ---- reader behaviour -------------------------------------------------------------------------------------------------------------------
def test_text_stream_survives_and_bad_arguments_leave_the_context_usable():
    k = 21
    reads = _reads(5, 3000)
    m = O.OracleMap()
    m.process(reads, k)
    keys, counts = m.arrays()
    want = check_twin(reads[:151 * 200], k, m, keys, counts)
    with native.DeviceCounter(k) as dc:
        dc.push(reads)
        whole = b"".join(dc.result_text("tsv", piece_bytes=64 << 10))
        before = stats_pair(dc)
        nr, nb = dc.result_text_begin("tsv")
        buf = np.empty(64 << 10, dtype=np.uint8)
        pieces = []
        while True:
            n = dc.result_text_next(buf)
            if n == 0:
                break
            pieces.append(buf[:n].tobytes())
            assert np.array_equal(dc.profile(reads[:151 * 200]), want)           # between two pieces of the stream
            assert np.array_equal(dev_profile(dc, reads[:151 * 200]), want)
        assert len(pieces) > 3 and b"".join(pieces) == whole and len(whole) == nb
        assert stats_pair(dc) == before
        L = native.lib()
        out = np.empty(64, dtype=np.uint32)
        b = np.frombuffer(b"ACGT" * 16, dtype=np.uint8).copy()
        assert L.kh_profile(dc._h, b.ctypes.data, None, 64, None) == native.KH_ERR_BAD_ARG
        assert L.kh_profile(dc._h, None, None, 64, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert L.kh_profile_device(dc._h, None, None, 64, 4096) == native.KH_ERR_BAD_ARG
        assert L.kh_profile_device(dc._h, 4096, None, 64, None) == native.KH_ERR_BAD_ARG
        assert np.array_equal(dc.profile(reads[:151 * 200]), want)               # still usable
        assert stats_pair(dc) == before


def test_pending_text_is_counted_first():
    k = 21
    recs = [bytes(r) for r in np.asarray(_reads(8, 300)).tobytes().split(b"\n") if r]
    text = b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs))
    m = O.count_records(recs, k)
    flat = flat_of(recs)
    want = oracle_profile(flat, k, m, positions=range(0, 4000))
    with native.DeviceCounter(k) as dc:
        dc.push_text(text, "fasta")
        got = dc.profile(flat)           # nothing else called since the push
        assert np.array_equal(got[:4000], want[:4000]) and int(got[0]) >= 1


def test_product_library_once():
    """The same call on the library as it ships (no test switches): a child process that loads libkmerhip.so."""
    child = r"""
import sys, os
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["KMERHIP_LIB"] = "libkmerhip.so"
import numpy as np, torch
import oracle_lib as O
from krust_amd import native
import test_gpu_profile as T
k = 31
b, q = O.synth_reads(3, 1 << 18, 150, 0, 3000)
b, q = np.asarray(b), np.asarray(q)
m = O.OracleMap(); m.process(b, k, qual=q, min_quality=20)
keys, counts = m.arrays()
want = T.check_twin(b, k, m, keys, counts, q, 20)
with native.DeviceCounter(k, min_quality=20) as dc:
    dc.push(b, q)
    assert np.array_equal(dc.profile(b, q), want)
    assert np.array_equal(T.dev_profile(dc, b, q), want)
print("RESULT ok", native.LIB_PATH)
"""
    import sys
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + child], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout and "libkmerhip.so" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---- command line -------------------------------------------------------------------------------------------------------------------------
def _fastq(recs, quals):
    return b"".join(b"@r%d\n%s\n+\n%s\n" % (i, r, q) for i, (r, q) in enumerate(zip(recs, quals)))


def _expected_lines(recs, quals, k, m, minq, fmt):
    lines = []
    for i, (r, q) in enumerate(zip(recs, quals)):
        p = oracle_profile(r, k, m, q if minq is not None else None, minq)[:max(len(r) - k + 1, 0)]
        if fmt == "profile":
            lines.append(" ".join("-" if v == NO else str(v) for v in p.tolist()))
        else:
            v = p[p != NO].astype(np.uint64)
            lines.append("\t".join(str(x) for x in (i, v.size, int((v > 0).sum()), int(v.min()) if v.size else 0, int(v.max()) if v.size else 0, int(v.sum()))))
    return "".join(l + "\n" for l in lines).encode()


@pytest.mark.parametrize("gz", [False, True])
def test_command_line_save_then_query_sequences(tmp_path, gz):
    k, minq = 21, 20
    rng = np.random.default_rng(9)
    b, q = O.synth_reads(31, 1 << 16, 150, 0, 1500)
    split = lambda a: [bytes(x) for x in np.asarray(a).tobytes().split(b"\n")[:-1]]
    recs, quals = split(b), split(q)
    counted, cq = recs[:1000], quals[:1000]
    other = recs[700:] + [b"ACGTN", b"", b"acgtacgtacgtacgtacgtacgtacgtt"]
    oq = quals[700:] + [b"IIIII", b"", b"I" * 29]
    # (the reader drops nothing: an empty FASTQ record is a record)
    src, qry = tmp_path / "counted.fq", tmp_path / ("other.fq.gz" if gz else "other.fq")
    src.write_bytes(_fastq(counted, cq))
    data = _fastq(other, oq)
    qry.write_bytes(gzip.compress(data) if gz else data)
    idx = tmp_path / "idx.kmix"
    r = subprocess.run([BIN, str(k), str(src), "--save", str(idx), "-q"], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr
    m = O.count_records(counted, k)           # (the index was saved without -Q: every k-mer of the file)
    batch = ["--__batch-kb", "64"]   # (hidden, as __parse: several reader batches, ordinals run on across them)
    for fmt in ("summary", "profile"):
        r = subprocess.run([BIN, "query", str(idx), "--sequences", str(qry), "-Q", str(minq), "-f", fmt, "-q", *batch], capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr
        want = _expected_lines(other, oq, k, m, minq, fmt)
        assert r.stdout == want, (fmt, r.stdout[:300], want[:300])
    # the default format is the summary; the banner follows the counting command's rules
    r = subprocess.run([BIN, "query", str(idx), "--sequences", str(qry), *batch], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == _expected_lines(other, oq, k, m, None, "summary")
    assert b"input-format: fastq (auto-detected)" in r.stderr and b"output-format: summary" in r.stderr
    assert (len(data) > 3 * (64 << 10))
