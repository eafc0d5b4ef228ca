"""kh_profile_records / kh_profile_records_device -- the profile of new sequences reduced per record on the device -- against the oracle.

The definition is the whole contract: with P what kh_profile* writes for the same bases, row r is the reduction over
P[rec_start[r] : rec_start[r + 1]] (tests/profile_expect.py: rows_of, numpy over the oracle's profile).  Small inputs take P
entry by entry from the oracle primitives; inputs at size take the numpy twin, checked against the primitives first.  All 8
words of every row are compared."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import profile_expect as E
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAT, NO, NONE = E.SAT, E.NO, E.NONE
KS = [1, 2, 5, 11, 16, 17, 21, 25, 31, 32]
RANGES = [(0, SAT), (1, 1), (2, SAT), (5, 3)]
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
GUARD = 0x7BADBEEF


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def dirty_records(seed, k, n=40, maxlen=120):
    """N runs, lower case, IUPAC codes, a CR at a line end, and records of length k-1, k, k+1."""
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTacgtNRYKMn", dtype=np.uint8)
    p = np.array([.2, .2, .2, .2, .03, .03, .03, .03, .02, .01, .01, .01, .02, .01])
    recs = [alpha[rng.choice(alpha.size, size=int(rng.integers(1, maxlen)), p=p / p.sum())].tobytes() for _ in range(n)]
    clean = lambda m: ACGT[rng.integers(0, 4, size=m)].tobytes()
    recs += [clean(max(k - 1, 1)), clean(k), clean(k + 1), clean(40) + b"NNNNNNNN" + clean(50), clean(30) + b"\r", b"N" * 20, b""]
    order = rng.permutation(len(recs))
    return [recs[i] for i in order]


def flat_of(recs):
    return np.frombuffer(b"".join(r + b"\n" for r in recs), dtype=np.uint8).copy()


def quals_for(rng, recs, filler_every=3):
    out = []
    for i, r in enumerate(recs):
        if i % filler_every == 0:
            out.append(b"\xff" * len(r))
        else:
            out.append(bytes(rng.choice(np.array([33, 35, 40, 52, 53, 54, 73, 125, 126, 127, 200, 254, 255], dtype=np.uint8), size=len(r))))
    return out


def reads(seed, n):
    b, _ = O.synth_reads(seed, 1 << 20, 150, 0, n, with_qual=False)
    return np.asarray(b)


# ---- the two forms ------------------------------------------------------------------------------------------------------------
def dev_rows(dc, flat, rs, qual=None, lo=1, hi=SAT, shift=5, row_shift=0):
    """kh_profile_records_device on torch tensors: the bases at an odd offset of their allocation, the rows between guard words
    (row_shift words into theirs: 0 = 16-byte aligned rows, 1 and 3 = rows at 4 mod 8, 2 = rows at 8 mod 16)."""
    import torch
    n, nrec = len(flat), len(rs) - 1
    tb = torch.zeros(n + shift + 64, dtype=torch.uint8, device="cuda:0")
    tb[shift:shift + n] = torch.from_numpy(np.ascontiguousarray(flat))
    tq = None
    if qual is not None:
        tq = torch.zeros(n + shift + 3 + 64, dtype=torch.uint8, device="cuda:0")
        tq[shift + 3:shift + 3 + n] = torch.from_numpy(np.ascontiguousarray(qual))
    trs = torch.from_numpy(np.ascontiguousarray(rs, dtype=np.uint64).view(np.int64)).to("cuda:0")
    pad = 8 + row_shift
    to = torch.full((nrec * 8 + 2 * pad,), GUARD, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    dc.profile_records_device(tb.data_ptr() + shift, None if tq is None else tq.data_ptr() + shift + 3, n, trs, nrec,
                              to.data_ptr() + 4 * pad, lo=lo, hi=hi)
    res = to.cpu().numpy().view(np.uint32)
    assert (res[:pad] == GUARD).all() and (res[pad + nrec * 8:] == GUARD).all(), "kh_profile_records_device wrote outside its nrec rows"
    return res[pad:pad + nrec * 8].reshape(nrec, 8).copy()


def both_forms(dc, flat, rs, want, qual=None, lo=1, hi=SAT, label=None, **kw):
    got_d = dev_rows(dc, flat, rs, qual, lo, hi, **kw)
    bad = np.flatnonzero((got_d != want).any(axis=1))
    assert bad.size == 0, ("device", label, lo, hi, bad[:5], got_d[bad[:3]], want[bad[:3]], np.asarray(rs)[bad[:3]])
    got_h = dc.profile_records(flat, rs, qual, lo=lo, hi=hi)
    bad = np.flatnonzero((got_h != want).any(axis=1))
    assert bad.size == 0, ("host", label, lo, hi, bad[:5], got_h[bad[:3]], want[bad[:3]], np.asarray(rs)[bad[:3]])
    return got_d


def stats_pair(dc):
    st = dc.finish()
    return st["kmers"], st["distinct"], st["slot_bytes"]


# ---- 1. every k -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_every_k_dirty_records_both_forms(k):
    counted = dirty_records(1000 + k, k)
    query = counted[::2] + dirty_records(2000 + k, k, n=25)
    fq = flat_of(query)
    rs = E.starts_of(fq)
    assert rs.size - 1 == len(query)
    m = O.count_records(counted, k)
    P = E.oracle_profile(fq, k, m)
    with native.DeviceCounter(k) as dc:
        dc.push(flat_of(counted))
        before = stats_pair(dc)
        for lo, hi in RANGES:
            want = E.rows_of(P, rs, lo, hi)
            assert np.array_equal(want, E.rows_of_slow(P, rs, lo, hi))
            both_forms(dc, fq, rs, want, lo=lo, hi=hi, label=k)
        assert stats_pair(dc) == before


# ---- 2. edges ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def body21():
    """Six tiles of one ACGT run with a few N, the table it was counted into (with a repeat, so that counts differ), and its
    profile from the checked twin."""
    k = 21
    rng = np.random.default_rng(7)
    body = ACGT[rng.integers(0, 4, size=6 * 4096 + 200)].copy()
    body[9000:9003] = ord("N")
    body[20000:21000] = body[1000:2000]      # counts of 2
    m = O.count_records(bytes(body).split(b"N"), k)
    keys, counts = m.arrays()
    P = E.check_twin(body, k, m, keys, counts)
    return k, body, P


def _edge_offsets(k, n):
    vals = set()
    for base in (0, 4096, 8192):
        for d in (15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, 4096 + k):
            vals.add(base + d)
    return sorted(v for v in vals if v <= n)


def test_edges_starts_and_lengths_around_16_64_4096(body21):
    k, body, P = body21
    with native.DeviceCounter(k) as dc:
        dc.push(body)
        offs = _edge_offsets(k, body.size)
        # segments cut at arbitrary places inside ACGT runs: consecutive records between the offsets, rec_start[0] > 0 and
        # rec_start[nrec] < n
        rs = np.array(offs, dtype=np.uint64)
        assert rs[0] > 0 and rs[-1] < body.size
        for lo, hi in RANGES:
            both_forms(dc, body, rs, E.rows_of(P, rs, lo, hi), lo=lo, hi=hi, label="cuts")
        # every length at every start, one record per call pair (start, start + length), with empty records around it
        for s in (15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, 4096 + k):
            ends = sorted({s + L for L in (15, 16, 17, 63, 64, 65, 4095, 4096, 4097, 4096 + k - 2, 4096 + k - 1, 4096 + k)})
            rs = np.array([s, s] + ends + [ends[-1]], dtype=np.uint64)
            both_forms(dc, body, rs, E.rows_of(P, rs, 2, SAT), lo=2, hi=SAT, label=("start", s))
        # rows at 4 mod 8: the sum is accumulated one word behind its place; rows at 8 mod 16: in place, but with 4-byte stores
        rs = np.array(offs, dtype=np.uint64)
        for row_shift in (1, 2, 3):
            got = dev_rows(dc, body, rs, lo=2, hi=SAT, row_shift=row_shift)
            assert np.array_equal(got, E.rows_of(P, rs, 2, SAT)), row_shift


def test_offsets_that_are_not_ascending_write_nothing_but_their_rows(body21):
    """The device form does not read the offsets back.  Offsets that break its contract give unspecified rows and nothing else:
    here 128 records all reach over one tile's whole run (far more long parts than a tile of ascending records can have), and many
    short ones overlap.  The guard words around the rows stay, and the next call on the context is right."""
    k, body, P = body21
    m = O.count_records(bytes(body).split(b"N"), k)
    keys, counts = m.arrays()
    with native.DeviceCounter(k) as dc:
        dc.merge_pairs(keys, counts)
        saw = np.tile(np.array([0, 4096], dtype=np.uint64), 129)[:257]
        saw[2::2] = 1                                            # {0, 4096, 1, 4096, 1, ...}
        zig = np.tile(np.array([5000, 4100, 9000, 8200, 8190, 12288, 0], dtype=np.uint64), 60)
        for rs in (saw, zig):
            for row_shift in (0, 1, 2):
                dev_rows(dc, body, rs, row_shift=row_shift)      # (asserts the guards)
        rs = np.array([0, 100, 4096, 4097, 13000, body.size], dtype=np.uint64)
        both_forms(dc, body, rs, E.rows_of(P, rs, 1, SAT), label="after bad offsets")


def test_edges_one_record_over_tiles_many_one_base_records_and_empty_runs(body21):
    k, body, P = body21
    n = body.size
    with native.DeviceCounter(k) as dc:
        dc.push(body)
        # one record over more than 3 tiles, between short ones
        rs = np.array([0, 100, 100 + 3 * 4096 + 500, n - 50], dtype=np.uint64)
        for lo, hi in RANGES:
            both_forms(dc, body, rs, E.rows_of(P, rs, lo, hi), lo=lo, hi=hi, label="long")
        # 5,000 one-base records (well over 2,000 parts in one tile), then the rest as one record
        rs = np.concatenate((np.arange(300, 5301), [n])).astype(np.uint64)
        want = E.rows_of(P, rs, 2, SAT)
        assert (want[:5000, E.WINDOWS] == 1).all()
        both_forms(dc, body, rs, want, lo=2, hi=SAT, label="one-base")
        # runs of empty records: 700 at one place in front, 300 in the middle of a tile, 1000 at the end
        rs = np.concatenate((np.full(700, 40), [40, 5000], np.full(300, 5000), [5000, 9001, 9001, 9002], np.full(1000, 16000))).astype(np.uint64)
        want = E.rows_of(P, rs, 1, SAT)
        assert (want[:700] == [0, 0, 0, 0, 0, 0, 0, NONE]).all()
        both_forms(dc, body, rs, want, label="empty runs")
        # misaligned bases
        rs = np.array(_edge_offsets(k, n), dtype=np.uint64)
        for shift in (0, 1, 4, 15, 16):
            assert np.array_equal(dev_rows(dc, body, rs, shift=shift), E.rows_of(P, rs, 1, SAT)), shift
        # the tail: a record that ends at n, where the last k - 1 entries are no windows
        rs = np.array([n - 300, n - k, n], dtype=np.uint64)
        want = E.rows_of(P, rs, 1, SAT)
        assert want[1, E.WINDOWS] == 1
        both_forms(dc, body, rs, want, label="tail")


# ---- 3. table forms and shards -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["direct", "partition"])
def test_table_forms(form):
    k = 21
    rd = reads(300 + k, 6000)
    m = O.OracleMap()
    m.process(rd, k)
    keys, counts = m.arrays()
    query = np.concatenate((rd[:151 * 1000], reads(900 + k, 300)))
    P = E.check_twin(query, k, m, keys, counts)
    rs = E.starts_of(query)
    with native.DeviceCounter(k, capacity_hint=3_000_000, path=form) as dc:
        dc.push(rd)
        st = dc.finish()
        assert st["slot_bytes"] == (16 if form == "direct" else 8) and (st["part_batches"] >= 1) == (form == "partition")
        for lo, hi in ((1, SAT), (2, 3)):
            both_forms(dc, query, rs, E.rows_of(P, rs, lo, hi), lo=lo, hi=hi, label=form)
        assert dc.finish()["slot_bytes"] == st["slot_bytes"]


def test_shard_tables_of_two():
    k = 21
    rd = reads(11, 3000)
    m = O.OracleMap()
    m.process(rd, k)
    keys, counts = m.arrays()
    full = E.rows_of(E.check_twin(rd, k, m, keys, counts), E.starts_of(rd), 1, SAT)
    rs = E.starts_of(rd)
    import krust_amd
    owners = O.owners(krust_amd, keys, k, 2)
    parts = []
    for r in range(2):
        with native.DeviceCounter(k, capacity_hint=1_000_000) as dc:
            dc.set_shard(r, 2)
            dc.merge_pairs(keys[owners == r], counts[owners == r])
            mine = E.rows_of(E.np_profile(rd, k, keys[owners == r], counts[owners == r]), rs, 1, SAT)
            parts.append(both_forms(dc, rd, rs, mine, label=("shard", r)))
    assert np.array_equal(parts[0][:, E.WINDOWS], parts[1][:, E.WINDOWS]) and np.array_equal(parts[0][:, E.WINDOWS], full[:, E.WINDOWS])
    assert np.array_equal(parts[0][:, E.PRESENT] + parts[1][:, E.PRESENT], full[:, E.PRESENT])
    s = lambda rows: rows[:, E.SUM_LO].astype(np.uint64) | (rows[:, E.SUM_HI].astype(np.uint64) << np.uint64(32))
    assert np.array_equal(s(parts[0]) + s(parts[1]), s(full))


# ---- 4. quality ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("minq", [0, 20, 93, 94, 255])
def test_quality_thresholds_with_the_filler(minq):
    k = 11
    rng = np.random.default_rng(50 + minq)
    counted = dirty_records(61, k)
    query = counted + dirty_records(62, k, n=20)
    cq, qq = quals_for(rng, counted), quals_for(rng, query)
    fq, q = flat_of(query), flat_of(qq)
    rs = E.starts_of(fq)
    m = O.count_records(counted, k, quals=cq, min_quality=minq)
    P = E.oracle_profile(fq, k, m, q, minq)
    with native.DeviceCounter(k, min_quality=minq) as dc:
        dc.push(flat_of(counted), flat_of(cq))
        both_forms(dc, fq, rs, E.rows_of(P, rs, 1, SAT), qual=q, label=minq)
    if minq == 20:   # a context without min_quality ignores qual
        m0 = O.count_records(counted, k)
        P0 = E.oracle_profile(fq, k, m0)
        assert not np.array_equal(P0, P)
        with native.DeviceCounter(k) as dc:
            dc.push(flat_of(counted))
            both_forms(dc, fq, rs, E.rows_of(P0, rs, 1, SAT), qual=q, label="no threshold")


# ---- 5. saturation --------------------------------------------------------------------------------------------------------------------
def test_saturated_counts_max_and_the_high_word_of_the_sum():
    k = 21
    rec = b"ACGTTGCAAGGCTTAACCGGTAGT"          # four windows
    wins = [rec[i:i + k] for i in range(4)]
    keys = np.array([O.canonical(w)[0] for w in wins], dtype=np.uint64)
    assert np.unique(keys).size == 4
    given = np.array([(1 << 32) + 5, 1 << 40, 0xFFFFFFFF, 7], dtype=np.uint64)
    flat = np.frombuffer(b"ACGT\n" + rec + b"\n" + wins[3] + b"\n", dtype=np.uint8).copy()
    rs = E.starts_of(flat)
    table = dict(zip(keys.tolist(), given.tolist()))
    P = E.oracle_profile(flat, k, table)
    want = E.rows_of(P, rs, 1, SAT)
    assert want[1].tolist() == [4, 4, 4, 7, SAT, (3 * SAT + 7) & 0xFFFFFFFF, (3 * SAT + 7) >> 32, NONE] and want[1, E.SUM_HI] == 3   # 3 * (2^32 - 2) + 7 = 3 * 2^32 + 1
    with native.DeviceCounter(k) as dc:
        dc.merge_pairs(keys, given)
        both_forms(dc, flat, rs, want, label="sat")
        both_forms(dc, flat, rs, E.rows_of(P, rs, SAT, SAT), lo=SAT, hi=SAT, label="sat range")


# ---- 6. the chunked host form -------------------------------------------------------------------------------------------------------------
def test_chunked_host_form_equals_device_form(body21, monkeypatch):
    k, body, P = body21
    n = body.size
    monkeypatch.setenv("KMERHIP_PROFILE_CHUNK_KB", "1")
    # a zero count inside the second chunk of a record that spans more than 3 chunks: first_low (lo = 1) lies there
    body = body.copy()
    body[2048 + 600: 2048 + 600 + 25] = np.frombuffer(b"GATTACAGATTACAGATTACACCCC", dtype=np.uint8)   # not counted
    rng = np.random.default_rng(3)
    cuts = np.sort(rng.choice(np.arange(6000, n), size=400, replace=False))
    rs = np.concatenate(([1500, 1500 + 3 * 1024 + 700], cuts)).astype(np.uint64)
    rs = np.unique(rs)
    assert rs[0] == 1500 and rs[1] > 1500 + 3 * 1024
    with native.DeviceCounter(k) as dc, native.PinnedArray(n) as pb:
        m = O.count_records(bytes(body21[1]).split(b"N"), k)
        keys, counts = m.arrays()
        P2 = E.check_twin(body, k, m, keys, counts)
        dc.merge_pairs(keys, counts)
        for lo, hi in ((1, SAT), (2, SAT)):
            want = E.rows_of(P2, rs, lo, hi)
            if lo == 1:
                assert 2048 - 1500 <= want[0, E.FIRST_LOW] < 3072 - 1500, want[0]      # inside the record's second chunk
            dev = both_forms(dc, body, rs, want, lo=lo, hi=hi, label="chunks")
            pb.array[:] = body
            assert np.array_equal(dc.profile_records(pb.array, rs, lo=lo, hi=hi), dev)   # kh_host_alloc memory: no bounce
            for shift in (1, 7, 20, 21, 22):       # the chunk edges at other places of the records
                sb = np.concatenate((np.full(shift, ord("N"), np.uint8), body))
                assert np.array_equal(dc.profile_records(sb, rs + np.uint64(shift), lo=lo, hi=hi), dev), shift


# ---- 7. a workgroup with more than one tile -----------------------------------------------------------------------------------------------
def test_more_tiles_than_workgroups():
    k = 21
    nbytes = 2048 * 4096 + 3 * 4096
    nreads = nbytes // 151 + 1
    rd = reads(5, nreads)[:nbytes].copy()
    # 2052 tiles on workgroups of 2 tiles each: every 8192 entries lies an edge between two workgroups' ranges
    s = (10 * 8192 - 9000) // 151 * 151
    rd[s:s + 19999] = ACGT[np.random.default_rng(1).integers(0, 4, size=19999)]
    rd[s + 19999] = 10
    m = O.OracleMap()
    m.process(rd[:151 * 20000], k)
    keys, counts = m.arrays()
    P = E.check_twin(rd, k, m, keys, counts)
    rs = E.starts_of(rd)
    i = int(np.searchsorted(rs, s))
    assert rs[i] == s and rs[i + 1] == s + 20000 and s < 10 * 8192 < 11 * 8192 < s + 20000
    want = E.rows_of(P, rs, 1, SAT)
    with native.DeviceCounter(k, capacity_hint=4_000_000) as dc:
        dc.merge_pairs(keys, counts)
        both_forms(dc, rd, rs, want, label="grid cap")


# ---- 8. contract ----------------------------------------------------------------------------------------------------------------------------
def test_contract_stream_bad_arguments_and_empty_calls():
    k = 21
    rd = reads(5, 3000)
    m = O.OracleMap()
    m.process(rd, k)
    keys, counts = m.arrays()
    q = rd[:151 * 200]
    rs = E.starts_of(q)
    want = E.rows_of(E.check_twin(q, k, m, keys, counts), rs, 1, SAT)
    import torch
    with native.DeviceCounter(k) as dc:
        dc.push(rd)
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
            if len(pieces) <= 3:
                first = both_forms(dc, q, rs, want, label="in a stream")
        assert len(pieces) > 3 and b"".join(pieces) == whole and len(whole) == nb
        assert stats_pair(dc) == before
        assert np.array_equal(dc.profile_records(q, rs), first)          # two calls: identical rows
        L = native.lib()
        BAD = native.KH_ERR_BAD_ARG
        rows = np.full(rs.size * 8 + 8, GUARD, dtype=np.uint32)
        call = lambda b, n, r, nrec, o: L.kh_profile_records(dc._h, b, None, n, r, nrec, 1, SAT, o)
        bp, rp, op = q.ctypes.data, rs.ctypes.data, rows.ctypes.data
        nrec = rs.size - 1
        assert call(None, q.size, rp, nrec, op) == BAD
        assert call(bp, q.size, None, nrec, op) == BAD
        assert call(bp, q.size, rp, nrec, None) == BAD
        assert call(bp, q.size, rp, nrec, rows.view(np.uint8)[2:].ctypes.data) == BAD                    # rows not 4-byte aligned
        down = rs.copy()
        down[5], down[6] = rs[6], rs[5]
        assert call(bp, q.size, down.ctypes.data, nrec, op) == BAD                                       # not ascending
        assert call(bp, q.size - 1, rp, nrec, op) == BAD                                                 # rec_start[nrec] > n
        huge = np.array([0, 1 << 32], dtype=np.uint64)
        assert call(bp, q.size, huge.ctypes.data, 1, op) == BAD                                          # (also beyond n)
        assert (rows == GUARD).all()
        dev = lambda b, n, r, nrec, o: L.kh_profile_records_device(dc._h, b, None, n, r, nrec, 1, SAT, o)
        assert dev(None, 64, 4096, 1, 4096) == BAD and dev(4096, 64, None, 1, 4096) == BAD and dev(4096, 64, 4096, 1, None) == BAD
        assert dev(4096, 64, 4096, 1, 4098) == BAD
        assert np.array_equal(dc.profile_records(q, rs), first)          # still usable
        # nrec == 0 writes nothing; n == 0 writes nrec empty rows
        assert call(bp, q.size, rp, 0, op) == 0 and call(None, 0, None, 0, None) == 0 and dev(None, 0, None, 0, None) == 0
        assert (rows == GUARD).all()
        zeros = np.zeros(4, dtype=np.uint64)
        assert call(None, 0, zeros.ctypes.data, 3, op) == 0
        assert (rows[:24].reshape(3, 8) == [0, 0, 0, 0, 0, 0, 0, NONE]).all() and (rows[24:] == GUARD).all()
        tz = torch.zeros(4, dtype=torch.int64, device="cuda:0")
        to = torch.full((40,), GUARD, dtype=torch.int32, device="cuda:0")
        assert dev(None, 0, tz.data_ptr(), 3, to.data_ptr() + 32) == 0
        r = to.cpu().numpy().view(np.uint32)
        assert (r[8:32].reshape(3, 8) == [0, 0, 0, 0, 0, 0, 0, NONE]).all() and (r[:8] == GUARD).all() and (r[32:] == GUARD).all()
        assert stats_pair(dc) == before


# ---- 9. the product library ----------------------------------------------------------------------------------------------------------------
def test_product_library_once():
    """One case of (1) on the library as it ships (no test switches): a child process that loads libkmerhip.so."""
    child = r"""
import sys, os
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["KMERHIP_LIB"] = "libkmerhip.so"
import numpy as np, torch
import oracle_lib as O
import profile_expect as E
from krust_amd import native
import test_gpu_profile_records as T
k = 31
counted = T.dirty_records(1000 + k, k)
query = counted[::2] + T.dirty_records(2000 + k, k, n=25)
fq = T.flat_of(query)
rs = E.starts_of(fq)
P = E.oracle_profile(fq, k, O.count_records(counted, k))
with native.DeviceCounter(k) as dc:
    dc.push(T.flat_of(counted))
    for lo, hi in T.RANGES:
        T.both_forms(dc, fq, rs, E.rows_of(P, rs, lo, hi), lo=lo, hi=hi, label="product")
print("RESULT ok", native.LIB_PATH)
"""
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + child], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout and "libkmerhip.so" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
