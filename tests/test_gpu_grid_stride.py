"""Every capped-grid kernel past its first grid stride.

A kernel that scans a table, a text or an array is launched on at most GRID_CAP = 2048 workgroups (ctx.hip.h: grid_for(), and the
launches of input.hip, batch.hip, join.hip, graph.hip and profile.hip that size their own grid) and covers the rest with a
grid-stride loop.  What a workgroup keeps from one trip of that loop to the next -- LDS queues and histograms, the barriers
that protect their reuse, prefetched tiles, accumulators flushed behind the loop -- is live only past 2048 tiles, which the suite's
small shapes never reach.  Sections 1-9 run under KMERHIP_GRID_CAP = 1 and 3 (test build): 1 sends one workgroup round its loop
as often as there are tiles, 3 divides no tile count here, so the workgroups make unequal numbers of trips.  Section 10 runs the
product library, whose cap is the constant, at sizes that really cross 2048 tiles.

Expected values never come from the library: they are the references the neighbouring files use (the oracle, numpy over its
counts, the Python line parsers of test_gpu_text, the string walk of test_gpu_unitigs), imported as namespaces.  Every case first
asserts, from its shape and the tile constants alone, that the loop under test makes at least three trips at cap 1 and two at cap 3.

Run with `pytest -m gpu` on an MI355X."""
import os
import subprocess
import sys
from collections import Counter

import numpy as np
import pytest

import oracle_lib as O
import profile_expect as E
import test_gpu_format as FM
import test_gpu_graph as G
import test_gpu_join as J
import test_gpu_profile as PF
import test_gpu_profile_records as PR
import test_gpu_readside as RS
import test_gpu_sorted as SO
import test_gpu_text as TX
import test_gpu_unitigs as UN
import krust_amd
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
NCPU = max(1, min(os.cpu_count() or 1, 16))
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)

# what one workgroup takes per trip of its loop (the constants of the kernels' sources)
BLOCK = 256                 # kernels.hip.h: lanes per workgroup = items per trip of an item-strided kernel
RAW_TILE = 16 * BLOCK       # rawparse.hip.h: bytes of text per tile; kernels.hip.h / profile.hip: positions per tile
COMPACT_TILE = 16 * BLOCK   # kernels.hip.h COMPACT_PER x BLOCK slots
JOIN_TILE = 8 * BLOCK       # join.hip JOIN_PER x BLOCK slots
GRAPH_TILE = 4 * BLOCK      # graph.hip GRAPH_PER x BLOCK slots (stats) / keys (masks)
FMT_TILE = 2 * BLOCK        # format.hip.h slots (or sorted pairs) per tile
SLOTS_DEFAULT = 1 << 20     # a table without a capacity hint
SLOTS_HINT = 1 << 23        # capacity_hint = 3 000 000: 2^11 regions, what the 8-byte image needs at k = 21
HINT = 3_000_000


@pytest.fixture(params=[1, 3], ids=["cap1", "cap3"])
def cap(request, monkeypatch):
    """KMERHIP_GRID_CAP for the contexts the test creates from here on (the test build reads it at kh_create and at every call).
    The value is the process's, not a context's: afterwards one kh_create without the variable puts it back to 2048, whatever runs
    next (kh_synth_reads_device, for one, takes no context)."""
    monkeypatch.setenv("KMERHIP_GRID_CAP", str(request.param))
    yield request.param
    monkeypatch.delenv("KMERHIP_GRID_CAP")
    native.DeviceCounter(21).close()


def trips(items, per_trip, cap):
    """Trips of workgroup 0 round its loop over `items` items, `per_trip` per workgroup and trip, on a grid of at most `cap`."""
    tiles = -(-int(items) // per_trip)
    return -(-tiles // min(cap, tiles))


def goes_round(items, per_trip, cap):
    t = trips(items, per_trip, cap)
    assert t >= (3 if cap == 1 else 2), (items, per_trip, cap, t)
    return t


def rnd(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


# ---- 1. text scan ------------------------------------------------------------------------------------------------------------------
PAD_TILES = 7   # 7 x 4096 > 2 x 4096 x 3: whatever follows lies in a later trip of its workgroup, at cap 1 and at cap 3


def padded(text):
    """A record of exactly PAD_TILES tiles in front of a FASTA text: its bytes keep their place inside units and tiles."""
    rng = np.random.default_rng(len(text))
    head = b">pad\n"
    pad = head + TX.rand_seq(rng, PAD_TILES * RAW_TILE - len(head) - 1) + b"\n"
    assert len(pad) == PAD_TILES * RAW_TILE
    return pad + text


def check_fasta(text, cap, ks=(4, 21)):
    goes_round(len(text), RAW_TILE, cap)
    assert len(text) > 2 * RAW_TILE * cap
    for k in ks:
        assert TX.device(text, "fasta", k, None) == TX.expect(text, "fasta", k, None), k


@pytest.mark.parametrize("name", sorted(TX._FASTA_UNIT_CASES))
def test_fasta_unit_cases(cap, name):
    check_fasta(padded(TX._FASTA_UNIT_CASES[name]), cap)


@pytest.mark.parametrize("seed", range(6))
def test_fasta_random_layouts(cap, seed):
    """Line and header lengths from 0 to several units, LF or CR LF, '>' inside lines, empty records, with or without the final
    line end (the shapes of test_gpu_text's random layouts)."""
    rng = np.random.default_rng(9100 + seed)
    eol = b"\r\n" if seed % 3 == 0 else b"\n"
    out = []
    for r in range(int(rng.integers(10, 60))):
        hl = int(rng.choice([0, 1, 7, 15, 16, 17, 60, 300, 1023, 1024, 5000])) if rng.random() < 0.5 else int(rng.integers(0, 200))
        out.append(b">" + TX.rand_seq(rng, hl, alphabet=b"ACGT >xyz|0123") + eol)
        for _ in range(int(rng.integers(0, 12))):
            ll = int(rng.choice([0, 1, 15, 16, 17, 60, 61, 70, 1023, 1024, 1025, 4095, 4096, 9000])) if rng.random() < 0.4 else int(rng.integers(1, 120))
            line = bytearray(TX.rand_seq(rng, ll))
            if ll > 3 and rng.random() < 0.1:
                line[int(rng.integers(1, ll))] = ord(">")
            out.append(bytes(line) + eol)
    text = b"".join(out)
    if seed % 2 and text.endswith(eol):
        text = text[: -len(eol)]
    check_fasta(padded(text), cap)


@pytest.mark.parametrize("k,minq", [(21, 20), (1, None)], ids=["k21-q20", "k1"])
@pytest.mark.parametrize("eol", [b"\n", b"\r\n"], ids=["lf", "crlf"])
def test_fastq_ragged_records(cap, eol, k, minq):
    nrec = 1000
    text = TX.make_fastq(np.random.default_rng(17), nrec, 0, 260, eol=eol)
    goes_round(len(text), RAW_TILE, cap)     # raw_nl_count / raw_line_starts / fastq_mark: by tile
    goes_round(nrec, BLOCK, cap)             # fastq_validate_kernel: by record
    assert TX.device(text, "fastq", k, minq) == TX.expect(text, "fastq", k, minq)


@pytest.mark.parametrize("where", ["last-trip", "trips-behind"])
@pytest.mark.parametrize("what", ["no-plus", "lengths"])
def test_fastq_refusal_in_a_later_trip(cap, what, where):
    """last-trip: the bad record's lane meets it in its last trip.  trips-behind: the lane makes further trips behind it -- what it
    found is carried to the end of its loop (at cap 1 the record is in the second of four trips; with two trips at cap 3, the first)."""
    rng = np.random.default_rng(23)
    nrec, stride = 1000, BLOCK * cap
    at = 800 + cap if where == "last-trip" else (300 if cap == 1 else 200)
    if where == "last-trip":
        assert at >= 800 and at // stride >= 1 and at + stride >= nrec
    else:
        assert at + stride < nrec and (cap != 1 or (at // stride >= 1 and at + 2 * stride < nrec))
    bad = {"no-plus": b"@r\nACGT\n-\nIIII\n", "lengths": b"@r\nACGT\n+\nIII\n"}[what]
    text = TX.make_fastq(rng, at, 0, 260) + bad + TX.make_fastq(rng, nrec - at - 1, 0, 260)
    goes_round(nrec, BLOCK, cap)
    TX._format_error(text, "fastq")


@pytest.mark.parametrize("what", ["space-lf", "tab-crlf", "bare-cr"])
def test_fasta_refusal_in_a_later_trip(cap, what):
    rng = np.random.default_rng(29)
    tile = 4 + cap
    at = tile * RAW_TILE + 1000
    head = b">r\n"
    tail = {"space-lf": b" \n", "tab-crlf": b"\t\r\n", "bare-cr": b"\rA"}[what]
    body = b"".join(TX.rand_seq(rng, 70, alphabet=b"ACGT") + b"\n" for _ in range(at // 71 + 1))[: at - len(head) - 10]
    text = head + body + TX.rand_seq(rng, 10, alphabet=b"ACGT") + tail + TX.rand_seq(rng, 9000, alphabet=b"ACGT") + b"\n"
    assert text[at] == tail[0] and at // RAW_TILE >= 4 and (at // RAW_TILE) // cap >= 1
    goes_round(len(text), RAW_TILE, cap)
    # the same text without the offending byte is accepted: the refusal is this byte's
    ok = text[:at] + text[at + 1:]
    assert TX.device(ok, "fasta", 5, None) == TX.expect(ok, "fasta", 5, None)
    TX._format_error(text, "fasta")


# ---- 2. direct count -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,minq", [(21, None), (31, 20)], ids=["k21", "k31-q20"])
def test_direct_count_of_ragged_dirty_records(cap, k, minq):
    recs = PF.dirty_records(500 + k, k, n=1000, maxlen=120)
    quals = PF.quals_for(np.random.default_rng(k), recs) if minq is not None else None
    flat = PF.flat_of(recs)
    assert 50_000 < flat.size < 80_000
    goes_round(flat.size, RAW_TILE, cap)
    want = O.count_records(recs, k, quals=quals, min_quality=minq).as_dict()
    assert len(want) > 200
    with native.DeviceCounter(k, min_quality=minq, path="direct") as dc:
        dc.push(flat, PF.flat_qual(quals) if quals is not None else None)
        st = dc.finish()
        assert st["part_batches"] == 0 and st["slot_bytes"] == 16 and st["table_slots"] == SLOTS_DEFAULT
        assert st["kmers"] == sum(want.values()) and st["distinct"] == len(want)
        assert dc.as_dict() == want


# ---- 3. table readers and writers through grid_for ---------------------------------------------------------------------------------
N_PAIRS = 3000
CHOSEN_COUNTS = np.array([1, 2, 3, 2 ** 31, 2 ** 32 + 1], dtype=U64)
_CACHE = {}


def chosen_pairs(k=21):
    if ("pairs", k) not in _CACHE:
        rng = np.random.default_rng(31 + k)
        keys = RS.draw_keys(krust_amd, k, N_PAIRS, rng)
        counts = CHOSEN_COUNTS[rng.integers(0, CHOSEN_COUNTS.size, size=N_PAIRS)]
        assert all(int((counts == c).sum()) > 300 for c in CHOSEN_COUNTS)
        absent = RS.draw_keys(krust_amd, k, N_PAIRS // 2, rng, avoid=keys)
        o = np.argsort(keys)
        _CACHE[("pairs", k)] = (keys[o], counts[o], absent)
    return _CACHE[("pairs", k)]


def image_reads(k=21):
    """2000 synthetic reads and the oracle's pairs (what test_gpu_readside counts on the partition path for its image)."""
    if ("image", k) not in _CACHE:
        bases, _ = O.synth_reads(RS.SEED, 1 << 18, 150, 0, 2000, with_qual=False)
        m = O.OracleMap()
        m.scan_flat(bases, k, nthreads=NCPU)
        keys, counts = m.arrays()
        keys, counts = np.asarray(keys, dtype=U64).copy(), np.asarray(counts, dtype=U64).copy()
        absent = RS.draw_keys(krust_amd, k, N_PAIRS // 2, np.random.default_rng(37), avoid=keys)
        _CACHE[("image", k)] = (np.asarray(bases), keys, counts, absent)
    return _CACHE[("image", k)]


def open_table(form, k=21):
    """(context, sorted keys, counts, absent keys, slots): the chosen pairs merged into a 16-byte table without a hint, or the reads
    counted on the partition path into the 8-byte image (which needs the hint's 2^11 regions at k = 21)."""
    if form == "wide":
        keys, counts, absent = chosen_pairs(k)
        dc = native.DeviceCounter(k)
        dc.merge_pairs(keys[::-1].copy(), counts[::-1].copy())
        st = dc.finish()
        assert st["slot_bytes"] == 16 and st["table_slots"] == SLOTS_DEFAULT and st["distinct"] == keys.size
        return dc, keys, counts, absent, SLOTS_DEFAULT
    bases, keys, counts, absent = image_reads(k)
    dc = native.DeviceCounter(k, capacity_hint=HINT, path="partition")
    dc.push(bases)
    st = dc.finish()
    assert st["slot_bytes"] == 8 and st["part_batches"] >= 1 and st["table_slots"] == SLOTS_HINT and st["distinct"] == keys.size
    return dc, keys, counts, absent, SLOTS_HINT


@pytest.mark.parametrize("form", ["wide", "image"])
def test_size_pairs_sorted_pairs_histogram_and_lookup(cap, form):
    dc, keys, counts, absent, slots = open_table(form)
    with dc:
        goes_round(slots, COMPACT_TILE, cap)      # compact_tiles (result, and the sort's compact_pairs)
        goes_round(slots, BLOCK, cap)             # table_count / table_hist and their ntable_ twins
        if form == "wide":
            goes_round(N_PAIRS, BLOCK, cap)       # table_merge_pairs_kernel
        for mc in (1, 2, 2 ** 32):
            sel = counts >= U64(mc)
            wk, wc = keys[sel], counts[sel]
            assert (form == "image" and mc == 2 ** 32) == (wk.size == 0)
            assert dc.result_size(mc) == wk.size
            gk, gc = dc.result(mc)
            assert np.array_equal(gk, wk) and np.array_equal(gc, wc), mc
            sk, sc = dc.result_sorted(mc)
            assert np.array_equal(sk, wk) and np.array_equal(sc, wc), mc
            assert dc.histogram(mc) == sorted(Counter(wc.tolist()).items()), mc
        rng = np.random.default_rng(41)
        pick = rng.permutation(keys.size)[:N_PAIRS // 2]
        probes = np.concatenate((keys[pick], absent))
        expect = np.concatenate((counts[pick], np.zeros(absent.size, dtype=U64)))
        o = rng.permutation(probes.size)
        assert probes.size == N_PAIRS
        goes_round(probes.size, BLOCK, cap)       # table_lookup_kernel / ntable_lookup_kernel
        assert np.array_equal(dc.lookup(probes[o]), expect[o])
        assert dc.finish()["slot_bytes"] == (16 if form == "wide" else 8)


def table_of(form, k, r, monkeypatch):
    """(context, slots) holding the reads r: the image through J.table (the hint's 2^11 regions are what it needs at k = 21), the
    16-byte table without a hint, at whatever size the library gives it."""
    if form == "image":
        return J.table("image", k, r, monkeypatch), SLOTS_HINT
    dc = native.DeviceCounter(k, path="direct")
    dc.push(r)
    st = dc.finish()
    assert st["slot_bytes"] == 16 and st["part_batches"] == 0 and SLOTS_DEFAULT <= st["table_slots"] < SLOTS_HINT
    return dc, st["table_slots"]


# ---- 4. join ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fa,fb", [("wide", "image"), ("image", "wide")])
def test_compare_and_combine(cap, fa, fb, monkeypatch):
    k = 21
    ra, rb, (u, ca, cb) = J.sample_ab(k)
    (a, sa), (b, sb) = table_of(fa, k, ra, monkeypatch), table_of(fb, k, rb, monkeypatch)
    # (dst takes the union's 1.2 M keys: the hint spares it growing once per case)
    with a, b, native.DeviceCounter(k, capacity_hint=HINT) as dst:
        assert (a.finish()["table_slots"], b.finish()["table_slots"]) == (sa, sb)
        goes_round(sa, JOIN_TILE, cap)            # compare scans a, then b; combine scans a (and b for a union)
        goes_round(sb, JOIN_TILE, cap)
        before = J.stats_of(a), J.stats_of(b)
        J.check_all_ops(a, b, dst, u, ca, cb, 1, 1, cases=[("intersect", "min"), ("union", "sum"), ("subtract", "sum")])
        w = J.np_words(ca, cb, 2, 1)
        assert 0 < w["shared"] < J.np_words(ca, cb)["shared"]
        assert a.compare(b, 2, 1) == w
        assert (J.stats_of(a), J.stats_of(b)) == before


# ---- 5. graph -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["wide", "image"])
def test_graph_stats(cap, form, monkeypatch):
    k = 21
    flat, keys, counts = G.main_input(k)
    dc, slots = table_of(form, k, flat, monkeypatch)
    with dc:
        assert dc.finish()["table_slots"] == slots
        goes_round(slots, GRAPH_TILE, cap)
        for mc in (1, 2):
            got = dc.graph_stats(mc)
            assert np.array_equal(got, G.main_words(k, mc)), (mc, np.flatnonzero(got != G.main_words(k, mc))[:8])


def test_graph_masks_device_alignments_and_canaries(cap):
    import torch
    k, n = 21, 5000
    flat, keys, counts = G.main_input(k)
    rng = np.random.default_rng(43)
    present = keys[rng.permutation(keys.size)[:3000]]
    absent = RS.draw_keys(krust_amd, k, 1500, rng, avoid=keys)
    invalid = np.concatenate((present[:200] | U64(1 << 63), G.np_revcomp(present[200:499], k), np.array([G.ALL], dtype=U64)))
    words = np.concatenate((present, absent, invalid))[rng.permutation(n)]
    assert words.size == n and int((~G.np_valid(words, k)).sum()) > 300
    want = G.np_masks(words, keys, k)
    assert int((want != 0).sum()) > 2500
    dev = torch.device("cuda:0")
    with native.DeviceCounter(k, device=0) as dc:
        dc.push(flat)
        assert dc.finish()["table_slots"] == SLOTS_DEFAULT
        d_keys = torch.from_numpy(words.view(np.int64).copy()).to(dev)
        raw = torch.empty(64 + 16 + n + 64 + 16 + 16, dtype=torch.uint8, device=dev)
        pad = (-raw.data_ptr()) % 16
        for off in range(4):
            goes_round(n + off, GRAPH_TILE, cap)      # a lane takes one group of four bytes: 1024 keys per workgroup and trip
            raw.fill_(0xAB)
            torch.cuda.synchronize()
            start = pad + 64 + off
            assert (raw.data_ptr() + start) % 4 == off
            dc.graph_masks_device(d_keys.data_ptr(), n, raw.data_ptr() + start, 1)
            host = raw.cpu().numpy()
            bad = np.flatnonzero(host[start:start + n] != want)
            assert bad.size == 0, (off, bad[:8])
            assert (host[:start] == 0xAB).all() and (host[start + n:] == 0xAB).all(), off


# ---- 6. unitigs ---------------------------------------------------------------------------------------------------------------------------
UNI_CHAINS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025, 2000]
UNI_PERIODS = [3, 64, 1500]


def unitig_input(k):
    """(flat, keys, counts): disjoint chains, three cycles, the 256 stars of test_gpu_graph, and 1000 reads of a 32 kb sequence with
    one substitution per hundred bases (tips and bubbles)."""
    if ("unitigs", k) not in _CACHE:
        rng = np.random.default_rng(900 + k)
        recs = []
        for i, L in enumerate(UNI_CHAINS):
            s = rnd(rng, L + k - 1)
            recs.append(UN.rc(s) if i % 2 else s)
        for i, p in enumerate(UNI_PERIODS):
            unit = b"ACG" if p == 3 else rnd(rng, p)
            circ = (unit * (k // p + 2))[:p + k - 1]
            recs.append(UN.rc(circ) if i % 2 else circ)
        recs += G.star_records(k)
        genome = np.frombuffer(rnd(rng, 1 << 15), dtype=np.uint8)
        for i in range(1000):
            s = int(rng.integers(0, genome.size - 150))
            read = genome[s:s + 150].copy()
            hit = rng.random(150) < 0.01
            read[hit] = ACGT[(np.searchsorted(ACGT, read[hit]) + rng.integers(1, 4, size=int(hit.sum()))) & 3]
            recs.append(UN.rc(read.tobytes()) if i % 2 else read.tobytes())
        flat = UN.flat_of(recs)
        _CACHE[("unitigs", k)] = (flat,) + UN.oracle_pairs(flat, k)
    return _CACHE[("unitigs", k)]


@pytest.mark.parametrize("k,form", [(21, "wide"), (31, "wide"), (21, "image")], ids=["k21-wide", "k31-wide", "k21-image"])
def test_unitigs_byte_for_byte(cap, k, form):
    flat, keys, counts = unitig_input(k)
    ref = UN.ref_of("grid-stride", keys, counts, k, 1)
    lens = set(int(v) for v in ref.rows[:, native.UNI_KMERS])
    assert set(UNI_CHAINS) <= lens and set(UNI_PERIODS) <= set(int(r[1]) for r in ref.rows if r[3])
    assert ref.rows.shape[0] > 1000 and ref.seen["minus_first"] > 0   # branches cut the reads into many unitigs
    n = keys.size
    goes_round(n, BLOCK, cap)                         # the eleven kernels of unitig.hip stride by node, state or 16 bases
    goes_round(len(ref.bases) // 16, BLOCK, cap)
    slots = SLOTS_HINT if form == "image" else SLOTS_DEFAULT
    goes_round(slots, COMPACT_TILE, cap)              # compact_pairs in front of them
    with native.DeviceCounter(k, capacity_hint=HINT if form == "image" else 0, path="partition" if form == "image" else None) as dc:
        dc.push(flat)
        st = dc.finish()
        assert st["table_slots"] == slots and st["slot_bytes"] == (8 if form == "image" else 16) and st["distinct"] == n
        UN.check_unitigs(dc, "grid-stride", keys, counts, k, 1, ref=ref)


# ---- 7. profile ---------------------------------------------------------------------------------------------------------------------------
def profile_input(k=21):
    """The counted reads, the oracle's map and pairs, a 40 000-base query with N and soft-masked stretches, and 1200 records of 0 .. 300
    bases cut out of it."""
    if ("profile", k) not in _CACHE:
        counted, _ = O.synth_reads(53, 1 << 16, 150, 0, 3000, with_qual=False)
        counted = np.asarray(counted)
        m = O.OracleMap()
        m.process(counted, k)
        keys, counts = m.arrays()
        keys, counts = np.asarray(keys, dtype=U64).copy(), np.asarray(counts, dtype=U64).copy()
        rng = np.random.default_rng(59)
        q = counted[counted != 10][:40_000].copy()        # reads end to end: windows inside a read are present, those across two are not
        assert q.size == 40_000
        for s in rng.integers(0, q.size - 400, size=12):
            q[s:s + int(rng.integers(1, 300))] = ord("N") if rng.random() < 0.5 else q[s:s + 1]   # (an N run, or a homopolymer the table lacks)
        for s in rng.integers(0, q.size - 400, size=12):
            n = int(rng.integers(1, 400))
            q[s:s + n] = np.where(np.isin(q[s:s + n], ACGT), q[s:s + n] | 32, q[s:s + n])           # soft-masked
        recs = []
        for _ in range(1200):
            L = int(rng.integers(0, 301))
            s = int(rng.integers(0, q.size - 300))
            recs.append(q[s:s + L].tobytes())
        _CACHE[("profile", k)] = (counted, m, keys, counts, q, recs)
    return _CACHE[("profile", k)]


def profile_table(form, k, counted):
    dc = native.DeviceCounter(k, capacity_hint=HINT if form == "image" else 0, path="partition" if form == "image" else "direct")
    dc.push(counted)
    st = dc.finish()
    assert st["slot_bytes"] == (8 if form == "image" else 16) and st["table_slots"] == (SLOTS_HINT if form == "image" else SLOTS_DEFAULT)
    return dc


@pytest.mark.parametrize("form", ["wide", "image"])
def test_profile_of_one_long_sequence(cap, form):
    k = 21
    counted, m, keys, counts, q, _ = profile_input(k)
    want = E.check_twin(q, k, m, keys, counts)
    assert int((want == E.NO).sum()) > 500 and int((want == 0).sum()) > 500 and int(((want > 0) & (want != E.NO)).sum()) > 20_000
    goes_round(q.size, RAW_TILE, cap)
    with profile_table(form, k, counted) as dc:
        got = PF.dev_profile(dc, q)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, ("device", bad[:8], got[bad[:8]], want[bad[:8]])
        got = dc.profile(q)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, ("host", bad[:8], got[bad[:8]], want[bad[:8]])


@pytest.mark.parametrize("form", ["wide", "image"])
def test_profile_records(cap, form):
    k = 21
    counted, m, keys, counts, _, recs = profile_input(k)
    fq = PR.flat_of(recs)
    rs = E.starts_of(fq)
    nrec = rs.size - 1
    assert nrec == len(recs) == 1200
    goes_round(nrec * 8, BLOCK, cap)      # profile_records_preset: by row word
    goes_round(nrec, BLOCK, cap)          # profile_records_finalize: by record
    goes_round(fq.size, RAW_TILE, cap)    # profile_records_kernel: by tile
    P = E.check_twin(fq, k, m, keys, counts)
    with profile_table(form, k, counted) as dc:
        for lo, hi in ((1, E.SAT), (2, 3)):
            PR.both_forms(dc, fq, rs, E.rows_of(P, rs, lo, hi), lo=lo, hi=hi, label=form)


# ---- 8. format ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["wide", "image"])
def test_result_text_in_small_pieces(cap, form):
    k = 21
    dc, keys, counts, _, slots = open_table(form, k)
    with dc:
        if form == "image":                   # (a few hundred records are enough for the text: the threshold keeps the host formatter quick)
            mc = 3
            sel = counts >= U64(mc)
            keys, counts = keys[sel], counts[sel]
        else:
            mc = 1
        goes_round(slots, FMT_TILE, cap)          # fmt_size_kernel over the table's slots ...
        goes_round(keys.size, FMT_TILE, cap)      # ... and over the sorted pairs
        kmers = [s.decode() for s in SO.kmers_of(keys, k)]
        want = dict(zip(kmers, counts.tolist()))
        for fmt in FM.FORMATS:
            nr, nb, pieces = FM.fetch(dc, fmt, mc, cap=4096)
            text = b"".join(pieces)
            assert nr == keys.size and nb == len(text) and len(pieces) > 3
            assert all(FM.ends_at_record_end(fmt, p, i == len(pieces) - 1) for i, p in enumerate(pieces))
            assert sorted(FM.split_records(fmt, text)) == FM.expected_records(fmt, want)
        whole, _ = SO.document("tsv", k, keys, counts)
        nr, nb, pieces = SO.fetch(dc, "tsv", mc, cap=4096)
        assert (nr, nb) == (keys.size, len(whole)) and b"".join(pieces) == whole and len(pieces) > 3


# ---- 9. exports and merges: three logical shards ------------------------------------------------------------------------------------
def shard_reads(k, n_reads=3000):
    if ("shards", k) not in _CACHE:
        bases, _ = O.synth_reads(RS.SEED, 1 << 16, 150, 0, n_reads, with_qual=False)
        m = O.OracleMap()
        m.scan_flat(bases, k, nthreads=NCPU)
        _CACHE[("shards", k)] = (np.asarray(bases), m.as_dict())
    return _CACHE[("shards", k)]


def test_by_owner_export_and_pair_merge(cap):
    import torch
    k, nshards, n_reads = 21, 3, 3000
    bases, want = shard_reads(k)
    per = n_reads // nshards
    goes_round(SLOTS_DEFAULT, BLOCK, cap)         # owner_count_kernel / owner_scatter_kernel: by slot
    exports = []
    for s in range(nshards):
        with native.DeviceCounter(k) as dc:
            dc.push(bases[s * per * 151:(s + 1) * per * 151])
            st = dc.finish()
            assert st["table_slots"] == SLOTS_DEFAULT
            n = st["distinct"]
            dk = torch.empty(n, dtype=torch.int64, device="cuda")
            dn = torch.empty(n, dtype=torch.int64, device="cuda")
            parts = dc.export_by_owner_device(nshards, dk.data_ptr(), dn.data_ptr(), n)
            assert int(parts.sum()) == n
            exports.append((dk, dn, np.concatenate([[0], np.cumsum(parts)]).astype(np.int64)))
    merged = {}
    for p in range(nshards):
        with native.DeviceCounter(k) as dc:
            for dk, dn, offs in exports:
                n = int(offs[p + 1] - offs[p])
                goes_round(n, BLOCK, cap)         # table_merge_pairs_kernel: by pair
                dc.merge_pairs_device(dk.data_ptr() + 8 * int(offs[p]), dn.data_ptr() + 8 * int(offs[p]), n)
            dc.finish()
            d = dc.as_dict()
        assert not (set(d) & set(merged)) and all(native.owner(key, k, nshards) == p for key in list(d)[:200])
        merged.update(d)
    assert merged == want


def test_dense_export_and_merge(cap):
    import torch
    k, nshards, n_reads = 11, 3, 3000
    bases, want = shard_reads(k)
    n = 1 << (2 * k)
    goes_round(SLOTS_DEFAULT, BLOCK, cap)         # table_to_dense_kernel: by slot
    goes_round(n, BLOCK, cap)                     # table_merge_dense_kernel: by entry
    total = torch.zeros(n, dtype=torch.int64, device="cuda")
    per = n_reads // nshards
    for s in range(nshards):
        with native.DeviceCounter(k) as dc:
            dc.push(bases[s * per * 151:(s + 1) * per * 151])
            assert dc.finish()["table_slots"] == SLOTS_DEFAULT
            arr = torch.full((n,), -1, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            dc.export_dense_device(arr.data_ptr(), n)
            d = dc.as_dict()
        host = arr.cpu().numpy()
        nz = np.flatnonzero(host)
        assert len(nz) == len(d) and all(d.get(int(i)) == int(host[i]) for i in nz)
        total += arr
    torch.cuda.synchronize()
    merged = {}
    for o in range(nshards):
        with native.DeviceCounter(k) as dc:
            dc.merge_dense_device(total.data_ptr(), n, o, nshards)
            dc.finish()
            d = dc.as_dict()
        assert all(native.owner(key, k, nshards) == o for key in d) and not (set(d) & set(merged))
        merged.update(d)
    assert merged == want


@pytest.mark.parametrize("npieces,hint", [(1, HINT), (2, 12_000_000)], ids=["whole", "two-pieces"])
def test_region_ordered_export_and_merge(cap, npieces, hint):
    """Three senders; the region-ordered merge shards by hash range, so its owners are a power of two: two of them.  A hint makes
    the tables large enough for shard_reduce_kernel (one lane per region of the window) to go round."""
    import torch
    k, nsend, nown, n_reads = 21, 3, 2, 3000
    bases, want = shard_reads(k)
    per = n_reads // nsend
    exports, nreg = [], None
    for s in range(nsend):
        with native.DeviceCounter(k, capacity_hint=hint) as dc:
            dc.push(bases[s * per * 151:(s + 1) * per * 151])
            st = dc.finish()
            R = st["table_slots"] // 4096
            nreg = R if nreg is None else nreg
            assert R == nreg and R % (nown * npieces) == 0
            goes_round(R, BLOCK, cap)                         # region_window_mask_kernel: by region of the table
            pieces, total = [], 0
            for piece in range(npieces):
                dc.set_region_window(piece, npieces)
                dk = torch.empty(st["distinct"], dtype=torch.int64, device="cuda")
                dn = torch.empty(st["distinct"], dtype=torch.int64, device="cuda")
                rc = torch.empty(R, dtype=torch.int32, device="cuda")
                parts, R2 = dc.export_regions_device(nown, dk.data_ptr(), dn.data_ptr(), st["distinct"], rc.data_ptr(), R)
                rch = rc.cpu().numpy().reshape(nown, npieces, -1)
                assert R2 == R and int(rch.sum()) == int(parts.sum()) == int(rch[:, piece].sum())   # zero outside the piece
                total += int(parts.sum())
                pieces.append((dk, dn, rc, np.concatenate([[0], np.cumsum(parts)]).astype(np.int64)))
            dc.set_region_window(0, 1)
            assert total == st["distinct"]
            exports.append(pieces)
    per_r = nreg // nown
    merged = {}
    for o in range(nown):
        with native.DeviceCounter(k, capacity_hint=hint) as dc:
            dc.set_shard(o, nown)
            for piece in range(npieces):
                dc.set_region_window(piece, npieces)
                dc.merge_regions_device(nreg, [e[piece][0].data_ptr() + 8 * int(e[piece][3][o]) for e in exports],
                                        [e[piece][1].data_ptr() + 8 * int(e[piece][3][o]) for e in exports],
                                        [e[piece][2].data_ptr() + 4 * per_r * o for e in exports])
            dc.set_region_window(0, 1)
            st = dc.finish()
            goes_round(st["table_slots"] // 4096 // npieces, BLOCK, cap)   # shard_reduce_kernel: by region of the shard's window
            d = dc.as_dict()
            assert st["distinct"] == len(d)
        assert not (set(d) & set(merged)) and all(native.owner(key, k, nown) == o for key in list(d)[:300])
        merged.update(d)
    assert merged == want


# ---- 10. natural sizes on the product library ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["fasta", "fastq", "graph_masks", "unitigs"])
def test_product_library_past_2048_tiles(case):
    """No switch: a child process loads libkmerhip.so, whose cap is the constant, and runs one input that crosses 2048 tiles (or
    524 288 items) against the oracle (tests/grid_stride_natural.py)."""
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    env.pop("KMERHIP_GRID_CAP", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "grid_stride_natural.py"), case], capture_output=True, text=True,
                       env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout and "libkmerhip.so" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    print(p.stdout[-500:])
