"""The multi-GPU merge with EMPTY and LOPSIDED ranks, through every route.

Every other multi-rank test of the suite gives each rank an equal share of the reads.  The product does not: `kmerust`
hands 128 MiB text chunks to the ranks in turn, so an input below 128 MiB on `--gpus 8` leaves seven ranks with an empty
table, the last rank of a real run is short, and a rank whose reads `-Q` masks entirely is empty too.  Here some senders
contribute nothing (or a single k-mer) to a receiver that other senders do feed: the case that reaches the merge kernels.

Reference everywhere: the oracle (tests/oracle_lib.py) over the concatenation of what every rank was given, restricted
with O.owners to the keys a rank owns -- never the library's own balanced run.  All comparisons are exact.

  A. logical shards through kh_export_regions_* / kh_merge_regions_* (wide, packed64, heads32), with the pointer of a sender
     that contributes nothing being its own buffer (`own`), ANOTHER sender's live segment (`poison`: valid memory full of
     units that would land in this shard -- the result must not change) or NULL (`null`: include/kmerhip.h, "a sender whose
     region counts are all zero is never dereferenced").  heads32 runs at k = 19: at k = 21 a table of 2^11 regions leaves
     31 hash bits below the region index, more than a head's 28.
  B. kh_group_merge over the route table of test_gpu_exchange.py, two rounds (the second with the loads moved on by one rank).
     `hole` empties rank W // 2 (at W = 2 that is rank 1: the same world as `only-first`, kept for the table's sake).
  C. RCCL: a communicator of one rank is covered by test_gpu_exchange.py; more than one RCCL rank needs more than one GPU.
  D. the image merge's failure code 2 (a region took in >= 2^32 occurrences) widens the shard WITHOUT growing it.
"""
import hashlib
import os

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
SEED = 20260130
NCPU = max(1, min(os.cpu_count() or 1, 16))
STRIDE = 151  # 150 bp + separator


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import krust_amd
    krust_amd.lib()
    return krust_amd


# ---- loads ----------------------------------------------------------------------------------------------------------
_STREAMS, _ORACLES = {}, {}
N_MASKED = 1000  # reads of the `masked-out` rank


def _stream(genome, n):
    if (genome, n) not in _STREAMS:
        _STREAMS[(genome, n)] = O.synth_reads(SEED, genome, 150, 0, n)
    return _STREAMS[(genome, n)]


def _oracle(bases, qual, k, minq):
    """Sorted (keys, counts) of the oracle's map of a flat buffer (kept: the same shares come back in many cases)."""
    if bases.size == 0:
        return np.empty(0, dtype=np.uint64), np.empty(0, dtype=np.uint64)
    h = hashlib.blake2b(bases.tobytes(), digest_size=16)
    if minq is not None:
        h.update(qual.tobytes())
    key = (h.digest(), k, minq)
    if key not in _ORACLES:
        m = O.OracleMap()
        m.scan_flat(bases, k, qual=qual if minq is not None else None, min_quality=minq, nthreads=NCPU)
        _ORACLES[key] = m.arrays()
    return _ORACLES[key]


def loads_of(pattern, W, k, n_reads, genome):
    """-> (per-rank list of (bases, qual), the set of ranks whose TABLE is meant to be empty, the special rank or None).
    All from one synth_reads stream: reads [0, n_reads) go to the ranks that get a share, what the special rank gets
    comes from the reads behind them."""
    bases, qual = _stream(genome, n_reads + N_MASKED)
    none = (bases[:0], qual[:0])
    cut = lambda lo, hi: (bases[lo * STRIDE: hi * STRIDE], qual[lo * STRIDE: hi * STRIDE])
    if pattern == "all-empty":
        return [none] * W, set(range(W)), None
    if pattern in ("only-first", "only-last"):
        full = 0 if pattern == "only-first" else W - 1
        return [cut(0, n_reads) if r == full else none for r in range(W)], set(range(W)) - {full}, None
    special = W // 2
    takers = [r for r in range(W) if r != special]
    per = n_reads // len(takers)
    out = [None] * W
    for i, r in enumerate(takers):
        out[r] = cut(i * per, n_reads if i == len(takers) - 1 else (i + 1) * per)
    if pattern == "hole":
        out[special] = none
        return out, {special}, special
    if pattern == "one-read":
        out[special] = cut(n_reads, n_reads + 1)
        return out, set(), special
    if pattern == "one-kmer":  # one record of exactly k bases
        o = n_reads * STRIDE
        out[special] = (np.concatenate([bases[o: o + k], bases[o + 150: o + 151]]), np.concatenate([qual[o: o + k], qual[o + 150: o + 151]]))
        assert out[special][0].size == k + 1
        return out, set(), special
    if pattern == "masked-out":  # non-empty input, every quality below min_quality
        b, q = cut(n_reads, n_reads + N_MASKED)
        q = q.copy()
        q[b != 10] = ord("!")
        out[special] = (b, q)
        return out, {special}, special
    raise AssertionError(pattern)


def oracle_of_loads(loads, k, minq):
    return _oracle(np.concatenate([b for b, _ in loads]), np.concatenate([q for _, q in loads]), k, minq)


def _hist(cnts):
    return dict(zip(*[a.tolist() for a in np.unique(np.asarray(cnts, dtype=np.uint64), return_counts=True)]))


# ---- A. logical shards through the public merge calls ---------------------------------------------------------------
FMT_NAMES = ["wide", "packed64", "heads32"]
UNIT = {0: 8, 1: 8, 2: 4}
_SENDERS = {}  # the last case's exports (its three pointer variants follow one another)


def _export(dc, fmt, nshards, st, R, torch):
    n = max(st["distinct"], 1)
    dk = torch.zeros(2 * n if fmt == 2 else n, dtype=torch.int64, device="cuda")
    dcnt = torch.zeros(n, dtype=torch.int64, device="cuda")
    rc = torch.zeros(R, dtype=torch.int32, device="cuda")
    if fmt == 1:
        res = dc.export_regions_packed_device(nshards, dk.data_ptr(), n, rc.data_ptr(), R)
    elif fmt == 2:
        res = dc.export_regions_heads_device(nshards, dk.data_ptr(), 4 * n, rc.data_ptr(), R)
    else:
        res = dc.export_regions_device(nshards, dk.data_ptr(), dcnt.data_ptr(), n, rc.data_ptr(), R)
    assert res is not None, "this k / table size must be representable in the format: the case list holds no other"
    parts, R2 = res
    assert R2 == R and int(rc.sum().item()) == int(parts.sum())
    return dk, dcnt, rc, parts


def senders_of(K, fmt, pattern, nshards, k, minq, n_reads=40_000, genome=1 << 17):
    import torch
    key = (fmt, pattern, nshards, k, minq)
    if key in _SENDERS:
        return _SENDERS[key]
    _SENDERS.clear()
    loads, empty, special = loads_of(pattern, nshards, k, n_reads, genome)
    senders, nreg = [None] * nshards, None
    for s, (b, q) in enumerate(loads):
        if b.size == 0:
            continue
        with K.DeviceCounter(k, min_quality=minq, capacity_hint=3_000_000) as dc:  # same hint -> same table size
            dc.push(b, q)
            st = dc.finish()
            assert (st["distinct"] == 0) == (s in empty), (s, st["distinct"])
            R = st["table_slots"] // 4096
            nreg = R if nreg is None else nreg
            assert R == nreg, "a sender's table_regions differs from the others'"
            dk, dcnt, rc, parts = _export(dc, fmt, nshards, st, R, torch)
            senders[s] = dict(keys=dk, cnts=dcnt, rc=rc, parts=parts, offs=np.concatenate([[0], np.cumsum(parts)]).astype(np.int64))
    assert nreg is not None
    for s in range(nshards):  # a rank that was given nothing: zero region counts and a 1-element key buffer, made by hand
        if senders[s] is None:
            senders[s] = dict(keys=torch.zeros(1, dtype=torch.int64, device="cuda"), cnts=torch.zeros(1, dtype=torch.int64, device="cuda"),
                              rc=torch.zeros(nreg, dtype=torch.int32, device="cuda"), parts=np.zeros(nshards, dtype=np.uint64),
                              offs=np.zeros(nshards + 1, dtype=np.int64))
    torch.cuda.synchronize()
    fk, fc = oracle_of_loads(loads, k, minq)
    _SENDERS[key] = (senders, nreg, empty, special, fk, fc, O.owners(K, fk, k, nshards))
    return _SENDERS[key]


def pointers_for(senders, o, fmt, variant, per_r):
    """Key / count / region-count pointers of every sender for receiver o; a sender without units for o by `variant`."""
    unit = UNIT[fmt]
    live = [s for s, e in enumerate(senders) if int(e["parts"][o]) > 0]
    kp, cp, rp = [], [], []
    for e in senders:
        src = e
        if int(e["parts"][o]) == 0:
            assert int(e["rc"][per_r * o: per_r * (o + 1)].sum().item()) == 0
            if variant == "null":
                kp.append(0)
                cp.append(0)
                rp.append(e["rc"].data_ptr() + 4 * per_r * o)
                continue
            if variant == "poison" and live:
                src = senders[live[0]]
        kp.append(src["keys"].data_ptr() + unit * int(src["offs"][o]))
        cp.append(src["cnts"].data_ptr() + 8 * int(src["offs"][o]))
        rp.append(e["rc"].data_ptr() + 4 * per_r * o)
    return kp, cp, rp


def merge_call(dc, fmt, nreg, kp, cp, rp):
    if fmt == 1:
        dc.merge_regions_packed_device(nreg, kp, rp)
    elif fmt == 2:
        dc.merge_regions_heads_device(nreg, kp, rp)
    else:
        dc.merge_regions_device(nreg, kp, cp, rp)


def check_lopsided(senders, nshards, pattern, empty, special):
    """The case is what its name says, per receiver."""
    for o in range(nshards):
        got = [int(e["parts"][o]) for e in senders]
        assert all(got[s] == 0 for s in empty), (o, got)
        assert any(g > 0 for s, g in enumerate(got) if s not in empty), (o, got)
    if pattern == "one-kmer":
        assert sorted(int(x) for x in senders[special]["parts"]) == [0] * (nshards - 1) + [1]


def check_shard(K, dc, o, fk, fc, owners, label):
    sel = owners == o
    st = dc.finish()
    keys, cnts = dc.result()
    assert np.array_equal(keys, fk[sel]) and np.array_equal(cnts, fc[sel]), f"shard {o} differs from the oracle ({label})"
    assert st["distinct"] == int(sel.sum()) and st["kmers"] == int(fc[sel].sum()), (label, o, st)
    foreign = fk[~sel][:2000]
    assert not dc.lookup(foreign).any(), f"shard {o} answers for keys it does not own ({label})"
    assert np.array_equal(dc.lookup(keys[:1000]), cnts[:1000])
    assert dict(dc.histogram()) == _hist(fc[sel]), (label, o)
    return st


A_CASES = [(fmt, 19 if fmt == 2 else 21, None, n, p) for fmt in (0, 1, 2) for n in (2, 4, 8) for p in ("only-first", "only-last", "hole", "one-kmer")]
A_CASES += [(0, 31, 20, 4, "masked-out")]
A_CASES += [(fmt, 9, None, 8, p) for fmt in (0, 1, 2) for p in ("only-last", "one-kmer")]  # the short-key geometry


@pytest.mark.parametrize("variant", ["own", "poison", "null"])
@pytest.mark.parametrize("fmt,k,minq,nshards,pattern", A_CASES,
                         ids=[f"{FMT_NAMES[f]}-k{k}{'q20' if q else ''}-w{n}-{p}" for f, k, q, n, p in A_CASES])
def test_logical_shards_with_empty_senders(K, fmt, k, minq, nshards, pattern, variant):
    senders, nreg, empty, special, fk, fc, owners = senders_of(K, fmt, pattern, nshards, k, minq)
    check_lopsided(senders, nshards, pattern, empty, special)
    per_r = nreg // nshards
    total = 0
    for o in range(nshards):
        kp, cp, rp = pointers_for(senders, o, fmt, variant, per_r)
        if variant == "null":
            assert all((p == 0) == (int(e["parts"][o]) == 0) for p, e in zip(kp, senders))
        with K.DeviceCounter(k, capacity_hint=3_000_000) as dc:
            dc.set_shard(o, nshards)
            merge_call(dc, fmt, nreg, kp, cp, rp)
            st = check_shard(K, dc, o, fk, fc, owners, f"{variant}")
            total += st["kmers"]
    assert total == int(fc.sum())


@pytest.mark.parametrize("variant", ["own", "null"])
@pytest.mark.parametrize("fmt,k", [(1, 21), (2, 19)], ids=["packed64-k21", "heads32-k19"])
def test_windowed_merge_where_a_sender_has_one_unit_in_one_piece(K, fmt, k, variant):
    """kh_set_region_window, 4 pieces, 2 shards: rank 0 holds all the reads, rank 1 one k-mer -- for the receiver that owns
    it three of the four pieces are empty from rank 1, for the other receiver all four."""
    import torch
    nshards, npieces = 2, 4
    loads, _, special = loads_of("one-kmer", nshards, k, 40_000, 1 << 17)
    fk, fc = oracle_of_loads(loads, k, None)
    owners = O.owners(K, fk, k, nshards)
    exports, nreg = [], None
    for b, q in loads:
        with K.DeviceCounter(k, capacity_hint=3_000_000) as dc:
            dc.push(b)
            st = dc.finish()
            R = st["table_slots"] // 4096
            nreg = R if nreg is None else nreg
            assert R == nreg
            pieces = []
            for piece in range(npieces):
                dc.set_region_window(piece, npieces)
                dk, dcnt, rc, parts = _export(dc, fmt, nshards, st, R, torch)
                pieces.append(dict(keys=dk, cnts=dcnt, rc=rc, parts=parts, offs=np.concatenate([[0], np.cumsum(parts)]).astype(np.int64)))
            dc.set_region_window(0, 1)
            exports.append(pieces)
    torch.cuda.synchronize()
    lone = sorted(int(exports[special][p]["parts"][o]) for p in range(npieces) for o in range(nshards))
    assert lone == [0] * (npieces * nshards - 1) + [1], lone
    per_r = nreg // nshards
    for o in range(nshards):
        with K.DeviceCounter(k, capacity_hint=3_000_000) as dc:
            dc.set_shard(o, nshards)
            for piece in range(npieces):
                dc.set_region_window(piece, npieces)
                kp, cp, rp = pointers_for([e[piece] for e in exports], o, fmt, variant, per_r)
                assert int(exports[0][piece]["parts"][o]) > 0
                merge_call(dc, fmt, nreg, kp, cp, rp)
            dc.set_region_window(0, 1)
            check_shard(K, dc, o, fk, fc, owners, f"windowed {variant}")


# ---- B. through kh_group_merge ------------------------------------------------------------------------------------
# (world, k, min_quality, KMERHIP_MERGE_PIECES, insert path): the route table of test_group_of_ranks_sharing_the_device
ROUTES = [(2, 19, None, "1", "partition"), (2, 19, None, None, "partition"), (4, 21, None, "1", None), (4, 21, None, "4", None),
          (8, 21, None, None, None), (2, 31, None, None, None), (3, 21, None, None, None), (3, 13, None, None, None), (2, 9, None, None, None)]
PATTERNS = ["only-first", "only-last", "hole", "one-read", "one-kmer", "all-empty"]
B_CASES = [(r, p, {}) for r in ROUTES for p in PATTERNS]
B_CASES += [((2, 31, 20, None, None), "masked-out", {})]
B_CASES += [((4, 21, None, "4", None), "only-first", {"KMERHIP_SELF_SEND": "1"}), ((4, 21, None, "1", None), "only-first", {"KMERHIP_NARROW": "0"})]
FAMILIES = ("regions-heads", "regions-packed", "regions", "pairs")
_FAMILIES_SEEN = set()  # route families a LOPSIDED case (one with a non-empty rank) went through


def _family(path):
    return path.split("-x")[0]


def group_case(K, monkeypatch, route, pattern, env, n_reads=120_000):
    world, k, minq, pieces, path = route
    if pieces is None:
        monkeypatch.delenv("KMERHIP_MERGE_PIECES", raising=False)
    else:
        monkeypatch.setenv("KMERHIP_MERGE_PIECES", pieces)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    loads, empty, special = loads_of(pattern, world, k, n_reads, 1 << 20)
    fk, fc = oracle_of_loads(loads, k, minq)
    owners = O.owners(K, fk, k, world)
    own_distinct = [_oracle(b, q, k, minq)[0].size for b, q in loads]
    assert all(own_distinct[r] == 0 for r in empty) and (pattern == "all-empty" or any(own_distinct))
    if pattern == "one-kmer":
        assert own_distinct[special] == 1
    with K.DeviceGroup(k, [0] * world, min_quality=minq, capacity_hint=3_000_000, path=path) as g:
        assert len(g) == world
        for rnd in range(2):  # the second round: the same group, reset, the loads moved on by one rank
            given = [loads[(r - rnd) % world] for r in range(world)]
            expect_local = [own_distinct[(r - rnd) % world] for r in range(world)]
            for dc, (b, q) in zip(g.counters, given):
                if rnd:
                    dc.reset()
                if b.size:  # (a rank that was given nothing never pushes, as in the product)
                    dc.push(b, q if minq is not None else None)
            infos = g.merge()
            paths = {i["path"] for i in infos}
            print(f"route {route} pattern {pattern} {env} round {rnd}: path {sorted(paths)}")
            assert len(paths) == 1, infos
            got = 0
            for r, (dc, info) in enumerate(zip(g.counters, infos)):
                sel = owners == r
                assert info["conserved"] == 1 and info["nranks"] == world, info
                assert info["local_distinct"] == expect_local[r], (r, info, expect_local)
                keys, cnts = dc.result()
                assert np.array_equal(keys, fk[sel]) and np.array_equal(cnts, fc[sel]), f"round {rnd}: shard {r} differs from the oracle"
                assert info["owned_distinct"] == int(sel.sum())
                assert np.array_equal(dc.lookup(keys[:1000]), cnts[:1000])
                assert not dc.lookup(fk[~sel][:2000]).any()
                got += int(cnts.sum())
            assert got == int(fc.sum())
            if pattern != "all-empty":
                _FAMILIES_SEEN.add(_family(paths.pop()))


@pytest.mark.parametrize("route,pattern,env", B_CASES,
                         ids=[f"w{r[0]}-k{r[1]}{'q20' if r[2] else ''}-p{r[3] or 'dflt'}-{p}" + "".join(f"-{n[8:].lower()}{v}" for n, v in e.items())
                              for r, p, e in B_CASES])
def test_group_merge_with_empty_and_lopsided_ranks(K, monkeypatch, route, pattern, env):
    group_case(K, monkeypatch, route, pattern, env)


def test_every_route_family_was_taken_by_a_lopsided_world(K, monkeypatch):
    """Over the cases above each of regions-heads*, regions-packed*, regions and pairs must have carried a lopsided world.
    (Run on its own, this test walks the route table itself with `only-first`.)"""
    if not set(FAMILIES) <= _FAMILIES_SEEN:
        for route in ROUTES:
            group_case(K, monkeypatch, route, "only-first", {}, n_reads=30_000)
    assert set(FAMILIES) <= _FAMILIES_SEEN, sorted(_FAMILIES_SEEN)


# ---- D. code 2 does not grow the table --------------------------------------------------------------------------------
def test_a_count_beyond_32_bits_in_the_image_merge_widens_without_growing(K):
    """The scenario of test_shard_image_counts_beyond_32_bits_fall_back (test_gpu_parity.py) twice into fresh receivers with the
    same hint: one rank's packed export merged as three senders, the homopolymer pushed 8 times (3 x count > 2^32: code 2, the
    shard is widened and the region re-inserted) and 4 times (3 x count < 2^32: the shard stays the 8-byte image).  Same keys,
    same number of incoming units, so the same sizing inputs: the table must have the same size in both."""
    import torch
    k, n_a = 21, 1_600_000
    poly = np.full((n_a, STRIDE), ord("A"), dtype=np.uint8)
    poly[:, 150] = 10
    other, _ = O.synth_reads(SEED, 1 << 18, 150, 0, 50_000, with_qual=False)
    base = dict(zip(*[a.tolist() for a in _oracle(other, None, k, None)]))
    ta = torch.from_numpy(poly.reshape(-1)).cuda()
    to = torch.from_numpy(other.copy()).cuda()
    torch.cuda.synchronize()
    stats = {}
    for pushes in (8, 4):
        with K.DeviceCounter(k, capacity_hint=6_000_000, path="partition") as dc:
            dc.push_device(to.data_ptr(), None, to.numel())
            for _ in range(pushes):
                dc.push_device(ta.data_ptr(), None, ta.numel())
            st = dc.finish()
            R = st["table_slots"] // 4096
            dk = torch.empty(st["distinct"], dtype=torch.int64, device="cuda")
            rc = torch.empty(R, dtype=torch.int32, device="cuda")
            parts, R2 = dc.export_regions_packed_device(1, dk.data_ptr(), st["distinct"], rc.data_ptr(), R)
            assert R2 == R and int(parts.sum()) == st["distinct"]
        one = dict(base)
        one[0] = one.get(0, 0) + pushes * n_a * 130
        if pushes == 8:
            assert 3 * one[0] > 1 << 32 > one[0]
        else:
            assert 3 * one[0] < 1 << 32
        with K.DeviceCounter(k, capacity_hint=6_000_000) as dc:
            dc.set_shard(0, 1)
            dc.merge_regions_packed_device(R, [dk.data_ptr()] * 3, [rc.data_ptr()] * 3)
            st = dc.finish()
            assert st["distinct"] == len(one) and st["kmers"] == 3 * sum(one.values())
            assert dc.as_dict() == {key: 3 * c for key, c in one.items()}
            assert int(dc.lookup(np.array([0], dtype=np.uint64))[0]) == 3 * one[0]
        stats[pushes] = (st, int(parts.sum()), R)
    (st8, units8, R8), (st4, units4, R4) = stats[8], stats[4]
    print(f"table_slots: {st8['table_slots']} (code 2) / {st4['table_slots']} (no code 2); grows {st8['grows']} / {st4['grows']}; "
          f"slot_bytes {st8['slot_bytes']} / {st4['slot_bytes']}")
    assert units8 == units4 and R8 == R4  # the same sizing inputs
    # the image applies where the 32 bits behind the shard table's level-1 digit hold all of the hash below it (merge.hip)
    regions = st4["table_slots"] // 4096
    assert regions >= R4 and 2 * k - min(10, regions.bit_length() - 1) <= 32, regions
    assert st4["slot_bytes"] == 8
    assert st8["slot_bytes"] == 16
    assert st8["table_slots"] == st4["table_slots"], "a count that left 32 bits doubled a table that was not full"
    assert st8["grows"] == st4["grows"]
