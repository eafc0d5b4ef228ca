"""kh_unitigs_* -- the unitigs of a count table -- against a reference in Python strings.

Expected values never come from the library.  The node set S is O.OracleMap's counts of the same flat buffer that was pushed (or
the chosen pairs that were merged), thresholded, as a dict from canonical strings to counts.  Successors, degrees and the four
link conditions of include/kmerhip.h are string arithmetic with that dict; chains are walked one node at a time, and the reading
and order rules are applied.  Rows and bases are compared byte for byte."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_graph as G
import test_gpu_join as T
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
ALL = (1 << 64) - 1
COMP = bytes.maketrans(b"ACGT", b"TGCA")
LETTERS = (b"A", b"C", b"G", b"T")


# ---- the reference: strings and a dict -----------------------------------------------------------------------------------------
def rc(s):
    return s[::-1].translate(COMP)


def canon(s):
    r = rc(s)
    return s if s <= r else r


def unpack(keys, k):
    """Packed keys -> k-letter byte strings (first base most significant)."""
    keys = np.asarray(keys, dtype=U64)
    codes = np.empty((keys.size, k), dtype=np.uint8)
    for i in range(k):
        codes[:, i] = ((keys >> U64(2 * (k - 1 - i))) & U64(3)).astype(np.uint8)
    text = np.frombuffer(b"ACGT", dtype=np.uint8)[codes]
    return [text[i].tobytes() for i in range(keys.size)]


def node_dict(keys, counts, k, mc):
    sk, sc = G.node_set(np.asarray(keys, dtype=U64), np.asarray(counts, dtype=U64), mc)
    return dict(zip(unpack(sk, k), (int(c) for c in sc)))


class Ref:
    """The unitigs of the node set S (canonical string -> count): rows as a (n, 4) uint64 array, bases as bytes, and what the
    walk met on its way (`seen`)."""

    def __init__(self, S, k):
        self.S, self.k = S, k
        self.seen = {"palindrome": 0, "loop": 0, "hairpin": 0, "minus_first": 0, "circular": 0}
        self.unitigs = []   # (first node's string, sequence, L, count sum, circular)
        self._walk()
        self.unitigs.sort(key=lambda u: u[0])
        rows = np.zeros((len(self.unitigs), 4), dtype=U64)
        start = 0
        for i, (_, seq, L, cs, circ) in enumerate(self.unitigs):
            assert len(seq) == L + k - 1
            for j, v in enumerate((start, L, cs % (1 << 64), 1 if circ else 0)):
                rows[i, j] = U64(v)
            start += len(seq)
        self.rows = rows
        self.bases = b"".join(u[1] for u in self.unitigs)

    @staticmethod
    def spell(u):
        return u[0] if u[1] == 0 else rc(u[0])

    def succ(self, u):
        w = self.spell(u)
        out = []
        for c in LETTERS:
            t = w[1:] + c
            y = canon(t)
            if y in self.S:
                out.append((y, 0 if t == y else 1))
        return out

    def link(self, u):
        """The compactable link out of u, or None."""
        su = self.succ(u)
        if len(su) != 1:
            return None
        v = su[0]
        back = len(self.succ((v[0], v[1] ^ 1))) == 1
        if v[0] == u[0]:
            self.seen["loop" if v[1] == u[1] else "hairpin"] += 1
            return None
        if rc(u[0]) == u[0] or rc(v[0]) == v[0]:
            if back:
                self.seen["palindrome"] += 1   # a link in every other respect
            return None
        return v if back else None

    def _chain_from(self, u):
        """u and what follows it along compactable links; closed = the walk came back to u."""
        chain = [u]
        while True:
            v = self.link(chain[-1])
            if v is None:
                return chain, False
            if v == u:
                return chain, True
            chain.append(v)

    def _walk(self):
        done = set()
        for x in sorted(self.S):
            if x in done:
                continue
            fwd, closed = self._chain_from((x, 0))
            if closed:
                m = min(n for n, _ in fwd)
                if (m, 0) not in fwd:                                   # the mirrored cycle holds (m, +)
                    fwd = [(n, s ^ 1) for n, s in reversed(fwd)]
                i = fwd.index((m, 0))
                chain = fwd[i:] + fwd[:i]
                self.seen["circular"] += 1
            else:
                bwd, closed2 = self._chain_from((x, 1))
                assert not closed2
                chain = [(n, s ^ 1) for n, s in reversed(bwd[1:])] + fwd
                if len(chain) > 1 and chain[-1][0] < chain[0][0]:
                    chain = [(n, s ^ 1) for n, s in reversed(chain)]
                assert len(chain) == 1 or chain[0][0] != chain[-1][0]
                if len(chain) == 1:
                    chain = [(x, 0)]
            nodes = [n for n, _ in chain]
            assert len(set(nodes)) == len(nodes) and not (set(nodes) & done)    # a chain never meets its own mirror image
            done.update(nodes)
            if chain[0][1] == 1:
                self.seen["minus_first"] += 1
            seq = self.spell(chain[0]) + b"".join(self.spell(u)[-1:] for u in chain[1:])
            self.unitigs.append((chain[0][0], seq, len(chain), sum(self.S[n] for n in nodes), closed))
        assert len(done) == len(self.S)


_REFS = {}


def ref_of(tag, keys, counts, k, mc):
    """The reference of (input, k, threshold), computed once."""
    key = (tag, k, max(mc, 1))
    if key not in _REFS:
        _REFS[key] = Ref(node_dict(keys, counts, k, mc), k)
    return _REFS[key]


# ---- what every table is held to ---------------------------------------------------------------------------------------------------
def kmers_of(rows, bases, k):
    """The canonical packed k-mers of all unitigs (numpy), window by window."""
    if bases.size == 0:
        return np.empty(0, dtype=U64)
    codes = ((bases >> 1) ^ (bases >> 2)) & 3
    nwin = bases.size - k + 1
    acc = np.zeros(nwin, dtype=U64)
    for i in range(k):
        acc = (acc << U64(2)) | codes[i:i + nwin].astype(U64)
    inside = np.ones(bases.size, dtype=bool)
    ends = (rows[:, native.UNI_START] + rows[:, native.UNI_KMERS] + U64(k - 1)).astype(np.int64)
    for d in range(1, k):                        # the last k - 1 bases of a unitig start no k-mer
        inside[ends - d] = False
    x = acc[inside[:nwin]]
    return np.minimum(x, G.np_revcomp(x, k))


def check_unitigs(dc, tag, keys, counts, k, mc, ref=None):
    ref = ref or ref_of(tag, keys, counts, k, mc)
    rows, bases = dc.unitigs(mc)
    assert rows.dtype == U64 and rows.shape == ref.rows.shape and bases.dtype == np.uint8
    assert np.array_equal(rows, ref.rows), (k, mc, np.argwhere(rows != ref.rows)[:4])
    assert bases.tobytes() == ref.bases, (k, mc)
    # invariants that need no reference
    sk, sc = G.node_set(np.asarray(keys, dtype=U64), np.asarray(counts, dtype=U64), mc)
    words = dc.graph_stats(mc)
    assert int(np.sum(rows[:, native.UNI_KMERS], dtype=U64)) == int(words[native.GRAPH_NODES]) == sk.size
    assert int(np.sum(rows[:, native.UNI_COUNT_SUM], dtype=U64)) == int(words[native.GRAPH_KMERS]) == int(np.sum(sc, dtype=U64))
    lens = rows[:, native.UNI_KMERS] + U64(k - 1)
    assert np.array_equal(rows[:, native.UNI_START], np.cumsum(lens, dtype=U64) - lens) and int(np.sum(lens, dtype=U64)) == bases.size
    assert np.array_equal(np.sort(kmers_of(rows, bases, k)), sk)          # exactly S, each once
    assert np.isin(bases, np.frombuffer(b"ACGT", dtype=np.uint8)).all()
    for r in rows[rows[:, native.UNI_FLAGS] == 1]:                        # a circular one starts at its smallest key, as +
        b = bases[int(r[0]):int(r[0]) + int(r[1]) + k - 1]
        one = np.array([[0, r[1], 0, 1]], dtype=U64)
        ks = kmers_of(one, b, k)
        first = b[:k].tobytes()
        assert canon(first) == first and int(ks.min()) == int(ks[0])
    return rows, bases, ref


def flat_of(records):
    return np.frombuffer(b"N" + b"N".join(records) + b"N", dtype=np.uint8)


def oracle_pairs(flat, k):
    m = O.OracleMap()
    m.process(flat, k)
    keys, counts = m.arrays()
    return np.asarray(keys, dtype=U64).copy(), np.asarray(counts, dtype=U64).copy()


# ---- small k, dense ---------------------------------------------------------------------------------------------------------------------
CHOSEN = {2: (b"CC", b"CA", b"AT"), 4: (b"GTGA", b"CACG", b"ACGT")}   # a chain that runs into a palindrome with no other neighbour


def pack_str(t):
    return sum(b"ACGT".index(ch) << (2 * (len(t) - 1 - i)) for i, ch in enumerate(t))


def small_case(k, density):
    """(keys, counts): a random subset of the canonical key space at that density, or the chosen keys."""
    if density == "chosen":
        assert all(canon(t) == t for t in CHOSEN[k])
        return np.array(sorted(pack_str(t) for t in CHOSEN[k]), dtype=U64), np.array([1, 2, 3], dtype=U64)
    rng = np.random.default_rng(1000 * k + int(density * 10))
    every = G.canonical_keys(k)
    if density == 1.0:
        keys = every
    else:
        keys = np.sort(rng.choice(every, size=max(int(round(every.size * density)), 1), replace=False)).astype(U64)
    counts = rng.integers(1, 4, size=keys.size).astype(U64)
    return keys, counts


SMALL = [(k, d) for k in (1, 2, 3, 4, 5) for d in (0.1, 0.5, 1.0)] + [(2, "chosen"), (4, "chosen")]


def test_small_inputs_hold_palindromes_loops_and_hairpins():
    """Precondition, from the reference alone: the small-k inputs meet a palindrome inside what would otherwise be a chain (k = 2
    and k = 4), a homopolymer loop and a hairpin, so those rules are exercised."""
    seen = {}
    for k, d in SMALL:
        for mc in (1, 2):
            keys, counts = small_case(k, d)
            r = ref_of(("small", d), keys, counts, k, mc)
            for name, v in r.seen.items():
                seen[(k, name)] = seen.get((k, name), 0) + v
    assert seen[(2, "palindrome")] > 0 and seen[(4, "palindrome")] > 0, seen
    assert sum(seen[(k, "loop")] for k in (1, 2, 3, 4, 5)) > 0 and sum(seen[(k, "hairpin")] for k in (1, 2, 3, 4, 5)) > 0, seen


@pytest.mark.parametrize("k,density", SMALL, ids=[f"k{k}-d{d}" for k, d in SMALL])
def test_small_k_dense(k, density):
    keys, counts = small_case(k, density)
    with native.DeviceCounter(k) as dc:
        dc.merge_pairs(keys, counts)
        for mc in (1, 2):
            check_unitigs(dc, ("small", density), keys, counts, k, mc)


# ---- chain lengths across tile and round edges -----------------------------------------------------------------------------------------
CHAIN_L = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 20000]
_CHAINS = {}


def chain_input(k):
    if k not in _CHAINS:
        rng = np.random.default_rng(40 + k)
        recs = []
        for i, L in enumerate(CHAIN_L):
            s = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L + k - 1)].tobytes()
            recs.append(rc(s) if i % 2 else s)          # half of them as their reverse complement
        flat = flat_of(recs)
        _CHAINS[k] = (flat,) + oracle_pairs(flat, k)
    return _CHAINS[k]


@pytest.mark.parametrize("k", [21, 31, 32])
def test_chain_lengths(k):
    flat, keys, counts = chain_input(k)
    ref = ref_of("chains", keys, counts, k, 1)
    assert sorted(int(v) for v in ref.rows[:, native.UNI_KMERS]) == sorted(CHAIN_L)   # the records are disjoint chains
    assert ref.seen["minus_first"] > 0                                                # first nodes in - orientation occur
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        check_unitigs(dc, "chains", keys, counts, k, 1)


# ---- cycles ----------------------------------------------------------------------------------------------------------------------------------
PERIODS = [3, 64, 65, 1000, 5000]
_CYCLES = {}


def cycle_input(k):
    if k not in _CYCLES:
        rng = np.random.default_rng(70 + k)
        recs = []
        for i, p in enumerate(PERIODS):
            unit = b"ACG" if p == 3 else np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=p)].tobytes()
            circ = (unit * (k // p + 2))[:p + k - 1]      # the circular sequence: one period plus its own first k - 1 letters
            recs.append(rc(circ) if i % 2 else circ)
            recs.append(np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=k + 100 * (i + 1))].tobytes())   # an ordinary chain
        flat = flat_of(recs)
        _CYCLES[k] = (flat,) + oracle_pairs(flat, k)
    return _CYCLES[k]


@pytest.mark.parametrize("k", [21, 31])
def test_cycles(k):
    flat, keys, counts = cycle_input(k)
    ref = ref_of("cycles", keys, counts, k, 1)
    assert ref.seen["circular"] >= len(PERIODS) and int(np.sum(ref.rows[:, native.UNI_FLAGS])) >= len(PERIODS)
    assert set(PERIODS) <= set(int(r[1]) for r in ref.rows if r[3])
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        rows, bases, _ = check_unitigs(dc, "cycles", keys, counts, k, 1)   # (it asserts where every circular unitig starts)
        assert int(np.sum(rows[:, native.UNI_FLAGS])) >= len(PERIODS)


# ---- branching, realistic ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_branching_reads_and_stars(k):
    flat, keys, counts = G.main_input(k)
    with native.DeviceCounter(k, capacity_hint=3_000_000) as dc:
        dc.push(flat)
        for mc in (0, 1, 2, 3, ALL):
            rows, _, ref = check_unitigs(dc, "main", keys, counts, k, mc)
            if mc == 1:
                assert rows.shape[0] > 256 and int(rows[:, native.UNI_KMERS].max()) > 30    # branches and chains
            if mc == ALL:
                assert rows.shape[0] == 0


# ---- table forms and geometries: identical bytes ----------------------------------------------------------------------------------------
FORMS = ["wide", "image", "regions3072", "grown", "narrow0", "hint1", "pow2"]


@pytest.mark.parametrize("form", FORMS)
def test_table_forms(form, monkeypatch):
    k = 21
    flat, keys, counts = G.main_input(k)
    if form in ("wide", "image", "regions3072", "grown"):
        dc = T.table(form, k, flat, monkeypatch)
    else:
        if form == "narrow0":
            monkeypatch.setenv("KMERHIP_NARROW", "0")
        if form == "pow2":
            monkeypatch.setenv("KMERHIP_POW2_TABLE", "1")
        dc = native.DeviceCounter(k, capacity_hint=1 if form == "hint1" else 3_000_000, path="partition" if form == "narrow0" else None)
        dc.push(flat)
        st = dc.finish()
        if form == "narrow0":
            assert st["slot_bytes"] == 16 and st["part_batches"] >= 1
        if form == "hint1":
            assert st["grows"] >= 1
        if form == "pow2":
            assert st["table_slots"] & (st["table_slots"] - 1) == 0
    with dc:
        before = T.stats_of(dc)
        for mc in (1, 2):
            check_unitigs(dc, "main", keys, counts, k, mc)
        assert T.stats_of(dc) == before


# ---- the contract ------------------------------------------------------------------------------------------------------------------------------
def test_read_only_pending_pushes_and_interleaved_readers(monkeypatch):
    k = 21
    flat, keys, counts = G.main_input(k)
    ref = ref_of("main", keys, counts, k, 1)
    with T.table("image", k, flat, monkeypatch) as dc:
        before = T.stats_of(dc)
        s0 = dc.result_sorted(1)
        nu, nb = dc.unitigs_begin(1)
        assert (nu, nb) == (ref.rows.shape[0], len(ref.bases))
        # readers between begin and copy
        n = C.c_uint64(0)
        assert native.lib().kh_result_size(dc._h, 1, C.byref(n)) == native.KH_OK and n.value == keys.size
        assert np.array_equal(dc.lookup(keys[:100]), counts[:100])
        dc.histogram()
        assert np.array_equal(dc.graph_stats(1), G.main_words(k, 1))
        assert np.array_equal(dc.graph_masks(keys[:100], 1), G.np_masks(keys[:100], keys, k))
        dc.profile(np.frombuffer(b"ACGT" * 20, dtype=np.uint8))
        rows, bases = dc.unitigs_copy(nu, nb)
        assert np.array_equal(rows, ref.rows) and bases.tobytes() == ref.bases
        # begin twice is allowed, and a second copy gives the same
        assert dc.unitigs_begin(2) == (ref_of("main", keys, counts, k, 2).rows.shape[0], len(ref_of("main", keys, counts, k, 2).bases))
        assert dc.unitigs_begin(1) == (nu, nb)
        rows2, bases2 = dc.unitigs_copy(nu, nb)
        assert np.array_equal(rows2, rows) and np.array_equal(bases2, bases)
        dc.unitigs_end()
        dc.unitigs_end()   # end without begin is allowed
        s1 = dc.result_sorted(1)
        assert T.stats_of(dc) == before and np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
    with native.DeviceCounter(k, capacity_hint=3_000_000) as dc:   # a pending push is counted first
        dc.push(flat)
        assert dc.unitigs_begin(1) == (ref.rows.shape[0], len(ref.bases))
        dc.unitigs_end()


def test_caps_between_canaries():
    k = 21
    flat, keys, counts = chain_input(k)
    ref = ref_of("chains", keys, counts, k, 1)
    L = native.lib()
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        nu, nb = dc.unitigs_begin(1)
        assert nu == ref.rows.shape[0] and nb == len(ref.bases) and nu > 2
        for rcap, bcap in [(0, nb), (1, nb), (nu - 1, nb), (nu, 0), (nu, 1), (nu, nb - 1), (0, 0), (nu, nb)]:
            rows = np.full(4 * nu + 8, 0xABABABABABABABAB, dtype=U64)
            bases = np.full(nb + 64, 0xAB, dtype=np.uint8)
            rc_ = L.kh_unitigs_copy(dc._h, rows[4:].ctypes.data, rcap, bases[32:].ctypes.data, bcap)
            if rcap < nu or bcap < nb:
                assert rc_ == native.KH_ERR_RANGE, (rcap, bcap)
                assert (rows == U64(0xABABABABABABABAB)).all() and (bases == 0xAB).all()      # NOTHING is written
            else:
                assert rc_ == native.KH_OK
                assert np.array_equal(rows[4:4 + 4 * nu].reshape(nu, 4), ref.rows) and bases[32:32 + nb].tobytes() == ref.bases
                assert (rows[:4] == U64(0xABABABABABABABAB)).all() and (rows[4 + 4 * nu:] == U64(0xABABABABABABABAB)).all()
                assert (bases[:32] == 0xAB).all() and (bases[32 + nb:] == 0xAB).all()
        # a NULL array with capacity 0 skips that array
        rows = np.zeros((nu, 4), dtype=U64)
        bases = np.zeros(nb, dtype=np.uint8)
        assert L.kh_unitigs_copy(dc._h, rows.ctypes.data, nu, None, 0) == native.KH_OK and np.array_equal(rows, ref.rows)
        assert L.kh_unitigs_copy(dc._h, None, 0, bases.ctypes.data, nb) == native.KH_OK and bases.tobytes() == ref.bases


def test_copy_device_unaligned_bases():
    import torch
    k = 21
    flat, keys, counts = chain_input(k)
    ref = ref_of("chains", keys, counts, k, 1)
    dev = torch.device("cuda:0")
    with native.DeviceCounter(k, capacity_hint=100_000, device=0) as dc:
        dc.push(flat)
        nu, nb = dc.unitigs_begin(1)
        d_rows = torch.zeros(4 * nu + 2, dtype=torch.int64, device=dev)
        raw = torch.full((nb + 64,), 0xAB, dtype=torch.uint8, device=dev)
        for off in (0, 1, 3, 7):
            raw.fill_(0xAB)
            d_rows.fill_(-1)
            torch.cuda.synchronize()
            dc.unitigs_copy_device(d_rows.data_ptr() + 8, nu, raw.data_ptr() + 16 + off, nb)
            host = raw.cpu().numpy()
            assert host[16 + off:16 + off + nb].tobytes() == ref.bases, off
            assert (host[:16 + off] == 0xAB).all() and (host[16 + off + nb:] == 0xAB).all()
            hr = d_rows.cpu().numpy().view(U64)
            assert np.array_equal(hr[1:1 + 4 * nu].reshape(nu, 4), ref.rows) and hr[0] == U64(ALL) and hr[-1] == U64(ALL)
        # too small: KH_ERR_RANGE, nothing written
        raw.fill_(0xAB)
        torch.cuda.synchronize()
        assert native.lib().kh_unitigs_copy_device(dc._h, d_rows.data_ptr() + 8, nu, raw.data_ptr(), nb - 1) == native.KH_ERR_RANGE
        assert (raw.cpu().numpy() == 0xAB).all()


def test_state_errors_and_empty_context():
    k = 21
    flat, keys, counts = chain_input(k)
    L = native.lib()
    rows = np.zeros((64, 4), dtype=U64)
    bases = np.zeros(1 << 16, dtype=np.uint8)
    copy = lambda dc: L.kh_unitigs_copy(dc._h, rows.ctypes.data, 64, bases.ctypes.data, bases.size)
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        assert L.kh_unitigs_end(dc._h) == native.KH_OK                       # end with nothing begun
        assert copy(dc) == native.KH_ERR_STATE and b"kh_unitigs_begin" in L.kh_last_error(dc._h)   # copy without begin
        assert dc.unitigs_begin(1) == (0, 0)                                  # an empty context works
        r, b = dc.unitigs_copy(0, 0)
        assert r.shape == (0, 4) and b.size == 0
        assert L.kh_unitigs_copy(dc._h, None, 0, None, 0) == native.KH_OK
        dc.push(flat)
        assert copy(dc) == native.KH_ERR_STATE                                # copy after kh_push
        nu, nb = dc.unitigs_begin(1)
        assert nu == len(CHAIN_L) and copy(dc) == native.KH_OK
        dc.reset()
        assert copy(dc) == native.KH_ERR_STATE                                # copy after kh_reset
        assert dc.unitigs_begin(1) == (0, 0)
        n1, n2 = C.c_uint64(7), C.c_uint64(7)
        assert L.kh_unitigs_begin(dc._h, 1, None, C.byref(n2)) == native.KH_ERR_BAD_ARG
        assert L.kh_unitigs_begin(None, 1, C.byref(n1), C.byref(n2)) == native.KH_ERR_BAD_ARG
        dc.push(flat)                                                         # usable afterwards
        assert dc.unitigs_begin(1)[0] == len(CHAIN_L)
    with native.DeviceCounter(k) as sh:                                       # a shard is refused, with kh_graph_*'s message
        sh.set_shard(0, 2)
        mine = keys[:64][np.array([native.owner(int(x), k, 2) == 0 for x in keys[:64]])]
        assert mine.size > 0
        sh.merge_pairs(mine, np.ones(mine.size, dtype=U64))
        n1, n2 = C.c_uint64(7), C.c_uint64(7)
        assert L.kh_unitigs_begin(sh._h, 1, C.byref(n1), C.byref(n2)) == native.KH_ERR_STATE
        assert b"the table is a shard; its k-mers' neighbours live on other owners" in L.kh_last_error(sh._h)
        assert (n1.value, n2.value) == (0, 0)
        assert sh.finish()["distinct"] == mine.size                           # usable afterwards


def test_count_sums_wrap_modulo_2_64():
    """Chosen counts: one chain of three nodes whose counts add up past 2^64."""
    k = 21
    s = b"ACGTTGCAAGGCTTAACCGATAG"[:k + 2]
    ks = [canon(s[i:i + k]) for i in range(3)]
    keys = np.array(sorted(pack_str(t) for t in ks), dtype=U64)
    counts = np.array([ALL - 1, 5, ALL], dtype=U64)
    with native.DeviceCounter(k) as dc:
        dc.merge_pairs(keys, counts)
        rows, bases, ref = check_unitigs(dc, "wrap", keys, counts, k, 1)
        assert rows.shape[0] == 1 and int(rows[0, native.UNI_KMERS]) == 3 and int(rows[0, native.UNI_COUNT_SUM]) == (2 * ALL + 4) % (1 << 64)


def test_product_library_once():
    """The same bytes on the library as it ships (no test switches): a child process that loads libkmerhip.so."""
    child = r"""
import sys, os
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["KMERHIP_LIB"] = "libkmerhip.so"
import numpy as np, torch
from krust_amd import native
import test_gpu_unitigs as U
k = 21
for tag, (flat, keys, counts) in (("chains", U.chain_input(k)), ("cycles", U.cycle_input(k))):
    with native.DeviceCounter(k, capacity_hint=3_000_000, path="partition") as a, native.DeviceCounter(k, path="direct") as b:
        a.push(flat)
        b.push(flat)
        assert a.finish()["slot_bytes"] == 8 and b.finish()["slot_bytes"] == 16
        for dc in (a, b):
            U.check_unitigs(dc, tag, keys, counts, k, 1)
print("RESULT ok", native.LIB_PATH)
"""
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + child], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout and "libkmerhip.so" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
