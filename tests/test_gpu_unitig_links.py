"""kh_unitigs_begin_linked / kh_unitigs_links_copy* -- the links between the unitigs of a count table -- against a reference in
Python strings.

Expected values never come from the library.  The unitigs are those of tests/test_gpu_unitigs.py's string walk (the same inputs
under the same tags, so that walk runs once per session); the links are derived from their sequences alone: a dictionary from
the spelled first k-mer of every unitig (entered as +) and the reverse complement of its last (entered as -), and for every end
k-mer w and letter c the string w[1:] + c, looked up there if its canonical form is a node.  The device's array must be that
list, sorted, word for word."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_graph as G
import test_gpu_join as T
import test_gpu_unitigs as U
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "unitig_links_child.py")
U64 = np.uint64
ALL = U.ALL


# ---- the reference: strings and a dict -----------------------------------------------------------------------------------------
def word(a, sa, b, sb):
    return ((2 * a + sa) << 32) | (2 * b + sb)


class LinkRef:
    """The links of a U.Ref: `links` (sorted uint64 words), and per unitig whether it is a palindrome."""

    def __init__(self, ref):
        k, S = ref.k, ref.S
        seqs = [u[1] for u in ref.unitigs]
        where = {}
        for j, s in enumerate(seqs):
            where[U.rc(s[-k:])] = (j, 1)
        for j, s in enumerate(seqs):
            where[s[:k]] = (j, 0)                      # + wins: a palindromic unitig is entered as +
        self.pal = [len(s) == k and U.rc(s) == s for s in seqs]
        self.degree = np.zeros((len(seqs), 2), dtype=np.int64)
        words = []
        for i, s in enumerate(seqs):
            for sign, w in ((0, s[-k:]), (1, U.rc(s[:k]))):
                for c in U.LETTERS:
                    t = w[1:] + c
                    if U.canon(t) in S:
                        assert t in where, (i, sign, t)       # a successor of an end state lies at an end of its unitig
                        j, sj = where[t]
                        words.append(word(i, sign, j, sj))
                        self.degree[i, sign] += 1
        words.sort()
        have = set(words)
        assert len(have) == len(words)                        # no word twice
        for w in words:                                       # the mirror of every link, modulo the sign of a palindrome
            a, sa, b, sb = w >> 33, (w >> 32) & 1, (w & 0xFFFFFFFF) >> 1, w & 1
            cands = [word(b, tb, a, ta) for tb in ((0, 1) if self.pal[b] else (1 - sb,)) for ta in ((0, 1) if self.pal[a] else (1 - sa,))]
            assert any(m in have for m in cands), (a, sa, b, sb)
        self.links = np.array(words, dtype=U64)


_LINKS = {}


def links_of(tag, keys, counts, k, mc):
    key = (tag, k, max(mc, 1))
    if key not in _LINKS:
        _LINKS[key] = LinkRef(U.ref_of(tag, keys, counts, k, mc))
    return _LINKS[key]


def pack_rows(strings, k):
    """Packed keys of equally long byte strings (numpy)."""
    if not strings:
        return np.empty(0, dtype=U64)
    b = np.frombuffer(b"".join(strings), dtype=np.uint8).reshape(len(strings), k)
    codes = ((b >> 1) ^ (b >> 2)) & 3
    acc = np.zeros(len(strings), dtype=U64)
    for i in range(k):
        acc = (acc << U64(2)) | codes[:, i].astype(U64)
    return acc


def degree_sum(dc, rows, bases, k, mc):
    """The sum of the out-degrees of all end states from kh_graph_masks of the end k-mers, which are cut from the bases: the + end
    spells the last k-mer of the sequence, the - end the reverse complement of the first."""
    raw = bases.tobytes()
    ends = []
    for r in rows:
        s = raw[int(r[0]):int(r[0]) + int(r[1]) + k - 1]
        ends += [s[-k:], U.rc(s[:k])]
    canon = [U.canon(w) for w in ends]
    sign = np.array([0 if w == c else 1 for w, c in zip(ends, canon)], dtype=np.uint8)   # (a palindrome: either nibble has the popcount)
    masks = dc.graph_masks(pack_rows(canon, k), mc) if ends else np.empty(0, dtype=np.uint8)
    bits = np.where(sign == 1, masks >> 4, masks & 15)
    return int(np.unpackbits(bits.astype(np.uint8)[:, None], axis=1).sum())


def check_linked(dc, tag, keys, counts, k, mc):
    ref = U.ref_of(tag, keys, counts, k, mc)
    lref = links_of(tag, keys, counts, k, mc)
    nu, nb, nl = dc.unitigs_begin_linked(mc)
    try:
        assert (nu, nb, nl) == (ref.rows.shape[0], len(ref.bases), lref.links.size), (k, mc, nu, nb, nl, lref.links.size)
        rows, bases = dc.unitigs_copy(nu, nb)
        links = dc.unitigs_links_copy(nl)
    finally:
        dc.unitigs_end()
    assert rows.dtype == U64 and rows.shape == ref.rows.shape and bases.dtype == np.uint8          # U.check_unitigs' comparison
    assert np.array_equal(rows, ref.rows), (k, mc, np.argwhere(rows != ref.rows)[:4])
    assert bases.tobytes() == ref.bases, (k, mc)
    assert links.dtype == U64 and links.shape == lref.links.shape
    bad = np.flatnonzero(links != lref.links)
    assert bad.size == 0, (k, mc, bad[:8], links[bad[:8]], lref.links[bad[:8]])
    assert (links[1:] > links[:-1]).all()                                                             # ascending, no word twice
    assert links.size == degree_sum(dc, rows, bases, k, mc), (k, mc)                                   # the independent degree check
    a, sa, b, sb = native.uni_link_fields(links)
    assert (a < max(nu, 1)).all() and (b < max(nu, 1)).all()
    return rows, bases, links, lref


# ---- dense small k: palindromes, loops, hairpins, k = 1 ---------------------------------------------------------------------------------
def test_small_inputs_hold_self_links_and_palindromic_unitigs():
    """Precondition, from the reference alone: among the small cases are links of a unitig to itself in every sign pair, and links
    into and out of palindromic unitigs."""
    seen = set()
    into_pal = 0
    for k, d in U.SMALL:
        keys, counts = U.small_case(k, d)
        for mc in (1, 2):
            lr = links_of(("small", d), keys, counts, k, mc)
            for w in lr.links.tolist():
                a, sa, b, sb = w >> 33, (w >> 32) & 1, (w & 0xFFFFFFFF) >> 1, w & 1
                if a == b:
                    seen.add((sa, sb))
                into_pal += lr.pal[b]
    assert seen == {(0, 0), (0, 1), (1, 0), (1, 1)} and into_pal > 0, (seen, into_pal)


@pytest.mark.parametrize("k,density", U.SMALL, ids=[f"k{k}-d{d}" for k, d in U.SMALL])
def test_small_k_dense(k, density):
    keys, counts = U.small_case(k, density)
    with native.DeviceCounter(k) as dc:
        dc.merge_pairs(keys, counts)
        for mc in (1, 2):
            check_linked(dc, ("small", density), keys, counts, k, mc)


# ---- cycles and disjoint chains -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_cycles(k):
    flat, keys, counts = U.cycle_input(k)
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        rows, _, links, _ = check_linked(dc, "cycles", keys, counts, k, 1)
    circ = np.flatnonzero(rows[:, native.UNI_FLAGS] == 1)
    assert circ.size >= len(U.PERIODS)
    want = sorted(word(int(i), s, int(i), s) for i in circ for s in (0, 1))     # i+ -> i+ and i- -> i-, nothing else:
    assert links.tolist() == want                                               # the ordinary chains have none


def test_disjoint_chains_have_no_links():
    """n_links == 0: nothing is allocated, and the copies accept NULL, 0."""
    k = 21
    flat, keys, counts = U.chain_input(k)
    L = native.lib()
    with native.DeviceCounter(k, capacity_hint=100_000, device=0) as dc:
        dc.push(flat)
        _, _, links, _ = check_linked(dc, "chains", keys, counts, k, 1)
        assert links.size == 0
        nu, nb, nl = dc.unitigs_begin_linked(1)
        assert nu == len(U.CHAIN_L) and nl == 0
        assert L.kh_unitigs_links_copy(dc._h, None, 0) == native.KH_OK
        assert L.kh_unitigs_links_copy_device(dc._h, None, 0) == native.KH_OK
        canary = np.full(4, 0xABABABABABABABAB, dtype=U64)
        assert L.kh_unitigs_links_copy(dc._h, canary.ctypes.data, 4) == native.KH_OK and (canary == U64(0xABABABABABABABAB)).all()
        dc.unitigs_end()


# ---- branching, realistic ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_branching_reads_and_stars(k):
    flat, keys, counts = G.main_input(k)
    with native.DeviceCounter(k, capacity_hint=3_000_000) as dc:
        dc.push(flat)
        for mc in (1, 2, ALL):
            if mc == ALL:
                assert dc.unitigs_begin_linked(mc) == (0, 0, 0)
                assert dc.unitigs_links_copy(0).size == 0
                dc.unitigs_end()
                continue
            rows, _, links, _ = check_linked(dc, "main", keys, counts, k, mc)
            if k == 11 and mc == 1:
                assert links.size > 100_000        # offsets cross every wave, block and scan-tile edge
            if mc == 1:
                assert links.size > rows.shape[0] // 2


# ---- table forms and geometries: identical bytes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", U.FORMS)
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
            check_linked(dc, "main", keys, counts, k, mc)
        assert T.stats_of(dc) == before


# ---- the contract ------------------------------------------------------------------------------------------------------------------------------
def test_caps_between_canaries():
    k = 21
    flat, keys, counts = U.cycle_input(k)
    lref = links_of("cycles", keys, counts, k, 1)
    L = native.lib()
    CAN = U64(0xABABABABABABABAB)
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        nu, nb, nl = dc.unitigs_begin_linked(1)
        assert nl == lref.links.size and nl > 2
        for cap in (0, 1, nl - 1, nl, nl + 3):
            buf = np.full(nl + 8, CAN, dtype=U64)
            rc_ = L.kh_unitigs_links_copy(dc._h, buf[4:].ctypes.data, cap)
            if cap < nl:
                assert rc_ == native.KH_ERR_RANGE and (buf == CAN).all(), cap          # NOTHING is written
                assert b"link array too small" in L.kh_last_error(dc._h)
            else:
                assert rc_ == native.KH_OK and np.array_equal(buf[4:4 + nl], lref.links)
                assert (buf[:4] == CAN).all() and (buf[4 + nl:] == CAN).all()
        assert L.kh_unitigs_links_copy(dc._h, None, 0) == native.KH_OK                  # a NULL array with capacity 0 skips
        assert L.kh_unitigs_links_copy(dc._h, None, nl) == native.KH_ERR_BAD_ARG
        n1, n2, n3 = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        assert L.kh_unitigs_begin_linked(dc._h, 1, C.byref(n1), C.byref(n2), None) == native.KH_ERR_BAD_ARG
        assert L.kh_unitigs_begin_linked(dc._h, 1, None, C.byref(n2), C.byref(n3)) == native.KH_ERR_BAD_ARG
        assert L.kh_unitigs_begin_linked(None, 1, C.byref(n1), C.byref(n2), C.byref(n3)) == native.KH_ERR_BAD_ARG
        assert dc.unitigs_begin_linked(1) == (nu, nb, nl)                               # usable afterwards


def test_copy_device_into_an_offset():
    import torch
    k = 21
    flat, keys, counts = U.cycle_input(k)
    lref = links_of("cycles", keys, counts, k, 1)
    dev = torch.device("cuda:0")
    with native.DeviceCounter(k, capacity_hint=100_000, device=0) as dc:
        dc.push(flat)
        nu, nb, nl = dc.unitigs_begin_linked(1)
        assert nl == lref.links.size
        d = torch.full((nl + 5,), -1, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        dc.unitigs_links_copy_device(d.data_ptr() + 24, nl + 2)
        h = d.cpu().numpy().view(U64)
        assert np.array_equal(h[3:3 + nl], lref.links) and (h[:3] == U64(ALL)).all() and (h[3 + nl:] == U64(ALL)).all()
        d.fill_(-1)
        torch.cuda.synchronize()
        assert native.lib().kh_unitigs_links_copy_device(dc._h, d.data_ptr() + 8, nl - 1) == native.KH_ERR_RANGE
        assert (d.cpu().numpy() == -1).all()
        dc.unitigs_links_copy_device(d, nl)                                             # a tensor as it is
        assert np.array_equal(d.cpu().numpy().view(U64)[:nl], lref.links)


def test_state_errors_readers_and_release(monkeypatch):
    k = 21
    flat, keys, counts = U.cycle_input(k)
    lref = links_of("cycles", keys, counts, k, 1)
    ref = U.ref_of("cycles", keys, counts, k, 1)
    L = native.lib()
    buf = np.zeros(lref.links.size + 16, dtype=U64)
    copy = lambda dc: L.kh_unitigs_links_copy(dc._h, buf.ctypes.data, buf.size)
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        assert copy(dc) == native.KH_ERR_STATE and b"kh_unitigs_begin_linked" in L.kh_last_error(dc._h)     # not begun
        assert dc.unitigs_begin_linked(1) == (0, 0, 0)                                                      # an empty context works
        assert copy(dc) == native.KH_OK and L.kh_unitigs_links_copy(dc._h, None, 0) == native.KH_OK
        dc.push(flat)
        assert copy(dc) == native.KH_ERR_STATE                                                              # stale: after a push
        nu, nb, nl = dc.unitigs_begin_linked(1)
        assert nl == lref.links.size
        # readers between begin and copy leave the links valid
        assert np.array_equal(dc.lookup(keys[:100]), counts[:100])
        dc.histogram()
        dc.graph_stats(1)
        assert np.array_equal(dc.unitigs_links_copy(nl), lref.links)
        rows, bases = dc.unitigs_copy(nu, nb)                                                               # kh_unitigs_copy after either begin
        assert np.array_equal(rows, ref.rows) and bases.tobytes() == ref.bases
        # a plain begin after a linked one releases the links: the copies refuse, and name the other begin
        assert dc.unitigs_begin(1) == (nu, nb)
        assert copy(dc) == native.KH_ERR_STATE and b"kh_unitigs_begin_linked" in L.kh_last_error(dc._h)
        assert L.kh_unitigs_links_copy_device(dc._h, None, 0) == native.KH_ERR_STATE
        rows, bases = dc.unitigs_copy(nu, nb)
        assert np.array_equal(rows, ref.rows) and bases.tobytes() == ref.bases
        # ... and a linked one after a plain one builds them again
        assert dc.unitigs_begin_linked(1) == (nu, nb, nl) and copy(dc) == native.KH_OK and np.array_equal(buf[:nl], lref.links)
        dc.unitigs_end()
        assert copy(dc) == native.KH_ERR_STATE                                                              # after kh_unitigs_end
        assert dc.unitigs_begin_linked(1) == (nu, nb, nl)
        dc.reset()
        assert copy(dc) == native.KH_ERR_STATE                                                              # after kh_reset
        rows, bases, links = dc.unitigs_linked(1)
        assert rows.shape == (0, 4) and bases.size == 0 and links.size == 0
    with native.DeviceCounter(k) as sh:                                                                     # a shard is refused
        sh.set_shard(0, 2)
        mine = keys[:64][np.array([native.owner(int(x), k, 2) == 0 for x in keys[:64]])]
        assert mine.size > 0
        sh.merge_pairs(mine, np.ones(mine.size, dtype=U64))
        n1, n2, n3 = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
        assert L.kh_unitigs_begin_linked(sh._h, 1, C.byref(n1), C.byref(n2), C.byref(n3)) == native.KH_ERR_STATE
        assert b"the table is a shard; its k-mers' neighbours live on other owners" in L.kh_last_error(sh._h)
        assert (n1.value, n2.value, n3.value) == (0, 0, 0)
        assert L.kh_unitigs_links_copy(sh._h, buf.ctypes.data, buf.size) == native.KH_ERR_STATE
        assert sh.finish()["distinct"] == mine.size                                                         # usable afterwards


# ---- fresh child processes: the product library, and past the first grid stride ------------------------------------------------------
_CHILD_DIED = []


def run_child(path, env, timeout):
    """One child under its own timeout.  After a child that ended on a signal or at its timeout no further one is started."""
    assert not _CHILD_DIED, f"not started: an earlier child ended on a signal or at its timeout ({_CHILD_DIED[0]})"
    try:
        p = subprocess.run([sys.executable, CHILD, str(path)], capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append("timeout")
        raise
    if p.returncode < 0:
        _CHILD_DIED.append(f"signal {-p.returncode}")
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def case_file(tmp_path, name):
    """The input of a child and what the reference expects of it."""
    if name == "branching":
        k, mc, hint = 21, 1, 3_000_000
        flat, keys, counts = G.main_input(k)
        tag, inp = "main", {"flat": flat}
    elif name == "cycles":
        k, mc, hint = 21, 1, 100_000
        flat, keys, counts = U.cycle_input(k)
        tag, inp = "cycles", {"flat": flat}
    else:
        k, mc, hint = 4, 1, 0
        keys, counts = U.small_case(k, 1.0)
        tag, inp = ("small", 1.0), {"keys": keys, "counts": counts}
    ref, lref = U.ref_of(tag, keys, counts, k, mc), links_of(tag, keys, counts, k, mc)
    path = tmp_path / f"{name}.npz"
    np.savez(path, k=k, mc=mc, hint=hint, rows=ref.rows, bases=np.frombuffer(ref.bases, dtype=np.uint8), links=lref.links, **inp)
    return path, ref, lref


def test_product_library_once(tmp_path):
    """The same bytes on the library as it ships (no test switches)."""
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    env.pop("KMERHIP_GRID_CAP", None)
    for name in ("cycles", "branching"):
        path, _, lref = case_file(tmp_path, name)
        out = run_child(path, env, 300)
        assert "libkmerhip.so" in out and f"links {lref.links.size}" in out, out


@pytest.mark.parametrize("cap", [1, 3])
@pytest.mark.parametrize("name", ["branching", "small"])
def test_past_the_first_grid_stride(tmp_path, name, cap):
    """KMERHIP_GRID_CAP (test build) = 1 and 3, one value per process: at 1 one workgroup goes round its loop as often as there are
    blocks of end states, at 3 the workgroups make unequal numbers of trips."""
    path, ref, lref = case_file(tmp_path, name)
    if name == "branching":
        blocks = -(-2 * ref.rows.shape[0] // 256)
        assert -(-blocks // min(cap, blocks)) >= (3 if cap == 1 else 2), blocks      # the link kernels' loops do go round
    env = dict(os.environ, KMERHIP_GRID_CAP=str(cap))
    assert env.get("KMERHIP_LIB") == "libkmerhip_testing.so"
    out = run_child(path, env, 300)
    assert f"cap {cap}" in out and "libkmerhip_testing.so" in out and f"links {lref.links.size}" in out, out
