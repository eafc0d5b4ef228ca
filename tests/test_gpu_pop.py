"""kh_pop_bubbles_into -- one round of bubble popping of a count table's compacted graph into another context -- against the rule in
Python strings (tests/test_pop_ref.py).

Expected values never come from the library: the unitigs and links are those of the string references of tests/test_gpu_unitigs.py
and tests/test_gpu_unitig_links.py, the decision and the surviving pairs are PopRef's.  The target table is compared word for word,
the nine statistics words exactly.  The input at size is a planted-variant one (planted()): the inputs of the neighbouring files
hold no class of three, and tests/test_gpu_unitigs.SMALL holds no class of two at all -- it serves as the "nothing is popped" case."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_clip_ref as CR
import test_gpu_graph as G
import test_gpu_join as T
import test_gpu_unitig_links as LR
import test_gpu_unitigs as U
import test_pop_ref as R
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "pop_child.py")
U64 = np.uint64
ALL = U.ALL
HINT = 3_000_000
_POPS = {}
_PLANTED = {}


def pop_of(tag, keys, counts, k, mc, max_kmers):
    key = (tag, k, max(mc, 1), max_kmers)
    if key not in _POPS:
        _POPS[key] = R.PopRef(U.ref_of(tag, keys, counts, k, mc), LR.links_of(tag, keys, counts, k, mc), max_kmers)
    return _POPS[key]


def words_dict(pr):
    return dict(zip(native.POP_NAMES, pr.words))


def check_pop(src, tag, keys, counts, k, mc, max_kmers, dst, pr=None):
    """One call into an EMPTY dst: its table against the reference's surviving pairs, the nine words, and src unchanged."""
    pr = pr or pop_of(tag, keys, counts, k, mc, max_kmers)
    before, s0 = T.stats_of(src), src.result_sorted(1)
    got = dst.pop_bubbles_into(src, mc, max_kmers)
    assert got == words_dict(pr), (k, mc, max_kmers, got, words_dict(pr))
    gk, gc = dst.result_sorted(1)
    assert gk.dtype == U64 and gk.shape == pr.keys.shape, (k, mc, max_kmers, gk.shape, pr.keys.shape)
    assert np.array_equal(gk, pr.keys) and np.array_equal(gc, pr.counts), (k, mc, max_kmers)
    st = dst.finish()
    assert st["distinct"] == pr.keys.size and st["kmers"] == pr.words[native.POP_KEPT_COUNT]
    s1 = src.result_sorted(1)
    assert T.stats_of(src) == before and np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
    return pr


# ---- the planted-variant input -----------------------------------------------------------------------------------------------------------
COUNTS = ((5, 3, 2), (3, 5, 1), (4, 4, 4), (2, 2, 1))
LETTERS = b"ACGT"


def planted_reads(k, seed=2026):
    """10 segments of 2000 random bases, three haplotypes of each as (sequence, count) reads.  About every 3k to 5k bases a site:
    a SNP, a SNP with a third allele, an insertion of 1 to 3 bases, or a SNP followed by another closer than k.  Haplotype 0 is the
    segment, 1 has every variant, 2 the third allele where there is one and else either of the two."""
    rng = np.random.default_rng(seed + k)
    reads = []
    for s in range(10):
        seg = CR.rand_bases(rng, 2000)
        haps = [bytearray(), bytearray(), bytearray()]
        pos = 0
        while True:
            nxt = pos + int(rng.integers(3 * k, 5 * k + 1))
            if nxt + 2 * k >= len(seg):
                break
            for h in haps:
                h += seg[pos:nxt]
            kind = int(rng.integers(0, 4))
            others = [c for c in LETTERS if c != seg[nxt]]
            pick = int(rng.integers(0, 2))                                 # what haplotype 2 takes where there are two alleles
            if kind == 2:                                                   # an insertion in front of seg[nxt]
                ins = CR.rand_bases(rng, int(rng.integers(1, 4)))
                haps[1] += ins
                if pick:
                    haps[2] += ins
                pos = nxt
                continue
            haps[0].append(seg[nxt])
            haps[1].append(others[0])
            haps[2].append(others[1] if kind == 1 else others[0] if pick else seg[nxt])
            pos = nxt + 1
            if kind == 3:                                                   # a second SNP closer than k
                d = int(rng.integers(1, k))
                for h in haps:
                    h += seg[pos:pos + d - 1]
                p2 = pos + d - 1
                alt = [c for c in LETTERS if c != seg[p2]][0]
                pick2 = int(rng.integers(0, 2))
                haps[0].append(seg[p2])
                haps[1].append(alt)
                haps[2].append(alt if pick2 else seg[p2])
                pos = p2 + 1
        for h in haps:
            h += seg[pos:]
        reads += [(bytes(h), c) for h, c in zip(haps, COUNTS[s % 4])]
    return reads


def planted(k):
    """(flat buffer to push, sorted keys, counts) of planted_reads(k): every read is in the buffer as often as its count says."""
    if k not in _PLANTED:
        reads = planted_reads(k)
        keys, counts = CR.pairs_of_S(CR.S_of_reads(reads, k), k)
        flat = np.frombuffer(b"N".join(seq for seq, c in reads for _ in range(c)) + b"N", dtype=np.uint8).copy()
        for a in (flat, keys, counts):
            a.setflags(write=False)
        _PLANTED[k] = (flat, keys, counts)
    return _PLANTED[k]


def bounds(k):
    return (k, 2 * k, ALL)


@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_the_planted_input_holds_every_kind_of_decision(k):
    """Precondition, from the reference alone, before any device call: popped unitigs, candidates that stay, a class of three,
    decisions by the mean count and by the index -- and enough unitigs for more than one workgroup."""
    flat, keys, counts = planted(k)
    assert 20_000 <= keys.size <= 34_000, keys.size
    for mk in bounds(k):
        pr = pop_of("planted", keys, counts, k, 1, mk)
        w = words_dict(pr)
        assert 500 <= w["unitigs"] <= 3500 and w["unitigs"] > 256, w
        assert w["popped"] > 0 and w["candidates"] - w["popped"] > 0 and w["bubbles"] > 0, (k, mk, w)
        assert pr.largest >= 3 and pr.by["mean"] > 0 and pr.by["index"] > 0, (k, mk, pr.largest, pr.by)
    mid = pop_of("planted", keys, counts, k, 1, 2 * k)
    assert mid.by["kmers"] > 0 and mid.alone > 0                                     # insertions with equal counts; candidates without a parallel
    if k == 21:
        assert keys.size == 26340 and mid.words[:3] == [801, 516, 241] and mid.words[native.POP_BUBBLES] == 188


# ---- A. hand-built graphs: every kind of decision ----------------------------------------------------------------------------------------
def built_cases(k):
    """(name, node set, max_kmers): the bubbles of tests/test_pop_ref.py, and a fork and a tip of tests/test_clip_ref.py."""
    S = lambda alleles: CR.S_of_reads(R.bubble_reads(k, alleles), k)
    out = [(f"snp{c1}{c2}", S([(b"A", b"", c1), (b"C", b"", c2)]), 2 * k) for c1, c2 in ((3, 2), (2, 3), (2, 2))]
    out.append(("insertion", S([(b"A", b"", 3), (b"C", b"GTC", 3)]), 2 * k))
    out.append(("three", S([(b"A", b"", 4), (b"C", b"", 3), (b"G", b"", 2)]), 2 * k))
    out.append(("below", S([(b"A", b"", 3), (b"C", b"", 2)]), k - 1))
    out.append(("at", S([(b"A", b"", 3), (b"C", b"", 2)]), k))
    out.append(("long-beside", S([(b"A", b"", 1), (b"C", b"G", 9)]), k))
    out.append(("long-beside+1", S([(b"A", b"", 1), (b"C", b"G", 9)]), k + 1))
    out.append(("fork", CR.S_of_reads(CR.fork_reads(k, 3, 2), k), ALL))
    out.append(("tip", CR.S_of_reads(CR.fork_reads(k, 9, 1, len1=10, len2=60), k), 2 * k))
    return out


@pytest.mark.parametrize("k", [21, 32])
def test_hand_built_bubbles(k):
    by = {"mean": 0, "kmers": 0, "index": 0}
    with native.DeviceCounter(k) as src, native.DeviceCounter(k) as dst:
        for name, S, mk in built_cases(k):
            keys, counts = CR.pairs_of_S(S, k)
            src.reset()
            dst.reset()
            src.merge_pairs(keys, counts)
            _, pr = R.pop_of_S(S, k, mk)
            check_pop(src, name, keys, counts, k, 1, mk, dst, pr=pr)
            for name_ in by:
                by[name_] += pr.by[name_]
            if name in ("below", "long-beside", "fork", "tip"):
                assert pr.words[native.POP_POPPED] == 0 and np.array_equal(dst.result_sorted(1)[0], keys)
    assert all(v > 0 for v in by.values()), by


def test_a_wrapped_count_sum_and_a_128_bit_comparison():
    """A SNP bubble with counts 2^62 + 1 and 2^62 at k = 21: the branches' COUNT_SUM wrap to 2^62 + 21 and 2^62, and their products
    with KMERS = 21 pass 2^64.  The words as stored decide: the first branch stays."""
    k = 21
    reads = R.bubble_reads(k, [(b"A", b"", (1 << 62) + 1), (b"C", b"", 1 << 62)])
    S = CR.S_of_reads(reads, k)
    ref, pr = R.pop_of_S(S, k, 2 * k)
    a, c = (R.branch_of(ref, r[0], k) for r in reads)
    assert [ref.unitigs[i][3] % (1 << 64) for i in (a, c)] == [(1 << 62) + 21, 1 << 62] and ref.unitigs[a][3] >= 1 << 64
    assert pr.popped[c] and not pr.popped[a] and pr.by["mean"] == 2 and pr.words[native.POP_POPPED_COUNT] == 1 << 62
    keys, counts = CR.pairs_of_S(S, k)
    with native.DeviceCounter(k) as src, native.DeviceCounter(k) as dst:
        src.merge_pairs(keys, counts)
        check_pop(src, "wrap", keys, counts, k, 1, 2 * k, dst, pr=pr)


# ---- dense small k: nothing is popped ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,density", U.SMALL, ids=[f"k{k}-d{d}" for k, d in U.SMALL])
def test_small_k_dense_pops_nothing(k, density):
    keys, counts = U.small_case(k, density)
    with native.DeviceCounter(k) as src, native.DeviceCounter(k) as dst:
        src.merge_pairs(keys, counts)
        for mk in (1, 3, ALL):
            dst.reset()
            pr = check_pop(src, ("small", density), keys, counts, k, 1, mk, dst)
            assert pr.words[2:5] == [0, 0, 0] and pr.words[native.POP_BUBBLES] == 0
            gk, gc = dst.result_sorted(1)
            assert np.array_equal(gk, keys) and np.array_equal(gc, counts)              # dst equals S


def test_small_k_dense_holds_self_blocked_unitigs():
    assert sum(pop_of(("small", d), *U.small_case(k, d), k, 1, ALL).self_blocked for k, d in U.SMALL) > 0


# ---- B. planted variants at size -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_planted_variants(k):
    flat, keys, counts = planted(k)
    refs = {mk: pop_of("planted", keys, counts, k, 1, mk) for mk in bounds(k)}
    with native.DeviceCounter(k, capacity_hint=HINT) as src, native.DeviceCounter(k, capacity_hint=HINT) as dst:
        src.push(flat)
        for mk in refs:
            dst.reset()
            check_pop(src, "planted", keys, counts, k, 1, mk, dst)


# ---- C. variants at k = 21 --------------------------------------------------------------------------------------------------------------------
def test_min_count_two():
    k = 21
    flat, keys, counts = planted(k)
    pr = pop_of("planted", keys, counts, k, 2, 2 * k)
    assert pr.keys.size < keys.size and pr.words[native.POP_UNITIGS] != pop_of("planted", keys, counts, k, 1, 2 * k).words[native.POP_UNITIGS]
    with native.DeviceCounter(k, capacity_hint=HINT) as src, native.DeviceCounter(k, capacity_hint=HINT) as dst:
        src.push(flat)
        check_pop(src, "planted", keys, counts, k, 2, 2 * k, dst)


@pytest.mark.parametrize("form", U.FORMS)
def test_table_forms_of_src(form, monkeypatch):
    """Every table form gives the same pairs and words.  The planted input is too small to make a table of 64 regions grow, so the
    "grown" form holds the reads and stars of tests/test_gpu_graph.py instead (classes of two, and popped unitigs, at min_count 1)."""
    k = 21
    tag, (flat, keys, counts) = ("main", G.main_input(k)) if form == "grown" else ("planted", planted(k))
    mk = k if form == "grown" else 2 * k
    assert pop_of(tag, keys, counts, k, 1, mk).words[native.POP_POPPED] > 0
    if form in ("wide", "image", "regions3072", "grown"):
        src = T.table(form, k, flat, monkeypatch)
    else:
        if form == "narrow0":
            monkeypatch.setenv("KMERHIP_NARROW", "0")
        if form == "pow2":
            monkeypatch.setenv("KMERHIP_POW2_TABLE", "1")
        src = native.DeviceCounter(k, capacity_hint=1 if form == "hint1" else HINT, path="partition" if form == "narrow0" else None)
        src.push(flat)
        src.finish()
    monkeypatch.delenv("KMERHIP_NARROW", raising=False)
    monkeypatch.delenv("KMERHIP_POW2_TABLE", raising=False)
    with src, native.DeviceCounter(k, capacity_hint=HINT) as dst:
        check_pop(src, tag, keys, counts, k, 1, mk, dst)


def test_dst_variants():
    """A dst without a hint, and one that already holds pairs: the counts add."""
    k, mk = 21, 42
    flat, keys, counts = planted(k)
    pr = pop_of("planted", keys, counts, k, 1, mk)
    with native.DeviceCounter(k, capacity_hint=HINT) as src:
        src.push(flat)
        with native.DeviceCounter(k) as plain:
            check_pop(src, "planted", keys, counts, k, 1, mk, plain)
        gone = np.setdiff1d(keys, pr.keys)
        assert gone.size >= 500
        rng = np.random.default_rng(9)
        mine_k = np.concatenate([rng.choice(pr.keys, 500, replace=False), rng.choice(gone, 500, replace=False)])
        mine_c = (np.arange(1000) + 7).astype(U64)
        want = dict(zip(pr.keys.tolist(), pr.counts.tolist()))
        for x, c in zip(mine_k.tolist(), mine_c.tolist()):
            want[x] = want.get(x, 0) + c
        with native.DeviceCounter(k, capacity_hint=HINT) as held:
            held.merge_pairs(mine_k, mine_c)
            assert held.pop_bubbles_into(src, 1, mk) == words_dict(pr)
            gk, gc = held.result_sorted(1)
            assert gk.size == pr.keys.size + 500 and dict(zip(gk.tolist(), gc.tolist())) == want


def test_a_pending_push_is_counted_first_and_begun_unitigs_are_released():
    k = 21
    flat, keys, counts = planted(k)
    pr = pop_of("planted", keys, counts, k, 1, 2 * k)
    L = native.lib()
    with native.DeviceCounter(k, capacity_hint=HINT) as src, native.DeviceCounter(k, capacity_hint=HINT) as dst:
        src.push(flat)
        assert dst.pop_bubbles_into(src) == words_dict(pr)                                   # the defaults: 1 and 2 k
        nu, nb, nl = src.unitigs_begin_linked(1)
        assert (nu, nl) == (pr.words[native.POP_UNITIGS], pr.words[native.POP_LINKS])
        dst.reset()
        assert dst.pop_bubbles_into(src, 1, 2 * k) == words_dict(pr)
        rows = np.zeros((nu, 4), dtype=U64)
        bases = np.zeros(nb, dtype=np.uint8)
        assert L.kh_unitigs_copy(src._h, rows.ctypes.data, nu, bases.ctypes.data, nb) == native.KH_ERR_STATE
        assert L.kh_unitigs_links_copy(src._h, None, 0) == native.KH_ERR_STATE
        assert src.unitigs_begin_linked(1) == (nu, nb, nl)                                   # and a begin works again
        src.unitigs_end()


def test_clip_and_pop_rounds_until_nothing_changes():
    """Two contexts ping-pong, a clip round and a pop round in turn with kh_reset between, against ClipRef and PopRef chained the
    same way; it ends when a round of each in a row changed nothing.  Then the unitigs of the final table."""
    k = 21
    flat, keys, counts = planted(k)
    S = U.node_dict(keys, counts, k, 1)
    a, b = native.DeviceCounter(k, capacity_hint=HINT), native.DeviceCounter(k, capacity_hint=HINT)
    with a, b:
        a.push(flat)
        rounds, quiet, removed = 0, 0, {"clip": 0, "pop": 0}
        while quiet < 2:
            which = "clip" if rounds % 2 == 0 else "pop"
            if which == "clip":
                _, ref = CR.clip_of_S(S, k, k)
                got = b.clip_tips_into(a, 1, k)
                assert got == dict(zip(native.CLIP_NAMES, ref.words)), (rounds, got, ref.words)
                n = got["clipped"]
            else:
                _, ref = R.pop_of_S(S, k, 2 * k)
                got = b.pop_bubbles_into(a, 1, 2 * k)
                assert got == words_dict(ref), (rounds, got, ref.words)
                n = got["popped"]
            gk, gc = b.result_sorted(1)
            assert np.array_equal(gk, ref.keys) and np.array_equal(gc, ref.counts), rounds
            S = ref.S_next
            removed[which] += n
            quiet = quiet + 1 if n == 0 else 0
            rounds += 1
            a.reset()
            a, b = b, a
            assert rounds <= 10, rounds
        assert removed["pop"] > 0 and 3 <= rounds <= 10, (rounds, removed)
        fk, fc = CR.pairs_of_S(S, k)
        U.check_unitigs(a, "simplified-final", fk, fc, k, 1, ref=U.Ref(S, k))


# ---- D. the contract ------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_contexts_usable():
    k = 21
    S = CR.S_of_reads(R.snp(k, 3, 2), k)
    keys, counts = CR.pairs_of_S(S, k)
    _, pr = R.pop_of_S(S, k, 2 * k)
    _, pr0 = R.pop_of_S(S, k, 0)
    L = native.lib()
    zeros = dict(zip(native.POP_NAMES, [0] * 9))
    out = np.full(native.POP_WORDS, 7, dtype=U64)
    with native.DeviceCounter(k) as src, native.DeviceCounter(k) as dst, native.DeviceCounter(k + 1) as other, native.DeviceCounter(k) as sh:
        assert dst.pop_bubbles_into(src, 1, k) == zeros                                                           # an empty src: KH_OK, all words 0
        assert dst.finish()["distinct"] == 0
        src.merge_pairs(keys, counts)
        assert L.kh_pop_bubbles_into(dst._h, dst._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert b"kh_pop_bubbles_into: dst must not be src" in L.kh_last_error(dst._h)
        assert L.kh_pop_bubbles_into(dst._h, None, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert L.kh_pop_bubbles_into(dst._h, src._h, 1, k, None) == native.KH_ERR_BAD_ARG
        assert L.kh_pop_bubbles_into(None, src._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert L.kh_pop_bubbles_into(other._h, src._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG and b"different k" in L.kh_last_error(other._h)
        assert L.kh_pop_bubbles_into(dst._h, other._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        sh.set_shard(0, 2)
        mine = keys[np.array([native.owner(int(x), k, 2) == 0 for x in keys])]
        sh.merge_pairs(mine, np.ones(mine.size, dtype=U64))
        assert L.kh_pop_bubbles_into(dst._h, sh._h, 1, k, out.ctypes.data) == native.KH_ERR_STATE                 # a shard as src
        assert L.kh_pop_bubbles_into(sh._h, src._h, 1, k, out.ctypes.data) == native.KH_ERR_STATE                 # ... and as dst
        assert (out == U64(7)).all()                                                                              # nothing was written
        assert sh.finish()["distinct"] == mine.size and other.finish()["distinct"] == 0 and dst.finish()["distinct"] == 0
        check_pop(src, "snp32", keys, counts, k, 1, 2 * k, dst, pr=pr)                                            # all of them usable
        assert np.array_equal(src.lookup(keys), counts)
        assert int(src.graph_stats(1)[native.GRAPH_NODES]) == keys.size
        dst.reset()
        check_pop(src, "snp32", keys, counts, k, 1, 0, dst, pr=pr0)                                               # max_kmers = 0 copies S
        gk, gc = dst.result_sorted(1)
        assert np.array_equal(gk, keys) and np.array_equal(gc, counts)
        dst.reset()
        assert dst.pop_bubbles_into(src, ALL, 2 * k) == zeros                                                     # an empty S
        assert dst.finish()["distinct"] == 0


# ---- E, F. fresh child processes: the product library, and past the first grid stride -------------------------------------------------------
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


def case_file(tmp_path, k):
    flat, keys, counts = planted(k)
    pr = pop_of("planted", keys, counts, k, 1, 2 * k)
    path = tmp_path / f"pop{k}.npz"
    np.savez(path, k=k, mc=1, max_kmers=2 * k, hint=HINT, flat=flat, keys=pr.keys, counts=pr.counts, words=np.array(pr.words, dtype=U64))
    return path, pr


def test_product_library_once(tmp_path):
    """The same pairs and words on the library as it ships (no test switches)."""
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    env.pop("KMERHIP_GRID_CAP", None)
    path, pr = case_file(tmp_path, 21)
    out = run_child(path, env, 300)
    assert "libkmerhip.so" in out and f"popped {pr.words[native.POP_POPPED]}" in out, out


@pytest.mark.parametrize("cap", [1, 3])
def test_past_the_first_grid_stride(tmp_path, cap):
    """KMERHIP_GRID_CAP (test build) = 1 and 3, one value per process: the two decision kernels run over the unitigs -- more than
    one workgroup's, so that at cap 1 a workgroup goes round their loops again --, the keep kernel over the nodes, which are more."""
    path, pr = case_file(tmp_path, 11)
    blocks = -(-pr.words[native.POP_UNITIGS] // 256)
    assert blocks > cap and -(-blocks // cap) >= 2, blocks
    env = dict(os.environ, KMERHIP_GRID_CAP=str(cap))
    assert env.get("KMERHIP_LIB") == "libkmerhip_testing.so"
    out = run_child(path, env, 300)
    assert f"cap {cap}" in out and "libkmerhip_testing.so" in out and f"popped {pr.words[native.POP_POPPED]}" in out, out
