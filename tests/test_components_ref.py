"""The connected components of the unitig graph (kh_unitigs_components*) and one round of dropping the small ones
(kh_drop_components_into): the reference, on the CPU alone.

Two independent constructions must agree on every input: (a) a union-find over the k-mer STRINGS of the node set -- two nodes join
when one is a successor or predecessor of the other --, mapped to unitigs through the k-mers of U.Ref's sequences; (b) a union-find
over the link WORDS of LR.LinkRef, ignoring signs and self links.  CompRef holds comp, the rows and three of the four words (the
rounds are the device's); DropRef the surviving pairs and the nine words.  The file also holds the inputs the GPU tests share (the
disjoint reads, the comb, the mixed table), a numpy model of hook-and-compress with its round bound on the comb, and the constants
of the header against the ctypes binding and the Rust crate."""
import math
import os
import re

import numpy as np
import pytest

import test_clip_ref as CR
import test_gpu_graph as G
import test_gpu_unitig_links as LR
import test_gpu_unitigs as U
from krust_amd import native

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
ALL = U.ALL
MOD = 1 << 64
K = 21


# ---- two union-finds -------------------------------------------------------------------------------------------------------------------
def _find(p, x):
    while p[x] != x:
        p[x] = p[p[x]]
        x = p[x]
    return x


def _union(p, a, b):
    ra, rb = _find(p, a), _find(p, b)
    if ra != rb:
        p[max(ra, rb)] = min(ra, rb)      # the smaller index stays the root: a set's root is its smallest member


def roots_by_links(nu, links):
    """Per unitig the smallest unitig index of its component, from the link words alone."""
    p = list(range(nu))
    for w in links.tolist():
        a, b = w >> 33, (w & 0xFFFFFFFF) >> 1
        if a != b:
            _union(p, a, b)
    return np.array([_find(p, u) for u in range(nu)], dtype=np.int64)


def unitig_kmers(ref):
    k = ref.k
    return [[U.canon(seq[j:j + k]) for j in range(L)] for _, seq, L, _, _ in ref.unitigs]


def roots_by_kmers(ref):
    """The same from the k-mer strings: nodes joined by successor / predecessor, then every unitig through its own k-mers."""
    S, k = ref.S, ref.k
    names = sorted(S)
    idx = {x: i for i, x in enumerate(names)}
    p = list(range(len(names)))
    for x in names:
        for w in (x, U.rc(x)):                       # (the successors of rc(x) are x's predecessors)
            for c in U.LETTERS:
                y = U.canon(w[1:] + c)
                if y in idx and y != x:
                    _union(p, idx[x], idx[y])
    first_of = {}                                    # node component -> the smallest unitig index that holds one of its nodes
    per_unitig = []
    for u, kmers in enumerate(unitig_kmers(ref)):
        rs = {_find(p, idx[x]) for x in kmers}
        assert len(rs) == 1, u                       # a unitig's k-mers follow each other: one component
        r = rs.pop()
        first_of.setdefault(r, u)
        per_unitig.append(r)
    return np.array([first_of[r] for r in per_unitig], dtype=np.int64)


class CompRef:
    """comp (uint32 per unitig), rows ((C, 4) uint64) and words (components, singletons, largest_kmers; the rounds are not the
    reference's) of a U.Ref and its LR.LinkRef.  by_kmers=False skips construction (a) -- for the callers that have checked it."""

    def __init__(self, ref, lref, by_kmers=True):
        nu = ref.rows.shape[0]
        roots = roots_by_links(nu, lref.links)
        if by_kmers:
            other = roots_by_kmers(ref)
            assert np.array_equal(roots, other), np.flatnonzero(roots != other)[:8]
        firsts = np.unique(roots)
        assert (roots <= np.arange(nu)).all() and (roots[firsts] == firsts).all()
        self.roots = roots
        self.comp = np.searchsorted(firsts, roots).astype(np.uint32)
        C = firsts.size
        rows = np.zeros((C, native.COMP_WORDS), dtype=U64)
        sums = [[0, 0, 0] for _ in range(C)]
        for u in range(nu):
            s = sums[int(self.comp[u])]
            s[0] += 1
            s[1] += int(ref.rows[u, native.UNI_KMERS])
            s[2] += int(ref.rows[u, native.UNI_COUNT_SUM])
        for c in range(C):
            rows[c] = [int(firsts[c]), sums[c][0], sums[c][1], sums[c][2] % MOD]
        self.rows = rows
        self.words = [C, int(np.sum(rows[:, native.COMP_UNITIGS] == 1)) if C else 0, int(rows[:, native.COMP_KMERS].max()) if C else 0]
        if nu:
            assert self.comp[0] == 0 and int(np.sum(rows[:, native.COMP_UNITIGS])) == nu


class DropRef:
    """One round of the rule on a U.Ref, its LR.LinkRef and its CompRef: `removed` per unitig, `words` (the nine of
    kh_drop_components_into), the surviving pairs `keys` / `counts` in ascending key order and as the dict `S_next`."""

    def __init__(self, ref, lref, cref, min_kmers):
        nu = ref.rows.shape[0]
        small = cref.rows[:, native.COMP_KMERS] < U64(min(min_kmers, ALL)) if cref.rows.size else np.zeros(0, dtype=bool)
        self.removed = small[cref.comp] if nu else np.zeros(0, dtype=bool)
        self.S_next = {}
        for u, kmers in enumerate(unitig_kmers(ref)):
            if not self.removed[u]:
                for x in kmers:
                    self.S_next[x] = ref.S[x]
        self.keys, self.counts = CR.pairs_of_S(self.S_next, ref.k) if self.S_next else (np.empty(0, dtype=U64), np.empty(0, dtype=U64))
        d = cref.rows[small]
        self.words = [nu, cref.rows.shape[0], int(d.shape[0]), int(np.sum(d[:, native.COMP_KMERS], dtype=U64)) if d.size else 0,
                      sum(int(x) for x in d[:, native.COMP_COUNT_SUM]) % MOD, len(self.S_next), sum(self.S_next.values()) % MOD,
                      int(lref.links.size), int(np.sum(self.removed))]


_COMPS = {}


def comp_of(tag, keys, counts, k, mc, by_kmers=True):
    key = (tag, k, max(mc, 1))
    if key not in _COMPS:
        _COMPS[key] = CompRef(U.ref_of(tag, keys, counts, k, mc), LR.links_of(tag, keys, counts, k, mc), by_kmers)
    return _COMPS[key]


def drop_of(tag, keys, counts, k, mc, min_kmers):
    return DropRef(U.ref_of(tag, keys, counts, k, mc), LR.links_of(tag, keys, counts, k, mc), comp_of(tag, keys, counts, k, mc), min_kmers)


def drop_of_S(S, k, min_kmers):
    ref = U.Ref(S, k)
    lref = LR.LinkRef(ref)
    return ref, DropRef(ref, lref, CompRef(ref, lref), min_kmers)


# ---- the numpy model of hook and compress ----------------------------------------------------------------------------------------------
def hook_and_compress(nu, links):
    """The device's rounds, synchronously: every link word with from < to reads the two labels a compress left, the greater one's
    parent takes the minimum of what is offered to it; then every unitig's parent is chased to its root.  Returns (labels, rounds),
    the last (empty) round included; 0 rounds without links."""
    a, b = (links >> U64(33)).astype(np.int64), ((links & U64(0xFFFFFFFF)) >> U64(1)).astype(np.int64)
    sel = a < b
    a, b = a[sel], b[sel]
    parent = np.arange(nu, dtype=np.int64)
    rounds = 0
    while links.size:
        ra, rb = parent[a], parent[b]
        d = ra != rb
        hi, lo = np.maximum(ra, rb)[d], np.minimum(ra, rb)[d]
        np.minimum.at(parent, hi, lo)                     # (hi is a root, lo < hi: every offer lowers, so "changed" is d.any())
        assert (parent <= np.arange(nu)).all()            # the invariant
        while True:
            nxt = parent[parent]
            if np.array_equal(nxt, parent):
                break
            parent = nxt
        rounds += 1
        if not d.any():
            break
        assert rounds <= nu
    return parent, rounds


def round_bound(nu):
    return 2 * math.ceil(math.log2(nu)) if nu > 1 else 2


# ---- the inputs the GPU tests share ------------------------------------------------------------------------------------------------------
_INPUTS = {}


def _once(key, make):
    if key not in _INPUTS:
        out = make()
        for a in out:
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _INPUTS[key] = out
    return _INPUTS[key]


COUNTS_C = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4097)


def disjoint_input(C, k):
    """C random reads of 2 k bases: k + 1 k-mers each, one unitig and one component per read unless two random k-mers meet --
    the reference counts, the tests assert."""
    def make():
        rng = np.random.default_rng(5000 + 31 * C + k)
        flat = U.flat_of([CR.rand_bases(rng, 2 * k) for _ in range(C)])
        return (flat,) + U.oracle_pairs(flat, k)
    return _once(("disjoint", C, k), make)


COMB_BASES = 270_000     # 3 k to 5 k between two teeth: 84 on average at k = 21, so more than 3000 teeth


def comb_reads(k, seed=11):
    """One random backbone and, every 3 k to 5 k bases, a second read that shares k - 1 + a few bases with it and then diverges
    for k bases: the backbone falls into one chain of unitigs, broken at every tooth, each tooth a tip of k k-mers."""
    rng = np.random.default_rng(seed + k)
    back = CR.rand_bases(rng, COMB_BASES)
    reads = [back]
    p = int(rng.integers(3 * k, 5 * k + 1))
    while p + 2 * k < len(back):
        few = int(rng.integers(1, 6))
        other = [c for c in b"ACGT" if c != back[p]]
        reads.append(back[p - (k - 1) - few:p] + bytes([other[int(rng.integers(0, 3))]]) + CR.rand_bases(rng, k - 1))
        p += int(rng.integers(3 * k, 5 * k + 1))
    return reads


def comb_input(k=K):
    def make():
        flat = U.flat_of(comb_reads(k))
        return (flat,) + U.oracle_pairs(flat, k)
    return _once(("comb", k), make)


WRAP = b"ACGTTGCAAGGCTTAACCGATAG"       # tests/test_gpu_unitigs.py::test_count_sums_wrap_modulo_2_64: three nodes, counts past 2^64
WRAP_COUNTS = (ALL - 1, 5, ALL)
N_DEBRIS = 3000


def mixed_input(k=K):
    """The comb, 3000 isolated reads of 2 k bases, the circles (and chains) of U.cycle_input, the 256 stars of G.star_records --
    one flat buffer to push -- and the three nodes whose counts add up past 2^64, to be merged on top: (flat, wrap keys, wrap
    counts, sorted keys, counts) of the whole table."""
    def make():
        rng = np.random.default_rng(77 + k)
        recs = comb_reads(k) + [CR.rand_bases(rng, 2 * k) for _ in range(N_DEBRIS)] + list(G.star_records(k))
        flat = np.concatenate((U.flat_of(recs), U.cycle_input(k)[0]))
        keys, counts = U.oracle_pairs(flat, k)
        names = [U.canon(WRAP[i:i + k]) for i in range(3)]
        wk = LR.pack_rows(sorted(names), k)
        wc = np.array(WRAP_COUNTS, dtype=U64)
        d = dict(zip(keys.tolist(), (int(c) for c in counts)))
        for x, c in zip(wk.tolist(), WRAP_COUNTS):
            d[x] = (d.get(x, 0) + c) % MOD
        allk = np.array(sorted(d), dtype=U64)
        return flat, wk, wc, allk, np.array([d[x] for x in allk.tolist()], dtype=U64)
    return _once(("mixed", k), make)


# ---- the two constructions agree ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,density", U.SMALL, ids=[f"k{k}-d{d}" for k, d in U.SMALL])
def test_small_k_dense(k, density):
    keys, counts = U.small_case(k, density)
    for mc in (1, 2):
        cr = comp_of(("small", density), keys, counts, k, mc)
        lref = LR.links_of(("small", density), keys, counts, k, mc)
        labels, _ = hook_and_compress(cr.comp.size, lref.links)
        assert np.array_equal(labels, cr.roots)


def test_self_links_join_nothing():
    """Among the small cases are unitigs whose only links are self links (a homopolymer loop, a hairpin, a circle): singletons."""
    lonely = 0
    for k, d in U.SMALL:
        keys, counts = U.small_case(k, d)
        cr, lref = comp_of(("small", d), keys, counts, k, 1), LR.links_of(("small", d), keys, counts, k, 1)
        a, b = lref.links >> U64(33), (lref.links & U64(0xFFFFFFFF)) >> U64(1)
        selfish = set(a[a == b].tolist()) - set(a[a != b].tolist())
        for u in selfish:
            assert int(cr.rows[int(cr.comp[u]), native.COMP_UNITIGS]) == 1
        lonely += len(selfish)
    assert lonely > 0


def test_disjoint_chains_and_cycles():
    flat, keys, counts = U.chain_input(K)
    cr = comp_of("chains", keys, counts, K, 1)
    assert LR.links_of("chains", keys, counts, K, 1).links.size == 0
    assert cr.words[:2] == [len(U.CHAIN_L), len(U.CHAIN_L)] and cr.words[2] == max(U.CHAIN_L)
    assert np.array_equal(cr.comp, np.arange(len(U.CHAIN_L)))
    flat, keys, counts = U.cycle_input(K)
    cr = comp_of("cycles", keys, counts, K, 1)
    assert cr.words[0] == cr.words[1] == 2 * len(U.PERIODS)            # a circle's closing link is a self link


@pytest.mark.parametrize("k", [21, 31])
def test_disjoint_reads_do_not_collide(k):
    for C in COUNTS_C:
        flat, keys, counts = disjoint_input(C, k)
        cr = comp_of(("disjoint", C), keys, counts, k, 1, by_kmers=C <= 257)
        assert cr.words == [C, C, k + 1], (C, cr.words)


def test_the_comb_is_one_chain_and_the_model_stays_under_the_round_bound():
    flat, keys, counts = comb_input()
    ref, lref = U.ref_of("comb", keys, counts, K, 1), LR.links_of("comb", keys, counts, K, 1)
    cr = comp_of("comb", keys, counts, K, 1)
    nu = ref.rows.shape[0]
    teeth = int(np.sum(ref.rows[:, native.UNI_KMERS] == U64(K)))
    assert cr.words[0] == 1 and teeth >= 3000 and nu - teeth >= 3000, (cr.words, nu, teeth)
    labels, rounds = hook_and_compress(nu, lref.links)
    assert (labels == 0).all()
    assert rounds <= round_bound(nu), (rounds, nu)
    # what plain label propagation would need: the chain's diameter, in the thousands
    deg = np.bincount((lref.links >> U64(33)).astype(np.int64), minlength=nu)
    assert int(np.sum(deg >= 3)) >= 3000


def test_the_mixed_table():
    flat, wk, wc, keys, counts = mixed_input()
    cr = comp_of("mixed", keys, counts, K, 1)
    comb = comp_of("comb", comb_input()[1], comb_input()[2], K, 1)
    giant = int(np.argmax(cr.rows[:, native.COMP_KMERS]))
    assert int(cr.rows[giant, native.COMP_KMERS]) == int(comb.rows[0, native.COMP_KMERS])
    assert cr.words[1] >= N_DEBRIS + len(U.PERIODS) and cr.words[0] > cr.words[1]      # lone unitigs, and stars of several
    wrapped = [r for r in cr.rows if int(r[native.COMP_KMERS]) == 3 and int(r[native.COMP_COUNT_SUM]) == (2 * ALL + 4) % MOD]
    assert len(wrapped) == 1
    labels, rounds = hook_and_compress(cr.comp.size, LR.links_of("mixed", keys, counts, K, 1).links)
    assert np.array_equal(labels, cr.roots) and rounds <= round_bound(cr.comp.size)


def test_drop_ref_on_a_fork_and_an_island():
    k = K
    rng = np.random.default_rng(5)
    island = CR.rand_bases(rng, k + 6)                                  # 7 k-mers, alone
    reads = CR.fork_reads(k, 3, 2) + [(island, 4)]
    S = CR.S_of_reads(reads, k)
    ref, d0 = drop_of_S(S, k, 0)
    assert d0.S_next == S and d0.words[2:5] == [0, 0, 0] and d0.words[8] == 0 and d0.words[1] == 2
    _, d1 = drop_of_S(S, k, 1)
    assert d1.words == d0.words
    _, at = drop_of_S(S, k, 7)                                          # exactly its size: it stays (<, not <=)
    assert at.words[2] == 0 and at.S_next == S
    _, above = drop_of_S(S, k, 8)
    assert above.words[2:5] == [1, 7, 28] and above.words[8] == 1 and len(above.S_next) == len(S) - 7
    assert above.words[5] == len(S) - 7 and above.words[0] == 4 and above.words[7] == d0.words[7] > 0
    _, every = drop_of_S(S, k, ALL)
    assert every.S_next == {} and every.words[2] == 2 and every.words[3] == len(S) and every.words[8] == 4
    _, again = drop_of_S(above.S_next, k, 8)                            # idempotent
    assert again.words[2] == 0 and again.S_next == above.S_next


# ---- the constants and the mirrors ------------------------------------------------------------------------------------------------------------
def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


COMP_W = ("FIRST", "UNITIGS", "KMERS", "COUNT_SUM")
CC_W = ("COMPONENTS", "SINGLETONS", "LARGEST_KMERS", "ROUNDS")
DROP_W = ("UNITIGS", "COMPONENTS", "DROPPED", "DROPPED_KMERS", "DROPPED_COUNT", "KEPT_KMERS", "KEPT_COUNT", "LINKS", "DROPPED_UNITIGS")


def test_header_words_agree_with_the_bindings_and_with_clip():
    header = _read("include", "kmerhip.h")
    rust = _read("bindings", "rust", "src", "lib.rs")
    for prefix, words in (("COMP", COMP_W), ("CC", CC_W), ("DROP", DROP_W)):
        n = int(re.search(r"#define\s+KH_%s_WORDS\s+(\d+)" % prefix, header).group(1))
        assert n == len(words) == getattr(native, prefix + "_WORDS")
        assert re.search(r"pub const %s_WORDS: usize = %d;" % (prefix, n), rust)
        for i, w in enumerate(words):
            assert int(re.search(r"#define\s+KH_%s_%s\s+(\d+)" % (prefix, w), header).group(1)) == i == getattr(native, "%s_%s" % (prefix, w))
            assert re.search(r"pub const %s_%s: usize = %d;" % (prefix, w, i), rust)
    assert native.DROP_NAMES == tuple(w.lower() for w in DROP_W) and native.CC_NAMES == tuple(w.lower() for w in CC_W)
    for w in ("UNITIGS", "KEPT_KMERS", "KEPT_COUNT", "LINKS"):         # the words the shared code checks and writes
        assert getattr(native, "DROP_" + w) == getattr(native, "CLIP_" + w) == getattr(native, "POP_" + w)


def test_symbols_declared_mapped_and_bound():
    header = re.sub(r"/\*.*?\*/", "", _read("include", "kmerhip.h"), flags=re.S)
    mapfile, rust, integ = _read("krust_amd", "csrc", "kmerhip.map"), _read("bindings", "rust", "src", "lib.rs"), _read("INTEGRATION.md")
    for name in ("kh_unitigs_components", "kh_unitigs_components_device", "kh_drop_components_into"):
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in mapfile and name in native.SYMBOLS
        assert re.search(r"pub fn %s\(" % name, rust) and re.search(r"\bfn %s\(" % name, integ)
    assert native.SYMBOLS["kh_drop_components_into"] == native.SYMBOLS["kh_clip_tips_into"]
    assert len(native.SYMBOLS["kh_unitigs_components"][1]) == 6 == len(native.SYMBOLS["kh_unitigs_components_device"][1])
    assert re.search(r"#define\s+KMERHIP_ABI_VERSION\s+2\b", header) and native.ABI_VERSION == 2
    for method in ("unitigs_components", "unitigs_components_device", "drop_components_into"):
        assert callable(getattr(native.DeviceCounter, method))
    assert re.search(r"pub fn unitigs_components\(", rust) and re.search(r"pub fn drop_components_into\(", rust)
    comp, unitig = _read("krust_amd", "csrc", "components.hip"), _read("krust_amd", "csrc", "unitig.hip")
    for kernel in ("comp_hook_kernel", "comp_compress_kernel", "comp_sum_kernel", "comp_write_kernel", "comp_drop_kernel"):
        assert re.search(r"\bvoid %s\(" % kernel, comp), kernel
    assert "components.hip" in _read("krust_amd", "csrc", "Makefile")
    assert re.search(r"static_assert\(KH_DROP_KEPT_KMERS == KH_CLIP_KEPT_KMERS && KH_DROP_KEPT_COUNT == KH_CLIP_KEPT_COUNT", unitig)
    assert re.search(r'extern "C" int kh_drop_components_into\(', unitig)


def test_the_library_exports_the_symbols():
    import ctypes as C
    native.lib()
    for so in ("libkmerhip.so", "libkmerhip_testing.so"):
        raw = C.CDLL(os.path.join(os.path.dirname(native.LIB_PATH), so))
        for name in ("kh_unitigs_components", "kh_unitigs_components_device", "kh_drop_components_into"):
            assert hasattr(raw, name), (so, name)
