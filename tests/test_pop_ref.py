"""The rule of kh_pop_bubbles_into (include/kmerhip.h, "bubble popping") in Python strings, and that rule on hand-built graphs.  No device.

PopRef is built from the string references of the unitigs (test_gpu_unitigs.Ref) and of their links (test_gpu_unitig_links.LinkRef),
as test_clip_ref.ClipRef is: the sorted link words regrouped by from-state, the candidate test, the exit pairs, the classes of
parallel candidates -- with every member asserted to be among the unitigs that enter a member's + exit, which is where the device
looks for them --, the comparison in Python integers, and the surviving pairs.  tests/test_gpu_pop.py holds the device to it."""
import numpy as np
import pytest

import test_clip_ref as CR
import test_gpu_unitig_links as LR
import test_gpu_unitigs as U

U64 = np.uint64
ALL = (1 << 64) - 1
KS = (11, 21, 32)


def beats(kmers_b, sum_b, idx_b, kmers_i, sum_i, idx_i):
    """Whether parallel candidate b beats candidate i (b != i): the comparator of the rule, the products as Python integers."""
    pb, pi = sum_b * kmers_i, sum_i * kmers_b
    if pb != pi:
        return pb > pi
    if kmers_b != kmers_i:
        return kmers_b > kmers_i
    return idx_b < idx_i


def decided_by(kmers_b, sum_b, kmers_i, sum_i):
    return "mean" if sum_b * kmers_i != sum_i * kmers_b else "kmers" if kmers_b != kmers_i else "index"


class PopRef:
    """One round of the rule on a U.Ref and its LR.LinkRef: `exits` (the sorted pair of to-states, or None) and `popped` per unitig,
    `classes` (exit pair -> the candidates that have it, ascending), `words` (the nine of kh_pop_bubbles_into), the surviving pairs
    `keys` / `counts` in ascending key order and as the dict `S_next`, and what the decisions met on their way: `by` (what decided
    each ordered pair of parallel candidates), `largest` (the largest class), `alone` (candidates without a parallel) and
    `self_blocked` (unitigs that pass every candidate test but the last: a link goes to the unitig itself)."""

    def __init__(self, ref, lref, max_kmers):
        k, nu = ref.k, len(ref.unitigs)
        out = {}
        for w in lref.links.tolist():                       # from-state -> to-states
            out.setdefault(w >> 32, []).append(w & 0xFFFFFFFF)
        kmers = [u[2] for u in ref.unitigs]
        sums = [u[3] % (1 << 64) for u in ref.unitigs]
        self.exits = exits = [None] * nu
        self.self_blocked = 0
        self.classes = classes = {}
        for i in range(nu):
            op, om = out.get(2 * i, []), out.get(2 * i + 1, [])
            if ref.unitigs[i][4] or kmers[i] > max_kmers or len(op) != 1 or len(om) != 1:
                continue
            if op[0] >> 1 == i or om[0] >> 1 == i:
                self.self_blocked += 1
                continue
            exits[i] = (min(op[0], om[0]), max(op[0], om[0]))
            classes.setdefault(exits[i], []).append(i)
        self.by = {"mean": 0, "kmers": 0, "index": 0}
        self.popped = popped = [False] * nu
        self.largest = max([len(m) for m in classes.values()], default=0)
        self.alone = sum(1 for m in classes.values() if len(m) == 1)
        assert self.largest <= 4
        for members in classes.values():
            for i in members:
                entering = [b >> 1 for b in out.get(out[2 * i][0] ^ 1, [])]     # where the device finds i's parallels, and i
                assert all(b in entering for b in members), (i, members, entering)
                for b in members:
                    if b != i:
                        self.by[decided_by(kmers[b], sums[b], kmers[i], sums[i])] += 1
                        popped[i] = popped[i] or beats(kmers[b], sums[b], b, kmers[i], sums[i], i)
            assert sum(1 for i in members if not popped[i]) == 1, members          # exactly one member of every class survives
        self.S_next = {}
        for i, (_, seq, L, _, _) in enumerate(ref.unitigs):
            if not popped[i]:
                for p in range(L):
                    x = U.canon(seq[p:p + k])
                    self.S_next[x] = ref.S[x]
        assert len(self.S_next) == sum(kmers[i] for i in range(nu) if not popped[i])
        names = sorted(self.S_next)
        self.keys = LR.pack_rows(names, k)
        self.counts = np.array([self.S_next[x] % (1 << 64) for x in names], dtype=U64)
        assert (self.keys[1:] > self.keys[:-1]).all()
        po = [i for i in range(nu) if popped[i]]
        self.words = [nu, sum(1 for e in exits if e is not None), len(po), sum(kmers[i] for i in po), sum(sums[i] for i in po) % (1 << 64),
                      len(names), sum(self.S_next.values()) % (1 << 64), int(lref.links.size),
                      sum(1 for m in classes.values() if len(m) >= 2)]
        assert self.words[3] + self.words[5] == len(ref.S)
        assert self.words[2] == self.words[1] - len(classes)


def pop_of_S(S, k, max_kmers):
    ref = U.Ref(S, k)
    return ref, PopRef(ref, LR.LinkRef(ref), max_kmers)


# ---- hand-built graphs --------------------------------------------------------------------------------------------------------------
def bubble_reads(k, alleles, seed=12):
    """Haplotypes left(150) + letter [+ inserted bases] + right(150) as (sequence, count) reads: `alleles` is a list of
    (letter, inserted bases, count).  The k-mers that hold the letter (or an inserted base) are the allele's branch: one unitig of
    k + len(inserted) k-mers between the unitig of the left flank and that of the right one.  (The seed is one whose flanks are
    plain chains at k = 11 too -- no k-mer beside its own reverse complement; the tests assert the unitig counts.)"""
    rng = np.random.default_rng(seed + k)
    left, right = CR.rand_bases(rng, 150), CR.rand_bases(rng, 150)
    return [(left + letter + ins + right, c) for letter, ins, c in alleles]


def branch_of(ref, read, k, ins=0):
    """The unitig of an allele's branch: the one that holds the k-mer which starts at the allele's letter."""
    x = U.canon(read[150:150 + k])
    hits = [i for i, u in enumerate(ref.unitigs) if any(U.canon(u[1][p:p + k]) == x for p in range(u[2]))]
    assert len(hits) == 1 and ref.unitigs[hits[0]][2] == k + ins, (hits, ins)
    return hits[0]


def snp(k, c1, c2):
    return bubble_reads(k, [(b"A", b"", c1), (b"C", b"", c2)])


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("c1,c2,loser", [(3, 2, 1), (2, 3, 0), (2, 2, None)])
def test_snp_loses_the_weaker_branch(k, c1, c2, loser):
    reads = snp(k, c1, c2)
    ref, pr = pop_of_S(CR.S_of_reads(reads, k), k, 2 * k)
    b = [branch_of(ref, r[0], k) for r in reads]
    flank = 150 - k + 1
    assert len(ref.unitigs) == 4 and sorted(u[2] for u in ref.unitigs) == sorted([k, k, flank, flank])
    assert pr.exits[b[0]] is not None and pr.exits[b[0]] == pr.exits[b[1]] and sum(1 for e in pr.exits if e is not None) == 2
    lost = b[loser] if loser is not None else max(b)              # equal mean and KMERS: the greater index goes
    assert [i for i, p in enumerate(pr.popped) if p] == [lost]
    assert pr.by == {"mean": 2 if loser is not None else 0, "kmers": 0, "index": 0 if loser is not None else 2}
    assert pr.largest == 2 and pr.alone == 0 and pr.self_blocked == 0
    assert pr.words == [4, 2, 1, k, k * min(c1, c2), 2 * flank + k, 2 * flank * (c1 + c2) + k * max(c1, c2), 8, 1]
    assert U.canon(reads[0 if lost == b[1] else 1][0][150:150 + k]) in pr.S_next
    assert U.canon(reads[1 if lost == b[1] else 0][0][150:150 + k]) not in pr.S_next


@pytest.mark.parametrize("k", KS)
def test_insertion_with_equal_counts_is_decided_by_kmers(k):
    reads = bubble_reads(k, [(b"A", b"", 3), (b"C", b"GTC", 3)])
    ref, pr = pop_of_S(CR.S_of_reads(reads, k), k, 2 * k)
    short, long_ = branch_of(ref, reads[0][0], k), branch_of(ref, reads[1][0], k, 3)
    assert pr.exits[short] == pr.exits[long_] is not None
    assert pr.popped[short] and not pr.popped[long_] and sum(pr.popped) == 1      # equal mean counts: the one of more k-mers stays
    assert pr.by == {"mean": 0, "kmers": 2, "index": 0} and pr.words[1:5] == [2, 1, k, 3 * k] and pr.words[8] == 1


@pytest.mark.parametrize("k", KS)
def test_three_alleles_leave_one(k):
    reads = bubble_reads(k, [(b"A", b"", 4), (b"C", b"", 3), (b"G", b"", 2)])
    ref, pr = pop_of_S(CR.S_of_reads(reads, k), k, 2 * k)
    b = [branch_of(ref, r[0], k) for r in reads]
    assert len(ref.unitigs) == 5 and pr.largest == 3 and list(pr.classes.values()) == [sorted(b)]
    assert [pr.popped[i] for i in b] == [False, True, True]
    assert pr.words[1:5] == [3, 2, 2 * k, 5 * k] and pr.words[8] == 1 and pr.by == {"mean": 6, "kmers": 0, "index": 0}


@pytest.mark.parametrize("k", KS)
def test_the_bound_is_inclusive(k):
    S = CR.S_of_reads(snp(k, 3, 2), k)
    _, below = pop_of_S(S, k, k - 1)
    assert below.words[1:5] == [0, 0, 0, 0] and below.words[8] == 0 and below.S_next == S
    _, at = pop_of_S(S, k, k)
    assert at.words[1:3] == [2, 1] and at.words[8] == 1
    _, zero = pop_of_S(S, k, 0)
    assert zero.words[:5] == [4, 0, 0, 0, 0] and zero.S_next == S               # max_kmers == 0 copies S


@pytest.mark.parametrize("k", KS)
def test_a_long_branch_beside_a_short_one_keeps_both(k):
    reads = bubble_reads(k, [(b"A", b"", 1), (b"C", b"G", 9)])                  # the insertion makes the strong branch k + 1 k-mers
    ref, pr = pop_of_S(CR.S_of_reads(reads, k), k, k)
    short = branch_of(ref, reads[0][0], k)
    assert pr.exits[short] is not None and pr.words[1:3] == [1, 0] and pr.words[8] == 0 and pr.alone == 1
    assert pr.S_next == ref.S
    _, wide = pop_of_S(ref.S, k, k + 1)                                          # with room for both, the weak short one goes
    assert wide.words[1:3] == [2, 1] and wide.popped[short] and wide.by["mean"] == 2


@pytest.mark.parametrize("k", [21, 32])
def test_tips_and_forks_are_no_bubbles(k):
    """The forks and tips of tests/test_clip_ref.py: dead ends have a side without a link, so nothing is a candidate that has a
    parallel, at any bound."""
    for reads in (CR.fork_reads(k, 3, 2), CR.fork_reads(k, 2, 2), CR.fork_reads(k, 9, 1, len1=10, len2=60), CR.fork_reads(k, 1, 9, len1=12, len2=8)):
        S = CR.S_of_reads(reads, k)
        for mk in (k, 2 * k, ALL):
            _, pr = pop_of_S(S, k, mk)
            assert pr.words[1:5] == [0, 0, 0, 0] and pr.words[8] == 0 and pr.S_next == S


def test_isolated_pieces_and_circles_are_never_candidates():
    rng = np.random.default_rng(3)
    unit = CR.rand_bases(rng, 30)
    reads = [(CR.rand_bases(rng, 25), 1), ((unit * 3)[:30 + 21 - 1], 2)]
    for mk in (1, 21, ALL):
        ref, pr = pop_of_S(CR.S_of_reads(reads, 21), 21, mk)
        assert sum(u[4] for u in ref.unitigs) == 1 and pr.words == [2, 0, 0, 0, 0, 35, 65, 2, 0] and pr.S_next == ref.S


def test_dense_small_k_pops_nothing_and_holds_self_blocked_unitigs():
    """From the reference alone: the dense small-k cases (palindromes, loops, hairpins) hold no class of two at any bound, and
    somewhere a unitig that passes every candidate test but the last."""
    blocked = 0
    for k, d in U.SMALL:
        keys, counts = U.small_case(k, d)
        S = U.node_dict(keys, counts, k, 1)
        for mk in (1, 3, ALL):
            _, pr = pop_of_S(S, k, mk)
            blocked += pr.self_blocked
            assert pr.words[2:5] == [0, 0, 0] and pr.words[8] == 0 and pr.S_next == S, (k, d, mk, pr.words)
    assert blocked >= 1, blocked


def test_the_comparator_handles_wrapped_sums_and_products_past_64_bits():
    big = (1 << 64) - 1
    assert beats(3, big, 1, 3, big - 1, 0) and not beats(3, big - 1, 0, 3, big, 1)
    assert beats(1 << 31, big, 5, (1 << 31) - 1, big, 4) is False                # equal sums: the mean of the shorter one is greater
    assert beats(2, 6, 9, 1, 3, 0) and not beats(1, 3, 0, 2, 6, 9)               # equal means: more k-mers
    assert beats(2, 6, 0, 2, 6, 1) and not beats(2, 6, 1, 2, 6, 0)               # a full tie: the smaller index
