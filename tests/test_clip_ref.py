"""The rule of kh_clip_tips_into (include/kmerhip.h, "tip clipping") in Python strings, and that rule on hand-built graphs.  No device.

ClipRef is built from the string references of the unitigs (test_gpu_unitigs.Ref) and of their links (test_gpu_unitig_links.LinkRef):
the sorted link words regrouped by from-state, the candidate test, the rivals of every link of a candidate's attached end -- with
`i in rivals` asserted for each --, the comparison, and the surviving pairs.  tests/test_gpu_clip.py holds the device to it."""
import numpy as np
import pytest

import test_gpu_unitig_links as LR
import test_gpu_unitigs as U

U64 = np.uint64
ALL = (1 << 64) - 1
K = 21


def beats(kmers_b, sum_b, idx_b, cand_b, kmers_i, sum_i, idx_i):
    """Whether rival b beats candidate i (b != i): the comparator of the rule."""
    return (not cand_b) or (kmers_b, sum_b, -idx_b) > (kmers_i, sum_i, -idx_i)


class ClipRef:
    """One round of the rule on a U.Ref and its LR.LinkRef: `cand` (0 / 1 = attached at + / 2 = attached at -) and `clipped` per
    unitig, `words` (the eight of kh_clip_tips_into), the surviving pairs `keys` / `counts` in ascending key order and as the dict
    `S_next`, and what the decisions met on their way (`by`, `multi`, `self_blocked`)."""

    def __init__(self, ref, lref, max_kmers):
        k, nu = ref.k, len(ref.unitigs)
        out = {}
        for w in lref.links.tolist():                       # from-state -> to-states
            out.setdefault(w >> 32, []).append(w & 0xFFFFFFFF)
        kmers = [u[2] for u in ref.unitigs]
        sums = [u[3] % (1 << 64) for u in ref.unitigs]
        self.cand = cand = [0] * nu
        self.self_blocked = 0
        for i in range(nu):
            op, om = out.get(2 * i, []), out.get(2 * i + 1, [])
            if ref.unitigs[i][4] or kmers[i] > max_kmers or bool(op) == bool(om):
                continue
            s = 0 if op else 1
            if any(t >> 1 == i for t in out[2 * i + s]):
                self.self_blocked += 1                      # a dead end whose attached end links to its own unitig
                continue
            cand[i] = 1 + s
        self.by = {"kmers": 0, "sum": 0, "index": 0, "non_candidate": 0}
        self.multi = 0
        self.clipped = clipped = [False] * nu
        for i in range(nu):
            if not cand[i]:
                continue
            ls = out[2 * i + cand[i] - 1]
            assert 1 <= len(ls) <= 4
            self.multi += len(ls) > 1
            every = True
            for t in ls:
                rivals = [b >> 1 for b in out.get(t ^ 1, [])]
                assert i in rivals, (i, t, rivals)
                beaten = False
                for b in rivals:
                    if b == i:
                        continue
                    if cand[b]:
                        self.by["kmers" if kmers[b] != kmers[i] else "sum" if sums[b] != sums[i] else "index"] += 1
                    else:
                        self.by["non_candidate"] += 1
                    beaten = beaten or beats(kmers[b], sums[b], b, bool(cand[b]), kmers[i], sums[i], i)
                every = every and beaten
            clipped[i] = every
        self.S_next = {}
        for i, (_, seq, L, _, _) in enumerate(ref.unitigs):
            if not clipped[i]:
                for p in range(L):
                    x = U.canon(seq[p:p + k])
                    self.S_next[x] = ref.S[x]
        assert len(self.S_next) == sum(kmers[i] for i in range(nu) if not clipped[i])
        names = sorted(self.S_next)
        self.keys = LR.pack_rows(names, k)
        self.counts = np.array([self.S_next[x] for x in names], dtype=U64)
        assert (self.keys[1:] > self.keys[:-1]).all()
        cl = [i for i in range(nu) if clipped[i]]
        self.words = [nu, sum(1 for c in cand if c), len(cl), sum(kmers[i] for i in cl), sum(sums[i] for i in cl) % (1 << 64),
                      len(names), sum(self.S_next.values()) % (1 << 64), int(lref.links.size)]
        assert self.words[3] + self.words[5] == len(ref.S)


def clip_of_S(S, k, max_kmers):
    ref = U.Ref(S, k)
    return ref, ClipRef(ref, LR.LinkRef(ref), max_kmers)


# ---- hand-built graphs --------------------------------------------------------------------------------------------------------------
def rand_bases(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].tobytes()


def S_of_reads(reads, k):
    """(sequence, count) reads -> the node set as a dict from canonical strings to counts."""
    S = {}
    for seq, c in reads:
        for p in range(len(seq) - k + 1):
            x = U.canon(seq[p:p + k])
            S[x] = S.get(x, 0) + c
    return S


def pairs_of_S(S, k):
    names = sorted(S)
    return LR.pack_rows(names, k), np.array([S[x] for x in names], dtype=U64)


def fork_reads(k, c1, c2, len1=11, len2=11, seed=7):
    """A 200-base stem with count 5 and two branches off its end: stem[-(k-1):] + a letter + len - 1 further bases each, so a
    branch is a unitig of len k-mers (11: a letter and 10 random bases)."""
    rng = np.random.default_rng(seed + k)
    stem = rand_bases(rng, 200)
    return [(stem, 5), (stem[-(k - 1):] + b"A" + rand_bases(rng, len1 - 1), c1), (stem[-(k - 1):] + b"C" + rand_bases(rng, len2 - 1), c2)]


def unitig_of(ref, seq):
    """The index of the unitig that spells seq or its reverse complement."""
    hits = [i for i, u in enumerate(ref.unitigs) if u[1] in (seq, U.rc(seq))]
    assert len(hits) == 1, (seq, len(hits))
    return hits[0]


def branches(ref, reads, k):
    """The unitigs of the branch reads: a branch is one unitig, its whole read."""
    return [unitig_of(ref, r[0]) for r in reads[1:]]


@pytest.mark.parametrize("k", [21, 32])
@pytest.mark.parametrize("c1,c2,loser", [(3, 2, 1), (2, 3, 0), (2, 2, None)])
def test_fork_loses_the_weaker_branch(k, c1, c2, loser):
    reads = fork_reads(k, c1, c2)
    ref, cr = clip_of_S(S_of_reads(reads, k), k, k)
    b = branches(ref, reads, k)
    stem = [i for i in range(len(ref.unitigs)) if i not in b]
    ns = 200 - k + 1
    assert len(ref.unitigs) == 3 and [ref.unitigs[i][2] for i in b] == [11, 11] and ref.unitigs[stem[0]][2] == ns
    assert cr.cand[b[0]] and cr.cand[b[1]] and not cr.cand[stem[0]]
    lost = b[loser] if loser is not None else max(b)             # equal (KMERS, COUNT_SUM): the larger index goes
    assert [i for i, c in enumerate(cr.clipped) if c] == [lost]
    assert cr.by["sum" if loser is not None else "index"] == 2 and cr.by["kmers"] == 0
    assert cr.words == [3, 2, 1, 11, 11 * min(c1, c2), ns + 11, 5 * ns + 11 * max(c1, c2), 4]
    # every bound that still holds the stem keeps it: its attached end meets no rival but itself
    _, big = clip_of_S(S_of_reads(reads, k), k, ALL)
    assert sum(1 for c in big.cand if c) == 3 and big.clipped == cr.clipped


def test_tip_beside_a_long_branch_is_lost():
    reads = fork_reads(K, 9, 1, len1=10, len2=60)                 # the short one has the HIGHER count: only candidates compare counts
    ref, cr = clip_of_S(S_of_reads(reads, K), K, K)
    short, long_ = branches(ref, reads, K)
    assert (ref.unitigs[short][2], ref.unitigs[long_][2]) == (10, 60)
    assert cr.cand[short] and not cr.cand[long_] and cr.clipped[short] and sum(cr.clipped) == 1
    assert cr.by == {"kmers": 0, "sum": 0, "index": 0, "non_candidate": 1}
    assert U.canon(reads[1][0][-K:]) not in cr.S_next and U.canon(reads[2][0][-K:]) in cr.S_next


@pytest.mark.parametrize("length,is_cand", [(K, True), (K + 1, False)])
def test_the_bound_is_inclusive(length, is_cand):
    reads = fork_reads(K, 1, 1, len1=length, len2=60)
    ref, cr = clip_of_S(S_of_reads(reads, K), K, K)
    tip = branches(ref, reads, K)[0]
    assert ref.unitigs[tip][2] == length and bool(cr.cand[tip]) == is_cand and cr.clipped[tip] == is_cand
    assert cr.words[1] == cr.words[2] == int(is_cand)


def test_two_branch_lengths_decide_by_kmers():
    reads = fork_reads(K, 1, 9, len1=12, len2=8)                  # the shorter one has the higher count, and loses
    ref, cr = clip_of_S(S_of_reads(reads, K), K, K)
    b = branches(ref, reads, K)
    assert cr.cand[b[0]] and cr.cand[b[1]] and cr.clipped[b[1]] and not cr.clipped[b[0]] and cr.by["kmers"] == 2


def test_isolated_pieces_and_circles_are_never_candidates():
    rng = np.random.default_rng(3)
    unit = rand_bases(rng, 30)
    reads = [(rand_bases(rng, K + 4), 1), ((unit * 3)[:30 + K - 1], 2)]
    for mk in (1, K, ALL):
        ref, cr = clip_of_S(S_of_reads(reads, K), K, mk)
        assert sorted(u[2] for u in ref.unitigs) == [5, 30] and sum(u[4] for u in ref.unitigs) == 1
        assert cr.cand == [0, 0] and cr.clipped == [False, False] and cr.words == [2, 0, 0, 0, 0, 35, 65, 2]
        assert cr.S_next == ref.S


def test_max_kmers_zero_copies_S():
    reads = fork_reads(K, 3, 2)
    ref, cr = clip_of_S(S_of_reads(reads, K), K, 0)
    assert cr.words[:5] == [3, 0, 0, 0, 0] and cr.S_next == ref.S


def test_dense_small_k_holds_a_dead_end_that_links_to_itself():
    """From the reference alone: among the dense small-k cases is a unitig that passes every candidate test but the last -- its
    attached end links to its own unitig -- and the prototype's candidate and clipped numbers at max_kmers 3."""
    blocked = 0
    table = {}
    for k, d in U.SMALL:
        keys, counts = U.small_case(k, d)
        _, cr = clip_of_S(U.node_dict(keys, counts, k, 1), k, 3)
        blocked += cr.self_blocked
        table[(k, d)] = (cr.words[1], cr.words[2])
    assert blocked >= 1, blocked
    want = {(4, 0.5): (9, 7), (5, 0.1): (12, 6), (5, 0.5): (32, 29), (4, "chosen"): (1, 0)}
    assert table == {c: want.get(c, (0, 0)) for c in U.SMALL}, table
