"""kh_clip_tips_into -- one round of tip clipping of a count table's compacted graph into another context -- against the rule in
Python strings (tests/test_clip_ref.py).

Expected values never come from the library: the unitigs and links are those of the string references of tests/test_gpu_unitigs.py
and tests/test_gpu_unitig_links.py (the same inputs under the same tags, so those walks run once per session), the decision and the
surviving pairs are ClipRef's.  The target table is compared word for word, the eight statistics words exactly."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_clip_ref as R
import test_gpu_graph as G
import test_gpu_join as T
import test_gpu_unitig_links as LR
import test_gpu_unitigs as U
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "clip_child.py")
U64 = np.uint64
ALL = U.ALL
_CLIPS = {}


def clip_of(tag, keys, counts, k, mc, max_kmers):
    key = (tag, k, max(mc, 1), max_kmers)
    if key not in _CLIPS:
        _CLIPS[key] = R.ClipRef(U.ref_of(tag, keys, counts, k, mc), LR.links_of(tag, keys, counts, k, mc), max_kmers)
    return _CLIPS[key]


def words_dict(cr):
    return dict(zip(native.CLIP_NAMES, cr.words))


def check_clip(src, tag, keys, counts, k, mc, max_kmers, dst, cr=None):
    """One call into an EMPTY dst: its table against the reference's surviving pairs, the eight words, and src unchanged."""
    cr = cr or clip_of(tag, keys, counts, k, mc, max_kmers)
    before, s0 = T.stats_of(src), src.result_sorted(1)
    got = dst.clip_tips_into(src, mc, max_kmers)
    assert got == words_dict(cr), (k, mc, max_kmers, got, words_dict(cr))
    gk, gc = dst.result_sorted(1)
    assert gk.dtype == U64 and gk.shape == cr.keys.shape, (k, mc, max_kmers, gk.shape, cr.keys.shape)
    assert np.array_equal(gk, cr.keys) and np.array_equal(gc, cr.counts), (k, mc, max_kmers)
    st = dst.finish()
    assert st["distinct"] == cr.keys.size and st["kmers"] == cr.words[native.CLIP_KEPT_COUNT]
    s1 = src.result_sorted(1)
    assert T.stats_of(src) == before and np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
    return cr


# ---- hand-built graphs: every kind of decision ----------------------------------------------------------------------------------------
def built_cases(k):
    """(name, node set, max_kmers): the forks and tips of tests/test_clip_ref.py."""
    out = [(f"fork{c1}{c2}", R.S_of_reads(R.fork_reads(k, c1, c2), k), k) for c1, c2 in ((3, 2), (2, 3), (2, 2))]
    out.append(("tip-long", R.S_of_reads(R.fork_reads(k, 9, 1, len1=10, len2=60), k), k))
    out.append(("bound", R.S_of_reads(R.fork_reads(k, 1, 1, len1=k, len2=60), k), k))
    out.append(("bound+1", R.S_of_reads(R.fork_reads(k, 1, 1, len1=k + 1, len2=60), k), k))
    out.append(("lengths", R.S_of_reads(R.fork_reads(k, 1, 9, len1=12, len2=8), k), k))
    out.append(("stem-too", R.S_of_reads(R.fork_reads(k, 3, 2), k), ALL))      # the stem is a candidate with two links out
    return out


def test_the_inputs_hold_every_kind_of_decision():
    """Precondition, from the reference alone: clipped unitigs, candidates that stay, candidate-against-candidate decisions by
    KMERS, by COUNT_SUM and by index, and a candidate with more than one link out of its attached end."""
    by = {"kmers": 0, "sum": 0, "index": 0, "non_candidate": 0}
    clipped = kept = multi = 0
    for _, S, mk in built_cases(21):
        _, cr = R.clip_of_S(S, 21, mk)
        for name in by:
            by[name] += cr.by[name]
        clipped += cr.words[native.CLIP_CLIPPED]
        kept += cr.words[native.CLIP_CANDIDATES] - cr.words[native.CLIP_CLIPPED]
        multi += cr.multi
    assert all(v > 0 for v in by.values()) and clipped > 0 and kept > 0 and multi > 0, (by, clipped, kept, multi)
    flat, keys, counts = G.main_input(11)                               # ... and all of them at size
    cr = clip_of("main", keys, counts, 11, 1, 11)
    assert all(v > 0 for v in cr.by.values()) and cr.multi > 0, (cr.by, cr.multi)


@pytest.mark.parametrize("k", [21, 32])
def test_forks_and_tips(k):
    with native.DeviceCounter(k) as src, native.DeviceCounter(k) as dst:
        for name, S, mk in built_cases(k):
            keys, counts = R.pairs_of_S(S, k)
            src.reset()
            dst.reset()
            src.merge_pairs(keys, counts)
            ref, cr = R.clip_of_S(S, k, mk)
            check_clip(src, name, keys, counts, k, 1, mk, dst, cr=cr)


# ---- dense small k -------------------------------------------------------------------------------------------------------------------
PROTOTYPE3 = {(4, 0.5): (9, 7), (5, 0.1): (12, 6), (5, 0.5): (32, 29), (4, "chosen"): (1, 0)}


@pytest.mark.parametrize("k,density", U.SMALL, ids=[f"k{k}-d{d}" for k, d in U.SMALL])
def test_small_k_dense(k, density):
    keys, counts = U.small_case(k, density)
    with native.DeviceCounter(k) as src, native.DeviceCounter(k) as dst:
        src.merge_pairs(keys, counts)
        for mk in (1, 3, ALL):
            dst.reset()
            cr = check_clip(src, ("small", density), keys, counts, k, 1, mk, dst)
            if mk == 3:
                assert (cr.words[1], cr.words[2]) == PROTOTYPE3.get((k, density), (0, 0))
            if cr.words[native.CLIP_CANDIDATES] == 0:                     # nothing is a candidate: dst equals S
                gk, gc = dst.result_sorted(1)
                assert np.array_equal(gk, keys) and np.array_equal(gc, counts)


# ---- branching, realistic ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mc", [1, 2])
@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_branching_reads_and_stars(k, mc):
    flat, keys, counts = G.main_input(k)
    refs = {mk: clip_of("main", keys, counts, k, mc, mk) for mk in (1, k, 2 * k)}
    for mk, cr in refs.items():                                         # from the reference, before the device is touched
        assert cr.words[native.CLIP_CANDIDATES] > cr.words[native.CLIP_CLIPPED] > 0, (k, mc, mk, cr.words)
    if (k, mc) == (11, 1):
        assert refs[11].words[:4] == [78992, 2732, 2544, 6817]
    if (k, mc) == (21, 2):
        assert [(c.words[1], c.words[2]) for c in refs.values()] == [(604, 360), (668, 360), (668, 360)]
    with native.DeviceCounter(k, capacity_hint=3_000_000) as src, native.DeviceCounter(k, capacity_hint=3_000_000) as dst:
        src.push(flat)
        for mk in refs:
            dst.reset()
            check_clip(src, "main", keys, counts, k, mc, mk, dst)


def test_rounds_until_nothing_is_clipped():
    """Two contexts ping-pong, kh_reset between rounds, against the reference iterated the same way; then the unitigs of the
    final table."""
    k = 21
    flat, keys, counts = G.main_input(k)
    S = U.node_dict(keys, counts, k, 1)
    a, b = native.DeviceCounter(k, capacity_hint=3_000_000), native.DeviceCounter(k, capacity_hint=3_000_000)
    with a, b:
        a.push(flat)
        rounds = 0
        while True:
            ref, cr = R.clip_of_S(S, k, k)
            got = b.clip_tips_into(a, 1, k)
            rounds += 1
            assert got == words_dict(cr), (rounds, got, cr.words)
            gk, gc = b.result_sorted(1)
            assert np.array_equal(gk, cr.keys) and np.array_equal(gc, cr.counts), rounds
            S = cr.S_next
            a.reset()
            a, b = b, a
            if got["clipped"] == 0:
                break
            assert rounds < 6, rounds
        assert 2 <= rounds <= 6
        fk, fc = R.pairs_of_S(S, k)
        U.check_unitigs(a, "clipped-final", fk, fc, k, 1, ref=U.Ref(S, k))


# ---- table forms of src: identical pairs and words ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", U.FORMS)
def test_table_forms_of_src(form, monkeypatch):
    k, mc = 21, 2
    flat, keys, counts = G.main_input(k)
    if form in ("wide", "image", "regions3072", "grown"):
        src = T.table(form, k, flat, monkeypatch)
    else:
        if form == "narrow0":
            monkeypatch.setenv("KMERHIP_NARROW", "0")
        if form == "pow2":
            monkeypatch.setenv("KMERHIP_POW2_TABLE", "1")
        src = native.DeviceCounter(k, capacity_hint=1 if form == "hint1" else 3_000_000, path="partition" if form == "narrow0" else None)
        src.push(flat)
        src.finish()
    monkeypatch.delenv("KMERHIP_NARROW", raising=False)
    monkeypatch.delenv("KMERHIP_POW2_TABLE", raising=False)
    with src, native.DeviceCounter(k, capacity_hint=3_000_000) as dst:
        check_clip(src, "main", keys, counts, k, mc, k, dst)


# ---- dst: it grows, it is hinted, it already holds pairs ------------------------------------------------------------------------------
def test_dst_variants(monkeypatch):
    k, mc = 21, 1
    flat, keys, counts = G.main_input(k)
    cr = clip_of("main", keys, counts, k, mc, k)
    with native.DeviceCounter(k, capacity_hint=3_000_000) as src:
        src.push(flat)
        monkeypatch.setenv("KMERHIP_TABLE_REGIONS", "64")               # a first table of 64 regions: the survivors do not fit it
        small = native.DeviceCounter(k)
        monkeypatch.delenv("KMERHIP_TABLE_REGIONS", raising=False)
        assert cr.keys.size > 64 * 4096 * 0.7
        with small:
            check_clip(src, "main", keys, counts, k, mc, k, small)
            assert small.finish()["grows"] >= 1
        with native.DeviceCounter(k, capacity_hint=cr.keys.size) as hinted:
            check_clip(src, "main", keys, counts, k, mc, k, hinted)
            assert hinted.finish()["grows"] == 0
        # 1000 chosen pairs, half of them survivors: the counts add
        gone = np.setdiff1d(keys, cr.keys)
        assert gone.size >= 500
        rng = np.random.default_rng(9)
        mine_k = np.concatenate([rng.choice(cr.keys, 500, replace=False), rng.choice(gone, 500, replace=False)])
        mine_c = (np.arange(1000) + 7).astype(U64)
        want = dict(zip(cr.keys.tolist(), cr.counts.tolist()))
        for x, c in zip(mine_k.tolist(), mine_c.tolist()):
            want[x] = want.get(x, 0) + c
        with native.DeviceCounter(k, capacity_hint=3_000_000) as held:
            held.merge_pairs(mine_k, mine_c)
            assert held.clip_tips_into(src, mc, k) == words_dict(cr)
            gk, gc = held.result_sorted(1)
            assert gk.size == cr.keys.size + 500 and dict(zip(gk.tolist(), gc.tolist())) == want


# ---- the contract ----------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_both_contexts_usable():
    k = 21
    reads = R.fork_reads(k, 3, 2)
    S = R.S_of_reads(reads, k)
    keys, counts = R.pairs_of_S(S, k)
    _, cr = R.clip_of_S(S, k, k)
    _, cr0 = R.clip_of_S(S, k, 0)
    L = native.lib()
    out = np.full(native.CLIP_WORDS, 7, dtype=U64)
    with native.DeviceCounter(k) as src, native.DeviceCounter(k) as dst, native.DeviceCounter(k + 1) as other, native.DeviceCounter(k) as sh:
        assert dst.clip_tips_into(src, 1, k) == dict(zip(native.CLIP_NAMES, [0] * 8))        # an empty src: KH_OK, all words 0
        assert dst.finish()["distinct"] == 0
        src.merge_pairs(keys, counts)
        assert L.kh_clip_tips_into(dst._h, dst._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG and b"dst must not be src" in L.kh_last_error(dst._h)
        assert L.kh_clip_tips_into(dst._h, None, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert L.kh_clip_tips_into(dst._h, src._h, 1, k, None) == native.KH_ERR_BAD_ARG
        assert L.kh_clip_tips_into(None, src._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert L.kh_clip_tips_into(other._h, src._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG and b"different k" in L.kh_last_error(other._h)
        assert L.kh_clip_tips_into(dst._h, other._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        sh.set_shard(0, 2)
        mine = keys[np.array([native.owner(int(x), k, 2) == 0 for x in keys])]
        sh.merge_pairs(mine, np.ones(mine.size, dtype=U64))
        assert L.kh_clip_tips_into(dst._h, sh._h, 1, k, out.ctypes.data) == native.KH_ERR_STATE                   # a shard as src
        assert L.kh_clip_tips_into(sh._h, src._h, 1, k, out.ctypes.data) == native.KH_ERR_STATE                   # ... and as dst
        assert (out == U64(7)).all()                                                                              # nothing was written
        assert sh.finish()["distinct"] == mine.size and other.finish()["distinct"] == 0 and dst.finish()["distinct"] == 0
        # unitigs src had begun are released by the call; the readers may follow
        nu, nb, nl = src.unitigs_begin_linked(1)
        assert nu == 3
        check_clip(src, "fork32", keys, counts, k, 1, k, dst, cr=cr)
        rows = np.zeros((nu, 4), dtype=U64)
        bases = np.zeros(nb, dtype=np.uint8)
        assert L.kh_unitigs_copy(src._h, rows.ctypes.data, nu, bases.ctypes.data, nb) == native.KH_ERR_STATE
        assert L.kh_unitigs_links_copy(src._h, None, 0) == native.KH_ERR_STATE
        assert np.array_equal(src.lookup(keys), counts)
        assert int(src.graph_stats(1)[native.GRAPH_NODES]) == keys.size
        assert src.unitigs_begin_linked(1) == (nu, nb, nl)                                                        # and a begin works again
        src.unitigs_end()
        dst.reset()
        check_clip(src, "fork32", keys, counts, k, 1, 0, dst, cr=cr0)                                             # max_kmers = 0 copies S
        gk, gc = dst.result_sorted(1)
        assert np.array_equal(gk, keys) and np.array_equal(gc, counts)
        dst.reset()
        assert dst.clip_tips_into(src, ALL, k) == dict(zip(native.CLIP_NAMES, [0] * 8))                           # an empty S
        assert dst.clip_tips_into(src) == words_dict(cr)                                                          # the defaults: 1 and k


def test_a_pending_push_is_counted_first():
    k = 21
    flat, keys, counts = G.main_input(k)
    cr = clip_of("main", keys, counts, k, 1, k)
    with native.DeviceCounter(k, capacity_hint=3_000_000) as src, native.DeviceCounter(k, capacity_hint=3_000_000) as dst:
        src.push(flat)
        assert dst.clip_tips_into(src, 1, k) == words_dict(cr)


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


def case_file(tmp_path, k):
    flat, keys, counts = G.main_input(k)
    cr = clip_of("main", keys, counts, k, 1, k)
    path = tmp_path / f"clip{k}.npz"
    np.savez(path, k=k, mc=1, max_kmers=k, hint=3_000_000, flat=flat, keys=cr.keys, counts=cr.counts, words=np.array(cr.words, dtype=U64))
    return path, cr


def test_product_library_once(tmp_path):
    """The same pairs and words on the library as it ships (no test switches)."""
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    env.pop("KMERHIP_GRID_CAP", None)
    path, cr = case_file(tmp_path, 21)
    out = run_child(path, env, 300)
    assert "libkmerhip.so" in out and f"clipped {cr.words[native.CLIP_CLIPPED]}" in out, out


@pytest.mark.parametrize("cap", [1, 3])
def test_past_the_first_grid_stride(tmp_path, cap):
    """KMERHIP_GRID_CAP (test build) = 1 and 3, one value per process: the two decision kernels run over the unitigs, the keep
    kernel over the nodes, which are more -- at cap 1 one workgroup goes round each loop at least three times."""
    path, cr = case_file(tmp_path, 11)
    blocks = -(-cr.words[native.CLIP_UNITIGS] // 256)
    assert cr.words[native.CLIP_UNITIGS] >= 3 * 256 * 3 and -(-blocks // min(cap, blocks)) >= 3, blocks
    env = dict(os.environ, KMERHIP_GRID_CAP=str(cap))
    assert env.get("KMERHIP_LIB") == "libkmerhip_testing.so"
    out = run_child(path, env, 300)
    assert f"cap {cap}" in out and "libkmerhip_testing.so" in out and f"clipped {cr.words[native.CLIP_CLIPPED]}" in out, out
