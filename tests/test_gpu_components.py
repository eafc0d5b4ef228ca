"""kh_unitigs_components* and kh_drop_components_into on the device, against tests/test_components_ref.py.

Expected values never come from the library: comp, the rows and the words are CompRef's (two union-finds that agree), the surviving
pairs and the nine words DropRef's.  Every case runs the host form and the device form; the device form writes between canaries
into pointers that are offset by one element.  The rounds are held to 1 <= rounds <= 2 * ceil(log2(n_unitigs)) where there are
links (the model of the ref file stays under it on the same inputs) and to 0 where there are none.

Run with `pytest -m gpu` on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_clip_ref as CR
import test_components_ref as R
import test_gpu_graph as G
import test_gpu_join as T
import test_gpu_pop as P
import test_gpu_unitig_links as LR
import test_gpu_unitigs as U
import test_pop_ref as PR
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "components_child.py")
U64 = np.uint64
ALL = U.ALL
K = R.K
HINT = 3_000_000
CANARY32, CANARY64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A


def cc_dict(cref, rounds):
    return dict(zip(native.CC_NAMES, list(cref.words) + [rounds]))


def device_form(dc, nu, C, comp_cap=None, row_cap=None):
    """kh_unitigs_components_device into arrays with one canary element in front and behind: (status, stats, comp, rows)."""
    import torch
    comp_cap = nu if comp_cap is None else comp_cap
    row_cap = C if row_cap is None else row_cap
    tc = torch.full((comp_cap + 2,), CANARY32, dtype=torch.int32, device="cuda")
    trw = torch.full((native.COMP_WORDS * row_cap + 2,), CANARY64, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    rc, st = dc.unitigs_components_device(tc.data_ptr() + 4 if comp_cap else None, comp_cap, trw.data_ptr() + 8 if row_cap else None, row_cap)
    hc, hr = tc.cpu().numpy().view(np.uint32), trw.cpu().numpy().view(U64)
    assert hc[0] == hc[-1] == CANARY32 and hr[0] == hr[-1] == CANARY64
    return rc, st, hc[1:-1], hr[1:-1].reshape(-1, native.COMP_WORDS)


def check_live(dc, ref, cref, nl):
    """Both forms on the live linked unitigs of dc against the reference; returns the rounds."""
    nu, C = ref.rows.shape[0], cref.rows.shape[0]
    comp, rows, st = dc.unitigs_components()
    rounds = st["rounds"]
    assert st == cc_dict(cref, rounds), (st, cref.words)
    assert (rounds == 0) if nl == 0 else (1 <= rounds <= R.round_bound(nu)), (rounds, nu, nl)
    assert comp.dtype == np.uint32 and comp.shape == cref.comp.shape and rows.shape == cref.rows.shape
    bad = np.flatnonzero(comp != cref.comp)
    assert bad.size == 0, (bad[:8], comp[bad[:8]], cref.comp[bad[:8]])
    assert np.array_equal(rows, cref.rows), np.argwhere(rows != cref.rows)[:4]
    rc, st2, dcomp, drows = device_form(dc, nu, C)
    assert rc == native.KH_OK and st2 == st
    assert np.array_equal(dcomp, cref.comp) and np.array_equal(drows, cref.rows)
    return rounds


def check_components(dc, tag, keys, counts, k, mc, by_kmers=True):
    ref, lref = U.ref_of(tag, keys, counts, k, mc), LR.links_of(tag, keys, counts, k, mc)
    cref = R.comp_of(tag, keys, counts, k, mc, by_kmers)
    nu, nb, nl = dc.unitigs_begin_linked(mc)
    try:
        assert (nu, nl) == (ref.rows.shape[0], lref.links.size)
        return check_live(dc, ref, cref, nl), cref
    finally:
        dc.unitigs_end()


# ---- dense small k, empty, minimal ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,density", U.SMALL, ids=[f"k{k}-d{d}" for k, d in U.SMALL])
def test_small_k_dense(k, density):
    keys, counts = U.small_case(k, density)
    with native.DeviceCounter(k) as dc:
        dc.merge_pairs(keys, counts)
        for mc in (1, 2):
            check_components(dc, ("small", density), keys, counts, k, mc)


def test_empty_and_single():
    k = K
    rng = np.random.default_rng(1)
    flat = U.flat_of([CR.rand_bases(rng, k + 3)])
    keys, counts = U.oracle_pairs(flat, k)
    with native.DeviceCounter(k) as dc:
        dc.push(flat)
        assert dc.unitigs_begin_linked(ALL) == (0, 0, 0)                          # an empty S
        comp, rows, st = dc.unitigs_components()
        assert comp.size == 0 and rows.size == 0 and st == dict(zip(native.CC_NAMES, [0, 0, 0, 0]))
        rc, st, _, _ = device_form(dc, 0, 0, comp_cap=3, row_cap=2)               # (nothing is written into arrays that are there)
        assert rc == native.KH_OK and st["components"] == 0
        dc.unitigs_end()
        rounds, cref = check_components(dc, "single", keys, counts, k, 1)
        assert rounds == 0 and cref.words == [1, 1, 4]


def test_disjoint_chains_have_no_links_and_no_rounds():
    flat, keys, counts = U.chain_input(K)
    with native.DeviceCounter(K, capacity_hint=100_000) as dc:
        dc.push(flat)
        rounds, cref = check_components(dc, "chains", keys, counts, K, 1)
        assert rounds == 0 and np.array_equal(cref.comp, np.arange(len(U.CHAIN_L)))


@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("C", R.COUNTS_C)
def test_component_counts_across_the_scans_and_a_waves_edges(C, k):
    flat, keys, counts = R.disjoint_input(C, k)
    with native.DeviceCounter(k, capacity_hint=400_000) as dc:
        dc.push(flat)
        rounds, cref = check_components(dc, ("disjoint", C), keys, counts, k, 1, by_kmers=C <= 257)
        assert cref.words == [C, C, k + 1] and rounds == 0


# ---- the comb and the mixed table -----------------------------------------------------------------------------------------------------------
def test_the_comb():
    flat, keys, counts = R.comb_input()
    with native.DeviceCounter(K, capacity_hint=HINT) as dc:
        dc.push(flat)
        rounds, cref = check_components(dc, "comb", keys, counts, K, 1)
        nu = cref.comp.size
        print(f"comb: {nu} unitigs, rounds {rounds}, bound {R.round_bound(nu)}")
        assert cref.words[0] == 1 and nu >= 6000 and 2 <= rounds <= R.round_bound(nu)


def mixed_table():
    flat, wk, wc, keys, counts = R.mixed_input()
    dc = native.DeviceCounter(K, capacity_hint=HINT)
    dc.push(flat)
    dc.merge_pairs(wk, wc)
    return dc, keys, counts


def test_the_mixed_table():
    dc, keys, counts = mixed_table()
    with dc:
        rounds, cref = check_components(dc, "mixed", keys, counts, K, 1)
        assert cref.words[1] >= R.N_DEBRIS and rounds >= 2
        assert ((2 * ALL + 4) % (1 << 64)) in cref.rows[:, native.COMP_COUNT_SUM].tolist()


# ---- table forms, grid stride, the product library ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", U.FORMS)
def test_table_forms(form, monkeypatch):
    k = K
    flat, keys, counts = G.main_input(k)
    if form in ("wide", "image", "regions3072", "grown"):
        dc = T.table(form, k, flat, monkeypatch)
    else:
        if form == "narrow0":
            monkeypatch.setenv("KMERHIP_NARROW", "0")
        if form == "pow2":
            monkeypatch.setenv("KMERHIP_POW2_TABLE", "1")
        dc = native.DeviceCounter(k, capacity_hint=1 if form == "hint1" else HINT, path="partition" if form == "narrow0" else None)
        dc.push(flat)
        dc.finish()
    with dc:
        before = T.stats_of(dc)
        for mc in (1, 2):
            check_components(dc, "main", keys, counts, k, mc, by_kmers=False)      # the same reference bytes for every form
        assert T.stats_of(dc) == before


def planted_case(k=K, mc=1):
    """Components and one drop on tests/test_gpu_pop.py's planted input (the children run it)."""
    flat, keys, counts = P.planted(k)
    with native.DeviceCounter(k, capacity_hint=HINT) as src, native.DeviceCounter(k, capacity_hint=HINT) as dst:
        src.push(flat)
        rounds, cref = check_components(src, "planted", keys, counts, k, mc)
        assert cref.comp.size > 768 and rounds >= 1                                    # (more than three workgroups' unitigs)
        check_drop(src, "planted", keys, counts, k, mc, int(cref.rows[:, native.COMP_KMERS].max()), dst)
    return cref


def disjoint_case(C=1025, k=K):
    flat, keys, counts = R.disjoint_input(C, k)
    with native.DeviceCounter(k, capacity_hint=400_000) as dc:
        dc.push(flat)
        check_components(dc, ("disjoint", C), keys, counts, k, 1, by_kmers=False)


_CHILD_DIED = []


def run_child(env, timeout=300):
    assert not _CHILD_DIED, f"not started: an earlier child ended on a signal or at its timeout ({_CHILD_DIED[0]})"
    try:
        p = subprocess.run([sys.executable, CHILD], capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append("timeout")
        raise
    if p.returncode < 0:
        _CHILD_DIED.append(f"signal {-p.returncode}")
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


def test_product_library_once():
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    env.pop("KMERHIP_GRID_CAP", None)
    assert "libkmerhip.so" in run_child(env)


@pytest.mark.parametrize("cap", [1, 3])
def test_past_the_first_grid_stride(cap):
    """KMERHIP_GRID_CAP (test build) = 1 and 3, one value per process: more unitigs and more links than cap workgroups hold, so
    every kernel of the build and the decide kernel go round their loops again."""
    env = dict(os.environ, KMERHIP_GRID_CAP=str(cap))
    assert env.get("KMERHIP_LIB") == "libkmerhip_testing.so"
    out = run_child(env)
    assert f"cap {cap}" in out and "libkmerhip_testing.so" in out


# ---- the contract -------------------------------------------------------------------------------------------------------------------------------
def test_caps_null_arrays_and_misalignment():
    import torch
    flat, keys, counts = R.disjoint_input(65, K)
    cref = R.comp_of(("disjoint", 65), keys, counts, K, 1)
    L = native.lib()
    with native.DeviceCounter(K, capacity_hint=100_000) as dc:
        dc.push(flat)
        nu, nb, nl = dc.unitigs_begin_linked(1)
        C = cref.rows.shape[0]
        assert (nu, C) == (65, 65)
        out = np.full(native.CC_WORDS, 7, dtype=U64)
        assert L.kh_unitigs_components(dc._h, None, 0, None, 0, out.ctypes.data) == native.KH_OK              # NULL arrays: sizing
        assert out.tolist() == cref.words + [0]
        for comp_cap, row_cap in ((nu - 1, C), (nu, C - 1), (1, 0), (0, 1)):                                   # too small: nothing written
            rc, st, dcomp, drows = device_form(dc, nu, C, comp_cap=comp_cap, row_cap=row_cap)
            assert rc == native.KH_ERR_RANGE and st == cc_dict(cref, 0), (comp_cap, row_cap, rc, st)
            assert (dcomp == CANARY32).all() and (drows == U64(CANARY64)).all()
            comp = np.full(max(comp_cap, 1), CANARY32, dtype=np.uint32)
            rows = np.full((max(row_cap, 1), 4), CANARY64, dtype=U64)
            out[:] = 7
            assert L.kh_unitigs_components(dc._h, comp.ctypes.data if comp_cap else None, comp_cap, rows.ctypes.data if row_cap else None, row_cap,
                                           out.ctypes.data) == native.KH_ERR_RANGE
            assert out.tolist() == cref.words + [0] and (comp == CANARY32).all() and (rows == U64(CANARY64)).all()
        for comp_cap, row_cap in ((nu + 3, C + 2), (nu, 0), (0, C)):                                            # room to spare; one array only
            rc, st, dcomp, drows = device_form(dc, nu, C, comp_cap=comp_cap, row_cap=row_cap)
            assert rc == native.KH_OK
            if comp_cap:
                assert np.array_equal(dcomp[:nu], cref.comp) and (dcomp[nu:] == CANARY32).all()
            if row_cap:
                assert np.array_equal(drows[:C], cref.rows) and (drows[C:] == U64(CANARY64)).all()
        comp = np.full(nu + 2, CANARY32, dtype=np.uint32)
        rows = np.full((C + 2, 4), CANARY64, dtype=U64)
        assert L.kh_unitigs_components(dc._h, comp.ctypes.data, nu + 2, rows.ctypes.data, C + 2, out.ctypes.data) == native.KH_OK
        assert np.array_equal(comp[:nu], cref.comp) and (comp[nu:] == CANARY32).all()
        assert np.array_equal(rows[:C], cref.rows) and (rows[C:] == U64(CANARY64)).all()
        # arguments
        t = torch.zeros(4 * C + 8, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        for fn in (L.kh_unitigs_components, L.kh_unitigs_components_device):
            assert fn(dc._h, None, 0, None, 0, None) == native.KH_ERR_BAD_ARG                                   # out is required
            assert fn(dc._h, None, nu, None, 0, out.ctypes.data) == native.KH_ERR_BAD_ARG                       # NULL with a cap
            assert fn(dc._h, None, 0, None, C, out.ctypes.data) == native.KH_ERR_BAD_ARG
            assert fn(None, None, 0, None, 0, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert L.kh_unitigs_components_device(dc._h, t.data_ptr() + 2, nu, None, 0, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert b"4-byte aligned" in L.kh_last_error(dc._h)
        assert L.kh_unitigs_components_device(dc._h, None, 0, t.data_ptr() + 4, C, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert b"8-byte aligned" in L.kh_last_error(dc._h)
        assert L.kh_unitigs_components(dc._h, None, 0, None, 0, out.ctypes.data + 4) == native.KH_ERR_BAD_ARG
        assert (t == 0).all().item()
        check_live(dc, U.ref_of(("disjoint", 65), keys, counts, K, 1), cref, nl)                               # still usable
        dc.unitigs_end()


def test_state_errors():
    flat, keys, counts = R.disjoint_input(2, K)
    L = native.lib()
    out = np.full(native.CC_WORDS, 7, dtype=U64)
    with native.DeviceCounter(K) as dc:
        dc.push(flat)
        for fn in (L.kh_unitigs_components, L.kh_unitigs_components_device):
            assert fn(dc._h, None, 0, None, 0, out.ctypes.data) == native.KH_ERR_STATE                          # before any begin
            assert b"kh_unitigs_begin_linked" in L.kh_last_error(dc._h)
            dc.unitigs_begin(1)
            assert fn(dc._h, None, 0, None, 0, out.ctypes.data) == native.KH_ERR_STATE                          # a plain begin built no links
            assert b"kh_unitigs_begin_linked, not kh_unitigs_begin" in L.kh_last_error(dc._h)
            dc.unitigs_begin_linked(1)
            assert fn(dc._h, None, 0, None, 0, out.ctypes.data) == native.KH_OK and out[0] == 2
            dc.unitigs_end()
            out[:] = 7
            assert fn(dc._h, None, 0, None, 0, out.ctypes.data) == native.KH_ERR_STATE                          # after kh_unitigs_end
            assert (out == U64(7)).all()
        dc.unitigs_begin_linked(1)
        dc.push(flat)                                                                                            # a writer makes them stale
        assert L.kh_unitigs_components(dc._h, None, 0, None, 0, out.ctypes.data) == native.KH_ERR_STATE


def test_readers_interleave_and_nothing_else_changes():
    """Components between locate, paths, link support and the pieces of a running text stream: all of them give what they give
    without it, and the table's statistics stay."""
    k = K
    flat, keys, counts = P.planted(k)
    ref, lref = U.ref_of("planted", keys, counts, k, 1), LR.links_of("planted", keys, counts, k, 1)
    cref = R.comp_of("planted", keys, counts, k, 1)
    reads = np.asarray(flat[:4000]).copy()
    rs = np.array([0, reads.size], dtype=U64)

    def others(dc):
        loc = dc.unitigs_locate(reads)
        run_start, runs = dc.unitigs_paths(reads, rs)
        sup, sst = dc.unitigs_link_support(run_start, runs)
        return loc, run_start, runs, sup, sst

    with native.DeviceCounter(k, capacity_hint=HINT) as a, native.DeviceCounter(k, capacity_hint=HINT) as b:
        a.push(flat)
        b.push(flat)
        before = T.stats_of(a)
        a.unitigs_begin_linked(1)
        want = others(a)
        text = a.unitigs_text("gfa", piece_bytes=1 << 14)
        a.unitigs_end()
        nu, nb, nl = b.unitigs_begin_linked(1)
        total = b.unitigs_text_begin("gfa")
        buf = np.empty(1 << 14, dtype=np.uint8)
        got_text = bytearray()
        n = b.unitigs_text_next(buf)
        got_text += buf[:n].tobytes()
        rounds = check_live(b, ref, cref, nl)                                     # builds the labels inside the stream
        got = others(b)
        check_live(b, ref, cref, nl)
        while True:
            n = b.unitigs_text_next(buf)
            if n == 0:
                break
            got_text += buf[:n].tobytes()
            comp, rows, st = b.unitigs_components()
            assert st["rounds"] == rounds and np.array_equal(comp, cref.comp)
        assert len(got_text) == total and bytes(got_text) == text
        for g, w in zip(got, want):
            assert (g == w) if isinstance(w, dict) else np.array_equal(g, w)
        assert np.array_equal(b.unitigs_links_copy(nl), lref.links)
        b.unitigs_end()
        assert T.stats_of(b) == before


# ---- kh_drop_components_into --------------------------------------------------------------------------------------------------------------------
def words_dict(dr):
    return dict(zip(native.DROP_NAMES, dr.words))


def check_drop(src, tag, keys, counts, k, mc, min_kmers, dst, dr=None):
    """One call into an EMPTY dst: its table against the reference's surviving pairs, the nine words, and src unchanged."""
    dr = dr or R.drop_of(tag, keys, counts, k, mc, min_kmers)
    before, s0 = T.stats_of(src), src.result_sorted(1)
    got = dst.drop_components_into(src, mc, min_kmers)
    assert got == words_dict(dr), (k, mc, min_kmers, got, words_dict(dr))
    gk, gc = dst.result_sorted(1)
    assert gk.dtype == U64 and gk.shape == dr.keys.shape, (k, mc, min_kmers, gk.shape, dr.keys.shape)
    assert np.array_equal(gk, dr.keys) and np.array_equal(gc, dr.counts), (k, mc, min_kmers)
    st = dst.finish()
    assert st["distinct"] == dr.keys.size and st["kmers"] == dr.words[native.DROP_KEPT_COUNT]
    s1 = src.result_sorted(1)
    assert T.stats_of(src) == before and np.array_equal(s0[0], s1[0]) and np.array_equal(s0[1], s1[1])
    return dr


def test_drop_bounds_on_the_mixed_table():
    """0 and 1 drop nothing; k + 1 is exactly the size of an isolated read's component and keeps it, k + 2 drops the 3000 of them;
    the giant's size keeps the giant alone, one more (and 2^64 - 1) drops everything and leaves a prefilled dst as it was."""
    src, keys, counts = mixed_table()
    cref = R.comp_of("mixed", keys, counts, K, 1)
    giant = int(cref.rows[:, native.COMP_KMERS].max())
    with src, native.DeviceCounter(K, capacity_hint=HINT) as dst:
        for bound in (0, 1):
            dr = check_drop(src, "mixed", keys, counts, K, 1, bound, dst)
            assert dr.words[native.DROP_DROPPED] == 0 and np.array_equal(dr.keys, keys) and np.array_equal(dr.counts, counts)
            dst.reset()
        at = check_drop(src, "mixed", keys, counts, K, 1, K + 1, dst)
        dst.reset()
        above = check_drop(src, "mixed", keys, counts, K, 1, K + 2, dst)
        assert above.words[native.DROP_DROPPED] - at.words[native.DROP_DROPPED] >= R.N_DEBRIS                     # the < of the rule
        dst.reset()
        only = check_drop(src, "mixed", keys, counts, K, 1, giant, dst)
        assert only.words[native.DROP_DROPPED] == cref.rows.shape[0] - 1 and only.words[native.DROP_KEPT_KMERS] == giant
        dst.reset()
        for bound in (giant + 1, ALL):
            dst.merge_pairs(keys[:3], np.full(3, 7, dtype=U64))
            dr = R.drop_of("mixed", keys, counts, K, 1, bound)
            assert dr.keys.size == 0 and dr.words[native.DROP_DROPPED] == cref.rows.shape[0]
            assert dst.drop_components_into(src, 1, bound) == words_dict(dr)
            gk, gc = dst.result_sorted(1)
            assert np.array_equal(gk, keys[:3]) and gc.tolist() == [7, 7, 7]
            dst.reset()


def test_drop_min_count_two_and_a_prefilled_dst():
    k = K
    flat, keys, counts = P.planted(k)
    cref2 = R.comp_of("planted", keys, counts, k, 2)
    sizes = np.sort(cref2.rows[:, native.COMP_KMERS])
    bound = int(sizes[-1])                                                         # keeps the largest component only
    with native.DeviceCounter(k, capacity_hint=HINT) as src, native.DeviceCounter(k) as dst:
        src.push(flat)
        dr = check_drop(src, "planted", keys, counts, k, 2, bound, dst)
        assert 0 < dr.words[native.DROP_DROPPED] == cref2.rows.shape[0] - int(np.sum(sizes == sizes[-1]))
        dst.reset()
        gone = np.setdiff1d(keys, dr.keys)
        mine_k = np.concatenate([dr.keys[:2], gone[:1]])                           # three keys: two that survive, one that does not
        dst.merge_pairs(mine_k, np.array([7, 8, 9], dtype=U64))
        want = dict(zip(dr.keys.tolist(), dr.counts.tolist()))
        for x, c in zip(mine_k.tolist(), (7, 8, 9)):
            want[x] = want.get(x, 0) + c
        assert dst.drop_components_into(src, 2, bound) == words_dict(dr)
        gk, gc = dst.result_sorted(1)
        assert gk.size == dr.keys.size + 1 and dict(zip(gk.tolist(), gc.tolist())) == want


@pytest.mark.parametrize("form", ["image", "regions3072"])
def test_drop_table_forms_of_src(form, monkeypatch):
    k = K
    flat, keys, counts = P.planted(k)
    cref = R.comp_of("planted", keys, counts, k, 1)
    bound = int(cref.rows[:, native.COMP_KMERS].max())
    src = T.table(form, k, np.asarray(flat), monkeypatch)
    with src, native.DeviceCounter(k, capacity_hint=HINT) as dst:
        check_drop(src, "planted", keys, counts, k, 1, bound, dst)


def test_drop_refusals_leave_both_contexts_usable():
    k = K
    S = CR.S_of_reads(PR.snp(k, 3, 2), k)
    keys, counts = CR.pairs_of_S(S, k)
    _, dr = R.drop_of_S(S, k, 2 * k)
    L = native.lib()
    zeros = dict(zip(native.DROP_NAMES, [0] * 9))
    out = np.full(native.DROP_WORDS, 7, dtype=U64)
    with native.DeviceCounter(k) as src, native.DeviceCounter(k) as dst, native.DeviceCounter(k + 1) as other, native.DeviceCounter(k) as sh:
        assert dst.drop_components_into(src, 1, k) == zeros                                                      # an empty src: KH_OK, all words 0
        src.merge_pairs(keys, counts)
        assert L.kh_drop_components_into(dst._h, dst._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert b"kh_drop_components_into: dst must not be src" in L.kh_last_error(dst._h)
        assert L.kh_drop_components_into(dst._h, None, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert L.kh_drop_components_into(dst._h, src._h, 1, k, None) == native.KH_ERR_BAD_ARG
        assert L.kh_drop_components_into(None, src._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        assert L.kh_drop_components_into(other._h, src._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG and b"different k" in L.kh_last_error(other._h)
        assert L.kh_drop_components_into(dst._h, other._h, 1, k, out.ctypes.data) == native.KH_ERR_BAD_ARG
        sh.set_shard(0, 2)
        mine = keys[np.array([native.owner(int(x), k, 2) == 0 for x in keys])]
        sh.merge_pairs(mine, np.ones(mine.size, dtype=U64))
        assert L.kh_drop_components_into(dst._h, sh._h, 1, k, out.ctypes.data) == native.KH_ERR_STATE            # a shard as src
        assert L.kh_drop_components_into(sh._h, src._h, 1, k, out.ctypes.data) == native.KH_ERR_STATE            # ... and as dst
        assert (out == U64(7)).all()
        assert sh.finish()["distinct"] == mine.size and other.finish()["distinct"] == 0 and dst.finish()["distinct"] == 0
        check_drop(src, "snp32-drop", keys, counts, k, 1, 2 * k, dst, dr=dr)                                     # all of them usable
        assert np.array_equal(src.lookup(keys), counts)
        dst.reset()
        assert dst.drop_components_into(src, ALL, 2 * k) == zeros                                                # an empty S
        assert dst.finish()["distinct"] == 0
        nu, nb, nl = src.unitigs_begin_linked(1)                                                                 # begun unitigs are released
        dst.reset()
        assert dst.drop_components_into(src) == words_dict(dr)                                                   # the defaults: 1 and 2 k
        assert L.kh_unitigs_links_copy(src._h, None, 0) == native.KH_ERR_STATE


def test_clip_pop_and_drop_rounds_end_in_a_graph_without_debris():
    """Two contexts ping-pong: a clip round, a pop round and a drop round in turn with kh_reset between, against ClipRef, PopRef
    and DropRef chained the same way, until a round of each in a row changed nothing.  A further drop at the same bound then drops
    nothing."""
    k = K
    bound = 4 * k
    flat, keys, counts = P.planted(k)
    S = U.node_dict(keys, counts, k, 1)
    a, b = native.DeviceCounter(k, capacity_hint=HINT), native.DeviceCounter(k, capacity_hint=HINT)
    with a, b:
        a.push(flat)
        rounds, quiet = 0, 0
        while quiet < 3:
            which = ("clip", "pop", "drop")[rounds % 3]
            if which == "clip":
                _, ref = CR.clip_of_S(S, k, k)
                got, want, n = b.clip_tips_into(a, 1, k), dict(zip(native.CLIP_NAMES, ref.words)), ref.words[native.CLIP_CLIPPED]
            elif which == "pop":
                _, ref = PR.pop_of_S(S, k, 2 * k)
                got, want, n = b.pop_bubbles_into(a, 1, 2 * k), dict(zip(native.POP_NAMES, ref.words)), ref.words[native.POP_POPPED]
            else:
                _, ref = R.drop_of_S(S, k, bound)
                got, want, n = b.drop_components_into(a, 1, bound), words_dict(ref), ref.words[native.DROP_DROPPED]
            assert got == want, (rounds, which, got, want)
            gk, gc = b.result_sorted(1)
            assert np.array_equal(gk, ref.keys) and np.array_equal(gc, ref.counts), (rounds, which)
            S = ref.S_next
            quiet = quiet + 1 if n == 0 else 0
            rounds += 1
            a.reset()
            a, b = b, a
            assert rounds <= 15, rounds
        _, last = R.drop_of_S(S, k, bound)
        got = b.drop_components_into(a, 1, bound)
        assert got == words_dict(last) and got["dropped"] == 0 and got["kept_kmers"] == len(S)
