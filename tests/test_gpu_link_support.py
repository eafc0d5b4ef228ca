"""kh_unitigs_link_support* -- how many reads walk every link of the live unitigs -- against link_support_ref of
tests/test_link_support_ref.py: a plain loop over the rows and a dict of the link words kh_unitigs_links_copy returns.

Every case runs the device form and the host form on the same inputs and compares the counters and all four statistics exactly, with
canaries on both sides of the counters.  The rows are the reference's (paths_ref over locate_ref: tests/test_gpu_paths.py holds the
device's rows to the same), or hand-made where a case needs rows no read gives.

Run with `pytest -m gpu` on an MI355X."""
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_join as TJ
import test_gpu_locate as L
import test_gpu_unitigs as U
import test_link_support_ref as S
from krust_amd import native
from test_gpu_paths import Walks, check_links, per_read, random_cuts

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "link_support_child.py")
U64, U32 = np.uint64, np.uint32
CANARY = 0xABABABABABABABAB
OK, STATE, BAD_ARG, RANGE = native.KH_OK, native.KH_ERR_STATE, native.KH_ERR_BAD_ARG, native.KH_ERR_RANGE
RW, SW = native.RUN_WORDS, native.SUP_WORDS
PAIRS, ADJACENT, CREDITED, MISSING = native.SUP_PAIRS, native.SUP_ADJACENT, native.SUP_CREDITED, native.SUP_MISSING
T = 1024      # rows per tile of link_support_kernel: kh::SUP_TILE of krust_amd/csrc/support.hip (tests/test_link_support_ref.py compares)
PADW = 4      # canary words on either side of the counters


class Got:
    def __init__(self, rc, support, stats):
        self.rc, self.support, self.stats = rc, support, stats


def _rows32(rows):
    return np.ascontiguousarray(rows, dtype=U32).reshape(-1, RW)


def _counters(nl, support0):
    buf = np.full(nl + 2 * PADW, CANARY, dtype=U64)
    buf[PADW:PADW + nl] = 0 if support0 is None else np.asarray(support0, dtype=U64)
    return buf


def _checked(buf, nl, who):
    assert (buf[:PADW] == U64(CANARY)).all() and (buf[PADW + nl:] == U64(CANARY)).all(), who + " wrote outside support"
    return buf[PADW:PADW + nl].copy()


def support_device(dc, run_start, rows, nl, support0=None, roff=0, cap=None):
    """kh_unitigs_link_support_device with d_runs 4 * roff bytes behind a 16-byte boundary; cap None: n_links."""
    import torch
    rs, rows = np.ascontiguousarray(run_start, dtype=U64), _rows32(rows)
    hr = np.zeros(rows.size + 8, dtype=U32)
    hr[4 + roff:4 + roff + rows.size] = rows.reshape(-1)
    t_rs, t_rows = torch.from_numpy(rs.view(np.int64)).cuda(), torch.from_numpy(hr.view(np.int32)).cuda()
    buf = _counters(nl, support0)
    t_sup = torch.from_numpy(buf.view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert t_rows.data_ptr() % 16 == 0
    out = np.full(SW, CANARY, dtype=U64)
    rc = native.lib().kh_unitigs_link_support_device(dc._h, t_rs.data_ptr(), rs.size - 1, t_rows.data_ptr() + 16 + 4 * roff, rows.shape[0],
                                                     t_sup.data_ptr() + 8 * PADW, nl if cap is None else cap, out.ctypes.data)
    return Got(rc, _checked(t_sup.cpu().numpy().view(U64), nl, "kh_unitigs_link_support_device"), out)


def support_host(dc, run_start, rows, nl, support0=None, cap=None):
    rs, rows = np.ascontiguousarray(run_start, dtype=U64), _rows32(rows)
    buf = _counters(nl, support0)
    out = np.full(SW, CANARY, dtype=U64)
    rc = native.lib().kh_unitigs_link_support(dc._h, rs.ctypes.data, rs.size - 1, rows.ctypes.data, rows.shape[0], buf[PADW:].ctypes.data,
                                              nl if cap is None else cap, out.ctypes.data)
    return Got(rc, _checked(buf, nl, "kh_unitigs_link_support"), out)


def both(dc, run_start, rows, links, support0=None, **kw):
    """The device form and the host form against the reference; returns the reference's (support, stats)."""
    want = S.link_support_ref(run_start, rows, links, support0)
    for call, extra in ((support_device, kw), (support_host, {})):
        got = call(dc, run_start, rows, links.size, support0, **extra)
        assert got.rc == OK, (call.__name__, got.rc, native.lib().kh_last_error(dc._h))
        assert np.array_equal(got.stats, want[1]), (call.__name__, got.stats.tolist(), want[1].tolist())
        if not np.array_equal(got.support, want[0]):
            i = int(np.flatnonzero(got.support != want[0])[0])
            raise AssertionError("%s: %d of %d counters differ, first %d (link %#x): %d for %d" %
                                 (call.__name__, int(np.sum(got.support != want[0])), links.size, i, int(links[i]), int(got.support[i]), int(want[0][i])))
    return want


def ref_rows(w, flat, rs):
    """(run_start, rows) of the reference for the records rs of flat on the graph of a Walks."""
    _, (run_start, rows, _) = w.want(flat, rs)
    return run_start, rows


# ---- dense small k ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_small_k_dense(k):
    rng = np.random.default_rng(900 + k)
    table_in = L.rand_letters(rng, 200 if k < 5 else 600, L.MESSY)
    query = L.rand_letters(rng, 3000, L.MESSY)
    with native.DeviceCounter(k) as dc:
        dc.push(table_in)
        credited = 0
        for mc in (1, 2):
            w = Walks(dc, k, mc)
            assert w.nu > 0
            for m in (40, 400):
                run_start, rows = ref_rows(w, query, random_cuts(rng, query.size, m))
                support, stats = both(dc, run_start, rows, w.g.links)
                assert int(stats[MISSING]) == 0 and int(stats[CREDITED]) == check_links(rows, run_start, w.g) > 0
                assert (np.diff(run_start.astype(np.int64)) == 0).any()        # empty records among them
                credited += int(stats[CREDITED])
        assert credited > 100                                                   # (the four runs together: the reads walk over many links)


# ---- reads with branches: one record per read ---------------------------------------------------------------------------------------------------
def branchy_case(k):
    recs, flat = L.branchy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        run_start, rows = ref_rows(w, flat, per_read(flat))
        support, stats = both(dc, run_start, rows, w.g.links)
        assert int(stats[MISSING]) == 0 and rows.shape[0] > T
        assert int(stats[CREDITED]) == check_links(rows, run_start, w.g) == int(support.sum()) > 100
        assert (support >= 2).any() and (support == 0).any()


@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_reads_with_branches(k):
    branchy_case(k)


def test_rows_left_on_the_device_by_the_paths_call_and_the_binding():
    import torch
    k = 21
    recs, flat = L.branchy()
    sub = flat[:151 * 200 + 1].copy()
    rs = per_read(sub)
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        nl = w.g.links.size
        run_start, rows = ref_rows(w, sub, rs)
        want = S.link_support_ref(run_start, rows, w.g.links)
        t_in, t_rs = torch.from_numpy(sub).cuda(), torch.from_numpy(rs.view(np.int64)).cuda()
        t_st = torch.zeros(rs.size, dtype=torch.int64, device="cuda")
        t_rows = torch.zeros(rows.shape[0] * RW, dtype=torch.int32, device="cuda")
        t_sup = torch.zeros(nl, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        rc, total = dc.unitigs_paths_device(t_in, None, sub.size, t_rs, rs.size - 1, t_st, t_rows, rows.shape[0])
        assert rc == OK and total == rows.shape[0]
        stats = dc.unitigs_link_support_device(t_st, rs.size - 1, t_rows, total, t_sup, nl)
        assert [stats[n] for n in native.SUP_NAMES] == want[1].tolist()
        assert np.array_equal(t_sup.cpu().numpy().view(U64), want[0])
        run_start2, rows2 = dc.unitigs_paths(sub, rs)
        support, stats = dc.unitigs_link_support(run_start2, rows2)              # a fresh array of n_links counters
        assert np.array_equal(support, want[0]) and [stats[n] for n in native.SUP_NAMES] == want[1].tolist()
        again, _ = dc.unitigs_link_support(run_start2, rows2, support)           # ... and added to
        assert again is support and np.array_equal(support, want[0] * U64(2))


# ---- the strand property ------------------------------------------------------------------------------------------------------------------------
def test_reverse_complemented_reads_credit_the_mirror_words():
    k = 21
    recs, flat = L.branchy()
    sub = recs[:200]
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 2)
        links = w.g.links
        f, b = U.flat_of(sub), U.flat_of([U.rc(r) for r in sub])
        fwd, fstats = both(dc, *ref_rows(w, f, per_read(f)), links)             # (both forms give exactly these)
        rev, rstats = both(dc, *ref_rows(w, b, per_read(b)), links)
        assert int(fstats[CREDITED]) == int(rstats[CREDITED]) > 100
        where = {int(x): i for i, x in enumerate(links)}
        perm = [where[int(x)] for x in native.link_mirror(links)]              # (odd k: the mirror of every link is in the list)
        assert np.array_equal(rev, fwd[perm]) and not np.array_equal(rev, fwd)


# ---- accumulation ---------------------------------------------------------------------------------------------------------------------------------
def test_counts_are_added_and_wrap():
    k = 21
    recs, flat = L.branchy()
    a, b = flat[:151 * 100 + 1].copy(), flat[151 * 100:151 * 250 + 1].copy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        links = w.g.links
        ra, rb = ref_rows(w, a, per_read(a)), ref_rows(w, b, per_read(b))
        first, _ = both(dc, *ra, links)
        second, _ = both(dc, *rb, links, support0=first)
        assert np.array_equal(second, first + S.link_support_ref(*rb, links)[0]) and not np.array_equal(second, first)
        seed = np.arange(links.size, dtype=U64) * U64(3) + U64(5)
        once = int(np.flatnonzero(S.link_support_ref(*rb, links)[0] == 1)[0])    # a counter that this batch credits exactly once
        seed[once] = U64(0xFFFFFFFFFFFFFFFF)
        wrapped, _ = both(dc, *rb, links, support0=seed)
        assert int(wrapped[once]) == 0


# ---- circular unitigs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_circular_unitigs(k):
    flat, keys, counts = U.cycle_input(k)
    records = flat.tobytes().strip(b"N").split(b"N")
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        links = w.g.links
        where = {int(x): i for i, x in enumerate(links)}
        rng = np.random.default_rng(34)
        both(dc, *ref_rows(w, flat, random_cuts(rng, flat.size, 30)), links)
        for i, p in enumerate(U.PERIODS):
            some = np.frombuffer(records[2 * i][:k], dtype=np.uint8).copy()     # one k-mer of the circle: which unitig it is
            u = int(ref_rows(w, some, [0, some.size])[1][0, native.RUN_STATE]) >> 1
            row = w.g.rows[u]
            assert int(row[native.UNI_FLAGS]) & native.UNI_CIRCULAR and int(row[native.UNI_KMERS]) == p
            start = int(row[native.UNI_START])
            unit = w.g.bases[start:start + p].tobytes()                         # one turn of the reported reading, from its first node
            read = (unit * (k // p + 4))[:(5 * p) // 2 + k - 1]                  # two and a half times round
            for r, sign in ((read, 0), (U.rc(read), 1)):
                buf = np.frombuffer(r, dtype=np.uint8).copy()
                run_start, rows = ref_rows(w, buf, [0, buf.size])
                assert rows.shape[0] == 3 and set(rows[:, native.RUN_STATE].tolist()) == {2 * u + sign}
                support, stats = both(dc, run_start, rows, links)
                mine, other = where[native.uni_link_word(u, sign, u, sign)], where[native.uni_link_word(u, 1 - sign, u, 1 - sign)]
                assert int(support[mine]) == 2 and int(support[other]) == 0 and int(support.sum()) == 2 and stats.tolist() == [2, 2, 2, 0]


# ---- one record with every run: thousands of crossings on one counter, over more than one tile ----------------------------------------------------
def test_one_record_with_every_run_and_one_hot_counter():
    k = 21
    flat = np.frombuffer(b"A" * 6000 + b"N" + b"AC" * 3000 + b"N" + b"ACG" * 2000 + b"N" + b"T" * 300, dtype=np.uint8).copy()
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        links = w.g.links
        run_start, rows = ref_rows(w, flat, [0, flat.size])                     # ONE record
        assert run_start.tolist() == [0, rows.shape[0]] and rows.shape[0] > 6 * T
        support, stats = both(dc, run_start, rows, links)
        sa = int(rows[0, native.RUN_STATE])                                     # the poly-A k-mer as the first window reads it
        loop = int(np.flatnonzero(links == U64((sa << 32) | sa))[0])
        assert int(support[loop]) == 6000 - k == 5979                           # every window of the poly-A stretch but the last turns once
        back = int(np.flatnonzero(links == U64(((sa ^ 1) << 32) | (sa ^ 1)))[0])
        assert int(support[back]) == 300 - k                                    # ... and the T stretch walks the same loop the other way
        assert int(stats[MISSING]) == 0 and int(stats[PAIRS]) == rows.shape[0] - 1


# ---- tile edges, with fabricated rows ---------------------------------------------------------------------------------------------------------------
_FORK = {}


def fork_input():
    """The branchy reads and a stem that goes on with each of the four letters: a state with four links out, and dead ends."""
    if not _FORK:
        rng = np.random.default_rng(35)
        stem = L.rand_letters(rng, 40).tobytes()
        recs = [stem + c + L.rand_letters(rng, 30).tobytes() for c in (b"A", b"C", b"G", b"T")]
        _FORK["flat"] = np.concatenate((L.branchy()[1], U.flat_of(recs)[1:]))
    return _FORK["flat"]


def fabricated(links, nu, n, rng):
    """n rows without a gap between them whose states walk the graph at random -- along a link, or anywhere --, with chosen crossings at
    chosen rows; returns the rows."""
    hi, lo = (links >> U64(32)).astype(np.int64), (links & U64(0xFFFFFFFF)).astype(np.int64)
    outs = np.bincount(hi, minlength=2 * nu)
    four = int(np.flatnonzero(outs == 4)[0])
    none = int(np.flatnonzero(outs == 0)[0])
    fourth = int(lo[np.flatnonzero(hi == four)[3]])
    st = np.empty(n, dtype=np.int64)
    st[0] = hi[0]
    for i in range(1, n):
        mine = np.flatnonzero(hi == st[i - 1])
        st[i] = lo[rng.choice(mine)] if mine.size and rng.random() < 0.7 else rng.integers(0, 2 * nu)
    chosen = [(hi[0], lo[0]), (hi[-1], lo[-1]), (four, fourth), (none, lo[0]), (2 * nu, lo[0]), (0xFFFFFFFF, lo[0]), (hi[0], 2 * nu),
              (hi[0], 0xFFFFFFFF), (2 * nu + 1, 2 * nu + 1)]
    for j, (a, b) in enumerate(chosen):
        if 3 * j + 5 < n:
            st[3 * j + 4], st[3 * j + 5] = a, b
    if n > T:
        st[T - 1], st[T] = hi[-1], lo[-1]                                       # the pair that straddles the tile edge: the last link
    if n > 2 * T:
        st[2 * T - 1], st[2 * T] = four, fourth
    rows = np.zeros((n, RW), dtype=U32)
    rows[:, native.RUN_STATE] = st.astype(U32)
    rows[:, native.RUN_QSTART] = np.arange(n, dtype=U32) * U32(7)
    rows[:, native.RUN_QEND] = rows[:, native.RUN_QSTART] + U32(7)
    return rows, len(chosen)


def tile_edge_case():
    k = 21
    flat = fork_input()
    rng = np.random.default_rng(36)
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        links = w.g.links
        for n in (T - 1, T, T + 1, 2 * T + 3):
            rows, n_chosen = fabricated(links, w.nu, n, rng)
            whole, stats = both(dc, [0, n], rows, links)                        # one record: the pair (T - 1, T) straddles the edge
            assert int(stats[PAIRS]) == int(stats[ADJACENT]) == n - 1 and int(stats[MISSING]) >= 6 and int(whole[0]) >= 1 and int(whole[-1]) >= 1
            cut = np.minimum(np.array([0, T - 1, T, T + 1, n], dtype=U64), U64(n))
            parts, pstats = both(dc, cut, rows, links)                          # boundaries at rows T - 1, T and T + 1
            from_edge, estats = both(dc, np.minimum(np.array([0, 0, T - 1, n], dtype=U64), U64(n)), rows, links)
            if n > T + 1:
                assert int(pstats[PAIRS]) == n - 4 and int(estats[PAIRS]) == n - 2
                assert int(whole[-1]) - int(parts[-1]) == 1 and int(from_edge[-1]) == int(whole[-1])   # cut exactly there: one credit less
            gap = rows.copy()
            gap[T // 2:, native.RUN_QSTART] += U32(1)                           # one gap in front of row T / 2, none elsewhere
            gap[T // 2:, native.RUN_QEND] += U32(1)
            _, gstats = both(dc, [0, n], gap, links)
            assert int(gstats[PAIRS]) - int(gstats[ADJACENT]) == 1


def test_tile_edges_with_fabricated_rows():
    tile_edge_case()


# ---- alignment ------------------------------------------------------------------------------------------------------------------------------------
def test_alignment_of_the_rows():
    k = 21
    flat = fork_input()
    rng = np.random.default_rng(37)
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        rows, _ = fabricated(w.g.links, w.nu, 2 * T + 3, rng)
        cut = np.array([0, 5, 5, T, T + 1, 2 * T + 3], dtype=U64)
        for roff in (0, 1, 2, 3):                                               # d_runs 16-, 4-, 8- and 4-byte aligned
            both(dc, cut, rows, w.g.links, roff=roff)


# ---- errors and states ----------------------------------------------------------------------------------------------------------------------------
def _small(w, flat):
    sub = flat[:151 * 20 + 1].copy()
    return ref_rows(w, sub, per_read(sub))


def test_state_errors_leave_the_outputs_untouched():
    k = 21
    recs, flat = L.branchy()
    lib = native.lib()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        links = w.g.links
        run_start, rows = _small(w, flat)
        want = both(dc, run_start, rows, links)
        dc.unitigs_end()

        def refused(text):
            for call in (support_device, support_host):
                got = call(dc, run_start, rows, links.size, support0=np.full(links.size, 9, dtype=U64))
                assert got.rc == STATE and text in lib.kh_last_error(dc._h), (call.__name__, got.rc, lib.kh_last_error(dc._h))
                assert (got.support == U64(9)).all() and (got.stats == U64(CANARY)).all()

        refused(b"no unitigs")                                                  # after kh_unitigs_end
        dc.unitigs_begin(1)
        refused(b"kh_unitigs_begin_linked")                                     # a plain begin built no links
        Walks(dc, k, 1)
        dc.push(np.frombuffer(b"ACGTTGCAAGGCTTAACCGATAGGA", dtype=np.uint8))
        refused(b"no unitigs")                                                  # a push made them stale
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        for call in (support_device, support_host):                             # before any begin
            got = call(dc, run_start, rows, links.size)
            assert got.rc == STATE and (got.stats == U64(CANARY)).all() and not got.support.any()
        dc.push(flat)
        w = Walks(dc, k, 1)
        assert np.array_equal(both(dc, run_start, rows, w.g.links)[0], want[0])


def test_cap_and_bad_arguments_leave_the_context_usable():
    import torch
    k = 21
    recs, flat = L.branchy()
    lib = native.lib()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        links = w.g.links
        nl = links.size
        run_start, rows = _small(w, flat)
        nrec, n = run_start.size - 1, rows.shape[0]
        seed = np.full(nl, 9, dtype=U64)
        for call in (support_device, support_host):                             # cap = n_links - 1: RANGE, nothing written
            for cap in (nl - 1, 0):
                got = call(dc, run_start, rows, nl, support0=seed, cap=cap)
                assert got.rc == RANGE and (got.support == U64(9)).all() and (got.stats == U64(CANARY)).all(), (call.__name__, cap)
            both(dc, run_start, rows, links)
        sup, out = np.full(nl + 2, 9, dtype=U64), np.full(SW, CANARY, dtype=U64)
        rows_h = _rows32(rows)
        rows_d = np.zeros(rows_h.size + 4, dtype=U32)
        rows_d[:rows_h.size] = rows_h.reshape(-1)
        t_rs, t_rows = torch.from_numpy(run_start.view(np.int64)).cuda(), torch.from_numpy(rows_d.view(np.int32)).cuda()
        t_sup = torch.from_numpy(sup.view(np.int64)).cuda()
        torch.cuda.synchronize()
        for f, r_, w_, s_ in ((lib.kh_unitigs_link_support, run_start.ctypes.data, rows_h.ctypes.data, sup.ctypes.data),
                              (lib.kh_unitigs_link_support_device, t_rs.data_ptr(), t_rows.data_ptr(), t_sup.data_ptr())):
            good = (dc._h, r_, nrec, w_, n, s_, nl, out.ctypes.data)

            def with_(**kw):
                names = ("ctx", "run_start", "nrec", "runs", "n_runs", "support", "cap", "out")
                return f(*[kw.get(name, v) for name, v in zip(names, good)])
            for bad in (dict(ctx=None), dict(run_start=None), dict(runs=None), dict(run_start=None, n_runs=0), dict(support=None),
                        dict(runs=w_ + 2), dict(run_start=r_ + 4), dict(support=s_ + 4)):
                assert with_(**bad) == BAD_ARG, bad
                if bad.get("ctx", 1) is not None:
                    both(dc, run_start, rows, links)                            # the next good call gives the right answer
            assert with_(runs=w_ + 2) == BAD_ARG and b"4-byte" in lib.kh_last_error(dc._h)
            assert with_(support=s_ + 4) == BAD_ARG and b"8-byte" in lib.kh_last_error(dc._h)
            assert with_(out=None) == OK                                        # out may be NULL
        assert (out == U64(CANARY)).all()
        assert (t_sup.cpu().numpy().view(U64)[nl:] == U64(9)).all() and (sup[nl:] == U64(9)).all()
        # the host form checks the offsets too
        down = run_start.copy()
        down[2] = down[1] + U64(1)
        down[3] = down[1]
        got = support_host(dc, down, rows, nl, support0=seed)
        assert got.rc == BAD_ARG and b"ascending" in lib.kh_last_error(dc._h) and (got.support == U64(9)).all()
        short = run_start.copy()
        short[-1] -= U64(1)
        got = support_host(dc, short, rows, nl, support0=seed)
        assert got.rc == BAD_ARG and b"n_runs" in lib.kh_last_error(dc._h) and (got.support == U64(9)).all() and (got.stats == U64(CANARY)).all()
        both(dc, run_start, rows, links)


def test_degenerate_inputs():
    k = 21
    recs, flat = L.branchy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        links = w.g.links
        run_start, rows = _small(w, flat)
        seed = np.full(links.size, 9, dtype=U64)
        for call in (support_device, support_host):
            for rs, rw in (([0, 0], rows[:0]), ([0, 1], rows[:1]), ([0, 0, 1, 1], rows[:1])):     # n_runs of 0 and 1
                got = call(dc, rs, rw, links.size, support0=seed)
                assert got.rc == OK and (got.support == U64(9)).all() and got.stats.tolist() == [0, 0, 0, 0], (call.__name__, rs)
            got = call(dc, [int(rows.shape[0])], rows, links.size, support0=seed)                 # nrec == 0
            assert got.rc == OK and (got.support == U64(9)).all() and got.stats.tolist() == [0, 0, 0, 0]
        lib, out = native.lib(), np.full(SW, CANARY, dtype=U64)
        assert lib.kh_unitigs_link_support(dc._h, None, 0, None, 0, None, 0, out.ctypes.data) == RANGE       # NULL support needs n_links == 0
    one = L.rand_letters(np.random.default_rng(38), 300)
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:                  # one unitig and no links
        dc.push(one)
        w = Walks(dc, k, 1)
        assert w.nu == 1 and w.g.links.size == 0
        rows = np.array([[0, 0, 0, 100], [0, 100, 100, 280]], dtype=U32)       # (hand-made: adjacent, and no link to credit)
        want = both(dc, [0, 2], rows, w.g.links)
        assert want[1].tolist() == [1, 1, 0, 1]
        lib, out = native.lib(), np.zeros(SW, dtype=U64)
        rs = np.array([0, 2], dtype=U64)
        assert lib.kh_unitigs_link_support(dc._h, rs.ctypes.data, 1, rows.ctypes.data, 2, None, 0, out.ctypes.data) == OK and out.tolist() == [1, 1, 0, 1]


# ---- a reader ---------------------------------------------------------------------------------------------------------------------------------------
def test_a_call_inside_a_gfa_stream_changes_nothing():
    k = 21
    recs, flat = L.branchy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        before = TJ.stats_of(dc)
        w = Walks(dc, k, 1)
        links = w.g.links
        run_start, rows = _small(w, flat)

        def document(calls):
            total = dc.unitigs_text_begin("gfa")
            doc, piece = bytearray(), np.empty(1000, dtype=np.uint8)
            while True:
                m = dc.unitigs_text_next(piece)
                if m == 0:
                    break
                doc += piece[:m].tobytes()
                if calls and len(doc) < 6000:
                    both(dc, run_start, rows, links)
            assert len(doc) == total
            return bytes(doc)

        plain = document(False)
        assert document(True) == plain and len(plain) > 6000
        assert TJ.stats_of(dc) == before
        assert np.array_equal(dc.unitigs_links_copy(links.size), links)


# ---- past the first grid stride: one process per cap ------------------------------------------------------------------------------------------------
_CHILD_DIED = []


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride(cap):
    """KMERHIP_GRID_CAP (test build), one value per process: one and three workgroups go round the tile loop many times.  After a child
    that ended on a signal or at its timeout no further one is started."""
    assert not _CHILD_DIED, "not started: an earlier child ended on a signal or at its timeout (%s)" % _CHILD_DIED[0]
    try:
        p = subprocess.run([sys.executable, CHILD], capture_output=True, text=True, env=dict(os.environ, KMERHIP_GRID_CAP=str(cap)), timeout=300, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _CHILD_DIED.append("timeout")
        raise
    if p.returncode < 0:
        _CHILD_DIED.append("signal %d" % -p.returncode)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
