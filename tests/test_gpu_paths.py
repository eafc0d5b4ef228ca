"""kh_unitigs_paths* -- reads as run-compressed walks over the live unitigs -- against paths_ref of tests/test_paths_ref.py: a plain
loop over the words that locate_ref (tests/test_locate_ref.py) gives for the unitigs kh_unitigs_copy returns.

Every case compares run_start, every row and the coverage array exactly, with canaries on both sides of all three outputs, in the
device form and in the host form on the same buffers.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_graph as G
import test_gpu_join as T
import test_gpu_locate as L
import test_gpu_unitigs as U
import test_locate_ref as R
import test_paths_ref as P
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64, U32 = np.uint64, np.uint32
CANARY, CANARY32 = 0xABABABABABABABAB, 0xCDCDCDCD
NO_WINDOW = native.LOC_NO_WINDOW
OK, STATE, BAD_ARG, RANGE = native.KH_OK, native.KH_ERR_STATE, native.KH_ERR_BAD_ARG, native.KH_ERR_RANGE
TILE, RW, CW = 4096, native.RUN_WORDS, native.COV_WORDS
PAD = 16      # canary rows in front of the caller's first row (64 words: a 16-byte boundary)


class Got:
    def __init__(self, rc, total, run_start, rows, cover):
        self.rc, self.total, self.run_start, self.rows, self.cover = rc, total, run_start, rows, cover


def _runs_buffer(run_cap, roff):
    return np.full(RW * (PAD + run_cap + PAD) + 4, CANARY32, dtype=U32), RW * PAD + roff


def _check_runs(buf, at, run_cap, who):
    """Nothing in front of row 0 and nothing at or behind row run_cap."""
    assert (buf[:at] == U32(CANARY32)).all() and (buf[at + RW * run_cap:] == U32(CANARY32)).all(), who + " wrote outside runs"
    return buf[at:at + RW * run_cap].reshape(run_cap, RW).copy()


def paths_device(dc, nu, flat, rs, qual=None, run_cap=None, cover0=None, with_cover=True, boff=0, qoff=0, roff=0):
    """kh_unitigs_paths_device with d_bases at byte boff (mod 16), d_qual at qoff, d_runs 4 * roff bytes behind a 16-byte boundary;
    run_cap None: sized by a first call with run_cap 0 and NULL rows.  cover0: what the coverage array holds before."""
    import torch
    n, nrec = int(flat.size), len(rs) - 1
    hb = np.full(n + 64, ord("A"), dtype=np.uint8)
    hb[16 + boff:16 + boff + n] = flat
    tb = torch.from_numpy(hb).cuda()
    tq = None
    if qual is not None:
        hq = np.full(n + 64, ord("I"), dtype=np.uint8)
        hq[16 + qoff:16 + qoff + n] = qual
        tq = torch.from_numpy(hq).cuda()
    t_rs = torch.from_numpy(np.asarray(rs, dtype=U64).view(np.int64)).cuda()
    t_st = torch.from_numpy(np.full(nrec + 1 + 8, CANARY, dtype=U64).view(np.int64)).cuda()
    hc = np.full(nu * CW + 8, CANARY, dtype=U64)
    hc[4:4 + nu * CW] = 0 if cover0 is None else np.asarray(cover0, dtype=U64).reshape(-1)
    t_cov = torch.from_numpy(hc.view(np.int64)).cuda()
    torch.cuda.synchronize()
    pb, pq = tb.data_ptr() + 16 + boff, None if tq is None else tq.data_ptr() + 16 + qoff
    p_st, p_cov = t_st.data_ptr() + 32, (t_cov.data_ptr() + 32) if with_cover else None
    if run_cap is None:
        rc, total = dc.unitigs_paths_device(pb, pq, n, t_rs, nrec, p_st, None, 0, p_cov)
        assert rc == (RANGE if total else OK)
        sized = t_st.cpu().numpy().view(U64)[4:4 + nrec + 1].copy()
        assert np.array_equal(t_cov.cpu().numpy().view(U64), hc) or total == 0, "a sizing call changed cover"
        run_cap = total
    else:
        sized = None
    buf, at = _runs_buffer(run_cap, roff)
    t_runs = torch.from_numpy(buf.view(np.int32)).cuda()
    torch.cuda.synchronize()
    assert t_runs.data_ptr() % 16 == 0 and tb.data_ptr() % 16 == 0
    rc, total = dc.unitigs_paths_device(pb, pq, n, t_rs, nrec, p_st, (t_runs.data_ptr() + 4 * at) if run_cap else None, run_cap, p_cov)
    st = t_st.cpu().numpy().view(U64)
    assert (st[:4] == U64(CANARY)).all() and (st[4 + nrec + 1:] == U64(CANARY)).all(), "kh_unitigs_paths_device wrote outside d_run_start"
    cov = t_cov.cpu().numpy().view(U64)
    assert (cov[:4] == U64(CANARY)).all() and (cov[4 + nu * CW:] == U64(CANARY)).all(), "kh_unitigs_paths_device wrote outside d_cover"
    rows = _check_runs(t_runs.cpu().numpy().view(U32), at, run_cap, "kh_unitigs_paths_device")
    if sized is not None:
        assert np.array_equal(sized, st[4:4 + nrec + 1]), "the sizing call's run_start differs"
    return Got(rc, total, st[4:4 + nrec + 1].copy(), rows[:min(total, run_cap)], cov[4:4 + nu * CW].reshape(nu, CW).copy())


def paths_host(dc, nu, flat, rs, qual=None, run_cap=None, cover0=None, with_cover=True):
    lib = native.lib()
    n, nrec = int(flat.size), len(rs) - 1
    a_rs = np.asarray(rs, dtype=U64)
    st = np.full(nrec + 1 + 8, CANARY, dtype=U64)
    cov = np.full(nu * CW + 8, CANARY, dtype=U64)
    cov[4:4 + nu * CW] = 0 if cover0 is None else np.asarray(cover0, dtype=U64).reshape(-1)
    total = C.c_uint64(0)
    p_cov = cov[4:].ctypes.data if with_cover else None
    qp = None if qual is None else qual.ctypes.data
    if run_cap is None:
        rc = lib.kh_unitigs_paths(dc._h, flat.ctypes.data, qp, n, a_rs.ctypes.data, nrec, st[4:].ctypes.data, None, 0, p_cov, C.byref(total))
        assert rc == (RANGE if total.value else OK), native.lib().kh_last_error(dc._h)
        run_cap = total.value
    buf, at = _runs_buffer(run_cap, 0)
    rc = lib.kh_unitigs_paths(dc._h, flat.ctypes.data, qp, n, a_rs.ctypes.data, nrec, st[4:].ctypes.data, buf[at:].ctypes.data if run_cap else None,
                              run_cap, p_cov, C.byref(total))
    assert (st[:4] == U64(CANARY)).all() and (st[4 + nrec + 1:] == U64(CANARY)).all(), "kh_unitigs_paths wrote outside run_start"
    assert (cov[:4] == U64(CANARY)).all() and (cov[4 + nu * CW:] == U64(CANARY)).all(), "kh_unitigs_paths wrote outside cover"
    rows = _check_runs(buf, at, run_cap, "kh_unitigs_paths")
    return Got(rc, total.value, st[4:4 + nrec + 1].copy(), rows[:min(total.value, run_cap)], cov[4:4 + nu * CW].reshape(nu, CW).copy())


class Walks:
    """A Graph of tests/test_gpu_locate.py and the reference's answers on it."""

    def __init__(self, dc, k, mc=1):
        self.g = L.Graph(dc, k, mc)
        self.dc, self.k, self.nu = dc, k, self.g.rows.shape[0]

    def want(self, flat, rs, qual=None):
        words = self.g.want(flat, qual)
        return words, P.paths_ref(words, rs, self.nu)

    def same(self, got, want, who, cover0=None):
        run_start, rows, cover = want
        assert got.rc == OK and got.total == rows.shape[0], (who, got.rc, got.total, rows.shape[0])
        assert np.array_equal(got.run_start, run_start), (who, "run_start", np.flatnonzero(got.run_start != run_start)[:5])
        if not np.array_equal(got.rows, rows):
            i = int(np.flatnonzero((got.rows != rows).any(axis=1))[0])
            raise AssertionError("%s, k=%d: %d of %d rows differ, first %d: %r for %r" %
                                 (who, self.k, int((got.rows != rows).any(axis=1).sum()), rows.shape[0], i, got.rows[i].tolist(), rows[i].tolist()))
        base = np.zeros_like(cover) if cover0 is None else np.asarray(cover0, dtype=U64).reshape(cover.shape)
        assert np.array_equal(got.cover, base + cover), (who, "cover")

    def both(self, flat, rs, qual=None, **kw):
        """The device form and the host form on one buffer; returns the reference's (words, (run_start, rows, cover))."""
        words, want = self.want(flat, rs, qual)
        self.same(paths_device(self.dc, self.nu, flat, rs, qual, **kw), want, "device")
        self.same(paths_host(self.dc, self.nu, flat, rs, qual), want, "host")
        return words, want


def random_cuts(rng, n, m, lo=0, hi=None):
    """m + 1 ascending offsets in [lo, hi]: some of them equal (empty records), most of them inside reads and runs."""
    hi = n if hi is None else hi
    cuts = np.sort(rng.integers(lo, hi + 1, size=m + 1))
    cuts[3:6] = cuts[3]                                         # three records that start at one entry, two of them empty
    return np.sort(cuts).astype(U64)


def per_read(flat, read_len=150):
    """One record per read of flat_of(): N r N r ... N."""
    assert (flat.size - 1) % (read_len + 1) == 0
    return np.arange(1, flat.size + 1, read_len + 1, dtype=U64)


# ---- dense small k ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", ["acgt", "messy"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_small_k_dense(k, alphabet):
    rng = np.random.default_rng(700 + k)
    letters = L.ACGT if alphabet == "acgt" else L.MESSY
    table_in = L.rand_letters(rng, 200 if k < 5 else 600, letters)
    query = L.rand_letters(rng, 3000, letters)
    with native.DeviceCounter(k) as dc:
        dc.push(table_in)
        for mc in (1, 2):
            w = Walks(dc, k, mc)
            assert w.nu > 0
            w.both(query, [0, query.size])
            words, (run_start, rows, cover) = w.both(query, random_cuts(rng, query.size, 40, lo=7, hi=query.size - 9))
            assert rows.shape[0] > 100 and (np.diff(run_start.astype(np.int64)) == 0).any()
            words, (run_start, rows, cover) = w.both(query, random_cuts(rng, query.size, 400))        # records of a few windows
            assert rows.shape[0] > 400


# ---- reads with branches: one record per read ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_reads_with_branches(k):
    import torch
    recs, flat = L.branchy()
    rs = per_read(flat)
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        for mc in (1, 2):
            w = Walks(dc, k, mc)
            words, (run_start, rows, cover) = w.both(flat, rs)
            own = L.locate_device(dc, flat)                                # the device's own words
            assert np.array_equal(P.expand(run_start, rows, rs, flat.size), P.places_inside(own, rs))
            assert int(cover[:, native.COV_WINDOWS].sum()) == int(np.sum(P.places_inside(own, rs) != U64(NO_WINDOW)))
            assert int(cover[:, native.COV_RUNS].sum()) == rows.shape[0]
            if mc == 1:
                places = int(np.sum(native.loc_is_place(words)))
                assert rows.shape[0] > len(recs) and w.nu > 100
                assert check_links(rows, run_start, w.g) > places // 100    # the reads walk over many links


def check_links(rows, run_start, g):
    """Consecutive runs of a record without a gap are joined by a link word; returns how many were."""
    links, joined = set(int(x) for x in g.links), 0
    for r in range(run_start.size - 1):
        part = rows[int(run_start[r]):int(run_start[r + 1])].tolist()
        for a, b in zip(part, part[1:]):
            if a[native.RUN_QEND] == b[native.RUN_QSTART]:
                assert (a[native.RUN_STATE] << 32) | b[native.RUN_STATE] in links, (a, b)
                joined += 1
    return joined


def test_reverse_complement_property_per_record():
    k = 21
    recs, flat = L.branchy()
    sub = recs[:200]
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 2)
        f, b = U.flat_of(sub), U.flat_of([U.rc(r) for r in sub])
        fwd = paths_device(dc, w.nu, f, per_read(f))
        rev = paths_device(dc, w.nu, b, per_read(b))
        assert fwd.rc == OK and rev.rc == OK and fwd.total == rev.total > 300
        for r in range(len(sub)):
            mine = fwd.rows[int(fwd.run_start[r]):int(fwd.run_start[r + 1])]
            theirs = rev.rows[int(rev.run_start[r]):int(rev.run_start[r + 1])]
            assert np.array_equal(theirs, P.mirrored(mine, len(sub[r]) - k + 1)), r


# ---- tile edges: one run across three tiles, record boundaries on a tile's edge --------------------------------------------------------------------
def test_one_long_run_and_records_cut_at_a_tile_edge():
    k = 21
    rng = np.random.default_rng(21)
    flat = L.rand_letters(rng, 10_000)
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        assert w.nu == 1
        words, (run_start, rows, cover) = w.both(flat, [0, flat.size])
        assert rows.shape[0] == 1 and rows[0, native.RUN_QEND] - rows[0, native.RUN_QSTART] == flat.size - k + 1
        words, (run_start, rows, cover) = w.both(flat, [0, TILE - 1, TILE, TILE + 1, flat.size])
        assert rows.shape[0] == 4 and run_start.tolist() == [0, 1, 2, 3, 4]
        w.both(flat, [5, 5, TILE, TILE, 2 * TILE, 2 * TILE, 9000])         # empty records on the edges, none at either end of the buffer
        w.both(flat, [flat.size, flat.size, flat.size])                     # records that start where the buffer ends


# ---- the densest ranks: every window a run ----------------------------------------------------------------------------------------------------------
def test_poly_a_and_short_periods_over_two_tiles():
    k = 21
    flat = np.frombuffer(b"A" * 6000 + b"N" + b"AC" * 3000 + b"N" + b"ACG" * 2000 + b"N" + b"T" * 300, dtype=np.uint8).copy()
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        words, (run_start, rows, cover) = w.both(flat, [0, flat.size])
        poly = rows[rows[:, native.RUN_QEND] <= 6000 - k + 1]
        assert poly.shape[0] == 6000 - k + 1 and (poly[:, native.RUN_QEND] - poly[:, native.RUN_QSTART] == 1).all()   # runs = windows
        assert rows.shape[0] > 6000 + 3000 - 50
        rng = np.random.default_rng(22)
        w.both(flat, random_cuts(rng, flat.size, 300))
        w.both(flat, [0, 6001, 12002, 18003, flat.size], roff=1)


# ---- quality masking ----------------------------------------------------------------------------------------------------------------------------
def test_quality_masking():
    k = 21
    recs, flat = L.branchy()
    sub = flat[:151 * 200 + 1].copy()
    rng = np.random.default_rng(23)
    qual = (33 + rng.integers(15, 41, size=sub.size)).astype(np.uint8)
    with native.DeviceCounter(k, min_quality=20, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        words, (run_start, rows, cover) = w.both(sub, per_read(sub), qual)
        plain, (_, prows, _) = w.both(sub, per_read(sub), None)
        assert int(np.sum(words == U64(NO_WINDOW))) - int(np.sum(plain == U64(NO_WINDOW))) > 300   # the threshold masks windows the letters allow


# ---- min_count 1 and 3 on the same table ------------------------------------------------------------------------------------------------------------
def test_min_count_1_and_3_on_the_same_table():
    k = 21
    recs, flat = L.branchy()
    sub = flat[:151 * 200 + 1].copy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        n_rows = {}
        for mc in (1, 3, 1):
            w = Walks(dc, k, mc)
            n_rows[mc] = w.both(sub, per_read(sub))[1][1].shape[0]
        assert n_rows[1] != n_rows[3]


# ---- circular unitigs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_circular_unitigs(k):
    flat, keys, counts = U.cycle_input(k)
    records = flat.tobytes().strip(b"N").split(b"N")
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        rng = np.random.default_rng(24)
        w.both(flat, random_cuts(rng, flat.size, 30))
        for i, p in enumerate(U.PERIODS):
            unit = records[2 * i][:p]
            read = (unit * (k // p + 4))[:(5 * p) // 2 + k - 1]            # two and a half times round
            for r in (read, U.rc(read)):
                buf = np.frombuffer(r, dtype=np.uint8).copy()
                words, (run_start, rows, cover) = w.both(buf, [0, buf.size])
                assert rows.shape[0] in (3, 4) and len(set(rows[:, native.RUN_STATE].tolist())) == 1            # a new run at every closing link
                assert (rows[1:, native.RUN_QSTART] == rows[:-1, native.RUN_QEND]).all()
                assert rows[1, native.RUN_QEND] - rows[1, native.RUN_QSTART] == p


# ---- table forms ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["wide", "image", "regions3072", "grown"])
def test_table_forms(form, monkeypatch):
    k = 21
    flat, keys, counts = G.main_input(k)
    sub = flat[:20 * 151].copy()
    with T.table(form, k, flat, monkeypatch) as dc:
        before = T.stats_of(dc)
        w = Walks(dc, k, 1)
        assert w.both(sub, [3, 1000, 1000, 2500, sub.size - 2])[1][1].shape[0] >= 3
        assert T.stats_of(dc) == before


# ---- chunks of 1024 window starts, in both forms --------------------------------------------------------------------------------------------------
def test_small_chunks_in_both_forms(monkeypatch):
    k = 21
    recs, flat = L.branchy()
    sub = flat[:20_000].copy()
    rng = np.random.default_rng(25)
    qual = (33 + rng.integers(5, 41, size=sub.size)).astype(np.uint8)
    long_rec = L.rand_letters(rng, 5000)                                    # one run over four chunk edges
    rs = np.sort(np.concatenate((per_read(flat)[:100], np.array([1024, 1024, 2048, 3071, 3072, 3073, 19_000], dtype=U64))))
    with native.DeviceCounter(k, min_quality=10, capacity_hint=200_000) as dc:
        dc.push(flat)
        dc.push(np.concatenate((np.frombuffer(b"N", dtype=np.uint8), long_rec)))
        w = Walks(dc, k, 1)
        words, want = w.want(sub, rs, qual)
        lwords, lwant = w.want(long_rec, [0, long_rec.size])
        assert lwant[1].shape[0] == 1
        whole = paths_device(dc, w.nu, sub, rs, qual)
        w.same(whole, want, "device, one chunk")
        monkeypatch.setenv("KMERHIP_PROFILE_CHUNK_KB", "1")
        try:
            w.same(paths_device(dc, w.nu, sub, rs, qual, boff=3, qoff=9), want, "device, chunks of 1024")
            w.same(paths_host(dc, w.nu, sub, rs, qual), want, "host, chunks of 1024")
            w.same(paths_device(dc, w.nu, long_rec, [0, long_rec.size]), lwant, "device, one run over four chunks")
            w.same(paths_host(dc, w.nu, long_rec, [0, long_rec.size]), lwant, "host, one run over four chunks")
            with native.PinnedArray(sub.size) as pb, native.PinnedArray(sub.size) as pq:
                pb.array[:] = sub
                pq.array[:] = qual
                w.same(paths_host(dc, w.nu, pb.array, rs, pq.array), want, "host, pinned, chunks of 1024")
        finally:
            monkeypatch.delenv("KMERHIP_PROFILE_CHUNK_KB")
        w.same(paths_host(dc, w.nu, sub, rs, qual), want, "host, one chunk")
        prof = dc.profile(sub, qual)                                        # the profile shares the chunk buffers: it still does what it did
        assert np.array_equal(words == U64(NO_WINDOW), prof == native.PROFILE_NO_WINDOW)
        assert np.array_equal(L.locate_host(dc, sub, qual), words)


# ---- alignment ------------------------------------------------------------------------------------------------------------------------------------
def test_alignment_of_rows_bases_and_qualities():
    k = 21
    recs, flat = L.branchy()
    sub = flat[:2 * TILE + 77].copy()
    rng = np.random.default_rng(26)
    qual = (33 + rng.integers(2, 41, size=sub.size)).astype(np.uint8)
    rs = random_cuts(rng, sub.size, 60)
    with native.DeviceCounter(k, min_quality=10, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        words, want = w.want(sub, rs, qual)
        single = int(np.sum(want[1][:, native.RUN_QEND] - want[1][:, native.RUN_QSTART] == 1))
        assert single > 5                                                   # rows that one lane writes whole
        for roff in (0, 1, 2):                                              # d_runs 16-, 4- and 8-byte aligned
            for boff, qoff in ((0, 0), (1, 1), (7, 12), (15, 4)):
                w.same(paths_device(dc, w.nu, sub, rs, qual, roff=roff, boff=boff, qoff=qoff), want, "device %d %d %d" % (roff, boff, qoff))


# ---- coverage -------------------------------------------------------------------------------------------------------------------------------------
def test_cover_accumulates_over_calls_and_may_be_null():
    k = 21
    recs, flat = L.branchy()
    a, b = flat[:151 * 100 + 1].copy(), flat[151 * 100:151 * 250 + 1].copy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        _, wa = w.want(a, per_read(a))
        _, wb = w.want(b, per_read(b))
        for call in (paths_device, paths_host):
            first = call(dc, w.nu, a, per_read(a))
            w.same(first, wa, call.__name__)
            second = call(dc, w.nu, b, per_read(b), cover0=first.cover)
            w.same(second, wb, call.__name__, cover0=wa[2])
            assert np.array_equal(second.cover, wa[2] + wb[2])
            none = call(dc, w.nu, a, per_read(a), with_cover=False, cover0=first.cover)
            assert none.rc == OK and np.array_equal(none.rows, wa[1]) and np.array_equal(none.cover, first.cover)   # (never touched)
        run_start, runs = dc.unitigs_paths(a, per_read(a))                  # the binding: sized by a first call
        assert np.array_equal(run_start, wa[0]) and np.array_equal(runs, wa[1])
        cover = np.zeros((w.nu, CW), dtype=U64)
        run_start, runs = dc.unitigs_paths(b, per_read(b), cover=cover)
        assert np.array_equal(runs, wb[1]) and np.array_equal(cover, wb[2])
        with pytest.raises(native.KmerHipError) as e:
            dc.unitigs_paths(b, per_read(b), cover=cover, run_cap=3)
        assert e.value.status == RANGE and np.array_equal(cover, wb[2])


# ---- run_cap ----------------------------------------------------------------------------------------------------------------------------------------
def test_run_cap():
    k = 21
    recs, flat = L.branchy()
    sub = flat[:151 * 60 + 1].copy()
    rs = per_read(sub)
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        _, want = w.want(sub, rs)
        total = want[1].shape[0]
        seed = np.arange(w.nu * CW, dtype=U64) + U64(5)
        for call in (paths_device, paths_host):
            for cap in (0, 1, total - 1):                                   # too small: RANGE, the counts complete, cover unchanged
                got = call(dc, w.nu, sub, rs, run_cap=cap, cover0=seed)
                assert got.rc == RANGE and got.total == total and np.array_equal(got.run_start, want[0]), (call.__name__, cap)
                assert np.array_equal(got.cover.reshape(-1), seed)
                assert b"run_cap" in native.lib().kh_last_error(dc._h)
            for cap in (total, total + 7):
                w.same(call(dc, w.nu, sub, rs, run_cap=cap, cover0=seed), want, call.__name__, cover0=seed)
        w.both(sub, rs)                                                     # the context is usable


# ---- degenerate inputs ------------------------------------------------------------------------------------------------------------------------------
def test_no_records_no_bases_and_an_empty_s():
    import torch
    k = 21
    recs, flat = L.branchy()
    sub = flat[:1000].copy()
    lib = native.lib()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        total = C.c_uint64(77)
        st = np.full(4, CANARY, dtype=U64)
        assert lib.kh_unitigs_paths(dc._h, sub.ctypes.data, None, sub.size, None, 0, None, None, 0, None, C.byref(total)) == OK and total.value == 0
        total.value = 77
        assert lib.kh_unitigs_paths(dc._h, sub.ctypes.data, None, sub.size, st.ctypes.data, 0, st.ctypes.data, None, 0, None, C.byref(total)) == OK
        assert total.value == 0 and (st == U64(CANARY)).all()             # nrec == 0: nothing else written
        t_in = torch.from_numpy(sub).cuda()
        total.value = 77
        assert lib.kh_unitigs_paths_device(dc._h, t_in.data_ptr(), None, sub.size, None, 0, None, None, 0, None, C.byref(total)) == OK and total.value == 0
        for call in (paths_device, paths_host):                             # n == 0 with records: every offset 0
            got = call(dc, w.nu, sub[:0], [0, 0, 0, 0])
            assert got.rc == OK and got.total == 0 and got.run_start.tolist() == [0, 0, 0, 0] and not got.cover.any()
        dc.reset()
        assert dc.unitigs_begin(1) == (0, 0)                                # an empty S
        for call in (paths_device, paths_host):
            got = call(dc, 0, sub, [0, 500, sub.size])
            assert got.rc == OK and got.total == 0 and got.run_start.tolist() == [0, 0, 0]
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:             # every k-mer below min_count: an empty S over a table that holds keys
        dc.push(flat)
        assert dc.unitigs_begin(1 << 40) == (0, 0)
        got = paths_device(dc, 0, sub, [0, sub.size])
        assert got.rc == OK and got.total == 0 and got.run_start.tolist() == [0, 0]


# ---- state ------------------------------------------------------------------------------------------------------------------------------------------
def test_state_errors_leave_the_outputs_untouched():
    import torch
    k = 21
    recs, flat = L.branchy()
    sub = flat[:1000].copy()
    rs = np.array([0, 400, 1000], dtype=U64)
    lib = native.lib()
    st, rows, cov = np.full(3, CANARY, dtype=U64), np.full(400, CANARY32, dtype=U32), np.full(4000, CANARY, dtype=U64)
    t_in, t_rs = torch.from_numpy(sub).cuda(), torch.from_numpy(rs.view(np.int64)).cuda()
    t_st, t_rows, t_cov = (torch.from_numpy(x.view(np.int64 if x.dtype == U64 else np.int32)).cuda() for x in (st, rows, cov))

    def refused(dc):
        total = C.c_uint64(0)
        for rc in (lib.kh_unitigs_paths(dc._h, sub.ctypes.data, None, sub.size, rs.ctypes.data, 2, st.ctypes.data, rows.ctypes.data, 100,
                                        cov.ctypes.data, C.byref(total)),
                   lib.kh_unitigs_paths_device(dc._h, t_in.data_ptr(), None, sub.size, t_rs.data_ptr(), 2, t_st.data_ptr(), t_rows.data_ptr(), 100,
                                               t_cov.data_ptr(), C.byref(total))):
            assert rc == STATE and b"no unitigs: kh_unitigs_begin first" in lib.kh_last_error(dc._h), (rc, lib.kh_last_error(dc._h))
        assert (st == U64(CANARY)).all() and (rows == U32(CANARY32)).all() and (cov == U64(CANARY)).all()
        assert (t_st.cpu().numpy().view(U64) == U64(CANARY)).all() and (t_rows.cpu().numpy().view(U32) == U32(CANARY32)).all()
        assert (t_cov.cpu().numpy().view(U64) == U64(CANARY)).all()

    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        refused(dc)                                                         # an empty context, before any begin
        dc.push(flat)
        refused(dc)                                                         # a table, before any begin
        w = Walks(dc, k, 1)
        w.both(sub, rs)
        dc.unitigs_end()
        refused(dc)                                                         # after kh_unitigs_end
        w = Walks(dc, k, 1)
        dc.push(np.frombuffer(b"ACGTTGCAAGGCTTAACCGATAGGA", dtype=np.uint8))
        refused(dc)                                                         # after a push
        w = Walks(dc, k, 1)
        w.both(sub, rs)


def test_bad_arguments_leave_the_context_usable():
    import torch
    k = 21
    recs, flat = L.branchy()
    sub = flat[:1000].copy()
    rs = np.array([0, 400, 1000, 0], dtype=U64)
    lib = native.lib()
    st, rows, cov = np.full(8, CANARY, dtype=U64), np.full(4000, CANARY32, dtype=U32), np.full(8000, CANARY, dtype=U64)
    t_in, t_rs = torch.from_numpy(sub).cuda(), torch.from_numpy(rs.view(np.int64)).cuda()
    t_st, t_rows, t_cov = (torch.from_numpy(x.view(np.int64 if x.dtype == U64 else np.int32)).cuda() for x in (st, rows, cov))
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        w = Walks(dc, k, 1)
        total = C.c_uint64(0)
        n = sub.size
        for f, b_, r_, s_, w_, c_ in ((lib.kh_unitigs_paths, sub.ctypes.data, rs.ctypes.data, st.ctypes.data, rows.ctypes.data, cov.ctypes.data),
                                      (lib.kh_unitigs_paths_device, t_in.data_ptr(), t_rs.data_ptr(), t_st.data_ptr(), t_rows.data_ptr(), t_cov.data_ptr())):
            good = (dc._h, b_, None, n, r_, 2, s_, w_, 1000, c_, C.byref(total))

            def with_(**kw):
                names = ("ctx", "bases", "qual", "n", "rec", "nrec", "run_start", "runs", "cap", "cover", "total")
                return f(*[kw.get(name, v) for name, v in zip(names, good)])
            assert with_(ctx=None) == BAD_ARG
            assert with_(total=None) == BAD_ARG
            assert with_(bases=None) == BAD_ARG
            assert with_(rec=None) == BAD_ARG and with_(run_start=None) == BAD_ARG
            assert with_(runs=None) == BAD_ARG
            assert with_(runs=w_ + 2) == BAD_ARG and b"4-byte" in lib.kh_last_error(dc._h)
            assert with_(rec=r_ + 4) == BAD_ARG and with_(run_start=s_ + 4) == BAD_ARG and with_(cover=c_ + 4) == BAD_ARG
            assert b"8-byte" in lib.kh_last_error(dc._h)
            assert with_(bases=None, n=0, nrec=0) == OK and total.value == 0   # NULL bases with n == 0 is no error
        bad = lib.kh_unitigs_paths                                          # the host form checks the offsets too
        args = lambda r, nrec: (dc._h, sub.ctypes.data, None, n, r.ctypes.data, nrec, st.ctypes.data, rows.ctypes.data, 1000, cov.ctypes.data, C.byref(total))
        assert bad(*args(rs, 3)) == BAD_ARG and b"ascending" in lib.kh_last_error(dc._h)
        assert bad(*args(np.array([0, 400, 1001], dtype=U64), 2)) == BAD_ARG and b"beyond n" in lib.kh_last_error(dc._h)
        assert (rows == U32(CANARY32)).all() and (cov == U64(CANARY)).all() and (t_rows.cpu().numpy().view(U32) == U32(CANARY32)).all()
        w.both(sub, rs[:3])                                                 # usable, and the unitigs are still live


def test_a_record_of_2_32_window_starts_is_refused_by_the_host_form():
    """Only the offsets are looked at before the refusal: n may be beyond the buffer."""
    k = 21
    lib = native.lib()
    recs, flat = L.branchy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        Walks(dc, k, 1)
        rs, st, total = np.array([0, 1 << 32], dtype=U64), np.zeros(2, dtype=U64), C.c_uint64(0)
        assert lib.kh_unitigs_paths(dc._h, flat.ctypes.data, None, 1 << 33, rs.ctypes.data, 1, st.ctypes.data, None, 0, None, C.byref(total)) == BAD_ARG
        assert b"2^32" in lib.kh_last_error(dc._h)


# ---- readers, streams and the place map ---------------------------------------------------------------------------------------------------------
def test_readers_between_two_calls_change_nothing():
    k = 21
    recs, flat = L.branchy()
    sub = flat[:6041].copy()
    rs = per_read(sub)
    with native.DeviceCounter(k, capacity_hint=3_000_000, path="partition") as dc:
        dc.push(flat)
        before = T.stats_of(dc)
        text = b"".join(bytes(p) for p in dc.result_text("tsv", 1))
        w = Walks(dc, k, 1)
        words, want = w.both(sub, rs)
        dc.lookup(np.arange(10, dtype=U64))
        dc.histogram()
        dc.graph_stats(1)
        dc.profile(sub)
        rows, bases = dc.unitigs_copy(w.g.rows.shape[0], w.g.bases.size)
        assert np.array_equal(rows, w.g.rows) and np.array_equal(dc.unitigs_links_copy(w.g.links.size), w.g.links)
        assert np.array_equal(L.locate_device(dc, sub), words)
        w.same(paths_device(dc, w.nu, sub, rs), want, "device, after the readers")
        # a whole kh_result_text_* stream with a call between two of its pieces
        n_rec, n_bytes = C.c_uint64(0), C.c_uint64(0)
        lib = native.lib()
        assert lib.kh_result_text_begin(dc._h, native.KH_OUT_TSV, 1, C.byref(n_rec), C.byref(n_bytes)) == OK
        buf, out, n = np.empty(1 << 16, dtype=np.uint8), bytearray(), C.c_uint64(1)
        while n.value:
            assert lib.kh_result_text_next(dc._h, buf.ctypes.data, buf.size, C.byref(n)) == OK
            out += buf[:n.value].tobytes()
            if len(out) < 1 << 18:
                w.same(paths_host(dc, w.nu, sub, rs), want, "host, inside a result text stream")
        assert bytes(out) == text
        # a kh_unitigs_text_* stream goes on across a call
        total = dc.unitigs_text_begin("gfa")
        doc, piece = bytearray(), np.empty(1000, dtype=np.uint8)
        while True:
            m = dc.unitigs_text_next(piece)
            if m == 0:
                break
            doc += piece[:m].tobytes()
            if len(doc) < 4000:
                w.same(paths_device(dc, w.nu, sub, rs), want, "device, inside a unitig text stream")
                w.same(paths_host(dc, w.nu, sub, rs), want, "host, inside a unitig text stream")
        assert len(doc) == total
        whole = bytearray()
        dc.unitigs_text_begin("gfa")
        while True:
            m = dc.unitigs_text_next(piece)
            if m == 0:
                break
            whole += piece[:m].tobytes()
        assert doc == whole
        assert T.stats_of(dc) == before


def test_one_place_map_for_locate_and_paths(tr):  # noqa: F811
    import torch
    k = 21
    recs, flat = L.branchy()
    sub = flat[:5000].copy()
    rs = np.array([0, 2500, 5000], dtype=U64)
    t_in = torch.from_numpy(sub).cuda()
    t_rs = torch.from_numpy(rs.view(np.int64)).cuda()
    t_out = torch.zeros(sub.size, dtype=torch.int64, device="cuda")
    t_st = torch.zeros(3, dtype=torch.int64, device="cuda")
    t_rows = torch.zeros(4 * 5000, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        slots = dc.finish()["table_slots"]
        maps = lambda ev: [e for e in ev if e[0] == "A" and e[1] == "dev" and int(e[3]) == 8 * slots]
        dc.unitigs_begin_linked(1)
        tr.sync()
        live = tr.snapshot()
        assert dc.unitigs_paths_device(t_in, None, sub.size, t_rs, 2, t_st, t_rows, 5000)[0] == OK    # the first call builds the map
        built = maps(tr.sync())
        assert len(built) == 1
        new = {p: v for p, v in tr.snapshot().items() if p not in live}
        assert list(new) == [built[0][2]], new                              # ... and nothing else of the call stays
        dc.unitigs_locate_device(t_in, None, sub.size, t_out)               # a later locate call finds it built and allocates nothing
        assert tr.sync() == []
        assert dc.unitigs_paths_device(t_in, None, sub.size, t_rs, 2, t_st, t_rows, 5000)[0] == OK
        ev = tr.sync()
        assert maps(ev) == [] and {p: v for p, v in tr.snapshot().items() if p not in live} == new      # its scratch came and went
        dc.unitigs_begin(2)                                                 # the other way round: locate builds, paths finds
        assert built[0][2] not in tr.snapshot()
        tr.sync()
        dc.unitigs_locate_device(t_in, None, sub.size, t_out)
        assert len(maps(tr.sync())) == 1
        assert dc.unitigs_paths_device(t_in, None, sub.size, t_rs, 2, t_st, t_rows, 5000)[0] == OK
        assert maps(tr.sync()) == []
        dc.unitigs_end()


# ---- grid stride and the product library: one process each ----------------------------------------------------------------------------------
CHILD = r"""
import sys, os
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from krust_amd import native
import test_gpu_locate as L, test_gpu_paths as P
k = 21
recs, flat = L.branchy()
rng = np.random.default_rng(31)
with native.DeviceCounter(k, capacity_hint=200_000) as dc:
    dc.push(flat)
    w = P.Walks(dc, k, 1)
    w.both(flat, P.per_read(flat))
    w.both(flat, P.random_cuts(rng, flat.size, 2000))
long_rec = L.rand_letters(rng, 10_000)
with native.DeviceCounter(k, capacity_hint=100_000) as dc:
    dc.push(long_rec)
    w = P.Walks(dc, k, 1)
    w.both(long_rec, [0, 4095, 4096, 4097, long_rec.size])
print("RESULT ok", native.LIB_PATH)
"""


def run_child(env):
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride(cap):
    """KMERHIP_GRID_CAP (test build), one value per process: one and three workgroups go round every kernel's loop many times."""
    run_child(dict(os.environ, KMERHIP_GRID_CAP=str(cap)))


def test_product_library_once():
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    env.pop("KMERHIP_GRID_CAP", None)
    assert "libkmerhip.so" in run_child(env)
