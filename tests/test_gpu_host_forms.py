"""The four host forms of the read side -- kh_profile, kh_profile_records, kh_unitigs_locate, kh_unitigs_paths -- walk their input
through ONE chunk pipeline (chunk_pipeline, krust_amd/csrc/profile.hip).  What that pipeline decides is pinned here for all four at
once, in chunks of 1024 window starts (KMERHIP_PROFILE_CHUNK_KB=1, test build): the input lengths at which the chunk arithmetic can
go wrong, pageable and pinned memory on either side, and the shared buffers growing between calls of one context.

Every host form must equal its device form on the same bytes exactly -- the device forms run before the chunk size is set: one
launch, no chunks -- and both are held to the Python references the forms' own tests use: profile_expect.py (the profile and the
rows of kh_profile_records), test_locate_ref.locate_ref and test_paths_ref.paths_ref.  No tolerance, no case left out.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import profile_expect as E
import test_gpu_locate as L
import test_gpu_paths as PA
import test_gpu_profile as TP
import test_gpu_profile_records as TR
import test_paths_ref as P
from krust_amd import native

pytestmark = pytest.mark.gpu

K, MINQ, CH = 21, 10, 1024
N_TABLE = 20_000
LO, HI = 2, E.SAT                       # (lo = 2: the reads carry substitutions, so first_low is set in many rows)
U64, U32 = np.uint64, np.uint32
# a last chunk of one window start, one shorter than k - 1, a window that straddles the chunk edge exactly, the halo of paths at the
# first and at the last chunk
LENGTHS = [1, K - 1, K, CH - 1, CH, CH + 1, CH + K - 2, CH + K - 1, 2 * CH, 2 * CH + 1, N_TABLE]


def rec_start_for(n):
    """A record over three chunk edges, several records inside one chunk, an empty record at a chunk edge; clipped to n, which leaves
    empty records and records that end with the buffer at the small lengths."""
    rs = np.array([0, 500, 500 + 3 * CH + 100, 3700, 3800, 3900, 4000, 4 * CH, 4 * CH, 5000, n], dtype=np.int64)
    return np.minimum(rs, n).astype(U64)


class World:
    """One table of N_TABLE bytes of reads, its live unitigs, and the references' answers for a prefix of those reads."""

    def __init__(self, dc):
        recs, flat = L.branchy()
        self.dc, self.flat = dc, flat[:N_TABLE].copy()
        rng = np.random.default_rng(41)
        self.qual = (33 + rng.integers(MINQ, 41, size=N_TABLE)).astype(np.uint8)
        self.qual[rng.random(N_TABLE) < 0.01] = 33 + MINQ - 1    # one base in a hundred below the threshold: four windows in five stay
        dc.push(self.flat)
        self.m = O.count_records(bytes(self.flat).split(b"N"), K)
        self.keys, self.counts = self.m.arrays()
        for q in (None, self.qual):       # the numpy twin against the oracle's primitives, once per quality setting
            E.check_twin(self.flat, K, self.m, self.keys, self.counts, q, None if q is None else MINQ)
        self.w = PA.Walks(dc, K, 1)
        self.nu = self.w.nu

    def inputs(self, n, with_qual):
        return self.flat[:n].copy(), (self.qual[:n].copy() if with_qual else None), rec_start_for(n)

    def want(self, sub, qual, rs):
        prof = E.np_profile(sub, K, self.keys, self.counts, qual, None if qual is None else MINQ)
        words, paths = self.w.want(sub, rs, qual)
        return prof, E.rows_of(prof, rs, LO, HI), words, paths

    def device(self, sub, qual, rs):
        return (TP.dev_profile(self.dc, sub, qual), TR.dev_rows(self.dc, sub, rs, qual, LO, HI), L.locate_device(self.dc, sub, qual),
                PA.paths_device(self.dc, self.nu, sub, rs, qual))

    def host(self, sub, qual, rs):
        return (self.dc.profile(sub, qual).copy(), self.dc.profile_records(sub, rs, qual, lo=LO, hi=HI).copy(), L.locate_host(self.dc, sub, qual),
                PA.paths_host(self.dc, self.nu, sub, rs, qual))

    def check(self, got, want, who):
        prof, rows, words, paths = want
        assert np.array_equal(got[0], prof), (who, "profile", np.flatnonzero(got[0] != prof)[:5])
        assert np.array_equal(got[1], rows), (who, "rows", np.flatnonzero((got[1] != rows).any(axis=1))[:5])
        assert np.array_equal(got[2], words), (who, "words", np.flatnonzero(got[2] != words)[:5])
        self.w.same(got[3], paths, who)


def same_paths(a, b):
    return (a.rc == b.rc and a.total == b.total and np.array_equal(a.run_start, b.run_start) and np.array_equal(a.rows, b.rows) and
            np.array_equal(a.cover, b.cover))


@pytest.fixture(scope="module")
def world():
    with native.DeviceCounter(K, min_quality=MINQ, capacity_hint=200_000) as dc:
        yield World(dc)


# ---- the edges of the chunk arithmetic ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_qual", [False, True], ids=["plain", "qual"])
@pytest.mark.parametrize("n", LENGTHS)
def test_host_forms_equal_device_forms_at_chunk_edges(world, n, with_qual, monkeypatch):
    sub, qual, rs = world.inputs(n, with_qual)
    dev = world.device(sub, qual, rs)                            # one launch each: no chunks
    monkeypatch.setenv("KMERHIP_PROFILE_CHUNK_KB", "1")
    host = world.host(sub, qual, rs)
    monkeypatch.delenv("KMERHIP_PROFILE_CHUNK_KB")
    for i, name in enumerate(("profile", "rows", "words")):
        assert np.array_equal(host[i], dev[i]), (name, n, np.flatnonzero((host[i] != dev[i]).reshape(host[i].shape[0], -1).any(axis=1))[:5])
    assert same_paths(host[3], dev[3]), ("paths", n, host[3].total, dev[3].total)
    want = world.want(sub, qual, rs)                             # the references: every form at every n
    world.check(dev, want, "device, n=%d" % n)
    world.check(host, want, "host, n=%d" % n)
    if n == N_TABLE:
        assert (want[0] != E.NO).sum() > n // 2 and want[3][1].shape[0] > 100 and (want[1][:, E.WINDOWS] > 0).sum() >= 8   # (not vacuous)


# ---- pageable and pinned memory on either side --------------------------------------------------------------------------------------------------
def paths_host_into(dc, sub, qual, rs, st, runs, cov):
    """kh_unitigs_paths into the caller's three arrays (cov zeroed first); returns copies of what it wrote."""
    total = C.c_uint64(0)
    cov[:] = 0
    rc = native.lib().kh_unitigs_paths(dc._h, sub.ctypes.data, None if qual is None else qual.ctypes.data, sub.size, rs.ctypes.data, rs.size - 1,
                                       st.ctypes.data, runs.ctypes.data, runs.size // native.RUN_WORDS, cov.ctypes.data, C.byref(total))
    assert rc == native.KH_OK, native.lib().kh_last_error(dc._h)
    return st.copy(), runs[:native.RUN_WORDS * total.value].reshape(-1, native.RUN_WORDS).copy(), cov.reshape(-1, native.COV_WORDS).copy()


@pytest.mark.parametrize("pin_out", [False, True], ids=["out-pageable", "out-pinned"])
@pytest.mark.parametrize("pin_in", [False, True], ids=["in-pageable", "in-pinned"])
def test_pageable_and_pinned_memory(world, pin_in, pin_out, monkeypatch):
    n = 2 * CH + 1
    dc = world.dc
    for with_qual in (False, True):
        sub, qual, rs = world.inputs(n, with_qual)
        nrec = rs.size - 1
        prof, rows, words, (run_start, runs, cover) = world.want(sub, qual, rs)
        cap = runs.shape[0] + 3
        sizes = [(n, np.uint8), (n, np.uint8), (n, U32), (nrec * native.REC_WORDS, U32), (n, U64), (nrec + 1, U64), (cap * native.RUN_WORDS, U32),
                 (world.nu * native.COV_WORDS, U64)]
        pins = [native.PinnedArray(m, dtype=t) for m, t in sizes]
        try:
            pb, pq = (pins[0].array, pins[1].array) if pin_in else (np.empty(n, np.uint8), np.empty(n, np.uint8))
            outs = [p.array for p in pins[2:]] if pin_out else [np.empty(m, dtype=t) for m, t in sizes[2:]]
            pb[:] = sub
            if with_qual:
                pq[:] = qual
            q = pq if with_qual else None
            for o in outs:
                o[:] = 0x5A
            monkeypatch.setenv("KMERHIP_PROFILE_CHUNK_KB", "1")
            got_prof = dc.profile(pb, q, out=outs[0])
            got_rows = dc.profile_records(pb, rs, q, lo=LO, hi=HI, out=outs[1])
            got_words = dc.unitigs_locate(pb, q, out=outs[2])
            got_st, got_runs, got_cov = paths_host_into(dc, pb, q, rs, outs[3], outs[4], outs[5])
            monkeypatch.delenv("KMERHIP_PROFILE_CHUNK_KB")
            assert np.array_equal(got_prof, prof) and np.array_equal(got_rows, rows) and np.array_equal(got_words, words)
            assert np.array_equal(got_st, run_start) and np.array_equal(got_runs, runs) and np.array_equal(got_cov, cover)
        finally:
            for p in pins:
                p.close()


# ---- one context: the shared buffers grow between the calls ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["forward", "reverse"])
def test_one_context_all_four_forms_in_turn(order, monkeypatch):
    """profile -> locate -> paths -> records -> profile on a fresh context: the chunk buffers are allocated for 4 bytes per window
    start, grow to 8 for locate, to chunk + 4 window starts for paths, and serve the two profile forms as they are; in reverse order
    the first call allocates the largest and the rest fit."""
    n = 5 * CH + 77
    with native.DeviceCounter(K, min_quality=MINQ, capacity_hint=200_000) as dc:
        wd = World(dc)
        sub, qual, rs = wd.inputs(n, True)
        prof, rows, words, paths = wd.want(sub, qual, rs)
        steps = [("profile", lambda: np.array_equal(dc.profile(sub, qual), prof)),
                 ("locate", lambda: np.array_equal(L.locate_host(dc, sub, qual), words)),
                 ("paths", lambda: wd.w.same(PA.paths_host(dc, wd.nu, sub, rs, qual), paths, "host") is None),
                 ("records", lambda: np.array_equal(dc.profile_records(sub, rs, qual, lo=LO, hi=HI), rows)),
                 ("profile", lambda: np.array_equal(dc.profile(sub, qual), prof))]
        monkeypatch.setenv("KMERHIP_PROFILE_CHUNK_KB", "1")
        for name, step in (steps if order == "forward" else steps[::-1]):
            assert step(), (order, name)
        monkeypatch.delenv("KMERHIP_PROFILE_CHUNK_KB")
        wd.check(wd.host(sub, qual, rs), (prof, rows, words, paths), "one chunk, afterwards")
