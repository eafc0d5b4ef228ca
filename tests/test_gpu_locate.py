"""kh_unitigs_locate* -- the k-mers of new sequences located on the live unitigs -- against the reference in Python strings of
tests/test_locate_ref.py: a dict from every window string of the unitigs that kh_unitigs_copy returns (held to the string walk by
tests/test_gpu_unitigs.py) and of their reverse complements to (unitig, offset, sign), looked up for every window of the input.

Every case checks every output word exactly, with canaries on both sides of the output, and on top of that what needs no reference:
a word is a place iff kh_profile says count >= min_count on the same buffers, KH_LOC_NO_WINDOW iff it says KH_PROFILE_NO_WINDOW, and
two consecutive places are neighbours in one unitig or the two ends of a link word of kh_unitigs_links_copy.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import test_gpu_graph as G
import test_gpu_join as T
import test_gpu_unitigs as U
import test_locate_ref as R
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
MESSY = np.frombuffer(b"ACGTACGTACGTacgtN", dtype=np.uint8)
CANARY = 0xABABABABABABABAB
NO_WINDOW, ABSENT = native.LOC_NO_WINDOW, native.LOC_ABSENT
OK, STATE, BAD_ARG = native.KH_OK, native.KH_ERR_STATE, native.KH_ERR_BAD_ARG
TILE = 4096


# ---- the calls, between canaries -----------------------------------------------------------------------------------------------------------
def locate_device(dc, flat, qual=None, boff=0, ooff=0, qoff=0):
    """kh_unitigs_locate_device with d_bases at byte boff (mod 16), d_qual at qoff and d_out at 8 * ooff behind 16-byte boundaries."""
    import torch
    n = int(flat.size)
    hb = np.full(n + 64, ord("A"), dtype=np.uint8)            # (valid bases all round: only [boff, boff + n) may be read as data)
    hb[16 + boff:16 + boff + n] = flat
    tb = torch.from_numpy(hb).cuda()
    tq = None
    if qual is not None:
        hq = np.full(n + 64, ord("I"), dtype=np.uint8)
        hq[16 + qoff:16 + qoff + n] = qual
        tq = torch.from_numpy(hq).cuda()
    to = torch.from_numpy(np.full(n + 8, CANARY, dtype=U64).view(np.int64)).cuda()
    torch.cuda.synchronize()
    assert tb.data_ptr() % 16 == 0 and to.data_ptr() % 16 == 0
    lo = 2 + ooff
    dc.unitigs_locate_device(tb.data_ptr() + 16 + boff, None if tq is None else tq.data_ptr() + 16 + qoff, n, to.data_ptr() + 8 * lo)
    host = to.cpu().numpy().view(U64)
    assert (host[:lo] == U64(CANARY)).all() and (host[lo + n:] == U64(CANARY)).all(), "kh_unitigs_locate_device wrote outside d_out"
    return host[lo:lo + n].copy()


def locate_host(dc, flat, qual=None, out=None):
    n = int(flat.size)
    arr = np.full(n + 8, CANARY, dtype=U64) if out is None else out
    arr[:] = U64(CANARY)
    got = dc.unitigs_locate(flat, qual, out=arr[4:4 + n])
    assert (arr[:4] == U64(CANARY)).all() and (arr[4 + n:] == U64(CANARY)).all(), "kh_unitigs_locate wrote outside out"
    return got.copy()


class Graph:
    """The live unitigs of dc at mc (linked), their copies and the reference's dict."""

    def __init__(self, dc, k, mc=1):
        self.dc, self.k, self.mc = dc, k, max(mc, 1)
        nu, nb, nl = dc.unitigs_begin_linked(mc)
        self.rows, self.bases = dc.unitigs_copy(nu, nb)
        self.links = dc.unitigs_links_copy(nl)
        self.places = R.place_dict(self.rows, self.bases, k)

    def want(self, flat, qual=None):
        return R.locate_ref(self.rows, self.bases, self.k, flat.tobytes(), None if qual is None else qual.tobytes(), self.dc.min_quality,
                            places=self.places)

    def check(self, got, flat, qual=None):
        """Every word against the reference; then the profile cross-check and the walk property.  Returns the link crossings."""
        want = self.want(flat, qual)
        assert got.dtype == U64 and got.shape == want.shape
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            raise AssertionError("k=%d: %d of %d words differ, first at %d (tile %d + %d): %r for %r, window %r" %
                                 (self.k, int(np.sum(got != want)), got.size, i, i // TILE, i % TILE, R.fields(got[i:i + 1]), R.fields(want[i:i + 1]),
                                  flat[i:i + self.k].tobytes()))
        prof = self.dc.profile(flat, qual)
        assert np.array_equal(got == U64(NO_WINDOW), prof == native.PROFILE_NO_WINDOW)
        assert np.array_equal(native.loc_is_place(got), (prof != native.PROFILE_NO_WINDOW) & (prof >= self.mc))
        return R.check_walk(got, self.rows, self.links, self.k)

    def both(self, flat, qual=None, **kw):
        """The device form and the host form on one buffer."""
        c = self.check(locate_device(self.dc, flat, qual, **kw), flat, qual)
        assert self.check(locate_host(self.dc, flat, qual), flat, qual) == c
        return c


def rand_letters(rng, n, alphabet=ACGT):
    return alphabet[rng.integers(0, alphabet.size, size=n)]


def mutated_reads(seed, genome_len, n_reads, read_len=150, rate=0.01):
    """Reads of a random genome, half of them reverse complements, with substitutions: branches, tips and bubbles in the graph."""
    rng = np.random.default_rng(seed)
    genome = rand_letters(rng, genome_len).tobytes()
    recs = []
    for i in range(n_reads):
        a = int(rng.integers(0, genome_len - read_len))
        r = bytearray(genome[a:a + read_len])
        for p in np.flatnonzero(rng.random(read_len) < rate):
            r[p] = b"ACGT"[int(rng.integers(0, 4))]
        recs.append(U.rc(bytes(r)) if i % 2 else bytes(r))
    return recs


_BRANCHY = {}


def branchy():
    """600 reads of 150 over a genome of 2^12: every base covered twenty times, one substitution per read."""
    if not _BRANCHY:
        recs = mutated_reads(11, 1 << 12, 600)
        _BRANCHY["recs"], _BRANCHY["flat"] = recs, U.flat_of(recs)
    return _BRANCHY["recs"], _BRANCHY["flat"]


# ---- dense small k: palindromes, loops, hairpins, unitigs of one node ------------------------------------------------------------------------
@pytest.mark.parametrize("alphabet", ["acgt", "messy"])
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5])
def test_small_k_dense(k, alphabet):
    rng = np.random.default_rng(300 + k)
    letters = ACGT if alphabet == "acgt" else MESSY
    table_in = rand_letters(rng, 200 if k < 5 else 600, letters)      # (k = 5: about half of the 512 canonical keys)
    query = rand_letters(rng, 3000, letters)
    with native.DeviceCounter(k) as dc:
        dc.push(table_in)
        for mc in (1, 2):
            g = Graph(dc, k, mc)
            assert g.rows.shape[0] > 0
            g.both(table_in)
            crossed = g.both(query)
            assert crossed > 0 or k == 1
            if k in (2, 4):
                pal = [w for w in g.places if U.rc(w) == w]
                assert pal, "no palindrome among the nodes"
                for w in pal:                                   # a palindrome is + whichever way it is read
                    f = R.fields(locate_device(dc, np.frombuffer(w + b"N" + U.rc(w), dtype=np.uint8)))
                    assert f[0] == f[k + 1] and f[0][1] == 0


# ---- reads with branches ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [11, 21, 31, 32])
def test_reads_with_branches(k):
    recs, flat = branchy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        for mc in (1, 2):
            g = Graph(dc, k, mc)
            crossed = g.both(flat)
            places = int(np.sum(native.loc_is_place(g.want(flat))))
            if mc == 1:
                assert g.rows.shape[0] > 100 and crossed > places // 100, (g.rows.shape[0], crossed, places)   # the reads walk over many links


def test_reverse_complement_property_per_record():
    k = 21
    recs, flat = branchy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        Graph(dc, k, 2)
        sub = recs[:200]
        fwd = locate_device(dc, U.flat_of(sub))
        rev = locate_device(dc, U.flat_of([U.rc(r) for r in sub]))
        at, some = 1, 0
        for r in sub:
            m = len(r)
            a, b = fwd[at:at + m - k + 1], rev[at:at + m - k + 1][::-1]
            place = native.loc_is_place(a)
            assert np.array_equal(place, native.loc_is_place(b)) and np.array_equal(a[~place], b[~place])
            ua, sa, ja = native.loc_unpack(a[place])
            ub, sb, jb = native.loc_unpack(b[place])
            assert np.array_equal(ua, ub) and np.array_equal(ja, jb) and np.array_equal(sa, 1 - sb)    # (k odd: no palindrome)
            some += int(place.sum())
            at += m + 1
        assert some > 10_000
    k = 4                                                       # even k: a palindrome is + both times
    rng = np.random.default_rng(5)
    r = rand_letters(rng, 400).tobytes()
    with native.DeviceCounter(k) as dc:
        dc.push(np.frombuffer(r, dtype=np.uint8))
        g = Graph(dc, k, 1)
        a = locate_device(dc, np.frombuffer(r, dtype=np.uint8))[:len(r) - k + 1]
        b = locate_device(dc, np.frombuffer(U.rc(r), dtype=np.uint8))[:len(r) - k + 1][::-1]
        pal = np.array([U.rc(r[i:i + k]) == r[i:i + k] for i in range(len(r) - k + 1)])
        assert pal.any() and native.loc_is_place(a).all()
        assert np.array_equal(a[pal], b[pal]) and np.array_equal(a[~pal] ^ U64(1 << 32), b[~pal])


# ---- total lengths: the tile's edges and the k - 1 results that belong to the tile before ----------------------------------------------------
def test_total_input_lengths():
    k = 21
    recs, flat = branchy()
    lengths = [0, 1, k - 1, k, k + 1, TILE - 1, TILE, TILE + 1, TILE + k - 1, 3 * TILE + 5]
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        g = Graph(dc, k, 1)
        for n in lengths:
            for start in (1, 70):                               # a read edge at the front, and the middle of a read
                g.both(flat[start:start + n].copy())


# ---- alignment ------------------------------------------------------------------------------------------------------------------------------------
def test_alignment_of_bases_qualities_and_output():
    k = 21
    recs, flat = branchy()
    rng = np.random.default_rng(9)
    sub = flat[:2 * TILE + 77].copy()
    qual = (33 + rng.integers(2, 41, size=sub.size)).astype(np.uint8)
    with native.DeviceCounter(k, min_quality=10, capacity_hint=200_000) as dc:
        dc.push(flat)
        g = Graph(dc, k, 1)
        for boff in (0, 1, 7, 15):
            for ooff in (0, 1):
                g.check(locate_device(dc, sub, None, boff=boff, ooff=ooff), sub)
                for qoff in (boff, (boff + 5) % 16):            # d_qual aligned with the bases' 16-byte units, and not
                    g.check(locate_device(dc, sub, qual, boff=boff, ooff=ooff, qoff=qoff), sub, qual)


# ---- quality masking ----------------------------------------------------------------------------------------------------------------------------
def test_quality_masking():
    k = 21
    recs, flat = branchy()
    rng = np.random.default_rng(10)
    qual = (33 + rng.integers(15, 41, size=flat.size)).astype(np.uint8)
    with native.DeviceCounter(k, min_quality=20, capacity_hint=200_000) as dc:
        dc.push(flat, qual)
        g = Graph(dc, k, 1)
        got = locate_device(dc, flat, qual)
        g.check(got, flat, qual)                                # (the no-window positions are those of kh_profile on the same buffers)
        g.check(locate_host(dc, flat, qual), flat, qual)
        plain = locate_device(dc, flat, None)
        g.check(plain, flat, None)
        masked = int(np.sum(got == U64(NO_WINDOW))) - int(np.sum(plain == U64(NO_WINDOW)))
        assert masked > 1000                                    # the threshold masks windows that the letters alone allow


# ---- circular unitigs -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [21, 31])
def test_circular_unitigs(k):
    flat, keys, counts = U.cycle_input(k)
    records = flat.tobytes().strip(b"N").split(b"N")
    with native.DeviceCounter(k, capacity_hint=100_000) as dc:
        dc.push(flat)
        g = Graph(dc, k, 1)
        circular = {u: int(r[native.UNI_KMERS]) for u, r in enumerate(g.rows) if int(r[native.UNI_FLAGS]) & native.UNI_CIRCULAR}
        assert set(U.PERIODS) <= set(circular.values())
        g.both(flat)
        for i, p in enumerate(U.PERIODS):
            unit = records[2 * i][:p]
            read = (unit * (k // p + 4))[:(5 * p) // 2 + k - 1]  # two and a half times round
            for r in (read, U.rc(read)):
                buf = np.frombuffer(r, dtype=np.uint8)
                got = locate_device(dc, buf)
                assert g.check(got, buf) >= 2                   # the closing link, at least twice
                u, s, j = native.loc_unpack(got[:len(r) - k + 1])
                assert native.loc_is_place(got[:len(r) - k + 1]).all() and len(set(u.tolist())) == 1 and circular[int(u[0])] == p
                assert len(set(s.tolist())) == 1
                step = np.diff(j.astype(np.int64))
                assert np.array_equal(np.unique(step), np.array(sorted({1 - p, 1}) if int(s[0]) == 0 else sorted({-1, p - 1})))   # L-1 -> 0 / 0 -> L-1


# ---- the index kernel: one long unitig, and many of one node -------------------------------------------------------------------------------
def test_long_chain_beside_many_unitigs_of_one_node():
    k = 21
    flat, keys, counts = U.chain_input(k)
    rng = np.random.default_rng(12)
    singles = [rand_letters(rng, k).tobytes() for _ in range(6000)]
    both = np.concatenate((flat, U.flat_of(singles)))
    with native.DeviceCounter(k, capacity_hint=400_000) as dc:
        dc.push(both)
        g = Graph(dc, k, 1)
        L = g.rows[:, native.UNI_KMERS]
        assert int(L.max()) >= 10_000 and int(np.sum(L == 1)) >= 5000
        g.check(locate_device(dc, both), both)
        long_read = flat[:30_000].copy()
        g.check(locate_host(dc, long_read), long_read)


# ---- min_count 1 and 3 on the same table: the index is rebuilt ---------------------------------------------------------------------------------
def test_min_count_1_and_3_on_the_same_table():
    k = 21
    recs, flat = branchy()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        prof = dc.profile(flat)
        words = {}
        for mc in (1, 3, 1):
            g = Graph(dc, k, mc)
            words[mc] = locate_device(dc, flat)
            g.check(words[mc], flat)
            g.check(locate_host(dc, flat), flat)
        between = (prof != native.PROFILE_NO_WINDOW) & (prof >= 1) & (prof < 3)
        assert between.sum() > 100 and (words[3][between] == U64(ABSENT)).all() and native.loc_is_place(words[1][between]).all()
        both = native.loc_is_place(words[3])
        assert (native.loc_unpack(words[1][both])[0] != native.loc_unpack(words[3][both])[0]).any()   # the unitigs are numbered anew


# ---- table forms ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["wide", "image", "regions3072", "grown"])
def test_table_forms(form, monkeypatch):
    k = 21
    flat, keys, counts = G.main_input(k)
    sub = flat[:20 * 151].copy()
    with T.table(form, k, flat, monkeypatch) as dc:
        before = T.stats_of(dc)
        g = Graph(dc, k, 1)
        assert g.both(sub) > 0
        assert T.stats_of(dc) == before


# ---- grid stride and the product library: one process each ----------------------------------------------------------------------------------
CHILD = r"""
import sys, os
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
from krust_amd import native
import test_gpu_locate as L, test_gpu_unitigs as U
k = 21
recs, flat = L.branchy()
for path in ("partition", "direct"):
    with native.DeviceCounter(k, capacity_hint=3_000_000, path=path) as dc:
        dc.push(flat)
        assert dc.finish()["slot_bytes"] == (8 if path == "partition" else 16)
        g = L.Graph(dc, k, 1)
        assert g.both(flat) > 0
cflat = U.chain_input(k)[0]
with native.DeviceCounter(k, capacity_hint=100_000) as dc:
    dc.push(cflat)
    g = L.Graph(dc, k, 1)
    g.check(L.locate_device(dc, cflat), cflat)
print("RESULT ok", native.LIB_PATH)
"""


def run_child(env):
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    return p.stdout


@pytest.mark.parametrize("cap", [1, 3])
def test_grid_stride(cap):
    """KMERHIP_GRID_CAP (test build), one value per process: one and three workgroups go round both kernels' loops many times."""
    run_child(dict(os.environ, KMERHIP_GRID_CAP=str(cap)))


def test_product_library_once():
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    env.pop("KMERHIP_GRID_CAP", None)
    assert "libkmerhip.so" in run_child(env)


# ---- the host form in chunks of 1024 window starts ---------------------------------------------------------------------------------------------
def test_host_form_in_small_chunks(monkeypatch):
    k = 21
    recs, flat = branchy()
    sub = flat[:20_000].copy()
    rng = np.random.default_rng(13)
    qual = (33 + rng.integers(5, 41, size=sub.size)).astype(np.uint8)
    with native.DeviceCounter(k, min_quality=10, capacity_hint=200_000) as dc:
        dc.push(flat)
        g = Graph(dc, k, 1)
        whole = locate_host(dc, sub, qual)
        monkeypatch.setenv("KMERHIP_PROFILE_CHUNK_KB", "1")
        got = locate_host(dc, sub, qual)                         # pageable memory
        monkeypatch.delenv("KMERHIP_PROFILE_CHUNK_KB")
        g.check(got, sub, qual)
        assert np.array_equal(got, whole)
        with native.PinnedArray(sub.size) as pb, native.PinnedArray(sub.size) as pq, native.PinnedArray(sub.size + 8, dtype=U64) as po:
            pb.array[:] = sub
            pq.array[:] = qual
            monkeypatch.setenv("KMERHIP_PROFILE_CHUNK_KB", "1")
            got = locate_host(dc, pb.array, pq.array, out=po.array)   # kh_host_alloc memory: no bounce
            monkeypatch.delenv("KMERHIP_PROFILE_CHUNK_KB")
            assert np.array_equal(got, whole)
        prof = dc.profile(sub, qual)                             # the profile shares the chunk buffers: it still does what it did
        assert np.array_equal(got == U64(NO_WINDOW), prof == native.PROFILE_NO_WINDOW)


# ---- state ------------------------------------------------------------------------------------------------------------------------------------------
def status_host(dc, flat, arr):
    return native.lib().kh_unitigs_locate(dc._h, flat.ctypes.data, None, flat.size, arr[4:].ctypes.data)


def test_state_errors_leave_the_output_untouched():
    import torch
    k = 21
    recs, flat = branchy()
    sub = flat[:1000].copy()
    L = native.lib()
    arr = np.full(sub.size + 8, CANARY, dtype=U64)
    t_in = torch.from_numpy(sub).cuda()
    t_out = torch.from_numpy(np.full(sub.size, CANARY, dtype=U64).view(np.int64)).cuda()

    def refused(dc):
        for rc in (status_host(dc, sub, arr), L.kh_unitigs_locate_device(dc._h, t_in.data_ptr(), None, sub.size, t_out.data_ptr())):
            assert rc == STATE and b"no unitigs: kh_unitigs_begin first" in L.kh_last_error(dc._h), (rc, L.kh_last_error(dc._h))
        assert (arr == U64(CANARY)).all() and (t_out.cpu().numpy().view(U64) == U64(CANARY)).all()

    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        refused(dc)                                              # an empty context, before any begin
        dc.push(flat)
        refused(dc)                                              # a table, before any begin
        g = Graph(dc, k, 1)
        g.check(locate_device(dc, sub), sub)
        dc.unitigs_end()
        refused(dc)                                              # after kh_unitigs_end
        g = Graph(dc, k, 1)
        dc.push(np.frombuffer(b"ACGTTGCAAGGCTTAACCGATAGGA", dtype=np.uint8))
        refused(dc)                                              # after a push
        g = Graph(dc, k, 1)
        g.check(locate_device(dc, sub), sub)
        dc.result_sorted(1)                                      # (may take the partition buffers: the unitigs are stale)
        refused(dc)
        g = Graph(dc, k, 1)
        dc.reset()
        refused(dc)                                              # after kh_reset
        assert dc.unitigs_begin(1) == (0, 0)                     # an empty S: only the two specials
        got = locate_device(dc, sub)
        want = np.where(R.window_starts(sub.tobytes(), k), U64(ABSENT), U64(NO_WINDOW))
        assert np.array_equal(got, want) and np.array_equal(locate_host(dc, sub), want)
    with native.DeviceCounter(k) as dc:                          # a context that never saw a push
        assert dc.unitigs_begin_linked(1) == (0, 0, 0)
        assert np.array_equal(locate_device(dc, sub), np.where(R.window_starts(sub.tobytes(), k), U64(ABSENT), U64(NO_WINDOW)))
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:  # every k-mer below min_count: an empty S over a table that holds keys
        dc.push(flat)
        assert dc.unitigs_begin(1 << 40) == (0, 0)
        assert np.array_equal(locate_device(dc, sub), np.where(R.window_starts(sub.tobytes(), k), U64(ABSENT), U64(NO_WINDOW)))


def test_bad_arguments_leave_the_context_usable():
    import torch
    k = 21
    recs, flat = branchy()
    sub = flat[:1000].copy()
    L = native.lib()
    arr = np.full(sub.size + 8, CANARY, dtype=U64)
    t_in = torch.from_numpy(sub).cuda()
    t_out = torch.zeros(sub.size + 2, dtype=torch.int64, device="cuda")
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        g = Graph(dc, k, 1)
        assert L.kh_unitigs_locate(None, sub.ctypes.data, None, sub.size, arr.ctypes.data) == BAD_ARG
        assert L.kh_unitigs_locate(dc._h, None, None, sub.size, arr.ctypes.data) == BAD_ARG
        assert L.kh_unitigs_locate(dc._h, sub.ctypes.data, None, sub.size, None) == BAD_ARG
        assert L.kh_unitigs_locate(dc._h, sub.ctypes.data, None, sub.size, arr.ctypes.data + 4) == BAD_ARG and L.kh_last_error(dc._h)
        assert L.kh_unitigs_locate_device(dc._h, None, None, sub.size, t_out.data_ptr()) == BAD_ARG
        assert L.kh_unitigs_locate_device(dc._h, t_in.data_ptr(), None, sub.size, None) == BAD_ARG
        assert L.kh_unitigs_locate_device(dc._h, t_in.data_ptr(), None, sub.size, t_out.data_ptr() + 4) == BAD_ARG
        assert (arr == U64(CANARY)).all()
        assert L.kh_unitigs_locate(dc._h, None, None, 0, None) == OK and L.kh_unitigs_locate_device(dc._h, None, None, 0, None) == OK   # n == 0
        g.both(sub)                                              # usable, and the unitigs are still live


def test_readers_between_two_locate_calls_change_nothing():
    k = 21
    recs, flat = branchy()
    sub = flat[:6000].copy()
    with native.DeviceCounter(k, capacity_hint=3_000_000, path="partition") as dc:
        dc.push(flat)
        before = T.stats_of(dc)
        text = b"".join(bytes(p) for p in dc.result_text("tsv", 1))
        g = Graph(dc, k, 1)
        first = locate_device(dc, sub)
        g.check(first, sub)
        dc.lookup(np.arange(10, dtype=U64))
        dc.histogram()
        dc.graph_stats(1)
        rows, bases = dc.unitigs_copy(g.rows.shape[0], g.bases.size)
        assert np.array_equal(rows, g.rows) and np.array_equal(dc.unitigs_links_copy(g.links.size), g.links)
        assert np.array_equal(locate_device(dc, sub), first)
        # a whole kh_result_text_* stream with a locate call between two of its pieces
        n_rec, n_bytes = C.c_uint64(0), C.c_uint64(0)
        L = native.lib()
        assert L.kh_result_text_begin(dc._h, native.KH_OUT_TSV, 1, C.byref(n_rec), C.byref(n_bytes)) == OK
        buf, out, n = np.empty(1 << 16, dtype=np.uint8), bytearray(), C.c_uint64(1)
        while n.value:
            assert L.kh_result_text_next(dc._h, buf.ctypes.data, buf.size, C.byref(n)) == OK
            out += buf[:n.value].tobytes()
            assert np.array_equal(locate_host(dc, sub[:2000].copy())[:1900], first[:1900])     # (the last k - 1 starts see the cut)
        assert bytes(out) == text
        # a kh_unitigs_text_* stream in pieces
        total = dc.unitigs_text_begin("gfa")
        doc, piece = bytearray(), np.empty(1000, dtype=np.uint8)
        while True:
            m = dc.unitigs_text_next(piece)
            if m == 0:
                break
            doc += piece[:m].tobytes()
            if len(doc) < 5000:
                assert np.array_equal(locate_device(dc, sub), first)
        assert len(doc) == total
        assert np.array_equal(locate_host(dc, sub), first)
        assert T.stats_of(dc) == before


# ---- the index's lifetime, from the allocation trace ---------------------------------------------------------------------------------------------
def test_index_lifetime(tr):  # noqa: F811
    k = 21
    recs, flat = branchy()
    sub = flat[:5000].copy()
    import torch
    t_in = torch.from_numpy(sub).cuda()
    t_out = torch.zeros(sub.size, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    with native.DeviceCounter(k, capacity_hint=200_000) as dc:
        dc.push(flat)
        slots = dc.finish()["table_slots"]
        tr.sync()
        dc.unitigs_begin(1)
        dc.unitigs_end()
        dc.unitigs_begin_linked(1)
        ev = tr.sync()
        assert not [e for e in ev if e[0] == "A" and int(e[3]) == 8 * slots], "a begin that is never located allocates no index"
        live = tr.snapshot()
        dc.unitigs_locate_device(t_in, None, sub.size, t_out)    # the first locate call: cap * 8 bytes, once
        ev = tr.sync()
        index = [e for e in ev if e[0] == "A" and e[1] == "dev" and int(e[3]) == 8 * slots]
        assert len(index) == 1, ev
        new = {p: v for p, v in tr.snapshot().items() if p not in live}
        assert list(new) == [index[0][2]], new                   # ... and nothing else stays
        dc.unitigs_locate_device(t_in, None, sub.size, t_out)    # later calls allocate nothing
        assert tr.sync() == []
        dc.unitigs_begin(2)                                      # the next begin releases it ...
        assert index[0][2] not in tr.snapshot()
        dc.unitigs_locate_device(t_in, None, sub.size, t_out)    # ... and the next locate call builds one for the new unitigs
        again = [e for e in tr.sync() if e[0] == "A" and int(e[3]) == 8 * slots]
        assert len(again) == 1
        dc.unitigs_end()
        assert again[0][2] not in tr.snapshot()                  # kh_unitigs_end releases it
