"""Every allocation failure of the C ABI, injected one at a time.

The test build routes every device and pinned-host allocation of the library through four wrappers (krust_amd/csrc/ctx.hip.h).
KMERHIP_ALLOC_FAIL=n makes the n-th allocation after the variable took that value fail, n+ that one and every later one, and
KMERHIP_ALLOC_TRACE=path appends one line per allocation, release and injected failure to a file -- the only way this file sees the
library's memory (no symbol is added).  One driver, sweep(): build a known state, arm n = 1, 2, 3, ..., call the operation, read
the trace.  While injections fire, the operation is held to the contract of include/kmerhip.h ("Allocation failures"):

  a reading call   KH_ERR_OOM, kh_last_error names the allocation, the context is not poisoned -- the same call repeated gives the
                   reference result --, the table's sorted pairs are the oracle's; for the calls that promise it, the live
                   allocations right after the failed call are those right before it
  a writing call   KH_ERR_OOM, then KH_ERR_STATE from a reader, then kh_reset, the same input counted again, the oracle's result --
                   or, where the library can work round the failure, KH_OK and the oracle's result at once
  kh_create        KH_ERR_OOM, *out NULL, nothing left allocated

The first n that injects nothing ends the sweep: the call made fewer than n allocations, and must be KH_OK with the reference
result.  Every step uses fresh contexts (so every allocation a fresh context reaches is failed once), ends with kh_destroy, and
the live allocations after it are those before kh_create: a leak check of every path, failed or not.

States: (a) a direct-path table of 300 synthetic reads, k = 21, and k = 31 with qualities at Q20; (b) the same reads through the
partitioned path, which leaves the 8-byte image and idle partition buffers that the readers take their scratch from; (c) such a
table widened by kh_merge_pairs / as the dst of kh_combine_into; (d) a table that must grow, forced (a tiny hint) and optional
(the pre-growth of an unhinted partitioned count).  Expected values: the oracle, and the references of the neighbouring files.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import oracle_lib as O
import profile_expect as E
import test_gpu_clip as CL
import test_gpu_format as FM
import test_gpu_graph as G
import test_gpu_join as J
import test_gpu_text as TX
import test_gpu_unitig_links as LR
import test_gpu_unitigs as UN
from krust_amd import native

pytestmark = pytest.mark.gpu

U64 = np.uint64
OK, OOM, STATE = native.KH_OK, native.KH_ERR_OOM, native.KH_ERR_STATE
SEED = 20260419
N_READS, READ_LEN = 300, 150
PART_HINT = 50_000_000      # tests/test_gpu_level2_lean.py: 2^27 slots, the arena level 2
MAX_N = 64                  # no operation here makes anywhere near that many allocations: the cap only keeps a driver bug from looping
WORKED_ROUND = {}           # (case, mode) -> the n at which an injected failure came back KH_OK: the fallbacks that were taken


def lib():
    return native.lib()


# ---- the trace ---------------------------------------------------------------------------------------------------------------------
class Trace:
    """The library's allocations as KMERHIP_ALLOC_TRACE records them: sync() reads what was appended since the last call and
    keeps the set of live pointers."""

    def __init__(self, path):
        self.path, self.pos, self.live, self.unknown = path, 0, {}, []

    def sync(self):
        with open(self.path) as f:
            f.seek(self.pos)
            data = f.read()
            self.pos = f.tell()
        assert data == "" or data.endswith("\n")
        events = []
        for line in data.splitlines():
            w = line.split()
            if w[0] == "A":
                assert w[1] in ("dev", "pin") and w[2] not in self.live, line
                self.live[w[2]] = (w[1], int(w[3]))
            elif w[0] == "F":
                if self.live.pop(w[1], None) is None:   # a release of what no traced allocation returned, or a second one:
                    self.unknown.append(w[1])            # the sweep lets none happen inside a step
            else:
                assert w[0] == "X" and w[2] in ("dev", "pin"), line
            events.append(tuple(w))
        return events

    def snapshot(self):
        self.sync()
        return dict(self.live)


@pytest.fixture(scope="module")
def tr(tmp_path_factory):
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    lib()
    path = str(tmp_path_factory.mktemp("alloc") / "trace.txt")
    open(path, "w").close()
    old = {v: os.environ.get(v) for v in ("KMERHIP_ALLOC_TRACE", "KMERHIP_ALLOC_FAIL")}
    os.environ["KMERHIP_ALLOC_TRACE"] = path
    os.environ.pop("KMERHIP_ALLOC_FAIL", None)
    yield Trace(path)
    for v, x in old.items():
        if x is None:
            os.environ.pop(v, None)
        else:
            os.environ[v] = x


def arm(value):
    os.environ["KMERHIP_ALLOC_FAIL"] = value


def disarm():
    """Unset, and one allocation made without it: the library looks at the variable when it allocates, and only a value it has
    SEEN to change re-arms -- two sweeps may end and begin with the same one."""
    os.environ.pop("KMERHIP_ALLOC_FAIL", None)
    p = C.c_void_p()
    assert lib().kh_host_alloc(C.byref(p), 1) == OK and lib().kh_host_free(p) == OK


def last_error(dc):
    return lib().kh_last_error(dc._h).decode()


def names_an_allocation(msg):
    return any(w in msg for w in ("Malloc", "memory", "buffers"))


# ---- inputs and their references, computed once ------------------------------------------------------------------------------------
class Input:
    def __init__(self, k, minq, genome, first=0, n_reads=N_READS):
        self.k, self.minq = k, minq
        self.bases, self.qual = O.synth_reads(SEED, genome, READ_LEN, first, n_reads, with_qual=True)
        m = O.OracleMap()
        m.process(self.bases, k, qual=self.qual if minq is not None else None, min_quality=minq)
        self.keys, self.counts = (np.asarray(x, dtype=U64).copy() for x in m.arrays())
        self.total, self.hist = m.total(), m.histogram()
        self.tag = ("alloc_fail", k, minq, genome, first, n_reads)
        for a in (self.bases, self.qual, self.keys, self.counts):
            a.setflags(write=False)

    @functools.lru_cache(maxsize=None)
    def device(self):
        import torch
        tb, tq = torch.from_numpy(self.bases.copy()).cuda(), torch.from_numpy(self.qual.copy()).cuda()
        torch.cuda.synchronize()
        return tb, tq

    @functools.lru_cache(maxsize=None)
    def str_dict(self):
        return {O.unpack(int(key), self.k): int(c) for key, c in zip(self.keys, self.counts)}


@functools.lru_cache(maxsize=None)
def inp(k=21, minq=None, genome=1 << 13, first=0, n_reads=N_READS):
    """genome 2^13: 300 reads cover it five times, so the table holds counts above 1, branches and tips."""
    return Input(k, minq, genome, first, n_reads)


def table_is(dc, I):
    """The table against the oracle: the k-mer total, the distinct keys, the sorted pairs."""
    st = dc.finish()
    assert st["kmers"] == I.total and st["distinct"] == I.keys.size, (st["kmers"], I.total, st["distinct"], I.keys.size)
    keys, counts = dc.result()
    assert np.array_equal(keys, I.keys) and np.array_equal(counts, I.counts)
    return st


def counted(I, state):
    """A finished context in state 'a' (the direct path: a 16-byte table, no partition buffers) or 'b' (the partitioned path: the
    8-byte image where k allows, idle partition buffers)."""
    tb, tq = I.device()
    if state == "a":
        dc = native.DeviceCounter(I.k, min_quality=I.minq, path="direct")
    else:
        dc = native.DeviceCounter(I.k, min_quality=I.minq, capacity_hint=PART_HINT, path="partition")
    dc.push_device(tb.data_ptr(), tq.data_ptr() if I.minq is not None else None, tb.numel())
    st = dc.finish()
    assert st["part_batches"] == (0 if state == "a" else 1) and st["distinct"] == I.keys.size
    if state == "b" and I.k == 21:
        assert st["slot_bytes"] == 8
    return dc


# ---- the driver ----------------------------------------------------------------------------------------------------------------------
class Op:
    """One operation on one state.  build() -> a state object (unarmed); call(st) -> the status of the operation (armed);
    ok(st) checks the reference result after a call that returned KH_OK; failed(st, rc, tr, before) holds a call during which
    an injection fired to the contract; close(st) destroys every context of the state."""
    name = "?"
    ok_at = frozenset()      # mode n: exactly these n come back KH_OK with the exact result -- the documented fallbacks, at the
                             # allocations they stand behind; every other injected failure is KH_ERR_OOM
    ok_at_plus = frozenset() # mode n+: the same where EVERY allocation from n on has a fallback

    def worked_round(self, st):
        pass

    def close(self, st):
        for dc in st.get("dcs", []):
            dc.close()
        for p in st.get("pinned", []):
            p.close()


def sweep(tr, op, mode, lo=1, hi=MAX_N):
    """n = lo .. hi (a sweep of many steps is split into cases: the one that starts at lo > 1 asserts by itself that the call
    makes at least lo allocations -- its first step must inject --, the one that ends at hi < MAX_N that it makes more than hi).
    An injected failure is a returned status, never a fault: should the runtime report an error all the same (KH_ERR_HIP), the
    whole run ends there -- nothing more is started on a device that may have faulted."""
    try:
        _sweep(tr, op, mode, lo, hi)
    except native.KmerHipError as e:
        if e.status == native.KH_ERR_HIP:
            disarm_quietly()
            pytest.exit("%s: a HIP runtime error (%s): nothing more is started on the device" % (op.name, e), 3)
        raise


def disarm_quietly():
    os.environ.pop("KMERHIP_ALLOC_FAIL", None)


def _sweep(tr, op, mode, lo, hi):
    injected, worked = [], []
    for n in range(lo, hi + 1):
        live0 = tr.snapshot()
        del tr.unknown[:]
        op.tr = tr
        st = op.build()
        ended = False
        try:
            before = tr.snapshot()
            arm("%d%s" % (n, mode))
            try:
                rc = op.call(st)
            finally:
                disarm()
            if rc == native.KH_ERR_HIP:
                pytest.exit("%s at n = %d%s: a HIP runtime error: nothing more is started on the device" % (op.name, n, mode), 3)
            fired = [e for e in st.get("events", []) + tr.sync() if e[0] == "X"]
            if fired:
                assert int(fired[0][1]) == n and [int(e[1]) for e in fired] == list(range(n, n + len(fired))), fired
                assert mode == "+" or len(fired) == 1, fired
                injected.append(n)
                if rc == OK:
                    assert n in (op.ok_at if mode == "" else op.ok_at_plus), (op.name, n, mode, "an injected failure came back KH_OK where no fallback is documented")
                    worked.append(n)
                    WORKED_ROUND.setdefault((op.name, mode), []).append(n)
                    op.worked_round(st)
                    op.ok(st)
                else:
                    op.failed(st, rc, tr, before)
            else:   # fewer than n allocations: the sweep ends with a call nothing interfered with
                assert rc == OK, (op.name, n, rc)
                op.ok(st)
                ended = True
        finally:
            op.close(st)
        left = tr.snapshot()
        assert left == live0, (op.name, n, "leaked", {p: v for p, v in left.items() if p not in live0})
        assert tr.unknown == [], (op.name, n, "released twice, or never allocated", tr.unknown)
        if ended:
            break
    else:
        assert hi < MAX_N, "%s: the sweep has not ended at n = %d" % (op.name, MAX_N)   # (hi < MAX_N: the next case goes on from there)
    assert injected, (op.name, "no step injected a failure: the sweep tested nothing")
    expect = op.ok_at if mode == "" else op.ok_at_plus   # every documented fallback of this range was TAKEN: KH_OK there, and nowhere else
    assert set(worked) == {n for n in expect if lo <= n <= min(hi, injected[-1])}, (op.name, mode, worked, sorted(expect))
    print("%s mode n%s: injected at n = %s%s" % (op.name, mode, injected,
                                                  ", KH_OK at %s" % WORKED_ROUND[(op.name, mode)] if (op.name, mode) in WORKED_ROUND else ""))


# ---- reading calls ---------------------------------------------------------------------------------------------------------------------
class Reader(Op):
    """run(dc, I) -> (status, value); want(I) -> the reference value.  strict: the header says nothing stays allocated."""

    def __init__(self, name, state, run, want, strict=False, k=21, minq=None):
        self.name, self.state, self.run, self.want, self.strict, self.k, self.minq = "%s[%s]" % (name, state), state, run, want, strict, k, minq
        self.msg = ERROR_TEXT.get(name)   # what kh_last_error says where the call has one allocation text of its own

    def build(self):
        I = inp(self.k, self.minq)
        return {"I": I, "dcs": [counted(I, self.state)]}

    def call(self, st):
        rc, st["got"] = self.run(st["dcs"][0], st["I"])
        return rc

    def ok(self, st):
        same(st["got"], self.want(st["I"]))
        table_is(st["dcs"][0], st["I"])

    def failed(self, st, rc, tr, before):
        dc, I = st["dcs"][0], st["I"]
        assert rc == OOM, rc
        msg = last_error(dc)
        assert names_an_allocation(msg) and "poisoned" not in msg, msg
        if self.msg:   # (the pinned staging of a host form says its own)
            assert self.msg in msg or "hipHostMalloc(stage)" in msg, (self.msg, msg)
        if self.strict:
            assert tr.snapshot() == before, (self.name, "the failed call left memory allocated")
        rc2, got = self.run(dc, I)          # not poisoned: the same call again, the reference result
        assert rc2 == OK, (rc2, last_error(dc))
        same(got, self.want(I))
        table_is(dc, I)                     # ... and the table is what it was


ERROR_TEXT = {"result_copy": "hipMalloc(result)", "histogram": "hipMalloc(histogram)", "lookup": "hipMalloc(lookup)", "compare": "hipMalloc(join words)",
              "graph_stats": "hipMalloc(graph words)", "graph_masks": "hipMalloc(graph masks)", "profile": "kh_profile: chunk buffers",
              "profile_q20": "kh_profile: chunk buffers", "result_sorted_device": "device memory for the sort"}


def same(got, want):
    if isinstance(want, (tuple, list)) and not (want and isinstance(want[0], tuple)):
        assert len(got) == len(want)
        for g, w in zip(got, want):
            same(g, w)
    elif isinstance(want, np.ndarray):
        assert isinstance(got, np.ndarray) and got.dtype == want.dtype and got.shape == want.shape and np.array_equal(got, want)
    else:
        assert got == want


def status_of(f):
    """What a method of native.DeviceCounter returns, as (status, value)."""
    try:
        return OK, f()
    except native.KmerHipError as e:
        return e.status, None


def r_copy(dc, I):
    return status_of(lambda: dc.result())


def r_sorted(dc, I):
    return status_of(lambda: dc.result_sorted())


def r_sorted_device(dc, I):
    import torch
    n = I.keys.size
    dk, dcn = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
    rc, got = status_of(lambda: dc.result_sorted_device(dk.data_ptr(), dcn.data_ptr(), n))
    return rc, None if rc != OK else (dk.cpu().numpy().view(U64)[:got], dcn.cpu().numpy().view(U64)[:got])


def w_pairs(I):
    return (I.keys, I.counts)


def r_histogram(dc, I):
    return status_of(lambda: dc.histogram())


def probe_keys(I):
    absent = np.setdiff1d(np.arange(1, 400, dtype=U64), I.keys)[:50]
    return np.concatenate((I.keys[::7], absent))


def r_lookup(dc, I):
    return status_of(lambda: dc.lookup(probe_keys(I)))


def w_lookup(I):
    keys = probe_keys(I)
    pos = np.minimum(np.searchsorted(I.keys, keys), I.keys.size - 1)
    return np.where(I.keys[pos] == keys, I.counts[pos], U64(0))


def text_of(dc, fmt, sorted_, device=False):
    import torch
    dc.result_text_begin(fmt, 1, sorted=sorted_)
    pieces = []
    buf = torch.empty(1 << 16, dtype=torch.uint8, device="cuda") if device else np.empty(1 << 16, dtype=np.uint8)
    while True:
        n = dc.result_text_device(buf) if device else dc.result_text_next(buf)
        if n == 0:
            return b"".join(pieces)
        pieces.append(bytes(buf[:n].cpu().numpy()) if device else buf[:n].tobytes())


def r_text(fmt, sorted_, device=False):
    def run(dc, I):
        rc, text = status_of(lambda: text_of(dc, fmt, sorted_, device))
        if rc != OK:
            return rc, None
        recs = FM.split_records(fmt, text)
        return rc, recs if sorted_ else sorted(recs)
    return run


def w_text(fmt, sorted_):
    def want(I):
        if sorted_:   # ascending key order = the k-mer strings in lexicographic order
            return [FM.record(fmt, km, c) for km, c in sorted(I.str_dict().items())]
        return FM.expected_records(fmt, I.str_dict())
    return want


def r_profile(dc, I):
    return status_of(lambda: dc.profile(I.bases, I.qual if I.minq is not None else None))


def w_profile(I):
    return E.np_profile(I.bases, I.k, I.keys, I.counts, I.qual if I.minq is not None else None, I.minq)


def r_profile_records(dc, I):
    return status_of(lambda: dc.profile_records(I.bases, E.starts_of(I.bases), I.qual if I.minq is not None else None, lo=2, hi=5).copy())


def w_profile_records(I):
    return E.rows_of(w_profile(I), E.starts_of(I.bases), 2, 5)


def r_compare(dc, I):
    return status_of(lambda: dc.compare(dc, 1, 2))


def w_compare(I):
    u, ca, cb = J.align(I.keys, I.counts, I.keys, I.counts)
    return J.np_words(ca, cb, 1, 2)


def r_graph_stats(dc, I):
    return status_of(lambda: dc.graph_stats(2))


def w_graph_stats(I):
    return G.np_words(I.keys, I.counts, 2, I.k)


def r_graph_masks(dc, I):
    return status_of(lambda: dc.graph_masks(probe_keys(I), 1))


def w_graph_masks(I):
    return G.np_masks(probe_keys(I), I.keys, I.k)


def r_unitigs(dc, I):
    return status_of(lambda: dc.unitigs(1))


def w_unitigs(I):
    ref = UN.ref_of(I.tag, I.keys, I.counts, I.k, 1)
    return (ref.rows, np.frombuffer(ref.bases, dtype=np.uint8))


def r_unitigs_linked(dc, I):
    return status_of(lambda: dc.unitigs_linked(2))


def w_unitigs_linked(I):
    ref, lref = UN.ref_of(I.tag, I.keys, I.counts, I.k, 2), LR.links_of(I.tag, I.keys, I.counts, I.k, 2)
    return (ref.rows, np.frombuffer(ref.bases, dtype=np.uint8), lref.links)


def r_unitigs_begin_only(linked):
    """kh_unitigs_begin[_linked] alone: the call whose header says that nothing stays allocated when it fails."""
    def run(dc, I):
        rc, got = status_of(lambda: dc.unitigs_begin_linked(1) if linked else dc.unitigs_begin(1))
        if rc == OK:
            dc.unitigs_end()
        return rc, got
    return run


def w_unitigs_begin_only(linked):
    def want(I):
        ref = UN.ref_of(I.tag, I.keys, I.counts, I.k, 1)
        sizes = (ref.rows.shape[0], len(ref.bases))
        return sizes + (LR.links_of(I.tag, I.keys, I.counts, I.k, 1).links.size,) if linked else sizes
    return want


READERS = [
    ("result_copy", r_copy, w_pairs, False),
    ("result_sorted", r_sorted, w_pairs, True),
    ("result_text_tsv", r_text("tsv", False), w_text("tsv", False), False),
    ("result_text_fasta_sorted", r_text("fasta", True), w_text("fasta", True), False),
    ("result_text_json_device", r_text("json", False, device=True), w_text("json", False), False),
    ("histogram", r_histogram, lambda I: I.hist, False),
    ("lookup", r_lookup, w_lookup, False),
    ("profile", r_profile, w_profile, False),
    ("profile_records", r_profile_records, w_profile_records, False),
    ("compare", r_compare, w_compare, False),
    ("graph_stats", r_graph_stats, w_graph_stats, False),
    ("graph_masks", r_graph_masks, w_graph_masks, True),
    ("unitigs", r_unitigs, w_unitigs, False),
    ("unitigs_linked", r_unitigs_linked, w_unitigs_linked, False),
    ("unitigs_begin", r_unitigs_begin_only(False), w_unitigs_begin_only(False), True),
    ("unitigs_begin_linked", r_unitigs_begin_only(True), w_unitigs_begin_only(True), True),
]
# result_sorted_device allocates only where there are no partition buffers to take its scratch from: state (a)
READER_CASES = [(name, s, run, want, strict) for name, run, want, strict in READERS for s in "ab"] + \
               [("result_sorted_device", "a", r_sorted_device, w_pairs, True)]


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("case", READER_CASES, ids=["%s-%s" % (c[0], c[1]) for c in READER_CASES])
def test_reading_calls(tr, case, mode):
    name, state, run, want, strict = case
    sweep(tr, Reader(name, state, run, want, strict), mode)


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
def test_profile_with_qualities(tr, mode):
    """k = 31 at Q20: the chunk buffers carry the quality bytes too."""
    sweep(tr, Reader("profile_q20", "a", r_profile, w_profile, False, k=31, minq=20), mode)


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("name,state", [("profile_records", "a"), ("result_copy", "b"), ("lookup", "b"), ("unitigs", "b")])
def test_readers_at_k31_q20(tr, name, state, mode):
    """k = 31 at Q20: the rows of kh_profile_records with qualities, and readers of a partitioned table that is NOT the 8-byte image
    (8-byte payloads end in the 16-byte table; its partition buffers are idle all the same)."""
    run, want, strict = {n: (r, w, s) for n, r, w, s in READERS}[name]
    sweep(tr, Reader(name + "_q20", state, run, want, strict, k=31, minq=20), mode)


def test_the_device_forms_allocate_nothing(tr):
    """kh_result_size, kh_result_copy_device, kh_profile_device, kh_profile_records_device, kh_graph_masks_device and the device
    copies of the unitigs write into the caller's memory and take no scratch: with EVERY allocation set to fail they return the
    reference result, and the trace holds no event of theirs.  (Nothing to sweep: there is no allocation to fail.)"""
    import torch
    I = inp()
    tb, _ = I.device()
    for state in "ab":
        dc = counted(I, state)
        try:
            nu, nb, nl = dc.unitigs_begin_linked(1)
            n, keys = I.keys.size, probe_keys(I)
            dk, dcn = torch.zeros(n, dtype=torch.int64, device="cuda"), torch.zeros(n, dtype=torch.int64, device="cuda")
            prof = torch.zeros(tb.numel(), dtype=torch.int32, device="cuda")
            starts = E.starts_of(I.bases)
            d_starts = torch.from_numpy(starts.view(np.int64).copy()).cuda()
            rows = torch.zeros((starts.size - 1) * 8, dtype=torch.int32, device="cuda")
            d_keys, masks = torch.from_numpy(keys.view(np.int64).copy()).cuda(), torch.zeros(keys.size, dtype=torch.uint8, device="cuda")
            u_rows, u_bases = torch.zeros(nu * 4, dtype=torch.int64, device="cuda"), torch.zeros(nb, dtype=torch.uint8, device="cuda")
            u_links = torch.zeros(max(nl, 1), dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            tr.sync()
            arm("1+")
            try:
                dc.unitigs_copy_device(u_rows, nu, u_bases, nb)      # (first: kh_result_copy_device enters as a writer would, and the unitigs go stale)
                dc.unitigs_links_copy_device(u_links, nl)
                assert dc.result_size(2) == int((I.counts >= 2).sum())
                got = dc.result_device(dk.data_ptr(), dcn.data_ptr(), n)
                dc.profile_device(tb, None, tb.numel(), prof)
                dc.profile_records_device(tb, None, tb.numel(), d_starts, starts.size - 1, rows, lo=2, hi=5)
                dc.graph_masks_device(d_keys, keys.size, masks, 1)
            finally:
                disarm()
            ev = tr.sync()
            assert [e for e in ev if e[0] == "X"] == [], ev                       # nothing tried to allocate
            assert [e[1:2] + e[3:] for e in ev if e[0] == "A"] == [("pin", "1")], ev  # (disarm()'s own byte)
            order = np.argsort(dk.cpu().numpy().view(U64)[:got], kind="stable")
            assert got == n and np.array_equal(dk.cpu().numpy().view(U64)[order], I.keys) and np.array_equal(dcn.cpu().numpy().view(U64)[order], I.counts)
            P = w_profile(I)
            assert np.array_equal(prof.cpu().numpy().view(np.uint32), P)
            assert np.array_equal(rows.cpu().numpy().view(np.uint32).reshape(-1, 8), E.rows_of(P, starts, 2, 5))
            assert np.array_equal(masks.cpu().numpy(), w_graph_masks(I))
            ref, lref = UN.ref_of(I.tag, I.keys, I.counts, I.k, 1), LR.links_of(I.tag, I.keys, I.counts, I.k, 1)
            assert np.array_equal(u_rows.cpu().numpy().view(U64).reshape(-1, 4), ref.rows) and u_bases.cpu().numpy().tobytes() == ref.bases
            assert np.array_equal(u_links.cpu().numpy().view(U64)[:nl], lref.links)
            dc.unitigs_end()
        finally:
            dc.close()


# ---- writing calls -------------------------------------------------------------------------------------------------------------------
class Writer(Op):
    """make(I) -> a fresh context; steps(dc, I, st): the calls of the operation as a list of functions that return a status --
    prep: how many of them are made BEFORE the injection is armed (they build the state).  The status of the operation is
    the first that is not KH_OK."""

    def __init__(self, name, make, steps, prep=0, I=None, want=None, ok_at=(), pinned=False):
        self.name, self.make, self.steps, self.prep, self.I, self.want = name, make, steps, prep, I or inp(), want
        self.ok_at, self.pinned = frozenset(ok_at), pinned

    def build(self):
        st = {"I": self.I, "dcs": [self.make(self.I)], "pinned": []}
        if self.pinned:
            for a in (self.I.bases, self.I.qual):
                p = native.PinnedArray(a.size)
                p.array[:] = a
                st["pinned"].append(p)
        self.run(st, 0, self.prep)
        return st

    def run(self, st, lo, hi=None):
        for f in self.steps(st["dcs"][0], st["I"], st)[lo:hi]:
            rc = f()
            if rc != OK:
                return rc
        return OK

    def call(self, st):
        return self.run(st, self.prep)

    def ok(self, st):
        table_is(st["dcs"][0], self.want or st["I"])

    def failed(self, st, rc, tr, before):
        dc = st["dcs"][0]
        assert rc == OOM, (rc, last_error(dc))
        assert names_an_allocation(last_error(dc)), last_error(dc)
        n = C.c_uint64(0)
        assert lib().kh_result_size(dc._h, 1, C.byref(n)) == STATE and "poisoned" in last_error(dc)   # poisoned: a reader is refused
        assert lib().kh_push_device(dc._h, None, None, 0) == STATE                                      # ... and so is a push
        assert lib().kh_reset(dc._h) == OK, last_error(dc)                                              # kh_reset lifts it
        assert dc.finish()["distinct"] == 0 and dc.result_size() == 0                                   # ... and leaves an empty context
        assert self.run(st, 0) == OK, last_error(dc)                                                    # the same input counted again
        self.ok(st)


def h(dc):
    return dc._h


def hint_of(I):
    return 2 * I.keys.size


def mk_direct(I):
    return native.DeviceCounter(I.k, min_quality=I.minq, path="direct")


def mk_part(I):
    return native.DeviceCounter(I.k, min_quality=I.minq, capacity_hint=PART_HINT, path="partition")


def mk_tiny(I):
    return native.DeviceCounter(I.k, min_quality=I.minq, capacity_hint=1, path="direct")


def mk_unhinted_part(I):
    """No hint, 8 regions (KMERHIP_TABLE_REGIONS, read at kh_create): the second partitioned push finds the table too small for
    what it may bring and tries to grow it first -- a growth that may fail (batch.hip count_device_range)."""
    os.environ["KMERHIP_TABLE_REGIONS"] = "8"
    try:
        return native.DeviceCounter(I.k, min_quality=I.minq, path="partition")
    finally:
        del os.environ["KMERHIP_TABLE_REGIONS"]


def mk_defer(I):
    return native.DeviceCounter(I.k, min_quality=I.minq, defer_text_scan=True)


def s_push_device(dc, I, st):
    tb, tq = I.device()
    return [lambda: lib().kh_push_device(h(dc), tb.data_ptr(), tq.data_ptr() if I.minq is not None else None, tb.numel())]


def s_push_host(dc, I, st):
    b, q = (st["pinned"][0].array, st["pinned"][1].array) if st["pinned"] else (I.bases, I.qual)
    return [lambda: lib().kh_push(h(dc), b.ctypes.data, q.ctypes.data if I.minq is not None else None, b.size),
            lambda: lib().kh_finish(h(dc), None)]


def s_push_twice(dc, I, st):
    """Two halves, each a push_device: the second meets a table that is not empty."""
    tb, tq = I.device()
    half = (N_READS // 2) * (READ_LEN + 1)
    q = lambda off: tq.data_ptr() + off if I.minq is not None else None
    return [lambda: lib().kh_push_device(h(dc), tb.data_ptr(), q(0), half),
            lambda: lib().kh_push_device(h(dc), tb.data_ptr() + half, q(half), tb.numel() - half)]


@functools.lru_cache(maxsize=None)
def texts(k, minq, fmt):
    """(text, second text, the Input-like reference of both) -- the references are the Python line parsers of test_gpu_text."""
    rng = np.random.default_rng(41 + k)
    mk = (lambda n: TX.make_fastq(rng, n, 30, 200)) if fmt == "fastq" else (lambda n: TX.make_fasta(rng, n, 30, 400, 60))
    t1, t2 = mk(120), mk(80)

    class W:
        pass
    out = []
    for parts in ((t1,), (t1, t2)):
        d = {}
        for t in parts:
            for key, c in TX.expect(t, fmt, k, minq).items():
                d[key] = d.get(key, 0) + c
        w = W()
        w.keys = np.array(sorted(d), dtype=U64)
        w.counts = np.array([d[x] for x in sorted(d)], dtype=U64)
        w.total = int(sum(d.values()))
        out.append(w)
    return t1, t2, out[0], out[1]


def s_text(fmt, n_texts=1):
    def steps(dc, I, st):
        t1, t2 = texts(I.k, I.minq, fmt)[:2]
        push = lambda t: (lambda: lib().kh_push_text(h(dc), np.frombuffer(t, dtype=np.uint8).ctypes.data, len(t), native._text_format(fmt)))
        return [push(t) for t in (t1, t2)[:n_texts]] + [lambda: lib().kh_finish(h(dc), None)]
    return steps


def s_merge_pairs(device):
    def steps(dc, I, st):
        import torch
        tb, _ = I.device()
        extra = inp(I.k, None, 1 << 13, N_READS, 100)   # the next 100 reads of the same genome: keys the table holds and new ones
        if device:
            if "dk" not in st:
                st["dk"], st["dc"] = (torch.from_numpy(a.view(np.int64).copy()).cuda() for a in (extra.keys, extra.counts))
                torch.cuda.synchronize()
            merge = lambda: lib().kh_merge_pairs_device(h(dc), st["dk"].data_ptr(), st["dc"].data_ptr(), extra.keys.size)
        else:
            merge = lambda: lib().kh_merge_pairs(h(dc), extra.keys.ctypes.data, extra.counts.ctypes.data, extra.keys.size)
        return [lambda: lib().kh_push_device(h(dc), tb.data_ptr(), None, tb.numel()), merge, lambda: lib().kh_finish(h(dc), None)]
    return steps


@functools.lru_cache(maxsize=None)
def merged_want():
    """The table of inp() after the pairs of the next 100 reads were merged in: count[key] += c."""
    I, extra = inp(), inp(21, None, 1 << 13, N_READS, 100)
    u, ca, cb = J.align(I.keys, I.counts, extra.keys, extra.counts)
    keys, counts = J.np_combine(u, ca, cb, "union", "sum")

    class W:
        pass
    w = W()
    w.keys, w.counts, w.total = keys, counts, I.total + extra.total
    return w


def writer_cases():
    big = inp(21, None, 1 << 20)      # 300 reads of a 2^20 genome: ~39,000 distinct keys, more than a table of 2^15 slots may hold
    q20 = inp(31, 20)
    W = Writer
    fq = lambda k, minq: texts(k, minq, "fastq")
    return [
        W("push_device-direct", mk_direct, s_push_device),
        W("push_device-partition", mk_part, s_push_device, ok_at=[30]),   # (allocation 30, the last: the 8-byte image -- without it the 16-byte table, batch.hip finish_batch)
        W("push_device-q20-partition", mk_part, s_push_device, I=q20),      # (8-byte payloads: no image, no fallback)
        W("push-pageable", mk_direct, s_push_host),
        W("push-pinned", mk_direct, s_push_host, pinned=True),
        W("push-pageable-q20", mk_direct, s_push_host, I=q20),
        W("finish", mk_direct, lambda dc, I, st: s_push_host(dc, I, st), prep=1),                         # (the pending push is counted by kh_finish)
        W("growth-forced", mk_tiny, s_push_device, I=big),
        W("growth-second-push", mk_tiny, s_push_twice, prep=1, I=big),
        W("pre-growth-optional", mk_unhinted_part, s_push_twice, prep=1, I=big, ok_at=[1]),            # (batch.hip: the pre-growth may fail)
        W("push_text-fasta", mk_direct, s_text("fasta"), want=texts(21, None, "fasta")[2], ok_at=[5]),   # (allocation 5: the generous text buffer -- without it the smaller one, input.hip scan_text)
        W("push_text-fastq", mk_direct, s_text("fastq"), want=fq(21, None)[2], ok_at=[5]),
        W("push_text-fastq-q20", mk_direct, s_text("fastq"), I=q20, want=fq(31, 20)[2], ok_at=[5]),
        W("push_text-fastq-deferred", mk_defer, s_text("fastq", 2), want=fq(21, None)[3], ok_at=[6]),
        W("push_text-fasta-deferred", mk_defer, s_text("fasta", 2), want=texts(21, None, "fasta")[3], ok_at=[6]),
        W("merge_pairs-a", mk_direct, s_merge_pairs(False), prep=1, want=merged_want()),
        W("merge_pairs-b-widens", mk_part, s_merge_pairs(False), prep=1, want=merged_want()),
        W("merge_pairs_device-b-widens", mk_part, s_merge_pairs(True), prep=1, want=merged_want()),
    ]


WRITER_NAMES = ["push_device-direct", "push_device-partition", "push_device-q20-partition", "push-pageable", "push-pinned", "push-pageable-q20",
                "finish", "growth-forced", "growth-second-push", "pre-growth-optional", "push_text-fasta", "push_text-fastq", "push_text-fastq-q20",
                "push_text-fastq-deferred", "push_text-fasta-deferred", "merge_pairs-a", "merge_pairs-b-widens", "merge_pairs_device-b-widens"]


# a partitioned count makes about 30 allocations in a fresh context: its sweep is three cases
RANGES = {"push_device-partition": [(1, 10), (11, 20), (21, MAX_N)], "push_device-q20-partition": [(1, 10), (11, 20), (21, MAX_N)]}
WRITER_CASES = [(name, lo, hi) for name in WRITER_NAMES for lo, hi in RANGES.get(name, [(1, MAX_N)])]


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("name,lo,hi", WRITER_CASES, ids=["%s%s" % (n, "" if (lo, hi) == (1, MAX_N) else "-from%d" % lo) for n, lo, hi in WRITER_CASES])
def test_writing_calls(tr, name, lo, hi, mode):
    cases = {w.name: w for w in writer_cases()}
    assert sorted(cases) == sorted(WRITER_NAMES)
    sweep(tr, cases[name], mode, lo, hi)


# ---- kh_export_by_owner_device: a writing call whose result lands in the caller's arrays --------------------------------------------
NPARTS = 4


class ExportByOwner(Writer):
    """The reads counted (prep), then the pairs exported by owner into device arrays of the caller.  The call's own scratch is the
    per-owner cursors; from state (b) it also widens the 8-byte image.  The clean run: every part holds exactly its own keys, all
    parts together the oracle's pairs, and the table is what it was."""

    def __init__(self, name, make):
        Writer.__init__(self, name, make, self.export_steps, prep=1)

    def export_steps(self, dc, I, st):
        import torch
        tb, _ = I.device()
        n = I.keys.size
        if "xk" not in st:
            st["xk"], st["xc"] = (torch.zeros(n, dtype=torch.int64, device="cuda") for _ in range(2))
            st["parts"] = np.zeros(NPARTS, dtype=U64)
            torch.cuda.synchronize()
        return [lambda: lib().kh_push_device(h(dc), tb.data_ptr(), None, tb.numel()),
                lambda: lib().kh_export_by_owner_device(h(dc), NPARTS, st["xk"].data_ptr(), st["xc"].data_ptr(), n, st["parts"].ctypes.data)]

    def ok(self, st):
        I = st["I"]
        keys, counts, parts = st["xk"].cpu().numpy().view(U64), st["xc"].cpu().numpy().view(U64), st["parts"]
        assert int(parts.sum()) == I.keys.size
        owners = np.array([native.owner(int(x), I.k, NPARTS) for x in keys])
        assert np.array_equal(owners, np.repeat(np.arange(NPARTS), parts.astype(np.int64)))   # grouped by owner, in owner order
        order = np.argsort(keys, kind="stable")
        assert np.array_equal(keys[order], I.keys) and np.array_equal(counts[order], I.counts)
        table_is(st["dcs"][0], I)


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("state", ["a", "b-widens"])
def test_export_by_owner(tr, state, mode):
    sweep(tr, ExportByOwner("export_by_owner-%s" % state, mk_direct if state == "a" else mk_part), mode)


# ---- kh_create ---------------------------------------------------------------------------------------------------------------------------
class Create(Op):
    name = "kh_create"

    def build(self):
        return {"dcs": []}

    def call(self, st):
        cfg = native.KhConfig(C.sizeof(native.KhConfig), 21, -1, -1, 0, None, 0, 0)
        st["h"] = C.c_void_p(0xDEAD)
        return lib().kh_create(C.byref(st["h"]), C.byref(cfg))

    def ok(self, st):
        dc = native.DeviceCounter._adopt(st["h"].value, 21, None)
        dc._owned = True
        st["dcs"].append(dc)
        I = inp()
        tb, _ = I.device()
        dc.push_device(tb.data_ptr(), None, tb.numel())
        table_is(dc, I)

    def failed(self, st, rc, tr, before):
        assert rc == OOM and st["h"].value is None, (rc, st["h"].value)
        assert tr.snapshot() == before, "a failed kh_create left memory allocated"


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
def test_create(tr, mode):
    sweep(tr, Create(), mode)


# ---- two tables: kh_combine_into and kh_clip_tips_into -----------------------------------------------------------------------------------
class Combine(Op):
    """dst: a state (b) table -- the 8-byte image, which the call widens -- of the reads; a = b: a state `src` table of the same
    reads.  union / sum of a table with itself doubles every count; dst ends with three times the oracle's."""

    def __init__(self, src):
        self.name, self.src = "combine_into[dst=b,src=%s]" % src, src

    def build(self):
        I = inp()
        return {"I": I, "dcs": [counted(I, "b"), counted(I, self.src)]}

    def call(self, st):
        dst, a = st["dcs"]
        n = C.c_uint64(0)
        rc = lib().kh_combine_into(h(dst), h(a), h(a), native.SET_UNION, native.CALC_SUM, 1, 1, C.byref(n))
        st["n_pairs"] = n.value
        return rc

    def want(self, I):
        u, ca, cb = J.align(I.keys, I.counts, I.keys, I.counts)
        keys, counts = J.np_combine(u, ca, cb, "union", "sum")
        assert np.array_equal(keys, I.keys)

        class W:
            pass
        w = W()
        w.keys, w.counts, w.total = keys, counts + I.counts, 3 * I.total
        return w, keys.size

    def ok(self, st):
        w, n_pairs = self.want(st["I"])
        assert st["n_pairs"] == n_pairs
        table_is(st["dcs"][0], w)
        table_is(st["dcs"][1], st["I"])

    def failed(self, st, rc, tr, before):
        dst, a = st["dcs"]
        I = st["I"]
        assert rc == OOM and names_an_allocation(last_error(dst)), (rc, last_error(dst))
        table_is(a, I)                                                     # the sources are only read: usable and unchanged
        assert lib().kh_result_size(h(dst), 1, C.byref(C.c_uint64(0))) == STATE
        assert lib().kh_reset(h(dst)) == OK
        tb, _ = I.device()
        dst.push_device(tb.data_ptr(), None, tb.numel())
        assert self.call(st) == OK, last_error(dst)
        self.ok(st)


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("src", ["a", "b"])
def test_combine_into(tr, src, mode):
    sweep(tr, Combine(src), mode)


PREFILL = 7


class Clip(Op):
    """src: a state (a) / (b) table; dst: a table that holds PREFILL at three of src's keys.  A failure of src's scratch leaves
    src usable and dst holding what it held (and nothing allocated); one on dst's side poisons dst alone."""

    def __init__(self, src):
        self.name, self.src = "clip_tips_into[src=%s]" % src, src

    def fill(self, dst, I):
        dst.merge_pairs(I.keys[:3], np.full(3, PREFILL, dtype=U64))
        assert dst.finish()["distinct"] == 3

    def build(self):
        I = inp()
        dst = native.DeviceCounter(I.k, path="direct")
        self.fill(dst, I)
        return {"I": I, "dcs": [dst, counted(I, self.src)]}

    def call(self, st):
        dst, src = st["dcs"]
        out = np.zeros(native.CLIP_WORDS, dtype=U64)
        rc = lib().kh_clip_tips_into(h(dst), h(src), 1, st["I"].k, out.ctypes.data)
        st["words"] = dict(zip(native.CLIP_NAMES, (int(x) for x in out)))
        return rc

    def ok(self, st):
        I = st["I"]
        cr = CL.clip_of(I.tag, I.keys, I.counts, I.k, 1, I.k)
        assert st["words"] == CL.words_dict(cr), (st["words"], CL.words_dict(cr))
        d = dict(zip(cr.keys.tolist(), cr.counts.tolist()))
        for key in I.keys[:3].tolist():
            d[key] = d.get(key, 0) + PREFILL
        gk, gc = st["dcs"][0].result_sorted()
        assert gk.tolist() == sorted(d) and gc.tolist() == [d[x] for x in sorted(d)]
        table_is(st["dcs"][1], I)

    def failed(self, st, rc, tr, before):
        dst, src = st["dcs"]
        I = st["I"]
        assert rc == OOM and names_an_allocation(last_error(dst)), (rc, last_error(dst))
        n = C.c_uint64(0)
        if lib().kh_result_size(h(dst), 1, C.byref(n)) == OK:              # src's scratch: dst holds what it held, nothing stays allocated
            assert tr.snapshot() == before, (self.name, "the failed call left memory allocated")
            gk, gc = dst.result_sorted()
            assert np.array_equal(gk, I.keys[:3]) and gc.tolist() == [PREFILL] * 3
        else:                                                              # dst's side: poisoned, until kh_reset
            assert "poisoned" in last_error(dst)
            assert lib().kh_reset(h(dst)) == OK
            self.fill(dst, I)
        table_is(src, I)                                                   # src: usable and unchanged, whichever side failed
        assert self.call(st) == OK, last_error(dst)
        self.ok(st)


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("src", ["a", "b"])
def test_clip_tips_into(tr, src, mode):
    sweep(tr, Clip(src), mode)


# ---- one logical-shard round per unit format: export on the sender, merge on the receiver ------------------------------------------------
class RegionRound(Op):
    """One sender, one receiver (kh_set_shard(0, 1)), as test_region_ordered_merge_logical_shards sets them up.  The status is that
    of the first call that fails; whichever context it poisoned is reset, refilled, and the round made again."""

    def __init__(self, fmt):
        self.name, self.fmt = "region_round[%s]" % fmt, fmt
        # merge.hip merge_regions: a fresh merge of packed pairs / heads builds the 8-byte image (allocation 5 of the round, the first
        # of the merge), or the 16-byte table where that has no room; wide pairs have no such fallback, and neither has the export
        self.ok_at = frozenset([5] if fmt != "wide" else [])

    def worked_round(self, st):
        assert not [e for e in st["events"] if e[0] == "X"], "the fallback that was taken is the merge's, not the export's"

    def build(self):
        import torch
        I = inp()
        snd = native.DeviceCounter(I.k, capacity_hint=PART_HINT, path="direct")   # (2^15 regions: 27 hash bits below the region index, heads take 28)
        tb, _ = I.device()
        snd.push_device(tb.data_ptr(), None, tb.numel())
        R = snd.finish()["table_slots"] // 4096
        rcv = native.DeviceCounter(I.k, capacity_hint=PART_HINT)
        rcv.set_shard(0, 1)
        n = I.keys.size
        st = {"I": I, "dcs": [snd, rcv], "R": R, "units": torch.zeros(4 * n, dtype=torch.int64, device="cuda"),
              "counts": torch.zeros(n, dtype=torch.int64, device="cuda"), "rc": torch.zeros(R, dtype=torch.int32, device="cuda")}
        torch.cuda.synchronize()
        return st

    def export(self, st):
        snd, R, n = st["dcs"][0], st["R"], st["I"].keys.size
        parts, nreg = np.zeros(1, dtype=U64), C.c_uint64(0)
        u, c, r = st["units"].data_ptr(), st["counts"].data_ptr(), st["rc"].data_ptr()
        if self.fmt == "wide":
            return lib().kh_export_regions_device(h(snd), 1, u, c, n, r, R, parts.ctypes.data, C.byref(nreg))
        if self.fmt == "packed":
            return lib().kh_export_regions_packed_device(h(snd), 1, u, n, r, R, parts.ctypes.data, C.byref(nreg))
        return lib().kh_export_regions_heads_device(h(snd), 1, u, 8 * n, r, R, parts.ctypes.data, C.byref(nreg))

    def merge(self, st):
        rcv, R = st["dcs"][1], st["R"]
        one = lambda t: (C.c_void_p * 1)(C.c_void_p(t.data_ptr()))
        if self.fmt == "wide":
            return lib().kh_merge_regions_device(h(rcv), 1, R, one(st["units"]), one(st["counts"]), one(st["rc"]))
        if self.fmt == "packed":
            return lib().kh_merge_regions_packed_device(h(rcv), 1, R, one(st["units"]), one(st["rc"]))
        return lib().kh_merge_regions_heads_device(h(rcv), 1, R, one(st["units"]), one(st["rc"]))

    def call(self, st):
        st["at"] = "export"
        rc = self.export(st)
        st["events"] = self.tr.sync()   # (what the export did, apart from what the merge does)
        if rc == OK:
            st["at"] = "merge"
            rc = self.merge(st)
        return rc

    def ok(self, st):
        snd, rcv = st["dcs"]
        assert rcv.finish()["distinct"] == st["I"].keys.size
        keys, counts = rcv.result()
        assert np.array_equal(keys, st["I"].keys) and np.array_equal(counts, st["I"].counts)
        table_is(snd, st["I"])

    def failed(self, st, rc, tr, before):
        snd, rcv = st["dcs"]
        I = st["I"]
        bad = snd if st["at"] == "export" else rcv
        assert rc == OOM and names_an_allocation(last_error(bad)), (rc, last_error(bad))
        assert lib().kh_result_size(h(bad), 1, C.byref(C.c_uint64(0))) == STATE
        assert lib().kh_reset(h(bad)) == OK
        if bad is snd:
            tb, _ = I.device()
            snd.push_device(tb.data_ptr(), None, tb.numel())
            assert self.export(st) == OK, last_error(snd)
        else:
            table_is(snd, I)
            rcv.set_shard(0, 1)
        assert self.merge(st) == OK, last_error(rcv)
        self.ok(st)


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("fmt", ["wide", "packed", "heads"])
def test_region_round(tr, fmt, mode):
    sweep(tr, RegionRound(fmt), mode)


# ---- kh_merge_across on a one-rank communicator --------------------------------------------------------------------------------------
class MergeAcross(Op):
    """A communicator of one rank: the whole sequence of the exchange -- digests, send and receive buffers, region counts, the export,
    the shard rebuilt by merge_regions -- with this context as its only peer.  A failure that the sequence works round (the
    kernels' digest partials, the shard's 8-byte image) is KH_OK with the exact table.  Every other one is KH_ERR_OOM: scratch of
    the exchange itself does not poison, what fails inside the counting or the merge does; either way the table's content is
    unspecified until kh_reset, after which the same input is counted and merged again.  (RCCL's own memory is not the wrappers'.)"""

    def __init__(self, state, ok_at):
        self.name, self.state, self.ok_at = "merge_across[%s]" % state, state, frozenset(ok_at)
        self.ok_at_plus = self.ok_at   # (behind the first digest partials come only more of them: one attempt per export and merge)

    def fill(self, dc, I):
        tb, _ = I.device()
        dc.push_device(tb.data_ptr(), None, tb.numel())
        assert dc.finish()["distinct"] == I.keys.size

    def build(self):
        I = inp()
        dc = mk_direct(I) if self.state == "a" else mk_part(I)
        st = {"I": I, "dcs": [dc]}
        dc.comm_init(1, 0, native.comm_unique_id())
        self.fill(dc, I)
        return st

    def call(self, st):
        info = native.KhMergeInfo()
        rc = lib().kh_merge_across(h(st["dcs"][0]), C.byref(info))
        st["info"] = native.merge_info_dict(info)
        return rc

    def ok(self, st):
        I = st["I"]
        assert st["info"]["owned_distinct"] == I.keys.size and st["info"]["conserved"] == 1, st["info"]
        table_is(st["dcs"][0], I)

    def failed(self, st, rc, tr, before):
        dc, I = st["dcs"][0], st["I"]
        assert rc == OOM and names_an_allocation(last_error(dc)), (rc, last_error(dc))
        msg = last_error(dc)
        rs = lib().kh_result_size(h(dc), 1, C.byref(C.c_uint64(0)))
        if "exchange" in msg or "region counts" in msg or "unit counts" in msg or "digests" in msg:
            assert rs == OK, (msg, "scratch of the exchange itself must not poison")      # (the header's one exception)
        else:
            assert rs in (OK, STATE), rs
        assert lib().kh_reset(h(dc)) == OK, last_error(dc)                                   # unspecified until kh_reset, whichever it was
        assert dc.finish()["distinct"] == 0
        self.fill(dc, I)
        assert self.call(st) == OK, last_error(dc)
        self.ok(st)


# State (a), a 16-byte table and no partition buffers: digests, send buffer, region counts, send counts (the exchange's own: KH_ERR_OOM
# without poisoning), merge_off and the scan scratch of the export (poisoning), three receive buffers, the region scratch of the merge
# -- 18 allocations, none with a fallback (wide pairs: the kernels take no digests).  State (b), the 8-byte image and idle partition
# buffers: the exchange BORROWS its scratch and the shard's table from them, so what is left are merge_off (1) and the scan scratch
# (2) of the export, and from 3 on the digest partials of merge.hip, which export and merge do without when they cannot have them.
# (exchange.hip's second attempt after release_part_buffers is not reached: it needs partition buffers of which nothing is lent, and
#  with such buffers the merge lends out the very first scratch it asks for.)
MERGE_OK_AT = {"a": [], "b": [3]}


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("state", ["a", "b"])
def test_merge_across_one_rank(tr, state, mode):
    sweep(tr, MergeAcross(state, MERGE_OK_AT[state]), mode)
