"""Level 2's arena kernel (krust_amd/csrc/partition.hip.h part2_arena_kernel) after its instruction diet: a wave loads whole pool
chunks 16 bytes a lane, the bucket counters count bytes, a flush writes its units in straight-line steps with the arena-full
path behind one test per bucket.  What the kernel leaves behind must be what it always was, so every case is an exact
comparison of result(), histogram() and the k-mer total with the CPU oracle, through the testing library and the partition
path: chunks that are not full (every fill residue mod 4, 4- and 8-byte payloads, narrowing), partitions of one, two and three
batches (the two register sets of the prefetch, a short last batch), every instance of the kernel (512 / 768 / 1024 buckets,
shift and multiply-add addresses), and a bucket heavy enough to overrun its bin and its arena."""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

SEED = 20260130
NCPU = 16
_READS = {}
_WANT = {}


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import krust_amd
    krust_amd.lib()  # ImportError if the HIP extension is missing: no silent fallback
    return krust_amd


def _reads(n_reads):
    """The first n_reads of one stream of synthetic 150-base reads (shared, never written to)."""
    if n_reads not in _READS:
        bases, _ = O.synth_reads(SEED + 77, 1 << 22, 150, 0, n_reads, with_qual=False)
        bases.setflags(write=False)
        _READS[n_reads] = bases
    return _READS[n_reads]


def _oracle(tag, bases, k):
    """(total, keys, counts, histogram) of the oracle for these bases, computed once per (input, k)."""
    if (tag, k) not in _WANT:
        m = O.OracleMap()
        total = m.scan_flat(bases, k, nthreads=NCPU)
        keys, cnts = m.arrays()
        _WANT[(tag, k)] = (total, keys, cnts, m.histogram())
    return _WANT[(tag, k)]


def _check(dc, st, want):
    total, want_k, want_c, want_h = want
    assert st["kmers"] == total and st["distinct"] == len(want_k)
    keys, cnts = dc.result()
    assert np.array_equal(keys, want_k) and np.array_equal(cnts, want_c)
    assert dc.histogram() == want_h


def _took_the_arena_kernel(st):
    assert st["stage_ms"]["level2"] > 0 and st["stage_ms"]["level2_count"] == 0, st["stage_ms"]


@pytest.mark.parametrize("k", [21, 22, 31])
def test_partly_filled_chunks(K, k):
    """Batches of 1, 2, 3, 5, 700 and 20,000 reads into one counter: 130 to 2.6 M payloads over 1024 partitions, so every chunk of
    the small batches holds 1..255 payloads, with fills of every residue mod 4 -- the checked form of the load, whose `have` mask
    is per payload of a lane's group of four.  k = 21: 4-byte chunks; 22: 8-byte chunks narrowed to 4-byte bins; 31: 8 bytes
    throughout.  1024 x 32 regions: the 512-bucket instance with shift addresses."""
    import torch
    pieces = [1, 2, 3, 5, 700, 20_000]
    bases = _reads(sum(pieces))
    want = _oracle("pieces", bases, k)
    tb = torch.from_numpy(bases.copy()).cuda()
    torch.cuda.synchronize()
    with K.DeviceCounter(k, capacity_hint=50_000_000, path="partition") as dc:
        at = 0
        for n in pieces:
            dc.push_device(tb.data_ptr() + at * 151, None, n * 151)
            at += n
        st = dc.finish()
        assert st["table_slots"] == 1 << 27
        _took_the_arena_kernel(st)
        _check(dc, st, want)


@pytest.mark.parametrize("k", [21, 31])
@pytest.mark.parametrize("n_reads", [140_000, 270_000])
def test_more_than_one_batch_per_partition(K, n_reads, k):
    """One push of 140,000 reads: ~69 chunks per partition -- one full batch of 64 (4-byte payloads; two of 32 for 8-byte ones) and
    a tail; of 270,000: three batches (five), the prefetch's two register sets through their odd case, a short last batch."""
    import torch
    bases = _reads(n_reads)
    want = _oracle(n_reads, bases, k)
    tb = torch.from_numpy(bases.copy()).cuda()
    torch.cuda.synchronize()
    with K.DeviceCounter(k, capacity_hint=50_000_000, path="partition") as dc:
        dc.push_device(tb.data_ptr(), None, tb.numel())
        st = dc.finish()
        _took_the_arena_kernel(st)
        _check(dc, st, want)


@pytest.mark.parametrize("k", [21, 25])
@pytest.mark.parametrize("b2", [32, 40, 640, 1000, 1024])
def test_every_instance(K, monkeypatch, b2, k):
    """1024 x {32, 40, 640, 1000, 1024} regions: the 512-bucket instance with shift and with multiply-add addresses, the 768-bucket
    one, and both 1024-bucket ones; k = 21 (4-byte payloads) and 25 (8-byte, narrowed where the bucket count is a power of two).
    The stage times say that the arena kernel took the batch."""
    import torch
    monkeypatch.setenv("KMERHIP_TABLE_REGIONS", str(1024 * b2))
    n_reads = 200_000 if b2 >= 640 else 60_000
    bases = _reads(n_reads)
    want = _oracle(n_reads, bases, k)
    tb = torch.from_numpy(bases.copy()).cuda()
    torch.cuda.synchronize()
    with K.DeviceCounter(k, capacity_hint=len(want[1]), path="partition") as dc:
        dc.push_device(tb.data_ptr(), None, tb.numel())
        st = dc.finish()
        assert st["table_slots"] == 1024 * b2 * 4096, st
        _took_the_arena_kernel(st)
        _check(dc, st, want)


@pytest.mark.parametrize("k", [21, 31])
def test_a_heavy_bucket(K, k):
    """3,000 copies of one read among 60,000 others: its buckets overrun their bins between two flushes (ranks beyond the bin, found
    by the one test per half batch) and then their arenas (the arena-full form of the flush, out of line); all of it reaches
    the table through the overflow list."""
    import torch
    base = _reads(60_000)
    bases = np.concatenate([base, np.tile(base[:151], 3000)])
    want = _oracle("heavy", bases, k)
    tb = torch.from_numpy(bases).cuda()
    torch.cuda.synchronize()
    with K.DeviceCounter(k, capacity_hint=50_000_000, path="partition") as dc:
        dc.push_device(tb.data_ptr(), None, tb.numel())
        st = dc.finish()
        _took_the_arena_kernel(st)
        _check(dc, st, want)
