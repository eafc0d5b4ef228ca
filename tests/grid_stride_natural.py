"""The child process of tests/test_gpu_grid_stride.py::test_product_library_past_2048_tiles: one input per case that crosses 2048
tiles (or 524 288 items) of a capped-grid kernel on the PRODUCT library, against the oracle.  `python grid_stride_natural.py CASE`."""
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["KMERHIP_LIB"] = "libkmerhip.so"
os.environ.pop("KMERHIP_GRID_CAP", None)

import numpy as np  # noqa: E402

import oracle_lib as O  # noqa: E402
from krust_amd import native  # noqa: E402

U64 = np.uint64
GRID_CAP, BLOCK, RAW_TILE = 2048, 256, 4096
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
T0 = time.time()


def note(what):
    print(f"[{time.time() - T0:6.2f} s] {what}", flush=True)


def sorted_pairs(m):
    keys, counts = m.arrays()
    return np.asarray(keys, dtype=U64), np.asarray(counts, dtype=U64)


# ---- FASTA: 2051 whole tiles and five bytes, ragged lines, CR LF, a header across two tile edges, no final line end -----------------------------------
def fasta():
    import test_gpu_text as TX
    size = 8 * (1 << 20) + 12 * 1024 + 5
    assert size // RAW_TILE == 2051 > GRID_CAP and size % RAW_TILE == 5   # (2052 tiles: the last one holds five bytes)
    rng = np.random.default_rng(101)
    genome = ACGT[rng.integers(0, 4, size=200_000)].tobytes()   # lines are cut out of 200 kb: the table stays small
    eol = b"\r\n"
    out, n = [], 0

    def lines_until(target, close):
        """Lines of 1 .. 199 bases (every 400th a short header: a new record) up to exactly `target` bytes; the last line ends
        with a line end iff close."""
        nonlocal n
        i = 0
        while n < target:
            left = target - n
            if left < 600:                                # the last line takes what is left
                L = left - (2 if close else 0)
                s = int(rng.integers(0, len(genome) - L))
                piece = genome[s:s + L] + (eol if close else b"")
            elif i % 400 == 399:
                piece = b">r%d some text" % i + eol
            else:
                L = int(rng.integers(1, 200))
                s = int(rng.integers(0, len(genome) - L))
                piece = genome[s:s + L] + eol
            out.append(piece)
            n += len(piece)
            i += 1
        assert n == target, (n, target)

    out.append(b">first\r\n")
    n = len(out[0])
    h0 = 2047 * RAW_TILE + 1000
    lines_until(h0, close=True)
    header = b">" + TX.rand_seq(rng, 2 * RAW_TILE - 600, alphabet=b"ACGT >xyz|0123") + eol   # starts in tile 2047, ends in tile 2049
    out.append(header)
    n += len(header)
    assert h0 // RAW_TILE == 2047 and (n - 1) // RAW_TILE == 2049
    lines_until(size, close=False)
    text = b"".join(out)
    assert len(text) == size and not text.endswith(b"\n")
    note("text built")
    recs, _ = TX.parse_fasta(text)
    assert len(recs) > 100
    wk, wc = sorted_pairs(O.count_records(recs, 21))
    note(f"oracle: {wk.size} distinct")
    with native.DeviceCounter(21, capacity_hint=2 * wk.size) as dc:
        dc.push_text(text, "fasta")
        st = dc.finish()
        gk, gc = dc.result()
    assert st["kmers"] == int(wc.sum()) and np.array_equal(gk, wk) and np.array_equal(gc, wc)


# ---- FASTQ: 524 300 records of one or two bases ---------------------------------------------------------------------------------
def fastq():
    nrec = 524_300
    assert nrec > GRID_CAP * BLOCK
    rng = np.random.default_rng(103)
    alpha = np.frombuffer(b"ACGTN", dtype=np.uint8)
    two = rng.random(nrec) < 0.3
    b1, b2 = alpha[rng.integers(0, 5, size=nrec)], alpha[rng.integers(0, 5, size=nrec)]
    recs = [(b"@\n%c%c\n+\nII\n" % (x, y)) if t else (b"@\n%c\n+\nI\n" % x) for t, x, y in zip(two.tolist(), b1.tolist(), b2.tolist())]
    text = b"".join(recs)
    seqs = [r.split(b"\n")[1] for r in recs]
    m = O.OracleMap()
    m.process(b"\n".join(seqs), 1)
    wk, wc = sorted_pairs(m)
    note("oracle")
    assert int(wc.sum()) == int(((b1 != ord("N")).sum()) + (two & (b2 != ord("N"))).sum()) and wk.size == 2
    with native.DeviceCounter(1) as dc:
        dc.push_text(text, "fastq")
        st = dc.finish()
        gk, gc = dc.result()
        assert st["kmers"] == int(wc.sum()) and np.array_equal(gk, wk) and np.array_equal(gc, wc)
        # the same text with one record missing its '+': record 524 290, whose lane is in its second trip, and record 5, in the first
        # trip of a lane that makes a second one behind it (what the lane found must survive the rest of its loop)
        for at in (524_290, 5):
            assert at >= GRID_CAP * BLOCK or at + GRID_CAP * BLOCK < nrec
            bad = b"".join(recs[:at]) + recs[at].replace(b"\n+\n", b"\n-\n") + b"".join(recs[at + 1:])
            assert len(bad) == len(text)
            dc.reset()
            try:
                dc.push_text(bad, "fastq")
                raise AssertionError("the text without a '+' was accepted")
            except native.KmerHipError as e:
                assert e.status == native.KH_ERR_FORMAT
            assert dc.finish()["kmers"] == 0
            dc.push(b"ACGTACGT")
            assert dc.finish()["kmers"] == 8


# ---- graph_masks: 2 100 000 keys against a table of 50 000 -------------------------------------------------------------------------
def graph_masks():
    import test_gpu_graph as G
    import test_gpu_readside as RS
    import krust_amd
    k, nq = 21, 2_100_000
    assert (nq + 3) // 4 > GRID_CAP * BLOCK          # four keys per lane
    rng = np.random.default_rng(107)
    seq = ACGT[rng.integers(0, 4, size=50_000 + k - 1)]
    m = O.OracleMap()
    m.process(seq, k)
    keys, _ = sorted_pairs(m)
    assert 49_000 < keys.size <= 50_000
    absent = RS.draw_keys(krust_amd, k, 20_000, rng, avoid=keys)
    pool = np.concatenate((keys, absent, keys[:5000] | U64(1 << 63), G.np_revcomp(keys[5000:10_000], k)))
    pool_masks = G.np_masks(pool, keys, k)
    assert int((pool_masks != 0).sum()) > 40_000 and int((~G.np_valid(pool, k)).sum()) == 10_000
    pick = rng.integers(0, pool.size, size=nq)
    pick[-pool.size:] = np.arange(pool.size)[::-1]   # every word of the pool at least once; the array ends with the table's own keys
    second = 4 * GRID_CAP * BLOCK                    # the first key of the workgroups' second trip
    assert nq - second > 2000 and int((pool_masks[pick][second:] != 0).sum()) > 2000   # non-zero masks there: an unwritten tail shows
    note("numpy masks")
    with native.DeviceCounter(k) as dc:
        dc.push(seq)
        assert dc.finish()["distinct"] == keys.size
        got = dc.graph_masks(pool[pick], 1)
    bad = np.flatnonzero(got != pool_masks[pick])
    assert bad.size == 0, (bad[:8], got[bad[:8]], pool_masks[pick][bad[:8]])


# ---- unitigs of more than 524 288 nodes --------------------------------------------------------------------------------------------
def simple_path_unitigs(recs, k):
    """(rows, bases) when every record is a simple path of its own -- asserted from the oracle's counts at k and k - 1: every
    canonical k-mer and every canonical (k - 1)-mer of the records occurs once, and no (k - 1)-mer is its own reverse complement.
    Two nodes are neighbours iff they share a (k - 1)-mer, so the only links are those between consecutive windows of a record, every
    node has at most one neighbour per side, and none is its own.  The unitigs are then the records: read so that the end node with
    the smaller key comes first, in ascending order of that key."""
    import test_gpu_graph as G
    import test_gpu_unitigs as UN
    assert k % 2 == 1                                     # (no k-mer is its own reverse complement)
    flat = UN.flat_of(recs)
    for kk in (k, k - 1):
        m = O.OracleMap()
        m.process(flat, kk)
        keys, counts = sorted_pairs(m)
        windows = sum(len(r) - kk + 1 for r in recs)
        assert keys.size == windows and int(counts.max()) == 1, (kk, keys.size, windows)
        if kk == k - 1:
            assert not (keys == G.np_revcomp(keys, kk)).any()
    out = []
    for r in recs:
        a, b = UN.canon(r[:k]), UN.canon(r[-k:])
        L = len(r) - k + 1
        seq = a if L == 1 else (r if a < b else UN.rc(r))
        out.append((min(a, b), seq, L))
    out.sort()
    rows = np.zeros((len(out), 4), dtype=U64)
    start = 0
    for i, (_, seq, L) in enumerate(out):
        rows[i] = (start, L, L, 0)
        start += len(seq)
    return flat, rows, b"".join(s for _, s, _ in out)


def unitigs():
    import test_gpu_unitigs as UN
    k = 31
    rng = np.random.default_rng(109)
    rs = lambda n: ACGT[rng.integers(0, 4, size=n)].tobytes()
    # the shortcut against the string walk, on a twin of a fiftieth of the size
    small = [rs(10_600)] + [rs(int(rng.integers(31, 61))) for _ in range(60)]
    sflat, srows, sbases = simple_path_unitigs(small, k)
    skeys, scounts = UN.oracle_pairs(sflat, k)
    ref = UN.Ref(UN.node_dict(skeys, scounts, k, 1), k)
    assert np.array_equal(ref.rows, srows) and ref.bases == sbases and ref.seen["minus_first"] > 0
    note("shortcut == string walk on the small twin")
    recs = [rs(530_000)] + [rs(int(rng.integers(31, 61))) for _ in range(3000)]
    flat, rows, bases = simple_path_unitigs(recs, k)
    n = int(rows[:, 1].sum())
    assert n > GRID_CAP * BLOCK and rows.shape[0] == 3001
    note(f"expected unitigs of {n} nodes")
    with native.DeviceCounter(k, capacity_hint=2 * n) as dc:
        dc.push(flat)
        assert dc.finish()["distinct"] == n
        grows, gbases = dc.unitigs(1)
    assert grows.shape == rows.shape and np.array_equal(grows, rows), np.argwhere(grows != rows)[:4]
    assert gbases.tobytes() == bases


if __name__ == "__main__":
    assert native.LIB_PATH.endswith("libkmerhip.so"), native.LIB_PATH
    {"fasta": fasta, "fastq": fastq, "graph_masks": graph_masks, "unitigs": unitigs}[sys.argv[1]]()
    note("done")
    print("RESULT ok", native.LIB_PATH)
