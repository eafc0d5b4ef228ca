"""GPU tests of the device-side output path: kh_result_text_begin / _next / _next_device (krust_amd/csrc/format.hip) and the
command line that streams it.  Expected values come from the oracle (tests/oracle_lib.py) and from strings built here in
Python from the formats of the reference's output_counts (src/run.rs:441-486) -- never from kh_result_copy + kh_unpack."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
FORMATS = ("fasta", "tsv", "json")


# ---- the formats, restated in Python ------------------------------------------------------------------------------------
def record(fmt, kmer, count, first=False):
    if fmt == "fasta":
        return f">{count}\n{kmer}\n".encode()
    if fmt == "tsv":
        return f"{kmer}\t{count}\n".encode()
    return (("[\n" if first else ",\n") + f'  {{\n    "kmer": "{kmer}",\n    "count": {count}\n  }}').encode()


def split_records(fmt, text):
    """The records of a whole document, each in the form record(fmt, .., first=False) gives; checks the framing."""
    if fmt == "fasta":
        lines = text.split(b"\n")
        assert lines[-1] == b"" and len(lines) % 2 == 1
        return [lines[i] + b"\n" + lines[i + 1] + b"\n" for i in range(0, len(lines) - 1, 2)]
    if fmt == "tsv":
        assert text == b"" or text.endswith(b"\n")
        return [l + b"\n" for l in text.split(b"\n")[:-1]]
    if text == b"[]\n":
        return []
    assert text.startswith(b"[\n  {\n") and text.endswith(b"\n  }\n]\n"), (text[:40], text[-40:])
    body = b",\n" + text[2:-3]
    parts = body.split(b",\n  {\n")
    assert parts[0] == b""
    return [b",\n  {\n" + p for p in parts[1:]]


def parse(fmt, text):
    """text -> {kmer: count}; every record must be exactly the bytes record() builds from what it parses to."""
    out = {}
    for rec in split_records(fmt, text):
        if fmt == "fasta":
            c, km = rec[1:-1].split(b"\n")
        elif fmt == "tsv":
            km, c = rec[:-1].split(b"\t")
        else:
            d = json.loads(rec[2:])
            assert list(d) == ["kmer", "count"]
            km, c = d["kmer"].encode(), d["count"]
        km = km.decode()
        assert km not in out
        out[km] = int(c)
        assert rec == record(fmt, km, out[km]), rec
    if fmt == "json":
        assert json.loads(text) == [{"kmer": k, "count": c} for k, c in out.items()]
    return out


def expected_records(fmt, d, min_count=1):
    return sorted(record(fmt, km, c) for km, c in d.items() if c >= min_count)


def empty_doc(fmt):
    return b"[]\n" if fmt == "json" else b""


def ends_at_record_end(fmt, piece, last):
    if fmt == "json":
        return piece.endswith(b"\n]\n") or piece == b"[]\n" if last else piece.endswith(b"\n  }")
    return piece.endswith(b"\n")


def fetch(dc, fmt, min_count=1, cap=1 << 20, device=False):
    """(n_records, n_bytes, pieces) of one whole stream, every piece fetched with room for `cap` bytes."""
    import torch
    nr, nb = dc.result_text_begin(fmt, min_count)
    pieces = []
    buf = torch.empty(cap + 7, dtype=torch.uint8, device="cuda:0")[7:] if device else np.empty(cap, dtype=np.uint8)  # (device: an unaligned start)
    while True:
        n = dc.result_text_device(buf) if device else dc.result_text_next(buf)
        if n == 0:
            break
        assert n <= cap
        pieces.append(bytes(buf[:n].cpu().numpy()) if device else buf[:n].tobytes())
    return nr, nb, pieces


def random_reads(seed, n=400, maxlen=180):
    rng = np.random.default_rng(seed)
    alpha = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)
    return [alpha[rng.choice(9, size=int(rng.integers(1, maxlen)), p=[.22, .22, .22, .22, .03, .03, .02, .02, .02])].tobytes() for _ in range(n)]


def flat(recs):
    return np.frombuffer(b"".join(r + b"\n" for r in recs), dtype=np.uint8).copy()


# ---- formats and table forms --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 11, 13, 21, 22, 31, 32])
@pytest.mark.parametrize("path", ["direct", "partition"])
def test_formats_on_both_table_forms(k, path):
    import krust_amd
    reads = random_reads(1000 + k, n=1500 if path == "partition" else 400)
    want = O.count_records(reads, k).as_str_dict(k)
    # (a table of 2^11 regions: at k = 21 the 32 hash bits below the level-1 digit fit the 8-byte image, tests/test_gpu_parity.py)
    with krust_amd.DeviceCounter(k, path=path, capacity_hint=3_000_000) as dc:
        dc.push(flat(reads))
        st = dc.finish()
        print(f"k={k} {path}: slot_bytes {st['slot_bytes']}, part_batches {st['part_batches']}, {len(want)} keys")
        if path == "direct":
            assert st["slot_bytes"] == 16 and st["part_batches"] == 0
        elif k <= 16 or k == 21:   # the 8-byte image, where it applies: the 2k hash bits below the level-1 digit fit 32
            assert st["slot_bytes"] == 8 and st["part_batches"] >= 1
        top = max(want.values())
        for fmt in FORMATS:
            for mc in (1, 2, top + 1):
                nr, nb, pieces = fetch(dc, fmt, mc)
                text = b"".join(pieces)
                assert len(text) == nb and nr == sum(1 for c in want.values() if c >= mc)
                got = parse(fmt, text)
                assert got == {km: c for km, c in want.items() if c >= mc}, (fmt, mc)
                assert sorted(split_records(fmt, text)) == expected_records(fmt, want, mc)
                if mc == top + 1:
                    assert text == empty_doc(fmt)
        assert dc.finish()["slot_bytes"] == st["slot_bytes"]  # (streaming converts nothing)


def test_table_never_pushed_to():
    import krust_amd
    with krust_amd.DeviceCounter(21) as dc:
        for fmt in FORMATS:
            nr, nb, pieces = fetch(dc, fmt)
            assert nr == 0 and b"".join(pieces) == empty_doc(fmt) and nb == len(empty_doc(fmt))


# ---- piece independence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", FORMATS)
def test_pieces_are_independent_of_cap(fmt):
    import krust_amd
    k = 21
    reads = random_reads(77, n=1500)
    want = O.count_records(reads, k).as_str_dict(k)
    with krust_amd.DeviceCounter(k) as dc:
        dc.push(flat(reads))
        dc.finish()
        nr, nb, one = fetch(dc, fmt, cap=64 << 20)
        whole = b"".join(one)
        assert len(one) == 1 and len(whole) == nb and nb > (1 << 20) + 3 and parse(fmt, whole) == want
        largest = max(len(r) for r in split_records(fmt, whole)) + (2 if fmt == "json" else 0)
        for cap, device in ((largest, False), (4096, False), ((1 << 20) + 3, False), (64 << 20, False),
                            (4096, True), ((1 << 20) + 3, True), (64 << 20, True)):
            _, nb2, pieces = fetch(dc, fmt, cap=cap, device=device)
            assert nb2 == nb and b"".join(pieces) == whole, (cap, device)
            assert all(ends_at_record_end(fmt, p, i == len(pieces) - 1) for i, p in enumerate(pieces)), (cap, device)
            if cap == largest:
                assert len(pieces) >= nr // 2
        # a cap below any record: KH_ERR_RANGE, nothing consumed, and the stream goes on
        dc.result_text_begin(fmt)
        buf = np.empty(1 << 20, dtype=np.uint8)
        n0 = dc.result_text_next(buf)
        with pytest.raises(krust_amd.KmerHipError) as ei:
            dc.result_text_next(buf[:8])
        assert ei.value.status == krust_amd.native.KH_ERR_RANGE
        rest = [buf[:n0].tobytes()]
        while True:
            n = dc.result_text_next(buf)
            if n == 0:
                break
            rest.append(buf[:n].tobytes())
        assert b"".join(rest) == whole
        # the generator of the binding, and pinned memory
        assert b"".join(dc.result_text(fmt, piece_bytes=300_000)) == whole
        with krust_amd.native.PinnedArray(1 << 20) as pa:
            dc.result_text_begin(fmt)
            got = []
            while True:
                n = dc.result_text_next(pa.array)
                if n == 0:
                    break
                got.append(pa.array[:n].tobytes())
            assert b"".join(got) == whole


# ---- large counts -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [5, 31])
def test_large_counts_have_exact_digits(k):
    import krust_amd
    reads = random_reads(5 + k, n=200)
    m = O.count_records(reads, k)
    want = m.as_str_dict(k)
    big = [2**32 + 5, 10**19, 2**64 - 1]
    keys = sorted(m.as_dict())
    fresh = [krust_amd.canonical(x, k)[0] for x in (0, 4**k // 3, 4**k // 7)]
    fresh = [x for x in dict.fromkeys(fresh) if x not in set(keys)] if k == 31 else []
    targets = (fresh + keys)[:3]
    with krust_amd.DeviceCounter(k) as dc:
        dc.push(flat(reads))
        dc.merge_pairs(np.array(targets, dtype=np.uint64), np.array([b - m.get(t) for b, t in zip(big, targets)], dtype=np.uint64))
        for t, b in zip(targets, big):
            want[O.unpack(t, k)] = b
        dc.finish()
        for fmt in FORMATS:
            nr, nb, pieces = fetch(dc, fmt)
            text = b"".join(pieces)
            assert parse(fmt, text) == want and nr == len(want)
            for b in big:
                assert str(b).encode() in text
        assert parse("tsv", b"".join(fetch(dc, "tsv", 2**32)[2])) == {km: c for km, c in want.items() if c >= 2**32}


# ---- state --------------------------------------------------------------------------------------------------------------
def test_stream_state():
    import krust_amd
    k = 13
    reads = random_reads(9, n=3000)
    want = O.count_records(reads, k).as_str_dict(k)
    STATE = krust_amd.native.KH_ERR_STATE
    buf = np.empty(4096, dtype=np.uint8)
    with krust_amd.DeviceCounter(k) as dc:
        with pytest.raises(krust_amd.KmerHipError) as ei:
            dc.result_text_next(buf)                       # next without begin
        assert ei.value.status == STATE
        dc.push(flat(reads))
        dc.finish()
        whole = b"".join(fetch(dc, "tsv", cap=4096)[2])
        assert parse("tsv", whole) == want
        # reads between the pieces leave the stream intact
        dc.result_text_begin("tsv")
        got, i = [], 0
        some = np.array([O.pack(km.encode()) for km in list(want)[:50]], dtype=np.uint64)
        while True:
            n = dc.result_text_next(buf)
            if n == 0:
                break
            got.append(buf[:n].tobytes())
            i += 1
            if i % 3 == 0:
                assert dc.result_size() == len(want)
                assert dc.lookup(some).tolist() == [want[O.unpack(int(x), k)] for x in some]
            if i == 5:
                assert sum(c * f for c, f in dc.histogram()) == sum(want.values())
        assert b"".join(got) == whole
        # a push ends the stream; a new begin starts one over the new table
        dc.result_text_begin("tsv")
        assert dc.result_text_next(buf) > 0
        dc.push(flat(reads))
        with pytest.raises(krust_amd.KmerHipError) as ei:
            dc.result_text_next(buf)
        assert ei.value.status == STATE
        assert parse("tsv", b"".join(fetch(dc, "tsv")[2])) == {km: 2 * c for km, c in want.items()}
        dc.result_text_begin("fasta")
        dc.reset()
        with pytest.raises(krust_amd.KmerHipError) as ei:
            dc.result_text_next(buf)
        assert ei.value.status == STATE
        L = krust_amd.lib()                                 # no such format
        assert L.kh_result_text_begin(dc._h, 7, 1, None, None) == krust_amd.native.KH_ERR_BAD_ARG
        assert L.kh_result_text_begin(dc._h, 0, 1, None, None) == krust_amd.native.KH_ERR_BAD_ARG


def test_readers_between_pieces_on_a_partitioned_table():
    """After a partitioned count the chunks live in the idle partition buffers: a formatted chunk (and the one formatted
    ahead of it) must survive the read-only calls made between two pieces."""
    import krust_amd
    k = 21
    reads = random_reads(4242, n=1500)
    want = O.count_records(reads, k).as_str_dict(k)
    with krust_amd.DeviceCounter(k, path="partition", capacity_hint=3_000_000) as dc:
        dc.push(flat(reads))
        st = dc.finish()
        assert st["part_batches"] >= 1 and st["slot_bytes"] == 8
        some = np.array([O.pack(km.encode()) for km in list(want)[:200]], dtype=np.uint64)
        some_counts = [want[O.unpack(int(x), k)] for x in some]
        for fmt, cap in (("fasta", 4096), ("json", 100_000), ("tsv", 1 << 20)):
            whole = b"".join(fetch(dc, fmt, cap=64 << 20)[2])
            assert parse(fmt, whole) == want
            dc.result_text_begin(fmt)
            buf = np.empty(cap, dtype=np.uint8)
            got, i = [], 0
            while True:
                n = dc.result_text_next(buf)
                if n == 0:
                    break
                got.append(buf[:n].tobytes())
                i += 1
                if i % 7 == 1:
                    assert dc.result_size() == len(want) and dc.result_size(2) == sum(1 for c in want.values() if c >= 2)
                    assert dc.lookup(some).tolist() == some_counts
                if i % 50 == 2:
                    assert sum(c * f for c, f in dc.histogram()) == sum(want.values())
                    assert dc.finish()["distinct"] == len(want)
            assert i >= 2 and b"".join(got) == whole, (fmt, cap)


@pytest.mark.parametrize("k", [9, 21])
def test_shards_after_a_two_rank_merge_stream(k):
    import krust_amd
    reads = random_reads(31 + k, n=2000)
    want = O.count_records(reads, k).as_str_dict(k)
    half = len(reads) // 2
    with krust_amd.DeviceGroup(k, [0, 0]) as g:
        g[0].push(flat(reads[:half]))
        g[1].push(flat(reads[half:]))
        g.merge()
        for fmt in FORMATS:
            got = {}
            for r in range(2):
                nr, nb, pieces = fetch(g[r], fmt, cap=1 << 18)
                d = parse(fmt, b"".join(pieces))
                assert len(d) == nr and not (set(d) & set(got))
                got.update(d)
            assert got == want, fmt


# ---- the product library ------------------------------------------------------------------------------------------------
CHILD = r'''
import os, sys
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import krust_amd
from krust_amd import native
import oracle_lib as O
import test_gpu_format as T
assert native.LIB_PATH.endswith("libkmerhip.so"), native.LIB_PATH
bases, _ = O.synth_reads(20260130, 1 << 20, 150, 0, 60_000, with_qual=False)
m = O.OracleMap()
m.scan_flat(bases, 21, nthreads=4)
want = m.as_str_dict(21)
with krust_amd.DeviceCounter(21) as dc:
    dc.push(bases)
    st = dc.finish()
    for fmt in T.FORMATS:
        nr, nb, pieces = T.fetch(dc, fmt, cap=3 << 20)
        text = b"".join(pieces)
        assert nr == len(want) and nb == len(text) and T.parse(fmt, text) == want, fmt
print("RESULT ok slot_bytes=%d" % st["slot_bytes"])
'''


def test_product_library_streams_text():
    env = dict(os.environ)
    env.pop("KMERHIP_LIB", None)
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + CHILD], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]


# ---- at size ------------------------------------------------------------------------------------------------------------
def test_two_million_reads_tsv():
    import torch
    import krust_amd
    n, rl, k = 2_000_000, 150, 21
    tb = torch.empty(n * (rl + 1), dtype=torch.uint8, device="cuda:0")
    krust_amd.synth_reads_device(tb.data_ptr(), None, 20260207, 1 << 22, rl, 0, n, device=0)
    torch.cuda.synchronize()
    with krust_amd.DeviceCounter(k, device=0) as dc:
        dc.push_device(tb.data_ptr(), None, tb.numel())
        st = dc.finish()
        t0 = time.time()
        nr, nb = dc.result_text_begin("tsv")
        assert nr == dc.result_size() == st["distinct"]
        with krust_amd.native.PinnedArray(64 << 20) as pa:
            chunks = []
            while True:
                got = dc.result_text_next(pa.array)
                if got == 0:
                    break
                chunks.append(pa.array[:got].copy())
        print(f"[at size] {nr} records, {nb} bytes of tsv in {time.time() - t0:.3f} s, slot_bytes {st['slot_bytes']}")
        text = np.concatenate(chunks)
        assert text.size == nb
        nl = np.flatnonzero(text == 10)
        assert nl.size == nr
        tabs = np.flatnonzero(text == 9)
        assert tabs.size == nr and np.all(tabs < nl) and np.all(tabs - np.concatenate(([-1], nl[:-1])) - 1 == k)
        # the counts parsed back: digits between each tab and its newline
        total = 0
        width = nl - tabs - 1
        for w in np.unique(width):
            idx = np.flatnonzero(width == w)
            digs = text[tabs[idx, None] + 1 + np.arange(w)[None, :]].astype(np.int64) - 48
            assert digs.min() >= 0 and digs.max() <= 9
            total += int((digs * (10 ** np.arange(w - 1, -1, -1, dtype=np.int64))[None, :]).sum())
        assert total == st["kmers"]
        # a 1/64 sample of the records against kh_lookup
        sel = np.arange(0, nr, 64)
        starts = np.concatenate(([0], nl[:-1] + 1))[sel]
        kmers = text[starts[:, None] + np.arange(k)[None, :]]
        code = ((kmers >> 1) ^ (kmers >> 2)) & 3
        keys = (code.astype(np.uint64) << (2 * np.arange(k - 1, -1, -1, dtype=np.uint64))[None, :]).sum(axis=1, dtype=np.uint64)
        cnts = np.array([int(bytes(text[t + 1:e])) for t, e in zip(tabs[sel], nl[sel])], dtype=np.uint64)
        assert np.array_equal(dc.lookup(keys), cnts)


# ---- the command line ---------------------------------------------------------------------------------------------------
def run_cli(*args, env=None):
    e = {**os.environ, "KMERUST_TIMING": "1", **(env or {})}
    r = subprocess.run([BIN, *args], capture_output=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    tline = [l for l in r.stderr.splitlines() if l.startswith(b'{"kmerust_timing"')][-1]
    return r.stdout, json.loads(tline)["kmerust_timing"]


def file_records(path):
    recs, cur = [], None
    with open(path, "rb") as f:
        lines = f.read().split(b"\n")
    if path.endswith(".fq"):
        return [lines[i + 1] for i in range(0, len(lines) - 1, 4)]
    for l in lines:
        if l.startswith(b">"):
            if cur is not None:
                recs.append(cur)
            cur = b""
        elif cur is not None:
            cur += l
    return recs + ([cur] if cur is not None else [])


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    from test_gpu_cli import _write_reads
    fq, fa = _write_reads(tmp_path_factory.mktemp("format_cli"))
    return [(os.path.join(ROOT, "tests", "fixtures", "simple.fa"), 3), (fq, 21), (fa, 32)]


@pytest.mark.parametrize("fmt", FORMATS)
def test_cli_streams_device_text(inputs, fmt, tmp_path):
    for path, k in inputs:
        want = O.count_records(file_records(path), k).as_str_dict(k)
        for extra in ([], ["--min-count", "2"], ["--save", str(tmp_path / "x.kmix")]):
            args = [str(k), path, "--format", fmt, "-q"] + extra
            mc = 2 if "--min-count" in extra else 1
            dev, tdev = run_cli(*args)
            host, thost = run_cli(*args, env={"KMERUST_HOST_FORMAT": "1"})
            assert tdev["writer"] == "device" and thost["writer"] == "host", (tdev, thost)
            exp = expected_records(fmt, want, mc)
            assert sorted(split_records(fmt, dev)) == sorted(split_records(fmt, host)) == exp, (path, extra)
            assert parse(fmt, dev) == {km: c for km, c in want.items() if c >= mc}
            if "--save" in extra:
                from test_gpu_cli import run as cli_run
                km = next(iter(want))
                q = cli_run("query", str(tmp_path / "x.kmix"), km)
                assert q.returncode == 0 and q.stdout.strip() == str(want[km]).encode()


def test_cli_default_format_is_device_fasta(inputs):
    path, k = inputs[1]
    out, t = run_cli(str(k), path, "-q")
    assert t["writer"] == "device" and parse("fasta", out) == O.count_records(file_records(path), k).as_str_dict(k)


def test_cli_several_ranks(inputs):
    path, k = inputs[1]
    one, _ = run_cli(str(k), path, "--format", "tsv", "-q")
    three, t3 = run_cli(str(k), path, "--format", "tsv", "-q", "--devices", "0,0,0")
    assert t3["writer"] == "device" and sorted(one.splitlines()) == sorted(three.splitlines()) and one
    fa3, tf = run_cli(str(k), path, "-q", "--devices", "0,0")
    assert tf["writer"] == "device" and parse("fasta", fa3) == parse("tsv", one)
    js, tj = run_cli(str(k), path, "--format", "json", "-q", "--devices", "0,0")
    assert tj["writer"] == "host" and parse("json", js) == parse("tsv", one)


def test_cli_fails_when_the_output_cannot_be_written(inputs):
    """A full disk: the streamed text must not end as a shorter output with exit status 0 (small texts take one pageable
    buffer, larger ones the pinned buffers and the writer thread)."""
    if not os.path.exists("/dev/full"):
        pytest.fail("/dev/full is needed for this test")
    for path, k in inputs[:2]:
        with open("/dev/full", "wb") as full:
            r = subprocess.run([BIN, str(k), path, "-q"], stdout=full, stderr=subprocess.PIPE, timeout=300)
        assert r.returncode == 1 and b"failed to write the output" in r.stderr, (path, r.returncode, r.stderr[-500:])
