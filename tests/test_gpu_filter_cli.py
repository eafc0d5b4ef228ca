"""The command line over kh_profile_records: `kmerust query --sequences -f summary` with the reduction on the device and on the host
(KMERUST_HOST_SUMMARY=1: the route before kh_profile_records) print the same bytes, those of the oracle; `kmerust filter` keeps
the records the oracle's table says it should, as they were read, in input order."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import profile_expect as E

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
K = 21
BATCH = ["--__batch-kb", "16"]   # (hidden, as __parse: several reader batches)


def _run(*args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    return subprocess.run([BIN, *args], capture_output=True, timeout=300, env=e)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """An index of 600 reads (the first 150 twice: counts of 2 and more) and 400 query records: counted ones, others, dirty ones."""
    d = tmp_path_factory.mktemp("filter_cli")
    b, q = O.synth_reads(31, 1 << 16, 150, 0, 900)
    split = lambda a: [bytes(x) for x in np.asarray(a).tobytes().split(b"\n")[:-1]]
    recs, quals = split(b), split(q)
    counted = recs[:600] + recs[:150]
    query = recs[100:200] + recs[560:840] + [b"ACGTN", b"", b"acgtacgtacgtacgtacgtacgtacgtt", recs[3][:40] + b"NNNN" + recs[4][:50], recs[5][:K]]
    qq = quals[100:200] + quals[560:840] + [b"IIIII", b"", b"I" * 29, b"I" * 94, b"#" * K]
    # a few records whose first half is counted twice and whose second half is not counted at all (the fraction rule's ground)
    for i in range(12):
        query.append(recs[i][:75 + i] + recs[850 + i][:75 - i])
        qq.append(quals[i][:75 + i] + quals[850 + i][:75 - i])
    src = d / "counted.fa"
    src.write_bytes(b"".join(b">c%d\n%s\n" % (i, r) for i, r in enumerate(counted)))
    idx = d / "idx.kmix"
    r = _run(str(K), str(src), "--save", str(idx), "-q")
    assert r.returncode == 0, r.stderr
    headers = [b"r%d some text/%d" % (i, i % 2 + 1) for i in range(len(query))]
    fa, fq, gz = d / "query.fa", d / "query.fq", d / "query.fq.gz"
    # (FASTA sequence lines wrap at 60 columns: the reader joins them)
    fa.write_bytes(b"".join(b">%s\n%s" % (h, b"".join(s[i:i + 60] + b"\n" for i in range(0, max(len(s), 1), 60))) for h, s in zip(headers, query)))
    fq_bytes = b"".join(b"@%s\n%s\n+\n%s\n" % (h, s, ql) for h, s, ql in zip(headers, query, qq))
    fq.write_bytes(fq_bytes)
    gz.write_bytes(gzip.compress(fq_bytes))
    m = O.count_records(counted, K)
    return dict(idx=str(idx), fa=str(fa), fq=str(fq), gz=str(gz), m=m, query=query, qq=qq, headers=headers)


_PROFILES = {}


def _rows(data, lo, hi, minq=None):
    """Row by row from the oracle's profile of every record (computed once per quality threshold, shared by the tests)."""
    if minq not in _PROFILES:
        _PROFILES[minq] = [E.oracle_profile(s + b"\n", K, data["m"], (ql + b"\n") if minq is not None else None, minq)
                           for s, ql in zip(data["query"], data["qq"])]
    return np.array([E.rows_of(P, [0, P.size], lo, hi)[0] for P in _PROFILES[minq]])


def _fasta(h, s):
    return b">%s\n%s\n" % (h, s)


def _fastq(h, s, ql):
    return b"@%s\n%s\n+\n%s\n" % (h, s, ql)


def test_summary_from_the_device_and_from_the_host_are_the_same_bytes(data):
    for path, minq in ((data["fa"], None), (data["fq"], 20), (data["gz"], None)):
        rows = _rows(data, 1, E.SAT, minq)
        want = b"".join(b"%d\t%d\t%d\t%d\t%d\t%d\n" % (i, r[E.WINDOWS], r[E.PRESENT], r[E.MIN], r[E.MAX], int(r[E.SUM_LO]) | (int(r[E.SUM_HI]) << 32))
                        for i, r in enumerate(rows))
        args = ["query", data["idx"], "--sequences", path, "-q", *BATCH] + (["-Q", str(minq)] if minq is not None else [])
        dev = _run(*args)
        host = _run(*args, env={"KMERUST_HOST_SUMMARY": "1"})
        assert dev.returncode == 0 and host.returncode == 0, (dev.stderr, host.stderr)
        assert dev.stdout == host.stdout, path
        assert dev.stdout == want, (path, dev.stdout[:200], want[:200])
    assert len(want) > 0 and os.path.getsize(data["fa"]) > 3 * (16 << 10)


@pytest.mark.parametrize("opts,lo,hi,n,f,minq", [([], 1, E.SAT, 1, 0.0, None),
                                                 (["--min-count", "2", "--max-count", "5", "--min-fraction", "0.5"], 2, 5, 1, 0.5, None),
                                                 (["-Q", "20"], 1, E.SAT, 1, 0.0, 20),
                                                 (["--min-kmers", "100", "--min-count=2"], 2, E.SAT, 100, 0.0, None)])
def test_filter_keeps_what_the_oracle_table_says(data, opts, lo, hi, n, f, minq):
    for kind in ("fa", "fq", "gz"):
        fastq = kind != "fa"
        rows = _rows(data, lo, hi, minq if fastq else None)      # (-Q is ignored for FASTA input)
        keep = [bool(r[E.WINDOWS] > 0 and r[E.IN_RANGE] >= n and float(r[E.IN_RANGE]) >= f * float(r[E.WINDOWS])) for r in rows]
        assert 0 < sum(keep) < len(keep), "the case decides nothing"
        text = [_fastq(h, s, ql) if fastq else _fasta(h, s) for h, s, ql in zip(data["headers"], data["query"], data["qq"])]
        plain = _run("filter", data["idx"], data[kind], *opts, *BATCH)
        inv = _run("filter", data["idx"], data[kind], *opts, "-v", "-q", *BATCH)
        assert plain.returncode == 0 and inv.returncode == 0, (plain.stderr, inv.stderr)
        assert plain.stdout == b"".join(t for t, kp in zip(text, keep) if kp), (kind, opts)
        assert inv.stdout == b"".join(t for t, kp in zip(text, keep) if not kp), (kind, opts)
        # {records}\t{kept} closes stderr unless -q; -v and the plain output partition the input, in order
        assert plain.stderr.endswith(b"\n%d\t%d\n" % (len(keep), sum(keep))), plain.stderr[-200:]
        assert b"\t" not in inv.stderr
        assert len(plain.stdout) + len(inv.stdout) == sum(len(t) for t in text)
