"""`kmerust unitigs` on a saved index, in its two formats, against the string reference of tests/test_gpu_unitigs.py on the oracle's
counts of the file."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_graph as G
import test_gpu_unitigs as U
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
K = 21
U64 = np.uint64


def _run(*args, env=None):
    r = subprocess.run([BIN, *[str(a) for a in args]], capture_output=True, timeout=300, env=None if env is None else {**os.environ, **env})
    return r.returncode, r.stdout.decode(), r.stderr.decode()


@pytest.fixture(scope="module")
def index(tmp_path_factory):
    """A FASTA file of 1 500 reads, the 256 stars and two circular sequences, its saved index, and the oracle's pairs of its records."""
    d = tmp_path_factory.mktemp("unitigs_cli")
    b, _ = O.synth_reads(41, 1 << 16, 150, 0, 1500, with_qual=False)
    rng = np.random.default_rng(3)
    circ = []
    for p in (64, 700):
        unit = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=p)].tobytes()
        circ.append((unit * 2)[:p + K - 1])
    recs = [bytes(x) for x in np.asarray(b).tobytes().split(b"\n")[:-1]] + G.star_records(K) + circ
    fa = d / "a.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    rc, _, err = _run(K, fa, "--save", d / "a.kmix", "-q")
    assert rc == 0, err
    keys, counts = O.count_records(recs, K).arrays()
    return {"dir": d, "kmix": d / "a.kmix", "keys": np.asarray(keys, dtype=U64).copy(), "counts": np.asarray(counts, dtype=U64).copy()}


def fasta_of(ref, k):
    """The text of -f fasta from the reference's rows and bases, by the format of `kmerust unitigs --help` (python only)."""
    out = []
    for i, r in enumerate(ref.rows):
        start, L, cs, fl = (int(v) for v in r)
        h = f">{i} LN:i:{L + k - 1} KC:i:{cs} km:f:{cs / L:.1f}" + (" CR:i:1" if fl & 1 else "")
        out.append(h + "\n" + ref.bases[start:start + L + k - 1].decode() + "\n")
    return "".join(out)


def summary_of(ref, k):
    lens = sorted((int(r[1]) + k - 1 for r in ref.rows), reverse=True)
    total, run, n50 = sum(lens), 0, 0
    for x in lens:
        run += x
        if 2 * run >= total:
            n50 = x
            break
    rows = [("unitigs", len(lens)), ("kmers", sum(int(r[1]) for r in ref.rows)), ("bases", total), ("circular", sum(int(r[3]) & 1 for r in ref.rows)),
            ("longest", lens[0] if lens else 0), ("n50", n50)]
    return "".join(f"{n}\t{v}\n" for n, v in rows)


@pytest.mark.parametrize("mc", [1, 2])
def test_fasta_and_summary(index, mc):
    ref = U.ref_of("cli", index["keys"], index["counts"], K, mc)
    if mc == 1:
        assert ref.seen["circular"] >= 2 and ref.seen["minus_first"] > 0 and ref.rows.shape[0] > 256
    flags = [] if mc == 1 else ["-m", mc]
    rc, out, err = _run("unitigs", index["kmix"], *flags)
    assert rc == 0 and err == "", err
    assert out == fasta_of(ref, K)
    rc, out2, err = _run("unitigs", index["kmix"], "-f", "fasta", f"--min-count={mc}")
    assert rc == 0 and out2 == out
    if mc == 1:
        assert " CR:i:1\n" in out
    rc, out, err = _run("unitigs", index["kmix"], "-f", "summary", *flags)
    assert rc == 0 and err == "", err
    assert out == summary_of(ref, K)


def test_same_bytes_for_two_table_geometries(index):
    rc, a, err = _run("unitigs", index["kmix"])
    assert rc == 0, err
    rc, b, err = _run("unitigs", index["kmix"], env={"KMERHIP_POW2_TABLE": "1"})
    assert rc == 0, err
    assert a == b and a.count(">") > 256


def test_refusals_and_empty_node_set(index, tmp_path):
    rc, out, err = _run("unitigs", tmp_path / "none.kmix")
    assert rc == 1 and out == "" and err.startswith("Application error:\n unitigs: ")
    rc, out, err = _run("unitigs", index["kmix"], "-m", 2 ** 62)    # an empty node set: no record
    assert rc == 0 and out == ""
    rc, out, err = _run("unitigs", index["kmix"], "-f", "summary", "-m", 2 ** 62)
    assert rc == 0 and out == "unitigs\t0\nkmers\t0\nbases\t0\ncircular\t0\nlongest\t0\nn50\t0\n"
    rc, out, err = _run("unitigs", index["kmix"], "-f", "tsv")
    assert rc == 2 and out == "" and err.splitlines()[0] == "error: invalid value 'tsv' for '--format <FORMAT>'"
    rc, out, err = _run("unitigs", index["kmix"], "--sorted")
    assert rc == 2 and err.splitlines()[0] == "error: unexpected argument '--sorted' found"
    rc, out, err = _run("unitigs")
    assert rc == 2 and err.splitlines()[0] == "error: the following required arguments were not provided:"
