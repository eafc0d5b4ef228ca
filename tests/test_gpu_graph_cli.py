"""`kmerust graph` on a saved index, in its three formats, against numpy on the oracle's counts of the file."""
import json
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_graph as G
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
    """A FASTA file of 1 500 reads and the 256 stars, its saved index, and the oracle's pairs of its records."""
    d = tmp_path_factory.mktemp("graph_cli")
    b, _ = O.synth_reads(41, 1 << 16, 150, 0, 1500, with_qual=False)
    recs = [bytes(x) for x in np.asarray(b).tobytes().split(b"\n")[:-1]] + G.star_records(K)
    fa = d / "a.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    rc, _, err = _run(K, fa, "--save", d / "a.kmix", "-q")
    assert rc == 0, err
    keys, counts = O.count_records(recs, K).arrays()
    return {"dir": d, "fa": fa, "kmix": d / "a.kmix", "keys": np.asarray(keys, dtype=U64).copy(), "counts": np.asarray(counts, dtype=U64).copy()}


def summary_rows(words):
    """The lines of -f summary from the 258 words, by the definitions of the issue (numpy / python only)."""
    cells = G.degree_cells(words)
    deg = lambda m: (bin(m >> 4).count("1"), bin(m & 15).count("1"))
    tot = lambda pred: sum(int(words[m]) for m in range(256) if pred(*deg(m)))
    rows = [("nodes", int(words[native.GRAPH_NODES])), ("kmers", int(words[native.GRAPH_KMERS])), ("arcs", sum(int(words[m]) * sum(deg(m)) for m in range(256))),
            ("isolated", int(words[0])), ("dead_ends", tot(lambda l, r: (l == 0) != (r == 0))), ("branching", tot(lambda l, r: l >= 2 or r >= 2)),
            ("simple", tot(lambda l, r: l == 1 and r == 1))]
    return rows + [(f"deg_{l}_{r}", int(cells[l, r])) for l in range(5) for r in range(5)]


def tsv_lines(keys, counts, masks):
    side = lambda b: "".join("ACGT"[c] for c in range(4) if b & (1 << c)) or "."
    return [f"{O.unpack(int(x), K)}\t{int(c)}\t{side(int(m) >> 4)}\t{side(int(m) & 15)}\n" for x, c, m in zip(keys, counts, masks)]


@pytest.mark.parametrize("mc", [1, 2])
def test_summary_and_json(index, mc):
    words = G.np_words(index["keys"], index["counts"], mc, K)
    rows = summary_rows(words)
    assert dict(rows)["nodes"] > 1000 and dict(rows)["branching"] > 0 and dict(rows)["simple"] > 0
    flags = [] if mc == 1 else ["-m", mc]
    rc, out, err = _run("graph", index["kmix"], *flags)
    assert rc == 0 and err == "", err
    assert out == "".join(f"{n}\t{v}\n" for n, v in rows)
    rc, out2, err = _run("graph", index["kmix"], "-f", "summary", f"--min-count={mc}")
    assert rc == 0 and out2 == out
    rc, out, err = _run("graph", index["kmix"], "-f", "json", *flags)
    assert rc == 0, err
    doc = json.loads(out)
    assert list(doc.items()) == rows and out.count("\n") == 1


@pytest.mark.parametrize("mc", [1, 2])
def test_tsv_unsorted_and_sorted(index, mc):
    sk, sc = G.node_set(index["keys"], index["counts"], mc)
    want = tsv_lines(sk, sc, G.np_masks(sk, sk, K))      # ascending key order
    assert len({l.split("\t", 2)[2] for l in want}) > 20   # many different (left, right) columns
    flags = [] if mc == 1 else ["-m", mc]
    rc, out, err = _run("graph", index["kmix"], "-f", "tsv", "--sorted", *flags)
    assert rc == 0, err
    assert out == "".join(want)
    rc, out, err = _run("graph", index["kmix"], "-f", "tsv", *flags)
    assert rc == 0, err
    assert sorted(out.splitlines(keepends=True)) == sorted(want)   # the same lines in table order


def test_sorted_tsv_is_the_same_bytes_for_two_table_geometries(index):
    rc, a, err = _run("graph", index["kmix"], "-f", "tsv", "--sorted")
    assert rc == 0, err
    rc, b, err = _run("graph", index["kmix"], "-f", "tsv", "--sorted", env={"KMERHIP_POW2_TABLE": "1"})
    assert rc == 0, err
    assert a == b and a.count("\n") == index["keys"].size


def test_errors(index, tmp_path):
    rc, out, err = _run("graph", tmp_path / "none.kmix")
    assert rc == 1 and out == "" and err.startswith("Application error:\n graph: ")
    rc, out, err = _run("graph", index["kmix"], "-m", 2 ** 62)    # an empty node set: all zero
    assert rc == 0 and out.splitlines()[0] == "nodes\t0" and all(l.endswith("\t0") for l in out.splitlines())
    rc, out, err = _run("graph", index["kmix"], "-f", "tsv", "-m", 2 ** 62)
    assert rc == 0 and out == ""
