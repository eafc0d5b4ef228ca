"""`kmerust gfa` on a saved index, in its two formats: the S lines against `kmerust unitigs` of the same index and against the string
reference of tests/test_gpu_unitigs.py, the L lines against the links that tests/test_gpu_unitig_links.py derives from the reference's
sequences, rendered here; the summary recomputed in Python from rows and links."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_graph as G
import test_gpu_unitig_links as LK
import test_gpu_unitigs as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
U64 = np.uint64


def _run(*args):
    r = subprocess.run([BIN, *[str(a) for a in args]], capture_output=True, timeout=300)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


def dense_records(k):
    """Every k-mer of a random 600-base sequence and of three homopolymer / repeat records: at k = 5 most of the key space, with
    loops, hairpins and branches everywhere."""
    rng = np.random.default_rng(5)
    return [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=600)].tobytes(), b"A" * 12, b"ACACACACAC", b"CCCCCCGGGGGG"]


def branching_records(k):
    b, _ = O.synth_reads(43, 1 << 15, 150, 0, 800, with_qual=False)
    rng = np.random.default_rng(7)
    unit = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=300)].tobytes()
    return [bytes(x) for x in np.asarray(b).tobytes().split(b"\n")[:-1]] + G.star_records(k) + [(unit * 2)[:300 + k - 1]]


@pytest.fixture(scope="module", params=[5, 21], ids=["k5-dense", "k21-branching"])
def index(request, tmp_path_factory):
    k = request.param
    d = tmp_path_factory.mktemp(f"gfa_cli_k{k}")
    recs = dense_records(k) if k == 5 else branching_records(k)
    fa = d / "f.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    rc, _, err = _run(k, fa, "--save", d / "idx.kmix", "-q")
    assert rc == 0, err
    keys, counts = O.count_records(recs, k).arrays()
    return {"k": k, "kmix": d / "idx.kmix", "keys": np.asarray(keys, dtype=U64).copy(), "counts": np.asarray(counts, dtype=U64).copy()}


def parse_gfa(text):
    lines = text.split("\n")
    assert lines[-1] == "" and lines[0] == "H\tVN:Z:1.0"
    body = [ln.split("\t") for ln in lines[1:-1]]
    kinds = "".join(f[0] for f in body)
    assert kinds == "S" * kinds.count("S") + "L" * kinds.count("L")        # segments first, then links
    return [f for f in body if f[0] == "S"], [f for f in body if f[0] == "L"]


def summary_of(ref, links, k):
    nu = ref.rows.shape[0]
    out = np.zeros((nu, 2), dtype=bool)
    self_links = 0
    for w in links.tolist():
        a, sa, b = w >> 33, (w >> 32) & 1, (w & 0xFFFFFFFF) >> 1
        out[a, sa] = True
        self_links += a == b
    dead = 2 - out.sum(axis=1)
    tips = sum(1 for i in range(nu) if dead[i] == 1 and not int(ref.rows[i, 3]) & 1 and int(ref.rows[i, 1]) <= k)
    rows = [("unitigs", nu), ("links", links.size), ("self_links", self_links), ("dead_ends", int(dead.sum())), ("isolated", int((dead == 2).sum())),
            ("tips", tips)]
    return "".join(f"{n}\t{v}\n" for n, v in rows)


@pytest.mark.parametrize("mc", [1, 2])
def test_gfa_and_summary(index, mc):
    k = index["k"]
    tag = ("gfa-cli", k)
    ref = U.ref_of(tag, index["keys"], index["counts"], k, mc)
    lref = LK.links_of(tag, index["keys"], index["counts"], k, mc)
    if mc == 1:
        assert ref.rows.shape[0] > (20 if k == 5 else 256) and lref.links.size > ref.rows.shape[0] // 2
        assert k == 5 or ref.seen["circular"] >= 1
    flags = [] if mc == 1 else ["-m", mc]
    rc, out, err = _run("gfa", index["kmix"], *flags)
    assert rc == 0 and err == "", err
    rc, out2, err = _run("gfa", index["kmix"], "-f", "gfa", f"--min-count={mc}")
    assert rc == 0 and out2 == out
    S, L = parse_gfa(out)
    # the S lines: the sequences and tags of `kmerust unitigs` of the same index, and of the reference
    rc, fasta, err = _run("unitigs", index["kmix"], *flags)
    assert rc == 0, err
    recs = fasta.split("\n")[:-1]
    assert len(recs) == 2 * len(S) == 2 * ref.rows.shape[0]
    for i, f in enumerate(S):
        header = recs[2 * i].split(" ")
        assert f[1] == str(i) == header[0][1:] and f[2] == recs[2 * i + 1] and f[3:] == header[1:], (i, f[:2], header)
        start, n, cs, fl = (int(v) for v in ref.rows[i])
        assert f[2] == ref.bases[start:start + n + k - 1].decode()
        assert f[3:] == [f"LN:i:{n + k - 1}", f"KC:i:{cs}", f"km:f:{cs / n:.1f}"] + (["CR:i:1"] if fl & 1 else []), (i, f[3:])
    # the L lines: the reference's links, in link order, with k - 1 bases of overlap
    want = [["L", str(w >> 33), "+-"[(w >> 32) & 1], str((w & 0xFFFFFFFF) >> 1), "+-"[w & 1], f"{k - 1}M"] for w in lref.links.tolist()]
    assert len(L) == len(want)
    assert L == want, next((i, a, b) for i, (a, b) in enumerate(zip(L, want)) if a != b)
    rc, out, err = _run("gfa", index["kmix"], "-f", "summary", *flags)
    assert rc == 0 and err == "", err
    assert out == summary_of(ref, lref.links, k)


def test_refusals_and_empty_node_set(index, tmp_path):
    rc, out, err = _run("gfa", tmp_path / "none.kmix")
    assert rc == 1 and out == "" and err.startswith("Application error:\n gfa: ")
    rc, out, err = _run("gfa", index["kmix"], "-m", 2 ** 62)          # an empty node set: the header line alone
    assert rc == 0 and out == "H\tVN:Z:1.0\n"
    rc, out, err = _run("gfa", index["kmix"], "-f", "summary", "-m", 2 ** 62)
    assert rc == 0 and out == "unitigs\t0\nlinks\t0\nself_links\t0\ndead_ends\t0\nisolated\t0\ntips\t0\n"
    rc, out, err = _run("gfa", index["kmix"], "-f", "fasta")
    assert rc == 2 and out == "" and err.splitlines()[0] == "error: invalid value 'fasta' for '--format <FORMAT>'"
