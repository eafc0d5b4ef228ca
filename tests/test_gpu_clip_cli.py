"""`kmerust clip` on a saved index: the sorted tsv of the last table against the surviving pairs of the rule in Python strings
(tests/test_clip_ref.py) iterated as the command iterates, the saved index through `kmerust unitigs` against the string reference of the
final set, and the round lines on stderr with their stop."""
import os
import re
import subprocess

import numpy as np
import pytest

import test_clip_ref as R
import test_gpu_graph as G
import test_gpu_unitigs as U

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
U64 = np.uint64
HEADER = "round\tunitigs\tcandidates\tclipped\tclipped_kmers\tkept_kmers\n"


def _run(*args):
    r = subprocess.run([BIN, *[str(a) for a in args]], capture_output=True, timeout=300)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


@pytest.fixture(scope="module", params=["fork", "main"])
def index(request, tmp_path_factory):
    """A saved index and its node set as a dict from canonical strings to counts."""
    k = 21
    d = tmp_path_factory.mktemp(f"clip_cli_{request.param}")
    if request.param == "fork":
        reads = R.fork_reads(k, 3, 2)
        recs = [seq for seq, c in reads for _ in range(c)]
        S = R.S_of_reads(reads, k)
    else:
        flat, keys, counts = G.main_input(k)
        recs = [r for r in re.split(rb"[^ACGT]+", flat.tobytes()) if r]
        S = U.node_dict(keys, counts, k, 1)
    fa = d / "f.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    rc, _, err = _run(k, fa, "--save", d / "idx.kmix", "-q")
    assert rc == 0, err
    return {"name": request.param, "k": k, "kmix": d / "idx.kmix", "S": S, "dir": d}


_ROUNDS = {}


def rounds_of(index, mc, max_kmers, limit):
    """The reference iterated as the command iterates: [(words, S_next)] until a round clips nothing or `limit` rounds have run."""
    key = (index["name"], mc, max_kmers, limit)
    if key not in _ROUNDS:
        S = {x: c for x, c in index["S"].items() if c >= mc}
        out = []
        while True:
            _, cr = R.clip_of_S(S, index["k"], max_kmers)
            out.append((cr.words, cr.S_next))
            S = cr.S_next
            if cr.words[2] == 0 or (limit and len(out) >= limit):
                break
        _ROUNDS[key] = out
    return _ROUNDS[key]


def tsv_of(S):
    return "".join(f"{x.decode()}\t{S[x]}\n" for x in sorted(S))


def stderr_of(rounds):
    return HEADER + "".join(f"{i + 1}\t{w[0]}\t{w[1]}\t{w[2]}\t{w[3]}\t{w[5]}\n" for i, (w, _) in enumerate(rounds))


def fasta_of(ref, k):
    out = []
    for i, r in enumerate(ref.rows):
        start, n, cs, fl = (int(v) for v in r)
        out.append(f">{i} LN:i:{n + k - 1} KC:i:{cs} km:f:{cs / n:.1f}" + (" CR:i:1" if fl & 1 else "") + "\n" + ref.bases[start:start + n + k - 1].decode() + "\n")
    return "".join(out)


def test_one_round_is_the_default(index):
    k = index["k"]
    rounds = rounds_of(index, 1, k, 1)
    assert len(rounds) == 1 and rounds[0][0][2] > 0                                   # the round clips something
    rc, out, err = _run("clip", index["kmix"], "--sorted", "-f", "tsv")
    assert rc == 0 and err == stderr_of(rounds), err
    assert out == tsv_of(rounds[-1][1])
    rc, out2, err = _run("clip", index["kmix"], "--sorted", "--format=tsv", "--rounds", 1, "--max-kmers", k, "-m", 1, "-q")
    assert rc == 0 and err == "" and out2 == out


def test_rounds_zero_runs_until_nothing_is_clipped_and_saves(index):
    k = index["k"]
    rounds = rounds_of(index, 1, k, 0)
    assert 2 <= len(rounds) <= 6 and rounds[-1][0][2] == 0 and all(w[2] > 0 for w, _ in rounds[:-1])
    final = rounds[-1][1]
    saved = index["dir"] / "clipped.kmix"
    rc, out, err = _run("clip", index["kmix"], "--rounds", 0, "--sorted", "-f", "tsv", "--save", saved)
    assert rc == 0 and err == stderr_of(rounds) + f"saved: {saved} ({len(final)} k-mers)\n", err
    assert out == tsv_of(final)
    rc, fasta, err = _run("unitigs", saved)                                          # the saved index is the final set
    assert rc == 0, err
    assert fasta == fasta_of(U.Ref(final, k), k)
    # a limit below the stop: two rounds' lines, and the table behind the second
    two = rounds_of(index, 1, k, 2)
    rc, out, err = _run("clip", index["kmix"], "--rounds=2", "--sorted", "-ftsv")
    assert rc == 0 and err == stderr_of(two) and out == tsv_of(two[-1][1])


def test_min_count_max_kmers_and_the_other_writers(index):
    k = index["k"]
    if index["name"] == "main":
        rounds = rounds_of(index, 2, 2 * k, 1)
        rc, out, err = _run("clip", index["kmix"], "-m", 2, "--max-kmers", 2 * k, "--sorted", "-f", "tsv")
        assert rc == 0 and err == stderr_of(rounds) and out == tsv_of(rounds[-1][1])
    kept = rounds_of(index, 1, k, 1)[-1][1]
    rc, out, err = _run("clip", index["kmix"], "-f", "tsv", "-q")                     # unsorted: the same lines in the table's order
    assert rc == 0 and sorted(out.splitlines()) == tsv_of(kept).splitlines()
    rc, out, err = _run("clip", index["kmix"], "-f", "histogram", "-q")
    hist = {}
    for c in kept.values():
        hist[c] = hist.get(c, 0) + 1
    assert rc == 0 and out == "".join(f"{c}\t{n}\n" for c, n in sorted(hist.items()))
    rc, out, err = _run("clip", index["kmix"], "--max-kmers", 0, "--rounds", 0, "--sorted", "-f", "tsv", "-q")   # nothing is a candidate: S
    assert rc == 0 and out == tsv_of(index["S"])
    rc, out, err = _run("clip", index["kmix"], "--sorted", "-q")                      # fasta, the default format
    assert rc == 0 and out == "".join(f">{kept[x]}\n{x.decode()}\n" for x in sorted(kept))


def test_refusals(index, tmp_path):
    rc, out, err = _run("clip", tmp_path / "none.kmix")
    assert rc == 1 and out == "" and err.startswith("Application error:\n clip: ")
    rc, out, err = _run("clip", index["kmix"], "-m", 2 ** 62, "-f", "tsv")           # an empty node set: one round of nothing
    assert rc == 0 and out == "" and err == HEADER + "1\t0\t0\t0\t0\t0\n"
