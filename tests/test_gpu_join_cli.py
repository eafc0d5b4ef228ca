"""`kmerust compare` / `kmerust combine` on two saved indexes, against numpy on the oracle's counts of the two files."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import test_gpu_join as T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
K = 21
U64 = np.uint64


def _records(first, n):
    b, _ = O.synth_reads(41, 1 << 16, 150, first, n, with_qual=False)
    return [bytes(x) for x in np.asarray(b).tobytes().split(b"\n")[:-1]]


def _run(*args):
    r = subprocess.run([BIN, *[str(a) for a in args]], capture_output=True, timeout=300)
    return r.returncode, r.stdout.decode(), r.stderr.decode()


@pytest.fixture(scope="module")
def indexes(tmp_path_factory):
    """A.fa, B.fa (reads 0..1500 and 700..2200 of one seed), their indexes, and numpy's view of both."""
    d = tmp_path_factory.mktemp("join_cli")
    out = {"dir": d}
    pairs = {}
    for name, first in (("a", 0), ("b", 700)):
        recs = _records(first, 1500)
        fa = d / f"{name}.fa"
        fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
        rc, _, err = _run(K, fa, "--save", d / f"{name}.kmix", "-q")
        assert rc == 0, err
        m = O.count_records(recs, K)
        keys, counts = m.arrays()
        pairs[name] = (np.asarray(keys, dtype=U64).copy(), np.asarray(counts, dtype=U64).copy())
        out[name] = d / f"{name}.kmix"
    out["u"], out["ca"], out["cb"] = T.align(*pairs["a"], *pairs["b"])
    return out


def _measures(w):
    div = lambda x, y: x / y if y else math.nan
    return {"jaccard": div(w["shared"], w["distinct_a"] + w["distinct_b"] - w["shared"]), "containment_a": div(w["shared"], w["distinct_a"]),
            "containment_b": div(w["shared"], w["distinct_b"]), "bray_curtis": 1 - div(2 * w["sum_min"], w["sum_a"] + w["sum_b"])}


@pytest.mark.parametrize("mins", [(1, 1), (2, 3)])
def test_compare_tsv_and_json(indexes, mins):
    w = T.np_words(indexes["ca"], indexes["cb"], *mins)
    ms = _measures(w)
    assert 0.2 < ms["jaccard"] < 0.8
    rc, out, err = _run("compare", indexes["a"], indexes["b"], "--min-count-a", mins[0], "--min-count-b", mins[1], "-q")
    assert rc == 0, err
    want = "".join(f"{n}\t{v}\n" for n, v in w.items()) + "".join(f"{n}\t{v:.6f}\n" for n, v in ms.items())
    assert out == want
    rc, out, err = _run("compare", indexes["a"], indexes["b"], f"--min-count-a={mins[0]}", f"--min-count-b={mins[1]}", "-f", "json", "-q")
    assert rc == 0, err
    doc = json.loads(out)
    assert list(doc) == list(w) + list(ms) and {n: doc[n] for n in w} == w
    assert all(f"{doc[n]:.6f}" == f"{ms[n]:.6f}" for n in ms)


def test_compare_with_an_empty_set_prints_nan(indexes):
    rc, out, err = _run("compare", indexes["a"], indexes["b"], "--min-count-a", 2 ** 63, "-q")
    assert rc == 0, err
    lines = dict(l.split("\t") for l in out.splitlines())
    assert lines["distinct_a"] == "0" and lines["containment_a"] == "nan" and lines["jaccard"] == "0.000000" and lines["containment_b"] == "0.000000"


@pytest.mark.parametrize("op,calc", [("intersect", "min"), ("union", "sum"), ("union", "right"), ("subtract", None), ("count-subtract", None)])
def test_combine_every_op(indexes, op, calc, tmp_path):
    ek, ec = T.np_combine(indexes["u"], indexes["ca"], indexes["cb"], op, calc or "sum")
    assert ek.size > 100
    cflag = ["-c", calc] if calc else []
    # tsv: the sorted lines are numpy's
    rc, out, err = _run("combine", op, indexes["a"], indexes["b"], *cflag, "-f", "tsv", "-q")
    assert rc == 0, err
    want = sorted(f"{O.unpack(int(key), K)}\t{int(c)}" for key, c in zip(ek, ec))
    assert sorted(out.splitlines()) == want
    # histogram: np.unique of the result counts; with -m the lower counts are gone
    for m in (1, 2):
        rc, out, err = _run("combine", op, indexes["a"], indexes["b"], *cflag, "-f", "histogram", "-m", m, "-q")
        assert rc == 0, err
        cnt, freq = np.unique(ec[ec >= U64(m)], return_counts=True)
        assert out == "".join(f"{int(c)}\t{int(f)}\n" for c, f in zip(cnt, freq))
    # --save: a following query of one shared k-mer (or one of a's own) gives the combined count; the text still goes to stdout
    saved = tmp_path / "c.kmix"
    rc, out, err = _run("combine", op, indexes["a"], indexes["b"], *cflag, "-f", "tsv", "--save", saved)
    assert rc == 0 and f"saved: {saved} ({ek.size} k-mers)" in err, err
    assert sorted(out.splitlines()) == want
    both = (indexes["ca"] > 0) & (indexes["cb"] > 0)
    pick = np.flatnonzero(both if op in ("intersect", "union", "count-subtract") else ~both & (indexes["ca"] > 0))[:3]
    for i in pick:
        key = indexes["u"][i]
        sel = ek == key
        expect = int(ec[sel][0]) if sel.any() else 0
        rc, out, err = _run("query", saved, O.unpack(int(key), K))
        assert rc == 0 and out.strip() == str(expect), (op, out, err)


def test_min_counts_and_fasta_and_json_output(indexes):
    ek, ec = T.np_combine(indexes["u"], indexes["ca"], indexes["cb"], "intersect", "max", 2, 1)
    rc, out, err = _run("combine", "intersect", indexes["a"], indexes["b"], "-c", "max", "--min-count-a", 2, "-f", "json", "-q")
    assert rc == 0, err
    doc = json.loads(out)
    assert sorted((d["kmer"], d["count"]) for d in doc) == sorted((O.unpack(int(key), K), int(c)) for key, c in zip(ek, ec))
    rc, out, err = _run("combine", "intersect", indexes["a"], indexes["b"], "-c", "max", "--min-count-a", 2, "-q")
    assert rc == 0, err
    lines = out.splitlines()
    assert sorted(zip(lines[1::2], lines[0::2])) == sorted((O.unpack(int(key), K), f">{int(c)}") for key, c in zip(ek, ec))


def test_indexes_with_different_k(indexes, tmp_path):
    fa = indexes["dir"] / "a.fa"
    rc, _, err = _run(19, fa, "--save", tmp_path / "a19.kmix", "-q")
    assert rc == 0, err
    for args in (("compare", indexes["a"], tmp_path / "a19.kmix"), ("combine", "union", tmp_path / "a19.kmix", indexes["b"])):
        rc, out, err = _run(*args, "-q")
        assert rc != 0 and out == "" and "k=21" in err and "k=19" in err and "mismatch" in err, err
