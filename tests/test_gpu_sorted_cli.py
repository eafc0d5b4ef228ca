"""GPU tests of `kmerust ... --sorted` (krust_amd/host): the records in ascending k-mer order, the same bytes on every route and for
every table geometry, reproducible index files.  The k-mers of one run all have one length, so byte order of tsv lines is key order;
what a sorted run must print is therefore built here from the UNSORTED run's output, never from another sorted one."""
import json
import os
import subprocess

import numpy as np
import pytest

from test_gpu_format import record

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")


def run(*args, env=None):
    r = subprocess.run([BIN, *args], capture_output=True, timeout=300, env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, (args, r.stderr[-2000:])
    return r.stdout


def fx(name):
    return os.path.join(ROOT, "tests", "fixtures", name)


@pytest.fixture(scope="module")
def reads(tmp_path_factory):
    """About 20,000 FASTQ reads off a 300 kb genome: a few hundred thousand distinct 21-mers, many of them seen several times."""
    rng = np.random.default_rng(20260207)
    genome = np.frombuffer(b"ACGTacgtN", dtype=np.uint8)[rng.choice(9, size=300_000, p=[.23, .23, .23, .23, .02, .02, .02, .01, .01])].tobytes()
    path = tmp_path_factory.mktemp("sorted_cli") / "reads.fq"
    with open(path, "wb") as f:
        for i in range(20_000):
            a, n = int(rng.integers(0, len(genome) - 160)), int(rng.integers(30, 160))
            f.write(b"@r%d\n%s\n+\n%s\n" % (i, genome[a:a + n], b"I" * n))
    return str(path)


def sorted_document(fmt, unsorted_tsv):
    """The sorted document of a format, from the lines of the unsorted tsv run."""
    pairs = sorted((l.split(b"\t")[0].decode(), int(l.split(b"\t")[1])) for l in unsorted_tsv.splitlines())
    if fmt == "json" and not pairs:
        return b"[]\n"
    return b"".join(record(fmt, km, c, first=(i == 0)) for i, (km, c) in enumerate(pairs)) + (b"\n]\n" if fmt == "json" else b"")


CASES = [("3", "simple.fa"), ("5", "simple.fa"), ("4", "with_n.fa"), ("5", "soft_masked.fa"), ("4", "simple.fq"), ("5", "simple.fa.gz")]


@pytest.mark.parametrize("k,name", CASES, ids=lambda v: str(v))
def test_fixtures_sorted_in_every_format(k, name):
    unsorted = run(k, fx(name), "-f", "tsv", "-q")
    assert unsorted or name == "soft_masked.fa"   # (k = 5 finds no k-mer there: the empty documents, json's "[]" among them)
    for fmt in ("tsv", "fasta", "json"):
        got = run(k, fx(name), "-f", fmt, "-q", "--sorted")
        assert got == sorted_document(fmt, unsorted), (k, name, fmt)
        if fmt == "json":
            assert [d["kmer"] for d in json.loads(got)] == sorted(d["kmer"] for d in json.loads(got))
        if fmt == "tsv":
            assert got == b"".join(sorted(unsorted.splitlines(keepends=True)))
    two = run(k, fx(name), "-f", "tsv", "-q", "--sorted", "-m", "2")
    assert two == b"".join(sorted(l for l in unsorted.splitlines(keepends=True) if int(l.split(b"\t")[1]) >= 2))


ROUTES = {"host-format": ({"KMERUST_HOST_FORMAT": "1"}, []),
          "two-ranks": ({"KMERUST_TEXT_CHUNK_KB": "64"}, ["--devices", "0,0"]),   # --gpus 2 on a one-GPU machine: the device listed twice
          "pow2-table": ({"KMERHIP_POW2_TABLE": "1"}, []),
          "hint-small": ({"KMERHIP_CAPACITY_HINT": "100000"}, []),
          "hint-large": ({"KMERHIP_CAPACITY_HINT": "40000000"}, [])}


@pytest.fixture(scope="module")
def default_runs(reads):
    unsorted = run("21", reads, "-f", "tsv", "-q")
    assert len(unsorted.splitlines()) > 200_000
    docs = {fmt: run("21", reads, "-f", fmt, "-q", "--sorted") for fmt in ("tsv", "fasta", "json")}
    return unsorted, docs


def test_generated_reads_sorted_in_every_format(default_runs):
    unsorted, docs = default_runs
    assert docs["tsv"] == b"".join(sorted(unsorted.splitlines(keepends=True)))
    for fmt, doc in docs.items():
        assert doc == sorted_document(fmt, unsorted), fmt
    assert unsorted != docs["tsv"]   # (the table's own order is another one: the flag did something)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_every_route_gives_the_default_routes_bytes(reads, default_runs, route):
    env, extra = ROUTES[route]
    _, docs = default_runs
    for fmt in ("tsv", "json"):
        assert run("21", reads, "-f", fmt, "-q", "--sorted", *extra, env=env) == docs[fmt], (route, fmt)
    assert run("21", reads, "-f", "histogram", "-q", "--sorted", *extra, env=env) == run("21", reads, "-f", "histogram", "-q")


def test_saved_index_is_reproducible(reads, default_runs, tmp_path):
    _, docs = default_runs
    files = []
    for i, route in enumerate(("hint-small", "pow2-table", "two-ranks")):
        env, extra = ROUTES[route]
        path = str(tmp_path / f"s{i}.kmix")
        out = run("21", reads, "-f", "tsv", "-q", "--sorted", "--save", path, *extra, env=env)
        assert out == docs["tsv"], route
        files.append(open(path, "rb").read())
    assert files[0] == files[1] == files[2] and len(files[0]) > 200_000 * 16
    plain = str(tmp_path / "plain.kmix")
    run("21", reads, "-f", "tsv", "-q", "--save", plain)
    assert len(open(plain, "rb").read()) == len(files[0])   # (the KMIX layout is the same; only the pairs' order differs)
    # the sorted index loads and answers as any other
    first = docs["tsv"].splitlines()[0].split(b"\t")
    r = subprocess.run([BIN, "query", str(tmp_path / "s0.kmix"), first[0].decode()], capture_output=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == first[1]


def test_combine_sorted(reads, tmp_path):
    a, b = str(tmp_path / "a.kmix"), str(tmp_path / "b.kmix")
    run("21", reads, "-q", "-f", "histogram", "--save", a)
    run("21", fx("simple.fq"), "-q", "-f", "histogram", "--save", b)
    unsorted = run("combine", "union", a, b, "-f", "tsv", "-q")
    assert len(unsorted.splitlines()) > 200_000
    got = run("combine", "union", a, b, "-f", "tsv", "-q", "--sorted")
    assert got == b"".join(sorted(unsorted.splitlines(keepends=True))) and got != unsorted
    assert run("combine", "union", a, b, "-f", "json", "-q", "--sorted") == sorted_document("json", unsorted)
    assert run("combine", "union", a, b, "-f", "histogram", "-q", "--sorted") == run("combine", "union", a, b, "-f", "histogram", "-q")
    u1, u2 = str(tmp_path / "u1.kmix"), str(tmp_path / "u2.kmix")
    assert run("combine", "union", a, b, "-f", "tsv", "-q", "--sorted", "--save", u1) == got
    assert run("combine", "union", a, b, "-f", "tsv", "-q", "--sorted", "--save", u2, env={"KMERUST_HOST_FORMAT": "1", "KMERHIP_POW2_TABLE": "1"}) == got
    assert open(u1, "rb").read() == open(u2, "rb").read()
