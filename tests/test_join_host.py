"""The host side of kh_compare / kh_combine_into without a device: the two symbols are declared, exported and bound; the derived
measures of `kmerust compare` on hand-computed words (tests/join_check.cpp); the usage errors of the two sub-commands."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")
NEW = ("kh_compare", "kh_combine_into")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_symbols_declared_mapped_and_bound():
    from krust_amd import native
    header = re.sub(r"/\*.*?\*/", "", _read("include", "kmerhip.h"), flags=re.S)
    mapfile = _read("krust_amd", "csrc", "kmerhip.map")
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} is not declared in kmerhip.h"
        assert name in mapfile, f"{name} is not listed in kmerhip.map"
        assert name in native.SYMBOLS, f"{name} is not in native.SYMBOLS"
    assert re.search(r"global:\s*kh_\*;", mapfile)
    for word in ("CMP_WORDS", "CMP_SUM_MIN", "SET_INTERSECT", "SET_COUNT_SUBTRACT", "CALC_MIN", "CALC_RIGHT"):
        value = int(re.search(r"#define\s+KH_%s\s+(\d+)" % word, header).group(1))
        assert getattr(native, word) == value, word
    assert callable(native.DeviceCounter.compare) and callable(native.DeviceCounter.combine_into)
    assert len(native.SYMBOLS["kh_compare"][1]) == 5 and len(native.SYMBOLS["kh_combine_into"][1]) == 8


def test_derived_measures(tmp_path):
    exe = str(tmp_path / "join_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, os.path.join(ROOT, "tests", "join_check.cpp")], check=True)
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "join_check ok" in p.stdout, p.stdout + p.stderr


def _run(*args):
    p = subprocess.run([BIN, *args], capture_output=True, text=True)
    return p.returncode, p.stdout, (p.stderr.splitlines() or [""])[0]


@pytest.mark.parametrize("args,first", [
    (["compare"], "error: the following required arguments were not provided:"),
    (["compare", "a.kmix"], "error: the following required arguments were not provided:"),
    (["compare", "a.kmix", "b.kmix", "c.kmix"], "error: unexpected argument 'c.kmix' found"),
    (["compare", "a.kmix", "b.kmix", "-f", "fasta"], "error: invalid value 'fasta' for '--format <FORMAT>'"),
    (["compare", "a.kmix", "b.kmix", "-c", "min"], "error: unexpected argument '-c' found"),
    (["combine"], "error: the following required arguments were not provided:"),
    (["combine", "union", "a.kmix"], "error: the following required arguments were not provided:"),
    (["combine", "xor", "a.kmix", "b.kmix"], "error: invalid value 'xor' for '<OP>'"),
    (["combine", "union", "a.kmix", "b.kmix", "-c", "avg"], "error: invalid value 'avg' for '--calc <CALC>'"),
    (["combine", "union", "a.kmix", "b.kmix", "-c"], "error: a value is required for '--calc <CALC>' but none was supplied"),
    (["combine", "union", "a.kmix", "b.kmix", "--min-count-a", "x"], "error: invalid value 'x' for '--min-count-a <N>': invalid digit found in string"),
])
def test_usage_errors(args, first):
    rc, out, err = _run(*args)
    assert rc == 2 and out == "" and err == first, (rc, out, err)


def test_help_names_the_sub_commands():
    p = subprocess.run([BIN, "--help"], capture_output=True, text=True)
    assert p.returncode == 0 and "kmerust compare <INDEX_A> <INDEX_B>" in p.stdout and "kmerust combine <intersect|union|subtract|count-subtract>" in p.stdout
