"""`kmerust unitigs -f fasta` and `kmerust gfa -f gfa` on a saved index with branches and a cycle, on their two routes: the text
formatted on the device (kh_unitigs_text_*, the default) and by the host writers (KMERUST_HOST_FORMAT=1).  Stdout is byte-identical,
and the KMERUST_TIMING=1 line on stderr names the writer."""
import json
import os
import subprocess

import pytest

import test_gpu_gfa_cli as GC

pytestmark = pytest.mark.gpu

BIN = GC.BIN


@pytest.fixture(scope="module")
def kmix(tmp_path_factory):
    k = 21
    d = tmp_path_factory.mktemp("unitig_text_cli")
    recs = GC.branching_records(k)                      # reads, stars, and one period-300 cycle
    fa = d / "f.fa"
    fa.write_bytes(b"".join(b">r%d\n%s\n" % (i, r) for i, r in enumerate(recs)))
    rc, _, err = GC._run(k, fa, "--save", d / "idx.kmix", "-q")
    assert rc == 0, err
    return d / "idx.kmix"


def run(args, **env):
    e = {k: v for k, v in os.environ.items() if k not in ("KMERUST_HOST_FORMAT", "KMERUST_TIMING")}
    e.update(env)
    r = subprocess.run([BIN, *[str(a) for a in args]], capture_output=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    return r.stdout, r.stderr.decode()


def timing_of(err):
    lines = [ln for ln in err.splitlines() if ln.startswith('{"kmerust_timing"')]
    assert len(lines) == 1, err
    return json.loads(lines[0])["kmerust_timing"]


@pytest.mark.parametrize("args", [("unitigs", "-f", "fasta"), ("gfa", "-f", "gfa"), ("gfa", "-f", "gfa", "-m", "2")], ids=["unitigs", "gfa", "gfa-m2"])
def test_both_routes_print_the_same_bytes(kmix, args):
    cmd = [args[0], kmix, *args[1:]]
    dev, dev_err = run(cmd, KMERUST_TIMING="1")
    host, host_err = run(cmd, KMERUST_TIMING="1", KMERUST_HOST_FORMAT="1")
    assert dev == host and len(dev) > 10_000
    assert "-m" in args or dev.count(b"CR:i:1") >= 1                                              # the cycle is there (its k-mers have count 1)
    assert args[0] == "unitigs" or dev.count(b"\nL\t") > 100                                      # ... and the branches
    td, th = timing_of(dev_err), timing_of(host_err)
    assert td["writer"] == "device" and th["writer"] == "host"
    for t in (td, th):
        assert t["result_s"] > 0 and t["write_s"] > 0 and t["total_s"] >= t["result_s"]
    plain, plain_err = run(cmd)                                                                   # nothing is printed without the variable
    assert plain == dev and "kmerust_timing" not in plain_err
    zero, zero_err = run(cmd, KMERUST_TIMING="1", KMERUST_HOST_FORMAT="0")                        # 0 is "not set"
    assert zero == dev and timing_of(zero_err)["writer"] == "device"


def test_summaries_are_unchanged(kmix):
    for cmd in (["unitigs", kmix, "-f", "summary"], ["gfa", kmix, "-f", "summary"]):
        a, _ = run(cmd)
        b, _ = run(cmd, KMERUST_HOST_FORMAT="1")
        assert a == b and a.startswith(b"unitigs\t")
