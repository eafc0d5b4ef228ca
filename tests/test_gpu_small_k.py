"""Small k (1..11) at size, on every table geometry and counting route, against the CPU oracle.

The reference serves k = 1..32 alike (src/kmer.rs:100-110) and benchmarks k = 5, 11, 21, 31.  Below k = 12 this design leaves
its headline route: level 1 runs the C++ window (never the written-out one for k <= 10, never the digit / payload form for
k < 10), an unhinted k < 10 table is sized for EVERY window (450 M windows: about 10 GB of table for the 512 keys of k = 5 --
the product's behaviour, measured here, not changed), a 10-bit level-1 digit meets a hash of 2k <= 10 bits (no payload bits at
all), every bucket is heavy, overflows its level-2 arena and is "hot" or just below it, and 32-bit counts overflow on their
own (S100M at k = 1: 7.5 G on each of two keys).  tests/test_geometry_small_k.py holds the geometry ARITHMETIC on the CPU;
this file holds what the kernels make of it:

  section 2  a few million windows: every k = 1..11 x {no quality, -Q 20} over table geometries (no hint, crowded, 2^12
             regions, 1024 x b2 with the 10-bit digit and 2k <, =, > 10, 1024 x 1024), paths, the 8-byte image on / off,
             payload width, level-1 bins -- a pairwise design (CASES below); three pushes, results in between, reset, again
  section 3  hundreds of millions of windows with the DEFAULT thresholds, random knobs (KMERHIP_SMALLK_SEEDS seeds)
  section 4  counts beyond 2^32 at k = 1, 2 and what exports / merges make of them; dense merges of huge counts;
             merge_across in an RCCL world of one
  section 5  the kmerust command line and the PRODUCT library at small k, unhinted

Every comparison is against tests/oracle_lib.py.  Run with `pytest -m gpu` on an MI355X.  Nothing here reads /root/reference."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCPU = max(1, min(os.cpu_count() or 1, 16))
SMALL_KS = list(range(1, 12))


@pytest.fixture(scope="module")
def K():
    import torch
    assert torch.cuda.is_available(), "these tests need a GPU"
    import krust_amd
    krust_amd.lib()  # ImportError if the HIP extension is missing: no silent fallback
    return krust_amd


def _setenv(monkeypatch, env):
    for name, val in env.items():
        if val is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, val)


# ---------------------------------------------------------------------------------------------------------------------
# the reads of sections 2, 4 (merge_across) and 5: N, lower case, low qualities, every length mod 16, both strands
# ---------------------------------------------------------------------------------------------------------------------
N_READS = 56_000
_READS = {}


def _make_records(n_reads=N_READS, seed=1105):
    """The _window_reads() recipe of test_gpu_parity.py at 56,000 reads (about 7 M windows: the largest of three pushes is
    above PART_MIN_WINDOWS = 2^22, so the automatic path choice partitions too)."""
    rng = np.random.default_rng(seed)
    genome = rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=1 << 18)
    recs, quals = [], []
    for i in range(n_reads):
        n = int(rng.integers(20, 240))
        o = int(rng.integers(0, genome.size - n))
        s = genome[o:o + n].copy()
        u = rng.random()
        if u > 0.9:
            a = int(rng.integers(0, n))
            s[a:a + int(rng.integers(1, 4))] = ord("N")
        if u < 0.05:
            s = np.frombuffer(s.tobytes().lower(), dtype=np.uint8).copy()
        if i % 2:
            s = np.frombuffer(s.tobytes().translate(bytes.maketrans(b"ACGTacgt", b"TGCAtgca"))[::-1], dtype=np.uint8).copy()
        recs.append(s.tobytes())
        quals.append(rng.choice(np.frombuffer(b"#5IIIIII", dtype=np.uint8), size=n).astype(np.uint8).tobytes())
    return recs, quals


def _reads():
    if not _READS:
        recs, quals = _make_records()
        bases = np.frombuffer(b"\n".join(recs) + b"\n", dtype=np.uint8)
        qual = np.frombuffer(b"\n".join(quals) + b"\n", dtype=np.uint8)
        ends = np.flatnonzero(bases == 10) + 1
        _READS.update(recs=recs, quals=quals, bases=bases, qual=qual, cuts=[0, int(ends[499]), int(ends[11_999]), bases.size], maps={})
    return _READS


def _oracle(k, minq, upto):
    """OracleMap of the first `upto` bytes of the reads (a record boundary)."""
    R = _reads()
    key = (k, minq, upto)
    if key not in R["maps"]:
        m = O.OracleMap()
        total = m.scan_flat(R["bases"][:upto], k, qual=R["qual"][:upto] if minq is not None else None, min_quality=minq, nthreads=NCPU)
        assert total == m.total()
        R["maps"][key] = m
    return R["maps"][key]


def _hist_of(counts, min_count=1):
    c = np.asarray(counts, dtype=np.uint64)
    v, f = np.unique(c[c >= min_count], return_counts=True)
    return list(zip(v.tolist(), f.tolist()))


def _check_everything(dc, st, m, k, what):
    """kmers, distinct, the whole sorted (key, count) arrays, histogram() and result() for min_count 1, 2, 10^6, lookups of every
    key of the key space (a sample of it beyond 2^16 keys), absent keys, and words that are no k-mer of this k (a bit at 2k, at 63)."""
    wk, wc = m.arrays()
    assert st["kmers"] == m.total(), (what, st["kmers"], m.total())
    assert st["distinct"] == len(m), (what, st["distinct"], len(m))
    keys, cnts = dc.result()
    assert np.array_equal(keys, wk) and np.array_equal(cnts, wc), (what, "result()", keys[:8], cnts[:8], wk[:8], wc[:8])
    for mc in (1, 2, 10 ** 6):
        sel = wc >= mc
        assert dc.histogram(min_count=mc) == m.histogram(min_count=mc) == _hist_of(wc, mc), (what, "histogram", mc)
        k2, c2 = dc.result(min_count=mc)
        assert np.array_equal(k2, wk[sel]) and np.array_equal(c2, wc[sel]), (what, "result(min_count)", mc)
    space = 1 << (2 * k)
    if space <= 1 << 16:
        probe = np.arange(space, dtype=np.uint64)
    else:
        rng = np.random.default_rng(k)
        probe = np.unique(np.concatenate([wk[:: max(1, len(wk) // 20_000)], rng.integers(0, space, size=20_000).astype(np.uint64),
                                          np.array([0, space - 1], dtype=np.uint64)]))
    base = probe[:: max(1, len(probe) // 512)]
    odd = np.concatenate([base | np.uint64(1 << (2 * k)), base | np.uint64(1 << 63), np.array([1 << (2 * k), 1 << 63, (1 << 64) - 2], dtype=np.uint64)])
    probe = np.concatenate([probe, odd])
    want = np.zeros(probe.size, dtype=np.uint64)
    ok = probe < np.uint64(space)
    pos = np.searchsorted(wk, probe[ok])
    pos[pos >= len(wk)] = 0
    hit = wk[pos] == probe[ok] if len(wk) else np.zeros(pos.size, dtype=bool)
    want[np.flatnonzero(ok)[hit]] = wc[pos[hit]]
    got = dc.lookup(probe)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (what, "lookup", [(hex(int(probe[i])), int(got[i]), int(want[i])) for i in bad[:8]])
    for i in np.linspace(0, probe.size - 1, num=64).astype(np.int64):   # (the vectorised expectation itself, against the oracle's map)
        assert int(want[i]) == m.get(int(probe[i])) or int(probe[i]) >= space


# ---------------------------------------------------------------------------------------------------------------------
# section 2: the geometry sweep, as a pairwise design
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRIES = ["nohint", "hint3000", "hint6M", "regions2048", "regions1024x24", "regions1024x160"]
PATHS = ["partition", "direct", "auto"]


def _cases():
    """Every geometry with every k; path, quality, KMERHIP_NARROW rotate against the geometry with k, so that every value of each
    occurs with every k and (over the ks) with every geometry.  KMERHIP_PAYLOAD=64 rides on k = 1, 5, 9, KMERHIP_P1_BINS=0 on
    k = 3, 9; the 64 GB table of 1024 x 1024 regions is one case each for k = 4, 5, 6."""
    out = []
    for k in SMALL_KS:
        geos = GEOMETRIES + (["regions1024x1024"] if k in (4, 5, 6) else [])
        for gi, geo in enumerate(geos):
            path = PATHS[(gi + k) % 3]
            minq = 20 if (gi + k) % 2 else None
            narrow = "0" if (gi + k // 2) % 2 else None
            env = {"KMERHIP_NARROW": narrow, "KMERHIP_PAYLOAD": None, "KMERHIP_P1_BINS": None}
            if k in (1, 5, 9) and gi % 3 == 1:
                env["KMERHIP_PAYLOAD"] = "64"
            if k in (3, 9) and gi % 3 == 2:
                env["KMERHIP_P1_BINS"] = "0"
            if geo == "regions1024x1024":
                path, narrow = "partition", None
                env["KMERHIP_NARROW"] = None
            out.append(dict(k=k, geo=geo, path=path, minq=minq, env=env))
        # what the rotation above leaves out for this k: both quality settings on the partitioned, unhinted table; both
        # KMERHIP_NARROW values on the partitioned path of a forced 10-bit digit
        out.append(dict(k=k, geo="nohint", path="partition", minq=None if (k % 2) else 20, env={"KMERHIP_NARROW": "0" if k % 2 else None, "KMERHIP_PAYLOAD": None, "KMERHIP_P1_BINS": None}))
    return out


CASES = _cases()


def _case_id(c):
    knobs = "".join(f"-{n[8:].lower()}{v}" for n, v in c["env"].items() if v is not None)
    return f"k{c['k']}-{c['geo']}-{c['path']}-{'q20' if c['minq'] else 'noqual'}{knobs}"


def test_the_sweep_names_every_value_with_every_k():
    """(so that a later change of CASES cannot silently drop one)"""
    for k in SMALL_KS:
        mine = [c for c in CASES if c["k"] == k]
        assert {c["geo"] for c in mine} >= set(GEOMETRIES), k
        assert {c["path"] for c in mine} == set(PATHS), k
        assert {c["minq"] for c in mine} == {None, 20}, k
        assert {c["env"]["KMERHIP_NARROW"] for c in mine} == {None, "0"}, k
        assert (k in (1, 5, 9)) == any(c["env"]["KMERHIP_PAYLOAD"] == "64" for c in mine), k
        assert (k in (3, 9)) == any(c["env"]["KMERHIP_P1_BINS"] == "0" for c in mine), k
        assert (k in (4, 5, 6)) == any(c["geo"] == "regions1024x1024" for c in mine), k
    assert sorted({c["k"] for c in CASES}) == SMALL_KS


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_small_k_geometry_sweep(K, monkeypatch, case):
    """Three pushes of different sizes into one context -- a fresh pass, a pass over what the first left (the 8-byte image where
    there is one), a pass after a result() --, everything checked after each finish(); then kh_reset and the whole input again."""
    import torch
    k, minq, geo = case["k"], case["minq"], case["geo"]
    R = _reads()
    cuts = R["cuts"]
    m_mid, m_all = _oracle(k, minq, cuts[2]), _oracle(k, minq, cuts[3])
    env = dict(case["env"])
    hint, regions = 0, None
    if geo == "hint3000":
        hint = 3_000
    elif geo == "hint6M":
        hint = 6_000_000
    elif geo.startswith("regions"):
        a, _, b = geo[7:].partition("x")
        regions = int(a) * (int(b) if b else 1)
        env["KMERHIP_TABLE_REGIONS"] = str(regions)
        hint = max(len(m_all), 1)    # (a hinted table keeps the geometry it was given)
    env.setdefault("KMERHIP_TABLE_REGIONS", None)
    _setenv(monkeypatch, env)
    tb = torch.from_numpy(R["bases"].copy()).cuda()
    tq = torch.from_numpy(R["qual"].copy()).cuda() if minq is not None else None
    torch.cuda.synchronize()
    what = _case_id(case)

    def push(dc, a, b):
        dc.push_device(tb.data_ptr() + a, tq.data_ptr() + a if tq is not None else None, b - a)

    with K.DeviceCounter(k, min_quality=minq, capacity_hint=hint, path=None if case["path"] == "auto" else case["path"]) as dc:
        push(dc, cuts[0], cuts[1])
        push(dc, cuts[1], cuts[2])
        st = dc.finish()
        _check_everything(dc, st, m_mid, k, what + " after two pushes")
        push(dc, cuts[2], cuts[3])
        st = dc.finish()
        if regions is not None:
            assert st["table_slots"] == regions * 4096 or st["grows"] > 0, (what, st["table_slots"], st["grows"])
        if geo == "hint6M":
            assert st["table_slots"] == 1 << 24 or st["grows"] > 0, (what, st["table_slots"])
        _check_everything(dc, st, m_all, k, what + " after three pushes")
        dc.reset()
        push(dc, cuts[0], cuts[3])
        st = dc.finish()
        _check_everything(dc, st, m_all, k, what + " after reset")


# ---------------------------------------------------------------------------------------------------------------------
# section 3: hundreds of millions of windows, default thresholds
# ---------------------------------------------------------------------------------------------------------------------
SMALLK_SEEDS = int(os.environ.get("KMERHIP_SMALLK_SEEDS", "11"))   # (more: KMERHIP_SMALLK_SEEDS=100 pytest ...)
LARGE_KNOBS = {
    "KMERHIP_HOT_CUT": [None, None, None, "200000"],
    "KMERHIP_SURVIVAL": [None, None, "0.1"],
    "KMERHIP_REGION_NT": [None, None, "512", "1024"],
    "KMERHIP_NARROW": [None, None, "0"],
    "KMERHIP_L2_SKEW_X": [None, None, "0"],
    "KMERHIP_L2_ARENA": [None, None, None, "0"],
    "KMERHIP_PART_BUDGET_GB": [None, None, "0.6", "2", "0.25"],    # (0.25 GB: three batches and more from 1.5 M reads up)
    "KMERHIP_OVF_AGG": [None, None, "1", "0"],
    "KMERHIP_TABLE_REGIONS": [None, None, None, "20480", "81920"],
}   # (test_gpu_stress.py MID_KNOBS without KMERHIP_ESTIMATE: the level-1 sample never sizes a k < 10 table)


def large_scenario(seed):
    rng = np.random.default_rng(110_000 + seed)
    k = SMALL_KS[seed % 11] if seed < 11 else int(rng.integers(1, 12))   # every k once in the first eleven seeds
    minq = 20 if seed % 3 == 2 else None
    n_reads = int(rng.integers(1_000_000, 3_000_001))
    glen = 1 << int(rng.integers(22, 28))
    share = float(rng.choice([0.0, 0.01, 0.1, 0.4]))
    unit = bytes(rng.choice(list(b"ACGT"), size=int(rng.integers(11, 60))).astype(np.uint8))
    rows = rng.choice(n_reads, size=int(share * n_reads), replace=False) if share else None
    hint_kind = str(rng.choice(["0", "3000", "distinct", "4xdistinct"]))
    env = {name: vals[int(rng.integers(0, len(vals)))] for name, vals in LARGE_KNOBS.items()}
    path = str(rng.choice(["partition", "partition", "auto"]))
    cuts = sorted({0, n_reads, *[int(x) for x in rng.integers(0, n_reads, size=int(rng.integers(0, 3)))]})
    return dict(k=k, minq=minq, n_reads=n_reads, glen=glen, share=share, unit=unit, rows=rows, hint_kind=hint_kind, env=env, path=path, cuts=cuts)


def test_the_large_scenarios_draw_every_small_k():
    assert SMALLK_SEEDS < 11 or sorted({large_scenario(s)["k"] for s in range(SMALLK_SEEDS)}) == SMALL_KS
    assert sorted({large_scenario(s)["k"] for s in range(11)}) == SMALL_KS   # (the default seed count)


@pytest.mark.parametrize("seed", range(SMALLK_SEEDS))
def test_small_k_random_route_same_map_at_a_few_hundred_million_windows(K, seed, monkeypatch):
    """1-3 M reads of 150 bp (150-450 M windows) from the device generator, a random share overwritten with repeats, where the
    DEFAULT thresholds bite at small k: every bucket heavy and over its arena, hot buckets above a thousandth of the batch,
    several batches per push.  At k <= 11 the oracle's whole map is small (at most 2.1 M keys): the full sorted arrays and the
    histogram are compared, not a digest.  Memory: an unhinted k < 10 context sizes its table for every window -- 450 M windows
    make about 10 GB of table beside the partition buffers; that is the product's behaviour and part of what is under test."""
    import torch
    sc = large_scenario(seed)
    k, minq, n_reads, rl = sc["k"], sc["minq"], sc["n_reads"], 150
    nbytes = n_reads * (rl + 1)
    tb = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    tq = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    K.synth_reads_device(tb.data_ptr(), tq.data_ptr(), 1777 + seed, sc["glen"], rl, 0, n_reads)
    if sc["rows"] is not None:
        units = [b"A", b"AC", b"GATTACA", sc["unit"]]
        rows = torch.from_numpy(sc["rows"]).cuda()
        v = tb.view(n_reads, rl + 1)
        for j, u in enumerate(units):
            v[rows[j::len(units)], :rl] = torch.from_numpy(np.resize(np.frombuffer(u, dtype=np.uint8), rl).copy()).cuda()
    torch.cuda.synchronize()
    host, hq = tb.cpu().numpy(), tq.cpu().numpy()
    m = O.OracleMap()
    total = m.scan_flat(host, k, qual=hq if minq is not None else None, min_quality=minq, nthreads=NCPU)
    wk, wc = m.arrays()
    assert total == int(wc.sum())
    hint = {"0": 0, "3000": 3_000, "distinct": len(wk), "4xdistinct": 4 * len(wk)}[sc["hint_kind"]]
    _setenv(monkeypatch, sc["env"])
    what = (f"seed {seed}: k={k} minq={minq} reads={n_reads} genome=2^{sc['glen'].bit_length() - 1} repeats={sc['share']} hint={hint} "
            f"path={sc['path']} cuts={sc['cuts']} env={ {a: b for a, b in sc['env'].items() if b} }")
    with K.DeviceCounter(k, min_quality=minq, capacity_hint=hint, path=None if sc["path"] == "auto" else sc["path"]) as dc:
        for a, b in zip(sc["cuts"], sc["cuts"][1:]):
            if b > a:
                dc.push_device(tb.data_ptr() + a * (rl + 1), tq.data_ptr() + a * (rl + 1) if minq is not None else None, (b - a) * (rl + 1))
        st = dc.finish()
        assert st["kmers"] == total and st["distinct"] == len(wk), (what, st["kmers"], total, st["distinct"], len(wk))
        keys, cnts = dc.result()
        assert np.array_equal(keys, wk) and np.array_equal(cnts, wc), (what, keys[:8], cnts[:8], wk[:8], wc[:8])
        assert dc.histogram() == m.histogram(), what


# ---------------------------------------------------------------------------------------------------------------------
# section 4: counts beyond 2^32 where small k puts them
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def three_million_reads(K):
    """One device buffer of 3 M x 150 bp (450 M windows), a third of the reads poly-A: at k = 1 both keys pass 2^32 after the same
    number of pushes that leaves AA alone above it at k = 2."""
    import torch
    n_reads, rl = 3_000_000, 150
    tb = torch.empty(n_reads * (rl + 1), dtype=torch.uint8, device="cuda")
    K.synth_reads_device(tb.data_ptr(), None, 4242, 1 << 24, rl, 0, n_reads)
    tb.view(n_reads, rl + 1)[::3, :rl] = ord("A")
    torch.cuda.synchronize()
    host = tb.cpu().numpy()
    maps = {}
    for k in (1, 2):
        m = O.OracleMap()
        m.scan_flat(host, k, nthreads=NCPU)
        maps[k] = m.arrays()
    pushes = (1 << 32) // int(maps[1][1].min()) + 1
    return tb, maps, pushes


def _roundtrip_exports(K, dc, st, k, wk, want_c, what):
    """From a table with counts beyond 2^32: heads / packed exports return None or round-trip exactly into two logical shards, the
    wide and the dense export always round-trip."""
    import torch
    nsh = 2
    R = st["table_slots"] // 4096
    want = dict(zip(wk.tolist(), want_c.tolist()))
    cap = 4 * len(wk) + 1024
    for fmt in ("heads", "packed", "wide"):
        dk = torch.zeros(cap, dtype=torch.int64, device="cuda")
        dcnt = torch.zeros(cap, dtype=torch.int64, device="cuda")
        rc = torch.zeros(R, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        if fmt == "heads":
            res = dc.export_regions_heads_device(nsh, dk.data_ptr(), 2 * cap, rc.data_ptr(), R)
        elif fmt == "packed":
            res = dc.export_regions_packed_device(nsh, dk.data_ptr(), cap, rc.data_ptr(), R)
        else:
            res = dc.export_regions_device(nsh, dk.data_ptr(), dcnt.data_ptr(), cap, rc.data_ptr(), R)
        if res is None:
            assert fmt != "wide"
            continue      # not representable: said so, nothing truncated
        parts, R2 = res
        assert R2 == R and int(rc.sum().item()) == int(parts.sum()), (what, fmt)
        offs = np.concatenate([[0], np.cumsum(parts)]).astype(np.int64)
        merged = {}
        for o in range(nsh):
            with K.DeviceCounter(k, capacity_hint=3_000) as rcv:
                rcv.set_shard(o, nsh)
                seg = rc.data_ptr() + 4 * (R // nsh) * o
                if fmt == "heads":
                    rcv.merge_regions_heads_device(R, [dk.data_ptr() + 4 * int(offs[o])], [seg])
                elif fmt == "packed":
                    rcv.merge_regions_packed_device(R, [dk.data_ptr() + 8 * int(offs[o])], [seg])
                else:
                    rcv.merge_regions_device(R, [dk.data_ptr() + 8 * int(offs[o])], [dcnt.data_ptr() + 8 * int(offs[o])], [seg])
                rcv.finish()
                d = rcv.as_dict()
                assert rcv.lookup(wk).tolist() == [d.get(int(x), 0) for x in wk], (what, fmt)
            assert all(K.owner(key, k, nsh) == o for key in d) and not (set(d) & set(merged)), (what, fmt)
            merged.update(d)
        assert merged == want, (what, fmt, merged, want)
    n = 1 << (2 * k)
    arr = torch.full((n,), -1, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    dc.export_dense_device(arr.data_ptr(), n)
    host = arr.cpu().numpy().astype(np.uint64)
    assert {int(i): int(host[i]) for i in np.flatnonzero(host)} == want, (what, "dense export")
    merged = {}
    for o in range(nsh):
        with K.DeviceCounter(k) as rcv:
            rcv.merge_dense_device(arr.data_ptr(), n, o, nsh)
            rcv.finish()
            d = rcv.as_dict()
        assert all(K.owner(key, k, nsh) == o for key in d)
        merged.update(d)
    assert merged == want, (what, "dense merge")


@pytest.mark.parametrize("k,hot_cut,ovf_agg", [(1, None, None), (1, "0", "0"), (1, None, "1"), (2, "0", None), (2, None, "0"), (2, "0", "1")],
                         ids=lambda v: "unset" if v is None else str(v))
def test_small_k_counts_beyond_32_bits(K, monkeypatch, three_million_reads, k, hot_cut, ovf_agg):
    """450 M windows pushed again and again through the partitioned path until every key of k = 1 is above 2^32 (at k = 2: AA
    above, the others below).  Hot buckets as shipped and off (the region pass's own overflow path), the overflow list summed in
    LDS, entry by entry and as the library chooses.  The 8-byte image cannot hold these counts: the table ends as 16-byte slots."""
    _setenv(monkeypatch, {"KMERHIP_HOT_CUT": hot_cut, "KMERHIP_OVF_AGG": ovf_agg})
    tb, maps, pushes = three_million_reads
    wk, wc1 = maps[k]
    want_c = wc1 * np.uint64(pushes)
    if k == 1:
        assert (want_c > np.uint64(1 << 32)).all()
    else:
        assert (want_c > np.uint64(1 << 32)).any() and (want_c < np.uint64(1 << 32)).any()
    what = f"k={k} hot_cut={hot_cut} ovf_agg={ovf_agg} pushes={pushes}"
    with K.DeviceCounter(k, path="partition") as dc:
        for _ in range(pushes):
            dc.push_device(tb.data_ptr(), None, tb.numel())
        st = dc.finish()
        assert st["kmers"] == int(want_c.sum()) and st["distinct"] == len(wk), (what, st)
        assert st["slot_bytes"] == 16, (what, st["slot_bytes"])
        keys, cnts = dc.result()
        assert np.array_equal(keys, wk) and np.array_equal(cnts, want_c), (what, keys, cnts, want_c)
        probe = np.concatenate([np.arange(1 << (2 * k), dtype=np.uint64), np.array([1 << (2 * k), 1 << 63], dtype=np.uint64)])
        d = dict(zip(wk.tolist(), want_c.tolist()))
        assert dc.lookup(probe).tolist() == [d.get(int(x), 0) for x in probe], what
        for mc in (1, 1 << 32):
            assert dc.histogram(min_count=mc) == _hist_of(want_c, mc), (what, mc)
        if ovf_agg is None or (k == 2 and ovf_agg == "0"):      # (one table of each k and hot-bucket setting)
            _roundtrip_exports(K, dc, st, k, wk, want_c, what)


@pytest.mark.parametrize("nparts", [1, 2, 3])
@pytest.mark.parametrize("k", [3, 11])
def test_dense_merge_of_huge_counts(K, k, nparts):
    """kh_merge_dense_device of a synthetic dense array with entries of 1, 2^32 - 1, 2^32, 2^40 and zeros, for owners of 1, 2
    and 3 parts: the map, lookups and the histogram exact."""
    import torch
    n = 1 << (2 * k)
    rng = np.random.default_rng(k)
    cand = np.arange(n, dtype=np.uint64) if k == 3 else rng.integers(0, n, size=6000).astype(np.uint64)
    keys = sorted({K.canonical(int(x), k)[0] for x in cand})
    vals = [1, (1 << 32) - 1, 1 << 32, 1 << 40, 0]
    want = {key: vals[i % 5] for i, key in enumerate(keys) if vals[i % 5]}
    dense = np.zeros(n, dtype=np.int64)
    for key, v in want.items():
        dense[key] = v
    td = torch.from_numpy(dense).cuda()
    torch.cuda.synchronize()
    merged = {}
    probe = np.array(keys + [n, 1 << 63], dtype=np.uint64)
    for o in range(nparts):
        with K.DeviceCounter(k) as dc:
            dc.merge_dense_device(td.data_ptr(), n, o, nparts)
            st = dc.finish()
            d = dc.as_dict()
            mine = {key: v for key, v in want.items() if K.owner(key, k, nparts) == o}
            assert d == mine, (k, nparts, o)
            assert st["distinct"] == len(mine) and st["kmers"] == sum(mine.values())
            assert dc.lookup(probe).tolist() == [mine.get(int(x), 0) for x in probe]
            assert dc.histogram() == _hist_of(list(mine.values())), (k, nparts, o)
            assert dc.histogram(min_count=1 << 32) == _hist_of(list(mine.values()), 1 << 32)
        merged.update(d)
    assert merged == want


@pytest.mark.parametrize("pieces", [None, "1"], ids=["pieces-default", "pieces1"])
@pytest.mark.parametrize("k", [5, 9])
def test_small_k_merge_across_world_of_one(K, monkeypatch, k, pieces):
    """kh_merge_across through RCCL in a world of one after about 7 M windows: the dense route (2k <= 26), the count sum
    conserved, the map the oracle's."""
    _setenv(monkeypatch, {"KMERHIP_MERGE_PIECES": pieces})
    R = _reads()
    m = _oracle(k, None, R["cuts"][3])
    wk, wc = m.arrays()
    with K.DeviceCounter(k) as dc:
        dc.comm_init(1, 0, K.comm_unique_id())
        dc.push(R["bases"])
        info = dc.merge_across()
        assert info["path"].startswith("dense"), info
        assert info["conserved"] == 1 and info["nranks"] == 1 and info["owned_distinct"] == len(wk), info
        assert info["merged_count_sum"] == info["sent_count_sum"] == m.total(), info
        st = dc.finish()
        _check_everything(dc, st, m, k, f"merge_across k={k} pieces={pieces}")


# ---------------------------------------------------------------------------------------------------------------------
# section 5: the command line and the product library
# ---------------------------------------------------------------------------------------------------------------------
BIN = os.path.join(ROOT, "krust_amd", "host", "kmerust")


@pytest.fixture(scope="module")
def read_files(tmp_path_factory):
    R = _reads()
    d = tmp_path_factory.mktemp("small_k")
    fq, fa = d / "reads.fastq", d / "reads.fasta"
    fq.write_bytes(b"".join(b"@r%d\n" % i + r + b"\n+\n" + q + b"\n" for i, (r, q) in enumerate(zip(R["recs"], R["quals"]))))
    fa.write_bytes(b"".join(b">r%d\n" % i + r + b"\n" for i, r in enumerate(R["recs"])))
    assert fq.stat().st_size > 13_000_000
    return str(fq), str(fa)


def _cli(*args, env=None):
    r = subprocess.run([BIN, *args, "-q"], capture_output=True, timeout=600, env=None if env is None else {**os.environ, **env})
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


@pytest.mark.parametrize("host_parse", [None, "1"], ids=["device-parse", "host-parse"])
def test_small_k_command_line(K, read_files, host_parse):
    """`kmerust 5 reads.fastq` and its kin on a file of about 7 M windows, no capacity hint (the default geometry a user gets):
    the output multiset equals the oracle's, with the device text scanner and with KMERUST_HOST_PARSE=1."""
    fq, fa = read_files
    R = _reads()
    env = {"KMERUST_HOST_PARSE": host_parse} if host_parse else None
    full = R["cuts"][3]

    def strs(k, minq):
        return _oracle(k, minq, full).as_str_dict(k)

    out = _cli("5", fq, "--format", "tsv", env=env)
    assert {l.split(b"\t")[0].decode(): int(l.split(b"\t")[1]) for l in out.splitlines()} == strs(5, None)
    assert len(out.splitlines()) == len(strs(5, None))
    out = _cli("5", fq, "--format", "histogram", env=env)
    assert [tuple(map(int, l.split(b"\t"))) for l in out.splitlines()] == _oracle(5, None, full).histogram()
    lines = _cli("3", fa, env=env).splitlines()                       # default format: ">{count}\n{kmer}"
    assert all(l.startswith(b">") for l in lines[::2]) and len(lines) == 2 * len(strs(3, None))
    assert {lines[i + 1].decode(): int(lines[i][1:]) for i in range(0, len(lines), 2)} == strs(3, None)
    out = _cli("9", fq, "-Q", "20", "--format", "tsv", env=env)
    assert {l.split(b"\t")[0].decode(): int(l.split(b"\t")[1]) for l in out.splitlines()} == strs(9, 20)
    assert len(out.splitlines()) == len(strs(9, 20))


PRODUCT_CHILD = r'''
import json, os, sys
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import krust_amd
from krust_amd import native
import oracle_lib as O
import test_gpu_small_k as T
assert native.LIB_PATH.endswith("libkmerhip.so"), native.LIB_PATH
R = T._reads()
out = {}
for k in (3, 5, 9):
    for minq in (None, 20):
        m = T._oracle(k, minq, R["cuts"][3])
        with krust_amd.DeviceCounter(k, min_quality=minq) as dc:      # unhinted: the geometry a user gets
            dc.push(R["bases"], R["qual"] if minq is not None else None)
            st = dc.finish()
            T._check_everything(dc, st, m, k, f"product library k={k} minq={minq}")
        out[f"k{k}-q{minq}"] = {"slots": st["table_slots"], "slot_bytes": st["slot_bytes"], "distinct": st["distinct"]}
print("RESULT " + json.dumps(out))
'''


def test_small_k_product_library_unhinted(K):
    """A fresh process loads the PRODUCT library (no test switches: KMERHIP_TABLE_REGIONS and KMERHIP_NARROW set here are ignored) and
    counts the section-2 reads at k = 3, 5, 9 without a hint: the whole map, histograms and lookups equal the oracle's."""
    env = dict(os.environ)
    env.pop("KMERHIP_LIB", None)
    env.update(KMERHIP_TABLE_REGIONS=str(1024 * 3), KMERHIP_NARROW="0")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\nimport sys\nsys.path.insert(0, ROOT)\n" + PRODUCT_CHILD], capture_output=True, text=True,
                       env=env, timeout=900, cwd=ROOT)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    res = json.loads([l for l in p.stdout.splitlines() if l.startswith("RESULT ")][-1][7:])
    assert len(res) == 6 and all(v["slots"] != 1024 * 3 * 4096 for v in res.values()), res
