"""kh_compare / kh_combine_into -- two count tables set against each other on the device -- against numpy.

Expected values never come from the library: the two tables are O.OracleMap counts of the reads (or chosen pairs), aligned on
the union of their key arrays, and every word and every result pair is numpy arithmetic on those two count vectors (uint64,
which wraps modulo 2^64 as the header says the sums do).  np.intersect1d / np.isin cross-check the alignment."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
from krust_amd import native

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = np.uint64
MAX = U64(0xFFFFFFFFFFFFFFFF)
OPS = ["intersect", "union", "subtract", "count-subtract"]
CALCS = ["min", "max", "sum", "left", "right"]
MINS = [(1, 1), (0, 0), (2, 1), (1, 3), (2 ** 64 - 1, 1)]
# every op, and every calc where the op uses it
CASES = [(op, calc) for op in ("intersect", "union") for calc in CALCS] + [("subtract", "sum"), ("count-subtract", "sum")]
SEED = 77


# ---- expected values -------------------------------------------------------------------------------------------------------
def align(ka, va, kb, vb):
    """(U, ca, cb): the sorted union of the keys and both count vectors over it, 0 where a table lacks the key."""
    ka, va, kb, vb = (np.asarray(x, dtype=U64) for x in (ka, va, kb, vb))
    u = np.union1d(ka, kb)
    ca, cb = np.zeros(u.size, dtype=U64), np.zeros(u.size, dtype=U64)
    ca[np.searchsorted(u, ka)] = va
    cb[np.searchsorted(u, kb)] = vb
    assert int((np.isin(u, ka) & np.isin(u, kb)).sum()) == np.intersect1d(ka, kb).size == int(((ca > 0) & (cb > 0)).sum())
    return u, ca, cb


def sets_of(ca, cb, min_a, min_b):
    xa = np.where(ca >= U64(max(min_a, 1)), ca, U64(0))
    xb = np.where(cb >= U64(max(min_b, 1)), cb, U64(0))
    return xa, xb


def np_words(ca, cb, min_a=1, min_b=1):
    xa, xb = sets_of(ca, cb, min_a, min_b)
    sh = (xa > 0) & (xb > 0)
    s = lambda v: int(np.sum(v, dtype=U64))  # (wraps modulo 2^64)
    return {"distinct_a": int((xa > 0).sum()), "distinct_b": int((xb > 0).sum()), "shared": int(sh.sum()), "sum_a": s(xa), "sum_b": s(xb),
            "shared_sum_a": s(xa[sh]), "shared_sum_b": s(xb[sh]), "sum_min": s(np.minimum(xa, xb)[sh])}


def np_combine(u, ca, cb, op, calc, min_a=1, min_b=1):
    """The sorted (keys, counts) of the set operation; a pair with count 0 is never produced."""
    xa, xb = sets_of(ca, cb, min_a, min_b)
    both = (xa > 0) & (xb > 0)
    if calc == "min":
        cc = np.minimum(xa, xb)
    elif calc == "max":
        cc = np.maximum(xa, xb)
    elif calc == "sum":
        cc = xa + xb
        cc = np.where(cc < xa, MAX, cc)  # saturates
    elif calc == "left":
        cc = xa
    else:
        cc = xb
    if op == "intersect":
        c = np.where(both, cc, U64(0))
    elif op == "union":
        c = np.where(both, cc, np.maximum(xa, xb))  # (a key of one set: its own count, the other is 0)
    elif op == "subtract":
        c = np.where(xb > 0, U64(0), xa)
    else:
        c = np.where(xa > xb, xa - np.minimum(xa, xb), U64(0))
    sel = c > 0
    return u[sel], c[sel]


_MAPS = {}


def reads(first, n):
    b, _ = O.synth_reads(SEED, 1 << 20, 150, first, n, with_qual=False)
    return np.asarray(b)


def oracle_pairs(k, first, n):
    """(reads, keys, counts) of reads [first, first + n), computed once."""
    if (k, first, n) not in _MAPS:
        r = reads(first, n)
        m = O.OracleMap()
        m.process(r, k)
        keys, counts = m.arrays()
        _MAPS[(k, first, n)] = (r, np.asarray(keys, dtype=U64).copy(), np.asarray(counts, dtype=U64).copy())
    return _MAPS[(k, first, n)]


def sample_ab(k):
    ra, ka, va = oracle_pairs(k, 0, 6000)
    rb, kb, vb = oracle_pairs(k, 3000, 6000)
    return ra, rb, align(ka, va, kb, vb)


# ---- tables in chosen forms ---------------------------------------------------------------------------------------------------
def table(form, k, r, monkeypatch):
    """A counter holding the reads r, in the form asked for; the form it reports is asserted."""
    if form == "regions3072":
        monkeypatch.setenv("KMERHIP_TABLE_REGIONS", "3072")
    if form == "grown":  # (hint 0, and a first table of 64 regions: these reads' keys do not fit it)
        monkeypatch.setenv("KMERHIP_TABLE_REGIONS", "64")
    hint = 0 if form in ("grown", "regions3072") else 3_000_000
    dc = native.DeviceCounter(k, capacity_hint=hint, path={"wide": "direct", "image": "partition"}.get(form))
    monkeypatch.delenv("KMERHIP_TABLE_REGIONS", raising=False)
    if form == "grown":
        dc.push(r[: r.size // 2])
        dc.finish()
        dc.push(r[r.size // 2:])
    else:
        dc.push(r)
    st = dc.finish()
    if form == "wide":
        assert st["slot_bytes"] == 16 and st["part_batches"] == 0
    if form == "image":
        assert st["slot_bytes"] == 8 and st["part_batches"] >= 1 and st["table_slots"] == (1 << 11) * 4096
    if form == "regions3072":
        assert st["table_slots"] == 3072 * 4096
    if form == "grown":
        assert st["grows"] >= 1 and st["table_slots"] > 64 * 4096
    return dc


def stats_of(dc):
    st = dc.finish()
    return tuple(st[f] for f in ("slot_bytes", "distinct", "kmers", "grows", "table_slots"))


def check_all_ops(a, b, dst, u, ca, cb, min_a, min_b, cases=CASES):
    assert a.compare(b, min_a, min_b) == np_words(ca, cb, min_a, min_b)
    for op, calc in cases:
        dst.reset()
        n = dst.combine_into(a, b, op, calc, min_a, min_b)
        ek, ec = np_combine(u, ca, cb, op, calc, min_a, min_b)
        gk, gc = dst.result()
        assert n == ek.size == gk.size, (op, calc, n, ek.size, gk.size)
        assert np.array_equal(gk, ek) and np.array_equal(gc, ec), (op, calc, min_a, min_b)
        st = dst.finish()
        assert st["distinct"] == ek.size and st["kmers"] == int(np.sum(ec, dtype=U64))


PAIRS = [("wide", "wide"), ("image", "image"), ("image", "wide"), ("wide", "image"), ("image", "regions3072"), ("grown", "image")]


@pytest.mark.parametrize("mins", MINS, ids=lambda m: f"min{m[0] if m[0] < 100 else 'max'}-{m[1]}")
@pytest.mark.parametrize("fa,fb", PAIRS)
def test_table_forms_k21(fa, fb, mins, monkeypatch):
    k = 21
    ra, rb, (u, ca, cb) = sample_ab(k)
    w = np_words(ca, cb)
    assert 0.3 < w["shared"] / w["distinct_a"] < 0.7 and w["shared_sum_a"] != w["shared_sum_b"]  # about half shared, other counts
    with table(fa, k, ra, monkeypatch) as a, table(fb, k, rb, monkeypatch) as b, native.DeviceCounter(k, capacity_hint=3_000_000) as dst:
        before = stats_of(a), stats_of(b)
        check_all_ops(a, b, dst, u, ca, cb, *mins)
        assert (stats_of(a), stats_of(b)) == before  # both sources only read, in the form they were in


@pytest.mark.parametrize("mins", MINS, ids=lambda m: f"min{m[0] if m[0] < 100 else 'max'}-{m[1]}")
@pytest.mark.parametrize("k", [5, 31, 32])
def test_wide_wide_other_k(k, mins, monkeypatch):
    ra, rb, (u, ca, cb) = sample_ab(k)
    if k == 5:
        assert u.size == 512 and (ca > 0).all() and (cb > 0).all()  # every canonical 5-mer in both tables
    with table("wide", k, ra, monkeypatch) as a, table("wide", k, rb, monkeypatch) as b, native.DeviceCounter(k, capacity_hint=3_000_000) as dst:
        check_all_ops(a, b, dst, u, ca, cb, *mins)


# ---- chosen counts ----------------------------------------------------------------------------------------------------------------
def test_chosen_counts_saturation_and_wrapping_sums():
    k = 21
    rng = np.random.default_rng(5)
    keys = np.unique(np.array([O.canonical(bytes(rng.choice(list(b"ACGT"), k).astype(np.uint8)))[0] for _ in range(40)], dtype=U64))
    assert keys.size >= 30
    both = [(2 ** 32 - 1, 1), (2 ** 32, 2 ** 32), (2 ** 40, 3), (2 ** 64 - 1, 2), (5, 5), (1, 7)]
    nb = len(both)
    ka = np.concatenate((keys[:nb], keys[nb:nb + 8]))            # the shared keys, then a-only ones
    va = np.array([x for x, _ in both] + [3, 2 ** 63, 2 ** 63, 9, 1, 2 ** 33, 4, 6], dtype=U64)
    kb = np.concatenate((keys[:nb], keys[nb + 8:nb + 14]))       # ... and b-only ones
    vb = np.array([y for _, y in both] + [2 ** 64 - 1, 2 ** 64 - 1, 8, 1, 2 ** 35, 2], dtype=U64)
    u, ca, cb = align(ka, va, kb, vb)
    with native.DeviceCounter(k) as a, native.DeviceCounter(k) as b, native.DeviceCounter(k) as dst:
        a.merge_pairs(ka, va)
        b.merge_pairs(kb, vb)
        assert a.finish()["slot_bytes"] == 16 and b.finish()["slot_bytes"] == 16
        for mins in MINS + [(6, 1), (2 ** 32, 3)]:
            w = np_words(ca, cb, *mins)
            assert a.compare(b, *mins) == w
            for op, calc in CASES:
                dst.reset()
                n = dst.combine_into(a, b, op, calc, *mins)
                ek, ec = np_combine(u, ca, cb, op, calc, *mins)
                gk, gc = dst.result()
                assert n == ek.size and np.array_equal(gk, ek) and np.array_equal(gc, ec), (op, calc, mins)
        # the sums wrap modulo 2^64 (a holds 2^64 - 1 and two 2^63, b two 2^64 - 1)
        w = np_words(ca, cb)
        full = sum(int(x) for x in va)
        assert full > 2 ** 64 and w["sum_a"] == full % 2 ** 64 and a.compare(b)["sum_a"] == w["sum_a"]
        # SUM saturates at 2^64 - 1 ...
        dst.reset()
        dst.combine_into(a, b, "intersect", "sum")
        got = dict(zip(*(x.tolist() for x in dst.result())))
        assert got[int(keys[3])] == 2 ** 64 - 1 and got[int(keys[0])] == 2 ** 32 and got[int(keys[1])] == 2 ** 33
        # ... and COUNT_SUBTRACT drops ca == cb and ca < cb
        dst.reset()
        dst.combine_into(a, b, "count-subtract")
        got = dict(zip(*(x.tolist() for x in dst.result())))
        assert int(keys[4]) not in got and int(keys[1]) not in got and int(keys[5]) not in got
        assert got[int(keys[0])] == 2 ** 32 - 2 and got[int(keys[2])] == 2 ** 40 - 3 and got[int(keys[3])] == 2 ** 64 - 3


# ---- edge cases -----------------------------------------------------------------------------------------------------------------
def test_empty_contexts():
    k = 21
    r, ka, va = oracle_pairs(k, 0, 2000)
    none = np.zeros(0, dtype=U64)
    with native.DeviceCounter(k) as full, native.DeviceCounter(k) as e1, native.DeviceCounter(k) as e2, native.DeviceCounter(k) as dst:
        full.push(r)
        for a, b, (pa, pva), (pb, pvb) in ((e1, full, (none, none), (ka, va)), (full, e1, (ka, va), (none, none)), (e1, e2, (none, none), (none, none))):
            u, ca, cb = align(pa, pva, pb, pvb)
            check_all_ops(a, b, dst, u, ca, cb, 1, 1, cases=[("intersect", "sum"), ("union", "sum"), ("subtract", "sum"), ("count-subtract", "sum")])
        assert e1.result_size() == 0 and e2.result_size() == 0 and full.result_size() == ka.size


def test_a_is_b():
    k = 21
    r, ka, va = oracle_pairs(k, 0, 2000)
    with native.DeviceCounter(k) as a, native.DeviceCounter(k) as dst:
        a.push(r)
        w = a.compare(a)
        assert w == np_words(va, va) and w["shared"] == w["distinct_a"] == w["distinct_b"] == ka.size and w["sum_min"] == w["sum_a"]
        assert dst.combine_into(a, a, "subtract") == 0 and dst.result_size() == 0
        assert dst.combine_into(a, a, "intersect", "left") == ka.size
        gk, gc = dst.result()
        assert np.array_equal(gk, ka) and np.array_equal(gc, va)


def test_dst_not_empty_and_dst_that_must_grow():
    k = 21
    ra, rb, (u, ca, cb) = sample_ab(k)
    ek, ec = np_combine(u, ca, cb, "union", "sum")
    with native.DeviceCounter(k) as a, native.DeviceCounter(k) as b, native.DeviceCounter(k, capacity_hint=1) as dst:
        a.push(ra)
        b.push(rb)
        slots0 = dst.finish()["table_slots"]
        assert slots0 < ek.size
        assert dst.combine_into(a, b, "union", "sum") == ek.size          # a table of a few regions: it grows
        st = dst.finish()
        assert st["grows"] >= 1 and st["table_slots"] > slots0 and st["distinct"] == ek.size
        gk, gc = dst.result()
        assert np.array_equal(gk, ek) and np.array_equal(gc, ec)
        assert dst.combine_into(a, b, "union", "sum") == ek.size          # the same again: count[key] += c
        gk, gc = dst.result()
        assert np.array_equal(gk, ek) and np.array_equal(gc, ec * U64(2))


# ---- the sources are only read ----------------------------------------------------------------------------------------------------
def test_text_stream_on_a_source_goes_on():
    k = 21
    ra, rb, (u, ca, cb) = sample_ab(k)
    with native.DeviceCounter(k) as a, native.DeviceCounter(k) as b, native.DeviceCounter(k, capacity_hint=2_000_000) as dst:
        a.push(ra)
        b.push(rb)
        whole = b"".join(a.result_text("tsv", piece_bytes=1 << 20))
        before = stats_of(a), stats_of(b)
        a.result_text_begin("tsv")
        buf = np.empty(1 << 20, dtype=np.uint8)
        pieces, step = [], 0
        while True:
            n = a.result_text_next(buf)
            if n == 0:
                break
            pieces.append(buf[:n].tobytes())
            if step == 0:
                assert a.compare(b) == np_words(ca, cb)
            elif step == 1:
                assert b.compare(a) == np_words(cb, ca)
            elif step == 2:
                assert dst.combine_into(a, b, "intersect", "min") == np_words(ca, cb)["shared"]
            step += 1
        assert step > 3 and b"".join(pieces) == whole
        assert (stats_of(a), stats_of(b)) == before


def test_pending_pushes_are_counted_first():
    k = 21
    ra, rb, (u, ca, cb) = sample_ab(k)
    with native.DeviceCounter(k) as a, native.DeviceCounter(k) as b, native.DeviceCounter(k) as dst:
        a.push(ra)          # no finish: the reads may still be pending
        b.push(rb)
        assert a.compare(b) == np_words(ca, cb)
    with native.DeviceCounter(k) as a, native.DeviceCounter(k) as b, native.DeviceCounter(k) as dst:
        a.push(ra)
        b.push(rb)
        ek, ec = np_combine(u, ca, cb, "count-subtract", "sum")
        assert dst.combine_into(a, b, "count-subtract") == ek.size
        gk, gc = dst.result()
        assert np.array_equal(gk, ek) and np.array_equal(gc, ec)


# ---- shards -------------------------------------------------------------------------------------------------------------------------
def test_equal_shards_add_up_and_mixed_shards_are_refused():
    import krust_amd
    k = 21
    _, ka, va = oracle_pairs(k, 0, 6000)
    _, kb, vb = oracle_pairs(k, 3000, 6000)
    u, ca, cb = align(ka, va, kb, vb)
    oa, ob = O.owners(krust_amd, ka, k, 2), O.owners(krust_amd, kb, k, 2)
    full = np_words(ca, cb, 2, 1)
    total = dict.fromkeys(full, 0)
    parts_k, parts_c = [], []
    L = native.lib()
    out = np.zeros(8, dtype=U64)
    ctxs = []
    try:
        for r in range(2):
            a, b, dst = (native.DeviceCounter(k, capacity_hint=1_000_000) for _ in range(3))
            ctxs += [a, b, dst]
            for dc in (a, b, dst):
                dc.set_shard(r, 2)
            a.merge_pairs(ka[oa == r], va[oa == r])
            b.merge_pairs(kb[ob == r], vb[ob == r])
            w = a.compare(b, 2, 1)
            ur, car, cbr = align(ka[oa == r], va[oa == r], kb[ob == r], vb[ob == r])
            assert w == np_words(car, cbr, 2, 1)
            for name in total:
                total[name] = (total[name] + w[name]) % 2 ** 64
            n = dst.combine_into(a, b, "union", "max", 2, 1)
            gk, gc = dst.result()
            assert n == gk.size
            parts_k.append(gk)
            parts_c.append(gc)
        assert total == full
        gk, gc = np.concatenate(parts_k), np.concatenate(parts_c)
        o = np.argsort(gk, kind="stable")
        ek, ec = np_combine(u, ca, cb, "union", "max", 2, 1)
        assert np.array_equal(gk[o], ek) and np.array_equal(gc[o], ec)
        # mixed shard states: a full table with a shard, and shard (0, 2) with shard (1, 2)
        a0, b0, d0, a1, b1, d1 = ctxs
        with native.DeviceCounter(k) as fa, native.DeviceCounter(k) as fd:
            fa.merge_pairs(ka, va)
            for x, y in ((fa, b0), (a0, b1)):
                assert L.kh_compare(x._h, y._h, 1, 1, out.ctypes.data) == native.KH_ERR_STATE
            for d, x, y in ((fd, fa, b0), (d0, a0, b1), (d1, a0, b0), (fd, a0, b0)):
                assert L.kh_combine_into(d._h, x._h, y._h, native.SET_UNION, native.CALC_SUM, 1, 1, None) == native.KH_ERR_STATE
            assert fa.result_size() == ka.size and a0.result_size() == int((oa == 0).sum()) and b1.result_size() == int((ob == 1).sum())
    finally:
        for dc in ctxs:
            dc.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_bad_arguments_leave_every_context_usable():
    k = 21
    r, ka, va = oracle_pairs(k, 0, 2000)
    L = native.lib()
    out = np.zeros(8, dtype=U64)
    BAD = native.KH_ERR_BAD_ARG
    with native.DeviceCounter(k) as a, native.DeviceCounter(k) as b, native.DeviceCounter(k) as dst, native.DeviceCounter(19) as c19:
        a.push(r)
        b.push(r[: r.size // 2])
        nb = b.result_size()
        c19.push(r[:151 * 100])
        n19 = c19.result_size()
        I, S = native.SET_INTERSECT, native.CALC_SUM
        assert L.kh_combine_into(a._h, a._h, b._h, I, S, 1, 1, None) == BAD     # dst is a
        assert b"dst" in L.kh_last_error(a._h)
        assert L.kh_combine_into(b._h, a._h, b._h, I, S, 1, 1, None) == BAD     # dst is b
        assert L.kh_combine_into(dst._h, a._h, c19._h, I, S, 1, 1, None) == BAD  # k 21 against k 19
        assert b"different k" in L.kh_last_error(dst._h)
        assert L.kh_combine_into(c19._h, a._h, b._h, I, S, 1, 1, None) == BAD
        assert L.kh_compare(a._h, c19._h, 1, 1, out.ctypes.data) == BAD
        assert b"different k" in L.kh_last_error(a._h)
        assert L.kh_combine_into(dst._h, a._h, b._h, 0, S, 1, 1, None) == BAD   # op 0, op 9
        assert L.kh_combine_into(dst._h, a._h, b._h, 9, S, 1, 1, None) == BAD
        assert L.kh_combine_into(dst._h, a._h, b._h, I, 0, 1, 1, None) == BAD   # calc 0 where the op uses it
        assert L.kh_combine_into(dst._h, a._h, b._h, native.SET_UNION, 6, 1, 1, None) == BAD
        assert L.kh_compare(a._h, b._h, 1, 1, None) == BAD                        # NULL out
        assert L.kh_compare(a._h, None, 1, 1, out.ctypes.data) == BAD and L.kh_compare(None, b._h, 1, 1, out.ctypes.data) == BAD
        assert L.kh_combine_into(dst._h, None, b._h, I, S, 1, 1, None) == BAD and L.kh_combine_into(None, a._h, b._h, I, S, 1, 1, None) == BAD
        assert (a.result_size(), b.result_size(), dst.result_size(), c19.result_size()) == (ka.size, nb, 0, n19)
        # calc is ignored where the op does not use it
        assert dst.combine_into(a, b, native.SET_SUBTRACT, 0) == ka.size - nb
        assert dst.result_size() == ka.size - nb


# ---- the library as it ships ------------------------------------------------------------------------------------------------------------
def test_product_library_once():
    """The same calls on the library as it ships (no test switches): a child process that loads libkmerhip.so."""
    child = r"""
import sys, os
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ["KMERHIP_LIB"] = "libkmerhip.so"
import numpy as np, torch
import oracle_lib as O
from krust_amd import native
import test_gpu_join as T
k = 21
ra, rb, (u, ca, cb) = T.sample_ab(k)
with native.DeviceCounter(k, capacity_hint=3_000_000, path="partition") as a, native.DeviceCounter(k, path="direct") as b, \
        native.DeviceCounter(k, capacity_hint=3_000_000) as dst:
    a.push(ra)
    b.push(rb)
    assert a.finish()["slot_bytes"] == 8 and b.finish()["slot_bytes"] == 16
    T.check_all_ops(a, b, dst, u, ca, cb, 2, 1)
print("RESULT ok", native.LIB_PATH)
"""
    import sys
    env = dict(os.environ, KMERHIP_LIB="libkmerhip.so")
    p = subprocess.run([sys.executable, "-c", f"ROOT = {ROOT!r}\n" + child], capture_output=True, text=True, env=env, timeout=600, cwd=ROOT)
    assert p.returncode == 0 and "RESULT ok" in p.stdout and "libkmerhip.so" in p.stdout, p.stdout[-2000:] + p.stderr[-4000:]
