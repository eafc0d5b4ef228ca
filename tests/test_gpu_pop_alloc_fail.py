"""Every allocation failure of one kh_pop_bubbles_into call, injected one at a time: the driver, the trace and the inputs are those of
tests/test_gpu_alloc_fail.py (sweep(): arm n = 1, 2, 3, ... until a call makes fewer than n allocations; every step uses fresh
contexts, ends with kh_destroy and leaves no live allocation).  The call has no documented fallback: every injected failure is
KH_ERR_OOM.  One on src's side (its scratch) leaves src usable, dst holding what it held and nothing allocated; one on dst's side
poisons dst alone, until kh_reset.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_alloc_fail as A
import test_gpu_pop as P
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
PREFILL = 7


class Pop(A.Op):
    """src: a state (a) / (b) table; dst: a table that holds PREFILL at three of src's keys."""

    def __init__(self, src):
        self.name, self.src = "pop_bubbles_into[src=%s]" % src, src

    def fill(self, dst, I):
        dst.merge_pairs(I.keys[:3], np.full(3, PREFILL, dtype=U64))
        assert dst.finish()["distinct"] == 3

    def build(self):
        I = A.inp()
        dst = native.DeviceCounter(I.k, path="direct")
        self.fill(dst, I)
        return {"I": I, "dcs": [dst, A.counted(I, self.src)]}

    def call(self, st):
        dst, src = st["dcs"]
        out = np.zeros(native.POP_WORDS, dtype=U64)
        rc = A.lib().kh_pop_bubbles_into(A.h(dst), A.h(src), 1, 2 * st["I"].k, out.ctypes.data)
        st["words"] = dict(zip(native.POP_NAMES, (int(x) for x in out)))
        return rc

    def ok(self, st):
        I = st["I"]
        pr = P.pop_of(I.tag, I.keys, I.counts, I.k, 1, 2 * I.k)
        assert st["words"] == P.words_dict(pr), (st["words"], P.words_dict(pr))
        d = dict(zip(pr.keys.tolist(), pr.counts.tolist()))
        for key in I.keys[:3].tolist():
            d[key] = d.get(key, 0) + PREFILL
        gk, gc = st["dcs"][0].result_sorted()
        assert gk.tolist() == sorted(d) and gc.tolist() == [d[x] for x in sorted(d)]
        A.table_is(st["dcs"][1], I)

    def failed(self, st, rc, tr, before):
        dst, src = st["dcs"]
        I = st["I"]
        assert rc == A.OOM and A.names_an_allocation(A.last_error(dst)), (rc, A.last_error(dst))
        n = C.c_uint64(0)
        if A.lib().kh_result_size(A.h(dst), 1, C.byref(n)) == A.OK:       # src's scratch: dst holds what it held, nothing stays allocated
            assert tr.snapshot() == before, (self.name, "the failed call left memory allocated")
            gk, gc = dst.result_sorted()
            assert np.array_equal(gk, I.keys[:3]) and gc.tolist() == [PREFILL] * 3
        else:                                                              # dst's side: poisoned, until kh_reset
            assert "poisoned" in A.last_error(dst)
            assert A.lib().kh_reset(A.h(dst)) == A.OK
            self.fill(dst, I)
        A.table_is(src, I)                                                 # src: usable and unchanged, whichever side failed
        assert self.call(st) == A.OK, A.last_error(dst)
        self.ok(st)


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("src", ["a", "b"])
def test_pop_bubbles_into(tr, src, mode):  # noqa: F811
    A.sweep(tr, Pop(src), mode)
