"""Every allocation failure of a first kh_unitigs_components and of a first kh_unitigs_components_device after a
kh_unitigs_begin_linked, and of one kh_drop_components_into call, injected one at a time: the driver, the trace and the inputs are
those of tests/test_gpu_alloc_fail.py (sweep(): arm n = 1, 2, 3, ... until the call makes fewer than n allocations; every step uses
fresh contexts, ends with kh_destroy and leaves no live allocation).

The device form allocates the labelling's scratch and the labels; the host form the pinned staging of the way back in front of
them.  Every injected failure is KH_ERR_OOM, the context is not poisoned, the unitigs are still live and their links copyable,
nothing of the labels or of the scratch stays allocated, and the same call again gives the reference's answer.  A second device-form
call allocates nothing and returns the same words.  The drop call follows kh_pop_bubbles_into: a failure on src's side leaves src
usable, dst holding what it held and nothing allocated; one on dst's side poisons dst alone, until kh_reset.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import test_components_ref as R
import test_gpu_alloc_fail as A
import test_gpu_unitig_links as LR
import test_gpu_unitigs as UN
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
PREFILL = 7


def refs(I):
    return UN.ref_of(I.tag, I.keys, I.counts, I.k, 1), LR.links_of(I.tag, I.keys, I.counts, I.k, 1), R.comp_of(I.tag, I.keys, I.counts, I.k, 1)


class Components(A.Op):
    """state: a table of state (a) / (b) with live linked unitigs that no call has asked for components yet; the call: the first one."""

    def __init__(self, state, device):
        self.name, self.state, self.device = "unitigs_components[%s,%s]" % (state, "device" if device else "host"), state, device

    def build(self):
        I = A.inp()
        dc = A.counted(I, self.state)
        idle = self.tr.snapshot()                 # what the context holds without unitigs
        nu, nb, nl = dc.unitigs_begin_linked(1)
        ref, lref, cref = refs(I)
        assert nu == cref.comp.size and nl == lref.links.size and cref.rows.shape[0] > 1 and nl > 0
        return {"I": I, "dcs": [dc], "idle": idle, "nu": nu, "nl": nl, "cref": cref, "links": lref.links}

    def call(self, st):
        dc, nu, C_ = st["dcs"][0], st["nu"], st["cref"].rows.shape[0]
        st["got"] = None
        out = np.zeros(native.CC_WORDS, dtype=U64)
        if self.device:
            import torch
            t_comp = torch.zeros(nu, dtype=torch.int32, device="cuda")
            t_rows = torch.zeros(C_ * native.COMP_WORDS, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            rc = native.lib().kh_unitigs_components_device(dc._h, t_comp.data_ptr(), nu, t_rows.data_ptr(), C_, out.ctypes.data)
            if rc == A.OK:
                st["got"] = (t_comp.cpu().numpy().view(np.uint32), t_rows.cpu().numpy().view(U64).reshape(-1, native.COMP_WORDS), out)
                st.setdefault("events", []).extend(self.tr.sync())             # (the sweep reads them)
                out2 = np.zeros(native.CC_WORDS, dtype=U64)                      # a second device-form call allocates nothing
                assert native.lib().kh_unitigs_components_device(dc._h, t_comp.data_ptr(), nu, t_rows.data_ptr(), C_, out2.ctypes.data) == A.OK
                assert [e for e in self.tr.sync() if e[0] == "A"] == [] and np.array_equal(out2, out)
            return rc
        comp = np.zeros(nu, dtype=np.uint32)                                    # (one call: the staging, the scratch and the labels under the sweep)
        rows = np.zeros((C_, native.COMP_WORDS), dtype=U64)
        rc = native.lib().kh_unitigs_components(dc._h, comp.ctypes.data, nu, rows.ctypes.data, C_, out.ctypes.data)
        if rc == A.OK:
            st["got"] = (comp, rows, out)
        return rc

    def ok(self, st):
        cref, nu = st["cref"], st["nu"]
        comp, rows, out = st["got"]
        assert np.array_equal(comp, cref.comp) and np.array_equal(rows, cref.rows)
        assert out[:3].tolist() == cref.words and 1 <= int(out[native.CC_ROUNDS]) <= R.round_bound(nu)
        dc = st["dcs"][0]
        labels = ("dev", 32 * cref.rows.shape[0] + 4 * nu)
        assert labels in self.tr.snapshot().values()                             # the labels live with the unitigs ...
        dc.unitigs_end()
        left = {p: v for p, v in self.tr.snapshot().items() if p not in st["idle"]}
        assert [v for v in left.values() if v[0] == "dev"] == [], ("left on the device after kh_unitigs_end", left)   # ... and die with them
        A.table_is(dc, st["I"])

    def failed(self, st, rc, tr, before):
        dc = st["dcs"][0]
        assert rc == A.OOM, rc
        msg = A.last_error(dc)
        assert A.names_an_allocation(msg) and "poisoned" not in msg, msg
        left = {p: v for p, v in tr.snapshot().items() if p not in before}
        assert [v for v in left.values() if v[0] == "dev"] == [], (self.name, "the failed call left device memory allocated", left)
        if self.device:
            assert left == {}, (self.name, "the failed call left memory allocated", left)
        else:                                     # (what the rule lets a context keep: the two pinned staging buffers)
            assert len(left) in (0, 2) and len(set(left.values())) <= 1, (self.name, "the failed call left memory allocated", left)
        assert np.array_equal(dc.unitigs_links_copy(st["nl"]), st["links"])      # the unitigs are still live
        assert self.call(st) == A.OK, A.last_error(dc)                           # the same call again
        self.ok(st)


CASES = [("a", False), ("b", False), ("a", True), ("b", True)]


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("state,device", CASES, ids=["%s-%s" % (s, "device" if d else "host") for s, d in CASES])
def test_unitigs_components(tr, state, device, mode):  # noqa: F811
    A.sweep(tr, Components(state, device), mode)


class Drop(A.Op):
    """src: a state (a) / (b) table; dst: a table that holds PREFILL at three of src's keys."""

    def __init__(self, src):
        self.name, self.src = "drop_components_into[src=%s]" % src, src

    def fill(self, dst, I):
        dst.merge_pairs(I.keys[:3], np.full(3, PREFILL, dtype=U64))
        assert dst.finish()["distinct"] == 3

    def bound(self, I):
        return int(refs(I)[2].rows[:, native.COMP_KMERS].max())                  # keeps the largest component, drops the rest

    def build(self):
        I = A.inp()
        dst = native.DeviceCounter(I.k, path="direct")
        self.fill(dst, I)
        return {"I": I, "dcs": [dst, A.counted(I, self.src)]}

    def call(self, st):
        dst, src = st["dcs"]
        out = np.zeros(native.DROP_WORDS, dtype=U64)
        rc = A.lib().kh_drop_components_into(A.h(dst), A.h(src), 1, self.bound(st["I"]), out.ctypes.data)
        st["words"] = dict(zip(native.DROP_NAMES, (int(x) for x in out)))
        return rc

    def ok(self, st):
        I = st["I"]
        dr = R.drop_of(I.tag, I.keys, I.counts, I.k, 1, self.bound(I))
        assert dr.words[native.DROP_DROPPED] > 0 and dr.keys.size > 0
        assert st["words"] == dict(zip(native.DROP_NAMES, dr.words)), (st["words"], dr.words)
        d = dict(zip(dr.keys.tolist(), dr.counts.tolist()))
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
def test_drop_components_into(tr, src, mode):  # noqa: F811
    A.sweep(tr, Drop(src), mode)
