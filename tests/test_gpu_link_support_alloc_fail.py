"""Every allocation failure of a first kh_unitigs_link_support and of a first kh_unitigs_link_support_device after a
kh_unitigs_begin_linked, injected one at a time: the driver, the trace and the inputs are those of tests/test_gpu_alloc_fail.py
(sweep(): arm n = 1, 2, 3, ... until the call makes fewer than n allocations; every step uses a fresh context, ends with kh_destroy and
leaves no live allocation).  The device form allocates the link index and nothing else; the host form the pinned staging of the way
back, the call's arrays and the index.  Every injected failure is KH_ERR_OOM, the context is not poisoned, the unitigs are still live
and their links copyable, nothing of the index or of the call's scratch stays allocated, and the same call again gives the
reference's answer.  A second device-form call allocates nothing.

Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import test_gpu_alloc_fail as A
import test_gpu_unitigs as UN
import test_link_support_ref as S
import test_locate_ref as R
import test_paths_ref as P
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture)

pytestmark = pytest.mark.gpu

U64 = np.uint64
N_READS = 40
N_BYTES = 151 * N_READS     # the first forty reads of the input


class Support(A.Op):
    """state: a table of state (a) / (b) with live linked unitigs that no call has asked for support yet; the call: the first one."""

    def __init__(self, state, device):
        self.name, self.state, self.device = "unitigs_link_support[%s,%s]" % (state, "device" if device else "host"), state, device

    def build(self):
        I = A.inp()
        dc = A.counted(I, self.state)
        idle = self.tr.snapshot()                 # what the context holds without unitigs
        nu, nb, nl = dc.unitigs_begin_linked(1)
        import torch
        t_links = torch.zeros(nl, dtype=torch.int64, device="cuda")             # (the device copy: the host copy would allocate the pinned
        torch.cuda.synchronize()                                                #  staging that the host form is to allocate under the sweep)
        dc.unitigs_links_copy_device(t_links, nl)
        links = t_links.cpu().numpy().view(U64).copy()
        ref = UN.ref_of(I.tag, I.keys, I.counts, I.k, 1)
        flat = np.asarray(I.bases[:N_BYTES]).copy()
        rs = np.arange(0, N_BYTES + 1, 151, dtype=U64)
        words = R.locate_ref(ref.rows, np.frombuffer(ref.bases, dtype=np.uint8), I.k, flat.tobytes())
        run_start, rows, _ = P.paths_ref(words, rs, nu)
        want = S.link_support_ref(run_start, rows, links)
        assert int(want[1][native.SUP_CREDITED]) > 10 and int(want[1][native.SUP_MISSING]) == 0
        return {"I": I, "dcs": [dc], "idle": idle, "nu": nu, "links": links, "run_start": run_start, "rows": rows, "want": want}

    def call(self, st):
        dc, run_start, rows, nl = st["dcs"][0], st["run_start"], st["rows"], st["links"].size
        st["got"] = None
        if self.device:
            import torch
            t_rs = torch.from_numpy(run_start.view(np.int64)).cuda()
            t_rows = torch.from_numpy(np.ascontiguousarray(rows).view(np.int32)).cuda()
            t_sup = torch.zeros(nl, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            out = np.zeros(native.SUP_WORDS, dtype=U64)
            rc = native.lib().kh_unitigs_link_support_device(dc._h, t_rs.data_ptr(), run_start.size - 1, t_rows.data_ptr(), rows.shape[0],
                                                             t_sup.data_ptr(), nl, out.ctypes.data)
            if rc == A.OK:
                st["got"] = (t_sup.cpu().numpy().view(U64), out)
                st.setdefault("events", []).extend(self.tr.sync())             # (the sweep reads them)
                out2 = np.zeros(native.SUP_WORDS, dtype=U64)                     # a second device-form call allocates nothing
                assert native.lib().kh_unitigs_link_support_device(dc._h, t_rs.data_ptr(), run_start.size - 1, t_rows.data_ptr(), rows.shape[0],
                                                                   t_sup.data_ptr(), nl, out2.ctypes.data) == A.OK
                assert [e for e in self.tr.sync() if e[0] == "A"] == [] and np.array_equal(out2, out)
            return rc

        def run():
            support, stats = dc.unitigs_link_support(run_start, rows)
            st["got"] = (support, np.array([stats[n] for n in native.SUP_NAMES], dtype=U64))
        return A.status_of(run)[0]

    def ok(self, st):
        for got, want in zip(st["got"], st["want"]):
            assert np.array_equal(got, want)
        dc = st["dcs"][0]
        index = ("dev", 8 * (2 * st["nu"] + native.SUP_WORDS))
        assert index in self.tr.snapshot().values()                              # the index lives with the unitigs ...
        dc.unitigs_end()
        left = {p: v for p, v in self.tr.snapshot().items() if p not in st["idle"]}
        assert [v for v in left.values() if v[0] == "dev"] == [], ("left on the device after kh_unitigs_end", left)   # ... and dies with them
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
        assert np.array_equal(dc.unitigs_links_copy(st["links"].size), st["links"])   # the unitigs are still live
        assert self.call(st) == A.OK, A.last_error(dc)                          # the same call again
        self.ok(st)


CASES = [("a", False), ("b", False), ("a", True), ("b", True)]


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("state,device", CASES, ids=["%s-%s" % (s, "device" if d else "host") for s, d in CASES])
def test_unitigs_link_support(tr, state, device, mode):  # noqa: F811
    A.sweep(tr, Support(state, device), mode)
