"""Every allocation failure of a first kh_unitigs_paths and of a first kh_unitigs_paths_device after a begin, injected one at a time:
the driver, the trace and the inputs are those of tests/test_gpu_alloc_fail.py (sweep(): arm n = 1, 2, 3, ... until the call makes
fewer than n allocations; every step uses a fresh context, ends with kh_destroy and leaves no live allocation).  The calls have no
documented fallback: every injected failure is KH_ERR_OOM, the context is not poisoned, the unitigs are still live and copyable,
nothing of the place map or of the call's scratch stays allocated, and the same call again gives the reference's answer.  After
kh_unitigs_end nothing of the unitigs or of the map is left on the device.

Run with `pytest -m gpu` on an MI355X."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_alloc_fail as A
import test_gpu_unitigs as UN
import test_locate_ref as R
import test_paths_ref as P
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture)

pytestmark = pytest.mark.gpu

N_READS = 40
N_BYTES = 151 * N_READS     # the first forty reads of the input


class Paths(A.Op):
    """state: a table of state (a) / (b) with live unitigs that no call has located yet; the call: the first paths call, with room for
    every run and a coverage array."""

    def __init__(self, state, device):
        self.name, self.state, self.device = "unitigs_paths[%s,%s]" % (state, "device" if device else "host"), state, device

    def build(self):
        I = A.inp()
        dc = A.counted(I, self.state)
        idle = self.tr.snapshot()                 # what the context holds without unitigs
        nu, nb = dc.unitigs_begin(1)
        ref = UN.ref_of(I.tag, I.keys, I.counts, I.k, 1)
        flat = np.asarray(I.bases[:N_BYTES]).copy()
        rs = np.arange(0, N_BYTES + 1, 151, dtype=np.uint64)
        words = R.locate_ref(ref.rows, np.frombuffer(ref.bases, dtype=np.uint8), I.k, flat.tobytes())
        want = P.paths_ref(words, rs, nu)
        assert want[1].shape[0] > N_READS and int(want[2][:, native.COV_WINDOWS].sum()) > 1000
        return {"I": I, "dcs": [dc], "idle": idle, "sizes": (nu, nb), "ref": ref, "flat": flat, "rs": rs, "want": want}

    def call(self, st):
        dc, flat, rs, (nu, nb) = st["dcs"][0], st["flat"], st["rs"], st["sizes"]
        cap = st["want"][1].shape[0]
        st["got"] = None
        if self.device:
            import torch
            tb, t_rs = torch.from_numpy(flat).cuda(), torch.from_numpy(rs.view(np.int64)).cuda()
            t_st = torch.zeros(rs.size, dtype=torch.int64, device="cuda")
            t_rows = torch.zeros(cap * native.RUN_WORDS, dtype=torch.int32, device="cuda")
            t_cov = torch.zeros(nu * native.COV_WORDS, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            total = C.c_uint64(0)
            rc = native.lib().kh_unitigs_paths_device(dc._h, tb.data_ptr(), None, flat.size, t_rs.data_ptr(), rs.size - 1, t_st.data_ptr(),
                                                      t_rows.data_ptr(), cap, t_cov.data_ptr(), C.byref(total))
            if rc == A.OK:
                st["got"] = (t_st.cpu().numpy().view(np.uint64), t_rows.cpu().numpy().view(np.uint32).reshape(-1, native.RUN_WORDS)[:total.value],
                             t_cov.cpu().numpy().view(np.uint64).reshape(nu, native.COV_WORDS))
            return rc

        def run():
            cover = np.zeros((nu, native.COV_WORDS), dtype=np.uint64)
            run_start, rows = dc.unitigs_paths(flat, rs, cover=cover, run_cap=cap)
            st["got"] = (run_start, rows, cover)
        return A.status_of(run)[0]

    def ok(self, st):
        for got, want in zip(st["got"], st["want"]):
            assert np.array_equal(got, want)
        dc = st["dcs"][0]
        dc.unitigs_end()
        left = {p: v for p, v in self.tr.snapshot().items() if p not in st["idle"]}
        devs = [v for v in left.values() if v[0] == "dev"]   # (pinned staging of the context stays: that of the copies, and the chunks' twins)
        if self.device:
            assert devs == [], ("left on the device after kh_unitigs_end", left)
        else:                                     # (the context's two chunk buffers stay, as kh_profile's do)
            assert len(devs) == 2 and devs[0] == devs[1], ("left on the device after kh_unitigs_end", left)
        A.table_is(dc, st["I"])

    def failed(self, st, rc, tr, before):
        dc, I = st["dcs"][0], st["I"]
        assert rc == A.OOM, rc
        msg = A.last_error(dc)
        assert A.names_an_allocation(msg) and "poisoned" not in msg, msg
        slots = dc.finish()["table_slots"]
        left = {p: v for p, v in tr.snapshot().items() if p not in before}
        assert not [v for v in left.values() if v == ("dev", 8 * slots)], (self.name, "the failed call left the place map allocated", left)
        if self.device:
            assert left == {}, (self.name, "the failed call left memory allocated", left)
        else:                                     # (what the rule lets a context keep: the chunk buffers and their pinned twins)
            devs = [v for v in left.values() if v[0] == "dev"]
            assert len(devs) in (0, 2) and len(set(devs)) <= 1, (self.name, "the failed call left memory allocated", left)
        nu, nb = st["sizes"]
        rows, bases = dc.unitigs_copy(nu, nb)                                   # the unitigs are still live
        assert np.array_equal(rows, st["ref"].rows) and bases.tobytes() == st["ref"].bases
        assert self.call(st) == A.OK, A.last_error(dc)                          # the same call again
        self.ok(st)


CASES = [("a", False), ("b", False), ("a", True), ("b", True)]


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("state,device", CASES, ids=["%s-%s" % (s, "device" if d else "host") for s, d in CASES])
def test_unitigs_paths(tr, state, device, mode):  # noqa: F811
    A.sweep(tr, Paths(state, device), mode)
