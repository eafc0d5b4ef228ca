"""Every allocation failure of a first kh_unitigs_locate and of a first kh_unitigs_locate_device after a begin, injected one at a time:
the driver, the trace and the inputs are those of tests/test_gpu_alloc_fail.py (sweep(): arm n = 1, 2, 3, ... until the call makes
fewer than n allocations; every step uses a fresh context, ends with kh_destroy and leaves no live allocation).  The calls have no
documented fallback: every injected failure is KH_ERR_OOM, the context is not poisoned, the unitigs are still live and copyable,
nothing of the place map stays allocated, and the same call again gives the right words.  After kh_unitigs_end nothing of the
unitigs or of the map is left on the device.

Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import test_gpu_alloc_fail as A
import test_gpu_unitigs as UN
import test_locate_ref as R
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture)

pytestmark = pytest.mark.gpu

N_BYTES = 151 * 40     # the first forty reads of the input


class Locate(A.Op):
    """state: a table of state (a) / (b) with live unitigs that no call has located yet; the call: the first locate."""

    def __init__(self, state, device):
        self.name, self.state, self.device = "unitigs_locate[%s,%s]" % (state, "device" if device else "host"), state, device

    def build(self):
        I = A.inp()
        dc = A.counted(I, self.state)
        idle = self.tr.snapshot()                 # what the context holds without unitigs
        nu, nb = dc.unitigs_begin(1)
        ref = UN.ref_of(I.tag, I.keys, I.counts, I.k, 1)
        flat = np.asarray(I.bases[:N_BYTES]).copy()
        want = R.locate_ref(ref.rows, np.frombuffer(ref.bases, dtype=np.uint8), I.k, flat.tobytes())
        assert int(np.sum(native.loc_is_place(want))) > 1000
        return {"I": I, "dcs": [dc], "idle": idle, "sizes": (nu, nb), "ref": ref, "flat": flat, "want": want}

    def call(self, st):
        dc, flat = st["dcs"][0], st["flat"]
        st["got"] = None

        def run():
            if self.device:
                import torch
                tb = torch.from_numpy(flat).cuda()
                to = torch.zeros(flat.size, dtype=torch.int64, device="cuda")
                torch.cuda.synchronize()
                dc.unitigs_locate_device(tb, None, flat.size, to)
                st["got"] = to.cpu().numpy().view(np.uint64)
            else:
                st["got"] = dc.unitigs_locate(flat)
        return A.status_of(run)[0]

    def ok(self, st):
        assert np.array_equal(st["got"], st["want"])
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
        nu, nb = st["sizes"]
        rows, bases = dc.unitigs_copy(nu, nb)                                   # the unitigs are still live
        assert np.array_equal(rows, st["ref"].rows) and bases.tobytes() == st["ref"].bases
        assert self.call(st) == A.OK, A.last_error(dc)                          # the same call again
        self.ok(st)


CASES = [("a", False), ("b", False), ("a", True), ("b", True)]


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("state,device", CASES, ids=["%s-%s" % (s, "device" if d else "host") for s, d in CASES])
def test_unitigs_locate(tr, state, device, mode):  # noqa: F811
    A.sweep(tr, Locate(state, device), mode)
