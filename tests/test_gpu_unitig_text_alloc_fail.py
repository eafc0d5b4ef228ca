"""Every allocation failure of kh_unitigs_text_begin and of the first kh_unitigs_text_next, injected one at a time: the driver, the
trace and the inputs are those of tests/test_gpu_alloc_fail.py (sweep(): arm n = 1, 2, 3, ... until the calls make fewer than n
allocations; every step uses a fresh context, ends with kh_destroy and leaves no live allocation).  The calls have no documented
fallback: every injected failure is KH_ERR_OOM, the context is not poisoned, the unitigs are still live and copyable, no stream is on,
and the retried calls give the right document.  After kh_unitigs_end nothing of the unitigs or of the stream is left allocated.

Run with `pytest -m gpu` on an MI355X."""
import numpy as np
import pytest

import test_gpu_alloc_fail as A
import test_gpu_unitig_links as LR
import test_gpu_unitig_text as X
import test_gpu_unitigs as UN
from krust_amd import native
from test_gpu_alloc_fail import tr  # noqa: F401  (the module's trace fixture)

pytestmark = pytest.mark.gpu


class Text(A.Op):
    """state: a table of state (a) / (b) with live linked unitigs; the call: begin and the first next (the whole document)."""

    def __init__(self, state, fmt, device):
        self.name, self.state, self.fmt, self.device = "unitigs_text[%s,%s,%s]" % (state, fmt, "device" if device else "host"), state, fmt, device

    def build(self):
        I = A.inp()
        dc = A.counted(I, self.state)
        idle = self.tr.snapshot()                 # what the context holds without unitigs
        nu, nb, nl = dc.unitigs_begin_linked(1)
        ref, lref = UN.ref_of(I.tag, I.keys, I.counts, I.k, 1), LR.links_of(I.tag, I.keys, I.counts, I.k, 1)
        want = X.document(self.fmt, ref.rows, np.frombuffer(ref.bases, dtype=np.uint8), lref.links, I.k)
        return {"I": I, "dcs": [dc], "idle": idle, "sizes": (nu, nb, nl), "ref": ref, "links": lref.links, "want": want}

    def call(self, st):
        dc = st["dcs"][0]
        st["got"] = None

        def both():
            total = dc.unitigs_text_begin(self.fmt)
            if self.device:
                import torch
                t = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
                n = dc.unitigs_text_next_device(t.data_ptr() + 1, total)
                st["got"] = t[1:1 + n].cpu().numpy().tobytes()
            else:
                buf = np.empty(total + 16, dtype=np.uint8)
                n = dc.unitigs_text_next(buf, total)
                st["got"] = buf[:n].tobytes()
        return A.status_of(both)[0]

    def ok(self, st):
        assert st["got"] == st["want"]
        dc = st["dcs"][0]
        dc.unitigs_end()
        pins = {p: v for p, v in self.tr.snapshot().items() if p not in st["idle"]}
        assert all(v[0] == "pin" for v in pins.values()), ("left allocated after kh_unitigs_end", pins)   # (the context's staging chunks stay)
        A.table_is(dc, st["I"])

    def failed(self, st, rc, tr, before):
        dc, I = st["dcs"][0], st["I"]
        assert rc == A.OOM, rc
        msg = A.last_error(dc)
        assert A.names_an_allocation(msg) and "poisoned" not in msg, msg
        left = {p: v for p, v in tr.snapshot().items() if p not in before}
        assert all(v[0] == "pin" for v in left.values()), (self.name, "the failed call left device memory allocated", left)
        nu, nb, nl = st["sizes"]
        rows, bases = dc.unitigs_copy(nu, nb)                                   # the unitigs are still live
        assert np.array_equal(rows, st["ref"].rows) and bases.tobytes() == st["ref"].bases
        assert np.array_equal(dc.unitigs_links_copy(nl), st["links"])
        assert A.status_of(lambda: dc.unitigs_text_next(np.empty(16, dtype=np.uint8)))[0] == A.STATE      # no stream is on
        assert self.call(st) == A.OK, A.last_error(dc)                          # the retried calls
        self.ok(st)


CASES = [("a", "gfa", False), ("b", "gfa", False), ("a", "fasta", False), ("a", "gfa", True)]


@pytest.mark.parametrize("mode", ["", "+"], ids=["n", "n+"])
@pytest.mark.parametrize("state,fmt,device", CASES, ids=["%s-%s-%s" % (s, f, "device" if d else "host") for s, f, d in CASES])
def test_unitigs_text(tr, state, fmt, device, mode):  # noqa: F811
    A.sweep(tr, Text(state, fmt, device), mode)
