"""The child process of tests/test_gpu_unitig_text.py::test_grid_stride: KMERHIP_GRID_CAP is one value per process, so the parent sets it
and starts this.  `python unitig_text_grid_child.py DIR`: the FASTA and GFA text of the branching input (k = 21, min_count 2) through
kh_unitigs_text_*, in chunks of eight tiles and as one chunk, against the bytes the parent left in DIR/fasta and DIR/gfa."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
os.environ.setdefault("KMERHIP_LIB", "libkmerhip_testing.so")   # (the cap is a switch of the test build)

import test_gpu_graph as G  # noqa: E402
from krust_amd import native  # noqa: E402

cap = int(os.environ["KMERHIP_GRID_CAP"])
assert cap in (1, 3), cap
k = 21
flat, keys, counts = G.main_input(k)
with native.DeviceCounter(k, capacity_hint=3_000_000) as dc:
    dc.push(flat)
    for fmt in ("fasta", "gfa"):
        want = open(os.path.join(sys.argv[1], fmt), "rb").read()
        assert len(want) >= 8 * native.UNI_TEXT_TILE
        for chunk_kb in (str(8 * native.UNI_TEXT_TILE // 1024), None):
            if chunk_kb is None:
                os.environ.pop("KMERHIP_UNI_TEXT_CHUNK_KB", None)
            else:
                os.environ["KMERHIP_UNI_TEXT_CHUNK_KB"] = chunk_kb
            if fmt == "gfa":
                dc.unitigs_begin_linked(2)
            else:
                dc.unitigs_begin(2)
            got = dc.unitigs_text(fmt)
            dc.unitigs_end()
            assert got == want, (fmt, chunk_kb, len(got), len(want))
print("unitig_text_grid_child ok (cap %d)" % cap)
