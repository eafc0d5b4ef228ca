"""Child of tests/test_gpu_components.py: the library (KMERHIP_LIB) and KMERHIP_GRID_CAP are one value per process, so the product
library's run and the runs past the first grid stride happen here, in a process that starts with them in its environment: the
components and one drop on the planted input, and 1025 disjoint reads.  Prints "cap <n>" and "RESULT ok <library>" at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from krust_amd import native  # noqa: E402
import test_gpu_components as GC  # noqa: E402

cap = os.environ.get("KMERHIP_GRID_CAP")
assert cap in (None, "1", "3")
cref = GC.planted_case()
if cap:
    blocks = -(-cref.comp.size // 256)
    assert blocks > int(cap) and -(-blocks // int(cap)) >= 2, blocks
GC.disjoint_case()
print("cap", cap)
print("RESULT ok", native.LIB_PATH)
