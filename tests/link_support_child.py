"""Child of tests/test_gpu_link_support.py::test_grid_stride: KMERHIP_GRID_CAP is one value per process, so the tile-edge case and the
branchy case run here, in a process that starts with the cap in its environment.  Prints "RESULT ok <library>" at the end."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from krust_amd import native  # noqa: E402
import test_gpu_link_support as GS  # noqa: E402

assert os.environ.get("KMERHIP_GRID_CAP") in ("1", "3")
GS.tile_edge_case()
GS.branchy_case(21)
print("RESULT ok", native.LIB_PATH)
