"""One fresh process for tests/test_gpu_unitig_links.py: loads an input and what the string reference expects of it (an .npz the
parent wrote), builds the linked unitigs once on whatever library and KMERHIP_GRID_CAP the environment names, compares bytes.

    unitig_links_child.py <case.npz>

The .npz holds k, mc, hint, then either `flat` (pushed) or `keys` and `counts` (merged as pairs), and rows, bases, links."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from krust_amd import native  # noqa: E402


def main():
    d = np.load(sys.argv[1])
    k, mc, hint = int(d["k"]), int(d["mc"]), int(d["hint"])
    with native.DeviceCounter(k, capacity_hint=hint) as dc:
        if "flat" in d.files:
            dc.push(d["flat"])
        else:
            dc.merge_pairs(d["keys"], d["counts"])
        rows, bases, links = dc.unitigs_linked(mc)
        assert np.array_equal(rows, d["rows"]), "rows"
        assert np.array_equal(bases, d["bases"]), "bases"
        assert links.dtype == np.uint64 and links.shape == d["links"].shape, (links.shape, d["links"].shape)
        bad = np.flatnonzero(links != d["links"])
        assert bad.size == 0, ("links", bad[:8], links[bad[:8]], d["links"][bad[:8]])
        # the plain begin on the same table: the same rows and bases, and no links to copy
        r2, b2 = dc.unitigs(mc)
        assert np.array_equal(r2, rows) and np.array_equal(b2, bases)
    print("RESULT ok", native.LIB_PATH, "cap", os.environ.get("KMERHIP_GRID_CAP", "-"), "links", links.size)


if __name__ == "__main__":
    main()
