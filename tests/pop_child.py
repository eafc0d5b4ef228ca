"""One fresh process for tests/test_gpu_pop.py: loads an input and what the string reference expects of one round of bubble popping
(an .npz the parent wrote), runs kh_pop_bubbles_into once on whatever library and KMERHIP_GRID_CAP the environment names, compares.

    pop_child.py <case.npz>

The .npz holds k, mc, max_kmers, hint, `flat` (pushed), and keys, counts, words: the surviving pairs and the nine words."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from krust_amd import native  # noqa: E402


def main():
    d = np.load(sys.argv[1])
    k, mc, mk, hint = int(d["k"]), int(d["mc"]), int(d["max_kmers"]), int(d["hint"])
    with native.DeviceCounter(k, capacity_hint=hint) as src, native.DeviceCounter(k, capacity_hint=hint) as dst:
        src.push(d["flat"])
        before = src.finish()["distinct"]
        got = dst.pop_bubbles_into(src, mc, mk)
        assert [got[n] for n in native.POP_NAMES] == [int(w) for w in d["words"]], (got, d["words"])
        gk, gc = dst.result_sorted(1)
        assert gk.shape == d["keys"].shape, (gk.shape, d["keys"].shape)
        bad = np.flatnonzero((gk != d["keys"]) | (gc != d["counts"]))
        assert bad.size == 0, ("pairs", bad[:8])
        assert src.finish()["distinct"] == before
    print("RESULT ok", native.LIB_PATH, "cap", os.environ.get("KMERHIP_GRID_CAP", "-"), "popped", got["popped"])


if __name__ == "__main__":
    main()
