"""KMERHIP_GRID_CAP is a switch of the test build only: the product library does not hold the name."""
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "krust_amd", "lib")


def test_grid_cap_switch_is_in_the_test_build_only():
    product, testing = os.path.join(LIB, "libkmerhip.so"), os.path.join(LIB, "libkmerhip_testing.so")
    if not (os.path.exists(product) and os.path.exists(testing)):
        pytest.skip("the libraries are not built")
    with open(testing, "rb") as f:
        assert b"KMERHIP_GRID_CAP" in f.read()
    with open(product, "rb") as f:
        assert b"KMERHIP_GRID_CAP" not in f.read()
