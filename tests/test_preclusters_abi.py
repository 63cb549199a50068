"""The device precluster step in the C ABI (CPU only): the two entry points
in the header and in the Python mirror, the timing slot, the ABI version
unchanged.  (test_rust_binding.py holds the header, the Rust declarations and
EXPORTED_SYMBOLS to one another.)"""
import os
import re

import galah_amd as ga
from conftest import ROOT

SYMBOLS = ("gg_preclusters", "gg_preclusters_device")


def _header():
    return open(os.path.join(ROOT, "include", "galahgpu.h")).read()


def test_symbols_in_the_header():
    h = _header()
    for s in SYMBOLS:
        assert re.search(r"\bgg_status\s+%s\s*\(" % s, h), s
    assert re.search(r"GG_KERNEL_PRECLUSTER\s*=\s*13\b", h) and re.search(r"GG_KERNEL_COUNT\s*=\s*14\b", h)


def test_symbols_exported():
    for s in SYMBOLS:
        assert s in ga.EXPORTED_SYMBOLS
        assert hasattr(ga.lib(), s)  # the built library carries it
    assert callable(ga.Context.preclusters) and callable(ga.Context.preclusters_device)


def test_kernel_slot_and_abi_version():
    assert ga.KERNEL_PRECLUSTER == 13
    assert ga.abi_version() == 7
