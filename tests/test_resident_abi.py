"""Clustering from resident sketches in the C ABI (CPU only): the three entry
points and the summary struct in the header and in the Python mirror, the
kernel count and the ABI version unchanged (additions only).
(test_rust_binding.py holds the header, the Rust declarations and
EXPORTED_SYMBOLS to one another.)"""
import ctypes
import os
import re

import galah_amd as ga
from conftest import ROOT

SYMBOLS = ("gg_ani_f32_device", "gg_cluster_rows_device", "gg_cluster_files_resident")
SUMMARY_FIELDS = (("n_pairs", "uint64_t"), ("ani_rechecked", "uint64_t"), ("n_preclusters", "uint32_t"),
                  ("largest_precluster", "uint32_t"), ("pair_passes", "uint32_t"), ("reserved", "uint32_t"))


def _header():
    return open(os.path.join(ROOT, "include", "galahgpu.h")).read()


def test_symbols_and_struct_in_the_header():
    h = _header()
    for s in SYMBOLS:
        assert re.search(r"\bgg_status\s+%s\s*\(" % s, h), s
    m = re.search(r"typedef\s+struct\s+gg_cluster_summary\s*\{(.*?)\}\s*gg_cluster_summary\s*;", h, flags=re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", " ", m.group(1), flags=re.S)
    fields = [tuple(reversed(f.split())) for f in body.split(";") if f.strip()]
    assert fields == list(SUMMARY_FIELDS)


def test_kernel_count_and_abi_version_unchanged():
    h = _header()
    assert re.search(r"GG_KERNEL_COUNT\s*=\s*14\b", h)
    assert re.search(r"#define\s+GG_ABI_VERSION\s+7u\b", h)
    assert ga.abi_version() == 7


def test_python_mirror():
    for s in SYMBOLS:
        assert s in ga.EXPORTED_SYMBOLS
        assert hasattr(ga.lib(), s)  # the built library carries it
    for name in ("ani_f32_device", "cluster_rows_device", "cluster_files_resident"):
        assert callable(getattr(ga.Context, name)), name
    # the mirror's struct has the header's layout: 2 x u64, 4 x u32
    assert [f for f, _ in ga._ClusterSummary._fields_] == [f for f, _ in SUMMARY_FIELDS]
    assert ctypes.sizeof(ga._ClusterSummary) == 32
