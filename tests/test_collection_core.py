"""The resident collection, CPU part.

The index arithmetic (galah_amd/csrc/collection_core.hpp) is driven on the host
by tests/cpp/test_collection_core.cpp, a stand-alone program built here plainly
and with the address and undefined-behaviour sanitizers: the merge positions
of an old list and a border against std::sort, the survivor / relabel rule
against std::remove_if, and the batch plan of the in-place row compaction
simulated row by row (every batch's destinations end before the first source
row that is yet to be read).  The rest checks the surface: the header, the
Python and Rust mirrors carry the new names, and the argument checks that
need no device."""
import ctypes
import os
import re
import subprocess

import pytest

import galah_amd as ga
from conftest import ROOT

SYMBOLS = ("gg_collection_create", "gg_collection_destroy", "gg_collection_stat", "gg_collection_load",
           "gg_collection_add_rows", "gg_collection_add_rows_device", "gg_collection_add_files",
           "gg_collection_remove", "gg_collection_cluster", "gg_collection_pairs", "gg_collection_rows",
           "gg_collection_view")
INVALID = 1  # GG_ERR_INVALID_ARG


def _build_core_test(exe, flags):
    src = os.path.join(ROOT, "tests", "cpp", "test_collection_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, exe)
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags +
                       ["-o", out, src], capture_output=True, text=True)
    return out, r


def _run_core_test(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word, cases, pairs = r.stdout.strip().splitlines()[-1].split()
    assert word == "ok" and int(cases) >= 400 and int(pairs) >= 100000, r.stdout
    print(r.stdout)


def test_collection_core_rules():
    exe, r = _build_core_test("test_collection_core", ["-O2"])
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def test_collection_core_rules_under_sanitizers():
    exe, r = _build_core_test("test_collection_core_san",
                              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_three_sides_carry_the_collection():
    header, rust = _read("include", "galahgpu.h"), _read("rust", "galah-gpu-sys", "src", "lib.rs")
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert name in ga.EXPORTED_SYMBOLS and hasattr(ga._L, name), name
    assert "typedef struct gg_collection gg_collection;" in header
    assert re.search(r"#\[repr\(C\)\]\s*pub struct gg_collection \{\s*_private: \[u8; 0\],\s*\}", rust)
    assert "#define GG_ABI_VERSION 7u" in header and ga.abi_version() == 7
    fields = [f for f, _ in ga._CollectionInfo._fields_]
    assert fields == ["n_pairs", "pair_capacity", "device_bytes", "n_rows", "row_capacity", "grows", "rows_moved"]
    assert ctypes.sizeof(ga._CollectionInfo) == 40


def test_null_handles_are_refused_without_a_device():
    L = ga._L
    info = ga._CollectionInfo()
    out = ctypes.c_void_p()
    n = ctypes.c_uint64()
    assert L.gg_collection_stat(None, ctypes.byref(info), None) == INVALID
    assert L.gg_collection_create(None, 0.95, 0, 0, ctypes.byref(out)) == INVALID and not out.value
    assert L.gg_collection_load(None, None, None, 0, None, None, 0, 0.95, ctypes.byref(out)) == INVALID
    assert L.gg_collection_add_rows(None, None, None, 0, ctypes.byref(n)) == INVALID
    assert L.gg_collection_add_rows_device(None, None, None, 0, ctypes.byref(n), None) == INVALID
    assert L.gg_collection_add_files(None, None, 0, None, ctypes.byref(n)) == INVALID
    assert L.gg_collection_remove(None, None, 0, None) == INVALID
    assert L.gg_collection_cluster(None, None, 0.95, None) == INVALID
    assert L.gg_collection_pairs(None, None, None, None) == INVALID
    assert L.gg_collection_rows(None, None, None) == INVALID
    assert L.gg_collection_view(None, None, None, None, None) == INVALID
    L.gg_collection_destroy(None)  # as free(NULL)
    assert b"null" in L.gg_thread_last_error()


def test_the_batch_knob_is_documented():
    assert "GALAHGPU_TEST_COLLECTION_BATCH" in _read("galah_amd", "csrc", "collection.cpp")
    design = _read("DESIGN.md")
    seven = design[design.index("\n## 7. "):]
    assert "GALAHGPU_TEST_COLLECTION_BATCH" in seven
