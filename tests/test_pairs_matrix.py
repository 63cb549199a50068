"""The pair form of the matrix product, CPU part.

The epilogue's rule (galah_amd/csrc/matrix_core.hpp, "the pair form") is
driven on the host by tests/cpp/test_matrix_pairs_core.cpp, a stand-alone
program built here plainly and with the address and undefined-behaviour
sanitizers: the tiled product through the core's index arithmetic with the
matrix instruction emulated, then the early exit, the candidate test, the pass
test and the emitted records against validate::merge_counts over all pairs.
The rest checks the surface: the header, the Python, Rust and C++ mirrors
carry the new names, the counts other tests pin have not moved, and the
argument checks that need no device."""
import ctypes
import os
import re
import subprocess

import pytest

import galah_amd as ga
from conftest import ROOT

SYMBOLS = ("gg_pairs_matrix_device", "gg_pairs_matrix", "gg_set_pairs_path", "gg_pairs_path", "gg_pairs_paths_taken",
           "gg_precluster_files_resident")
INVALID = 1  # GG_ERR_INVALID_ARG


def _build_core_test(exe, flags):
    src = os.path.join(ROOT, "tests", "cpp", "test_matrix_pairs_core.cpp")
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
    assert word == "ok" and int(cases) >= 3000 and int(pairs) >= 50000, r.stdout
    print(r.stdout)


def test_pair_core_rules_equal_the_merge():
    exe, r = _build_core_test("test_matrix_pairs_core", ["-O2"])
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def test_pair_core_rules_under_sanitizers():
    exe, r = _build_core_test("test_matrix_pairs_core_san",
                              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_every_mirror_carries_the_names():
    header = _read("include", "galahgpu.h")
    rust = _read("rust", "galah-gpu-sys", "src", "lib.rs")
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in ga.EXPORTED_SYMBOLS, name
        assert hasattr(ga.lib(), name), name
        assert re.search(r"pub fn %s\(" % name, rust), name
    assert "gg_pairs_matrix_summary" in header and "pub struct gg_pairs_matrix_summary" in rust
    for k, name in enumerate(("GG_PAIRS_PATH_DEFAULT", "GG_PAIRS_PATH_MATRIX", "GG_PAIRS_PATH_AUTO")):
        assert re.search(r"%s = %d\b" % (name, k), header), name
        assert re.search(r"pub const %s: c_int = %d;" % (name, k), rust), name
    assert ga.PAIRS_PATHS == ("default", "matrix", "auto")
    hpp = _read("include", "galah_finch.hpp")
    assert re.search(r"inline std::vector<gg_pair> pairs_matrix\(", hpp)
    assert "gg_precluster_files_resident" in hpp and "gg_set_pairs_path" in hpp and "int pairs_path" in hpp
    for method in ("pairs_matrix", "pairs_matrix_device", "set_pairs_path", "pairs_paths_taken",
                   "precluster_files_resident"):
        assert callable(getattr(ga.Context, method)), method


def test_cpp_mirror_option_compiles():
    """The program that drives the mirror's option on the GPU (test_pairs_matrix_gpu.py) compiles against the headers."""
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Werror", "-fsyntax-only",
                        "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "test_pairs_path_mirror.cpp")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_summary_struct_layout():
    S = ga._PairsMatrixSummary
    assert [f for f, _ in S._fields_] == ["n_entries", "n_columns", "column_entries", "n_pairs", "chunk_rounds",
                                          "index_reads", "path", "pair_passes"]
    assert ctypes.sizeof(S) == 56 and S.path.offset == 48 and S.pair_passes.offset == 52


def test_pinned_counts_have_not_moved():
    header = _read("include", "galahgpu.h")
    assert ga.abi_version() == 7 and re.search(r"#define GG_ABI_VERSION 7u", header)
    assert re.search(r"GG_KERNEL_COUNT = 14\b", header)
    assert re.search(r"GG_PATH_COUNT = 5\b", header)


def test_null_context_is_invalid():
    L = ga.lib()
    out, cnt = ctypes.c_void_p(), ctypes.c_uint64()
    summary = ga._PairsMatrixSummary()
    assert L.gg_pairs_matrix(None, None, None, 0, None, 0, ctypes.c_float(0.9), ctypes.byref(out), ctypes.byref(cnt),
                             ctypes.byref(summary)) == INVALID
    assert L.gg_pairs_matrix_device(None, None, None, 0, None, 0, ctypes.c_float(0.9), None, 0, None, None,
                                    None) == INVALID
    assert L.gg_set_pairs_path(None, 0) == INVALID
    assert L.gg_pairs_path(None) == -1
    assert L.gg_pairs_paths_taken(None, None) == INVALID
    pp, ap = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.gg_precluster_files_resident(None, None, 0, ctypes.c_float(0.9), None, ctypes.byref(pp), ctypes.byref(ap),
                                          ctypes.byref(cnt), None) == INVALID
    assert b"null context" in L.gg_thread_last_error()


def test_preclusterer_option_defaults_to_none():
    assert ga.FinchPreclusterer(0.9).pairs_path is None
    assert ga.FinchPreclusterer(0.9, 1000, 21, None).pairs_path is None
    assert ga.FinchPreclusterer(0.9, pairs_path="matrix").pairs_path == "matrix"
    with pytest.raises(ValueError):
        ga.FinchPreclusterer(0.9, pairs_path="dense")
