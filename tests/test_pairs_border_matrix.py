"""The border form of the matrix product, CPU part.

The rule (galah_amd/csrc/matrix_core.hpp, "the border form") is driven on the
host by tests/cpp/test_matrix_border_core.cpp, a stand-alone program built here
plainly and with the address and undefined-behaviour sanitizers: the tiled
product through the core's index arithmetic with the matrix instruction
emulated, over the border's positions, tile-pair numbering, column rule and
visited rule, against validate::merge_counts over all border pairs.  The rest
checks the surface: the header, the Python and Rust mirrors carry the new
names, the pinned counts have not moved, the argument checks that need no
device, and that FinchPreclusterer.update sets and restores the pairs path
around its context call."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import galah_amd as ga
from conftest import ROOT

SYMBOLS = ("gg_pairs_border_matrix_device", "gg_pairs_border_matrix")
INVALID = 1  # GG_ERR_INVALID_ARG


def _build_core_test(exe, flags):
    src = os.path.join(ROOT, "tests", "cpp", "test_matrix_border_core.cpp")
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


def test_border_core_rules_equal_the_merge():
    exe, r = _build_core_test("test_matrix_border_core", ["-O2"])
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def test_border_core_rules_under_sanitizers():
    exe, r = _build_core_test("test_matrix_border_core_san",
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
    for method in ("pairs_border_matrix", "pairs_border_matrix_device"):
        assert callable(getattr(ga.Context, method)), method
    # gg_set_pairs_path's comment lists the border calls it now routes
    comment = header[header.index("/* What produces the pairs inside"):header.index("gg_status gg_set_pairs_path")]
    for name in ("gg_pairs_border,", "gg_pairs_border_device", "gg_update_files"):
        assert name in comment, name


def test_pinned_counts_have_not_moved():
    header = _read("include", "galahgpu.h")
    assert ga.abi_version() == 7 and re.search(r"#define GG_ABI_VERSION 7u", header)
    assert re.search(r"GG_KERNEL_COUNT = 14\b", header)
    assert re.search(r"GG_PATH_COUNT = 5\b", header)
    assert ctypes.sizeof(ga._PairsMatrixSummary) == 56


def test_null_context_is_invalid():
    L = ga.lib()
    out, cnt = ctypes.c_void_p(), ctypes.c_uint64()
    summary = ga._PairsMatrixSummary()
    assert L.gg_pairs_border_matrix(None, None, None, 0, 0, ctypes.c_float(0.9), ctypes.byref(out), ctypes.byref(cnt),
                                    ctypes.byref(summary)) == INVALID
    assert b"null context" in L.gg_thread_last_error()
    assert L.gg_pairs_border_matrix_device(None, None, None, 0, 0, ctypes.c_float(0.9), None, 0, None, None,
                                           None) == INVALID
    assert b"null context" in L.gg_thread_last_error()


class _FakeContext:
    """What FinchPreclusterer.update asks of the cached context, recorded."""

    def __init__(self, device_count=1, fail=False):
        self.device_count = device_count
        self.pairs_path = "default"
        self.calls = []
        self.fail = fail

    def set_pairs_path(self, path):
        assert path in ga.PAIRS_PATHS
        before, self.pairs_path = self.pairs_path, path
        self.calls.append(("set", path))
        return before

    def update_files(self, old_sketches, old_lens, new_paths, min_ani, cache_dir=None):
        self.calls.append(("update_files", self.pairs_path, len(old_lens), list(new_paths)))
        if self.fail:
            raise ga.GalahGpuError(2, "no device")
        n = len(new_paths)
        return (np.zeros((n, 1000), np.uint64), np.zeros(n, np.uint32), np.zeros(0, ga.PAIR_DTYPE),
                np.zeros(0, np.float32))


@pytest.mark.parametrize("path", (None, "default", "matrix", "auto"))
def test_update_sets_and_restores_the_path(monkeypatch, path):
    fake = _FakeContext()
    monkeypatch.setattr(ga, "_context", lambda k, s: fake)
    pre = ga.FinchPreclusterer(0.9, pairs_path=path)
    state = pre.distances_state(["a.fna", "b.fna"])
    assert state.paths == ["a.fna", "b.fna"] and len(state.pairs) == 0
    if path is None:  # exactly the call made so far
        assert fake.calls == [("update_files", "default", 0, ["a.fna", "b.fna"])]
    else:
        assert fake.calls == [("set", path), ("update_files", path, 0, ["a.fna", "b.fna"]), ("set", "default")]
    assert fake.pairs_path == "default"
    fake.calls.clear()
    state = pre.update(state, ["c.fna"])
    assert state.paths == ["a.fna", "b.fna", "c.fna"]
    assert [c for c in fake.calls if c[0] == "update_files"] == [("update_files", path or "default", 2, ["c.fna"])]
    assert fake.pairs_path == "default"


def test_update_restores_the_path_after_a_failure(monkeypatch):
    fake = _FakeContext(fail=True)
    fake.pairs_path = "auto"  # whatever was set before is put back, not "default"
    monkeypatch.setattr(ga, "_context", lambda k, s: fake)
    with pytest.raises(RuntimeError, match="Failed to sketch genomes with finch"):
        ga.FinchPreclusterer(0.9, pairs_path="matrix").distances_state(["a.fna"])
    assert fake.calls == [("set", "matrix"), ("update_files", "matrix", 0, ["a.fna"]), ("set", "auto")]
    assert fake.pairs_path == "auto"


def test_update_ignores_the_option_on_several_devices(monkeypatch):
    fake = _FakeContext(device_count=2)
    monkeypatch.setattr(ga, "_context", lambda k, s: fake)
    ga.FinchPreclusterer(0.9, pairs_path="matrix").distances_state(["a.fna"])
    assert fake.calls == [("update_files", "default", 0, ["a.fna"])]
