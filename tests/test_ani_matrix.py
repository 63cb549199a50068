"""The dense ANI matrix, the parts that need no device:

  - the rules of galah_amd/csrc/matrix_core.hpp driven on the host by
    tests/cpp/test_matrix_core.cpp (the tiled incidence product through the
    core's own index arithmetic against finch's merge, the column rule
    against a std::map), built plainly and, where the compiler has the
    runtimes, with -fsanitize=address,undefined, run stand-alone;
  - the header, the Python mirror and the Rust file carry the four entry
    points and the struct; the ABI version and the kernel count are unchanged;
  - gg_ani_matrix_host on the 27 golden sketches: equal to ani_pairs_host over
    all 729 cells and to tests/golden/pairs_k21_s1000.tsv over its 351 pairs,
    (len, len, 1.0) on the diagonal;
  - every invalid argument of the host-input forms is rejected;
  - write_ani_matrix round-trips names and values.

The kernels are checked in test_ani_matrix_gpu.py (GPU).  CPU only."""
import ctypes
import io
import os
import re
import subprocess

import numpy as np
import pytest

import galah_amd as ga
from conftest import ROOT

SYMBOLS = ("gg_ani_matrix_host", "gg_ani_matrix", "gg_ani_matrix_device", "gg_ani_matrix_files")
FIELDS = ("n_entries", "n_columns", "column_entries", "ani_rechecked")


def _build_core_test(exe, flags):
    src = os.path.join(ROOT, "tests", "cpp", "test_matrix_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, exe)
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags +
                       ["-o", out, src], capture_output=True, text=True)
    return out, r


def _run_core_test(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word, cases, cells = r.stdout.strip().splitlines()[-1].split()
    assert word == "ok" and int(cases) >= 3000 and int(cells) >= 300000, r.stdout
    print(r.stdout)


def test_core_rules_tiled_product_equals_the_merge():
    exe, r = _build_core_test("test_matrix_core", ["-O2"])
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def test_core_rules_under_sanitizers():
    exe, r = _build_core_test("test_matrix_core_san",
                              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def test_header_mirror_and_binding_carry_the_matrix():
    header = open(os.path.join(ROOT, "include", "galahgpu.h")).read()
    rust = open(os.path.join(ROOT, "rust", "galah-gpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert re.search(r"gg_status\s+%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert name in ga.EXPORTED_SYMBOLS
        assert hasattr(ga.lib(), name)
    body = re.search(r"typedef struct gg_matrix_summary \{(.*?)\} gg_matrix_summary;", header, flags=re.S).group(1)
    assert tuple(re.findall(r"uint64_t (\w+);", body)) == FIELDS
    rbody = re.search(r"pub struct gg_matrix_summary \{(.*?)\}", rust, flags=re.S).group(1)
    assert tuple(re.findall(r"pub (\w+): u64,", rbody)) == FIELDS
    assert tuple(f for f, _ in ga._MatrixSummary._fields_) == FIELDS
    assert ctypes.sizeof(ga._MatrixSummary) == 32
    assert set(ga._MatrixSummary().as_dict()) == set(FIELDS)
    assert ga.abi_version() == 7
    assert re.search(r"#define\s+GG_ABI_VERSION\s+7u?\b", header)
    assert re.search(r"GG_KERNEL_COUNT\s*=\s*14\b", header)
    for name in ("ani_matrix", "ani_matrix_device", "ani_matrix_files"):
        assert callable(getattr(ga.Context, name))
    assert "ani_matrix(" in open(os.path.join(ROOT, "include", "galah_finch.hpp")).read()


def test_host_matrix_on_the_golden_sketches(golden):
    sk, lens = golden["sketches"], golden["lens"]
    n = len(lens)
    assert n == 27
    common, total, ani = ga.ani_matrix_host(sk, lens)
    assert common.shape == total.shape == ani.shape == (n, n) and ani.dtype == np.float32
    pairs, pani = ga.ani_pairs_host(sk, lens, [(a, b) for a in range(n) for b in range(n)])
    assert np.array_equal(common.reshape(-1), pairs["common"])
    assert np.array_equal(total.reshape(-1), pairs["total"])
    assert ani.tobytes() == pani.tobytes()
    assert len(golden["pairs"]) == 351
    for i, j, c, t, a in golden["pairs"]:
        for x, y in ((i, j), (j, i)):
            assert (int(common[x, y]), int(total[x, y])) == (c, t)
            assert ani[x, y] == a
    for g in range(n):
        assert (int(common[g, g]), int(total[g, g])) == (int(lens[g]), int(lens[g])) and ani[g, g] == np.float32(1.0)


def test_host_matrix_listed_rows_any_order_and_twice(golden):
    sk, lens = golden["sketches"], golden["lens"]
    rows = [5, 0, 26, 5, 13]
    common, total, ani = ga.ani_matrix_host(sk, lens, rows=rows)
    pairs, pani = ga.ani_pairs_host(sk, lens, [(a, b) for a in rows for b in rows])
    assert np.array_equal(common.reshape(-1), pairs["common"]) and np.array_equal(total.reshape(-1), pairs["total"])
    assert ani.tobytes() == pani.tobytes()
    assert int(common[0, 3]) == int(total[0, 3]) == int(lens[5])  # the same row by a repeated index
    # an empty row: 0 and 0 everywhere, itself included
    lens0 = lens.copy()
    lens0[13] = 0
    common, total, ani = ga.ani_matrix_host(sk, lens0, rows=rows)
    assert not common[4].any() and not total[4].any() and not ani[:, 4].any()


def _host_call(sk, lens, n, s, k, rows, m, outs=(True, True, True)):
    bufs = [np.zeros(max(m, 1) ** 2 if m <= 64 else 1, t) for t in (np.uint32, np.uint32, np.float32)]
    ptrs = [ga._ptr(b) if on else None for b, on in zip(bufs, outs)]
    return ga.lib().gg_ani_matrix_host(ga._ptr(sk), ga._ptr(lens), n, s, k, None if rows is None else ga._ptr(rows), m,
                                       *ptrs)


def test_host_matrix_rejects_invalid_arguments():
    INVALID = 1  # GG_ERR_INVALID_ARG
    sk = np.arange(1, 4 * 8 + 1, dtype=np.uint64).reshape(4, 8)
    lens = np.array([8, 3, 0, 8], np.uint32)
    rows = np.array([0, 1, 2, 3], np.uint32)
    assert _host_call(sk, lens, 4, 8, 21, rows, 4) == ga.GG_OK
    assert _host_call(sk, lens, 4, 8, 21, np.array([0, 4], np.uint32), 2) == INVALID  # an index >= n
    assert _host_call(sk, np.array([8, 9, 0, 8], np.uint32), 4, 8, 21, rows, 4) == INVALID  # lens[g] > sketch_size
    assert _host_call(sk, lens, 4, 8, 21, np.zeros(32769, np.uint32), 32769) == INVALID  # m > 32768
    assert _host_call(sk, lens, 4, 8, 21, None, 5) == INVALID  # rows == NULL with m > n
    assert _host_call(sk, lens, 4, 8, 21, rows, 4, outs=(False, False, False)) == INVALID  # no output
    assert _host_call(sk, lens, 4, 8, 21, None, 4) == ga.GG_OK
    assert _host_call(sk, lens, 4, 8, 21, rows, 0) == ga.GG_OK  # m == 0 writes nothing
    for outs in ((True, False, False), (False, True, False), (False, False, True)):
        assert _host_call(sk, lens, 4, 8, 21, rows, 4, outs=outs) == ga.GG_OK
    with pytest.raises(ga.GalahGpuError):
        ga.ani_matrix_host(sk, lens, rows=[0, 7])


def test_write_ani_matrix_round_trips(tmp_path):
    names = ["a.fna", "dir/b c.fna", "z"]
    ani = np.array([[1.0, 0.9808188, 0.0], [0.9808188, 1.0, 0.98405427], [0.0, 0.98405427, 1.0]], np.float32)
    text = io.StringIO()
    ga.write_ani_matrix(text, names, ani)
    path = tmp_path / "m.tsv"
    ga.write_ani_matrix(str(path), names, ani)
    assert path.read_text() == text.getvalue()
    lines = text.getvalue().split("\n")
    assert lines[-1] == "" and len(lines) == 5
    assert lines[0].split("\t") == [""] + names
    assert lines[2].split("\t") == ["dir/b c.fna", "0.9808188", "1", "0.98405427"]
    back = np.array([[np.float32(v) for v in l.split("\t")[1:]] for l in lines[1:4]], np.float32)
    assert [l.split("\t")[0] for l in lines[1:4]] == names and back.tobytes() == ani.tobytes()
    with pytest.raises(ValueError):
        ga.write_ani_matrix(io.StringIO(), names[:2], ani)
