"""The dense ANI matrices of many groups in one call, the
parts that need no device:

  - the grouped rules of galah_amd/csrc/matrix_core.hpp driven on the host by
    tests/cpp/test_matrix_groups_core.cpp (the grouped column rule against a
    std::map over (group, hash), the workgroup -> (group, ti, tj) search, the
    cells' offsets and the limits, the tiled product group by group against
    finch's merge), built plainly and, where the compiler has the runtimes,
    with -fsanitize=address,undefined, run stand-alone;
  - gg_ani_matrix_groups_host on the 27 golden sketches grouped by the
    preclusters of tests/golden/pairs_k21_s1000.tsv at 0.9: every block equals
    the same rows' block of ani_matrix_host;
  - every invalid argument is rejected.  The limit on the tile pairs cannot
    be broken alone: a group of m >= 2 positions has at most m^2 / 4 tile
    pairs, so 2^31 of them need 2^33 cells; it is checked on the rule itself
    in the C++ program, as is the limit on the sketch slots at a sketch size
    of 1 (2^31 positions would need 8 GiB of offsets), which is checked here
    through the host form at the largest sketch size;
  - the header, the Python mirror and the Rust file carry the five entry
    points; the ABI version and the kernel count are unchanged.

The kernels are checked in test_ani_matrix_groups_gpu.py (GPU).  CPU only."""
import os
import re
import subprocess

import numpy as np
import pytest

import galah_amd as ga
from conftest import ROOT

SYMBOLS = ("gg_ani_matrix_group_cells", "gg_ani_matrix_groups_host", "gg_ani_matrix_groups",
           "gg_ani_matrix_groups_device", "gg_precluster_matrices_files")
INVALID = 1  # GG_ERR_INVALID_ARG


def _build_core_test(exe, flags):
    src = os.path.join(ROOT, "tests", "cpp", "test_matrix_groups_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, exe)
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags +
                       ["-o", out, src], capture_output=True, text=True)
    return out, r


def _run_core_test(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word, cases, cells, workgroups = r.stdout.strip().splitlines()[-1].split()
    assert word == "ok" and int(cases) >= 2000 and int(cells) >= 300000 and int(workgroups) >= 2000, r.stdout
    print(r.stdout)


def test_grouped_core_rules_equal_the_merge():
    exe, r = _build_core_test("test_matrix_groups_core", ["-O2"])
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def test_grouped_core_rules_under_sanitizers():
    exe, r = _build_core_test("test_matrix_groups_core_san",
                              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def golden_groups(golden):
    keep = [(i, j, c, t) for i, j, c, t, a in golden["pairs"] if a >= ga.parse_percentage(0.9)]
    return ga.preclusters(len(golden["lens"]), np.array(keep, dtype=ga.PAIR_DTYPE))


def test_host_groups_on_the_golden_preclusters(golden):
    sk, lens = golden["sketches"], golden["lens"]
    groups = golden_groups(golden)
    assert sum(len(g) for g in groups) == 27 and len(groups[0]) >= 2 and len(groups[-1]) == 1
    common, total, ani, cells = ga.ani_matrix_groups_host(sk, lens, groups)
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.uint32)
    assert cells.dtype == np.uint64 and cells.tolist() == np.concatenate([[0], np.cumsum([len(g) ** 2 for g in groups])]).tolist()
    assert cells.tolist() == ga.ani_matrix_group_cells(offsets).tolist()
    assert len(common) == len(total) == len(ani) == int(cells[-1]) and ani.dtype == np.float32
    ac, at, aa = ga.ani_matrix_host(sk, lens)
    for g, rows in enumerate(groups):
        ix = np.ix_(rows, rows)
        assert np.array_equal(ga.ani_matrix_block(common, offsets, cells, g), ac[ix]), g
        assert np.array_equal(ga.ani_matrix_block(total, offsets, cells, g), at[ix]), g
        assert ga.ani_matrix_block(ani, offsets, cells, g).tobytes() == np.ascontiguousarray(aa[ix]).tobytes(), g
    # the CSR form, a row twice in a group and in two groups, an empty group
    members = np.array([5, 0, 5, 13, 0], np.uint32)
    offsets = np.array([0, 3, 3, 5], np.uint32)
    common, total, ani, cells = ga.ani_matrix_groups_host(sk, lens, members, offsets)
    assert cells.tolist() == [0, 9, 9, 13]
    for g, rows in enumerate(([5, 0, 5], [], [13, 0])):
        ix = np.ix_(rows, rows)
        assert np.array_equal(ga.ani_matrix_block(common, offsets, cells, g), ac[ix])
        assert ga.ani_matrix_block(ani, offsets, cells, g).tobytes() == np.ascontiguousarray(aa[ix]).tobytes()


def _host_call(sk, lens, n, s, k, members, offsets, outs=(True, True, True), cells=64):
    bufs = [np.zeros(cells, t) for t in (np.uint32, np.uint32, np.float32)]
    ptrs = [ga._ptr(b) if on else None for b, on in zip(bufs, outs)]
    return ga.lib().gg_ani_matrix_groups_host(ga._ptr(sk), ga._ptr(lens), n, s, k, ga._ptr(members), ga._ptr(offsets),
                                              len(offsets) - 1, *ptrs)


def _cells_call(offsets):
    offsets = np.ascontiguousarray(offsets, dtype=np.uint32)
    return ga.lib().gg_ani_matrix_group_cells(ga._ptr(offsets), len(offsets) - 1, ga._ptr(np.zeros(len(offsets), np.uint64)))


def test_groups_reject_invalid_arguments():
    sk = np.arange(1, 4 * 8 + 1, dtype=np.uint64).reshape(4, 8)
    lens = np.array([8, 3, 0, 8], np.uint32)
    members = np.array([0, 1, 2, 3, 1], np.uint32)
    offsets = np.array([0, 2, 2, 5], np.uint32)
    assert _host_call(sk, lens, 4, 8, 21, members, offsets) == ga.GG_OK
    assert _host_call(sk, lens, 4, 8, 21, np.array([0, 1, 2, 4, 1], np.uint32), offsets) == INVALID  # an index >= n
    assert _host_call(sk, lens, 4, 8, 21, members, np.array([0, 3, 2, 5], np.uint32)) == INVALID  # descending offsets
    assert _host_call(sk, lens, 4, 8, 21, members, np.array([1, 2, 2, 5], np.uint32)) == INVALID  # not from 0
    assert _host_call(sk, lens, 4, 8, 21, members, offsets, outs=(False, False, False)) == INVALID  # no output
    assert _host_call(sk, np.array([8, 9, 0, 8], np.uint32), 4, 8, 21, members, offsets) == INVALID  # lens > sketch_size
    for outs in ((True, False, False), (False, True, False), (False, False, True)):
        assert _host_call(sk, lens, 4, 8, 21, members, offsets, outs=outs) == ga.GG_OK
    assert _host_call(sk, lens, 4, 8, 21, members, np.array([0, 0, 0], np.uint32), outs=(False,) * 3) == ga.GG_OK  # nothing to do
    # the limits.  Cells: one group of 65,536 positions is 2^32 of them; 65,535 is within
    assert _cells_call([0, 65535]) == ga.GG_OK
    assert _cells_call([0, 65536]) == INVALID
    assert _cells_call([0, 46341, 92682]) == INVALID  # two groups of 2^31 + 4,633 cells each
    assert _cells_call([0, 5, 3]) == INVALID and _cells_call([2, 5]) == INVALID
    with pytest.raises(ga.GalahGpuError):
        ga.ani_matrix_group_cells([0, 65536])
    # sketch slots: 180,000 positions in groups of 2 at sketch size 12,000 are 2.16e9 >= 2^31 slots
    # (720,000 cells and 90,000 tile pairs: the other two limits hold); rejected before any row is read
    big = np.arange(0, 180001, 2, dtype=np.uint32)
    wide = np.zeros((2, 12000), np.uint64)
    assert _cells_call(big) == ga.GG_OK
    assert _host_call(wide, np.zeros(2, np.uint32), 2, 12000, 21, np.zeros(180000, np.uint32), big, cells=1) == INVALID
    small = np.arange(0, 178001, 2, dtype=np.uint32)  # 178,000 * 12,000 < 2^31
    assert _host_call(wide, np.zeros(2, np.uint32), 2, 12000, 21, np.zeros(178000, np.uint32), small, cells=4 * 89000) == ga.GG_OK
    with pytest.raises(ga.GalahGpuError):
        ga.ani_matrix_groups_host(sk, lens, [[0, 7]])


def test_header_mirror_and_binding_carry_the_groups():
    header = open(os.path.join(ROOT, "include", "galahgpu.h")).read()
    rust = open(os.path.join(ROOT, "rust", "galah-gpu-sys", "src", "lib.rs")).read()
    for name in SYMBOLS:
        assert re.search(r"gg_status\s+%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert name in ga.EXPORTED_SYMBOLS
        assert hasattr(ga.lib(), name)
    assert ga.abi_version() == 7
    assert re.search(r"#define\s+GG_ABI_VERSION\s+7u?\b", header)
    assert re.search(r"GG_KERNEL_COUNT\s*=\s*14\b", header)
    for name in ("ani_matrix_groups", "ani_matrix_groups_device", "precluster_matrices_files"):
        assert callable(getattr(ga.Context, name))
    for name in ("ani_matrix_groups_host", "ani_matrix_group_cells", "ani_matrix_block", "precluster_ani_matrices"):
        assert callable(getattr(ga, name))
    assert "precluster_ani_matrices(" in open(os.path.join(ROOT, "include", "galah_finch.hpp")).read()
