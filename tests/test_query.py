"""The query of a resident collection, CPU part.

The table and key rules (galah_amd/csrc/query_core.hpp) are driven on the host
by tests/cpp/test_query_core.cpp, a stand-alone program built here plainly and
with the address and undefined-behaviour sanitizers.  The host forms
(gg_query_host, gg_query_best_host) are held to the CPU oracle, to
pairs_border_host and to a plain Python loop on every scenario of
tests/query_cases.py.  The rest checks the surface: the three sides carry the
names, the argument checks that need no device, and the knob's documentation."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import galah_amd as ga
import query_cases as qc
from conftest import ROOT
from test_pair_edges import assert_pairs, quads

f32 = np.float32
SYMBOLS = ("gg_query_host", "gg_query_rows", "gg_query_rows_device", "gg_query_best_host", "gg_query_best_device",
           "gg_collection_query_rows", "gg_collection_query_files", "gg_collection_classify_rows",
           "gg_collection_classify_files")
INVALID = 1  # GG_ERR_INVALID_ARG
NONE = 0xFFFFFFFF


def _build_core_test(exe, flags):
    src = os.path.join(ROOT, "tests", "cpp", "test_query_core.cpp")
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    out = os.path.join(build, exe)
    r = subprocess.run([os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wno-unknown-pragmas"] + flags +
                       ["-o", out, src], capture_output=True, text=True)
    return out, r


def _run_core_test(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    word, cases, keys = r.stdout.strip().splitlines()[-1].split()
    assert word == "ok" and int(cases) >= 20000 and int(keys) >= 1000000, r.stdout
    assert len(re.findall(r"longest chain \d+ slots", r.stdout)) == 5, r.stdout
    print(r.stdout)


def test_query_core_rules():
    exe, r = _build_core_test("test_query_core", ["-O2"])
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


def test_query_core_rules_under_sanitizers():
    exe, r = _build_core_test("test_query_core_san",
                              ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    if r.returncode != 0 and re.search(r"cannot find -l(asan|ubsan)|libasan|libubsan", r.stderr):
        pytest.skip("the compiler has no sanitizer runtimes")
    assert r.returncode == 0, r.stderr
    _run_core_test(exe)


THR = f32(0.9)


@pytest.mark.parametrize("name", sorted(qc.CASES))
def test_query_host_equals_the_oracle_and_the_border(name):
    """gg_query_host == oracle.pairs(rows ++ queries) filtered to i < n <= j
    == pairs_border_host(rows ++ queries, n_old = n) filtered to i < n, in
    content and order."""
    sk, lens, q_sk, q_lens = qc.CASES[name][0]()
    n = len(lens)
    exp = qc.expected(name, qc.bits(THR))
    got = ga.query_host(sk, lens, q_sk, q_lens, THR)
    assert_pairs(got, exp, name)
    border = ga.pairs_border_host(np.concatenate([sk, q_sk]), np.concatenate([lens, q_lens]), n, THR)
    assert_pairs(got, quads(border[border["i"] < n]), name + " against the border")
    assert name in ("empty_queries",) or len(exp) > 0


@pytest.mark.parametrize("thr", [0.0, -1.0])
def test_query_host_at_zero_returns_every_cell(thr):
    sk, lens, q_sk, q_lens = qc.table()
    n, nq = len(lens), len(q_lens)
    got = quads(ga.query_host(sk, lens, q_sk, q_lens, f32(thr)))
    assert len(got) == n * nq and (got[:, :2] == [(i, n + q) for i in range(n) for q in range(nq)]).all()
    assert (got[:, 2] == 0).any() and ((got[:, 2] == 0) & (got[:, 3] == 0)).any()
    assert_pairs(ga.query_host(sk, lens, q_sk, q_lens, f32(thr)), qc.expected("table", qc.bits(thr)), "table at %r" % thr)


def best_loop(n, nq, q, ani, rank):
    """The rule as a plain loop: per query the candidate of the largest f32
    ANI, ties to the smallest rank."""
    best = [(NONE, n + x, 0, 0) for x in range(nq)]
    best_ani = [f32(0)] * nq
    held = [None] * nq
    for row, a in zip(q.tolist(), ani):
        r = row[0] if rank is None else int(rank[row[0]])
        if r == NONE:
            continue
        x = row[1] - n
        if held[x] is None or a > held[x][0] or (a == held[x][0] and r < held[x][1]):
            held[x], best[x], best_ani[x] = (a, r), tuple(row), a
    return np.array(best, dtype=np.uint32).reshape(nq, 4), np.array(best_ani, dtype=np.float32)


@pytest.mark.parametrize("name", sorted(qc.CASES))
def test_query_best_host_equals_a_plain_loop(name):
    sk, lens, q_sk, q_lens = qc.CASES[name][0]()
    n, nq = len(lens), len(q_lens)
    pairs = ga.query_host(sk, lens, q_sk, q_lens, THR)
    q = quads(pairs)
    ani = np.array([ga.ani_f32(int(c), int(t)) for c, t in q[:, 2:]], dtype=np.float32)
    rng = np.random.default_rng(n)
    perm = rng.permutation(n).astype(np.uint32)
    some = perm.copy()
    some[rng.random(n) < 0.4] = NONE
    shuffled = rng.permutation(len(q))
    for what, rank in (("every row", None), ("a permutation", perm), ("some rows", some),
                       ("no row", np.full(n, NONE, np.uint32))):
        exp, exp_ani = best_loop(n, nq, q, ani, rank)
        for order in (np.arange(len(q)), shuffled):  # no order of the list is assumed
            best, best_ani = ga.query_best_host(n, nq, pairs[order], ani[order], rank)
            assert (quads(best) == exp).all() and (best_ani.view(np.uint32) == exp_ani.view(np.uint32)).all(), (name, what)
    if name == "table":  # the duplicated query and its equal row: ANI 1.0, found by each copy
        best, best_ani = ga.query_best_host(n, nq, pairs, ani, None)
        assert [int(best[x]["i"]) for x in (3, 5, 7)] == [3, 3, 3] and (best_ani[[3, 5, 7]] == 1.0).all()
        assert int(best[4]["i"]) == NONE  # the empty query


def test_query_best_host_ties_and_checks():
    pairs = np.array([(0, 3, 5, 9), (1, 3, 5, 9), (2, 3, 4, 9)], dtype=ga.PAIR_DTYPE)
    ani = np.array([0.95, 0.95, 0.9], dtype=np.float32)
    for rank, winner in (([0, 1, 2], 0), ([1, 0, 2], 1), ([NONE, 7, 0], 1), ([NONE, NONE, 0], 2)):
        best, best_ani = ga.query_best_host(3, 1, pairs, ani, np.array(rank, np.uint32))
        assert int(best[0]["i"]) == winner and best_ani[0] == ani[winner], rank
    zero = np.array([0.0, -0.0, 0.0], dtype=np.float32)  # equal as values: the rank decides
    assert int(ga.query_best_host(3, 1, pairs, zero, np.array([2, 0, 1], np.uint32))[0][0]["i"]) == 1
    for bad_pairs, bad_ani, rank in (
            (np.array([(3, 3, 1, 1)], dtype=ga.PAIR_DTYPE), [0.5], None),       # i >= n
            (np.array([(0, 2, 1, 1)], dtype=ga.PAIR_DTYPE), [0.5], None),       # j < n
            (np.array([(0, 4, 1, 1)], dtype=ga.PAIR_DTYPE), [0.5], None),       # j - n >= nq
            (pairs[:1], [np.nan], None),                                        # NaN ANI
            (pairs, ani, np.array([4, 4, 1], np.uint32))):                      # two candidates of one rank
        with pytest.raises(ga.GalahGpuError) as e:
            ga.query_best_host(3, 1, bad_pairs, np.array(bad_ani, np.float32), rank)
        assert e.value.status == INVALID
    ga.query_best_host(3, 1, pairs, ani, np.array([NONE, NONE, 1], np.uint32))  # (the mark may repeat)


def test_query_host_checks():
    sk, lens, q_sk, q_lens = qc.one_hash()
    with pytest.raises(ga.GalahGpuError) as e:
        ga.query_host(sk, lens, q_sk, q_lens, f32(np.nan))
    assert e.value.status == INVALID
    long = q_lens.copy()
    long[0] = 2
    for a, b in ((lens, long), (np.array([2, 1, 1, 0, 1], np.uint32), q_lens)):
        with pytest.raises(ga.GalahGpuError) as e:
            ga.query_host(sk, a, q_sk, b, THR)
        assert e.value.status == INVALID and "sketch longer" in str(e.value)
    assert len(ga.query_host(sk[:0], lens[:0], q_sk, q_lens, THR)) == 0
    assert len(ga.query_host(sk, lens, q_sk[:0], q_lens[:0], THR)) == 0


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_the_three_sides_carry_the_query():
    header, rust = _read("include", "galahgpu.h"), _read("rust", "galah-gpu-sys", "src", "lib.rs")
    for name in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert re.search(r"pub fn %s\(" % name, rust), name
        assert name in ga.EXPORTED_SYMBOLS and hasattr(ga._L, name), name
    assert "#define GG_ABI_VERSION 7u" in header and ga.abi_version() == 7
    assert re.search(r"GG_KERNEL_COUNT = 14\b", header) and re.search(r"GG_KERNEL_COUNT: \w+ = 14;", rust)
    assert "galah::query_rows" in _read("DESIGN.md") and "inline std::vector<gg_pair> query_rows(" in _read(
        "include", "galah_finch.hpp")
    for method in ("query_rows", "query_rows_device", "query_best_device", "collection_query_rows",
                   "collection_query_files", "collection_classify_rows", "collection_classify_files"):
        assert callable(getattr(ga.Context, method)), method
    assert callable(ga.Collection.query) and callable(ga.Collection.classify)


def test_null_arguments_are_refused_without_a_device():
    L = ga._L
    out, out2 = ctypes.c_void_p(), ctypes.c_void_p()
    n = ctypes.c_uint64()
    refs = (ctypes.byref(out), ctypes.byref(out2), ctypes.byref(n))
    assert L.gg_query_rows(None, None, None, 0, None, None, 0, 0.9, *refs) == INVALID
    assert b"null context" in L.gg_thread_last_error()
    assert L.gg_query_rows_device(None, None, None, 0, None, None, 0, 0.9, None, 0, None, None) == INVALID
    assert L.gg_query_best_device(None, 0, 0, None, None, 0, None, None, None, None) == INVALID
    assert L.gg_collection_query_rows(None, None, None, 0, 0.9, *refs) == INVALID
    assert b"null collection" in L.gg_thread_last_error()
    assert L.gg_collection_query_files(None, None, 0, None, 0.9, None, None, *refs) == INVALID
    assert L.gg_collection_classify_rows(None, None, None, 0, None, None, None) == INVALID
    assert L.gg_collection_classify_files(None, None, 0, None, None, None, None) == INVALID
    assert L.gg_query_host(None, None, 1, None, None, 1, 64, 21, 0.9, ctypes.byref(out), ctypes.byref(n)) == INVALID
    assert b"null" in L.gg_thread_last_error()
    assert L.gg_query_host(None, None, 0, None, None, 0, 64, 21, 0.9, None, ctypes.byref(n)) == INVALID
    assert L.gg_query_host(None, None, 0, None, None, 0, 64, 0, 0.9, ctypes.byref(out), ctypes.byref(n)) == INVALID
    assert L.gg_query_best_host(1, 1, None, None, 1, None, None, None) == INVALID
    # n + nq == 2^31 is refused before any array is read
    assert L.gg_query_host(None, None, 0, ctypes.byref(n), ctypes.byref(n), 2**31, 64, 21, 0.9, ctypes.byref(out),
                           ctypes.byref(n)) == INVALID
    assert b"2^31" in L.gg_thread_last_error()
    assert not out.value and not out2.value


def test_the_batch_knob_is_documented():
    assert "GALAHGPU_TEST_QUERY_BATCH" in _read("galah_amd", "csrc", "query.cpp")
    design = _read("DESIGN.md")
    seven = design[design.index("\n## 7. "):]
    assert "GALAHGPU_TEST_QUERY_BATCH" in seven
    assert "\n### 4.17 " in design
