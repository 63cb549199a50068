"""The pair form of the matrix product on the device (DESIGN.md 4.12;
galah_amd/csrc/ani_matrix.hip): the passing pairs of a set of rows from
common = A A^T on the i8 matrix instruction, through the thresholded epilogue.

The reference is always the host merge: ga.pairs_border_host(sk, lens, 0,
min_ani, k) gives every passing pair sorted by (i, j); for a row list it is
applied to sk[rows] and the indices are mapped back.  Equality is of the sorted
(i, j, common, total) tuples, without tolerance.  The sizes are those at which
the kernel takes another path: m around the 16-row blocks and the 64-row
tiles, column counts around the 512-column chunks, no column at all, the
largest sketch size, a tile pair left before the epilogue, every branch of the
epilogue inside one tile, the output capacity, more rows than the dense matrix
takes, the tile pairs in more launches than one."""
import ctypes

import numpy as np
import pytest

import galah_amd as ga

pytestmark = pytest.mark.gpu

INVALID = 1  # GG_ERR_INVALID_ARG
F = lambda x: float(np.float32(x))  # noqa: E731  (a threshold as the f32 the library takes)


def tuples(p):
    return list(zip(p["i"].tolist(), p["j"].tolist(), p["common"].tolist(), p["total"].tolist()))


def reference(sk, lens, min_ani, rows=None, k=21):
    """The passing pairs by the host merge, sorted (i, j, common, total) tuples of row indices."""
    if rows is None:
        return tuples(ga.pairs_border_host(sk, lens, 0, min_ani, k))
    rows = np.asarray(rows, dtype=np.int64)
    if len(rows) < 2:
        return []
    p = ga.pairs_border_host(sk[rows], lens[rows], 0, min_ani, k)
    a, b = rows[p["i"]], rows[p["j"]]
    return sorted(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist(), p["common"].tolist(), p["total"].tolist()))


def check(ctx, sk, lens, min_ani, rows=None, what=""):
    ref = reference(sk, lens, min_ani, rows, ctx.k)
    pairs, summary = ctx.pairs_matrix(sk, lens, min_ani, rows)
    got = tuples(pairs)
    assert got == ref, "%s: %d pairs, the merge passes %d" % (what, len(got), len(ref))
    assert summary["n_pairs"] == len(ref) and summary["path"] == "matrix"
    return ref, summary


def rows_from_sets(sets, s):
    sk = np.zeros((len(sets), s), np.uint64)
    lens = np.zeros(len(sets), np.uint32)
    for g, h in enumerate(sets):
        v = np.unique(np.asarray(list(h), dtype=np.uint64))
        sk[g, :len(v)] = v
        lens[g] = len(v)
    return sk, lens


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


# ---- 1. the golden sketches -------------------------------------------------
@pytest.mark.parametrize("pct,count", ((95, None), (90, 161), (0.0, 351)))
def test_golden(gpu_ctx, golden, pct, count):
    thr = float(ga.parse_percentage(pct))
    sk, lens = golden["sketches"], golden["lens"]
    ref, summary = check(gpu_ctx, sk, lens, thr, what="golden %s" % pct)
    assert ref == tuples(gpu_ctx.pairs(sk, lens, thr))
    if count is not None:
        assert len(ref) == count
    assert summary["n_entries"] == int(lens.sum()) and summary["pair_passes"] == 1
    assert 0 < 2 * summary["n_columns"] <= summary["column_entries"] <= summary["n_entries"]
    assert summary["chunk_rounds"] == -(-summary["n_columns"] // 512)  # 27 rows: one tile pair
    assert summary["index_reads"] == summary["column_entries"] ** 2 // summary["n_columns"]


@pytest.fixture()
def routed_ctx():
    """A context of its own, so that the session's keeps the default path."""
    ctx = ga.Context(k=21, sketch_size=1000, seed=0)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("path", ga.PAIRS_PATHS)
def test_golden_files_resident(routed_ctx, golden, path):
    thr = float(ga.parse_percentage(90))
    exp_pairs, exp_ani = routed_ctx.precluster_files(golden["paths"], thr)
    assert routed_ctx.set_pairs_path(path) == "default" and routed_ctx.pairs_path == path
    pairs, ani, summary = routed_ctx.precluster_files_resident(golden["paths"], thr)
    assert pairs.tobytes() == exp_pairs.tobytes() and len(pairs) == 161
    assert ani.dtype == np.float32 and ani.tobytes() == exp_ani.tobytes()
    assert summary["n_pairs"] == 161 and summary["pair_passes"] == 1
    assert (summary["n_columns"] > 0) == (path != "default")


# ---- 2. the edge set ------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx64():
    ctx = ga.Context(k=21, sketch_size=64, seed=0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def edge_set():
    """200 rows of at most 64 hashes over shared pools; one hash in every
    non-empty row; rows 3 and 4 identical; rows g = 0 mod 10 empty, 1 mod 10 of
    length 1, 2 mod 10 short.  The hash every row holds is the largest of all:
    finch's merge ends with the shorter row, so a length-1 row whose hash
    were the others' smallest would have common = total = 1 with each."""
    rng = np.random.default_rng(20261020)
    everywhere = 2 ** 64 - 59
    pools = [np.arange(100 + 1000 * p, 100 + 1000 * p + 90, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             for p in range(4)]
    sets = []
    for g in range(200):
        kind = g % 10
        if kind == 0:
            sets.append(set())
        elif kind == 1:
            sets.append({everywhere})
        elif kind == 2:
            sets.append({everywhere} | set(rng.choice(pools[g % 4], 3, replace=False).tolist()))
        else:
            sets.append({everywhere} | set(rng.choice(pools[g % 4], 63, replace=False).tolist()))
    sets[4] = set(sets[3])
    sk, lens = rows_from_sets(sets, 64)
    full = np.array([g for g in range(200) if g % 10 > 2 and g not in (3, 4)])
    return sk, lens, rng.permutation(full)


def edge_rows(order, m):
    """m rows without repeats: the two identical rows first and last (the
    first and the last tile), two empty rows, a length-1 and a short row."""
    if m == 1:
        return [3]
    rows = [int(r) for r in order[:m]]
    rows[0], rows[-1] = 3, 4
    if m >= 16:
        rows[3], rows[m - 3], rows[5], rows[m // 2] = 0, 10, 1, 2
    assert len(set(rows)) == m
    return rows


@pytest.mark.parametrize("m", (1, 2, 16, 17, 63, 64, 65, 130))
def test_edge_set(ctx64, edge_set, m):
    sk, lens, order = edge_set
    rows = edge_rows(order, m)
    ref, _ = check(ctx64, sk, lens, 0.0, rows, "m=%d at 0.0" % m)
    assert len(ref) == m * (m - 1) // 2  # every pair, those with the empty rows as (i, j, 0, 0)
    if m >= 16:
        assert (0, 10, 0, 0) in ref and sum(1 for r in ref if r[3] == 0) == 2 * (m - 2) + 1
    ref, _ = check(ctx64, sk, lens, 0.5, rows, "m=%d at 0.5" % m)
    assert m < 16 or 0 < len(ref) < m * (m - 1) // 2
    ref, _ = check(ctx64, sk, lens, 1.0, rows, "m=%d at 1.0" % m)
    assert ref == ([(3, 4, 64, 64)] if m >= 2 else [])


# ---- 3. column-count edges ------------------------------------------------------
@pytest.mark.parametrize("columns", (0, 511, 512, 513, 1025))
def test_column_count_edges(columns):
    """Rows 0 and 1 share exactly `columns` hashes, every row has hashes of its own."""
    shared = set(range(10, 10 + 3 * columns, 3))
    sets = [shared | set(range(11, 11 + 3 * 9, 3)), shared | set(range(12, 12 + 3 * 7, 3)),
            set(range(10 ** 9, 10 ** 9 + 40))]
    with ga.Context(k=21, sketch_size=1040, seed=0) as ctx:
        sk, lens = rows_from_sets(sets, 1040)
        ref0, summary = check(ctx, sk, lens, 0.0, what="columns=%d at 0.0" % columns)
        ref9, _ = check(ctx, sk, lens, F(0.9), what="columns=%d at 0.9" % columns)
    assert summary["n_columns"] == columns and summary["column_entries"] == 2 * columns
    assert len(ref0) == 3 and ref0[0][:3] == (0, 1, columns)
    assert ref9 == ([ref0[0]] if columns >= 511 else [])


# ---- 4. the graded set ---------------------------------------------------------------
@pytest.fixture(scope="module")
def graded():
    """130 rows of 1,000 hashes: member g keeps all but 7 g hashes of one base
    and has 7 g of its own, so every threshold cuts through every tile."""
    rng = np.random.default_rng(412)
    v = np.unique(rng.integers(1, 2 ** 63, 1000 + 130 * 7 * 130 + 4096, dtype=np.uint64))
    v = rng.permutation(v)
    base, own = v[:1000], v[1000:]
    sk = np.zeros((130, 1000), np.uint64)
    at = 0
    for g in range(130):
        drop = rng.choice(1000, 7 * g, replace=False)
        keep = np.delete(base, drop)
        sk[g] = np.sort(np.concatenate([keep, own[at:at + 7 * g]]))
        at += 7 * g
    return sk, np.full(130, 1000, np.uint32)


@pytest.fixture(scope="module")
def graded_ref(graded):
    sk, lens = graded
    return {thr: reference(sk, lens, F(thr)) for thr in (0.9, 0.95, 0.98, 0.99)}


@pytest.mark.parametrize("thr", (0.9, 0.95, 0.98, 0.99))
def test_graded_set(gpu_ctx, graded, graded_ref, thr):
    sk, lens = graded
    ref = graded_ref[thr]
    print("graded set at %s: %d of 8385 pairs" % (thr, len(ref)))
    assert 0 < len(ref) < 8385
    pairs, summary = gpu_ctx.pairs_matrix(sk, lens, F(thr))
    assert tuples(pairs) == ref
    assert summary["n_pairs"] == len(ref) and summary["chunk_rounds"] == 6 * -(-summary["n_columns"] // 512)


# ---- 5. the output capacity -----------------------------------------------------------
def test_device_form_drops_past_the_capacity(gpu_ctx, graded, graded_ref):
    import torch
    sk, lens = graded
    ref = graded_ref[0.9]
    assert len(ref) > 200
    d_sk, d_lens = to_dev(sk), to_dev(lens)
    canary = np.full(4 * 150, 0xA5A5A5A5, np.uint32)
    d_out = to_dev(canary)
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        summary = gpu_ctx.pairs_matrix_device(d_sk, d_lens, 130, None, 130, F(0.9), d_out, 100, d_count,
                                              stream=stream.cuda_stream)
    stream.synchronize()
    assert int(d_count.item()) == len(ref) == summary["n_pairs"]
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[400:] == 0xA5A5A5A5).all()  # nothing past out_cap
    first = tuples(out[:400].view(ga.PAIR_DTYPE))
    assert len(set(first)) == 100 and set(first) <= set(ref)
    # a second call appends: the count grows by the number found again
    summary = gpu_ctx.pairs_matrix_device(d_sk, d_lens, 130, None, 130, F(0.9), d_out, 100, d_count)
    assert int(d_count.item()) == 2 * len(ref) and summary["n_pairs"] == len(ref)
    assert (d_out.cpu().numpy().view(np.uint32)[400:] == 0xA5A5A5A5).all()


def test_host_form_retries_at_the_exact_count(gpu_ctx, graded, graded_ref, monkeypatch):
    sk, lens = graded
    monkeypatch.setenv("GALAHGPU_TEST_PAIRS_CAP", "100")
    pairs, summary = gpu_ctx.pairs_matrix(sk, lens, F(0.9))
    assert tuples(pairs) == graded_ref[0.9] and summary["pair_passes"] == 2
    monkeypatch.delenv("GALAHGPU_TEST_PAIRS_CAP")
    pairs, summary = gpu_ctx.pairs_matrix(sk, lens, F(0.9))
    assert tuples(pairs) == graded_ref[0.9] and summary["pair_passes"] == 1


# ---- 6. wide sketches: many chunks into one accumulator ----------------------------------
def test_many_chunks_at_the_largest_sketch_size():
    s = 12000
    sets = []
    for grp in range(2):
        full = np.arange(1, s + 1, dtype=np.uint64) * np.uint64(977) + np.uint64(grp * 3)
        for replaced in (0, 300, 3000):  # hashes of the base replaced by the row's own
            own = np.arange(1, replaced + 1, dtype=np.uint64) * np.uint64(977) + np.uint64(grp * 3 + 1 + (replaced > 300))
            sets.append(np.concatenate([full[replaced:], own]))
    sk, lens = rows_from_sets(sets, s)
    assert lens.tolist() == [s] * 6
    with ga.Context(k=21, sketch_size=s, seed=0) as ctx:
        ref0, summary = check(ctx, sk, lens, 0.0, what="s=12000 at 0.0")
        ref9, _ = check(ctx, sk, lens, F(0.99), what="s=12000 at 0.99")
    # a group's columns are the 11,700 hashes two or three of its rows keep; the two groups' interleave
    assert summary["n_columns"] == 2 * 11700 and summary["chunk_rounds"] == 46
    assert len(ref0) == 15 and sum(1 for r in ref0 if r[2] == 0) == 9
    assert ref9 == [(0, 1, 11700, 12300), (3, 4, 11700, 12300)]


# ---- 7. the limits, and the host form's checks ---------------------------------------------
def test_limits_are_checked_before_any_row_is_read(gpu_ctx, ctx64):
    import torch
    tiny = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    slots = -(-2 ** 31 // 1000)  # the first m with m s >= 2^31 at s = 1,000
    tile_pairs = 65535 * 64 + 1  # the first m of 65,536 tiles: 65,536 * 65,537 / 2 >= 2^31 tile pairs (m s < 2^31 at s = 64)
    assert (slots - 1) * 1000 < 2 ** 31 <= slots * 1000 and 65535 * 65536 // 2 < 2 ** 31 and tile_pairs * 64 < 2 ** 31
    for ctx, m in ((gpu_ctx, slots), (ctx64, tile_pairs)):
        with pytest.raises(ga.GalahGpuError) as e:
            ctx.pairs_matrix_device(tiny, tiny, m, None, m, F(0.9), tiny, 0, d_count)
        assert e.value.status == INVALID
        assert int(d_count.item()) == 0
    L = ga.lib()
    sk, lens = np.zeros(8, np.uint64), np.zeros(8, np.uint32)
    out, cnt = ctypes.c_void_p(), ctypes.c_uint64()
    st = L.gg_pairs_matrix(gpu_ctx._c, sk.ctypes.data_as(ctypes.c_void_p), lens.ctypes.data_as(ctypes.c_void_p), 2200000,
                           None, 2200000, ctypes.c_float(0.9), ctypes.byref(out), ctypes.byref(cnt), None)
    assert st == INVALID and not out.value and cnt.value == 0


def test_host_form_checks_its_rows(gpu_ctx, golden):
    sk, lens = golden["sketches"], golden["lens"]
    for rows in ([0, 5, 5], [0, 27], [3, 2 ** 32 - 1]):
        with pytest.raises(ga.GalahGpuError) as e:
            gpu_ctx.pairs_matrix(sk, lens, F(0.9), rows)
        assert e.value.status == INVALID
    with pytest.raises(ga.GalahGpuError) as e:
        gpu_ctx.pairs_matrix(sk, lens, float("nan"))
    assert e.value.status == INVALID
    long = lens.copy()
    long[7] = 1001
    with pytest.raises(ga.GalahGpuError) as e:
        gpu_ctx.pairs_matrix(sk, long, F(0.9))
    assert e.value.status == INVALID
    assert ga.lib().gg_set_pairs_path(gpu_ctx._c, 3) == INVALID and gpu_ctx.pairs_path == "default"
    with pytest.raises(ValueError):
        gpu_ctx.set_pairs_path("dense")
    # a row list in any order, and fewer than two rows
    rows = [26, 0, 13, 7, 1]
    check(gpu_ctx, sk, lens, F(0.9), rows, "listed rows")
    assert len(gpu_ctx.pairs_matrix(sk, lens, F(0.9), [4])[0]) == 0
    assert len(gpu_ctx.pairs_matrix(sk, lens, F(0.9), [])[0]) == 0


def test_device_form_rows_out_of_range_and_listed_twice(gpu_ctx, golden):
    """d_rows is not checked: an index >= n is an empty row, a row listed twice
    gets its pairs once per position and none with itself."""
    import torch
    sk, lens = golden["sketches"], golden["lens"]
    thr = float(ga.parse_percentage(90))
    rows = np.array([0, 1, 2, 1, 99, 3, 4, 5, 6, 7, 8], np.uint32)
    d_out = torch.zeros(4 * 200, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    gpu_ctx.pairs_matrix_device(to_dev(sk), to_dev(lens), 27, to_dev(rows), len(rows), thr, d_out, 200, d_count)
    n = int(d_count.item())
    got = sorted(tuples(d_out.cpu().numpy().view(np.uint32)[:4 * n].view(ga.PAIR_DTYPE)))
    valid = [0, 1, 2, 3, 4, 5, 6, 7, 8]
    ref = reference(sk, lens, thr, valid)
    assert got == sorted(ref + [r for r in ref if 1 in r[:2]])


# ---- 8. routing -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed_rows(graded):
    """The graded set and 70 rows that share nothing with anything."""
    sk, lens = graded
    rng = np.random.default_rng(99)
    own = np.sort(rng.permutation(70 * 1000).astype(np.uint64).reshape(70, 1000) * np.uint64(7919) + np.uint64(1), axis=1)
    assert not np.isin(own, sk).any()
    return np.concatenate([sk, own]), np.concatenate([lens, np.full(70, 1000, np.uint32)])


ROUTES = (("matrix", None, "matrix"), ("auto", "0", "auto"), ("auto", "1e30", "default"))


def run_rows(ctx, sk, lens):
    import torch
    n = len(lens)
    d_rep = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    summary, _, _, _ = ctx.cluster_rows_device(to_dev(sk), to_dev(lens), n, F(0.9), F(0.95), d_rep)
    return d_rep.cpu().numpy().view(np.uint32).tolist(), summary


def same_clustering(got, exp):
    assert got[0] == exp[0]
    for f in ("n_pairs", "n_preclusters", "largest_precluster"):
        assert got[1][f] == exp[1][f], f


@pytest.mark.parametrize("which", ("mixed", "golden"))
def test_routing_of_cluster_rows_device(routed_ctx, mixed_rows, golden, which, monkeypatch):
    sk, lens = mixed_rows if which == "mixed" else (golden["sketches"], golden["lens"])
    before = routed_ctx.pairs_paths_taken()
    exp = run_rows(routed_ctx, sk, lens)
    assert exp[1]["n_pairs"] > 0 and 1 < exp[1]["n_preclusters"] < len(lens)
    taken = routed_ctx.pairs_paths_taken()
    assert taken == dict(before, default=before["default"] + 1)
    for path, ratio, slot in ROUTES:
        if ratio is None:
            monkeypatch.delenv("GALAHGPU_PAIRS_MATRIX_RATIO", raising=False)
        else:
            monkeypatch.setenv("GALAHGPU_PAIRS_MATRIX_RATIO", ratio)
        routed_ctx.set_pairs_path(path)
        same_clustering(run_rows(routed_ctx, sk, lens), exp)
        now = routed_ctx.pairs_paths_taken()
        assert now == dict(taken, **{slot: taken[slot] + 1}), (path, ratio)
        taken = now


def test_routing_of_cluster_files_resident(routed_ctx, golden, monkeypatch):
    thr, T = F(0.9), F(0.95)
    exp = routed_ctx.cluster_files_resident(golden["paths"], thr, T)
    exp = (exp[0].tolist(), exp[1])
    taken = routed_ctx.pairs_paths_taken()
    assert taken == {"default": 1, "matrix": 0, "auto": 0}
    for path, ratio, slot in ROUTES:
        if ratio is None:
            monkeypatch.delenv("GALAHGPU_PAIRS_MATRIX_RATIO", raising=False)
        else:
            monkeypatch.setenv("GALAHGPU_PAIRS_MATRIX_RATIO", ratio)
        routed_ctx.set_pairs_path(path)
        rep_of, summary = routed_ctx.cluster_files_resident(golden["paths"], thr, T)
        same_clustering((rep_of.tolist(), summary), exp)
        now = routed_ctx.pairs_paths_taken()
        assert now == dict(taken, **{slot: taken[slot] + 1}), (path, ratio)
        taken = now


def test_preclusterer_option(golden):
    exp = ga.cluster(golden["paths"], ga.FinchPreclusterer(0.9), ga.FinchClusterer(0.95))
    cached = ga._context(21, 1000)
    taken = cached.pairs_paths_taken()
    got = ga.cluster(golden["paths"], ga.FinchPreclusterer(0.9, pairs_path="matrix"), ga.FinchClusterer(0.95))
    assert got == exp
    assert cached.pairs_path == "default"  # put back: the cached context is shared
    one = cached.device_count == 1  # (several devices: the option is ignored)
    assert cached.pairs_paths_taken()["matrix"] == taken["matrix"] + (1 if one else 0)
    d_exp = ga.FinchPreclusterer(0.9).distances(golden["paths"])
    d_got = ga.FinchPreclusterer(0.9, pairs_path="auto").distances(golden["paths"])
    assert d_got == d_exp and len(d_exp) == 161
    assert cached.pairs_path == "default"


# ---- 9. more rows than the dense matrix takes ---------------------------------------------------
def test_more_rows_than_the_dense_cap(ctx64):
    """33,000 rows of 8 hashes that share nothing, but for two planted pairs
    across distant tiles: the positions part beyond 32,768 rows, and 133,386
    tile pairs of which all but a few are left before the epilogue."""
    m = 33000
    sk = np.zeros((m, 64), np.uint64)
    sk[:, :8] = (np.arange(m, dtype=np.uint64)[:, None] * np.uint64(16) + np.arange(1, 9, dtype=np.uint64)[None, :])
    lens = np.full(m, 8, np.uint32)
    sk[32990, :8] = sk[5, :8]            # identical
    sk[32800, :7] = sk[100, 1:8]         # 7 of 8 shared; its own last hash stays the largest
    planted = [5, 100, 32800, 32990]
    rest = np.delete(sk[:, :8], planted, axis=0)
    assert len(np.unique(rest)) == rest.size and not np.isin(sk[planted, :8], rest).any()
    ref = reference(sk, lens, F(0.9), planted)
    assert [r[:2] for r in ref] == [(5, 32990), (100, 32800)]
    pairs, summary = ctx64.pairs_matrix(sk, lens, F(0.9))
    assert tuples(pairs) == ref
    assert summary["n_columns"] == 15 and summary["column_entries"] == 30 and summary["n_entries"] == 8 * m
    assert summary["chunk_rounds"] == 516 * 517 // 2


# ---- 10. the tile pairs in several launches ------------------------------------------------------
@pytest.mark.parametrize("slice_", (1, 4, 5, 6, 7))
def test_tile_pairs_in_slices(gpu_ctx, graded, graded_ref, monkeypatch, slice_):
    """One launch takes fewer than 2^24 workgroups, so a call goes in slices of
    2^23 tile pairs, each with the number of its first tile pair.  The knob
    lowers the slice: the graded set's 6 tile pairs in 6, 2 (4 + 2, 5 + 1) and
    1 launches, every pair found once."""
    sk, lens = graded
    monkeypatch.setenv("GALAHGPU_TEST_PAIRS_SLICE", str(slice_))
    pairs, summary = gpu_ctx.pairs_matrix(sk, lens, F(0.95))
    assert tuples(pairs) == graded_ref[0.95] and summary["n_pairs"] == len(pairs)


def test_sliced_launches_on_the_routed_path(routed_ctx, mixed_rows, monkeypatch):
    sk, lens = mixed_rows  # 200 rows: 4 tiles, 10 tile pairs
    exp = run_rows(routed_ctx, sk, lens)
    routed_ctx.set_pairs_path("matrix")
    monkeypatch.setenv("GALAHGPU_TEST_PAIRS_SLICE", "3")
    same_clustering(run_rows(routed_ctx, sk, lens), exp)
    assert routed_ctx.pairs_paths_taken()["matrix"] == 1


# ---- 11. the option through the C++ mirror ---------------------------------------------------------
def test_cpp_mirror_pairs_path(golden):
    import os
    import subprocess
    from conftest import GOLD_DATA, ROOT
    build = os.path.join(ROOT, "tests", "cpp", "build")
    os.makedirs(build, exist_ok=True)
    exe = os.path.join(build, "test_pairs_path_mirror")
    lib = os.path.join(ROOT, "galah_amd", "lib")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O1", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_pairs_path_mirror.cpp"),
                           "-L", lib, "-lgalahgpu", "-Wl,-rpath," + lib])
    r = subprocess.run([exe, GOLD_DATA] + golden["names"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip() == "ok"
