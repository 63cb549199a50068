"""The border form of the matrix product on the device (DESIGN.md 4.13;
galah_amd/csrc/ani_matrix.hip): the pairs that rows n_old .. n-1 add to a
finished run, from common = A A^T on the i8 matrix instruction with the new
rows at the first positions, the border tile pairs, the border column rule and
the thresholded epilogue.

The reference is always the host merge, ga.pairs_border_host (finch's literal
merge over every border pair); equality is of the sorted (i, j, common, total)
tuples, without tolerance.  The sizes are the smallest at which each piece can
go wrong: n and n_new around the 64-row tiles (the mixed new / old tile row),
the seam between the triangle and the rectangle of the numbering inside and
between launches, old-only columns beyond a chunk, tile pairs that end without
a chunk or jump first, the output capacity, many chunks, more rows than the
dense matrix takes, the limits and the degenerate sizes; then the routing of
the border calls by the context's pairs path."""
import functools

import numpy as np
import pytest

import border_cases as bc
import cluster_ref
import galah_amd as ga

pytestmark = pytest.mark.gpu

INVALID = 1  # GG_ERR_INVALID_ARG
F = lambda x: float(np.float32(x))  # noqa: E731  (a threshold as the f32 the library takes)
f32 = np.float32


def tuples(p):
    return list(zip(p["i"].tolist(), p["j"].tolist(), p["common"].tolist(), p["total"].tolist()))


def border_ref(sk, lens, n_old, min_ani, k=21):
    return tuples(ga.pairs_border_host(sk, lens, n_old, min_ani, k))


def border_count(n, n_old):
    n_new = n - n_old
    return n_new * n_old + n_new * (n_new - 1) // 2


def check(ctx, sk, lens, n_old, min_ani, what=""):
    ref = border_ref(sk, lens, n_old, min_ani, ctx.k)
    pairs, summary = ctx.pairs_border_matrix(sk, lens, n_old, min_ani)
    got = tuples(pairs)
    assert got == ref, "%s: %d pairs, the merge passes %d" % (what, len(got), len(ref))
    assert summary["n_pairs"] == len(ref) and summary["path"] == "matrix"
    return ref, summary


def to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


def device_border(ctx, call, d_sk, d_lens, n, n_old, min_ani, cap=1 << 16):
    """The device form `call` into a fresh buffer -> sorted tuples."""
    import torch
    d_out = torch.zeros(4 * cap, dtype=torch.int32, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    call(d_sk, d_lens, n, n_old, min_ani, d_out, cap, d_count)
    torch.cuda.synchronize()
    cnt = int(d_count.item())
    assert cnt <= cap
    return sorted(tuples(d_out.cpu().numpy().view(np.uint32)[:4 * cnt].view(ga.PAIR_DTYPE)))


@pytest.fixture(scope="module")
def ctx64():
    ctx = ga.Context(k=21, sketch_size=64, seed=0)
    yield ctx
    ctx.close()


@pytest.fixture()
def routed_ctx():
    """A context of its own, so that the session's keeps the default path."""
    ctx = ga.Context(k=21, sketch_size=1000, seed=0)
    yield ctx
    ctx.close()


# ---- 1. the golden sketches -------------------------------------------------
@pytest.mark.parametrize("pct", (0.0, 90, 95))
def test_golden(gpu_ctx, golden, pct):
    thr = float(ga.parse_percentage(pct))
    sk, lens = golden["sketches"], golden["lens"]
    everything = tuples(gpu_ctx.pairs(sk, lens, thr))
    for n_old in (0, 1, 13, 26, 27):
        ref, summary = check(gpu_ctx, sk, lens, n_old, thr, "golden %s n_old=%d" % (pct, n_old))
        assert ref == [r for r in everything if r[1] >= n_old]
        if pct == 0.0:
            assert len(ref) == border_count(27, n_old)
        if n_old < 27:
            assert summary["n_entries"] == int(lens.sum()) and summary["pair_passes"] == 1
            assert summary["chunk_rounds"] == -(-summary["n_columns"] // 512)  # 27 rows: one tile pair
            assert (summary["n_columns"], summary["column_entries"]) == bc.dict_border_columns(sk, lens, n_old)
        else:
            assert summary["n_entries"] == summary["n_columns"] == 0  # nothing is run


# ---- 2. the edge set ------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_set():
    """193 rows of at most 64 hashes over four shared pools; rows g = 0 mod 10
    empty, 1 mod 10 of length 1, 2 mod 10 short, the rest 40 to 64 long; the
    hash 0 in every third non-empty row, 2^64 - 1 in every row of length 2 or
    more; rows 3 and 4 identical, rows 191 and 192 identical."""
    rng = np.random.default_rng(20261020)
    top = 2 ** 64 - 1
    pools = [np.arange(100 + 1000 * p, 100 + 1000 * p + 90, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             for p in range(4)]
    sets = []
    for g in range(193):
        kind = g % 10
        if kind == 0:
            h = set()
        elif kind == 1:
            h = {top - 7}
        elif kind == 2:
            h = {top} | set(rng.choice(pools[g % 4], 3, replace=False).tolist())
        else:
            h = {top} | set(rng.choice(pools[g % 4], int(rng.integers(39, 63)), replace=False).tolist())
        if h and g % 3 == 0:
            h.add(0)
        sets.append(h)
    sets[4] = set(sets[3])
    sets[192] = set(sets[191])
    sk = np.zeros((193, 64), np.uint64)
    lens = np.zeros(193, np.uint32)
    for g, h in enumerate(sets):
        v = np.array(sorted(h), dtype=np.uint64)
        sk[g, :len(v)] = v
        lens[g] = len(v)
    assert (sk[lens > 1, 0] == 0).any() and (sk[np.arange(193), np.maximum(lens, 1) - 1] == top).any()
    return sk, lens


@pytest.mark.parametrize("n", (2, 64, 65, 130, 193))
def test_edge_set(ctx64, n):
    sk, lens = edge_set()
    sk, lens = sk[:n], lens[:n]
    for n_new in sorted({v for v in (1, 63, 64, 65, n - 1, n) if 1 <= v <= n}):
        n_old = n - n_new
        ref, _ = check(ctx64, sk, lens, n_old, 0.0, "n=%d n_new=%d at 0.0" % (n, n_new))
        assert len(ref) == border_count(n, n_old)  # every border pair, those with an empty row as (i, j, 0, 0)
        ref5, _ = check(ctx64, sk, lens, n_old, 0.5, "n=%d n_new=%d at 0.5" % (n, n_new))
        assert len(ref5) < len(ref) or n < 64
        ref1, _ = check(ctx64, sk, lens, n_old, 1.0, "n=%d n_new=%d at 1.0" % (n, n_new))
        assert all(r[2] == r[3] for r in ref1)
        if n == 193:
            assert (191, 192, int(lens[191]), int(lens[191])) in ref1


# ---- 3. the graded set: the identity -------------------------------------------------
@pytest.fixture(scope="module")
def graded():
    """130 rows of 1,000 hashes: member g keeps all but 7 g hashes of one base
    and has 7 g of its own, so every threshold cuts through every tile (the
    recipe of test_pairs_matrix_gpu.py)."""
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


@pytest.mark.parametrize("thr", (0.9, 0.95, 0.98))
def test_graded_identity(gpu_ctx, graded, thr):
    sk, lens = graded
    everything = tuples(gpu_ctx.pairs_matrix(sk, lens, F(thr))[0])
    assert 0 < len(everything) < 8385
    assert gpu_ctx.pairs_path == "default"
    for n_old in (0, 64, 100, 129, 130):
        border, summary = gpu_ctx.pairs_border_matrix(sk, lens, n_old, F(thr))
        border = tuples(border)
        old = tuples(gpu_ctx.pairs_matrix(sk[:n_old], lens[:n_old], F(thr))[0]) if n_old else []
        assert not set(old) & set(border)
        assert sorted(old + border) == everything, n_old
        assert border == tuples(gpu_ctx.pairs_border(sk, lens, n_old, F(thr))), n_old  # the index border (DEFAULT)
        assert border == border_ref(sk, lens, n_old, F(thr)), n_old
        if n_old == 100:  # 30 new rows: one new tile against three
            assert summary["chunk_rounds"] == 3 * -(-summary["n_columns"] // 512)


# ---- 4. the border column rule ----------------------------------------------------------
def test_column_rule(ctx64):
    sk, lens, n_old = bc.scenario_columns()
    for thr in (0.0, 0.5, F(0.9)):
        ref, summary = check(ctx64, sk, lens, n_old, thr, "columns at %s" % thr)
        assert (summary["n_columns"], summary["column_entries"]) == bc.dict_border_columns(sk, lens, n_old) == (35, 83)
        assert summary["n_entries"] == int(lens.sum()) and summary["chunk_rounds"] == 3
        assert summary["index_reads"] == bc.index_reads_bound(35, 83, 45) <= bc.exact_index_reads(sk, lens, n_old)
    assert (126, 127) in [r[:2] for r in ref]  # at 0.9: the two new rows that share hashes with each other only
    # the full matrix call over the same rows keeps the old-only columns: more than a chunk of them
    assert gpu_summary_columns(ctx64, sk, lens) > 512 + 35 - 1


def gpu_summary_columns(ctx, sk, lens):
    return ctx.pairs_matrix(sk, lens, F(0.9))[1]["n_columns"]


# ---- 5. jumps and the early exit -----------------------------------------------------------
@pytest.mark.parametrize("slice_", (None, 1))
def test_jumps_and_early_exit(ctx64, monkeypatch, slice_):
    """border_cases.scenario_jumps (pinned by test_border_schedule.py): a tile
    pair that ends without running a chunk because the old tile's pieces are
    empty, one that jumps over the first chunk and then runs, and the mixed
    new / old tile row -- in one launch, and one tile pair per launch."""
    sk, lens, n_old = bc.scenario_jumps()
    if slice_ is not None:
        monkeypatch.setenv("GALAHGPU_TEST_PAIRS_SLICE", str(slice_))
    for thr in (0.0, F(0.9), F(0.98)):
        ref, summary = check(ctx64, sk, lens, n_old, thr, "jumps at %s" % thr)
        assert (summary["n_columns"], summary["column_entries"]) == bc.dict_border_columns(sk, lens, n_old)
        assert summary["chunk_rounds"] == 5 * 2
    assert len(border_ref(sk, lens, n_old, 0.0)) == border_count(300, 280)
    assert 0 < len(border_ref(sk, lens, n_old, F(0.9))) < border_count(300, 280)


# ---- 6. slices across the seam ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pooled_rows():
    """200 rows at s = 64, row g drawing 60 hashes of pool g % 4 (90 hashes):
    rows of one pool pass 0.9 with one another, rows of different pools share
    nothing."""
    rng = np.random.default_rng(200)
    sk = np.zeros((200, 64), np.uint64)
    for g in range(200):
        pool = np.uint64(1 + ((g % 4) << 20)) + np.arange(90, dtype=np.uint64)
        sk[g, :60] = np.sort(rng.choice(pool, 60, replace=False))
    return sk, np.full(200, 60, np.uint32)


@pytest.mark.parametrize("slice_", (1, 2, 3, 4, 7))
def test_slices_across_the_seam(ctx64, monkeypatch, slice_):
    """200 rows, 100 of them new: Tn = 2, T = 4, 3 tile pairs of the triangle
    and 4 of the rectangle, in launches of 1, 2, 3, 4 and 7 -- a slice ends at
    the seam (3), begins on it (4 = 3 + 1) or straddles it (2, 4, 7)."""
    sk, lens = pooled_rows()
    monkeypatch.setenv("GALAHGPU_TEST_PAIRS_SLICE", str(slice_))
    ref, summary = check(ctx64, sk, lens, 100, F(0.9), "slice %d" % slice_)
    assert 1000 < len(ref) < border_count(200, 100)
    assert summary["chunk_rounds"] == 7 * -(-summary["n_columns"] // 512)


# ---- 7. the output capacity ----------------------------------------------------------------------
def test_device_form_drops_past_the_capacity(gpu_ctx, graded):
    import torch
    sk, lens = graded
    ref = border_ref(sk, lens, 100, F(0.9))
    assert len(ref) > 200
    d_sk, d_lens = to_dev(sk), to_dev(lens)
    d_out = to_dev(np.full(4 * 150, 0xA5A5A5A5, np.uint32))
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        summary = gpu_ctx.pairs_border_matrix_device(d_sk, d_lens, 130, 100, F(0.9), d_out, 100, d_count,
                                                     stream=stream.cuda_stream)
    stream.synchronize()
    assert int(d_count.item()) == len(ref) == summary["n_pairs"]
    out = d_out.cpu().numpy().view(np.uint32)
    assert (out[400:] == 0xA5A5A5A5).all()  # nothing past out_cap
    first = tuples(out[:400].view(ga.PAIR_DTYPE))
    assert len(set(first)) == 100 and set(first) <= set(ref)
    # a second call appends: the count grows by the number found again; without a summary as well
    summary = gpu_ctx.pairs_border_matrix_device(d_sk, d_lens, 130, 100, F(0.9), d_out, 100, d_count)
    assert int(d_count.item()) == 2 * len(ref) and summary["n_pairs"] == len(ref)
    assert gpu_ctx.pairs_border_matrix_device(d_sk, d_lens, 130, 100, F(0.9), d_out, 100, d_count,
                                              want_summary=False) is None
    assert int(d_count.item()) == 3 * len(ref)
    assert (d_out.cpu().numpy().view(np.uint32)[400:] == 0xA5A5A5A5).all()


def test_host_form_retries_at_the_exact_count(gpu_ctx, graded, monkeypatch):
    sk, lens = graded
    ref = border_ref(sk, lens, 100, F(0.9))
    monkeypatch.setenv("GALAHGPU_TEST_PAIRS_CAP", "100")
    pairs, summary = gpu_ctx.pairs_border_matrix(sk, lens, 100, F(0.9))
    assert tuples(pairs) == ref and summary["pair_passes"] == 2
    monkeypatch.delenv("GALAHGPU_TEST_PAIRS_CAP")
    pairs, summary = gpu_ctx.pairs_border_matrix(sk, lens, 100, F(0.9))
    assert tuples(pairs) == ref and summary["pair_passes"] == 1


# ---- 8. wide sketches: many chunks into one accumulator ----------------------------------
def test_many_chunks_at_the_largest_sketch_size():
    s = 12000
    rows = []
    for g in range(16):  # rows of one base, g * 150 hashes replaced by the row's own
        full = np.arange(1, s + 1, dtype=np.uint64) * np.uint64(977)
        own = np.arange(1, 150 * g + 1, dtype=np.uint64) * np.uint64(977) + np.uint64(1 + g)
        rows.append(np.sort(np.concatenate([full[150 * g:], own])))
    sk = np.stack(rows)
    lens = np.full(16, s, np.uint32)
    with ga.Context(k=21, sketch_size=s, seed=0) as ctx:
        ref0, summary = check(ctx, sk, lens, 13, 0.0, "s=12000 at 0.0")
        ref9, _ = check(ctx, sk, lens, 13, F(0.991), "s=12000 at 0.991")
    assert len(ref0) == 3 * 13 + 3 and 0 < len(ref9) < len(ref0)
    # the columns are the base hashes the first new row keeps: 12,000 - 13 x 150, in 20 chunks of one tile pair
    assert summary["n_columns"] == 10050 and summary["chunk_rounds"] == 20


# ---- 9. more rows than the dense matrix takes ---------------------------------------------------
def test_more_rows_than_the_dense_cap():
    """33,000 rows of 8 hashes at s = 16 that share nothing, 100 of them new,
    but for planted pairs: beyond kMaxRows the positions part takes its offsets
    from a scan, and of the 2 x 516 - 1 border tile pairs nearly all are left
    before the epilogue."""
    n, n_old = 33000, 32900
    sk = np.zeros((n, 16), np.uint64)
    sk[:, :8] = (np.arange(n, dtype=np.uint64)[:, None] * np.uint64(16) + np.arange(1, 9, dtype=np.uint64)[None, :])
    lens = np.full(n, 8, np.uint32)
    sk[32990, :8] = sk[5, :8]            # new = old, identical
    sk[32905, :7] = sk[20000, 1:8]       # new with 7 of an old row's 8; its own last hash stays the largest
    sk[32999, :8] = sk[32901, :8]        # new = new
    sk[100, :8] = sk[7, :8]              # old = old: no border pair, and no column
    with ga.Context(k=21, sketch_size=16, seed=0) as ctx:
        pairs, summary = ctx.pairs_border_matrix(sk, lens, n_old, F(0.9))
    assert tuples(pairs) == border_ref(sk, lens, n_old, F(0.9))
    assert [(int(p["i"]), int(p["j"])) for p in pairs] == [(5, 32990), (20000, 32905), (32901, 32999)]
    assert summary["n_columns"] == 8 + 7 + 8 and summary["column_entries"] == 46 and summary["n_entries"] == 8 * n
    assert summary["chunk_rounds"] == 2 * 3 // 2 + 2 * (516 - 2)


# ---- 10. the limits and the degenerate sizes ---------------------------------------------------------
def test_limits_are_checked_before_any_row_is_read(gpu_ctx, routed_ctx):
    import torch
    tiny = torch.zeros(8, dtype=torch.int64, device="cuda")
    d_count = torch.zeros(1, dtype=torch.int64, device="cuda")
    slots = -(-2 ** 31 // 1000)  # the first n with n s >= 2^31 at s = 1,000
    assert (slots - 1) * 1000 < 2 ** 31 <= slots * 1000
    for n, n_old in ((10, 11), (slots, slots - 1)):
        with pytest.raises(ga.GalahGpuError) as e:
            gpu_ctx.pairs_border_matrix_device(tiny, tiny, n, n_old, F(0.9), tiny, 0, d_count)
        assert e.value.status == INVALID
    # the host form: the limits come before the arrays are looked at
    L = ga.lib()
    import ctypes
    sk, lens = np.zeros(8, np.uint64), np.zeros(8, np.uint32)
    out, cnt = ctypes.c_void_p(), ctypes.c_uint64()
    for n, n_old in ((10, 11), (slots, slots - 1)):
        st = L.gg_pairs_border_matrix(gpu_ctx._c, sk.ctypes.data_as(ctypes.c_void_p),
                                      lens.ctypes.data_as(ctypes.c_void_p), n, n_old, ctypes.c_float(0.9),
                                      ctypes.byref(out), ctypes.byref(cnt), None)
        assert st == INVALID and not out.value and cnt.value == 0
    with pytest.raises(ga.GalahGpuError) as e:
        gpu_ctx.pairs_border_matrix(np.zeros((4, 1000), np.uint64), np.zeros(4, np.uint32), 2, float("nan"))
    assert e.value.status == INVALID
    # the routed device call under MATRIX refuses the same sizes, before any row is read
    routed_ctx.set_pairs_path("matrix")
    before = routed_ctx.pairs_paths_taken()
    for n, n_old in ((10, 11), (slots, slots - 1)):
        with pytest.raises(ga.GalahGpuError) as e:
            routed_ctx.pairs_border_device(tiny, tiny, n, n_old, F(0.9), tiny, 0, d_count)
        assert e.value.status == INVALID
    assert routed_ctx.pairs_paths_taken() == before and int(d_count.item()) == 0


def test_auto_falls_back_at_the_slot_limit(routed_ctx):
    """The first n with n s >= 2^31 at s = 1,000, one new row: AUTO cannot take
    the product and runs the index border's call as DEFAULT does (there, with
    the index out of its own range, the gate kernel's border form).  All rows
    are empty but the new row and one old row, which are identical."""
    import torch
    n = -(-2 ** 31 // 1000)
    d_sk = torch.zeros(n * 1000, dtype=torch.int64, device="cuda")
    d_lens = torch.zeros(n, dtype=torch.int32, device="cuda")
    row = torch.arange(1, 11, dtype=torch.int64, device="cuda") * 977
    for g in (5, n - 1):
        d_sk[g * 1000:g * 1000 + 10] = row
        d_lens[g] = 10
    results = {}
    for path in ("default", "auto"):
        routed_ctx.set_pairs_path(path)
        before = routed_ctx.pairs_paths_taken()
        results[path] = device_border(routed_ctx, routed_ctx.pairs_border_device, d_sk, d_lens, n, n - 1, F(0.9), cap=16)
        assert routed_ctx.pairs_paths_taken() == dict(before, default=before["default"] + 1), path
    assert results["auto"] == results["default"] == [(5, n - 1, 10, 10)]


def test_degenerate_sizes(gpu_ctx, golden):
    import torch
    sk, lens = golden["sketches"], golden["lens"]
    thr = float(ga.parse_percentage(90))
    # n_old == n: nothing, and the count is left as it is
    pairs, summary = gpu_ctx.pairs_border_matrix(sk, lens, 27, thr)
    assert len(pairs) == 0 and summary["n_pairs"] == 0 and summary["pair_passes"] == 0
    d_count = torch.full((1,), 7, dtype=torch.int64, device="cuda")
    d_out = to_dev(np.full(16, 0xA5A5A5A5, np.uint32))
    summary = gpu_ctx.pairs_border_matrix_device(to_dev(sk), to_dev(lens), 27, 27, thr, d_out, 4, d_count)
    assert int(d_count.item()) == 7 and summary["n_pairs"] == 0
    assert (d_out.cpu().numpy().view(np.uint32) == 0xA5A5A5A5).all()
    # fewer than two rows
    assert len(gpu_ctx.pairs_border_matrix(sk[:1], lens[:1], 0, thr)[0]) == 0
    assert len(gpu_ctx.pairs_border_matrix(sk[:0], lens[:0], 0, thr)[0]) == 0
    # n_old == 0: the pair form over all rows, columns and all
    pairs, summary = gpu_ctx.pairs_border_matrix(sk, lens, 0, thr)
    full, full_summary = gpu_ctx.pairs_matrix(sk, lens, thr)
    assert pairs.tobytes() == full.tobytes() and len(pairs) == 161
    for f in ("n_entries", "n_columns", "column_entries", "chunk_rounds", "n_pairs"):
        assert summary[f] == full_summary[f], f


# ---- 11. routing ------------------------------------------------------------------------------------
ROUTES = (("default", None, "default"), ("matrix", None, "matrix"), ("auto", "0", "auto"), ("auto", "1e30", "default"))
SPLIT_OLD = 20


def set_route(ctx, monkeypatch, path, ratio):
    if ratio is None:
        monkeypatch.delenv("GALAHGPU_PAIRS_MATRIX_RATIO", raising=False)
    else:
        monkeypatch.setenv("GALAHGPU_PAIRS_MATRIX_RATIO", ratio)
    ctx.set_pairs_path(path)


def test_routing_of_the_border_calls(routed_ctx, graded, monkeypatch):
    sk, lens = graded
    thr, n, n_old = F(0.9), 130, 100
    ref = border_ref(sk, lens, n_old, thr)
    assert len(ref) > 100
    d_sk, d_lens = to_dev(sk), to_dev(lens)
    taken = routed_ctx.pairs_paths_taken()
    assert taken == {"default": 0, "matrix": 0, "auto": 0}
    for path, ratio, slot in ROUTES:
        set_route(routed_ctx, monkeypatch, path, ratio)
        assert tuples(routed_ctx.pairs_border(sk, lens, n_old, thr)) == ref, (path, ratio)
        now = routed_ctx.pairs_paths_taken()
        assert now == dict(taken, **{slot: taken[slot] + 1}), (path, ratio)
        taken = now
        assert device_border(routed_ctx, routed_ctx.pairs_border_device, d_sk, d_lens, n, n_old, thr) == ref, (path, ratio)
        now = routed_ctx.pairs_paths_taken()
        assert now == dict(taken, **{slot: taken[slot] + 1}), (path, ratio)
        taken = now
        # nothing to evaluate: nothing is run and nothing is counted, on any path
        assert len(routed_ctx.pairs_border(sk, lens, n, thr)) == 0
        assert routed_ctx.pairs_paths_taken() == taken


def test_routing_of_update_files(routed_ctx, golden, monkeypatch):
    thr = float(ga.parse_percentage(90))
    old_sk, old_lens = golden["sketches"][:SPLIT_OLD], golden["lens"][:SPLIT_OLD]
    new_paths = golden["paths"][SPLIT_OLD:]
    exp = None
    taken = routed_ctx.pairs_paths_taken()
    for path, ratio, slot in ROUTES:
        set_route(routed_ctx, monkeypatch, path, ratio)
        sk, lens, pairs, ani = routed_ctx.update_files(old_sk, old_lens, new_paths, thr)
        now = routed_ctx.pairs_paths_taken()
        assert now == dict(taken, **{slot: taken[slot] + 1}), (path, ratio)
        taken = now
        if exp is None:
            exp = (sk, lens, pairs, ani)
            assert tuples(pairs) == border_ref(golden["sketches"], golden["lens"], SPLIT_OLD, thr) and len(pairs) > 0
        assert (sk == exp[0]).all() and (lens == exp[1]).all()
        assert pairs.tobytes() == exp[2].tobytes(), (path, ratio)
        assert ani.dtype == np.float32 and ani.tobytes() == exp[3].tobytes(), (path, ratio)


def golden_clusters(golden, thr, cluster_ani):
    import oracle
    rows = [r for r in golden["pairs"] if oracle.ani(r[2], r[3]) >= np.float64(thr)]
    q = np.array([r[:4] for r in rows], dtype=np.uint32).reshape(-1, 4)
    ani = np.array([np.float32(oracle.ani(r[2], r[3])) for r in rows], dtype=np.float32)
    n = len(golden["paths"])
    return cluster_ref.clusters_ref(cluster_ref.cluster_ref(n, q[:, :2], ani, f32(cluster_ani))), q


def test_preclusterer_option_on_update(golden):
    thr = ga.parse_percentage(90)
    exp_clusters, q = golden_clusters(golden, thr, 0.95)
    cached = ga._context(21, 1000)
    one = cached.device_count == 1  # (several devices: the option is ignored)
    plain = ga.FinchPreclusterer(thr)
    old = plain.distances_state(golden["paths"][:SPLIT_OLD])
    exp = plain.update(old, golden["paths"][SPLIT_OLD:])
    assert [tuple(r) for r in q.tolist()] == tuples(exp.pairs)
    for path in ("matrix", "auto"):
        taken = cached.pairs_paths_taken()
        got = ga.FinchPreclusterer(thr, pairs_path=path).update(old, golden["paths"][SPLIT_OLD:])
        assert got.paths == exp.paths and got.pairs.tobytes() == exp.pairs.tobytes()
        assert got.ani.tobytes() == exp.ani.tobytes() and got.cache() == exp.cache()
        assert cached.pairs_path == "default"  # put back: the cached context is shared
        now = cached.pairs_paths_taken()
        assert sum(now.values()) == sum(taken.values()) + 1
        if path == "matrix":
            assert now["matrix"] == taken["matrix"] + (1 if one else 0)
    taken = cached.pairs_paths_taken()
    clusters, state = ga.cluster_update(old, golden["paths"][SPLIT_OLD:], ga.FinchPreclusterer(thr, pairs_path="matrix"),
                                        ga.FinchClusterer(0.95))
    assert clusters == exp_clusters
    assert clusters == ga.cluster_update(old, golden["paths"][SPLIT_OLD:], plain, ga.FinchClusterer(0.95))[0]
    assert state.pairs.tobytes() == exp.pairs.tobytes() and cached.pairs_path == "default"
    assert cached.pairs_paths_taken()["matrix"] == taken["matrix"] + (1 if one else 0)
    # distances_state under the option: the whole run as a border from nothing
    whole = ga.FinchPreclusterer(thr, pairs_path="matrix").distances_state(golden["paths"])
    assert whole.pairs.tobytes() == exp.pairs.tobytes() and cached.pairs_path == "default"
