"""The dense ANI matrix on the device (galah_amd/csrc/ani_matrix.hip):
common = A A^T on the i8 matrix instruction, total by the rank rule, the f32
ANI bit for bit.  The reference is always ani_pairs_host (finch's merge) over
all m^2 cells and ga.ani_f32 of its integers; common, total and the f32 bit
pattern must be equal -- there is no tolerance.  The sizes are those at which
the kernel takes another path: m around the 16-row blocks and the 64-row
tiles, column counts around the 64-column k-steps and the 512-column chunks,
the largest sketch size (many chunks into one accumulator), no column at all,
every tile and chunk full."""
import numpy as np
import pytest

import galah_amd as ga

pytestmark = pytest.mark.gpu


def reference(sk, lens, rows=None, k=21):
    """(common, total, ani) [m, m] by the host merge and ga.ani_f32."""
    rows = list(range(len(lens))) if rows is None else [int(r) for r in rows]
    m = len(rows)
    pairs, _ = ga.ani_pairs_host(sk, lens, [(a, b) for a in rows for b in rows], k=k)
    key = (pairs["common"].astype(np.uint64) << np.uint64(32)) | pairs["total"].astype(np.uint64)
    u, inv = np.unique(key, return_inverse=True)
    vals = np.array([ga.ani_f32(int(x) >> 32, int(x) & 0xFFFFFFFF, k) for x in u], np.float32)
    return pairs["common"].reshape(m, m), pairs["total"].reshape(m, m), vals[inv].reshape(m, m)


def assert_equal(got, ref, what=""):
    for name, g, r in zip(("common", "total", "ani"), got, ref):
        if g.tobytes() != r.tobytes():
            bad = np.argwhere(g.view(np.uint32) != r.view(np.uint32))
            a, b = bad[0]
            raise AssertionError("%s %s: %d cells differ, first (%d, %d): %r, expected %r"
                                 % (what, name, len(bad), a, b, g[a, b], r[a, b]))


def check(ctx, sk, lens, rows=None, what=""):
    ref = reference(sk, lens, rows, ctx.k)
    common, total, ani, summary = ctx.ani_matrix(sk, lens, rows)
    assert_equal((common, total, ani), ref, what)
    return ref, summary


def rows_from_sets(sets, s):
    sk = np.zeros((len(sets), s), np.uint64)
    lens = np.zeros(len(sets), np.uint32)
    for g, h in enumerate(sets):
        v = np.unique(np.asarray(list(h), dtype=np.uint64))
        sk[g, :len(v)] = v
        lens[g] = len(v)
    return sk, lens


# ---- 1. the golden sketches -------------------------------------------------
def test_golden_all_rows(gpu_ctx, golden):
    _, summary = check(gpu_ctx, golden["sketches"], golden["lens"], what="golden")
    assert summary["n_entries"] == int(golden["lens"].sum())
    assert 0 < 2 * summary["n_columns"] <= summary["column_entries"] <= summary["n_entries"]


def test_golden_files_against_the_table(gpu_ctx, golden):
    common, total, ani, _ = gpu_ctx.ani_matrix_files(golden["paths"])
    assert common.shape == (27, 27)
    for i, j, c, t, a in golden["pairs"]:
        for x, y in ((i, j), (j, i)):
            assert (int(common[x, y]), int(total[x, y])) == (c, t) and ani[x, y] == a
    lens = golden["lens"]
    assert np.array_equal(np.diag(common), lens) and np.array_equal(np.diag(total), lens)
    assert (np.diag(ani) == np.float32(1.0)).all()


# ---- 2. the edge set ------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx64():
    ctx = ga.Context(k=21, sketch_size=64, seed=0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def edge_set():
    """150 rows of at most 64 hashes over shared pools; one hash in every
    non-empty row; rows 3 and 4 identical; rows 140 and 141 share exactly one
    hash and nothing with any other row but the hash every row holds."""
    rng = np.random.default_rng(20261020)
    everywhere = 5
    pools = [np.arange(100 + 1000 * p, 100 + 1000 * p + 90, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             for p in range(4)]
    sets = []
    for g in range(150):
        kind = g % 10
        if kind == 0:
            sets.append(set())  # empty
        elif kind == 1:
            sets.append({everywhere})  # length 1
        elif kind == 2:
            sets.append({everywhere} | set(rng.choice(pools[g % 4], 3, replace=False).tolist()))  # short
        else:
            sets.append({everywhere} | set(rng.choice(pools[g % 4], 63, replace=False).tolist()))
    sets[4] = set(sets[3])
    sets[140] = {everywhere, 7} | set(range(10 ** 6, 10 ** 6 + 20))
    sets[141] = {everywhere, 7} | set(range(2 * 10 ** 6, 2 * 10 ** 6 + 30))
    sk, lens = rows_from_sets(sets, 64)
    order = rng.permutation(150)
    order = order[(order != 140) & (order != 141)]
    return sk, lens, order


@pytest.mark.parametrize("m", (1, 2, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130))
def test_edge_set(ctx64, edge_set, m):
    sk, lens, order = edge_set
    rows = [int(r) for r in order[:m]]
    if m >= 2:
        rows[0], rows[-1] = 140, 141  # the pair sharing one hash (and the common one): first and last tile
    if m >= 15:
        rows[m // 2] = rows[1]  # one row listed twice
        rows[2], rows[m - 2] = 3, 4  # the identical rows
        rows[3], rows[4], rows[5] = 0, 1, 2  # an empty, a length-1 and a short row
    ref, _ = check(ctx64, sk, lens, rows, what="m=%d" % m)
    if m >= 2:
        assert int(ref[0][0, m - 1]) == 2  # the one hash and the one every row holds


# ---- 3. column-count edges ------------------------------------------------------
@pytest.mark.parametrize("columns", (0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025))
def test_column_count_edges(columns):
    """Rows 0 and 1 share exactly `columns` hashes, every row has hashes of its own."""
    shared = set(range(10, 10 + 3 * columns, 3))
    sets = [shared | set(range(11, 11 + 3 * 9, 3)), shared | set(range(12, 12 + 3 * 7, 3)),
            set(range(10 ** 9, 10 ** 9 + 40))]
    with ga.Context(k=21, sketch_size=1040, seed=0) as ctx:
        sk, lens = rows_from_sets(sets, 1040)
        ref, summary = check(ctx, sk, lens, what="columns=%d" % columns)
    assert summary["n_columns"] == columns and summary["column_entries"] == 2 * columns
    assert summary["n_entries"] == int(lens.sum())
    assert int(ref[0][0, 1]) == columns and int(ref[0][0, 2]) == 0


# ---- 4. accumulation across many chunks -------------------------------------------
def test_many_chunks_at_the_largest_sketch_size():
    s = 12000
    full = np.arange(1, s + 1, dtype=np.uint64) * np.uint64(977)
    half = np.concatenate([full[::2], np.arange(1, s // 2 + 1, dtype=np.uint64) * np.uint64(977) + np.uint64(1)])
    sk, lens = rows_from_sets([full, full, full, half], s)
    assert lens.tolist() == [s] * 4
    with ga.Context(k=21, sketch_size=s, seed=0) as ctx:
        ref, summary = check(ctx, sk, lens, what="s=12000")
    assert int(ref[0][0, 1]) == 12000 and int(ref[0][1, 2]) == 12000 and int(ref[0][0, 3]) == 6000
    assert summary["n_columns"] == 12000 and summary["column_entries"] == 3 * 12000 + 6000


# ---- 5. / 6. no shared hash, and a dense group --------------------------------------
@pytest.fixture(scope="module")
def disjoint_rows():
    rng = np.random.default_rng(5)
    v = rng.permutation(200 * 1000).astype(np.uint64).reshape(200, 1000) * np.uint64(7919) + np.uint64(1)
    return np.sort(v, axis=1), np.full(200, 1000, np.uint32)


@pytest.fixture(scope="module")
def dense_rows():
    rng = np.random.default_rng(6)
    pool = np.unique(rng.integers(1, 2 ** 62, 1200, dtype=np.uint64))[:1100]
    assert len(pool) == 1100
    sk = np.stack([np.sort(rng.choice(pool, 1000, replace=False)) for _ in range(200)])
    return sk, np.full(200, 1000, np.uint32)


def test_no_shared_hash(gpu_ctx, disjoint_rows):
    sk, lens = disjoint_rows
    ref, summary = check(gpu_ctx, sk, lens, what="disjoint")
    assert summary["n_columns"] == 0 and summary["column_entries"] == 0 and summary["n_entries"] == 200000
    off = ~np.eye(200, dtype=bool)
    assert not ref[0][off].any() and not ref[2][off].any()
    # total still follows the rank rule: |T| + #{s <= last T}, which differs from pair to pair
    assert (ref[1][off] >= 1000).all() and (ref[1][off] < 2000).any() and len(np.unique(ref[1][off])) > 1


def test_dense_group(gpu_ctx, dense_rows):
    sk, lens = dense_rows
    ref, summary = check(gpu_ctx, sk, lens, what="dense")
    assert summary["n_columns"] == 1100 and summary["column_entries"] == 200000
    assert ref[0][~np.eye(200, dtype=bool)].min() >= 900


# ---- 7. the device form ---------------------------------------------------------------
def test_device_form_on_a_stream(gpu_ctx, golden):
    import torch
    sk, lens = golden["sketches"], golden["lens"]
    n = len(lens)
    ref = reference(sk, lens)
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def fresh(dtype):
        return torch.full((n, n), -7, dtype=dtype, device="cuda")

    with torch.cuda.stream(stream):
        # all three, d_rows = NULL
        d_c, d_t, d_a = fresh(torch.int32), fresh(torch.int32), fresh(torch.float32)
        torch.cuda.synchronize()
        summary = gpu_ctx.ani_matrix_device(d_sk, d_lens, n, None, n, d_c, d_t, d_a, stream=stream.cuda_stream)
        got = (d_c.cpu().numpy().view(np.uint32), d_t.cpu().numpy().view(np.uint32), d_a.cpu().numpy())
        assert_equal(got, ref, "device form")
        assert summary["n_entries"] == int(lens.sum())
        # each output alone
        for which in range(3):
            out = [None, None, None]
            out[which] = fresh(torch.float32 if which == 2 else torch.int32)
            torch.cuda.synchronize()
            gpu_ctx.ani_matrix_device(d_sk, d_lens, n, None, n, *out, stream=stream.cuda_stream)
            g = out[which].cpu().numpy()
            assert (g if which == 2 else g.view(np.uint32)).tobytes() == ref[which].tobytes(), which
        # an index >= n is an empty row
        rows = np.array([3, n, 0, 2 ** 32 - 1, 3], np.uint32)
        d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
        d_c, d_t, d_a = (fresh(torch.int32)[:5, :5].contiguous(), fresh(torch.int32)[:5, :5].contiguous(),
                         fresh(torch.float32)[:5, :5].contiguous())
        torch.cuda.synchronize()
        gpu_ctx.ani_matrix_device(d_sk, d_lens, n, d_rows, 5, d_c, d_t, d_a, stream=stream.cuda_stream)
    c, t, a = d_c.cpu().numpy(), d_t.cpu().numpy(), d_a.cpu().numpy()
    sub = [0, 2, 4]
    exp = reference(sk, lens, [3, 0, 3])
    assert np.array_equal(c[np.ix_(sub, sub)].view(np.uint32), exp[0])
    assert np.array_equal(t[np.ix_(sub, sub)].view(np.uint32), exp[1])
    assert a[np.ix_(sub, sub)].tobytes() == exp[2].tobytes()
    for e in (1, 3):
        assert not c[e].any() and not c[:, e].any() and not t[e].any() and not t[:, e].any()
        assert not a[e].any() and not a[:, e].any()
    # m == 0 writes nothing
    assert gpu_ctx.ani_matrix_device(d_sk, d_lens, n, None, 0, d_c, d_t, d_a)["n_entries"] == 0


# ---- 8. the margin flags every entry ----------------------------------------------------
def test_every_entry_flagged_second_pass(gpu_ctx, dense_rows, monkeypatch):
    """E = 2^0: every cell with 0 < common < total is flagged, 19,900 upper-triangle
    cells against a first list of 4,096; the second pass runs and the result is unchanged."""
    sk, lens = dense_rows
    ref = reference(sk, lens)
    upper = np.triu(np.ones((200, 200), dtype=bool), 1)
    inner = int(((ref[0] > 0) & (ref[0] < ref[1]) & upper).sum())
    assert inner > 4096
    monkeypatch.setenv("GALAHGPU_TEST_ANI_MARGIN_LOG2", "0")
    common, total, ani, summary = gpu_ctx.ani_matrix(sk, lens)
    assert_equal((common, total, ani), ref, "margin")
    assert summary["ani_rechecked"] == 2 * inner
    monkeypatch.delenv("GALAHGPU_TEST_ANI_MARGIN_LOG2")
    common, total, ani, summary = gpu_ctx.ani_matrix(sk, lens)
    assert_equal((common, total, ani), ref, "default margin")
    assert summary["ani_rechecked"] < 200
