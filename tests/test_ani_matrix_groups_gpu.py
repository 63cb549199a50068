"""The dense ANI matrices of many groups in one call on the device (DESIGN.md
4.11; galah_amd/csrc/ani_matrix.hip, the grouped form).  The reference is
always finch's merge: ani_pairs_host over a block's cells and ga.ani_f32 of
its integers; common, total and the f32 bit pattern of every cell of every
block must be equal -- there is no tolerance.  The sizes are those at which
the grouped form takes another path: group sizes around the 64-position tiles
(tiles are local to a group), groups of one and of none (no product
workgroup), the same hash in several groups (a column of each or of none),
column counts around the 512-column chunks with ids local to a group, a long
tile-pair prefix to search, more positions than the one-matrix form takes."""
import numpy as np
import pytest

import galah_amd as ga

pytestmark = pytest.mark.gpu


def block_reference(sk, lens, rows, k=21):
    """(common, total, ani) [m, m] of one group by the host merge and ga.ani_f32."""
    rows = [int(r) for r in rows]
    m = len(rows)
    if m == 0:
        z = np.zeros((0, 0), np.uint32)
        return z, z, np.zeros((0, 0), np.float32)
    pairs, _ = ga.ani_pairs_host(sk, lens, [(a, b) for a in rows for b in rows], k=k)
    key = (pairs["common"].astype(np.uint64) << np.uint64(32)) | pairs["total"].astype(np.uint64)
    u, inv = np.unique(key, return_inverse=True)
    vals = np.array([ga.ani_f32(int(x) >> 32, int(x) & 0xFFFFFFFF, k) for x in u], np.float32)
    return pairs["common"].reshape(m, m), pairs["total"].reshape(m, m), vals[inv].reshape(m, m)


def reference(sk, lens, groups, k=21):
    """The flat (common, total, ani) of the groups, block after block."""
    blocks = [block_reference(sk, lens, g, k) for g in groups]
    return tuple(np.concatenate([b[w].reshape(-1) for b in blocks]) if blocks else np.zeros(0, t)
                 for w, t in ((0, np.uint32), (1, np.uint32), (2, np.float32)))


def assert_equal(got, ref, groups, what=""):
    cells = np.concatenate([[0], np.cumsum([len(g) ** 2 for g in groups])])
    for name, g, r in zip(("common", "total", "ani"), got, ref):
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        if g.tobytes() != r.tobytes():
            bad = np.flatnonzero(g.view(np.uint32) != r.view(np.uint32))
            grp = int(np.searchsorted(cells, bad[0], side="right")) - 1
            a, b = divmod(int(bad[0] - cells[grp]), len(groups[grp]))
            raise AssertionError("%s %s: %d cells differ, first in group %d (m %d) at (%d, %d): %r, expected %r"
                                 % (what, name, len(bad), grp, len(groups[grp]), a, b, g[bad[0]], r[bad[0]]))


def check(ctx, sk, lens, groups, what="", ref=None):
    ref = reference(sk, lens, groups, ctx.k) if ref is None else ref
    common, total, ani, cells, summary = ctx.ani_matrix_groups(sk, lens, groups)
    assert cells.tolist() == np.concatenate([[0], np.cumsum([len(g) ** 2 for g in groups])]).tolist()
    assert_equal((common, total, ani), ref, groups, what)
    return ref, summary


def rows_from_sets(sets, s):
    sk = np.zeros((len(sets), s), np.uint64)
    lens = np.zeros(len(sets), np.uint32)
    for g, h in enumerate(sets):
        v = np.unique(np.asarray(list(h), dtype=np.uint64))
        sk[g, :len(v)] = v
        lens[g] = len(v)
    return sk, lens


def dict_columns(sk, lens, groups):
    """(columns, column entries) by the grouped rule, from a dict per group."""
    columns = entries = 0
    for g in groups:
        held = {}
        for r in g:
            for h in sk[r, :lens[r]].tolist():
                held[h] = held.get(h, 0) + 1
        columns += sum(1 for c in held.values() if c >= 2)
        entries += sum(c for c in held.values() if c >= 2)
    return columns, entries


@pytest.fixture(scope="module")
def ctx64():
    ctx = ga.Context(k=21, sketch_size=64, seed=0)
    yield ctx
    ctx.close()


# ---- 1. the golden sketches ---------------------------------------------------
@pytest.fixture(scope="module")
def golden_groups(golden):
    keep = [(i, j, c, t) for i, j, c, t, a in golden["pairs"] if a >= ga.parse_percentage(0.9)]
    return ga.preclusters(len(golden["lens"]), np.array(keep, dtype=ga.PAIR_DTYPE))


@pytest.fixture(scope="module")
def golden_ref(golden, golden_groups):
    return reference(golden["sketches"], golden["lens"], golden_groups)


def test_golden_preclusters(gpu_ctx, golden, golden_groups, golden_ref):
    _, summary = check(gpu_ctx, golden["sketches"], golden["lens"], golden_groups, "golden", golden_ref)
    assert summary["n_entries"] == int(golden["lens"].sum())
    columns, entries = dict_columns(golden["sketches"], golden["lens"], golden_groups)
    assert (summary["n_columns"], summary["column_entries"]) == (columns, entries)


def test_golden_files_preclusters_and_matrices(gpu_ctx, golden, golden_groups, golden_ref):
    members, offsets, cells, common, total, ani, summary = gpu_ctx.precluster_matrices_files(
        golden["paths"], ga.parse_percentage(0.9))
    groups = [members[offsets[g]:offsets[g + 1]].tolist() for g in range(len(offsets) - 1)]
    assert groups == golden_groups
    assert cells.tolist() == ga.ani_matrix_group_cells(offsets).tolist()
    assert_equal((common, total, ani), golden_ref, groups, "files")
    assert summary["n_entries"] == int(golden["lens"].sum())
    block = ga.ani_matrix_block(ani, offsets, cells, 0)
    assert block.shape == (len(groups[0]),) * 2 and (np.diag(block) == np.float32(1.0)).all()


# ---- 2. tile edges inside groups ------------------------------------------------
@pytest.fixture(scope="module")
def edge_set():
    """150 rows of at most 64 hashes over shared pools, as test_ani_matrix_gpu.py's:
    one hash in every non-empty row; rows 3 and 4 identical; rows 140 and 141
    share exactly one hash and nothing else but the hash every row holds."""
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
    return rows_from_sets(sets, 64)


EDGE_SIZES = [130, 65, 64, 63, 33, 17, 16, 2, 1, 0, 1]


@pytest.fixture(scope="module")
def edge_groups():
    rng = np.random.default_rng(7)
    groups = []
    for m in EDGE_SIZES:
        rows = [int(r) for r in rng.permutation(150)[:m]]
        if m >= 2:
            rows[0], rows[-1] = 140, 141  # the pair sharing one hash: first and last tile of the group
        if m >= 16:
            rows[m // 2] = rows[1]  # one row listed twice
            rows[2], rows[m - 2] = 3, 4  # the identical rows
            rows[3], rows[4], rows[5] = 0, 1, 2  # an empty, a length-1 and a short row
        groups.append(rows)
    groups[-3], groups[-1] = [0], [13]  # the groups of one: an empty row and a full one
    return groups


@pytest.mark.parametrize("order", ("as listed", "reversed"))
def test_tile_edges_inside_groups(ctx64, edge_set, edge_groups, order):
    sk, lens = edge_set
    groups = edge_groups if order == "as listed" else edge_groups[::-1]
    assert [len(g) for g in groups] == (EDGE_SIZES if order == "as listed" else EDGE_SIZES[::-1])
    ref, summary = check(ctx64, sk, lens, groups, order)
    assert (summary["n_columns"], summary["column_entries"]) == dict_columns(sk, lens, groups)
    # cell (0, 129) of the group of 130, rows 140 and 141: the one hash and the one every row holds
    assert int(ref[0][129 if order == "as listed" else len(ref[0]) - 130 * 130 + 129]) == 2


# ---- 3. the same hashes in several groups ------------------------------------------
def test_hashes_across_groups(ctx64):
    sets = [{11, 12, 101, 102}, {11, 201, 202}, {11, 12, 301}, {301, 401}, {501, 502}]
    sk, lens = rows_from_sets(sets, 64)
    # 11: r0, r1, r2 -- a column of the first group only; 12: r0, r2 -- of none; r1 also listed in the third group
    groups = [[0, 1], [2, 3], [4, 1]]
    ref, summary = check(ctx64, sk, lens, groups, "across ")
    assert summary["n_columns"] == dict_columns(sk, lens, groups)[0] == 2  # 11 in the first group, 301 in the second
    assert summary["column_entries"] == 4 and summary["n_entries"] == int(lens[[0, 1, 2, 3, 4, 1]].sum())
    assert ref[0].tolist() == [4, 1, 1, 3, 3, 1, 1, 2, 2, 0, 0, 3]


# ---- 4. chunk edges with group-local column ids --------------------------------------
def test_chunk_edges_with_local_numbering():
    """A first group of 7 columns, then groups of exactly 0, 511, 512, 513 and
    1,025 columns over the same hashes: a group's ids begin at 0 whatever lies
    before it."""
    s, counts = 1040, (7, 0, 511, 512, 513, 1025)
    sets, groups = [], []
    for g, c in enumerate(counts):
        shared = set(range(10, 10 + 3 * c, 3))
        base = 10 ** 9 * (g + 1)
        sets += [shared | set(range(base + 1, base + 10)), shared | set(range(base + 11, base + 18)),
                 set(range(base + 21, base + 61))]
        groups.append([3 * g, 3 * g + 1, 3 * g + 2])
    sk, lens = rows_from_sets(sets, s)
    with ga.Context(k=21, sketch_size=s, seed=0) as ctx:
        ref, summary = check(ctx, sk, lens, groups, "chunk edges ")
    assert summary["n_columns"] == sum(counts) and summary["column_entries"] == 2 * sum(counts)
    assert [int(ref[0][9 * g + 1]) for g in range(len(counts))] == list(counts)


# ---- 5. degenerate groups ----------------------------------------------------------------
def test_degenerate_groups(ctx64):
    sets = [set(), set(), set()] + [set(range(1000 * g, 1000 * g + 50)) for g in range(1, 71)]
    sk, lens = rows_from_sets(sets, 64)
    groups = [[0, 1, 2], list(range(3, 73))]  # every row empty; 70 rows that share nothing (two tiles)
    ref, summary = check(ctx64, sk, lens, groups, "degenerate ")
    assert summary["n_columns"] == 0 and summary["column_entries"] == 0 and summary["n_entries"] == 70 * 50
    assert not ref[0][:9].any() and not ref[1][:9].any() and not ref[2][:9].any()
    block = ref[0][9:].reshape(70, 70)
    assert np.array_equal(block, np.diag(np.full(70, 50, np.uint32)))


# ---- 6. many chunks into one accumulator -----------------------------------------------------
def test_groups_at_the_largest_sketch_size():
    s = 12000
    full = np.arange(1, s + 1, dtype=np.uint64) * np.uint64(977)
    half = np.concatenate([full[::2], np.arange(1, s // 2 + 1, dtype=np.uint64) * np.uint64(977) + np.uint64(1)])
    third = np.concatenate([full[::3], np.arange(1, s - s // 3 + 1, dtype=np.uint64) * np.uint64(977) + np.uint64(2)])
    sk, lens = rows_from_sets([full, half, third, full], s)
    assert lens.tolist() == [s] * 4
    groups = [[0, 1, 2], [3, 0, 1, 2] * 17 + [1, 2]]  # 3 and 70 positions over four rows
    assert len(groups[1]) == 70
    block = block_reference(sk, lens, [0, 1, 2, 3])  # every cell of both blocks is a cell of these 16
    ref = tuple(np.concatenate([block[w][np.ix_(g, g)].reshape(-1) for g in groups]) for w in range(3))
    with ga.Context(k=21, sketch_size=s, seed=0) as ctx:
        check(ctx, sk, lens, groups, "s=12000", ref)
    assert int(block[0][0, 3]) == 12000 and int(block[0][0, 1]) == 6000 and int(block[0][0, 2]) == 4000


# ---- 7. / 8. many small groups; more positions than one matrix takes ----------------------------
def clustered_rows(n_clusters, per, s, seed):
    """n_clusters * per rows of s hashes: a cluster's rows draw from a pool of their own (3 s / 2 hashes)."""
    rng = np.random.default_rng(seed)
    sk = np.zeros((n_clusters * per, s), np.uint64)
    for c in range(n_clusters):
        pool = np.uint64(1 + c * 4 * s) + rng.permutation(3 * s // 2 * 2)[:3 * s // 2].astype(np.uint64)
        for r in range(per):
            sk[c * per + r] = np.sort(rng.choice(pool, s, replace=False))
    return sk, np.full(n_clusters * per, s, np.uint32)


def grouped_reference(sk, lens, groups, k=21):
    """reference() with one ani_pairs_host call for all groups (many small groups)."""
    listed = [(a, b) for g in groups for a in g for b in g]
    pairs, _ = ga.ani_pairs_host(sk, lens, listed, k=k)
    key = (pairs["common"].astype(np.uint64) << np.uint64(32)) | pairs["total"].astype(np.uint64)
    u, inv = np.unique(key, return_inverse=True)
    vals = np.array([ga.ani_f32(int(x) >> 32, int(x) & 0xFFFFFFFF, k) for x in u], np.float32)
    return pairs["common"].copy(), pairs["total"].copy(), vals[inv]


def test_many_small_groups(ctx64):
    sk, lens = clustered_rows(1000, 6, 64, 8)
    lens[::97] = 0  # some empty rows, some of them alone in a group
    rng = np.random.default_rng(9)
    sizes = rng.integers(1, 4, 3000)
    rows = rng.integers(0, 6, sizes.sum())
    groups, at = [], 0
    for g, m in enumerate(sizes):
        groups.append([(g % 1000) * 6 + int(r) for r in rows[at:at + m]])  # rows of one cluster, repeats allowed
        at += m
    ref = grouped_reference(sk, lens, groups)
    _, summary = check(ctx64, sk, lens, groups, "3000 groups", ref)
    assert summary["n_columns"] > 0
    assert (ref[0] > 0).sum() > 3000


def test_more_positions_than_one_matrix_takes():
    s = 16
    sk, lens = clustered_rows(5000, 8, s, 10)
    groups = [list(range(8 * c, 8 * c + 8)) for c in range(5000)]
    ref = grouped_reference(sk, lens, groups)
    assert len(ref[0]) == 320000
    with ga.Context(k=21, sketch_size=s, seed=0) as ctx:
        _, summary = check(ctx, sk, lens, groups, "40000 positions", ref)
    assert summary["n_entries"] == 40000 * s
    off = ref[0].reshape(5000, 8, 8)[:, ~np.eye(8, dtype=bool)]
    assert off.min() >= 8  # two rows of 16 from a pool of 24


# ---- 9. one group of all rows is the one-matrix form ----------------------------------------------
def test_one_group_equals_the_matrix(gpu_ctx, golden):
    sk, lens = golden["sketches"], golden["lens"]
    rows = list(range(26, -1, -1)) + [3]
    common, total, ani, cells, summary = gpu_ctx.ani_matrix_groups(sk, lens, [rows])
    mc, mt, ma, msummary = gpu_ctx.ani_matrix(sk, lens, rows)
    assert cells.tolist() == [0, 28 * 28]
    assert common.tobytes() == mc.tobytes() and total.tobytes() == mt.tobytes() and ani.tobytes() == ma.tobytes()
    assert summary == msummary


# ---- 10. the device form ------------------------------------------------------------------------
def test_device_form_on_a_stream(gpu_ctx, golden, golden_groups, golden_ref):
    import torch
    sk, lens = golden["sketches"], golden["lens"]
    n = len(lens)
    offsets = np.concatenate([[0], np.cumsum([len(g) for g in golden_groups])]).astype(np.uint32)
    members = np.concatenate(golden_groups).astype(np.uint32)
    cells = int(ga.ani_matrix_group_cells(offsets)[-1])
    d_sk = torch.from_numpy(sk.view(np.int64)).cuda()
    d_lens = torch.from_numpy(lens.view(np.int32)).cuda()
    d_members = torch.from_numpy(members.view(np.int32)).cuda()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()

    def fresh(dtype, count=cells):
        return torch.full((count,), -7, dtype=dtype, device="cuda")

    with torch.cuda.stream(stream):
        d_c, d_t, d_a = fresh(torch.int32), fresh(torch.int32), fresh(torch.float32)
        torch.cuda.synchronize()
        summary = gpu_ctx.ani_matrix_groups_device(d_sk, d_lens, n, d_members, offsets, d_c, d_t, d_a,
                                                   stream=stream.cuda_stream)
        got = (d_c.cpu().numpy().view(np.uint32), d_t.cpu().numpy().view(np.uint32), d_a.cpu().numpy())
        assert_equal(got, golden_ref, golden_groups, "device form")
        assert summary["n_entries"] == int(lens.sum())
        for which in range(3):  # each output alone
            out = [None, None, None]
            out[which] = fresh(torch.float32 if which == 2 else torch.int32)
            torch.cuda.synchronize()
            gpu_ctx.ani_matrix_groups_device(d_sk, d_lens, n, d_members, offsets, *out, stream=stream.cuda_stream)
            g = out[which].cpu().numpy()
            assert (g if which == 2 else g.view(np.uint32)).tobytes() == golden_ref[which].tobytes(), which
        # an index >= n is an empty row: in a group of three and alone in a group
        rows = np.array([3, n, 0, 2 ** 32 - 1], np.uint32)
        d_rows = torch.from_numpy(rows.view(np.int32)).cuda()
        d_c, d_t, d_a = fresh(torch.int32, 10), fresh(torch.int32, 10), fresh(torch.float32, 10)
        torch.cuda.synchronize()
        gpu_ctx.ani_matrix_groups_device(d_sk, d_lens, n, d_rows, np.array([0, 3, 4], np.uint32), d_c, d_t, d_a,
                                         stream=stream.cuda_stream)
    c, t, a = d_c.cpu().numpy(), d_t.cpu().numpy(), d_a.cpu().numpy()
    exp = block_reference(sk, lens, [3, 0])
    sub = np.ix_([0, 2], [0, 2])
    assert np.array_equal(c[:9].reshape(3, 3)[sub].view(np.uint32), exp[0])
    assert np.array_equal(t[:9].reshape(3, 3)[sub].view(np.uint32), exp[1])
    assert a[:9].reshape(3, 3)[sub].tobytes() == exp[2].tobytes()
    for x in (c, t, a):
        assert not x[:9].reshape(3, 3)[1].any() and not x[:9].reshape(3, 3)[:, 1].any() and not x[9]
    # no group, and groups without a position, write nothing
    assert gpu_ctx.ani_matrix_groups_device(d_sk, d_lens, n, d_rows, np.array([0], np.uint32), d_c)["n_entries"] == 0
    assert gpu_ctx.ani_matrix_groups_device(d_sk, d_lens, n, d_rows, np.array([0, 0, 0], np.uint32), d_c)["n_entries"] == 0


# ---- 11. the margin flags every entry ---------------------------------------------------------------
def test_every_entry_flagged_second_pass(ctx64, monkeypatch):
    """E = 2^0: every cell with 0 < common < total is flagged, on both sides of
    the diagonal, against a first list of 4,096; the second pass runs and both
    mirrored cells of both blocks hold the host's value."""
    sk, lens = clustered_rows(1, 203, 64, 11)
    groups = [list(range(200)), [200, 201, 202]]
    ref = reference(sk, lens, groups)
    inner = int(((ref[0] > 0) & (ref[0] < ref[1])).sum())  # off-diagonal cells, both triangles
    assert inner > 4096 and inner % 2 == 0
    assert int(((ref[0][40000:] > 0) & (ref[0][40000:] < ref[1][40000:])).sum()) == 6
    monkeypatch.setenv("GALAHGPU_TEST_ANI_MARGIN_LOG2", "0")
    _, summary = check(ctx64, sk, lens, groups, "margin", ref)
    assert summary["ani_rechecked"] == inner
    monkeypatch.delenv("GALAHGPU_TEST_ANI_MARGIN_LOG2")
    _, summary = check(ctx64, sk, lens, groups, "default margin", ref)
    assert summary["ani_rechecked"] < 200
