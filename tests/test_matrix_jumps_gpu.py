"""The chunk loop's jump on the device, in all three forms of mx_common_kernel
(galah_amd/csrc/ani_matrix.hip): the dense matrix, the
grouped matrices and the passing-pair list.

A tile pair jumps over every chunk of 512 columns in which either tile holds
nothing: it sets k0, passes a barrier, searches every row's cursor again from
its last value and carries the accumulators across the gap.  On clustered
input that is the normal path, and no fixture of the three other matrix files
takes it (test_matrix_schedule.py shows that, and shows what each scenario
here contains: matrix_cases.py holds the inputs and the model of the loop).

The references and the equality rules are those of the three other files:
ani_pairs_host (finch's merge) over all cells and ga.ani_f32 of its integers
for the dense and the grouped form -- common, total and the f32 bit pattern
equal; pairs_border_host as sorted (i, j, common, total) tuples for the pair
form.  There is no tolerance.  The device's counts of columns are compared
with the model's.

Also here, two edges of the shared prologue: the hashes 0 and 2^64 - 1 as
columns (the sort's padding is the key ~0, a row's unused slots hold 0), and
mx_offsets_kernel's scan past its first wave."""
import numpy as np
import pytest

import galah_amd as ga
import matrix_cases as mc

pytestmark = pytest.mark.gpu

F = lambda x: float(np.float32(x))  # noqa: E731  (a threshold as the f32 the library takes)


# ---- references ---------------------------------------------------------------------------
def dense_reference(sk, lens, rows=None, k=21):
    """(common, total, ani) [m, m] by the host merge and ga.ani_f32."""
    rows = list(range(len(lens))) if rows is None else [int(r) for r in rows]
    m = len(rows)
    pairs, _ = ga.ani_pairs_host(sk, lens, [(a, b) for a in rows for b in rows], k=k)
    key = (pairs["common"].astype(np.uint64) << np.uint64(32)) | pairs["total"].astype(np.uint64)
    u, inv = np.unique(key, return_inverse=True)
    vals = np.array([ga.ani_f32(int(x) >> 32, int(x) & 0xFFFFFFFF, k) for x in u], np.float32)
    return pairs["common"].reshape(m, m), pairs["total"].reshape(m, m), vals[inv].reshape(m, m)


def groups_reference(sk, lens, groups):
    blocks = [dense_reference(sk, lens, g) for g in groups]
    return tuple(np.concatenate([b[w].reshape(-1) for b in blocks]) for w in range(3))


def assert_dense_equal(got, ref, what):
    for name, g, r in zip(("common", "total", "ani"), got, ref):
        assert g.shape == r.shape, (what, name)
        if g.tobytes() != r.tobytes():
            bad = np.argwhere(g.view(np.uint32) != r.view(np.uint32))
            at = tuple(int(x) for x in bad[0])
            raise AssertionError("%s %s: %d cells differ, first %r: %r, expected %r"
                                 % (what, name, len(bad), at, g[at], r[at]))


def check_dense(ctx, sk, lens, rows, ref, sched, what):
    common, total, ani, summary = ctx.ani_matrix(sk, lens, rows)
    assert_dense_equal((common, total, ani), ref, what)
    assert (summary["n_columns"], summary["column_entries"]) == (sched.n_columns, sched.column_entries)
    assert summary["n_entries"] == sum(sched.lens)
    return common, total, ani


def tuples(p):
    return list(zip(p["i"].tolist(), p["j"].tolist(), p["common"].tolist(), p["total"].tolist()))


def pairs_reference(sk, lens, min_ani, rows=None):
    """The passing pairs by the host merge, sorted (i, j, common, total) tuples of row indices."""
    if rows is None:
        return tuples(ga.pairs_border_host(sk, lens, 0, min_ani))
    rows = np.asarray(rows, dtype=np.int64)
    p = ga.pairs_border_host(sk[rows], lens[rows], 0, min_ani)
    a, b = rows[p["i"]], rows[p["j"]]
    return sorted(zip(np.minimum(a, b).tolist(), np.maximum(a, b).tolist(), p["common"].tolist(), p["total"].tolist()))


def check_pairs(ctx, sk, lens, min_ani, rows, ref, sched, what):
    pairs, summary = ctx.pairs_matrix(sk, lens, min_ani, rows)
    got = tuples(pairs)
    if got != ref:
        missing, extra = sorted(set(ref) - set(got)), sorted(set(got) - set(ref))
        raise AssertionError("%s: %d pairs, the merge passes %d; missing %r, not in the merge %r"
                             % (what, len(got), len(ref), missing[:3], extra[:3]))
    assert summary["n_pairs"] == len(ref) and summary["path"] == "matrix"
    assert (summary["n_columns"], summary["column_entries"]) == (sched.n_columns, sched.column_entries)
    assert summary["chunk_rounds"] == len(sched.pairs) * -(-sched.n_columns // mc.CHUNK)


@pytest.fixture(scope="module")
def ctx64():
    ctx = ga.Context(k=21, sketch_size=64, seed=0)
    yield ctx
    ctx.close()


@pytest.fixture(scope="module")
def ctx128():
    ctx = ga.Context(k=21, sketch_size=128, seed=0)
    yield ctx
    ctx.close()


# ---- scenario A: banded clusters, rows in cluster order -------------------------------------
@pytest.fixture(scope="module")
def a_sched():
    return mc.chunk_schedule(*mc.scenario_a())


@pytest.fixture(scope="module")
def a_dense():
    return dense_reference(*mc.scenario_a())


def test_a_dense(ctx64, a_sched, a_dense):
    """300 rows in 5 tiles (the last of 44): 22 jumps over the 15 tile pairs,
    five of which run no chunk at all."""
    sk, lens = mc.scenario_a()
    s = a_sched
    assert s.n_jumps() > 0 and s.first_jump_then_shared() and s.run_jump_run(2) and s.jump_without_run()
    common, total, _ = check_dense(ctx64, sk, lens, None, a_dense, s, "scenario A")
    # a cell whose common comes only from chunks after a jump from 0, and one that collects on both sides of a gap
    model = s.common()
    for _, (a, b) in s.first_jump_then_shared() + s.run_jump_run(2):
        assert int(common[a, b]) == int(model[a, b]) > 0
    # a tile pair that jumped and ran nothing: common 0, total by the rank rule (at least the shorter row's length)
    for ti, tj in s.jump_without_run():
        rows, cols = slice(64 * ti, 64 * ti + 64), slice(64 * tj, 64 * tj + 64)
        assert not common[rows, cols].any() and not common[cols, rows].any()
        assert np.array_equal(total[rows, cols], a_dense[1][rows, cols])
        assert (total[rows, cols] >= np.minimum.outer(lens[rows], lens[cols])).all()


def test_a_dense_one_row_in_two_tiles(ctx64):
    sk, lens = mc.scenario_a()
    rows = mc.scenario_a_listed()
    s = mc.chunk_schedule(sk, lens, rows)
    assert s.n_jumps() > 0
    common, total, ani = check_dense(ctx64, sk, lens, rows, dense_reference(sk, lens, rows), s, "scenario A, listed")
    a, b = mc.A_TWICE
    assert int(common[a, b]) == int(total[a, b]) == int(lens[a]) and ani[a, b] == np.float32(1.0)


def test_a_pairs_every_pair(ctx64, a_sched):
    """At 0.0 pairs without a shared hash pass: no tile pair may leave early, and every cell is emitted."""
    sk, lens = mc.scenario_a()
    ref = pairs_reference(sk, lens, 0.0)
    assert len(ref) == 300 * 299 // 2 and a_sched.jump_without_run()
    check_pairs(ctx64, sk, lens, 0.0, None, ref, a_sched, "scenario A at 0.0")


@pytest.mark.parametrize("thr", (0.9, 0.98))
def test_a_pairs_at_a_threshold(ctx64, a_sched, thr, monkeypatch):
    """Some pairs pass, not all, and none without a shared hash: the tile
    pairs that ran no chunk leave before the epilogue."""
    sk, lens = mc.scenario_a()
    ref = pairs_reference(sk, lens, F(thr))
    print("scenario A at %s: %d of %d pairs" % (thr, len(ref), 300 * 299 // 2))
    assert 0 < len(ref) < 300 * 299 // 2 and all(r[2] > 0 for r in ref)
    check_pairs(ctx64, sk, lens, F(thr), None, ref, a_sched, "scenario A at %s" % thr)
    assert tuples(ctx64.pairs(sk, lens, F(thr))) == ref  # K2, the default pair kernel
    monkeypatch.setenv("GALAHGPU_TEST_PAIRS_SLICE", "1")  # a launch per tile pair
    check_pairs(ctx64, sk, lens, F(thr), None, ref, a_sched, "scenario A at %s, sliced" % thr)


# ---- scenario B: boundary ids after a jump ----------------------------------------------------
@pytest.fixture(scope="module")
def b_dense():
    return dense_reference(*mc.scenario_b())


def test_b_boundary_ids_after_a_jump(ctx128, b_dense):
    """matrix_cases.scenario_b: four tiles at s = 128 over 2,560 columns whose
    id is their number (tile 3 only supplies two holders for every column).
    Tile 0 holds 0 .. 511, then 1535, then 2048 and on; tile 1 begins at 1023
    and its rows hold 1023 / 1024, 1535 / 1536 and 2047 / 2048 on either side
    and on both; tile 2 is tile 1 with one id of chunk 0 in front.  Tile pair
    (0, 1) jumps 0 -> 512 -> 1024 (two jumps in a row), runs, jumps 1536 ->
    2048, runs; tile pair (0, 2) runs chunk 0 and jumps 512 -> 1024 with tile
    2's cursors already moved.  After those jumps cursor_at starts from a
    non-zero cursor and ends at an id equal to k0, behind an id equal to
    k0 - 1, and at k0 + 511 (asserted from the model in
    test_matrix_schedule.py and here)."""
    sk, lens = mc.scenario_b()
    s = mc.chunk_schedule(sk, lens)
    assert s.pairs[(0, 1)].kinds() == "jjrjr" and s.pairs[(0, 2)].kinds() == "rjrjr"
    for what in ("k0", "k0-1", "k0+511"):
        assert (what, 2048) in s.pairs[(0, 1)].landings() and (what, 1024) in s.pairs[(0, 2)].landings()
    check_dense(ctx128, sk, lens, None, b_dense, s, "scenario B")


def test_b_in_the_pair_and_the_grouped_form(ctx128, b_dense):
    """Scenario B's rows of tile 0 hold 72 ids before the first gap, more than
    one step of the scatter takes: the one scenario in which a cursor kept
    from before a jump loses entries, so it goes through the other two
    instantiations as well -- as pairs at a threshold that passes pairs of
    the tile pair (0, 1), and as a group behind another group."""
    sk, lens = mc.scenario_b()
    s = mc.chunk_schedule(sk, lens)
    ref = pairs_reference(sk, lens, F(0.8))
    assert 0 < len(ref) < 256 * 255 // 2 and any(r[0] < 64 <= r[1] < 128 for r in ref)
    check_pairs(ctx128, sk, lens, F(0.8), None, ref, s, "scenario B at 0.8")
    groups = [list(range(192, 256)), list(range(256))]
    first = tuple(x[192:, 192:] for x in b_dense)
    common, total, ani, cells, summary = ctx128.ani_matrix_groups(sk, lens, groups)
    assert cells.tolist() == [0, 64 * 64, 64 * 64 + 256 * 256]
    assert_dense_equal(tuple(x[:4096].reshape(64, 64) for x in (common, total, ani)), first, "scenario B, the filler group")
    assert_dense_equal(tuple(x[4096:].reshape(256, 256) for x in (common, total, ani)), b_dense, "scenario B as a group")
    assert summary["n_columns"] == 2 * mc.B_COLUMNS


# ---- scenario C: the grouped form -----------------------------------------------------------------
@pytest.fixture(scope="module")
def c_blocks(a_dense):
    sk, lens, groups = mc.scenario_c()
    return [a_dense if g == list(range(300)) else dense_reference(sk, lens, g) for g in groups]


@pytest.mark.parametrize("order", ("as listed", "reversed"))
def test_c_groups(ctx64, a_sched, c_blocks, order):
    """A group of more than 512 columns first (global ids far from local
    ones), scenario A as a group, a group of one, and a two-tile group over
    hashes that are columns of scenario A's group too."""
    sk, lens, groups = mc.scenario_c()
    scheds = mc.group_schedules(sk, lens, groups)
    assert scheds[0].n_columns > mc.CHUNK and scheds[1].events() == a_sched.events() and scheds[1].n_jumps() > 0
    blocks = c_blocks
    if order == "reversed":
        groups, scheds, blocks = groups[::-1], scheds[::-1], blocks[::-1]
    ref = tuple(np.concatenate([b[w].reshape(-1) for b in blocks]) for w in range(3))
    common, total, ani, cells, summary = ctx64.ani_matrix_groups(sk, lens, groups)
    assert cells.tolist() == np.concatenate([[0], np.cumsum([len(g) ** 2 for g in groups])]).tolist()
    for g, (lo, hi) in enumerate(zip(cells[:-1], cells[1:])):
        m = len(groups[g])
        assert_dense_equal(tuple(x[int(lo):int(hi)].reshape(m, m) for x in (common, total, ani)),
                           blocks[g], "scenario C %s, group %d of %d rows" % (order, g, m))
    assert common.tobytes() == ref[0].tobytes() and total.tobytes() == ref[1].tobytes() and ani.tobytes() == ref[2].tobytes()
    assert summary["n_columns"] == sum(s.n_columns for s in scheds)
    assert summary["column_entries"] == sum(s.column_entries for s in scheds)


# ---- scenario D: rows not in cluster order -----------------------------------------------------------
def test_d_shuffled_rows(ctx128):
    """200 rows of 40 clusters in a fixed permuted order: full tiles hold rows
    of nearly every cluster and run every chunk, the last tile of 8 rows jumps
    between the bands of its rows."""
    sk, lens, rows = mc.scenario_d()
    s = mc.chunk_schedule(sk, lens, rows)
    assert s.n_jumps() >= 1 and s.run_jump_run_events()
    check_dense(ctx128, sk, lens, rows, dense_reference(sk, lens, rows), s, "scenario D")
    ref = pairs_reference(sk, lens, F(0.98), rows)
    assert 0 < len(ref) < 200 * 199 // 2
    check_pairs(ctx128, sk, lens, F(0.98), rows, ref, s, "scenario D at 0.98")


# ---- the hashes 0 and 2^64 - 1 as columns ----------------------------------------------------------------
def test_extreme_hashes_dense_and_pairs(ctx64):
    sk, lens = mc.extreme_hash_rows()
    s = mc.chunk_schedule(sk, lens)
    ref = dense_reference(sk, lens)
    assert int(ref[0][2, 3]) == int(ref[0][2, 4]) == int(ref[0][3, 4]) == 1  # 2^64 - 1 alone
    assert int(ref[0][0, 6]) == int(ref[0][1, 6]) == 1 and int(ref[0][0, 1]) == 2  # 0 alone; 0 and 10
    check_dense(ctx64, sk, lens, None, ref, s, "extreme hashes")
    for thr in (0.0, 0.95):
        pref = pairs_reference(sk, lens, F(thr))
        assert (len(pref) == 28) == (thr == 0.0) and (2, 4, 1, 4) in pref and (0, 6, 1, 1) in pref
        check_pairs(ctx64, sk, lens, F(thr), None, pref, s, "extreme hashes at %s" % thr)


@pytest.mark.parametrize("which", (0, 1), ids=("holders together", "holders apart"))
def test_extreme_hashes_groups(ctx64, which):
    sk, lens = mc.extreme_hash_rows()
    groups = mc.EXTREME_GROUPS[which]
    scheds = mc.group_schedules(sk, lens, groups)
    ref = groups_reference(sk, lens, groups)
    common, total, ani, _, summary = ctx64.ani_matrix_groups(sk, lens, groups)
    assert_dense_equal((common, total, ani), ref, "extreme hashes, groups %d" % which)
    assert summary["n_columns"] == sum(s.n_columns for s in scheds)
    assert summary["column_entries"] == sum(s.column_entries for s in scheds)
    if which == 0:
        assert int(common[2 * 4 + 3]) == 1  # rows 2 and 3 share 2^64 - 1 only


# ---- mx_offsets_kernel past one wave of its scan -------------------------------------------------------------
def test_offsets_scan_past_one_wave():
    """2,100 positions: 66 of mx_offsets_kernel's threads hold lengths (32
    positions each), so the exclusive sum of the lengths crosses the first
    wave of the workgroup's scan; lengths from 0 to 16."""
    sk, lens = mc.offsets_rows()
    ref = pairs_reference(sk, lens, F(mc.OFFSETS_MIN_ANI))
    assert 0 < len(ref) < 2100 * 2099 // 2
    with ga.Context(k=21, sketch_size=16, seed=0) as ctx:
        pairs, summary = ctx.pairs_matrix(sk, lens, F(mc.OFFSETS_MIN_ANI))
    assert tuples(pairs) == ref
    assert summary["n_entries"] == int(lens.sum()) and summary["n_pairs"] == len(ref)
    assert (summary["n_columns"], summary["column_entries"]) == mc.dict_columns(sk, lens, range(2100))
