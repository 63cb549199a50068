"""The chunk loop of the matrix product on paper: which
chunks a tile pair runs and which it jumps over, from the numpy model of
matrix_cases.py.  CPU only.

mx_common_kernel walks the columns in chunks of 512 and jumps over every chunk
in which either row tile holds nothing.  The fixtures of test_ani_matrix_gpu.py,
test_ani_matrix_groups_gpu.py and test_pairs_matrix_gpu.py never make it jump
(the last tests of this file record that); test_matrix_jumps_gpu.py runs inputs
that do.  This file

  - keeps the model honest: for every scenario the common counts collected
    from the chunks the model says are run, and from those alone, equal
    finch's merge (ga.ani_pairs_host) over all cells, so the model jumps over
    nothing that is shared; the counts of columns equal a plain dict's (the
    host forms of the matrix report no column counts; the device's summary is
    compared with the model in the GPU file);
  - pins what each scenario must contain, condition by condition, so that an
    edit of a generator cannot silently take the jumps away.
"""
import numpy as np
import pytest

import galah_amd as ga
import matrix_cases as mc


def merge_common(sk, lens, rows):
    rows = [int(r) for r in rows]
    pairs, _ = ga.ani_pairs_host(sk, lens, [(a, b) for a in rows for b in rows])
    return pairs["common"].reshape(len(rows), len(rows)).astype(np.int64)


def assert_model_is_the_merge(sched, sk, lens):
    assert np.array_equal(sched.common(), merge_common(sk, lens, sched.rows))
    assert (sched.n_columns, sched.column_entries) == mc.dict_columns(sk, lens, sched.rows)
    for a, piece in enumerate(sched.pieces):
        assert (np.diff(piece) > 0).all() and len(piece) <= sched.lens[a]


# ---- scenario A: banded clusters, rows in cluster order --------------------------------
@pytest.fixture(scope="module")
def sched_a():
    sk, lens = mc.scenario_a()
    return mc.chunk_schedule(sk, lens)


def test_scenario_a_model_equals_the_merge(sched_a):
    sk, lens = mc.scenario_a()
    assert_model_is_the_merge(sched_a, sk, lens)
    listed = mc.chunk_schedule(sk, lens, mc.scenario_a_listed())
    assert_model_is_the_merge(listed, sk, lens)
    assert listed.n_jumps() > 0 and listed.rows[5] == listed.rows[200] and 5 // mc.TILE != 200 // mc.TILE


def test_scenario_a_conditions(sched_a):
    s = sched_a
    common = s.common()
    assert s.m == 300 and s.tiles == 5 and len(s.pairs) == 15 and s.n_columns > 5 * mc.CHUNK
    # 1. an off-diagonal tile pair begins with a jump from 0 and a cell's common comes only from chunks after it
    first = s.first_jump_then_shared()
    assert first, "no tile pair jumps from 0 and then finds a shared column"
    (ti, tj), (a, b) = first[0]
    assert ti < tj and s.pairs[(ti, tj)].events[0][:2] == ("jump", 0) and common[a, b] > 0
    # 2. run, a jump over two chunks or more, run: one cell collects common on both sides of the gap
    both = s.run_jump_run(min_chunks=2)
    assert both, "no cell collects common before and after a jump over two chunks"
    (ti, tj), (a, b) = both[0]
    p = s.pairs[(ti, tj)]
    cell = [(k0, int(c[a - ti * mc.TILE, b - tj * mc.TILE])) for k0, c in p.runs]
    wide = [e for e in p.jumps() if e[2] - e[1] >= 2 * mc.CHUNK]
    assert any(sum(v for k0, v in cell if k0 < e[1]) > 0 and sum(v for k0, v in cell if k0 >= e[2]) > 0 for e in wide)
    assert a != b and common[a, b] == sum(v for _, v in cell)
    # 3. an off-diagonal tile pair jumps and runs nothing: every cell of it holds common 0
    none = s.jump_without_run()
    assert none, "no tile pair jumps without running a chunk"
    for ti, tj in none:
        assert ti < tj and not common[ti * 64:ti * 64 + 64, tj * 64:tj * 64 + 64].any()
    # 4. a diagonal tile jumps (over columns held only inside other tiles)
    assert s.diagonal_with_jump(), "no diagonal tile pair jumps"
    # 5. a tile pair ends with one tile exhausted while the other holds 512 ids or more
    assert s.ends_with_ids_left(mc.CHUNK), "no tile pair ends with 512 ids left in one tile"
    # 6. the last tile is not full
    assert s.last_tile_not_full() and s.m % mc.TILE == 44
    # and jumps are what this input is mostly about
    jumps = [e for p in s.pairs.values() for e in p.jumps()]
    assert len(jumps) >= len(s.pairs) and any(e[1] == 0 for e in jumps) and any(e[2] - e[1] >= 1024 for e in jumps)


# ---- scenario B: boundary ids after a jump ---------------------------------------------------
def test_scenario_b_layout():
    """The layout of matrix_cases.scenario_b as the model sees it."""
    sk, lens = mc.scenario_b()
    s = mc.chunk_schedule(sk, lens)
    assert_model_is_the_merge(s, sk, lens)
    assert s.n_columns == mc.B_COLUMNS and s.m == 256
    # a column's id is its number: every piece is the row's hashes mapped back
    for a, piece in enumerate(s.pieces):
        assert np.array_equal(piece, (sk[a, :lens[a]].astype(np.int64) - 1000) // 7)
    tile = [np.unique(np.concatenate(s.pieces[64 * t:64 * t + 64])) for t in range(4)]
    assert np.array_equal(tile[0][:512], np.arange(512)) and tile[0][512] == 1535 and tile[0][513] == 2048
    assert tile[1][0] == 1023 and tile[2][0] == 0 and len(tile[3]) == mc.B_COLUMNS
    for edge in (1023, 1024, 1535, 1536, 2047, 2048):  # in tile 1, with and without the neighbour on the other side
        assert edge in tile[1]
    held = [set(p.tolist()) for p in s.pieces[64:128]]
    for lo in (1023, 1535, 2047):
        assert any(lo in h and lo + 1 in h for h in held) and any(lo in h and lo + 1 not in h for h in held)
        assert any(lo not in h and lo + 1 in h for h in held)
    p01, p02 = s.pairs[(0, 1)], s.pairs[(0, 2)]
    assert p01.events == [("jump", 0, 512), ("jump", 512, 1024), ("run", 1024), ("jump", 1536, 2048), ("run", 2048)]
    assert p02.events == [("run", 0), ("jump", 512, 1024), ("run", 1024), ("jump", 1536, 2048), ("run", 2048)]
    # the cursors found after a jump from a cursor that had moved: at k0, past k0 - 1, at k0 + 511
    for what in ("k0", "k0-1", "k0+511"):
        assert (what, 2048) in p01.landings(), what
        assert (what, 1024) in p02.landings() and (what, 2048) in p02.landings(), what


# ---- scenario C: the grouped form ---------------------------------------------------------------
def test_scenario_c_groups(sched_a):
    sk, lens, groups = mc.scenario_c()
    scheds = mc.group_schedules(sk, lens, groups)
    for g, s in zip(groups, scheds):
        assert_model_is_the_merge(s, sk, lens)
    # the host form of the groups is the merge per group too
    common = ga.ani_matrix_groups_host(sk, lens, groups)[0]
    assert np.array_equal(common, np.concatenate([s.common().reshape(-1) for s in scheds]))
    assert [s.m for s in scheds] == [28, 300, 1, 100]
    assert scheds[0].n_columns > mc.CHUNK and scheds[0].tiles == 1  # the ids of every later group are large
    # group 1 is scenario A with ids local to the group: the same events, so conditions 1 - 5 hold
    assert scheds[1].events() == sched_a.events() and scheds[1].tiles >= 3
    s = scheds[1]
    assert s.first_jump_then_shared() and s.run_jump_run(2) and s.jump_without_run() and s.diagonal_with_jump()
    assert s.ends_with_ids_left(mc.CHUNK)
    assert not scheds[2].pairs
    # the same hash is a column of group 1 and of group 3
    assert scheds[3].tiles == 2
    in1 = np.unique(np.concatenate([sk[r, :lens[r]] for r in groups[1]]))
    held = np.concatenate([sk[r, :lens[r]] for r in groups[3]])
    u, cnt = np.unique(held, return_counts=True)
    assert np.isin(u[cnt >= 2], in1).sum() > mc.CHUNK
    # the columns of the call are the groups' columns added up
    assert sum(s.n_columns for s in scheds) == sum(mc.dict_columns(sk, lens, g)[0] for g in groups)


# ---- scenario D: rows not in cluster order ---------------------------------------------------------
def test_scenario_d_shuffled():
    sk, lens, rows = mc.scenario_d()
    s = mc.chunk_schedule(sk, lens, rows)
    assert_model_is_the_merge(s, sk, lens)
    assert sorted(rows) == list(range(200)) and rows != sorted(rows)
    assert s.n_jumps() >= 1, "the shuffled rows no longer jump"
    assert s.run_jump_run_events(), "no tile pair runs, jumps and runs again"
    assert s.last_tile_not_full()


# ---- the small edges of the prologue ------------------------------------------------------------------
def test_extreme_hashes_are_columns():
    sk, lens = mc.extreme_hash_rows()
    assert (lens < 64).all() and lens[5] == 0
    s = mc.chunk_schedule(sk, lens)
    assert_model_is_the_merge(s, sk, lens)
    column_hashes = sorted(h for h in set(sk[0, :4].tolist()) | {mc.H_MAX} if sum(
        h in sk[r, :lens[r]].tolist() for r in range(len(lens))) >= 2)
    assert column_hashes[0] == 0 and column_hashes[-1] == mc.H_MAX and s.n_columns == len(column_hashes)
    assert sk[2, lens[2] - 1] == mc.H_MAX and len(s.pieces[2]) == 1  # ends in it and holds no other column
    assert lens[4] == 1 and sk[4, 0] == mc.H_MAX
    last = s.n_columns - 1
    assert [a for a, p in enumerate(s.pieces) if last in p] == [2, 3, 4]
    assert [a for a, p in enumerate(s.pieces) if 0 in p] == [0, 1, 6]
    same, apart = (mc.group_schedules(sk, lens, g) for g in mc.EXTREME_GROUPS)
    for sg in same + apart:
        assert_model_is_the_merge(sg, sk, lens)
    # rows 2 and 3 in one group: 2^64 - 1 is that group's last column; its holders apart: a column of no group
    assert len(same[0].pieces[2]) == 1 and same[0].pieces[2][0] == same[0].n_columns - 1
    for g, sg in zip(mc.EXTREME_GROUPS[1], apart):
        assert sum(r in (2, 3, 4) for r in g) <= 1 and all(len(sg.pieces[g.index(r)]) == 0 for r in (2, 4) if r in g)


def test_offsets_rows():
    sk, lens = mc.offsets_rows()
    assert len(lens) == 2100 and -(-2100 // 32) == 66 > 64  # positions in 66 threads: past one wave of the scan
    assert lens.min() == 0 and lens.max() == 16 and len(set(lens.tolist())) == 17
    for r in range(0, 2100, 7):
        assert (np.diff(sk[r, :lens[r]].astype(np.int64)) > 0).all()
    ref = ga.pairs_border_host(sk, lens, 0, float(np.float32(mc.OFFSETS_MIN_ANI)))
    assert 0 < len(ref) < 2100 * 2099 // 2


# ---- the fixtures of the three GPU files, rebuilt with their seeds: none of them jumps -----------------
def rows_from_sets(sets, s):
    sk = np.zeros((len(sets), s), np.uint64)
    lens = np.zeros(len(sets), np.uint32)
    for g, h in enumerate(sets):
        v = np.unique(np.asarray(list(h), dtype=np.uint64))
        sk[g, :len(v)] = v
        lens[g] = len(v)
    return sk, lens


def graded():
    """test_pairs_matrix_gpu.py's graded set."""
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


def dense_rows():
    """test_ani_matrix_gpu.py's dense group."""
    rng = np.random.default_rng(6)
    pool = np.unique(rng.integers(1, 2 ** 62, 1200, dtype=np.uint64))[:1100]
    sk = np.stack([np.sort(rng.choice(pool, 1000, replace=False)) for _ in range(200)])
    return sk, np.full(200, 1000, np.uint32)


def edge_set():
    """test_ani_matrix_gpu.py's edge set (test_ani_matrix_groups_gpu.py's is the same), and its row order."""
    rng = np.random.default_rng(20261020)
    everywhere = 5
    pools = [np.arange(100 + 1000 * p, 100 + 1000 * p + 90, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
             for p in range(4)]
    sets = []
    for g in range(150):
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
    sets[140] = {everywhere, 7} | set(range(10 ** 6, 10 ** 6 + 20))
    sets[141] = {everywhere, 7} | set(range(2 * 10 ** 6, 2 * 10 ** 6 + 30))
    sk, lens = rows_from_sets(sets, 64)
    order = rng.permutation(150)
    order = order[(order != 140) & (order != 141)]
    return sk, lens, order


def edge_rows(order, m):
    rows = [int(r) for r in order[:m]]
    rows[0], rows[-1] = 140, 141
    rows[m // 2] = rows[1]
    rows[2], rows[m - 2] = 3, 4
    rows[3], rows[4], rows[5] = 0, 1, 2
    return rows


def existing_fixture(name):
    """-> (sk, lens, rows, tile pairs)"""
    if name == "graded":
        return graded() + (None, 6)
    if name == "dense_rows":
        return dense_rows() + (None, 10)
    sk, lens, order = edge_set()
    if name == "edge set, all rows":
        return sk, lens, None, 6
    m = int(name.split("=")[1])
    return sk, lens, edge_rows(order, m), -(-m // 64) * (-(-m // 64) + 1) // 2


@pytest.mark.parametrize("name", ("graded", "dense_rows", "edge set, all rows", "edge set, m = 130", "edge set, m = 65"))
def test_existing_fixtures_never_jump(name):
    """Why test_matrix_jumps_gpu.py exists: the earlier fixtures take the
    `kc != k0` branch of the chunk loop in no tile pair."""
    sk, lens, rows, tile_pairs = existing_fixture(name)
    s = mc.chunk_schedule(sk, lens, rows)
    assert len(s.pairs) == tile_pairs and s.n_columns > 0
    assert s.n_jumps() == 0, name
    assert all(e[0] == "run" for p in s.pairs.values() for e in p.events)


def test_golden_sketches_never_jump(golden):
    s = mc.chunk_schedule(golden["sketches"], golden["lens"])
    assert len(s.pairs) == 1 and s.n_jumps() == 0
